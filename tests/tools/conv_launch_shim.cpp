// TEST INFRASTRUCTURE: plain-int doors to the launch decisions of csrc/conv_launch.hpp for tests/test_conv_launch_cpu.py
// (c++ -O1 -shared -fPIC, no offload: the header is host code).  Returns 0 and the decision's fields, or MOPOE_ERR_ARG and the
// message the library would hand to mopoe_last_error().
#include <string.h>

#include "../../mopoe-mimic_amd/csrc/conv_launch.hpp"

using namespace mopoe;

static mopoe_conv_geom geom(const int* v) {   // N, Hs, Ws, Hb, Wb, Cin, Cout, kh, kw, sh, sw, ph, pw, transposed
  mopoe_conv_geom g;
  g.N = v[0]; g.Hs = v[1]; g.Ws = v[2]; g.Hb = v[3]; g.Wb = v[4]; g.Cin = v[5]; g.Cout = v[6];
  g.kh = v[7]; g.kw = v[8]; g.sh = v[9]; g.sw = v[10]; g.ph = v[11]; g.pw = v[12]; g.transposed = v[13];
  return g;
}

extern "C" long long shim_ws_counter_bytes(void) { return (long long)WS_COUNTER_BYTES; }
extern "C" long long shim_ws_recommended(void) { return (long long)WS_RECOMMENDED; }

// row i of a family's tile table (non-zero past its end) -> kernel, id, bm, bn, threads, bk, stages, bn_form, in_kernel, kind, kind_bn
extern "C" int shim_gather_tile(int family, int i, int* out) {
  if (i < 0 || i >= (family ? BF16_NTILES : F32_NTILES)) return 1;
  const GatherTile& t = (family ? BF16_GATHER_TILES : F32_GATHER_TILES)[i];
  const int r[11] = {t.kernel, t.id, t.bm, t.bn, t.threads(), t.bk, t.stages, t.bn_form, t.in_kernel, t.kind, t.kind_bn};
  memcpy(out, r, sizeof r);
  return 0;
}

// ... of its weight-gradient table -> route, id, T, kp, kind
extern "C" int shim_wgrad_tile(int family, int i, int* out) {
  const int n = (int)(family ? sizeof(BF16_WGRAD_TILES) : sizeof(F32_WGRAD_TILES)) / (int)sizeof(WgradTile);
  if (i < 0 || i >= n) return 1;
  const WgradTile& t = (family ? BF16_WGRAD_TILES : F32_WGRAD_TILES)[i];
  const int r[5] = {t.route, t.id, t.T, t.kp, t.kind};
  memcpy(out, r, sizeof r);
  return 0;
}

// in: dest_on_small, Ck, Cn, w_nk, bn_on_load, mask kind, relu_bn mode, mix, out_f32, aligned, plan tile, plan split,
//     !MOPOE_NO_XCD_REMAP, !MOPOE_BF16_NO_GLDS (every tensor the flags call for is present, its BatchNorm has the right C)
// out: vec, tile, emu, spec, nsplit, reduce, gx, nNt, nphase, bm, bn, bk, rows_per_phase, rows_total, kind, slab offset
extern "C" int shim_gather(int family, const int* gv, const int* in, long long ws_bytes, long long* out, char* msg, int msg_n) {
  const mopoe_conv_geom g = geom(gv);
  const bool al = in[9] != 0, mix = in[7] != 0, relu = in[6] != 0 || mix;
  const int Hy = in[0] ? g.Hs : g.Hb, Wy = in[0] ? g.Ws : g.Wb;
  GatherFacts f = {in[0], in[1], in[2], in[3], in[4] ? 1 : 0, in[1], relu ? (mix ? 1 : in[6]) : 0, in[2], relu,
                   in[5], in[5] != 0, in[5] == 1 ? Hy * Wy : 1, mix, mix, in[8] != 0,
                   al, al, al, al, al, al, in[10], in[11], ws_bytes > 0, (size_t)ws_bytes, in[12] != 0, in[13] != 0};
  GatherDecision d;
  memset(&d, 0, sizeof d);
  if (int rc = decide_gather((ConvFamily)family, &g, f, d, msg, (size_t)msg_n)) return rc;
  const long long r[16] = {d.vec, d.tile, d.emu, d.spec, d.nsplit, d.reduce, d.gx, d.nNt, d.nphase, d.bm, d.bn, d.bk,
                           d.rows_per_phase, d.rows_total, d.kind, (long long)d.slab_offset};
  memcpy(out, r, sizeof r);
  return 0;
}

// in: bn_on_load, aligned, plan tile, plan split, !MOPOE_NO_XCD_REMAP, !MOPOE_BF16_NO_GLDS
// out: route, T, big, merge, vec, split, chunk, atomic, fast, spec, nI, nJ, gx, gy, gz, kind
extern "C" int shim_wgrad(int family, const int* gv, const int* in, long long* out, char* msg, int msg_n) {
  const mopoe_conv_geom g = geom(gv);
  WgradFacts f = {in[0] ? 1 : 0, g.Cin, in[1] != 0, in[1] != 0, in[2], in[3], in[4] != 0, in[5] != 0};
  WgradDecision d;
  memset(&d, 0, sizeof d);
  if (int rc = decide_wgrad((ConvFamily)family, &g, f, d, msg, (size_t)msg_n)) return rc;
  const long long r[16] = {d.route, d.T, d.big, d.merge, d.vec, d.split, d.chunk, d.atomic, d.fast, d.spec, d.nI, d.nJ,
                           d.gx, d.gy, d.gz, d.kind};
  memcpy(out, r, sizeof r);
  return 0;
}
