// Launch decisions of the implicit-GEMM convolution families (conv_gemm.hip: fp32, conv_gemm_bf16.hip: bf16 storage).
//
// Plain C++17 host code without a HIP type in it: the host compiler builds it alone, and tests/test_conv_launch_cpu.py
// holds it against the restatement in tests/plan_cases.py on a machine without a GPU.  It has
//   * the constants a decision depends on,
//   * ONE table per tile family with every fact of a tile written once -- the launchers' dispatch expands the same lists, so
//     a tile's template arguments and what the host assumes about it cannot drift apart,
//   * decide_gather / decide_wgrad: (geometry, fusion facts, alignment facts, plan, workspace size, A/B switches) -> what to
//     launch, or MOPOE_ERR_ARG with the message in a caller's buffer.  No device pointer, no getenv, no HIP call.
// The launchers fill the kernel argument struct from the decision, open the profiling scope, dispatch and check the launch.
#ifndef MOPOE_CONV_LAUNCH_HPP   // (guards rather than #pragma once: the header is also compiled alone)
#define MOPOE_CONV_LAUNCH_HPP
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <algorithm>

#include "../../include/mopoe_hip.h"

#ifndef TILE_N64_REMAINDER
#define TILE_N64_REMAINDER 64
#endif
#ifndef SPLIT_BLOCKS
#define SPLIT_BLOCKS 256   // grids below this many blocks split the tap x channel reduction
#endif
#ifndef SPLIT_TARGET
#define SPLIT_TARGET 512   // ... until about this many blocks are in flight
#endif
#ifndef PERSIST_BLOCKS
// upper bound on blocks of one launch (each block walks the M tiles it owns).  512 = exactly the 2 x 8-wave blocks a CU
// holds: fastest for a kernel that is alone on the chip, but inside the replayed step such a kernel keeps every CU for its
// whole duration and the other branches' small kernels wait.  With 2048 blocks retire 4x as often: C2 step +1...2 %
// (5250-5260 -> 5305-5370 samples/s; 4096: 5339, 16384: 5324); the bf16 family measured the other way and stays at 512.
#define PERSIST_BLOCKS 2048
#endif
#ifndef PERSIST_BLOCKS_BF16
#define PERSIST_BLOCKS_BF16 512
#endif

namespace mopoe {

constexpr int MAX_BN_C = 1024;
constexpr size_t WS_RECOMMENDED = 64u << 20;
// head of the conv workspace: one int arrival counter per output tile of a split reduction (zero between launches);
// the fp32 slabs of a split reduction follow it
constexpr size_t WS_COUNTER_BYTES = 64u << 10;
constexpr long WS_MAX_TILES = (long)(WS_COUNTER_BYTES / sizeof(int));
constexpr int BK = 16;    // fp32: K chunk of the register-staged wgrad kernel and of the 64x64 gather tile
constexpr int BKH = 32;   // bf16: K chunk in elements (two 16-deep MFMA steps); Ck % BKH == 0 is required

// ---- profiling kinds (api.hip) ----------------------------------------------------------------------
// one kind per kernel instantiation, so that the names bench.py reports are the names rocprofv3 prints:
//   gather, vector path:  tile * 4 + spec            (tile 0..7, spec 0..3)        kinds  0..31
//   gather, scalar path:  32 + {0: 128x128, 1: 256x64, 2: 64x64}                   kinds 32..34
//   wgrad,  vector path:  36 + (128x128 ? 0 : 3) + spec   (spec 0..2)              kinds 36..41
//   wgrad,  scalar path:  42 + (128x128 ? 0 : 1)                                   kinds 42..43
//   direct (LDS-free) gather: 44 + (tile - 8) * 4 + spec                           kinds 44..59
//   bf16 gather:          60 + tile * 3 + (spec - 1)     (tile 0..4, spec 1..3)    kinds 60..74
//   bf16 wgrad:           75 + (128x128 ? 0 : 2) + (BN+ReLU on x ? 1 : 0)          kinds 75..78
//   bf16 gather, LDS-DMA: 80 + (tile - 5) * 2 + (input gradient ? 1 : 0)           kinds 80..93
//   the same with BN + ReLU on the operand (tiles 5, 7, 9, 11): 94, 95, 96, 98
//   bf16 wgrad, LDS-DMA:  100 + (128x128 ? 0 : 2) + (BN+ReLU on x ? 1 : 0)         kinds 100..103
//   fp32 gather, LDS-DMA: 104 + (tile - 12) * 3 + (spec - 1)                       kinds 104..115
//   fp32 wgrad, LDS-DMA:  116 + (128x128 ? 0 : 2) + (BN+ReLU on x ? 1 : 0)         kinds 116..119
//   bf16 wgrad, two taps per block: 120 + (transposed conv ? 1 : 0); four taps per block: 122 + (S tile 128 ? 1 : 0)
//   (124..129: pointwise.hip, PROF_PW_FRONT in common.hpp)
//   fp32 gather, LDS-DMA, products on the bf16 pipe: 130 + (tile - 16) * 2 + (input gradient ? 1 : 0)   kinds 130..137
//   fp32 wgrad,  LDS-DMA, products on the bf16 pipe: 138 + (128x128 ? 0 : 1)       kinds 138..139
//   fp32 wgrad, four taps per block, products on the bf16 pipe (tile 9)            kinds 140..143: (S tile 128 ? 2 : 0) + (transposed conv ? 1 : 0)
// The tables below carry each tile's FIRST kind; kind_of_* adds the offset of the instantiation.
enum { PROF_GATHER_SCALAR = 32 };

enum ConvFamily { CONV_F32 = 0, CONV_BF16 = 1 };

// ---- gather tiles ------------------------------------------------------------------------------------------------------
// kernels (enumerators G_...): LDS_S / LDS = gather_gemm_kernel (register-staged through LDS; LDS_S also has a scalar-path form, four waves
// on the same block tile), DIRECT = direct_gemm_kernel (LDS-free), GLDS = gather_gemm_f32_glds_kernel (LDS-DMA), EMU = the same
// with the fp32 products on the bf16 matrix pipe, HREG = gather_gemm_bf16_kernel, HGLDS = gather_gemm_bf16_glds_kernel,
// HNONE = a number kept for a tile that is not built.
enum GatherKernel { G_LDS_S, G_LDS, G_DIRECT, G_GLDS, G_EMU, G_HREG, G_HGLDS, G_HNONE };
struct GatherTile {
  GatherKernel kernel;
  int id;
  int bm, bn;          // block rows x columns
  int wgm, wgn, wgk;   // wave grid (threads = 64 * wgm * wgn * wgk)
  int bk;              // K chunk (channels)
  int stages;          // LDS buffers
  int persist;         // resident-block cap of the persistent grid
  bool bn_form;        // a BN -> ReLU-on-load instantiation exists
  bool in_kernel;      // a split reduction finishes in the tile's last-arriving block (else: splitk_epilogue_kernel)
  int kind, kind_bn;   // first profiling kind; bf16 LDS-DMA: the kind of the BN-on-load form
  constexpr int threads() const { return 64 * wgm * wgn * wgk; }
};

// fp32 family, plan tiles 0..19.  Resident blocks: 8-wave blocks 2 per CU (PERSIST_BLOCKS), 4-wave blocks 3 per CU; the LDS-DMA
// tiles by their LDS footprint (1 or 2 per CU).  (17 and 18, whose 2 x 2 waves would each split fragments a neighbour splits
// too, partition K instead: 2 x 1 x 2 waves.  Same block, same stages, same epilogue layout.)
//   X(kernel, id, BM, BN, WGM, WGN, WGK, BK, LDS buffers, resident cap, BN form, in-kernel reduction, first kind)
#define MOPOE_F32_GATHER_TILES(X)                                                    \
  X(LDS_S,   0, 128, 128, 2, 4, 1, 16, 2, PERSIST_BLOCKS,         true,  true,    0) \
  X(LDS_S,   1, 256,  64, 4, 2, 1, 16, 2, PERSIST_BLOCKS,         true,  true,    4) \
  X(LDS_S,   2,  64,  64, 2, 2, 1, 16, 2, PERSIST_BLOCKS * 3 / 2, true,  true,    8) \
  X(LDS,     3, 256, 128, 4, 2, 1, 16, 2, PERSIST_BLOCKS,         true,  true,   12) \
  X(LDS,     4, 128,  64, 2, 2, 1, 16, 2, PERSIST_BLOCKS * 3 / 2, true,  true,   16) \
  X(LDS,     5,  64,  64, 2, 2, 1, 32, 2, PERSIST_BLOCKS * 3 / 2, true,  true,   20) \
  X(LDS,     6, 128,  64, 2, 2, 1, 32, 2, PERSIST_BLOCKS * 3 / 2, true,  true,   24) \
  X(LDS,     7, 128, 128, 2, 2, 1, 16, 2, PERSIST_BLOCKS * 3 / 2, true,  true,   28) \
  X(DIRECT,  8, 128, 128, 2, 2, 1,  8, 0, 4096,                   true,  false,  44) \
  X(DIRECT,  9, 256,  64, 4, 1, 1,  8, 0, 4096,                   true,  false,  48) \
  X(DIRECT, 10,  64,  64, 2, 2, 1,  8, 0, 4096,                   true,  false,  52) \
  X(DIRECT, 11, 128,  64, 2, 1, 1,  8, 0, 4096,                   true,  false,  56) \
  X(GLDS,   12, 128, 128, 2, 2, 1, 32, 2, 512,                    true,  true,  104) \
  X(GLDS,   13, 128,  64, 2, 2, 1, 32, 3, 512,                    false, true,  107) \
  X(GLDS,   14,  64,  64, 2, 2, 1, 32, 4, 512,                    true,  true,  110) \
  X(GLDS,   15, 256, 128, 4, 2, 1, 32, 2, 256,                    true,  true,  113) \
  X(EMU,    16, 128, 128, 2, 2, 1, 32, 2, 512,                    false, true,  130) \
  X(EMU,    17, 128,  64, 2, 1, 2, 32, 3, 512,                    false, true,  132) \
  X(EMU,    18,  64,  64, 2, 1, 2, 32, 4, 512,                    false, true,  134) \
  X(EMU,    19, 256, 128, 4, 2, 1, 32, 3, 256,                    false, true,  136)

// bf16 family, plan tiles 0..11.  Resident blocks: 8-wave tiles 2 per CU, 4-wave register-staged tiles 3 per CU; the LDS-DMA
// tiles by their LDS footprint (64 KB -> 2 per CU, 48 KB -> 3 per CU, 96 KB and more -> 1 per CU).  With BN on load: tiles 5,
// 7, 9 (two buffers) and 11 (four; the three-buffer forms exceed 256 registers).  8 = 256x128 with three buffers spills
// registers and is not built.
//   X(kernel, id, BM, BN, WGM, WGN, BK, LDS buffers, resident cap, BN form, first kind, kind of an LDS-DMA tile's BN form)
#define MOPOE_BF16_GATHER_TILES(X)                                              \
  X(HREG,   0, 128, 128, 2, 2, 32, 2, PERSIST_BLOCKS_BF16 * 3 / 2, true,  60,  0) \
  X(HREG,   1, 256,  64, 4, 1, 32, 2, PERSIST_BLOCKS_BF16 * 3 / 2, true,  63,  0) \
  X(HREG,   2,  64,  64, 2, 2, 32, 2, PERSIST_BLOCKS_BF16 * 3 / 2, true,  66,  0) \
  X(HREG,   3, 256, 128, 4, 2, 32, 2, PERSIST_BLOCKS_BF16,         true,  69,  0) \
  X(HREG,   4, 128,  64, 4, 1, 32, 2, PERSIST_BLOCKS_BF16 * 3 / 2, true,  72,  0) \
  X(HGLDS,  5, 128, 128, 2, 2, 64, 2, 512,                         true,  80, 94) \
  X(HGLDS,  6, 128, 128, 2, 2, 64, 3, 256,                         false, 82,  0) \
  X(HGLDS,  7, 256, 128, 4, 2, 64, 2, 256,                         true,  84, 95) \
  X(HNONE,  8, 256, 128, 4, 2, 64, 3, 256,                         false, 86,  0) \
  X(HGLDS,  9, 128,  64, 4, 1, 64, 2, 768,                         true,  88, 96) \
  X(HGLDS, 10, 128,  64, 4, 1, 64, 3, 512,                         false, 90,  0) \
  X(HGLDS, 11,  64,  64, 2, 2, 64, 4, 512,                         true,  92, 98)

#define MOPOE_TILE_ROW_F32(K_, ID_, BM_, BN_, WM_, WN_, WK_, BK_, ST_, P_, X_, R_, KIND_) {G_##K_, ID_, BM_, BN_, WM_, WN_, WK_, BK_, ST_, P_, X_, R_, KIND_, 0},
#define MOPOE_TILE_ROW_BF16(K_, ID_, BM_, BN_, WM_, WN_, BK_, ST_, P_, X_, KIND_, KINDX_) {G_##K_, ID_, BM_, BN_, WM_, WN_, 1, BK_, ST_, P_, X_, true, KIND_, KINDX_},
constexpr GatherTile F32_GATHER_TILES[] = {MOPOE_F32_GATHER_TILES(MOPOE_TILE_ROW_F32)};
constexpr GatherTile BF16_GATHER_TILES[] = {MOPOE_BF16_GATHER_TILES(MOPOE_TILE_ROW_BF16)};
#undef MOPOE_TILE_ROW_F32
#undef MOPOE_TILE_ROW_BF16
constexpr int F32_NTILES = (int)(sizeof(F32_GATHER_TILES) / sizeof(GatherTile));
constexpr int BF16_NTILES = (int)(sizeof(BF16_GATHER_TILES) / sizeof(GatherTile));
constexpr int F32_EMU_FIRST = 16, F32_EMU_SHIFT = 4;   // plan tiles 16..19 = tiles 12..15 with split-bf16 products

// ---- weight-gradient tiles ---------------------------------------------------------------------------------------------
// routes: W_REG = register-staged through LDS, W_GLDS = LDS-DMA, W_EMU = LDS-DMA with the fp32 products on the bf16 pipe,
// W_MERGE = LDS-DMA with two taps per block, W_FOUR = four taps (one parity class of a k4 s2 p1 kernel) per block.
enum WgradRoute { W_REG, W_GLDS, W_EMU, W_MERGE, W_FOUR };
struct WgradTile {
  WgradRoute route;
  int id;
  int T;               // channels per block side (W_FOUR: channels of the small-grid operand; the gathered side has 64)
  int kp;              // pixels per chunk (W_FOUR: per 8 x 8 tile)
  int stages, stages_bn;   // LDS buffers of the plain / BN-on-load form (0: not a template argument)
  int min_chunks;      // a block of a split pixel reduction keeps at least this many chunks
  int kind;            // first profiling kind
};
// every block has 256 threads
constexpr int WGRAD_THREADS = 256;
//   X(route, id, T, pixels per chunk, buffers, buffers with BN on load, least chunks per block, first kind)
// fp32 family: plan tiles -1, 0, 1 = 0 (2 where a side has <= 64 channels)
#define MOPOE_F32_WGRAD_TILES(X)        \
  X(W_REG,   0, 128, 16, 2, 2, 8,  36)  \
  X(W_REG,   2,  64, 16, 2, 2, 8,  39)  \
  X(W_GLDS,  5, 128, 32, 2, 2, 4, 116)  \
  X(W_GLDS,  6,  64, 32, 4, 2, 4, 118)  \
  X(W_EMU,   7, 128, 32, 2, 0, 4, 138)  \
  X(W_EMU,   8,  64, 32, 4, 0, 4, 139)  \
  X(W_FOUR,  9,  64, 64, 0, 0, 1, 140)  \
  X(W_FOUR, 10, 128, 64, 0, 0, 1, 142)
// bf16 family: no plan = 5 / 6 (MOPOE_BF16_NO_GLDS: 0 / 2); plan tiles 0, 1, 3, 4 = 0 (2 where a side has <= 64 channels)
#define MOPOE_BF16_WGRAD_TILES(X)       \
  X(W_REG,   0, 128, 32, 2, 2, 4,  75)  \
  X(W_REG,   2,  64, 32, 2, 2, 4,  77)  \
  X(W_GLDS,  5, 128, 64, 0, 0, 4, 100)  \
  X(W_GLDS,  6,  64, 64, 0, 0, 4, 102)  \
  X(W_MERGE, 7, 128, 64, 0, 0, 4, 120)  \
  X(W_FOUR,  8,  64, 64, 0, 0, 1, 122)  \
  X(W_FOUR,  9, 128, 64, 0, 0, 1, 123)
#define MOPOE_WTILE_ROW(R_, ID_, T_, KP_, ST_, STX_, MC_, KIND_) {R_, ID_, T_, KP_, ST_, STX_, MC_, KIND_},
constexpr WgradTile F32_WGRAD_TILES[] = {MOPOE_F32_WGRAD_TILES(MOPOE_WTILE_ROW)};
constexpr WgradTile BF16_WGRAD_TILES[] = {MOPOE_BF16_WGRAD_TILES(MOPOE_WTILE_ROW)};
#undef MOPOE_WTILE_ROW
constexpr int PROF_WGRAD_SCALAR = 42;   // fp32 scalar path: 42 (128x128), 43 (64x64)

inline const WgradTile* wgrad_tile(ConvFamily fam, int id) {
  const WgradTile* t = fam == CONV_F32 ? F32_WGRAD_TILES : BF16_WGRAD_TILES;
  const int n = fam == CONV_F32 ? (int)(sizeof(F32_WGRAD_TILES) / sizeof(WgradTile)) : (int)(sizeof(BF16_WGRAD_TILES) / sizeof(WgradTile));
  for (int i = 0; i < n; ++i)
    if (t[i].id == id) return t + i;
  return nullptr;
}

// ---- helpers shared by both families --------------------------------------------------------------------------------
inline long cdiv(long a, long b) { return (a + b - 1) / b; }

inline int refuse(char* msg, size_t n, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, n, fmt, ap);
  va_end(ap);
  return MOPOE_ERR_ARG;
}

inline int ilog2_exact(long v) {
  if (v <= 0 || (v & (v - 1))) return -1;
  int l = 0;
  while ((1L << l) < v) ++l;
  return l;
}

// what the caller knows about a gather launch beyond the geometry
struct GatherFacts {
  int dest_on_small;     // 1 -> form 0 (Y on the small grid), 0 -> form 1 (Y on the big grid)
  int Ck, Cn, w_nk;
  int bn_mode, bn_C;     // BN -> ReLU on load
  int relu_mode, relu_C; // relu_bn (input gradient) or, with a residual mix, the shortcut's BatchNorm
  bool xin;              // xin (or the mix's s) present
  int mask_kind;
  bool mask_ptr;
  int rows_per_sample;
  bool mix, mix_valid;   // residual mix asked for / has s and a BatchNorm (bf16: and a bf16 result)
  bool out_f32;          // bf16 family: fp32 result
  bool al_x, al_w, al_y, al_xin, al_mask, al_mix;   // 16-byte alignment (absent tensors: true)
  int plan_tile, plan_split;   // no plan: -1, 0
  bool ws;               // a workspace pointer was given
  size_t ws_bytes;
  bool xcd_remap, bf16_glds;   // A/B switches: !MOPOE_NO_XCD_REMAP, !MOPOE_BF16_NO_GLDS
};

enum SplitReduce { REDUCE_NONE = 0, REDUCE_IN_KERNEL = 1, REDUCE_EPILOGUE = 2 };

struct GatherDecision {
  bool vec;              // fp32: vector path (bf16: always)
  int tile;              // after the fall-backs (fp32 split-bf16 forms: 12..15 with emu set)
  bool emu;
  const GatherTile* t;   // the tile's table row
  int spec;              // 0 run-time flags | 1 forward, plain operand | 2 forward, BN+ReLU on the operand | 3 input gradient
  int nsplit;
  SplitReduce reduce;
  size_t slab_offset;    // byte offset of the slabs in the workspace (the counters sit at 0)
  long gx;
  int nNt, nphase;
  int bm, bn, bk;
  int form, Hx, Wx, Hy, Wy, Hq, Wq;
  long rows_per_phase, rows_total;
  bool vecA, vecB;
  unsigned x_bytes, w_bytes;
  int xcd_remap;
  double flops, bytes;
  int kind;
};

// form 0 ("gather from the big grid"): Y on the conv's small grid, X on the big grid.  form 1 ("sub-pixel phases"): Y on
// the big grid, X on the small grid, one phase (oy % sh, ox % sw) at a time.
inline void gather_geometry(const mopoe_conv_geom* g, int dest_on_small, GatherDecision& d) {
  if (dest_on_small) {
    d.form = 0; d.Hx = g->Hb; d.Wx = g->Wb; d.Hy = g->Hs; d.Wy = g->Ws; d.Hq = g->Hs; d.Wq = g->Ws; d.nphase = 1;
  } else {
    d.form = 1; d.Hx = g->Hs; d.Wx = g->Ws; d.Hy = g->Hb; d.Wy = g->Wb; d.Hq = g->Hb / g->sh; d.Wq = g->Wb / g->sw;
    d.nphase = g->sh * g->sw;
  }
  d.rows_per_phase = (long)g->N * d.Hq * d.Wq;
  d.rows_total = (long)g->N * d.Hy * d.Wy;
}

inline int gather_checks(const mopoe_conv_geom* g, const GatherFacts& f, const GatherDecision& d, char* msg, size_t n) {
  if (f.bn_mode != 0 && (f.bn_C != f.Ck || f.Ck > MAX_BN_C)) return refuse(msg, n, "bn_in channel mismatch (%d vs %d)", f.bn_C, f.Ck);
  if (f.relu_mode != 0 && (f.relu_C != f.Cn || !f.xin)) return refuse(msg, n, "relu_bn needs xin and C == %d", f.Cn);
  if (f.mask_kind != 0 && !f.mask_ptr) return refuse(msg, n, "mask pointer missing");
  if (f.mask_kind == 1 && f.rows_per_sample != d.Hy * d.Wy) return refuse(msg, n, "channel mask: rows_per_sample must be Hout*Wout");
  if (d.rows_total >= (1L << 31) || (long)g->N * d.Hx * d.Wx >= (1L << 31)) return refuse(msg, n, "conv: more than 2^31 rows");
  return MOPOE_OK;
}

// split-K for grids that cannot fill the chip -> the number of blocks sharing one tile's reduction (1 = none), or 0 where the
// plan's split does not fit the slabs.  `per`: bytes of one fp32 slab; `kw`: channels an iteration stands for in the policy.
inline long split_k(int plan_split, int iters, long blocks, size_t per, bool can_split, size_t slab_bytes, int below, int target, int kw) {
  long ns = 1;
  if (plan_split > 0) {
    ns = std::min<long>(plan_split, iters);
    if (ns >= 2 && (!can_split || (size_t)ns * per > slab_bytes)) return 0;
  } else if (can_split && blocks < below && (long)iters * kw >= 256) {
    ns = std::min<long>((target + blocks - 1) / blocks, (long)iters * kw / 128);
    if ((size_t)ns * per > slab_bytes) ns = (long)(slab_bytes / per);
  }
  return std::max<long>(ns, 1);
}

// persistent M loop: at most `persist` blocks in flight, column statistics leave a block once
inline long persistent_gx(long nMt, long persist, int nNt, int nphase, int nsplit) {
  return std::min<long>(nMt, std::max<long>(1, persist / ((long)nNt * nphase * nsplit)));
}

inline int kind_of_gather(const GatherTile& t, bool vec, int spec) {
  switch (t.kernel) {
    case G_LDS_S: case G_LDS: return vec ? t.kind + spec : PROF_GATHER_SCALAR + t.id;
    case G_DIRECT: return t.kind + spec;
    case G_GLDS: case G_HREG: return t.kind + (spec - 1);
    case G_EMU: return t.kind + (spec == 3 ? 1 : 0);
    default: return spec == 2 ? t.kind_bn : t.kind + (spec == 3 ? 1 : 0);
  }
}

inline int decide_gather(ConvFamily fam, const mopoe_conv_geom* g, const GatherFacts& f, GatherDecision& d, char* msg, size_t n) {
  const int Ck = f.Ck, Cn = f.Cn;
  const bool h = fam == CONV_BF16, bn_on_load = f.bn_mode != 0;
  const size_t esz = h ? 2 : 4;
  gather_geometry(g, f.dest_on_small, d);
  const size_t xb = (size_t)g->N * d.Hx * d.Wx * Ck * esz;
  const size_t wb = (size_t)g->kh * g->kw * g->Cin * g->Cout * esz;
  d.emu = false;
  d.xcd_remap = f.xcd_remap ? 1 : 0;
  d.vecA = (Ck % 4 == 0) && f.al_x;
  d.vecB = (g->Cout % 4 == 0) && f.al_w;
  if (h) {
    if (Ck % BKH != 0 || Cn % 8 != 0 || g->Cout % 8 != 0)
      return refuse(msg, n, "bf16 conv: K channels must be a multiple of 32 and N channels of 8 (Ck = %d, Cn = %d)", Ck, Cn);
    if (!f.al_x || !f.al_w || !f.al_y || !f.al_xin || xb >= (1ull << 31) || wb >= (1ull << 31))
      return refuse(msg, n, "bf16 conv: tensors must be 16-byte aligned and smaller than 2 GiB");
    d.vec = true;
    if (f.mix && (!f.mix_valid || f.out_f32 || !f.al_mix)) return refuse(msg, n, "conv_fwd_mix_bf16: needs an aligned bf16 s, its BatchNorm and a bf16 result");
  } else {
    // branch-free buffer loads need 16-byte alignment, channel counts that are multiples of 4 and < 2 GiB operands
    // (the vector path's row-major epilogue moves the result, xin and the mask in float4 pieces: Cn % 4 == 0, aligned rows)
    d.vec = d.vecA && d.vecB && xb < (1ull << 31) && wb < (1ull << 31) && Cn % 4 == 0 && f.al_y && f.al_xin && (f.mask_kind == 0 || f.al_mask);
    // residual mix in the epilogue: the shortcut's BN rides in relu_bn, its tensor in xin (vector path only)
    if (f.mix && !f.mix_valid) return refuse(msg, n, "conv_fwd_mix: needs s and its BatchNorm");
    if (f.mix && (!d.vec || !f.al_mix)) return refuse(msg, n, "conv_fwd_mix: channel counts must be multiples of 4 and tensors 16-byte aligned");
  }
  d.x_bytes = (unsigned)std::min<size_t>(xb, 0x7fffffffu);
  d.w_bytes = (unsigned)std::min<size_t>(wb, 0x7fffffffu);
  if (int rc = gather_checks(g, f, d, msg, n)) return rc;

  // ---- tile choice -------------------------------------------------------------------------------------------
  // Wide outputs take the 128x128 tile (best operand reuse); when that leaves the chip under-filled the tap x channel
  // reduction is split across blocks instead of shrinking the tile.
  int cfg;
  if (h) {
    if (Cn > 64) cfg = d.rows_per_phase >= 256L * 128 ? 3 : (d.rows_per_phase > 64 ? 0 : 2);
    else cfg = d.rows_per_phase >= 256L * 64 ? 1 : 2;
    const bool glds_ok = Ck % 64 == 0;
    if (glds_ok && f.bf16_glds) cfg = cfg == 0 ? 5 : (cfg == 3 ? 7 : (cfg == 4 ? 9 : cfg));
    if (f.plan_tile >= 0) {
      if (f.plan_tile >= BF16_NTILES) return refuse(msg, n, "bf16 conv plan: tile %d (0..%d)", f.plan_tile, BF16_NTILES - 1);
      const GatherTile& p = BF16_GATHER_TILES[f.plan_tile];
      // (never offered by the tuner, no longer reachable through a plan)
      if (p.kernel == G_HNONE) return refuse(msg, n, "bf16 conv plan: tile 8 (256x128, three LDS buffers) is not built: it spills registers; use 7");
      if (p.kernel == G_HGLDS && (!glds_ok || (bn_on_load && !p.bn_form)))
        return refuse(msg, n, "bf16 conv plan: tile %d (LDS-DMA family) needs K channels %% 64 == 0 (Ck = %d) and, with BN on load, one of the tiles 5, 7, 9, 11", f.plan_tile, Ck);
      cfg = f.plan_tile;
    }
  } else {
    if (Cn > 64) cfg = (d.rows_per_phase > 64 || Cn >= 256) ? 0 : 2;
    else cfg = d.rows_per_phase >= 256L * 64 ? 1 : 2;
    // a 128-wide tile would be half empty for the last 64 columns (Cout = 192, 320): use 64-wide tiles instead
    if (cfg == 0 && (Cn % 128) == 64 && d.rows_per_phase >= 256L * TILE_N64_REMAINDER) cfg = 1;
    if (f.plan_tile >= 0) {
      if (f.plan_tile >= F32_NTILES) return refuse(msg, n, "conv plan: tile %d (see mopoe_conv_plan in mopoe_hip.h: 0..19)", f.plan_tile);
      cfg = f.plan_tile;
      if (cfg >= F32_EMU_FIRST) {
        if (bn_on_load) return refuse(msg, n, "conv plan: tile %d (split-bf16 products) has no BN-on-load form", cfg);
        d.emu = true;
        cfg -= F32_EMU_SHIFT;
      }
      // LDS-DMA family: vector path, K channels a multiple of 32.  A plan that asks for one where it does not apply is refused
      // (the tuner never offers it).
      if (F32_GATHER_TILES[cfg].kernel == G_GLDS && (!d.vec || Ck % 32 != 0 || (bn_on_load && !F32_GATHER_TILES[cfg].bn_form)))
        return refuse(msg, n, "conv plan: tile %d (LDS-DMA family) needs the vector path, K channels %% 32 == 0 (Ck = %d) and, with BN on load, tile 12, 14 or 15", cfg, Ck);
      if (cfg >= 3 && !d.vec) cfg = cfg == 3 ? 0 : 2;   // the extra tiles exist for the vector path only
      if ((cfg == 5 || cfg == 6) && Ck % 32 != 0) cfg -= 3;   // 5, 6 = tiles 2, 4 with a 32-deep K chunk
      if (F32_GATHER_TILES[cfg].kernel == G_DIRECT && (!d.vec || Ck % 8 != 0 || f.mix)) cfg = (cfg == 8) ? 0 : (cfg == 9 ? 1 : (cfg == 10 ? 2 : 4));   // LDS-free kernels (no residual mix)
    }
  }
  const GatherTile& t = h ? BF16_GATHER_TILES[cfg] : F32_GATHER_TILES[cfg + (d.emu ? F32_EMU_SHIFT : 0)];
  d.tile = cfg; d.t = &t; d.bm = t.bm; d.bn = t.bn; d.bk = t.bk;
  const long nMt = cdiv(d.rows_per_phase, t.bm);
  d.nNt = (int)cdiv(Cn, t.bn);
  const int nkc = (int)cdiv(Ck, t.bk);    // K chunks per tap
  const int iters = (f.dest_on_small ? g->kh * g->kw : std::max(1, (g->kh / g->sh) * (g->kw / g->sw))) * nkc;
  const long blocks = nMt * d.nNt * d.nphase;
  const size_t per = (size_t)d.rows_total * Cn * sizeof(float);
  // workspace = [arrival counters: WS_COUNTER_BYTES, zero between launches][fp32 slabs]
  const bool have_ws = f.ws && f.ws_bytes > WS_COUNTER_BYTES;
  const bool can_split = have_ws && (!h || blocks <= WS_MAX_TILES);
  const size_t slab_bytes = can_split ? f.ws_bytes - WS_COUNTER_BYTES : 0;
  const long ns = h ? split_k(f.plan_split, iters, blocks, per, can_split, slab_bytes, 256, 512, BKH)
                    : split_k(f.plan_split, iters, blocks, per, can_split, slab_bytes, SPLIT_BLOCKS, SPLIT_TARGET, t.bk);
  if (ns == 0) {
    const long want = std::min<long>(f.plan_split, iters);
    if (h) return refuse(msg, n, "bf16 conv plan: split %ld needs %zu workspace bytes (have %zu) and at most %zu output tiles (have %ld)", want,
                         (size_t)want * per + WS_COUNTER_BYTES, f.ws ? f.ws_bytes : (size_t)0, WS_COUNTER_BYTES / sizeof(int), blocks);
    return refuse(msg, n, "conv plan: split %ld needs %zu workspace bytes (have %zu)", want, (size_t)want * per, slab_bytes);
  }
  d.nsplit = (int)ns;
  d.slab_offset = WS_COUNTER_BYTES;
  // vector path, LDS kernels: the reduction finishes in the tile's last-arriving block (gemm_epilogue_rows.inc); the
  // scalar path and the LDS-free kernels park raw slabs for splitk_epilogue_kernel
  d.reduce = ns < 2 ? REDUCE_NONE : (d.vec && t.in_kernel ? REDUCE_IN_KERNEL : REDUCE_EPILOGUE);
  if (d.reduce == REDUCE_IN_KERNEL && blocks > WS_MAX_TILES)
    return refuse(msg, n, "conv: split reduction over %ld output tiles (at most %zu)", blocks, WS_COUNTER_BYTES / sizeof(int));
  d.gx = persistent_gx(nMt, t.persist, d.nNt, d.nphase, d.nsplit);
  // specialised main loops (spec != 0): vector path with Ck a multiple of the K chunk (every layer of the four networks
  // except the image-side edge layers, which do not come here, and the vocabulary projection's input gradient)
  d.spec = (d.vec && Ck % t.bk == 0) ? (f.w_nk ? 3 : (bn_on_load ? 2 : 1)) : 0;
  // algorithmic flops: every (output pixel, tap that exists) pair; bytes: one read of the gathered activation +
  // one write of the result
  const double taps_eff = f.dest_on_small ? (double)g->kh * g->kw : (double)g->kh * g->kw / ((double)g->sh * g->sw);
  d.flops = 2.0 * (double)g->N * d.Hy * d.Wy * (double)Cn * (double)Ck * taps_eff;
  d.bytes = h ? (double)xb + (double)d.rows_total * Cn * (f.out_f32 ? 4.0 : 2.0)
              : ((double)g->N * d.Hx * d.Wx * Ck + (double)d.rows_total * Cn) * sizeof(float);
  d.kind = kind_of_gather(t, d.vec, d.spec);
  return MOPOE_OK;
}

// ---- weight gradients ------------------------------------------------------------------------------------------------
struct WgradFacts {
  int bn_mode, bn_C;
  bool al_x, al_dy;
  int plan_tile, plan_split;   // no plan: -1, 0
  bool xcd_remap, bf16_glds;
};

struct WgradDecision {
  const WgradTile* t;    // the tile's table row
  WgradRoute route;
  bool vec;              // fp32: vector path (bf16: always)
  int T;                 // block side in channels (four-tap route: channels of the small-grid operand, "cs")
  bool big;              // T == 128
  int merge;             // two-tap route: 1 = conv with Cin = 64, 2 = transposed conv with Cout = 64
  bool bn_on_load;
  int fast;              // fp32: fast pixel addressing; bf16: small grid a power of two (pow2)
  int spec;              // fp32 register-staged vector path: 0 run-time flags | 1 plain operand | 2 BN+ReLU on x
  int lg_ws, lg_hw;      // bf16: log2 of Ws and Hs*Ws (-1: not a power of two)
  int x_is_big;
  long Ms;
  long split, chunk;
  int atomic;
  int vecI, vecJ;
  int nI, nJ;
  unsigned gx, gy, gz;
  unsigned x_bytes, dy_bytes;
  size_t dw_bytes;
  int xcd_remap;
  double flops, bytes;
  int kind;
};

inline bool four_tap_geometry(const mopoe_conv_geom* g) {
  return g->kh == 4 && g->kw == 4 && g->sh == 2 && g->sw == 2 && g->ph == 1 && g->pw == 1 &&
         g->Hs % 8 == 0 && g->Ws % 8 == 0 && g->Hb == 2 * g->Hs && g->Wb == 2 * g->Ws;
}

// split the pixel reduction over `split` blocks of whole chunks of kp pixels, at most max_split
inline void pixel_split(long Ms, long split, int kp, long max_split, WgradDecision& d) {
  if (split > max_split) split = max_split;
  if (split < 1) split = 1;
  long chunk = (Ms + split - 1) / split;
  chunk = (chunk + kp - 1) / kp * kp;
  d.chunk = chunk;
  d.split = (Ms + chunk - 1) / chunk;
  d.atomic = d.split > 1;
}

// four-tap route: the 8 x 8 tiles of the small grid split until about `target` blocks are in flight (chunk in tiles)
inline void four_tap_split(long ntiles, long cblocks, int plan_split, int target, WgradDecision& d) {
  long split = plan_split > 0 ? plan_split : (target + cblocks - 1) / cblocks;
  if (split > ntiles) split = ntiles;
  if (split < 1) split = 1;
  d.chunk = (ntiles + split - 1) / split;
  d.split = (ntiles + d.chunk - 1) / d.chunk;
  d.atomic = d.split > 1;
}

inline int decide_wgrad(ConvFamily fam, const mopoe_conv_geom* g, const WgradFacts& f, WgradDecision& d, char* msg, size_t n) {
  const bool h = fam == CONV_BF16, xf = f.bn_mode != 0;
  const int tile = f.plan_tile, plan_split = f.plan_split;
  const size_t esz = h ? 2 : 4;
  d.x_is_big = g->transposed ? 0 : 1;
  d.Ms = (long)g->N * g->Hs * g->Ws;
  d.bn_on_load = xf;
  d.merge = 0;
  d.xcd_remap = f.xcd_remap ? 1 : 0;
  if (xf && (f.bn_C != g->Cin || g->Cin > MAX_BN_C)) return refuse(msg, n, "wgrad bn_in channel mismatch");
  if (h && (g->Cin % 8 != 0 || g->Cout % 8 != 0)) return refuse(msg, n, "bf16 wgrad: channel counts must be multiples of 8 (%d, %d)", g->Cin, g->Cout);
  const size_t rows_x = (size_t)g->N * (g->transposed ? g->Hs * g->Ws : g->Hb * g->Wb);
  const size_t rows_dy = (size_t)g->N * (g->transposed ? g->Hb * g->Wb : g->Hs * g->Ws);
  const size_t xb = rows_x * g->Cin * esz, db = rows_dy * g->Cout * esz;
  d.vecI = (g->Cin % 4 == 0) && f.al_x;
  d.vecJ = (g->Cout % 4 == 0) && f.al_dy;
  if (h) {
    if (!f.al_x || !f.al_dy || xb >= (1ull << 31) || db >= (1ull << 31)) return refuse(msg, n, "bf16 wgrad: tensors must be 16-byte aligned and smaller than 2 GiB");
    d.vec = true;
  } else {
    d.vec = d.vecI && d.vecJ && xb < (1ull << 31) && db < (1ull << 31);
    if (rows_x >= (1ull << 31) || rows_dy >= (1ull << 31)) return refuse(msg, n, "wgrad: more than 2^31 rows");
  }
  d.x_bytes = (unsigned)std::min<size_t>(xb, 0x7fffffffu);
  d.dy_bytes = (unsigned)std::min<size_t>(db, 0x7fffffffu);
  d.lg_ws = ilog2_exact(g->Ws);
  d.lg_hw = ilog2_exact((long)g->Hs * g->Ws);
  // fp32, fast pixel addressing: chunks of BK = 16 pixels never straddle an image row (or cover whole rows of one image);
  // bf16: the pixel -> (image, y, x) split is shifts and masks
  const int hw_s = g->Hs * g->Ws;
  d.fast = h ? (d.lg_ws >= 0 && d.lg_hw >= 0) : (d.vec && ((g->Ws % BK == 0) || (BK % g->Ws == 0 && hw_s % BK == 0)));
  d.spec = d.fast ? (xf ? 2 : 1) : 0;
  const int taps = g->kh * g->kw;
  d.dw_bytes = (size_t)taps * g->Cin * g->Cout * sizeof(float);
  d.flops = 2.0 * (double)d.Ms * g->Cin * (double)g->Cout * taps;
  d.bytes = h ? (double)xb + (double)db
              : ((double)g->N * g->Hs * g->Ws * (g->transposed ? g->Cin : g->Cout)
                 + (double)g->N * g->Hb * g->Wb * (g->transposed ? g->Cout : g->Cin)) * sizeof(float);   // both operands, once
  const bool big = g->Cin > 64 && g->Cout > 64;
  const WgradTile* p = wgrad_tile(fam, tile);    // the plan's tile, where it names one of the table's
  // (mirrors the tuner, mimic_amd/ops.py: _wgrad_candidates -- the 128 tile on LDS-DMA is never offered with <= 64 channels on a
  // side: it would run half-empty MFMA tiles)
  const bool needs_big = p && p->T == 128 && (p->route == W_GLDS || p->route == W_EMU);

  if (h && needs_big && !big) return refuse(msg, n, "bf16 wgrad plan: tile 5 (128x128 on LDS-DMA) needs more than 64 channels on both sides (%d, %d)", g->Cin, g->Cout);
  if (h && tile > 9) return refuse(msg, n, "bf16 wgrad plan: tile %d (0, 2, 5, 6, 7, 8, 9)", tile);
  if (p && p->route == W_FOUR) {
    if (xf || !d.vec || !four_tap_geometry(g))
      return h ? refuse(msg, n, "bf16 wgrad plan: tiles 8 / 9 (four taps per block) need a plain operand, k4 s2 p1 and a small grid of whole 8 x 8 tiles")
               : refuse(msg, n, "wgrad plan: tiles 9 / 10 (four taps per block) need a plain operand, the vector path, k4 s2 p1 and a small grid of whole 8 x 8 tiles");
    const int Cg = d.x_is_big ? g->Cin : g->Cout, Csm = d.x_is_big ? g->Cout : g->Cin;
    if (p->T == 128 && Csm % 128 != 0)
      return h ? refuse(msg, n, "bf16 wgrad plan: tile 9 needs a multiple of 128 channels on the small-grid operand")
               : refuse(msg, n, "wgrad plan: tile 10 needs a multiple of 128 channels on the small-grid operand (%d)", Csm);
    const long cgrid = cdiv(Cg, 64) * cdiv(Csm, p->T);
    four_tap_split((long)g->N * (g->Hs / 8) * (g->Ws / 8), cgrid * 4, plan_split, h ? 512 : 256, d);
    d.t = p; d.route = W_FOUR; d.T = p->T; d.big = p->T == 128;
    d.nI = d.nJ = 0;
    d.gx = (unsigned)cgrid; d.gy = 4; d.gz = (unsigned)d.split;
    d.bytes = (double)xb + (double)db;
    d.kind = h ? p->kind : p->kind + (d.x_is_big ? 0 : 1);
    return MOPOE_OK;
  }
  int id;   // the table row that runs
  if (h) {
    // tile 7: the 128 tile on LDS-DMA with TWO taps per block on the side of the gathered operand when that side has 64 channels
    // (conv_gemm_bf16_glds.inc, MERGE): convs with Cin = 64 (1), transposed convs with Cout = 64 (2); plain operands, even tap count
    const int merge_ok = (!xf && taps % 2 == 0) ? (d.x_is_big ? (g->Cin == 64 ? 1 : 0) : (g->Cout == 64 ? 2 : 0)) : 0;
    if (p && p->route == W_MERGE && !merge_ok)
      return refuse(msg, n, "bf16 wgrad plan: tile 7 (two taps per block) needs a plain operand, an even tap count and 64 channels on the gathered side");
    // no tile asked for: the LDS-DMA form (MOPOE_BF16_NO_GLDS = the register-staged one)
    const bool glds = tile >= 0 ? tile >= 5 : f.bf16_glds;
    if (p && p->route == W_MERGE) { id = p->id; d.merge = merge_ok; }
    else id = (glds ? 5 : 0) + (((p && p->T == 64) || !big) ? (glds ? 1 : 2) : 0);
  } else {
    if (p && p->route == W_EMU && xf) return refuse(msg, n, "wgrad plan: tile %d (split-bf16 products) has no BN-on-load form", tile);
    if (needs_big && !big) return refuse(msg, n, "wgrad plan: tile %d (128x128 on LDS-DMA) needs more than 64 channels on both sides (%d, %d)", tile, g->Cin, g->Cout);
    if (tile > 2 && !(p && p->id >= 5)) return refuse(msg, n, "wgrad plan: tile %d (see mopoe_conv_plan in mopoe_hip.h: -1, 0, 2, 5, 6, 7, 8, 9, 10)", tile);
    if (p && p->id >= 5 && !d.vec) return refuse(msg, n, "wgrad plan: the LDS-DMA tiles need the vector path (channel counts %% 4 == 0, aligned tensors)");
    id = (p && p->id >= 2) ? p->id : (big ? 0 : 2);   // the plan may ask for 64x64 tiles on wide layers too
  }
  const WgradTile* t = wgrad_tile(fam, id);
  d.t = t; d.route = t->route; d.T = t->T; d.big = t->T == 128;
  d.nI = d.merge == 1 ? 1 : (int)cdiv(g->Cin, t->T);
  d.nJ = d.merge == 2 ? 1 : (int)cdiv(g->Cout, t->T);
  const int gy = d.merge ? taps / 2 : taps;
  const long tiles = (long)d.nI * d.nJ * gy;
  // split the pixel reduction until ~1024 blocks are in flight, keeping >= min_chunks K-chunks per block
  const long per_block = (long)t->min_chunks * t->kp;
  pixel_split(d.Ms, plan_split > 0 ? plan_split : (1024 + tiles - 1) / tiles, t->kp, (d.Ms + per_block - 1) / per_block, d);
  d.gx = (unsigned)(d.nI * d.nJ); d.gy = (unsigned)gy; d.gz = (unsigned)d.split;
  switch (t->route) {
    case W_MERGE: d.kind = t->kind + d.merge - 1; break;
    case W_EMU: d.kind = t->kind; break;
    case W_REG: d.kind = h ? t->kind + (xf ? 1 : 0) : (d.vec ? t->kind + d.spec : PROF_WGRAD_SCALAR + (d.big ? 0 : 1)); break;
    default: d.kind = t->kind + (xf ? 1 : 0); break;
  }
  return MOPOE_OK;
}

}  // namespace mopoe

#endif  // MOPOE_CONV_LAUNCH_HPP
