"""TEST INFRASTRUCTURE: the committed launch-plan table (mimic_amd/plans_gfx950.json, or the candidate table named by
MOPOE_PLAN_TABLE -- the file read is ops.PLAN_TABLE_PATH) turned into test cases: every (op, geometry, fusion) -> (tile, split)
entry at its own layer geometry, with the batch reduced to the smallest one that keeps the launch on the same code path.

  * parse_key / lookup: a table key -> (op, Geom, fusion flags) and its plan THROUGH ops._table_plan, so that the lookup logic
    (the mask / no-mask fallback of forward convs, the remap used when F32_SPLIT_BF16 is off) is part of what is tested;
  * gather_path / wgrad_path: a host-side restatement of what the library does with a plan (csrc/conv_gemm.hip,
    conv_gemm_bf16.hip: launch_gather, mopoe_conv_wgrad*): edge-kernel routing, vector / scalar decision, the tile after the
    fall-backs, fast addressing, four-tap eligibility, the effective split, refusals.  tests/test_plan_table_cpu.py asserts
    with it that the reduced batch keeps every one of these.  The restatement is independent of the library on purpose:
    tests/test_conv_launch_cpu.py checks it against the decision functions the launchers run (csrc/conv_launch.hpp), on every
    case of the table and on a sweep of tiles, splits, fusions and geometries the table does not reach;
  * reduced_batch: the rule itself (see its docstring);
  * all_cases(): the case list (table entries, remapped plans, opposite-mask forms, mode-3 input gradients), grouped so that
    cases of one (storage family, layer shape, batch) share x, w, dy and the fp64 evaluations of the convolutions;
  * Bundle / run_case / reference / compare: inputs, the call in the keyed form on any backend with the signatures of
    mimic_amd.ops (the HIP library on the GPU, tests/torch_backend.py in fp32 on the CPU), the fp64 evaluation of
    tests/torch_backend.py on the same fp32 (or bf16-rounded) operands, and the project's existing gates element by element.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch

import torch_backend as TB
from mimic_amd import ops
from mimic_amd.ops import Bn, Geom, Mask

BF = torch.bfloat16
ULP = 2.0 ** -7                       # one bf16 rounding step, relative (tests/test_bf16_gpu.py)
WS_BYTES = 64 << 20                   # WS_RECOMMENDED (csrc/conv_launch.hpp); the CPU file checks it against the library
WS_COUNTER_BYTES = ops.WS_COUNTER_BYTES
MIN_ROWS = 1025                       # four 256-row tiles and a one-row tail
GEOM_FIELDS = ("N", "Hs", "Ws", "Hb", "Wb", "Cin", "Cout", "kh", "kw", "sh", "sw", "ph", "pw", "transposed")
MIX_A, MIX_B = 2.0, 0.3


class PlanRefused(Exception):
    """the library would answer MOPOE_ERR_ARG to this plan on this launch"""


# ---- keys ------------------------------------------------------------------------------------------------------------------
def _flag(s):
    return {"0": False, "1": True, "torch.bfloat16": BF, "torch.float32": torch.float32}.get(s, s)


def parse_key(key: str):
    """'op|14 geometry numbers|flags' -> (op, Geom, flags tuple) with flags as ops.conv_* build them"""
    op, geo, flags = key.split("|")
    v = [int(t) for t in geo.split(",")]
    assert len(v) == 14, key
    g = Geom(*v[:13], bool(v[13]))
    fl = tuple(_flag(t) for t in flags.split(","))
    assert ops.plan_key_str((op, g) + fl) == key, key
    return op, g, fl


def table_keys():
    ops._table_plan(("fwd", Geom(1, 1, 1, 1, 1, 4, 4, 1, 1, 1, 1, 0, 0, False), False, False, False))   # (loads the table)
    return sorted(ops._plan_table)


def lookup(op, g, flags, split_bf16=True):
    """(found, (tile, split) or None) through ops._table_plan, with the F32_SPLIT_BF16 switch as given"""
    prev = ops.F32_SPLIT_BF16
    ops.F32_SPLIT_BF16 = split_bf16
    try:
        found, p = ops._table_plan((op, g) + tuple(flags))
    finally:
        ops.F32_SPLIT_BF16 = prev
    return found, (None if p is None else (int(p.tile), int(p.split)))


def is16(op):
    return op.endswith("16")


def kind_of(op):
    return op[:-2] if is16(op) else op


# ---- what the library does with a plan --------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _edge_ok(g, c):
    return (g.kh, g.kw, g.sh, g.sw) == (3, 3, 2, 2) and c % 4 == 0 and c >= 4


_T32_BM = (128, 256, 64, 256, 128, 64, 128, 128, 128, 256, 64, 128, 128, 128, 64, 256)
_T32_BN = (128, 64, 64, 128, 64, 64, 64, 128, 128, 64, 64, 64, 128, 64, 64, 128)
_T16_BM = (128, 256, 64, 256, 128, 128, 128, 256, 256, 128, 128, 64)
_T16_BN = (128, 64, 64, 128, 64, 128, 128, 128, 128, 64, 64, 64)


def gather_path(op, g: Geom, bn_on_load: bool, mask: bool, stats: bool, relu_bn: bool, mix: bool, bias: bool, plan, ws_bytes=WS_BYTES):
    """launch_gather of either family (and the edge routing in front of it) as a dict; PlanRefused where the library refuses"""
    kind, f16 = kind_of(op), is16(op)
    if kind == "fwd":
        dest_small, ck, cn = not g.transposed, g.Cin, g.Cout
    else:
        dest_small, ck, cn = g.transposed, g.Cout, g.Cin
    if not f16:
        plain = not bn_on_load and not mask
        if kind == "fwd" and plain and not g.transposed and g.Cin == 1 and not bias and _edge_ok(g, g.Cout):
            return dict(route="edge_expand")
        if kind == "fwd" and plain and g.transposed and g.Cout == 1 and not stats and _edge_ok(g, g.Cin):
            return dict(route="edge_reduce")
        if kind == "dgrad" and g.transposed and g.Cout == 1 and not relu_bn and _edge_ok(g, g.Cin):
            return dict(route="edge_expand")
    if dest_small:
        hx, wx, hy, wy, hq, wq, nphase = g.Hb, g.Wb, g.Hs, g.Ws, g.Hs, g.Ws, 1
        taps = g.kh * g.kw
    else:
        hx, wx, hy, wy, hq, wq, nphase = g.Hs, g.Ws, g.Hb, g.Wb, g.Hb // g.sh, g.Wb // g.sw, g.sh * g.sw
        taps = max(1, (g.kh // g.sh) * (g.kw // g.sw))
    rpp, rows_total = g.N * hq * wq, g.N * hy * wy
    esz = 2 if f16 else 4
    xb, wb = g.N * hx * wx * ck * esz, g.kh * g.kw * g.Cin * g.Cout * esz
    per = rows_total * cn * 4
    slab = ws_bytes - WS_COUNTER_BYTES
    tile, split = plan if plan is not None else (-1, 0)
    if f16:
        if ck % 32 or cn % 8 or g.Cout % 8 or xb >= 1 << 31 or wb >= 1 << 31:
            raise PlanRefused("bf16 conv: channel counts / sizes")
        if cn > 64:
            cfg = 3 if rpp >= 256 * 128 else (0 if rpp > 64 else 2)
        else:
            cfg = 1 if rpp >= 256 * 64 else 2
        glds_ok = ck % 64 == 0
        if glds_ok:
            cfg = {0: 5, 3: 7, 4: 9}.get(cfg, cfg)
        if tile >= 0:
            if tile >= 12 or tile == 8 or (tile >= 5 and (not glds_ok or (bn_on_load and tile in (6, 8, 10)))):
                raise PlanRefused(f"bf16 conv plan: tile {tile}")
            cfg = tile
        bm, bn = _T16_BM[cfg], _T16_BN[cfg]
        n_mt, n_nt = _cdiv(rpp, bm), _cdiv(cn, bn)
        iters = taps * (ck // (64 if cfg >= 5 else 32))
        blocks = n_mt * n_nt * nphase
        can_split = blocks <= WS_COUNTER_BYTES // 4
        ns = 1
        if split > 0:
            ns = min(split, iters)
            if ns >= 2 and (not can_split or ns * per > slab):
                raise PlanRefused(f"bf16 conv plan: split {ns} (workspace / output tiles)")
        elif can_split and blocks < 256 and iters >= 8:
            ns = min(_cdiv(512, blocks), iters // 4)
            if ns * per > slab:
                ns = slab // per
        return dict(route="gemm", vec=True, tile=cfg, emu=False, nsplit=max(ns, 1), multi_m=n_mt > 1, fast=True, bm=bm, rows=rpp)
    vec = ck % 4 == 0 and g.Cout % 4 == 0 and cn % 4 == 0 and xb < 1 << 31 and wb < 1 << 31
    if mix and not vec:
        raise PlanRefused("conv_fwd_mix: vector path only")
    if cn > 64:
        cfg = 0 if (rpp > 64 or cn >= 256) else 2
    else:
        cfg = 1 if rpp >= 256 * 64 else 2
    if cfg == 0 and cn % 128 == 64 and rpp >= 256 * 64:
        cfg = 1
    emu = False
    if tile >= 0:
        if tile > 19:
            raise PlanRefused(f"conv plan: tile {tile}")
        cfg = tile
        if cfg >= 16:
            if bn_on_load:
                raise PlanRefused(f"conv plan: tile {tile} has no BN-on-load form")
            emu, cfg = True, cfg - 4
        if cfg >= 12 and (not vec or ck % 32 or (bn_on_load and cfg == 13)):
            raise PlanRefused(f"conv plan: tile {tile} (LDS-DMA family)")
        if cfg >= 3 and not vec:
            cfg = 0 if cfg == 3 else 2
        if cfg in (5, 6) and ck % 32:
            cfg -= 3
        if 8 <= cfg < 12 and (not vec or ck % 8 or mix):
            cfg = {8: 0, 9: 1, 10: 2, 11: 4}[cfg]
    bm, bn = _T32_BM[cfg], _T32_BN[cfg]
    n_mt, n_nt = _cdiv(rpp, bm), _cdiv(cn, bn)
    gbk = 32 if (cfg in (5, 6) or cfg >= 12) else (8 if cfg >= 8 else 16)
    iters = taps * _cdiv(ck, gbk)
    blocks = n_mt * n_nt * nphase
    ns = 1
    if split > 0:
        ns = min(split, iters)
        if ns >= 2 and ns * per > slab:
            raise PlanRefused(f"conv plan: split {ns} needs {ns * per} workspace bytes")
    elif blocks < 256 and iters * gbk >= 256:
        ns = min(_cdiv(512, blocks), iters * gbk // 128)
        if ns * per > slab:
            ns = slab // per
    ns = max(ns, 1)
    if ns >= 2 and vec and (cfg < 8 or cfg >= 12) and blocks > WS_COUNTER_BYTES // 4:
        raise PlanRefused(f"conv: split reduction over {blocks} output tiles")
    return dict(route="gemm", vec=vec, tile=cfg, emu=emu, nsplit=ns, multi_m=n_mt > 1, fast=vec and ck % gbk == 0, bm=bm, rows=rpp)


def _four_tap_geom(g):
    return ((g.kh, g.kw, g.sh, g.sw, g.ph, g.pw) == (4, 4, 2, 2, 1, 1) and g.Hs % 8 == 0 and g.Ws % 8 == 0
            and g.Hb == 2 * g.Hs and g.Wb == 2 * g.Ws)


def _pixel_split(ms, split, kp, max_chunks):
    split = max(1, min(split, _cdiv(ms, max_chunks)))
    chunk = _cdiv(_cdiv(ms, split), kp) * kp
    return _cdiv(ms, chunk)


def wgrad_path(op, g: Geom, bn_on_load: bool, plan):
    """mopoe_conv_wgrad / mopoe_conv_wgrad_bf16 as a dict; PlanRefused where the library refuses"""
    f16 = is16(op)
    ms = g.N * g.Hs * g.Ws
    taps = g.kh * g.kw
    tile, split = plan if plan is not None else (-1, 0)
    x_is_big = not g.transposed
    cg, csm = (g.Cin, g.Cout) if x_is_big else (g.Cout, g.Cin)
    big = g.Cin > 64 and g.Cout > 64
    if f16:
        if g.Cin % 8 or g.Cout % 8:
            raise PlanRefused("bf16 wgrad: channel counts")
        if tile == 5 and not big:
            raise PlanRefused("bf16 wgrad plan: tile 5 needs more than 64 channels on both sides")
        if tile in (2, 6):
            big = False
        glds = tile >= 5 if tile >= 0 else True
        merge_ok = (not bn_on_load and taps % 2 == 0) and ((g.Cin == 64) if x_is_big else (g.Cout == 64))
        if tile > 9:
            raise PlanRefused(f"bf16 wgrad plan: tile {tile}")
        if tile >= 8:
            cs = 128 if tile == 9 else 64
            if bn_on_load or not _four_tap_geom(g) or (cs == 128 and csm % 128):
                raise PlanRefused(f"bf16 wgrad plan: tile {tile} (four taps per block)")
            ntiles = g.N * (g.Hs // 8) * (g.Ws // 8)
            cblocks = _cdiv(cg, 64) * _cdiv(csm, cs) * 4
            s = max(1, min(split if split > 0 else _cdiv(512, cblocks), ntiles))
            s = _cdiv(ntiles, _cdiv(ntiles, s))
            return dict(route="four_tap", vec=True, fast=True, tile=tile, T=cs, split=s)
        if tile == 7 and not merge_ok:
            raise PlanRefused("bf16 wgrad plan: tile 7 (two taps per block)")
        merge = tile == 7
        if merge:
            big = True
        t = 128 if big else 64
        n_i = 1 if (merge and x_is_big) else _cdiv(g.Cin, t)
        n_j = 1 if (merge and not x_is_big) else _cdiv(g.Cout, t)
        tiles = n_i * n_j * (taps // 2 if merge else taps)
        kp = 64 if glds else 32
        s = _pixel_split(ms, split if split > 0 else _cdiv(1024, tiles), kp, 4 * kp)
        pow2 = (g.Ws & (g.Ws - 1)) == 0 and ((g.Hs * g.Ws) & (g.Hs * g.Ws - 1)) == 0
        return dict(route="glds" if glds else "reg", vec=True, fast=pow2, tile=tile, T=t, split=s)
    if not bn_on_load and ((not g.transposed and g.Cin == 1 and _edge_ok(g, g.Cout)) or (g.transposed and g.Cout == 1 and _edge_ok(g, g.Cin))):
        return dict(route="edge_wgrad")
    rows_x = g.N * (g.Hs * g.Ws if g.transposed else g.Hb * g.Wb)
    rows_dy = g.N * (g.Hb * g.Wb if g.transposed else g.Hs * g.Ws)
    vec = g.Cin % 4 == 0 and g.Cout % 4 == 0 and rows_x * g.Cin * 4 < 1 << 31 and rows_dy * g.Cout * 4 < 1 << 31
    hw = g.Hs * g.Ws
    fast = vec and (g.Ws % 16 == 0 or (16 % g.Ws == 0 and hw % 16 == 0))
    if tile in (9, 10):
        cs = 128 if tile == 10 else 64
        if bn_on_load or not vec or not _four_tap_geom(g) or (cs == 128 and csm % 128):
            raise PlanRefused(f"wgrad plan: tile {tile} (four taps per block)")
        ntiles = g.N * (g.Hs // 8) * (g.Ws // 8)
        cblocks = _cdiv(cg, 64) * _cdiv(csm, cs) * 4
        s = max(1, min(split if split > 0 else _cdiv(256, cblocks), ntiles))
        s = _cdiv(ntiles, _cdiv(ntiles, s))
        return dict(route="four_tap", vec=vec, fast=fast, tile=tile, T=cs, split=s)
    wemu = tile in (7, 8)
    if wemu and bn_on_load:
        raise PlanRefused(f"wgrad plan: tile {tile} has no BN-on-load form")
    if tile in (2, 6, 8):
        big = False
    elif tile in (5, 7):
        if not big:
            raise PlanRefused(f"wgrad plan: tile {tile} needs more than 64 channels on both sides")
    elif tile > 2:
        raise PlanRefused(f"wgrad plan: tile {tile}")
    glds = tile >= 5
    if glds and not vec:
        raise PlanRefused("wgrad plan: the LDS-DMA tiles need the vector path")
    t = 128 if big else 64
    tiles = _cdiv(g.Cin, t) * _cdiv(g.Cout, t) * taps
    kp = 32 if glds else 16
    s = _pixel_split(ms, split if split > 0 else _cdiv(1024, tiles), kp, 128)
    return dict(route="emu" if wemu else ("glds" if glds else "reg"), vec=vec, fast=fast, tile=tile, T=t, split=s)


# ---- cases -----------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    key: str                      # the table entry this case stands for
    variant: str                  # "table" | "split_bf16_off" | "opposite_mask" | "bn_mode3"
    op: str
    table_geom: Geom
    flags: tuple
    plan: Optional[Tuple[int, int]]
    g: Geom = None                # the geometry the case runs at (reduced batch)
    covers: list = field(default_factory=list)   # table keys that reduce to this very case

    @property
    def id(self):
        return f"{self.key}#{self.variant}"

    @property
    def f16(self):
        return is16(self.op)

    @property
    def kind(self):
        return kind_of(self.op)

    # fusion flags by name
    @property
    def bn(self):          # BN -> ReLU on the gathered operand (fwd, wgrad) / relu_bn + sums (dgrad)
        return bool(self.flags[0])

    @property
    def mask(self):
        return self.kind == "fwd" and bool(self.flags[1])

    @property
    def stats(self):
        return self.kind == "fwd" and bool(self.flags[2])

    @property
    def mix(self):
        return self.kind == "fwd" and self.flags[-1] == "mix"

    @property
    def out_dtype(self):
        if not self.f16 or self.kind == "wgrad":
            return torch.float32
        return self.flags[3] if self.kind == "fwd" else self.flags[2]

    @property
    def bias(self):
        """the image stem is the one forward conv the networks call without a bias (nets.py: ops.conv_fwd(x, conv1.weight, gs,
        out_stats=)); dgrad and wgrad have none"""
        return self.kind == "fwd" and not (not self.table_geom.transposed and self.table_geom.Cin == 1)

    @property
    def text(self):
        """a 1 x L map of the text networks: nn.Dropout (per element); the 2-D blocks use nn.Dropout2d (per sample and channel)"""
        t = self.table_geom
        return t.Hs == 1 and t.Hb == 1 and max(t.Ws, t.Wb) > 1

    def path(self, g=None):
        g = g or self.g
        if self.kind == "wgrad":
            return wgrad_path(self.op, g, self.bn, self.plan)
        return gather_path(self.op, g, self.kind == "fwd" and self.bn, self.mask, self.stats, self.kind == "dgrad" and self.bn,
                           self.mix, self.bias, self.plan)

    @property
    def macs(self):
        g = self.g
        return g.N * g.Hs * g.Ws * g.Cin * g.Cout * g.taps


PATH_KEYS = ("route", "vec", "tile", "emu", "fast", "T", "multi_m", "nsplit", "split")


def same_path(a, b):
    return all(a.get(k) == b.get(k) for k in PATH_KEYS)


def reduced_batch(case: Case) -> int:
    """Hs, Ws, Hb, Wb, channels, kernel, stride and padding stay the layer's own; only N shrinks, to the smallest N' <= N with
      * N' Hs Ws >= 1025 output rows (four 256-row tiles and a one-row tail), or N' = N if the layer never has that many;
      * N' >= 2 (a per-(sample, channel) mask has a boundary);
      * weight gradients: the pixel split the plan asks for survives the library's clamp -- tiles 0 / 2 / 5..8 need
        N' Hs Ws >= 128 (split - 1) + 1, the four-tap tiles N' (Hs/8) (Ws/8) >= split -- and the effective split after the
        library's chunk rounding is the one the launch has at the table's N;
      * 256-row tiles: rows >= 256;
      * and, checked rather than assumed, the same path as at N (same_path: routing, vector / scalar, tile after the fall-backs,
        fast addressing, four-tap form, effective split, more than one M tile where the original has more than one)."""
    t = case.table_geom
    full = case.path(t)
    hw = t.Hs * t.Ws
    lo = max(2, _cdiv(MIN_ROWS, hw))
    if case.kind == "wgrad" and case.plan is not None:
        tile, split = case.plan
        if full["route"] == "four_tap":
            lo = max(lo, _cdiv(split, (t.Hs // 8) * (t.Ws // 8)))
        else:
            lo = max(lo, _cdiv(128 * (split - 1) + 1, hw))
    if full.get("bm") == 256:
        lo = max(lo, _cdiv(256, full["rows"] // t.N))
    for n in range(min(lo, t.N), t.N + 1):
        if same_path(case.path(t.with_batch(n)), full):
            return n
    return t.N


def _mode3_layer(g: Geom) -> bool:
    """conv2 of a residual block whose front (conv1 64 -> 64, 1 x 1) runs as streaming kernels: d1 is never stored and conv2's
    input gradient reads its ReLU mask and x-hat off a2 = relu(bn2(d1)) (trunk.py: Bn mode 3; ops.block_front_supported)"""
    rps_in = g.Hs * g.Ws if g.transposed else g.Hb * g.Wb
    return g.Cin == 64 and g.taps > 1 and rps_in % 32 == 0 and not (g.Hs == 1 and g.Hb == 1)


def all_cases():
    """-> (cases, left_out): every table entry as a case (entries that differ in N alone and reduce to the same launch are one
    case covering both), + the remapped plan of every fp32 entry the F32_SPLIT_BF16-off remap changes, + the opposite-mask form
    of every forward entry that _table_plan would serve from it, + the mode-3 form of the input gradients that have one"""
    raw = []
    for key in table_keys():
        op, g, fl = parse_key(key)
        found, plan = lookup(op, g, fl)
        assert found, key
        raw.append(Case(key, "table", op, g, fl, plan))
        if not is16(op):
            _, off = lookup(op, g, fl, split_bf16=False)
            if off != plan:
                raw.append(Case(key, "split_bf16_off", op, g, fl, off))
        if kind_of(op) == "fwd":
            opp = fl[:1] + (not fl[1],) + fl[2:]
            if ops.plan_key_str((op, g) + opp) not in ops._plan_table:
                found, p2 = lookup(op, g, opp)
                assert found and p2 == plan, key
                raw.append(Case(key, "opposite_mask", op, g, opp, p2))
        if kind_of(op) == "dgrad" and fl[0] and _mode3_layer(g):
            raw.append(Case(key, "bn_mode3", op, g, fl, plan))
    cases, seen, left_out = [], {}, []
    for c in raw:
        try:
            c.g = c.table_geom.with_batch(reduced_batch(c))
        except PlanRefused as e:
            left_out.append((c.id, str(e)))
            continue
        ident = (c.variant, c.op, c.g, c.flags, c.plan)
        if ident in seen:
            seen[ident].covers.append(c.key)
            continue
        c.covers = [c.key]
        seen[ident] = c
        cases.append(c)
    return cases, left_out


def shape_of(g: Geom):
    return tuple(getattr(g, f) for f in GEOM_FIELDS[1:])


def groups(cases):
    """{(family, layer shape): {N': [cases]}}: one test per key, one Bundle per N'"""
    out = {}
    for c in cases:
        out.setdefault(("bf16" if c.f16 else "fp32", shape_of(c.g)), {}).setdefault(c.g.N, []).append(c)
    return out


def share_batches(cases):
    """cases of one (family, shape) run at ONE batch where they can: the largest N' any of them needs, for every case whose own
    table N allows it and whose path it keeps (fewer distinct (shape, N') -> fewer inputs and fp64 convolutions)"""
    by_shape = {}
    for c in cases:
        by_shape.setdefault((c.f16, shape_of(c.g)), []).append(c)
    for cs in by_shape.values():
        top = max(c.g.N for c in cs)
        for c in cs:
            if c.g.N < top <= c.table_geom.N and same_path(c.path(c.table_geom.with_batch(top)), c.path(c.table_geom)):
                c.g = c.table_geom.with_batch(top)
    return cases


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _seed(s: str) -> int:
    return zlib.crc32(s.encode())


def _bn_from(x, c, gen, dev):
    """train-mode BatchNorm (mode 1) with the batch statistics of x; |gamma| >= 0.25 so that a margin on x is one on bn(x)"""
    gamma = 1 + 0.3 * torch.randn(c, generator=gen, device=dev)
    gamma = torch.where(gamma.abs() < 0.25, torch.full_like(gamma, 0.25), gamma)
    beta = 0.2 * torch.randn(c, generator=gen, device=dev)
    x2 = x.reshape(-1, c).double()
    return Bn(gamma, beta, 1, sums=torch.stack([x2.sum(0), (x2 * x2).sum(0)]), count=x2.shape[0])


def _clear_of_zero(x, bn, margin, dtype):
    """move the elements of x whose pre-activation bn(x) lies within `margin` of zero away from it (the BatchNorm keeps the sums
    it was given): the ReLU mask of an input gradient is then the same in fp32, in fp64 and in the kernel's fma, and the
    reference cannot leave the bar through a sign decided by the last bit"""
    _, _, scale, shift = TB.bn_coef(bn)
    for _ in range(4):
        v = x.double() * scale + shift
        near = v.abs() < margin
        if not bool(near.any()):
            break
        target = torch.where(v >= 0, 2.0 * margin, -2.0 * margin)
        x = torch.where(near, ((target - shift) / scale), x.double()).to(dtype)
    v = x.double() * scale + shift
    assert float(v.abs().min()) >= 0.5 * margin, float(v.abs().min())
    return x


class Bundle:
    """x, w, dy, the operand's BatchNorm and the fp64 convolutions of one (storage family, geometry): shared by its cases and
    left unchanged by them.  Values seeded from crc32 of the shape (shared tensors) and of the case id (everything else)."""

    def __init__(self, f16: bool, g: Geom, dev):
        self.f16, self.g, self.dev = f16, g, torch.device(dev)
        self.dtype = BF if f16 else torch.float32
        gen = self.gen(("bf16|" if f16 else "fp32|") + ",".join(map(str, shape_of(g))) + f"|{g.N}")
        rn = lambda shape: torch.randn(shape, generator=gen, device=self.dev)
        x = rn(g.in_shape).to(self.dtype)
        self.w = (rn((g.taps, g.Cin, g.Cout)) / math.sqrt(g.taps * g.Cin)).to(self.dtype)
        self.dy = rn(g.out_shape).to(self.dtype)
        self.bn = _bn_from(x.float(), g.Cin, gen, self.dev)
        self.x = _clear_of_zero(x, self.bn, 5e-2 if f16 else 1e-3, self.dtype)
        # mode 3 (conv_dgrad reads the ACTIVATION a = relu(bn(.))): exact zeros where the ReLU cut
        self.act = torch.relu(rn(g.in_shape)).to(self.dtype)
        self._core = {}
        if f16:     # the weight and gradient of the image-side fp32 tensors do not occur: bf16 entries are GEMM layers only
            assert min(g.Cin, g.Cout) > 1

    def gen(self, s):
        return torch.Generator(device=self.dev).manual_seed(_seed(s))

    # fp64 evaluations of tests/torch_backend.py on the same operands, once per bundle
    def core(self, what):
        if what not in self._core:
            g, d = self.g, torch.float64
            if what == "fwd":
                r = TB.conv_fwd(self.x.to(d), self.w.to(d), g)
            elif what == "fwd_bn":
                # bf16 family: the operand relu(bn(x)) rounded to bf16 as the emulation rounds it, then fp64 products
                r = TB.conv_fwd(TB._act16(self.x, self.bn).to(d), self.w.to(d), g) if self.f16 else \
                    TB.conv_fwd(self.x.to(d), self.w.to(d), g, bn_in=self.bn)
            elif what == "dgrad":
                r = TB.conv_dgrad(self.dy.to(d), self.w.to(d), g)
            elif what == "wgrad":
                r = TB.conv_wgrad(self.x.to(d), self.dy.to(d), g)
            elif what == "wgrad_bn":
                r = TB.conv_wgrad(TB._act16(self.x, self.bn).to(d), self.dy.to(d), g) if self.f16 else \
                    TB.conv_wgrad(self.x.to(d), self.dy.to(d), g, bn_in=self.bn)
            self._core[what] = r
        return self._core[what]


def case_inputs(case: Case, b: Bundle):
    """everything a case needs beyond the bundle, seeded from crc32 of the case id"""
    g, dev = b.g, b.dev
    gen = b.gen(case.id)
    h = {}
    if case.kind == "fwd":
        rows_out = math.prod(g.out_shape[:3])
        if case.bias:
            h["bias"] = 0.1 * torch.randn(g.Cout, generator=gen, device=dev)
        if case.mask:
            if case.text:
                h["mask"] = Mask((torch.rand(g.out_shape, generator=gen, device=dev) < 0.5).float() * 2, 2, rows_out // g.N)
            else:
                h["mask"] = Mask((torch.rand(g.N, g.Cout, generator=gen, device=dev) < 0.5).float() * 2, 1, rows_out // g.N)
        if case.stats:
            h["stats0"] = (5.0 * torch.randn(2, g.Cout, generator=gen, device=dev)).double() + 1.0
        if case.mix:
            s = torch.randn(g.out_shape, generator=gen, device=dev).to(case.out_dtype)
            h["s"], h["bns"] = s, _bn_from(s.float(), g.Cout, gen, dev)
    elif case.kind == "dgrad" and case.bn:
        h["sums0"] = (5.0 * torch.randn(2, g.Cin, generator=gen, device=dev)).double() + 1.0
        if case.variant == "bn_mode3":
            h["relu_bn"], h["xin"] = Bn(b.bn.gamma, b.bn.beta, 3, sums=b.bn.sums, count=b.bn.count), b.act
        else:
            h["relu_bn"], h["xin"] = b.bn, b.x
    return h


def run_case(case: Case, b: Bundle, h, backend):
    """the call in the keyed form on `backend` (mimic_amd.ops, or tests/torch_backend.py in fp32) -> {name: tensor}"""
    g = b.g
    if case.kind == "fwd":
        st = h["stats0"].clone() if case.stats else None
        y = backend.conv_fwd(b.x, b.w, g, bn_in=b.bn if case.bn else None, bias=h.get("bias"), mask=h.get("mask"), out_stats=st,
                             out_dtype=case.out_dtype, mix=(h["s"], h["bns"], MIX_A, MIX_B) if case.mix else None)
        return dict(y=y, stats=st) if case.stats else dict(y=y)
    if case.kind == "dgrad":
        sm = h["sums0"].clone() if case.bn else None
        dx = backend.conv_dgrad(b.dy, b.w, g, relu_bn=h.get("relu_bn"), xin=h.get("xin"), bwd_sums=sm, out_dtype=case.out_dtype)
        return dict(dx=dx, sums=sm) if case.bn else dict(dx=dx)
    return dict(dw=backend.conv_wgrad(b.x, b.dy, g, bn_in=b.bn if case.bn else None))


def reference(case: Case, b: Bundle, h):
    """fp64: the bundle's convolution + the epilogue of tests/torch_backend.py (conv_fwd / conv_dgrad) restated on it, with the
    bf16 family's rounding points; tests/test_plan_table_cpu.py holds this restatement equal to torch_backend's own"""
    if case.kind == "fwd":
        y = b.core("fwd_bn" if case.bn else "fwd")
        if case.bias:
            y = y + h["bias"]
        if case.mask:
            y = y * TB._mask_mult(y, h["mask"])
        if case.mix:
            _, _, scale, shift = TB.bn_coef(h["bns"])
            y = MIX_A * (h["s"].double() * scale + shift) + MIX_B * y
        if case.out_dtype == BF:
            y = y.to(BF).double()
        out = dict(y=y)
        if case.stats:
            y2 = y.reshape(-1, y.shape[-1])
            out["stats"] = h["stats0"] + torch.stack([y2.sum(0), (y2 * y2).sum(0)])
        return out
    if case.kind == "dgrad":
        dx = b.core("dgrad")
        if not case.bn:
            return dict(dx=dx.to(BF).double() if case.out_dtype == BF else dx)
        xin = h["xin"].double()
        mean, rstd, scale, shift = TB.bn_coef(h["relu_bn"])
        dx = dx * ((xin * scale + shift) > 0).to(dx.dtype)
        if case.out_dtype == BF:
            dx = dx.to(BF).double()
        xhat = (xin - mean) * rstd
        c = dx.shape[-1]
        sums = h["sums0"] + torch.stack([dx.reshape(-1, c).sum(0), (dx * xhat).reshape(-1, c).sum(0)])
        return dict(dx=dx, sums=sums)
    return dict(dw=b.core("wgrad_bn" if case.bn else "wgrad"))


# ---- gates -----------------------------------------------------------------------------------------------------------------
def bars(case: Case):
    """{result: (rtol, atol_rel)} of `check` (|got - ref| <= atol_rel max|ref| + rtol |ref|) -- the project's existing ones:
    fp32 tensors 2e-4 / 2e-4, fp32 weight gradients 5e-4 (3e-4 on the four-tap tiles), statistics 1e-4, sums 2e-4
    (tests/test_hip_ops_gpu.py); bf16 family as tests/test_bf16_gpu.py: a bf16 result one rounding step (1.01 ULP) + 2e-4 of the
    scale (1.5e-3 with BN -> ReLU on the operand), fp32 results as in fp32, statistics and sums 2e-3, weight gradients 3e-4
    (2e-3 / 1e-3 with BN -> ReLU on the operand)"""
    if not case.f16:
        if case.kind == "fwd":
            return dict(y=(2e-4, 2e-4), stats=(1e-4, 1e-4))
        if case.kind == "dgrad":
            return dict(dx=(2e-4, 2e-4), sums=(2e-4, 2e-4))
        four = case.plan is not None and case.plan[0] in (9, 10)
        return dict(dw=(3e-4, 3e-4) if four else (5e-4, 5e-4))
    if case.kind == "wgrad":
        return dict(dw=(2e-3, 1e-3) if case.bn else (3e-4, 3e-4))
    out16 = case.out_dtype == BF
    if case.kind == "fwd":
        on_load = case.bn
        return dict(y=((1.01 * ULP) if out16 else 2e-4, 1.5e-3 if (on_load and out16) else 2e-4), stats=(2e-3, 2e-3))
    return dict(dx=((1.01 * ULP) if out16 else 2e-4, 2e-4), sums=(2e-3, 2e-3))


def fp32_claim(case: Case) -> bool:
    """plain-operand cases on the fp32 tiles with the products on the bf16 matrix pipe (gather 16..19, weight gradient 7..10):
    also relative L2 < 2e-6 and max error < 1e-5 of max|ref| against fp64 (test_f32_products_on_the_bf16_pipe)"""
    if case.f16 or case.plan is None or (case.kind == "fwd" and case.bn) or (case.kind == "wgrad" and case.bn):
        return False
    return case.plan[0] in ((7, 8, 9, 10) if case.kind == "wgrad" else (16, 17, 18, 19))


def measure(got, ref, rtol, atol_rel):
    """on the tensors' device -> (worst error / bound, relative L2, max error / max|ref|, finite)"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = max(float(ref.abs().max()), 1e-6)
    err = (got - ref).abs()
    bound = atol_rel * scale + rtol * ref.abs()
    return (float((err / bound).max()), float(err.norm() / ref.norm().clamp_min(1e-300)), float(err.max()) / scale,
            bool(torch.isfinite(got).all()))


def compare(case: Case, got, ref, bar_scale=1.0, log=None, claim=True):
    """every result of the case against its fp64 reference, element by element; -> (worst ratio, worst relative L2).
    bar_scale scales the bars of fp32-typed results (the CPU file runs the fp32 references at half of them); a result STORED in
    bf16 keeps its bar: one rounding step is the grain of the format, half a step is not a bound a correctly rounded value meets"""
    worst, worst_l2, fails = 0.0, 0.0, []
    for name, (rtol, atol_rel) in bars(case).items():
        if name not in ref:
            continue
        stored16 = case.out_dtype == BF and case.kind != "wgrad"
        k = 1.0 if stored16 else bar_scale
        ratio, l2, mx, finite = measure(got[name], ref[name], k * rtol, k * atol_rel)
        worst, worst_l2 = max(worst, ratio), max(worst_l2, l2 if name in ("y", "dx", "dw") else 0.0)
        if not finite:
            fails.append(f"{name}: not finite")
        if not ratio <= 1.0:
            fails.append(f"{name}: worst error / bound {ratio:.3f} (rtol {k * rtol:.2e}, atol {k * atol_rel:.2e} of max|ref|; rel L2 {l2:.2e})")
        if name in ("y", "dx", "dw") and claim and fp32_claim(case) and not (l2 < 2e-6 and mx < 1e-5):
            fails.append(f"{name}: fp32 claim on the bf16 pipe: rel L2 {l2:.3e} (< 2e-6), max {mx:.3e} (< 1e-5)")
        if name in ("y", "dx") and got[name].dtype != case.out_dtype:
            fails.append(f"{name}: dtype {got[name].dtype}, keyed {case.out_dtype}")
    if log is not None:
        p = case.plan
        log(f"plan_table/{case.id}: N'={case.g.N} plan={'static' if p is None else f't{p[0]}s{p[1]}'} relL2={worst_l2:.3e} worst/bound={worst:.3f}"
            + ("" if not fails else "  FAIL " + "; ".join(fails)))
    return worst, worst_l2, fails
