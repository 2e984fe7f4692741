"""The launch decisions of the conv families (csrc/conv_launch.hpp: decide_gather / decide_wgrad, the code the launchers of
conv_gemm.hip and conv_gemm_bf16.hip run) against their independent restatement in tests/plan_cases.py (gather_path /
wgrad_path), on the CPU: tests/tools/conv_launch_shim.cpp is built with the host compiler, loaded with ctypes, and nothing is
launched.

  * every case of the committed plan table, at the table's geometry and at the reduced one the GPU file runs;
  * a sweep over what the table does not reach: every tile id from -1 to two past the family's last, splits 0 / 1 / 3 / 64, the
    fusions of each op, a second workspace size (counters + three output slabs), on geometries chosen for the branches (direct
    tiles, scalar path, K chunks that do not divide, the 64-column remainder, fewer than 64 rows, more output tiles than arrival
    counters, four-tap and two-tap weight gradients);
  * every accepted decision's profiling kind is one ops.PROF_KINDS names, with the kernel of the decided tile and its block;
  * the tile tables of mimic_amd/ops.py (tuner candidates, kernel names) agree with the header's on every field they share.

Edge-kernel routing happens in the extern "C" entry points in front of the decision and is not part of it: those cases are
skipped, and the test holds the skipped set to exactly them.
"""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

import plan_cases as PC
from mimic_amd import ops
from mimic_amd.ops import Geom

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = os.path.join(HERE, "tools", "conv_launch_shim.cpp")
WGRAD_ROUTES = ("reg", "glds", "emu", "glds", "four_tap")     # WgradRoute -> the mirror's name (two taps per block: an LDS-DMA form)
GATHER_OUT = ("vec", "tile", "emu", "spec", "nsplit", "reduce", "gx", "nNt", "nphase", "bm", "bn", "bk", "rows", "rows_total", "kind", "slab_offset")
WGRAD_OUT = ("route", "T", "big", "merge", "vec", "split", "chunk", "atomic", "fast", "spec", "nI", "nJ", "gx", "gy", "gz", "kind")
GATHER_TILE = ("kernel", "id", "bm", "bn", "threads", "bk", "stages", "bn_form", "in_kernel", "kind", "kind_bn")
WGRAD_TILE = ("route", "id", "T", "kp", "kind")
GATHER_KERNELS = ("LDS_S", "LDS", "DIRECT", "GLDS", "EMU", "HREG", "HGLDS", "HNONE")     # enum GatherKernel, without G_
WGRAD_ROUTE_NAMES = ("W_REG", "W_GLDS", "W_EMU", "W_MERGE", "W_FOUR")                     # enum WgradRoute


@pytest.fixture(scope="session")
def shim(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    so = str(tmp_path_factory.mktemp("conv_launch") / "conv_launch_shim.so")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-o", so, SHIM_SRC])
    lib = ctypes.CDLL(so)
    lib.shim_ws_counter_bytes.restype = lib.shim_ws_recommended.restype = ctypes.c_longlong
    lib.shim_gather.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    lib.shim_wgrad.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    lib.shim_gather_tile.argtypes = lib.shim_wgrad_tile.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    # the library's tile tables: {(family, "gather" | "wgrad"): [row as a dict]}
    lib.tiles = {}
    for fam, (grp, door, fields) in itertools.product((0, 1), (("gather", lib.shim_gather_tile, GATHER_TILE), ("wgrad", lib.shim_wgrad_tile, WGRAD_TILE))):
        buf, rows = (ctypes.c_int * len(fields))(), []
        while door(fam, len(rows), buf) == 0:
            rows.append(dict(zip(fields, buf)))
        assert door(fam, -1, buf) != 0 and door(fam, len(rows) + 1, buf) != 0
        lib.tiles[(fam, grp)] = rows
    return lib


def _geom_ints(g):
    return (ctypes.c_int * 14)(*[int(getattr(g, f)) for f in PC.GEOM_FIELDS])


_OUT = (ctypes.c_longlong * 16)()
_MSG = ctypes.create_string_buffer(512)


def decide(lib, op, g, bn=False, mask=0, relu_bn=0, mix=False, out_f32=False, plan=None, ws_bytes=PC.WS_BYTES, aligned=True,
           xcd_remap=True, glds=True):
    """the library's decision as a dict with the mirror's keys (+ the rest of the decision), or PlanRefused with its message"""
    kind, fam = PC.kind_of(op), 1 if PC.is16(op) else 0
    tile, split = plan if plan is not None else (-1, 0)
    if kind == "wgrad":
        args = (ctypes.c_int * 6)(int(bn), int(aligned), tile, split, int(xcd_remap), int(glds))
        rc = lib.shim_wgrad(fam, _geom_ints(g), args, _OUT, _MSG, len(_MSG))
        if rc:
            assert rc == -1, rc
            raise PC.PlanRefused(_MSG.value.decode())
        d = dict(zip(WGRAD_OUT, _OUT), fam=fam, group="wgrad")
        d.update(route=WGRAD_ROUTES[d["route"]], route_id=d["route"], vec=bool(d["vec"]), tile=tile,
                 fast=bool(d["fast"]) or (fam == 1 and d["route"] == 4))     # (the mirror's bf16 four-tap form carries fast = True)
        return d
    fwd = kind == "fwd"
    dest_small, ck, cn = (not g.transposed, g.Cin, g.Cout) if fwd else (g.transposed, g.Cout, g.Cin)
    args = (ctypes.c_int * 14)(int(dest_small), ck, cn, 0 if fwd else 1, int(bn), int(mask), int(relu_bn), int(mix), int(out_f32),
                               int(aligned), tile, split, int(xcd_remap), int(glds))
    rc = lib.shim_gather(fam, _geom_ints(g), args, ws_bytes, _OUT, _MSG, len(_MSG))
    if rc:
        assert rc == -1, rc
        raise PC.PlanRefused(_MSG.value.decode())
    d = dict(zip(GATHER_OUT, _OUT), fam=fam, group="gather")
    d.update(route="gemm", vec=bool(d["vec"]), emu=bool(d["emu"]), fast=d["spec"] != 0, multi_m=PC._cdiv(d["rows"], d["bm"]) > 1)
    return d


COMPARED = PC.PATH_KEYS + ("bm", "rows")


def differences(mirror, lib):
    return {k: (mirror[k], lib[k]) for k in COMPARED if k in mirror and mirror[k] != lib[k]}


def _template_ints(name):
    return [int(x) for x in name[name.index("<") + 1:-1].split(", ") if x.isdigit()]


def _block_of(kernel, args):
    """(bm, bn) a gather kernel's template arguments stand for: BM, BN lead them, except direct_gemm_kernel<WGM, WGN, MI, NI, spec>
    (32 x 32 MFMA tiles: MI x NI per wave)"""
    return (32 * args[0] * args[2], 32 * args[1] * args[3]) if kernel == "DIRECT" else (args[0], args[1])


def check_kind(lib, d):
    """the decision's kind has a name in ops.PROF_KINDS, and it is the kernel of the decided tile with the decided block"""
    name = ops.PROF_KINDS[d["kind"]] if 0 <= d["kind"] < len(ops.PROF_KINDS) else None
    assert name is not None, d
    if d["group"] == "gather":
        row = lib.tiles[(d["fam"], "gather")][d["tile"] + (4 if d["emu"] else 0)]
        kernel = GATHER_KERNELS[row["kernel"]]
        assert (row["bm"], row["bn"]) == (d["bm"], d["bn"]) and name.startswith(ops._GATHER_KERNELS[kernel] + "<"), (name, d)
        assert _block_of(kernel, _template_ints(name)) == (d["bm"], d["bn"]), (name, d)
        assert ("false" in name) == (d["fam"] == 0 and not d["vec"]), (name, d)      # (the scalar path's forms, and no other, say so)
    else:
        mine = [t for t in (ops._BF16_WGRAD_TILES if d["fam"] else ops._F32_WGRAD_TILES)
                if (t.route, t.T) == (WGRAD_ROUTE_NAMES[d["route_id"]], d["T"])]
        assert len(mine) == 1 and name.startswith(mine[0].kernel + "<") and _template_ints(name)[0] == d["T"], (name, d)


# ---- the tuner's tile tables (mimic_amd/ops.py) against the library's ----------------------------------------------------------------
def test_the_tuners_tile_tables_restate_the_librarys(shim):
    for fam, mine in ((0, ops._F32_GATHER_TILES), (1, ops._BF16_GATHER_TILES)):
        theirs = shim.tiles[(fam, "gather")]
        assert len(mine) == len(theirs) and [t.id for t in mine] == [r["id"] for r in theirs] == list(range(len(mine)))
        for t, r in zip(mine, theirs):
            assert (GATHER_KERNELS.index(t.kernel), t.bm, t.bn, int(t.bn_form), t.kind, t.kind_bn or 0) == \
                   (r["kernel"], r["bm"], r["bn"], r["bn_form"], r["kind"], r["kind_bn"]), (t, r)
            assert t.k_multiple in (1, r["bk"]), (t, r)      # where the tuner asks for a K multiple it is the tile's K chunk
            assert (t.scalar_targs is not None) == (t.kernel == "LDS_S") and (t.kernel == "LDS_S" or fam == 1) != t.vec_only, t
            # the template arguments say what the row says: block, waves and, where they are arguments, K chunk and LDS buffers
            a = _template_ints(f"<{t.targs.format(1)}>")
            waves = a[0] * a[1] if t.kernel == "DIRECT" else a[2] * a[3] * (a[6] if t.kernel in ("GLDS", "EMU") else 1)
            assert _block_of(t.kernel, a) == (t.bm, t.bn) and 64 * waves == r["threads"], (t, r)
            if t.kernel in ("LDS_S", "LDS"):
                assert a[4] == r["bk"] and (not t.scalar_targs or _template_ints(f"<{t.scalar_targs}>")[:2] == [t.bm, t.bn]), (t, r)
            if t.kernel in ("GLDS", "EMU", "HGLDS"):
                assert a[5] == r["stages"] and (t.kernel == "HGLDS" or a[7] == (t.kernel == "EMU")), (t, r)
            # a twin is the same block on the fp32 MFMA
            if t.twin is not None:
                assert t.kernel == "EMU" and (mine[t.twin].kernel, mine[t.twin].bm, mine[t.twin].bn) == ("GLDS", t.bm, t.bn), t
            assert (t.twin is not None) == (t.kernel == "EMU"), t
    for fam, mine in ((0, ops._F32_WGRAD_TILES), (1, ops._BF16_WGRAD_TILES)):
        theirs = shim.tiles[(fam, "wgrad")]
        assert len(mine) == len(theirs)
        for t, r in zip(mine, theirs):
            assert (WGRAD_ROUTE_NAMES.index(t.route), t.id, t.T, t.kind) == (r["route"], r["id"], r["T"], r["kind"]), (t, r)
            assert all(_template_ints(f"<{a}>")[0] == t.T for a in t.targs + ((t.scalar_targs,) if t.scalar_targs else ())), t
            # a twin runs without the bf16 matrix pipe on the same block -- of a four-tap tile (64 gathered channels x T): on
            # the 64 x 64 register-staged tile, whatever T
            assert (t.twin is not None) == (fam == 0 and t.route in ("W_EMU", "W_FOUR")), t
            if t.twin is not None:
                twin = [u for u in mine if u.id == t.twin]
                assert len(twin) == 1 and (twin[0].route, twin[0].T) == (("W_REG", 64) if t.route == "W_FOUR" else ("W_GLDS", t.T)), t
    # no kind is named twice: every name of PROF_KINDS comes from one row and one instantiation
    kinds = [k for t in ops._F32_GATHER_TILES + ops._BF16_GATHER_TILES for k, _ in ops._gather_kinds(t)] + \
            [32 + t.id for t in ops._F32_GATHER_TILES if t.scalar_targs] + \
            [t.kind + i for t in ops._F32_WGRAD_TILES + ops._BF16_WGRAD_TILES for i in range(len(t.targs))] + [42, 43] + list(range(124, 130))
    assert len(kinds) == len(set(kinds)) and set(kinds) == {i for i, n in enumerate(ops.PROF_KINDS) if n is not None}
    assert len(ops.PROF_KINDS) == 144      # include/mopoe_hip.h: MOPOE_PROF_KINDS


# ---- the committed plan table ------------------------------------------------------------------------------------------------
def _case_decision(lib, c, g):
    relu = (3 if c.variant == "bn_mode3" else 1) if (c.kind == "dgrad" and c.bn) else 0
    return decide(lib, c.op, g, bn=c.kind != "dgrad" and c.bn, mask=(2 if c.text else 1) if c.mask else 0, relu_bn=relu, mix=c.mix,
                  out_f32=c.f16 and c.kind != "wgrad" and c.out_dtype != PC.BF, plan=c.plan)


def test_every_case_of_the_plan_table_decides_as_the_mirror_says(shim):
    assert shim.shim_ws_recommended() == PC.WS_BYTES and shim.shim_ws_counter_bytes() == PC.WS_COUNTER_BYTES
    cases, left_out = PC.all_cases()
    assert cases and not left_out
    n, edge, bad = 0, [], []
    for c in cases:
        for g in (c.table_geom, c.g):
            n += 1
            want = c.path(g)
            if want["route"].startswith("edge_"):
                edge.append((c.id, g.N))
                continue
            got = _case_decision(shim, c, g)
            check_kind(shim, got)
            diff = differences(want, got)
            if diff:
                bad.append((c.id, g.N, diff))
    assert not bad, f"{len(bad)} of {n} evaluations differ (mirror, library): {bad[:5]}"
    assert n == 2 * len(cases)
    # the skipped evaluations are the image-side single-channel layers and nothing else, and they are few
    assert all(min(PC.parse_key(i.split("#")[0])[1].Cin, PC.parse_key(i.split("#")[0])[1].Cout) == 1 for i, _ in edge)
    assert 0 < len(edge) < 0.02 * n, (len(edge), n)


# ---- the sweep -------------------------------------------------------------------------------------------------------------------
def _k4s2(n, hs, cin, cout, t):
    return Geom(n, hs, hs, 2 * hs, 2 * hs, cin, cout, 4, 4, 2, 2, 1, 1, t)


def _same(n, h, w, cin, cout, k, t=False):
    return Geom(n, h, w, h, w, cin, cout, k, k, 1, 1, k // 2, k // 2, t)


GEOMS = [_k4s2(4, hs, ci, co, t) for hs in (8, 32) for (ci, co) in ((64, 128), (128, 64), (128, 256), (32, 32)) for t in (False, True)] + [
    _same(8, 16, 16, 64, 256, 1),                               # 1 x 1
    _same(4, 16, 16, 64, 64, 3),                                # k3 s1 p1
    Geom(8, 1, 64, 1, 128, 128, 128, 1, 4, 1, 2, 0, 1, False),   # a 1 x L text map
    Geom(8, 1, 24, 1, 48, 128, 64, 1, 4, 1, 2, 0, 1, True),      # ... whose length is no power of two
    _same(4, 16, 16, 40, 64, 3),                                # Ck % 32 != 0, % 8 == 0: 5 / 6 fall back, LDS-DMA refused, direct tiles run
    _same(4, 16, 16, 36, 68, 3),                                # % 4 == 0 only: the direct tiles fall back
    _same(4, 16, 16, 96, 128, 3),                               # Ck % 64 != 0, % 32 == 0: the bf16 LDS-DMA tiles are refused
    _same(4, 16, 16, 6, 10, 3),                                 # channel counts no multiples of 4: scalar path; bf16 refuses
    _same(16, 32, 32, 64, 192, 3),                              # Cn % 128 == 64 with 16384 rows per phase
    _same(16, 32, 32, 192, 64, 3, True),
    _same(2, 4, 4, 128, 128, 3),                                # fewer than 64 rows
    _same(2, 4, 4, 64, 320, 1),
    _same(64, 128, 128, 64, 128, 1),                            # more output tiles than arrival counters
    _k4s2(2, 24, 64, 128, False),                               # four taps per block on a grid that is no power of two
    _k4s2(2, 12, 64, 128, False),                               # ... and on one that is not made of 8 x 8 tiles
]
SPLITS = (0, 1, 3, 64)
LAST = {("fp32", "gather"): 19, ("bf16", "gather"): 11, ("fp32", "wgrad"): 10, ("bf16", "wgrad"): 9}
# tile ids the parent library has no acceptance for (outside the family's list, or not built) ...
NEVER_ACCEPTED = {("fp32", "gather"): {20, 21}, ("bf16", "gather"): {8, 12, 13}, ("fp32", "wgrad"): {3, 4, 11, 12}, ("bf16", "wgrad"): {10, 11}}
# ... and the ones it has no plan-dependent refusal for (fp32 weight gradients on the register-staged tiles take any layer)
NEVER_REFUSED = {("fp32", "wgrad"): {-1, 0, 1, 2}}


def _sweep(lib):
    """-> [(family, kind, op, g, flags, plan, ws, mirror result or None, library result or None)]"""
    out = []
    for f16, kind in itertools.product((False, True), ("fwd", "dgrad", "wgrad")):
        fam, grp = "bf16" if f16 else "fp32", "wgrad" if kind == "wgrad" else "gather"
        op = kind + ("16" if f16 else "")
        flag_sets = {"fwd": list(itertools.product((False, True), repeat=3)), "dgrad": [(False,), (True,)], "wgrad": [(False,), (True,)]}[kind]
        for g in GEOMS:
            rows_out = (g.N * g.Hs * g.Ws if not g.transposed else g.N * g.Hb * g.Wb) if kind == "fwd" else \
                       (g.N * g.Hb * g.Wb if not g.transposed else g.N * g.Hs * g.Ws)
            cn = g.Cout if kind == "fwd" else g.Cin
            sizes = (None,) if kind == "wgrad" else (PC.WS_BYTES, PC.WS_COUNTER_BYTES + 3 * rows_out * cn * 4)
            for tile, split, flags, ws in itertools.product(range(-1, LAST[(fam, grp)] + 3), SPLITS, flag_sets, sizes):
                plan = (tile, split)
                try:
                    if kind == "wgrad":
                        want = PC.wgrad_path(op, g, flags[0], plan)
                    elif kind == "fwd":
                        want = PC.gather_path(op, g, flags[0], flags[1], False, False, flags[2], True, plan, ws_bytes=ws)
                    else:
                        want = PC.gather_path(op, g, False, False, False, flags[0], False, False, plan, ws_bytes=ws)
                except PC.PlanRefused:
                    want = None
                try:
                    if kind == "wgrad":
                        got = decide(lib, op, g, bn=flags[0], plan=plan)
                    elif kind == "fwd":
                        got = decide(lib, op, g, bn=flags[0], mask=int(flags[1]), mix=flags[2], plan=plan, ws_bytes=ws)
                    else:
                        got = decide(lib, op, g, relu_bn=int(flags[0]), plan=plan, ws_bytes=ws)
                except PC.PlanRefused as e:
                    got = None
                    assert str(e), (op, g, plan)
                out.append((fam, grp, op, g, flags, plan, ws, want, got))
    return out


def test_the_sweep_decides_as_the_mirror_says_and_reaches_every_branch(shim):
    res = _sweep(shim)
    bad = []
    for fam, grp, op, g, flags, plan, ws, want, got in res:
        assert want is None or not want["route"].startswith("edge_"), (op, g)
        if (want is None) != (got is None):
            bad.append((op, g, flags, plan, ws, "mirror " + ("refuses" if want is None else "accepts")))
        elif got is not None:
            check_kind(shim, got)
            diff = differences(want, got)
            if diff:
                bad.append((op, g, flags, plan, ws, diff))
    assert not bad, f"{len(bad)} of {len(res)} evaluations differ (mirror, library): {bad[:5]}"

    # a refusal and an acceptance for every tile id of every family, where the library has both
    for key, last in LAST.items():
        mine = [(r[5][0], r[8] is not None) for r in res if (r[0], r[1]) == key]
        ids = set(range(-1, last + 3))
        accepted, refused = {t for t, ok in mine if ok}, {t for t, ok in mine if not ok}
        assert accepted == ids - NEVER_ACCEPTED[key], (key, sorted(ids - accepted))
        assert refused == ids - NEVER_REFUSED.get(key, set()), (key, sorted(ids - refused))

    # every fall-back branch of the fp32 gather family
    moved = {(r[5][0], r[8]["tile"], r[8]["vec"]) for r in res if r[0] == "fp32" and r[1] == "gather" and r[8] is not None and r[5][0] >= 0}
    vec_moves = {(p, t) for p, t, v in moved if v and p != t and not (p >= 16 and t == p - 4)}
    # (6 -> 3: the library subtracts 3 from both 32-deep tiles, so 6 = 128x64 lands on 3 = 256x128 and not on its 16-deep twin 4;
    # the mirror says the same, and this file holds behaviour as it is)
    assert vec_moves == {(5, 2), (6, 3), (8, 0), (9, 1), (10, 2), (11, 4)}, sorted(vec_moves)
    scalar_moves = {(p, t) for p, t, v in moved if not v}
    assert scalar_moves == {(0, 0), (1, 1), (2, 2), (3, 0)} | {(p, 2) for p in range(4, 12)}, sorted(scalar_moves)
    assert {p for p, t, v in moved if 8 <= p < 12 and p == t} == {8, 9, 10, 11}        # (and the direct tiles themselves run)
    assert {(p, t) for p, t, v in moved if p >= 16} == {(p, p - 4) for p in range(16, 20)}
    # the static choice takes the 64-column remainder and the small tile
    static = {r[8]["tile"] for r in res if r[0] == "fp32" and r[1] == "gather" and r[8] is not None and r[5][0] == -1}
    assert static >= {0, 1, 2}, static
    # both kinds of reduction, in both families the one they have
    assert {r[8]["reduce"] for r in res if r[0] == "fp32" and r[1] == "gather" and r[8] is not None} == {0, 1, 2}
    assert {r[8]["reduce"] for r in res if r[0] == "bf16" and r[1] == "gather" and r[8] is not None} == {0, 1}
    # every weight-gradient route, the two-tap merge in both directions, scalar path and both addressing forms
    for fam, routes in (("fp32", {0, 1, 2, 4}), ("bf16", {0, 1, 3, 4})):
        got = [r[8] for r in res if r[0] == fam and r[1] == "wgrad" and r[8] is not None]
        assert {d["route_id"] for d in got} == routes, fam
        assert {bool(d["fast"]) for d in got} == {False, True}, fam
    assert {r[8]["merge"] for r in res if r[0] == "bf16" and r[1] == "wgrad" and r[8] is not None} == {0, 1, 2}
    assert {r[8]["vec"] for r in res if r[0] == "fp32" and r[8] is not None} == {False, True}


def test_refusals_carry_the_librarys_text(shim):
    g = _same(4, 16, 16, 40, 64, 3)
    with pytest.raises(PC.PlanRefused, match=r"^conv plan: tile 13 \(LDS-DMA family\) needs the vector path, K channels % 32 == 0 \(Ck = 40\) and, with BN on load, tile 12, 14 or 15$"):
        decide(shim, "fwd", g, plan=(13, 0))
    with pytest.raises(PC.PlanRefused, match=r"^bf16 conv: K channels must be a multiple of 32 and N channels of 8 \(Ck = 40, Cn = 64\)$"):
        decide(shim, "fwd16", g)
    with pytest.raises(PC.PlanRefused, match=r"^conv plan: split 3 needs 786432 workspace bytes \(have 65536\)$"):
        decide(shim, "fwd", _same(4, 16, 16, 64, 64, 3), plan=(2, 3), ws_bytes=2 * PC.WS_COUNTER_BYTES)
    with pytest.raises(PC.PlanRefused, match=r"^wgrad plan: tile 5 \(128x128 on LDS-DMA\) needs more than 64 channels on both sides \(64, 128\)$"):
        decide(shim, "wgrad", _k4s2(4, 8, 64, 128, False), plan=(5, 0))
    with pytest.raises(PC.PlanRefused, match=r"^bf16 wgrad: tensors must be 16-byte aligned and smaller than 2 GiB$"):
        decide(shim, "wgrad16", _k4s2(4, 8, 64, 128, False), aligned=False)
