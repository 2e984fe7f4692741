"""The committed launch-plan table (ops.PLAN_TABLE_PATH: mimic_amd/plans_gfx950.json, or the candidate table MOPOE_PLAN_TABLE
names) as far as it can be judged without a GPU -- the host side of tests/test_plan_table_gpu.py:

  * every plan is one today's candidate functions offer for its geometry and fusion at the library's workspace size (a plan
    they would not offer -- a 128 x 128 weight-gradient tile on a 64-channel layer -- fails here), the remapped plans with
    F32_SPLIT_BF16 off likewise;
  * the case list (tests/plan_cases.py) covers every entry, leaves none out, and its reduced batch keeps every launch on the
    path it has at the table's batch;
  * the fp64 reference the GPU file compares with is tests/torch_backend.py's own arithmetic, and torch_backend in fp32 stays
    within HALF of each GPU bar of it on these inputs (as tests/test_arena_cpu.py shows for the hostile sets), for every case
    under 0.2 G multiply-adds and at least one case of every (op, tile) pair.
"""
import ctypes

import pytest
import torch

import plan_cases as PC
import torch_backend as TB
from mimic_amd import ops

CASES, LEFT_OUT = PC.all_cases()
PC.share_batches(CASES)
N_CASES = len(CASES)          # tests/test_plan_table_gpu.py logs one line per case: the same number
CPU_MACS = 0.2e9


def _candidates(op, g, flags, split_bf16=True):
    prev = ops.F32_SPLIT_BF16
    ops.F32_SPLIT_BF16 = split_bf16
    try:
        kind = PC.kind_of(op)
        if kind == "wgrad":
            return ops._wgrad_candidates(g, bf16=PC.is16(op), plain_operand=not flags[0])
        plain = (not flags[0]) if kind == "fwd" else True
        fn = ops._gather_candidates_bf16 if PC.is16(op) else ops._gather_candidates
        return fn(kind, g, PC.WS_BYTES, plain_operand=plain)
    finally:
        ops.F32_SPLIT_BF16 = prev


def _not_offered(split_bf16):
    bad = []
    for key in PC.table_keys():
        op, g, fl = PC.parse_key(key)
        found, plan = PC.lookup(op, g, fl, split_bf16)
        assert found, key
        cands = _candidates(op, g, fl, split_bf16)
        if plan is None:
            if cands:
                bad.append((key, None, "the static heuristic on a layer that has candidates"))
        elif plan not in cands:
            bad.append((key, plan, sorted(cands)))
    return bad


def test_workspace_size_is_the_librarys():
    lib = ctypes.CDLL(ops.LIB_PATH)
    lib.mopoe_conv_workspace_bytes.restype = ctypes.c_size_t
    assert int(lib.mopoe_conv_workspace_bytes()) == PC.WS_BYTES


def test_every_committed_plan_is_one_the_candidate_functions_offer():
    assert len(PC.table_keys()) > 0
    bad = _not_offered(True)
    assert not bad, f"{len(bad)} entries hold a plan the tuner would not offer today: {bad[:5]}"


def test_every_remapped_plan_is_offered_with_the_bf16_pipe_switched_off():
    bad = _not_offered(False)
    assert not bad, f"{len(bad)} remapped plans the tuner would not offer with F32_SPLIT_BF16 off: {bad[:5]}"


def test_a_plan_the_candidate_functions_do_not_offer_is_found(monkeypatch):
    """a 128 x 128 weight-gradient tile on a 64-channel layer, put into a copy of the table in place of a real entry"""
    key = next(k for k in PC.table_keys() if k.startswith("wgrad|") and PC.parse_key(k)[1].Cin == 64 and PC.parse_key(k)[1].Cout > 1)
    monkeypatch.setitem(ops._plan_table, key, [5, 1])
    assert [b[0] for b in _not_offered(True)] == [key]
    op, g, fl = PC.parse_key(key)
    with pytest.raises(PC.PlanRefused):
        PC.wgrad_path(op, g, fl[0], (5, 1))


def test_the_case_list_covers_every_entry_and_leaves_none_out():
    assert LEFT_OUT == [], f"cases the library refuses: {LEFT_OUT[:5]}"
    keys = set(PC.table_keys())
    covered = {k for c in CASES if c.variant == "table" for k in c.covers}
    assert covered == keys, sorted(keys - covered)[:5]
    assert len({c.id for c in CASES}) == N_CASES
    # the fallback forms: one remapped case per fp32 entry the remap changes, one opposite-mask case per forward entry whose
    # opposite is not itself an entry
    for key in keys:
        op, g, fl = PC.parse_key(key)
        if not PC.is16(op) and PC.lookup(op, g, fl, False)[1] != PC.lookup(op, g, fl)[1]:
            assert any(key in c.covers and c.variant == "split_bf16_off" for c in CASES), key
        if PC.kind_of(op) == "fwd" and ops.plan_key_str((op, g) + fl[:1] + (not fl[1],) + fl[2:]) not in keys:
            assert any(key in c.covers and c.variant == "opposite_mask" for c in CASES), key


def test_the_reduced_batch_keeps_every_launch_on_its_path():
    bad = []
    for c in CASES:
        t, g = c.table_geom, c.g
        assert PC.shape_of(t) == PC.shape_of(g) and 1 <= g.N <= t.N, c.id
        full, red = c.path(t), c.path(g)
        why = [k for k in PC.PATH_KEYS if full.get(k) != red.get(k)]
        if g.N < t.N:
            if g.N < 2:
                why.append("N' < 2")
            if g.N * g.Hs * g.Ws < PC.MIN_ROWS:
                why.append("fewer than 1025 output rows")
        if full["route"] == "four_tap":       # four-tap eligibility and the library's clamp of the pixel-tile split
            if not PC._four_tap_geom(g) or g.N * (g.Hs // 8) * (g.Ws // 8) < red["split"]:
                why.append("four-tap form")
        if full.get("bm") == 256 and red["rows"] < 256:
            why.append("256-row tile on fewer than 256 rows")
        if c.kind != "wgrad" and c.plan is not None and full["route"] == "gemm" and red["nsplit"] != c.plan[1]:
            why.append(f"effective split {red['nsplit']}")
        if why:
            bad.append((c.id, g.N, why))
    assert not bad, f"{len(bad)} cases leave their path: {bad[:5]}"


def test_weight_gradient_splits_are_the_tables_after_the_librarys_clamp():
    """the pixel split a weight-gradient plan asks for passes the library's clamp (max_split) at the reduced batch wherever it
    passes it at the table's; what remains different from the request is the chunk rounding (a chunk is a whole number of
    16 / 32 / 64-pixel stages), the same at both batches"""
    for c in CASES:
        if c.kind != "wgrad" or c.plan is None:
            continue
        full, red = c.path(c.table_geom), c.path(c.g)
        assert red["split"] == full["split"] and 1 <= red["split"] <= c.plan[1], (c.id, red["split"], full["split"])


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _small(c):
    return c.macs < CPU_MACS


def _cpu_selection():
    chosen = {c.id for c in CASES if _small(c)}
    by_pair = {}
    for c in CASES:
        by_pair.setdefault((c.op, None if c.plan is None else c.plan[0]), []).append(c)
    for pair, cs in by_pair.items():
        if not any(c.id in chosen for c in cs):
            chosen.add(min(cs, key=lambda c: c.macs).id)
    return chosen


CPU_IDS = _cpu_selection()
CPU_GROUPS = {k: {n: [c for c in cs if c.id in CPU_IDS] for n, cs in byn.items()} for k, byn in PC.groups(CASES).items()}
CPU_GROUPS = {k: {n: cs for n, cs in byn.items() if cs} for k, byn in CPU_GROUPS.items()}
CPU_GROUPS = {k: v for k, v in CPU_GROUPS.items() if v}


def test_the_cpu_selection_has_every_op_and_tile():
    pairs = {(c.op, None if c.plan is None else c.plan[0]) for c in CASES}
    assert {(c.op, None if c.plan is None else c.plan[0]) for c in CASES if c.id in CPU_IDS} == pairs
    assert all(c.id in CPU_IDS for c in CASES if _small(c))


def _full_torch_backend(c, b, h):
    """tests/torch_backend.py itself in fp64 on the case's operands (fp32 family)"""
    d = torch.float64
    g = b.g
    bn64 = b.bn
    if c.kind == "fwd":
        st = h["stats0"].clone() if c.stats else None
        y = TB.conv_fwd(b.x.to(d), b.w.to(d), g, bn_in=bn64 if c.bn else None, bias=h.get("bias"), mask=h.get("mask"), out_stats=st,
                        mix=(h["s"].to(d), h["bns"], PC.MIX_A, PC.MIX_B) if c.mix else None)
        return dict(y=y, stats=st) if c.stats else dict(y=y)
    if c.kind == "dgrad":
        sm = h["sums0"].clone() if c.bn else None
        dx = TB.conv_dgrad(b.dy.to(d), b.w.to(d), g, relu_bn=h.get("relu_bn"), xin=None if not c.bn else h["xin"].to(d), bwd_sums=sm)
        return dict(dx=dx, sums=sm) if c.bn else dict(dx=dx)
    return dict(dw=TB.conv_wgrad(b.x.to(d), b.dy.to(d), g, bn_in=bn64 if c.bn else None))


@pytest.mark.parametrize("group", sorted(CPU_GROUPS), ids=lambda k: f"{k[0]}-" + "x".join(map(str, k[1])))
def test_fp32_reference_within_half_of_each_bar(group):
    """torch_backend in fp32 (the reference of the per-kernel tests) against the fp64 evaluation the GPU file compares with, at
    half of every bar (results stored in bf16: at their bar -- plan_cases.compare); for the fp32 family the fp64 reference,
    which shares one convolution among the cases of a shape and restates the epilogue, is also held equal to torch_backend's
    own fp64 result"""
    for n, cs in CPU_GROUPS[group].items():
        b = PC.Bundle(group[0] == "bf16", cs[0].g, "cpu")
        for c in cs:
            assert c.g == b.g
            h = PC.case_inputs(c, b)
            ref = PC.reference(c, b, h)
            if not c.f16:
                own = _full_torch_backend(c, b, h)
                for name, t in own.items():
                    assert t.dtype == torch.float64
                    torch.testing.assert_close(ref[name], t, rtol=1e-12, atol=1e-12 * max(1.0, float(t.abs().max())), msg=lambda m: f"{c.id}/{name}: {m}")
            got = PC.run_case(c, b, h, TB)
            _w, _l2, fails = PC.compare(c, got, ref, bar_scale=0.5, claim=False)
            assert not fails, (c.id, fails)
