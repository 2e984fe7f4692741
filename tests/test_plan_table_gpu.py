"""Every committed launch plan at kernel level, on its own layer geometry (ops.PLAN_TABLE_PATH: mimic_amd/plans_gfx950.json, or
the candidate table MOPOE_PLAN_TABLE names): the (tile, split) plans bench.py and a training run launch for c1, c2, c3, c5 and
c2d128, each forced with ops.force_plan on ops.conv_fwd / conv_dgrad / conv_wgrad in the form its key names, at the layer's
own maps, channels, kernel, stride and padding with the batch reduced by tests/plan_cases.py: reduced_batch (the CPU file
asserts that the reduction keeps the launch on its path), and compared ON THE DEVICE, element by element, with the fp64
evaluation of tests/torch_backend.py on the same fp32 (or bf16-rounded) operands.

One test per (storage family, layer shape); the cases of a shape share x, w, dy and the fp64 convolutions.  Besides the
table's entries: the remapped plan of every fp32 entry the F32_SPLIT_BF16-off remap changes, the opposite-mask form that
ops._table_plan serves from every forward entry, and the Bn mode 3 form of the input gradients that have one (conv2 behind a
streamed block front).  `None` entries run on the library's static heuristic (plan = NULL).

Gates: the existing ones (plan_cases.bars, fp32_claim).  Per case also: the conv workspace beyond its 64 KiB of arrival
counters is NaN before the launch and the counters are all zero after it; every result is finite; out_stats / bwd_sums start
non-zero and have grown by the reference's sums.  Every tensor is owned and every plan is one the library validates: nothing
can fault; a case the library refuses fails its test by name.  Each case logs its relative L2 and worst error / bound ratio to
the per-kernel parity log (the one test_hip_ops_gpu._log appends to).
"""
import pytest
import torch

import plan_cases as PC
from mimic_amd import ops
from test_hip_ops_gpu import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES, LEFT_OUT = PC.all_cases()
PC.share_batches(CASES)
GROUPS = PC.groups(CASES)
EXERCISED = {}              # group -> table keys whose cases ran (and how many cases) in this session


@pytest.fixture(autouse=True)
def _static_heuristic_unless_forced(monkeypatch):
    """plan = NULL for the table's `None` entries whatever MOPOE_AUTOTUNE says: no tuner, no table lookup, no cached plan"""
    monkeypatch.setattr(ops, "AUTOTUNE", False)
    monkeypatch.setattr(ops, "TABLE_ONLY", False)
    ops.clear_plans()
    yield
    ops.clear_plans()


def _poison_scratch():
    ws, n = ops._workspace(torch.device(DEV, torch.cuda.current_device()))
    ws[ops.WS_COUNTER_BYTES:ops.WS_COUNTER_BYTES + (n - ops.WS_COUNTER_BYTES) // 4 * 4].view(torch.float32).fill_(float("nan"))
    return ws


def test_the_parametrisation_is_the_whole_table():
    assert LEFT_OUT == [], f"cases the library refuses: {LEFT_OUT[:5]}"
    keys = set(PC.table_keys())
    assert {k for byn in GROUPS.values() for cs in byn.values() for c in cs if c.variant == "table" for k in c.covers} == keys
    assert sum(len(cs) for byn in GROUPS.values() for cs in byn.values()) == len(CASES)


@pytest.mark.parametrize("group", sorted(GROUPS), ids=lambda k: f"{k[0]}-" + "x".join(map(str, k[1])))
def test_committed_plans_of_a_layer_shape(group):
    failures, ran = [], []
    for n, cs in sorted(GROUPS[group].items()):
        b = PC.Bundle(group[0] == "bf16", cs[0].g, DEV)
        for c in cs:
            h = PC.case_inputs(c, b)
            ref = PC.reference(c, b, h)
            ws = _poison_scratch()
            try:
                if c.plan is None:
                    got = PC.run_case(c, b, h, ops)
                else:
                    with ops.force_plan(*c.plan):
                        got = PC.run_case(c, b, h, ops)
            except ops.MopoeHipError as e:        # a stale entry: the library no longer takes this plan here
                failures.append(f"{c.id} (N' = {c.g.N}, plan {c.plan}): refused: {e}")
                _log(f"plan_table/{c.id}: N'={c.g.N} plan={c.plan} REFUSED {e}")
                continue
            torch.cuda.synchronize()
            if bool(ws[:ops.WS_COUNTER_BYTES].any()):
                failures.append(f"{c.id}: arrival counters of the conv workspace left non-zero")
                ws[:ops.WS_COUNTER_BYTES].zero_()
            _worst, _l2, fails = PC.compare(c, got, ref, log=_log)
            failures += [f"{c.id} (N' = {c.g.N}, plan {c.plan}): {f}" for f in fails]
            ran.append(c)
    EXERCISED[group] = ran
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:20])


# ---- last: it reads what the tests above recorded ------------------------------------------------------------------------------
def test_the_table_keys_exercised_are_the_table_keys():
    """the set of table keys exercised equals the set of table keys, and the number of cases run the number of cases.  Shapes
    whose test did not run in this session (a -k selection) are not judged; a full run of the file judges the whole table"""
    assert EXERCISED, "no shape of the table ran"
    want = {k for grp in EXERCISED for cs in GROUPS[grp].values() for c in cs for k in c.covers}
    got = {k for ran in EXERCISED.values() for c in ran for k in c.covers}
    n_want = sum(len(cs) for grp in EXERCISED for cs in GROUPS[grp].values())
    n_got = sum(len(ran) for ran in EXERCISED.values())
    _log(f"plan_table: {len(EXERCISED)} of {len(GROUPS)} shapes ran, {n_got} of {n_want} of their cases, {len(got)} of {len(PC.table_keys())} table keys")
    assert got == want and n_got == n_want, (sorted(want - got)[:5], n_got, n_want)
    if len(EXERCISED) == len(GROUPS):
        assert got == set(PC.table_keys()) and n_got == len(CASES)
