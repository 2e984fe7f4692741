"""trunk.py on the HIP kernels: two-block chains of every kind of residual block, in the three modes and on every A/B route, held
element by element to oracle/mopoe_ref._resblock chained under autograd in fp64 (tests/trunk_cases.py).

fp32 family: output, input gradient, every parameter gradient and the running statistics within K x the oracle's own
fp32-vs-fp64 deviation on that tensor (nothing excluded: the seeds keep every ReLU input of the reference 5e-5 from zero), the
stored ReLU patterns equal to the reference's, the launches the route is named after seen by a recorder, every gradient a view
into the BackwardArena.  bf16 family: per-tensor norms against the bf16-mode oracle and the fp64 truth.

K and the bf16 cap are twice the worst figure measured on one MI355X, rounded up (DESIGN.md section 8 holds the table; every run
appends its figures, one line per tensor, to the parity log of tests/test_hip_ops_gpu.py)."""
import pytest
import torch

import trunk_cases as TC
from test_hip_ops_gpu import _log as _parity_log

pytestmark = pytest.mark.gpu

K = 10.0              # error / the oracle's fp32 deviation, per tensor: twice the worst measured (4.51), rounded up
BF16_CAP = 5e-2       # rel-L2 against the bf16-mode oracle, per tensor: twice the worst measured (2.46e-2), rounded up

# whatever K is, no bar reaches the per-kernel bars of tests/test_hip_ops_gpu.py::check (2e-4 of the scale for tensors, 5e-4 for
# weight gradients, 1e-4 for statistics): the oracle's deviation is at most DEV_MAX in a case that runs at all
assert K <= 32 and K * TC.DEV_MAX <= 1e-4
assert BF16_CAP <= TC.BF16_CAP_MAX


def _log(line):
    _parity_log("trunk_chain " + line)


def _assert_lanes(rec, route):
    """the side-stream lanes: weight gradients (lane 0) and the shortcut branch (lane 1) leave the main stream unless switched off"""
    main = rec.streams("block_out_bwd")
    assert len(main) == 1
    every = set().union(*(rec.streams(n) for n in TC.RECORDED))
    if route == "nolanes":
        assert every == main, "a launch left the main stream with the lanes off"
    else:
        assert rec.streams("conv_wgrad").isdisjoint(main), "weight gradients ran on the main stream"
        assert len(rec.streams("conv_fwd")) == 2 and len(rec.streams("conv_dgrad")) == 2, "the shortcut branch ran on the main stream"


@pytest.mark.parametrize("case,mode,route", TC.all_params())
def test_chain_fp32(case, mode, route, monkeypatch):
    ref = TC.reference(case, mode)
    TC.assert_margin(ref)
    TC.set_route(monkeypatch, route)
    rec = TC.Recorder(monkeypatch)
    run = TC.run_trunk(ref.built, mode, "cuda", masks=ref.r64.masks)
    TC.assert_route(rec, ref.built.case, mode, route)
    _assert_lanes(rec, route)
    TC.assert_host_state(run, mode)
    assert TC.assert_relu_patterns(run, ref.r64) == (0 if route == "mat0" else 2)
    assert set(run.tensors) == set(ref.r64.tensors), set(run.tensors) ^ set(ref.r64.tensors)
    bad, worst = {}, (0.0, None)
    for name in sorted(ref.r64.tensors):
        err = TC.error(name, run.tensors[name], ref.r64.tensors)
        ratio = err / ref.dev[name]
        _log(f"fp32 {case} {mode} {route} {name}: hip_error={err:.3e} oracle_fp32_deviation={ref.dev[name]:.3e} ratio={ratio:.2f}")
        worst = max(worst, (ratio, name))
        if ratio > K:
            bad[name] = (err, ref.dev[name])
    _log(f"fp32 {case} {mode} {route} WORST ratio={worst[0]:.2f} ({worst[1]})")
    print(f"worst hip_error / oracle_fp32_deviation: {worst[0]:.2f} ({worst[1]})")
    assert not bad, f"{case} {mode} {route}: (error, oracle fp32 deviation) {bad}"


@pytest.mark.parametrize("case", TC.BF16_CASES)
@pytest.mark.parametrize("mode", TC.MODES)
def test_chain_bf16(case, mode, monkeypatch):
    ref = TC.reference_bf16(case, mode)
    rec = TC.Recorder(monkeypatch)
    run = TC.run_trunk(ref.built, mode, "cuda", masks=ref.truth.masks, bf16=True, x=ref.x, gout=ref.gout)
    TC.assert_route(rec, ref.built.case, mode, "default", bf16=True)
    if ref.built.case.chans[0] == 64:
        # the streamed forward front ran (d1 never written) and conv2's input gradient read the stored activation (Bn mode 3)
        nf = len(ref.built.case.fronts[TC.MODES.index(mode)])
        assert nf >= 1 and rec.count("block_front_apply") == nf and rec.count("conv_dgrad", bn_mode=3) == nf
        assert sum(1 for sv in run.saved if sv["d1"] is None) == nf
    _assert_lanes(rec, "default")
    TC.assert_host_state(run, mode)
    assert run.tensors["out"].dtype == torch.bfloat16 and run.tensors["dx"].dtype == torch.bfloat16
    fig = TC.bf16_figures(run, ref)
    for name, (r16, e_hip, e_orc) in sorted(fig.items()):
        _log(f"bf16 {case} {mode} {name}: rel_l2_vs_bf16_oracle={r16:.3e} to_fp64={e_hip:.3e} oracle_to_fp64={e_orc:.3e}")
    worst = max(fig.items(), key=lambda kv: kv[1][0])
    _log(f"bf16 {case} {mode} WORST rel_l2={worst[1][0]:.3e} ({worst[0]})")
    print(f"worst rel-L2 against the bf16-mode oracle: {worst[1][0]:.3e} ({worst[0]})")
    TC.assert_bf16(run, ref, BF16_CAP, f"{case} {mode}")
