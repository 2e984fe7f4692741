"""trunk.py's chain rule on the CPU: trunk_forward / trunk_backward / apply_running_updates drive the EMULATED ops
(tests/torch_backend.py) through two-block chains and every tensor they produce is compared, element by element, with
oracle/mopoe_ref._resblock chained under autograd in fp64 (tests/trunk_cases.py).  Emulation and oracle are both CPU fp32
arithmetic, so the bar of a tensor is 8 x the oracle's own fp32-vs-fp64 deviation on it.

Measured (this file, all 48 chains): worst error / deviation 4.74 (ragged, train, default route, chain.0.0.bn2.weight; every
other case stays below 3.6); the bf16 emulation's worst rel-L2 against the bf16-mode oracle 2.46e-2 (dec2d, train_nodrop,
chain.0.0.upsample.0.bias).  Nothing disagreed beyond the bar once the seeds also had to keep the fp32 oracle itself within
DEV_MAX of fp64: a first seed of rows48 ended on a 3-row BatchNorm with a channel of variance 2e-3, where the oracle strayed 2.6e-6
and the emulation 1.9e-5 -- one rounding error times 1 / sigma, drawn once by each (tests/trunk_cases.py: DEV_MAX)."""
import pytest
import torch

import torch_backend as TB
import trunk_cases as TC

CPU_K = 8.0


@pytest.mark.parametrize("case", [c.name for c in TC.CASES])
@pytest.mark.parametrize("mode", TC.MODES)
def test_margin(case, mode):
    """every ReLU input of the fp64 reference keeps M = 5e-5 from zero: asserted from the reference alone"""
    ref = TC.reference(case, mode)
    TC.assert_margin(ref)
    # the fp32 oracle then has the fp64 run's ReLU masks, element for element
    for a, b in zip(ref.r32.relu_in, ref.r64.relu_in):
        assert torch.equal(a > 0, b > 0)


@pytest.mark.parametrize("case,mode,route", TC.all_params())
def test_chain_emulated(case, mode, route, monkeypatch):
    ref = TC.reference(case, mode)
    TC.assert_margin(ref)
    TB.install(monkeypatch)
    TC.set_route(monkeypatch, route)
    rec = TC.Recorder(monkeypatch)
    run = TC.run_trunk(ref.built, mode, "cpu", masks=ref.r64.masks)
    TC.assert_route(rec, ref.built.case, mode, route)
    TC.assert_host_state(run, mode)
    assert TC.assert_relu_patterns(run, ref.r64) == (0 if route == "mat0" else 2)
    assert set(run.tensors) == set(ref.r64.tensors), set(run.tensors) ^ set(ref.r64.tensors)
    bad, worst = {}, (0.0, None)
    for name in sorted(ref.r64.tensors):
        err = TC.error(name, run.tensors[name], ref.r64.tensors)
        worst = max(worst, (err / ref.dev[name], name))
        if err > CPU_K * ref.dev[name]:
            bad[name] = (err, ref.dev[name])
    print(f"worst error / oracle_fp32_deviation: {worst[0]:.2f} ({worst[1]})")
    assert not bad, f"{case} {mode} {route}: (error, oracle fp32 deviation) {bad}"


@pytest.mark.parametrize("case", TC.BF16_CASES)
@pytest.mark.parametrize("mode", TC.MODES)
def test_chain_emulated_bf16(case, mode, monkeypatch):
    """the bf16 family's chain on the emulation (its rounding points are the kernels'): the gates of the GPU test"""
    ref = TC.reference_bf16(case, mode)
    TB.install(monkeypatch)
    rec = TC.Recorder(monkeypatch)
    run = TC.run_trunk(ref.built, mode, "cpu", masks=ref.truth.masks, bf16=True, x=ref.x, gout=ref.gout)
    TC.assert_route(rec, ref.built.case, mode, "default", bf16=True)
    TC.assert_host_state(run, mode)
    fig = TC.assert_bf16(run, ref, TC.BF16_CAP_MAX, f"{case} {mode}")
    worst = max(fig.items(), key=lambda kv: kv[1][0])
    print(f"bf16 {case} {mode}: worst rel-L2 {worst[1][0]:.3e} ({worst[0]})")
