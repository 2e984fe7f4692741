"""--max_grad_norm on the host: the restatement of the clip kernels (tests/torch_backend_clip.py) under optim.HipAdam against
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam evaluated in fp64, the two documented differences from torch, the flag
through parse_flags / default_flags / check_flags / set_optimizer, the scalar pack and the launcher's result line, and the
header of the clip entry points against the library and against the GPU file's guard-band table."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import mopoe_ref as R
import torch_backend_clip as TBC
from model_util import build_exp
from mimic_amd import run_epochs as RE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7,), (3, 5, 4), (1,), (130, 33), (2, 2), (4097,)]
LR, EPS = 3e-3, 1e-3      # (eps far above Adam's default: m / (sqrt(v) + eps) is scale-invariant in g up to eps, and the
#                            comparison has to see the scale in the parameters, not only in the moments)


def _grads(gen, k):
    return [torch.randn(s, generator=gen) * (10.0 ** ((i % 3) - 1)) * (1.0 + k) for i, s in enumerate(SHAPES)]


def _run(monkeypatch, max_norm_of, steps):
    """HipAdam with the restated ops on fp32 tensors, and clip_grad_norm_ + optim.Adam on double copies, over the same
    gradients.  max_norm_of(norm of step 0) -> max_grad_norm.  -> (mine, ref, optimiser, norms torch returned)"""
    from mimic_amd.optim import HipAdam
    TBC.install(monkeypatch)
    gen = torch.Generator().manual_seed(11)
    mine = [torch.nn.Parameter(torch.randn(*s, generator=gen)) for s in SHAPES]
    ref = [torch.nn.Parameter(p.detach().double().clone()) for p in mine]
    grads = [_grads(gen, k) for k in range(steps)]
    norm0 = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads[0]))
    max_norm = max_norm_of(norm0)
    opt = HipAdam(mine, lr=LR, betas=(0.9, 0.999), eps=EPS, max_grad_norm=max_norm)
    opt_ref = torch.optim.Adam(ref, lr=LR, betas=(0.9, 0.999), eps=EPS)
    norms, states = [], []
    for gs in grads:
        for a, b, g in zip(mine, ref, gs):
            a.grad, b.grad = g.clone(), g.double().clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_(ref, max_norm, norm_type=2)))
        opt_ref.step()
        opt.step()
        states.append(opt.clip_state.clone())
        for a, g in zip(mine, gs):
            assert torch.equal(a.grad, g)                      # difference 1: p.grad is not rewritten
    return mine, ref, opt, opt_ref, norms, states, max_norm


def _agree(mine, ref, opt, opt_ref, steps):
    """fp32 against fp64.  Parameters: `steps` roundings of p (2^-24 |p| each) + the update, at most a few lr per step, whose
    fp32 evaluation (two moments rounded to float, sqrt, one division) is good to ~1e-6 relative of lr: 1e-5 lr allowed.
    Moments: a few float roundings per step on values that do not cancel below the gradients' own size."""
    for a, b in zip(mine, ref):
        tol = steps * 2.0 ** -24 * float(a.detach().abs().max()) + 1e-5 * LR * steps
        assert float((a.detach().double() - b.detach()).abs().max()) <= tol, (a.shape, tol)
        for key in ("exp_avg", "exp_avg_sq"):
            x, y = opt.state[a][key].double(), opt_ref.state[b][key]
            assert float((x - y).abs().max()) <= 1e-6 * float(y.abs().max()), (a.shape, key)


def test_norm_below_max_norm_is_plain_adam(monkeypatch):
    mine, ref, opt, opt_ref, norms, states, max_norm = _run(monkeypatch, lambda n: 2.0 * n, 1)
    _agree(mine, ref, opt, opt_ref, 1)
    st = states[0]
    assert float(st[1]) == 1.0 and float(st[2]) == 0.0 and float(st[3]) == 0.0
    assert abs(float(st[0]) - norms[0]) <= 2.0 ** -23 * norms[0]
    assert float(opt._step) == 1


def test_norm_above_max_norm_scales_the_update(monkeypatch):
    mine, ref, opt, opt_ref, norms, states, max_norm = _run(monkeypatch, lambda n: 0.25 * n, 1)
    _agree(mine, ref, opt, opt_ref, 1)
    st = states[0]
    want = max_norm / (norms[0] + 1e-6)
    assert abs(float(st[1]) - want) <= 2.0 ** -23 * want and 0.24 < float(st[1]) < 0.26
    assert abs(float(st[0]) - norms[0]) <= 2.0 ** -23 * norms[0]              # the norm BEFORE clipping, as torch returns it
    # the same gradients without clipping (a bound four times the norm) lead somewhere else
    unclipped = _run(monkeypatch, lambda n: 4.0 * n, 1)
    d = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(mine, unclipped[0]))
    assert d > 100 * 1e-5 * LR, d                              # far outside the agreement bound: clipping is visible


def test_three_step_sequence(monkeypatch):
    """the gradients grow from step to step (x1, x2, x3): with max_norm = 1.5 x the first norm, step 0 is not clipped and
    steps 1 and 2 are, each by its own scale"""
    mine, ref, opt, opt_ref, norms, states, max_norm = _run(monkeypatch, lambda n: 1.5 * n, 3)
    _agree(mine, ref, opt, opt_ref, 3)
    scales = [float(s[1]) for s in states]
    assert scales[0] == 1.0 and 0.7 < scales[1] < 0.8 and 0.45 < scales[2] < 0.55, scales
    for s, n in zip(states, norms):
        assert abs(float(s[0]) - n) <= 2.0 ** -23 * n
    assert float(opt._step) == 3 and float(states[-1][3]) == 0.0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_norm_skips_the_step(monkeypatch, bad):
    """difference 2: nothing changes, the skip counter goes up, and the next finite step is step number 2"""
    from mimic_amd.optim import HipAdam
    TBC.install(monkeypatch)
    gen = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=gen)) for s in SHAPES]
    opt = HipAdam(ps, lr=LR, max_grad_norm=1.0)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen)
    opt.step()
    snap = [p.detach().clone() for p in ps] + [opt._moments.clone(), opt._step.clone(), opt._coef.clone()]
    for k in (1, 2):
        ps[3].grad[5, 7] = bad
        opt.step()
        now = [p.detach() for p in ps] + [opt._moments, opt._step, opt._coef]
        assert all(torch.equal(a, b) for a, b in zip(snap, now))
        assert float(opt.clip_state[2]) == 1.0 and float(opt.clip_state[3]) == k and float(opt.clip_state[1]) == 0.0
    ps[3].grad[5, 7] = 0.5
    opt.step()
    assert float(opt._step) == 2 and float(opt.clip_state[2]) == 0.0 and float(opt.clip_state[3]) == 2.0
    assert all(not torch.equal(a, b.detach()) for a, b in zip(snap[:len(ps)], ps))


def test_hip_adam_arguments(monkeypatch):
    from mimic_amd.optim import HipAdam
    TBC.install(monkeypatch)
    ps = [torch.nn.Parameter(torch.zeros(5000)), torch.nn.Parameter(torch.zeros(3))]
    off = HipAdam(ps)
    assert off.max_grad_norm == 0.0 and off.clip_state is None and off._clip_scratch is None
    assert "max_grad_norm" not in off.state_dict()["param_groups"][0]           # the unclipped optimiser's state_dict is today's
    on = HipAdam(ps, max_grad_norm=2.5)
    assert on.max_grad_norm == 2.5 and tuple(on.clip_state.shape) == (4,) and on.clip_state.dtype == torch.float32
    assert on._clip_scratch.dtype == torch.float64 and on._clip_scratch.numel() == 3      # 2 chunks + 1
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            HipAdam(ps, max_grad_norm=bad)
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        on.early_begin()


# ---- flags ---------------------------------------------------------------------------------------------------------------------
def test_flag_parsing_and_defaults(monkeypatch):
    from mimic_amd import main_mimic as MM
    from mimic_amd.utils.experiment import check_flags, default_flags
    monkeypatch.delenv("MOPOE_TORCH_ADAM", raising=False)
    assert default_flags(device=None).max_grad_norm == 0.0
    assert MM.parse_flags([]).max_grad_norm == 0.0
    f = MM.parse_flags(["--max_grad_norm", "1.5"])
    assert f.max_grad_norm == 1.5 and isinstance(f.max_grad_norm, float)
    check_flags(f)
    for bad in (-0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            check_flags(default_flags(device=None, max_grad_norm=bad))
    with pytest.raises(ValueError, match="max_grad_norm"):
        MM.Main(MM.parse_flags(["--max_grad_norm", "-1"]))
    monkeypatch.setenv("MOPOE_TORCH_ADAM", "1")
    check_flags(default_flags(device=None))                                # the switch alone stays allowed
    with pytest.raises(ValueError, match=r"(?s)max_grad_norm.*MOPOE_TORCH_ADAM"):
        check_flags(default_flags(device=None, max_grad_norm=1.0))


def _tiny_exp(monkeypatch, **flag_overrides):
    TBC.install(monkeypatch)
    cfg = R.Cfg(img_size=64, class_dim=8, DIM_img=4, DIM_text=4, vocab_size=50, batch_size=4)
    sd = R.init_state(cfg, seed=2)
    batch, eps = R.synthetic_batch(cfg, 4, seed=3)
    exp = build_exp(cfg, sd, "cpu", "train_nodrop", eps=eps)
    for k, v in flag_overrides.items():
        setattr(exp.flags, k, v)
    return exp, batch


def _hip_adam(exp):
    exp.set_hip_adam(list(exp.mm_vae.parameters()), exp.flags.initial_learning_rate, (0.9, 0.999), [])
    return exp.optimizer


def test_the_default_experiment_does_not_clip(monkeypatch):
    from mimic_amd import nets
    from mimic_amd.optim import HipAdam
    monkeypatch.delenv("MOPOE_TORCH_ADAM", raising=False)
    exp, batch = _tiny_exp(monkeypatch)
    assert exp.flags.max_grad_norm == 0.0
    opt = _hip_adam(exp)
    assert isinstance(opt, HipAdam) and opt.max_grad_norm == 0.0 and opt.clip_state is None
    pack = RE.ScalarPack(exp.flags.device)
    armed = []
    real_begin = opt.early_begin
    monkeypatch.setattr(opt, "early_begin", lambda: (armed.append(nets.EARLY_STEP[0]), real_begin())[1])
    RE.train_step(exp, (dict(batch), None), None, pack)
    assert len(armed) == 1                                      # the per-network early updates are still what runs by default
    names = list(pack.read())
    assert len(names) == 18 and "grad_norm" not in names and "skipped_steps" not in names
    # parameters on the CPU: set_optimizer falls back to PyTorch's Adam, which would train without the clip -> refused
    exp.flags.max_grad_norm = 1.0
    with pytest.raises(ValueError, match="max_grad_norm"):
        exp.set_optimizer()
    monkeypatch.setenv("MOPOE_TORCH_ADAM", "1")
    with pytest.raises(ValueError, match=r"(?s)max_grad_norm.*MOPOE_TORCH_ADAM"):
        exp.set_optimizer()


def test_a_clipping_experiment_on_the_host(monkeypatch):
    """exp.set_hip_adam passes the flag on; train_step does not arm the early updates; the pack carries the two names, and
    grad_norm is the fp64 norm of p.grad"""
    from mimic_amd import nets
    monkeypatch.delenv("MOPOE_TORCH_ADAM", raising=False)
    exp, batch = _tiny_exp(monkeypatch, max_grad_norm=0.75)
    opt = _hip_adam(exp)
    assert opt.max_grad_norm == 0.75 and opt.clip_state is not None
    seen = []
    real_step = opt.step
    monkeypatch.setattr(opt, "step", lambda: (seen.append(nets.EARLY_STEP[0]), real_step())[1])
    monkeypatch.setattr(opt, "early_step", lambda *a, **k: pytest.fail("early_step under max_grad_norm"))
    pack = RE.ScalarPack(exp.flags.device)
    RE.train_step(exp, (dict(batch), None), None, pack)
    assert seen == [None] and nets.EARLY_STEP[0] is None
    got = pack.read()
    assert list(got)[-2:] == ["grad_norm", "skipped_steps"] and len(got) == 20
    norm = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in exp.mm_vae.parameters() if p.grad is not None))
    assert abs(got["grad_norm"] - norm) <= 2.0 ** -23 * norm and got["skipped_steps"] == 0.0
    assert norm > 0.75 and float(opt.clip_state[1]) < 1.0       # (this model's first gradients are far above the bound)


def test_result_line_with_and_without_clipping():
    from mimic_amd import main_mimic as MM
    h = lambda last: {"epoch": 0, "train": {"graphed_steps": 3, "last": last}, "test": {"total_loss": 1.5}}
    assert MM.result_line([h({"total_loss": 2.0})]) == {"epochs": 1, "last_test_loss": 1.5, "graphed_steps_last_epoch": 3}
    line = MM.result_line([h({"total_loss": 2.0, "grad_norm": 7.25, "skipped_steps": 2.0})])
    assert line["last_grad_norm"] == 7.25 and line["skipped_steps"] == 2 and isinstance(line["skipped_steps"], int)


# ---- the header of the clip entry points against the library and the GPU file's table ---------------------------------------------
def _declared(header):
    text = open(os.path.join(REPO, "include", header)).read()
    return set(re.findall(r"\b(mopoe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_every_clip_entry_point_is_exported_and_guarded():
    import test_grad_clip_gpu as G
    from mimic_amd import ops
    if not os.path.exists(ops.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    names = _declared("mopoe_hip_optim.h")
    assert names == {"mopoe_grad_norm_partials", "mopoe_grad_norm", "mopoe_adam_step_clipped"}
    lib = ctypes.CDLL(ops.LIB_PATH)
    for fn in names:
        assert hasattr(lib, fn), fn
    assert not names & _declared("mopoe_hip.h"), "the clip entry points live in their own header"
    # mopoe_grad_norm_partials is host arithmetic (it returns a size, like mopoe_conv_workspace_bytes): no guarded case
    assert set(G.GUARDED) == names - {"mopoe_grad_norm_partials"}
    for fn, test in G.GUARDED.items():
        assert callable(getattr(G, test, None)), (fn, test)
    lib.mopoe_abi_version.restype = ctypes.c_int
    assert lib.mopoe_abi_version() == ops.ABI_VERSION == 25
    # the size query needs no device: chunks of 4096 per record with n > 0, and the restatement agrees
    sizes = [1, 3, 4096, 4097, 0, 3 * 4096 + 1]
    assert ops.grad_norm_partials(sizes) == TBC.grad_norm_partials(sizes) == 1 + 1 + 1 + 2 + 0 + 4
    assert ops.grad_norm_partials([]) == 0
