"""--ema_decay on the host: the header of the two EMA entry points against the library and against the GPU file's guard-band
table, the flag through parse_flags / default_flags / check_flags / Main / set_optimizer, the launcher's result line, and
optim.HipAdam driven on the restatement of the kernels (tests/torch_backend_ema.py): where the update is issued, what
withholds it, the swap and its guard, exp.averaged_weights(), and the decay rule against hand values."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import mopoe_ref as R
import torch_backend_ema as TBE
from model_util import build_exp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7,), (3, 5, 4), (1,), (130, 33), (2, 2), (4097,)]
NO_GRAD = 4              # the tensor of SHAPES that never receives a gradient
LR = 3e-3


# ---- the header against the library and the GPU file's table --------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(REPO, "include", header)).read()
    return set(re.findall(r"\b(mopoe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_every_ema_entry_point_is_exported_and_guarded():
    import test_ema_gpu as G
    from mimic_amd import ops
    if not os.path.exists(ops.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    names = _declared("mopoe_hip_ema.h")
    assert names == {"mopoe_ema_update", "mopoe_ema_swap"}
    lib = ctypes.CDLL(ops.LIB_PATH)
    for fn in names:
        assert hasattr(lib, fn), fn
    for other in ("mopoe_hip.h", "mopoe_hip_optim.h", "mopoe_hip_data.h"):
        assert not names & _declared(other), f"the EMA entry points live in their own header, not in {other}"
    assert set(G.GUARDED) == names
    for fn, test in G.GUARDED.items():
        assert callable(getattr(G, test, None)) and test.startswith("test_"), (fn, test)
    lib.mopoe_abi_version.restype = ctypes.c_int
    assert lib.mopoe_abi_version() == ops.ABI_VERSION == 25
    assert callable(ops.ema_update) and callable(ops.ema_swap)
    assert ctypes.sizeof(ops._EmaSeg) == 32           # mopoe_ema_seg: three pointers and an int64


# ---- flags -------------------------------------------------------------------------------------------------------------------
def test_flag_parsing_defaults_and_refusals(monkeypatch):
    from mimic_amd import main_mimic as MM
    from mimic_amd.utils.experiment import check_flags, default_flags
    monkeypatch.delenv("MOPOE_TORCH_ADAM", raising=False)
    assert default_flags(device=None).ema_decay == 0.0
    assert MM.parse_flags([]).ema_decay == 0.0
    f = MM.parse_flags(["--ema_decay", "0.999"])
    assert f.ema_decay == 0.999 and isinstance(f.ema_decay, float)
    check_flags(f)
    for bad in (-0.1, 1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            check_flags(default_flags(device=None, ema_decay=bad))
        with pytest.raises(ValueError, match="ema_decay"):            # in the launcher process, before any child starts
            MM.Main(MM.parse_flags(["--ema_decay", repr(bad)]))
    monkeypatch.setenv("MOPOE_TORCH_ADAM", "1")
    check_flags(default_flags(device=None))                            # the switch alone stays allowed
    with pytest.raises(ValueError, match=r"(?s)ema_decay.*MOPOE_TORCH_ADAM"):
        check_flags(default_flags(device=None, ema_decay=0.9))
    with pytest.raises(ValueError, match=r"(?s)ema_decay.*MOPOE_TORCH_ADAM"):
        MM.Main(MM.parse_flags(["--ema_decay", "0.9"]))


def _tiny_exp(monkeypatch, **flag_overrides):
    TBE.install(monkeypatch)
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


def test_set_optimizer_refuses_an_average_on_the_cpu(monkeypatch):
    """parameters on the CPU: set_optimizer falls back to PyTorch's Adam, which would train without the average -> refused"""
    monkeypatch.delenv("MOPOE_TORCH_ADAM", raising=False)
    exp, _ = _tiny_exp(monkeypatch)
    exp.set_optimizer()                                                # the default (decay 0) is PyTorch's Adam here, as before
    assert isinstance(exp.optimizer, torch.optim.Adam)
    with exp.averaged_weights() as on:                                 # ... and the context manager does nothing
        assert on is False
    exp.flags.ema_decay = 0.9
    with pytest.raises(ValueError, match="ema_decay"):
        exp.set_optimizer()
    monkeypatch.setenv("MOPOE_TORCH_ADAM", "1")
    with pytest.raises(ValueError, match=r"(?s)ema_decay.*MOPOE_TORCH_ADAM"):
        exp.set_optimizer()


def test_result_line_with_and_without_the_average():
    from mimic_amd import main_mimic as MM
    h = lambda test: {"epoch": 0, "train": {"graphed_steps": 3, "last": {"total_loss": 2.0}}, "test": test}
    assert MM.result_line([h({"total_loss": 1.5})]) == {"epochs": 1, "last_test_loss": 1.5, "graphed_steps_last_epoch": 3}
    line = MM.result_line([h({"total_loss": 1.5, "weights": "ema"})])
    assert line == {"epochs": 1, "last_test_loss": 1.5, "graphed_steps_last_epoch": 3, "eval_weights": "ema"}


# ---- the decay rule ----------------------------------------------------------------------------------------------------------
def test_decay_rule_against_hand_values(monkeypatch):
    # through the optimiser: one element, p pinned to 1 (lr 0), average 0 -> after the step at counter s the average is
    # w = float32(1 - d), d from the counter the optimiser itself advanced
    from mimic_amd.optim import HipAdam
    TBE.install(monkeypatch)
    for s, d in ((1, 2.0 / 11.0), (89, 90.0 / 99.0), (10 ** 6, 0.999)):
        p = torch.nn.Parameter(torch.ones(1))
        opt = HipAdam([p], lr=0.0, ema_decay=0.999)
        opt._step.fill_(float(s - 1))
        opt._ema_flat.zero_()
        p.grad = torch.ones(1)
        opt.step()
        assert float(opt._step) == s and float(p) == 1.0
        assert float(opt.ema_tensors()[0]) == float(np.float32(1.0 - d)), (s, float(opt.ema_tensors()[0]))
    assert TBE.decay_at(0.999, 1) == 2.0 / 11.0
    assert TBE.decay_at(0.999, 89) == 90.0 / 99.0
    assert TBE.decay_at(0.999, 10 ** 6) == 0.999
    assert TBE.decay_at(0.5, 1) == 2.0 / 11.0 and TBE.decay_at(0.5, 8) == 0.5 and TBE.decay_at(0.5, 9) == 0.5
    assert TBE.weight_at(0.999, 1) == float(np.float32(9.0 / 11.0))
    assert TBE.weight_at(0.999, 10 ** 6) == float(np.float32(1.0 - 0.999))
    # ... and through the op: one element, ema 0, p 1 -> ema = w
    for s, d in ((1, 2.0 / 11.0), (89, 90.0 / 99.0), (10 ** 6, 0.999)):
        p, e = torch.ones(1), torch.zeros(1)
        TBE.ema_update([p], [e], 0.999, torch.tensor(float(s)))
        assert float(e) == float(np.float32(1.0 - d)), (s, float(e))
    for bad in (1.0, -1e-3, float("nan"), float("inf")):
        from mimic_amd import ops
        with pytest.raises(ops.MopoeHipError, match="decay"):
            TBE.ema_update([torch.ones(1)], [torch.zeros(1)], bad, torch.tensor(1.0))


# ---- optim.HipAdam on the restatement ------------------------------------------------------------------------------------------
def _params(seed=11):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=gen)) for s in SHAPES], gen


def _set_grads(ps, gen):
    for i, p in enumerate(ps):
        p.grad = None if i == NO_GRAD else torch.randn(p.shape, generator=gen)


def _ref_step(ref, ps, decay, s):
    """the fp64 recurrence with w the float32 nearest to 1 - d"""
    w = TBE.weight_at(decay, s)
    return [r + w * (p.detach().double() - r) for r, p in zip(ref, ps)]


def test_hip_adam_arguments(monkeypatch):
    from mimic_amd.optim import HipAdam
    TBE.install(monkeypatch)
    ps, _ = _params()
    off = HipAdam(ps)
    assert off.ema_decay == 0.0 and off._ema is None and off._ema_flat is None
    assert "ema_decay" not in off.state_dict()["param_groups"][0]           # the optimiser's state_dict is today's
    for what in (off.swap_ema, off.ema_tensors, off.reset_ema):
        with pytest.raises(RuntimeError, match="ema_decay"):
            what()
    for bad in (-0.1, 1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            HipAdam(ps, ema_decay=bad)
    on = HipAdam(ps, ema_decay=0.9)
    assert on.ema_decay == 0.9 and on._ema_flat.shape == on._moments[0].shape and on._ema_flat.dtype == torch.float32
    assert "ema_decay" not in on.state_dict()["param_groups"][0]
    for e, m, p in zip(on.ema_tensors(), on._m, ps):                   # at the moments' offsets, initialised from the parameters
        assert e.shape == p.shape and torch.equal(e, p.detach())
        assert e.data_ptr() - on._ema_flat.data_ptr() == m.data_ptr() - on._moments.data_ptr()
    with torch.no_grad():
        ps[0].add_(1.0)
    assert not torch.equal(on.ema_tensors()[0], ps[0].detach())
    on.reset_ema()
    assert torch.equal(on.ema_tensors()[0], ps[0].detach())


def test_update_follows_each_adam_launch_for_tensors_with_a_gradient(monkeypatch):
    from mimic_amd.optim import HipAdam
    TBE.install(monkeypatch)
    ps, gen = _params()
    decay, steps = 0.9, 4
    opt = HipAdam(ps, lr=LR, ema_decay=decay)
    ref = [p.detach().double().clone() for p in ps]
    ptr = [p.data_ptr() for p in ps]
    biggest = [p.detach().abs().clone() for p in ps]
    for k in range(steps):
        _set_grads(ps, gen)
        del TBE.CALLS[:]
        opt.step()
        assert float(opt._step) == k + 1
        ref = _ref_step(ref, ps, decay, k + 1)
        biggest = [torch.maximum(b, torch.maximum(p.detach().abs(), e.abs())) for b, p, e in zip(biggest, ps, opt.ema_tensors())]
        # one Adam launch, one update right behind it, over the same tensors: those with a gradient, each once
        assert [c[0] for c in TBE.CALLS] == ["adam_step", "ema_update"]
        assert TBE.CALLS[0][1] == TBE.CALLS[1][1] == [q for i, q in enumerate(ptr) if i != NO_GRAD]
    for i, (e, r, b) in enumerate(zip(opt.ema_tensors(), ref, biggest)):
        if i == NO_GRAD:
            assert torch.equal(e, ps[i].detach())                      # never updated: the average is the parameter itself
            continue
        assert bool(((e.double() - r).abs() <= 4 * steps * 2.0 ** -24 * b.double()).all()), i
        assert not torch.equal(e, ps[i].detach())


def test_update_runs_with_the_early_per_network_launches(monkeypatch):
    """a step in parts: early_begin launches no update (no tensor), every early_step / held / final launch is followed by
    the update of exactly its tensors, and every tensor with a gradient is updated once per step"""
    from mimic_amd.optim import HipAdam
    TBE.install(monkeypatch)
    ps, gen = _params()
    opt = HipAdam(ps, lr=LR, ema_decay=0.9)
    ptr = [p.data_ptr() for p in ps]
    for k in range(2):
        _set_grads(ps, gen)
        del TBE.CALLS[:]
        opt.early_begin()
        assert TBE.CALLS == [("adam_step", [])] and float(opt._step) == k + 1
        opt.early_step(ps[:2], [p.grad for p in ps[:2]])
        opt.early_step(ps[2:3], [ps[2].grad], inline=True)             # held back ...
        assert [c[0] for c in TBE.CALLS] == ["adam_step", "adam_step", "ema_update"]
        opt.step()                                                      # ... until here, then the rest
        names = [c[0] for c in TBE.CALLS]
        assert names == ["adam_step"] + ["adam_step", "ema_update"] * 3
        for a, b in zip(TBE.CALLS[1::2], TBE.CALLS[2::2]):
            assert a[1] == b[1]
        updated = sum((c[1] for c in TBE.CALLS if c[0] == "ema_update"), [])
        assert sorted(updated) == sorted(q for i, q in enumerate(ptr) if i != NO_GRAD)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_skipped_step_does_not_move_the_average(monkeypatch, bad):
    from mimic_amd.optim import HipAdam
    TBE.install(monkeypatch)
    ps, gen = _params()
    opt = HipAdam(ps, lr=LR, max_grad_norm=1.0, ema_decay=0.5)
    _set_grads(ps, gen)
    opt.step()
    snap = opt._ema_flat.clone()
    ps[3].grad[5, 7] = bad
    del TBE.CALLS[:]
    opt.step()
    assert float(opt.clip_state[2]) == 1.0 and float(opt._step) == 1
    assert [c[0] for c in TBE.CALLS] == ["adam_step", "ema_update"]       # issued with the clip state, which withholds it
    assert torch.equal(opt._ema_flat, snap)
    ps[3].grad[5, 7] = 0.5
    opt.step()
    assert float(opt.clip_state[2]) == 0.0 and float(opt._step) == 2 and not torch.equal(opt._ema_flat, snap)


def test_swap_twice_restores_everything_and_training_is_refused_in_between(monkeypatch):
    from mimic_amd import layout
    from mimic_amd.optim import HipAdam
    TBE.install(monkeypatch)
    ps, gen = _params()
    opt = HipAdam(ps, lr=LR, ema_decay=0.5)
    opt.lowp = [p.detach().to(torch.bfloat16).reshape(-1).clone() if i in (1, 3) else None for i, p in enumerate(ps)]
    for _ in range(2):
        _set_grads(ps, gen)
        opt.step()
    for lp, p in zip(opt.lowp, ps):
        assert lp is None or torch.equal(lp, p.detach().reshape(-1).to(torch.bfloat16))
    live = [p.detach().clone() for p in ps]
    avg = [e.clone() for e in opt.ema_tensors()]
    low = [None if lp is None else lp.clone() for lp in opt.lowp]
    state = [opt._moments.clone(), opt._step.clone()]
    epoch = layout.param_epoch()
    opt.swap_ema()
    assert opt.ema_swapped and layout.param_epoch() == epoch + 1
    for p, e, a, l, lp in zip(ps, opt.ema_tensors(), avg, live, opt.lowp):
        assert torch.equal(p.detach(), a) and torch.equal(e, l)
        assert lp is None or torch.equal(lp, a.reshape(-1).to(torch.bfloat16))
    for what, call in (("step", opt.step), ("early_begin", opt.early_begin),
                       ("early_step", lambda: opt.early_step(ps[:1], [ps[0].grad]))):
        with pytest.raises(RuntimeError, match="swap"):
            call()
    opt.swap_ema()
    assert not opt.ema_swapped and layout.param_epoch() == epoch + 2
    for p, e, a, l, lp, lo in zip(ps, opt.ema_tensors(), avg, live, opt.lowp, low):
        assert torch.equal(p.detach().view(torch.int32), l.view(torch.int32)) and torch.equal(e.view(torch.int32), a.view(torch.int32))
        assert lp is None or torch.equal(lp.view(torch.int16), lo.view(torch.int16))
    assert torch.equal(opt._moments, state[0]) and torch.equal(opt._step, state[1])
    opt.step()                                                          # ... and training goes on


def test_averaged_weights_swaps_back_when_its_body_raises(monkeypatch):
    monkeypatch.delenv("MOPOE_TORCH_ADAM", raising=False)
    exp, batch = _tiny_exp(monkeypatch, ema_decay=0.5)
    from mimic_amd import run_epochs as RE
    opt = _hip_adam(exp)
    assert opt.ema_decay == 0.5                                         # set_hip_adam passes the flag on
    RE.train_step(exp, (dict(batch), None), None, None)
    RE.train_step(exp, (dict(batch), None), None, None)
    live = [p.detach().clone() for p in exp.mm_vae.parameters()]
    avg = [e.clone() for e in opt.ema_tensors()]
    assert any(not torch.equal(a, l) for a, l in zip(avg, live))
    with exp.averaged_weights() as on:
        assert on is True and opt.ema_swapped
        assert all(torch.equal(p.detach(), a) for p, a in zip(exp.mm_vae.parameters(), avg))
    assert not opt.ema_swapped
    with pytest.raises(KeyError, match="inside"):
        with exp.averaged_weights():
            assert opt.ema_swapped
            raise KeyError("inside")
    assert not opt.ema_swapped
    assert all(torch.equal(p.detach(), l) for p, l in zip(exp.mm_vae.parameters(), live))
    assert all(torch.equal(e, a) for e, a in zip(opt.ema_tensors(), avg))
