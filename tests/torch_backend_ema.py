"""TEST INFRASTRUCTURE: plain-PyTorch restatement of ops.ema_update and ops.ema_swap (include/mopoe_hip_ema.h,
csrc/ema.hip), with the same signatures.  Used on CPU in place of the HIP ops (install) and on the GPU box as the reference
the kernels are compared with.  Never imported by the product package.

Semantics: s = step, d = min(decay, (1 + s) / (10 + s)) in double, w = float32(1 - d), ema = fma(w, p - ema, ema) -- the
difference rounded to float, the fma evaluated in double and rounded once (a float product is exact in double; the double
sum is then rounded a second time, which differs from the one rounding of a hardware fma only on a 2^-29-wide band around a
float tie: the last-bit allowance of the tests covers it).  A clip state that says skip: nothing changes.  Swap: the values
of p and ema exchanged, the bf16 copies rewritten from the new p."""
from __future__ import annotations

import numpy as np
import torch

import torch_backend_clip
from mimic_amd import ops as real_ops

OP_NAMES = ["ema_update", "ema_swap"]
CALLS = []      # (name, [data_ptr of every parameter of the call]) in call order, ops.adam_step included (install)


def install(monkeypatch):
    """torch_backend_clip.install plus the two EMA ops; every adam_step / ema_update / ema_swap call is logged in CALLS
    (cleared here) so that a test can see their order (pytest monkeypatch; undone after the test)."""
    import sys
    torch_backend_clip.install(monkeypatch)
    me = sys.modules[__name__]
    del CALLS[:]
    adam = real_ops.adam_step        # (the restatement torch_backend_clip just installed)

    def adam_step(params, grads, *a, **k):
        CALLS.append(("adam_step", [p.data_ptr() for p, g in zip(params, grads) if g is not None]))
        return adam(params, grads, *a, **k)

    monkeypatch.setattr(real_ops, "adam_step", adam_step)
    for name in OP_NAMES:
        monkeypatch.setattr(real_ops, name, getattr(me, name))


def decay_at(decay, s) -> float:
    """the decay in force at step counter s: min(decay, (1 + s) / (10 + s)), in double"""
    s = float(s)
    return min(float(decay), (1.0 + s) / (10.0 + s))


def weight_at(decay, s) -> float:
    """w: the float32 nearest to 1 - decay_at, as a Python float"""
    return float(np.float32(1.0 - decay_at(decay, s)))


def _check(who, params, emas, decay=0.0):
    if not (0.0 <= float(decay) < 1.0):
        raise real_ops.MopoeHipError(f"{who}: decay must be finite and in [0, 1)")
    for p, e in zip(params, emas):
        if p.dtype != torch.float32 or e.dtype != torch.float32 or p.numel() != e.numel():
            raise real_ops.MopoeHipError(f"{who}: parameters and averages must be fp32 tensors of equal size")


def ema_update(params, emas, decay, step, clip=None):
    _check("ema_update", params, emas, decay)
    CALLS.append(("ema_update", [p.data_ptr() for p in params]))
    if clip is not None and float(clip[2]) != 0.0:
        return
    w = weight_at(decay, float(step))
    for p, e in zip(params, emas):
        pf, ef = p.detach().reshape(-1), e.reshape(-1)
        diff = pf - ef                                                 # float
        ef.copy_((w * diff.double() + ef.double()).float())


def ema_swap(params, emas, lowp=None):
    _check("ema_swap", params, emas)
    CALLS.append(("ema_swap", [p.data_ptr() for p in params]))
    for i, (p, e) in enumerate(zip(params, emas)):
        pf, ef = p.detach().view(-1).view(torch.int32), e.view(-1).view(torch.int32)     # raw words: bits preserved
        tmp = pf.clone()
        pf.copy_(ef)
        ef.copy_(tmp)
        if lowp is not None and lowp[i] is not None:
            lowp[i].view(-1).copy_(p.detach().view(-1))
