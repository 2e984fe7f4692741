"""TEST INFRASTRUCTURE: plain-PyTorch restatement of ops.grad_norm, ops.grad_norm_partials and ops.adam_step(clip=...)
(include/mopoe_hip_optim.h, csrc/adam.hip), with the same signatures.  Used on CPU in place of the HIP ops (install) and on
the GPU box as the reference the kernels are compared with.  Never imported by the product package.

Semantics: torch.nn.utils.clip_grad_norm_(norm_type=2) -- total_norm = sqrt(sum g^2), scale = min(1, max_norm /
(total_norm + 1e-6)) -- with the sums in double and ONE rounding of norm and scale to float; a norm that is not finite as a
float sets skip, and the clipped step then changes nothing."""
from __future__ import annotations

import torch

import torch_backend
from mimic_amd import ops as real_ops

OP_NAMES = ["grad_norm", "grad_norm_partials", "adam_step"]
CHUNK = 4096


def install(monkeypatch):
    """torch_backend.install plus the clip ops (pytest monkeypatch; undone after the test)."""
    import sys
    torch_backend.install(monkeypatch)
    me = sys.modules[__name__]
    for name in OP_NAMES:
        monkeypatch.setattr(real_ops, name, getattr(me, name))


def grad_norm_partials(numels) -> int:
    return sum((int(n) + CHUNK - 1) // CHUNK for n in numels if int(n) > 0)


def norm_and_scale64(grads, max_norm):
    """-> (total_norm, scale) as float64 tensors, before any rounding to float"""
    total = torch.zeros((), dtype=torch.float64)
    for g in grads:
        if g is not None and g.numel():
            total = total + g.detach().double().pow(2).sum().cpu()
    norm = total.sqrt()
    return norm, torch.clamp(max_norm / (norm + 1e-6), max=1.0)


def grad_norm(grads, max_norm, state, scratch):
    need = grad_norm_partials([g.numel() for g in grads if g is not None])
    if scratch.numel() < need:
        raise real_ops.MopoeHipError(f"grad_norm: scratch holds {scratch.numel()} doubles, the gradients need {need}")
    if not (0.0 <= float(max_norm) < float("inf")):
        raise real_ops.MopoeHipError("grad_norm: max_norm must be finite and >= 0")
    norm64, scale64 = norm_and_scale64(grads, float(max_norm))
    norm = norm64.float()
    skip = 0.0 if bool(torch.isfinite(norm)) else 1.0
    state[0] = norm
    state[1] = 0.0 if skip else scale64.float()
    state[2] = skip
    state[3] += skip
    return state


def adam_step(params, grads, ms, vs, step, lr, beta1, beta2, eps, coef, lowp=None, prep=True, clip=None):
    """torch_backend.adam_step on scale * g (the product formed in float, as the kernel forms it); skip: nothing changes"""
    if clip is not None:
        if float(clip[2]) != 0.0:
            return
        scale = clip[1].to(torch.float32)
        grads = [None if g is None else g.float() * scale.to(g.device) for g in grads]
    torch_backend.adam_step(params, grads, ms, vs, step, lr, beta1, beta2, eps, coef, lowp=lowp, prep=prep)
