"""TEST INFRASTRUCTURE: plain-PyTorch restatement of ops.latent_style_fwd / ops.latent_style_bwd (the style latents of the
factorized representation), with the same signatures; the backward is taken by autograd through the forward.  Used on
CPU in place of the HIP ops (install) and on the GPU box as the reference the kernels are compared with.  Never imported by
the product package.

Reference arithmetic: mimic/networks/VAEtrimodalMimic.py:31-62, utils/utils.py:45-48, evaluation/losses.py:34-42,
divergence_measures/kl_div.py:8-16, ConvNetworksImgMimic.py:43-49, ConvNetworksTextMimic.py:43-54."""
from __future__ import annotations

import torch

import torch_backend_methods
from mimic_amd import ops as real_ops

OP_NAMES = ["latent_style_fwd", "latent_style_bwd"]


def install(monkeypatch):
    """torch_backend_methods.install (every other op) plus the two style ops (pytest monkeypatch; undone after the test)."""
    import sys
    torch_backend_methods.install(monkeypatch)
    me = sys.modules[__name__]
    for name in OP_NAMES:
        monkeypatch.setattr(real_ops, name, getattr(me, name))


def _core(smu, slv, eps_s, z, norm):
    zcat, klds = [], []
    for m in range(3):
        if smu[m] is None:
            zcat.append(None)
            klds.append(torch.zeros((), dtype=torch.float32, device=z.device))
            continue
        zs = eps_s[m] * torch.exp(0.5 * slv[m]) + smu[m]
        zcat.append(torch.cat((zs, z), dim=1))
        klds.append(-0.5 * torch.sum(1 - slv[m].exp() - smu[m].pow(2) + slv[m]) / norm)
    return zcat, torch.stack(klds)


def latent_style_fwd(smu, slv, eps_s, z, norm):
    with torch.no_grad():
        return _core(smu, slv, eps_s, z, norm)


def latent_style_bwd(smu, slv, eps_s, d, norm, g_zcat, g_klds):
    present = [m for m in range(3) if smu[m] is not None]
    b = smu[present[0]].shape[0]
    dev = smu[present[0]].device
    mu_l = [None if t is None else t.detach().clone().requires_grad_(True) for t in smu]
    lv_l = [None if t is None else t.detach().clone().requires_grad_(True) for t in slv]
    z = torch.zeros(b, d, dtype=smu[present[0]].dtype, device=dev, requires_grad=True)
    g_zcat = list(g_zcat) if g_zcat is not None else [None] * 3
    with torch.enable_grad():
        zcat, klds = _core(mu_l, lv_l, eps_s, z, norm)
        total = 0.0
        for o, g in zip(zcat, g_zcat):
            if g is not None and o is not None:
                total = total + (o * g).sum()
        if g_klds is not None:
            total = total + (klds * g_klds).sum()
    leaves = [t for t in mu_l + lv_l if t is not None] + [z]
    grads = torch.autograd.grad(total, leaves, allow_unused=True) if torch.is_tensor(total) else [None] * len(leaves)
    fix = lambda g, t: torch.zeros_like(t) if g is None else g.detach()
    it = iter(grads[:-1])
    dmu = [None if t is None else fix(next(it), t) for t in mu_l]
    dlv = [None if t is None else fix(next(it), t) for t in lv_l]
    return dmu, dlv, fix(grads[-1], z)
