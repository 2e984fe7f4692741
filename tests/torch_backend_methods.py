"""TEST INFRASTRUCTURE: plain-PyTorch restatement of ops.latent_mixture_fwd / ops.latent_mixture_bwd (method 'moe' and
'jsd'), with the same signatures; the backward is taken by autograd through the forward.  Used on CPU in place of the HIP
ops (install) and on the GPU box as the reference the kernels are compared with.  Never imported by the product package.

Reference arithmetic: mimic/utils/BaseMMVae.py:101-111,139-196 (moe_fusion), utils/utils.py:55-77,
evaluation/divergence_measures/mm_div.py:20-32,67-106, kl_div.py:8-16."""
from __future__ import annotations

import torch

import torch_backend
from mimic_amd import ops as real_ops

OP_NAMES = ["latent_mixture_fwd", "latent_mixture_bwd"]
_MEMBER_ORDER = (1, 0, 2)  # sorted-by-name order inside a subset: Lateral, PA, text


def install(monkeypatch):
    """torch_backend.install plus the two mixture ops (pytest monkeypatch; undone after the test)."""
    import sys
    torch_backend.install(monkeypatch)
    me = sys.modules[__name__]
    for name in OP_NAMES:
        monkeypatch.setattr(real_ops, name, getattr(me, name))


def _select(parts, starts):
    return torch.cat([parts[j][starts[j]:starts[j + 1]] for j in range(len(parts))])


def _kl(mu0, lv0, mu1=None, lv1=None, norm=1.0):
    if mu1 is None:
        return -0.5 * torch.sum(1 - lv0.exp() - mu0.pow(2) + lv0) / norm
    return -0.5 * torch.sum(1 - lv0.exp() / lv1.exp() - (mu0 - mu1).pow(2) / lv1.exp() + lv0 - lv1) / norm


def _core(method, mu_in, lv_in, eps, member_row_start, comp_row_start, w, norm):
    present = [s for s in range(3) if mu_in[s] is not None]
    avail = sum(1 << s for s in present)
    subsets = [m for m in real_ops.SUBSET_MASKS if (m & ~avail) == 0]
    sub_mu, sub_lv = [], []
    for sm in subsets:
        members = [s for s in _MEMBER_ORDER if sm & (1 << s)]
        starts = member_row_start[len(members) - 1]
        sub_mu.append(_select([mu_in[s] for s in members], starts))
        sub_lv.append(_select([lv_in[s] for s in members], starts))
    sub_mu, sub_lv = torch.stack(sub_mu), torch.stack(sub_lv)
    cm = [mu_in[s] for s in present]
    cl = [lv_in[s] for s in present]
    if method == "jsd":
        cm.append(torch.zeros_like(cm[0]))
        cl.append(torch.zeros_like(cl[0]))
    comp_mu, comp_lv = torch.stack(cm), torch.stack(cl)
    jm, jl = _select(cm, comp_row_start), _select(cl, comp_row_start)
    z = eps * torch.exp(0.5 * jl) + jm
    klds = torch.stack([_kl(sub_mu[k], sub_lv[k], norm=norm) for k in range(len(subsets))])
    wt = torch.tensor(list(w), dtype=torch.float32, device=eps.device)
    pd_mu = pd_lv = None
    if method == "jsd":
        # alpha_poe (mm_div.py:20-32) over the components, alphas = w
        T = 1 / (torch.exp(comp_lv) + 1e-8)
        a = wt.view(-1, 1, 1)
        pd_var = 1.0 / torch.sum(a * T, dim=0)
        pd_mu = pd_var * torch.sum(a * comp_mu * T, dim=0)
        pd_lv = torch.log(pd_var)
        indiv = torch.stack([_kl(comp_mu[c], comp_lv[c], pd_mu, pd_lv, norm) for c in range(len(cm))])
    else:
        indiv = torch.stack([_kl(comp_mu[c], comp_lv[c], norm=norm) for c in range(len(cm))])
    jd = (wt * indiv).sum().reshape(1)
    return sub_mu, sub_lv, comp_mu, comp_lv, jm, jl, z, klds, indiv, jd, pd_mu, pd_lv


def latent_mixture_fwd(method, mu_in, lv_in, eps, member_row_start, comp_row_start, w, norm):
    with torch.no_grad():
        return _core(method, mu_in, lv_in, eps, member_row_start, comp_row_start, w, norm)


def latent_mixture_bwd(method, mu_in, lv_in, eps, member_row_start, comp_row_start, w, norm, g_sub_mu, g_sub_lv,
                       g_comp_mu, g_comp_lv, g_jm, g_jl, g_z, g_klds, g_indiv, g_jd, g_pd_mu=None, g_pd_lv=None):
    mu_l = [None if t is None else t.detach().clone().requires_grad_(True) for t in mu_in]
    lv_l = [None if t is None else t.detach().clone().requires_grad_(True) for t in lv_in]
    gs = (g_sub_mu, g_sub_lv, g_comp_mu, g_comp_lv, g_jm, g_jl, g_z, g_klds, g_indiv, g_jd, g_pd_mu, g_pd_lv)
    with torch.enable_grad():
        outs = _core(method, mu_l, lv_l, eps, member_row_start, comp_row_start, w, norm)
        total = 0.0
        for o, g in zip(outs, gs):
            if g is not None and o is not None:
                total = total + (o * g).sum()
    leaves = [t for t in mu_l + lv_l if t is not None]
    grads = torch.autograd.grad(total, leaves, allow_unused=True) if torch.is_tensor(total) else [None] * len(leaves)
    it = iter(grads)
    dmu = [None if t is None else next(it) for t in mu_l]
    dlv = [None if t is None else next(it) for t in lv_l]
    fix = lambda g, t: torch.zeros_like(t) if g is None else g
    return ([None if t is None else fix(g, t).detach() for g, t in zip(dmu, mu_l)],
            [None if t is None else fix(g, t).detach() for g, t in zip(dlv, lv_l)])
