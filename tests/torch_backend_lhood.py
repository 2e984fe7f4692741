"""TEST INFRASTRUCTURE: plain-PyTorch restatement of ops.lhood_style_sample / ops.lhood_estimates (the factorized
likelihood estimator), with the same signatures.  Used on CPU in place of the HIP ops (install) and on the GPU box as the
reference the kernels are compared with.  Never imported by the product package.

Reference arithmetic: mimic/evaluation/eval_metrics/likelihood.py:17-96, mimic/utils/likelihood.py:13-220."""
from __future__ import annotations

import torch

import torch_backend_style
from mimic_amd import ops as real_ops
from mimic_amd.utils.likelihood import gaussian_log_pdf, log_mean_exp, unit_gaussian_log_pdf

OP_NAMES = ["lhood_style_sample", "lhood_estimates"]


def install(monkeypatch):
    """torch_backend_style.install (every other op) plus the two estimator ops (pytest monkeypatch; undone after the test)."""
    import sys
    torch_backend_style.install(monkeypatch)
    me = sys.modules[__name__]
    for name in OP_NAMES:
        monkeypatch.setattr(real_ops, name, getattr(me, name))


def _draw(mu, logvar, eps):
    k, b, d = eps.shape
    mu_r = mu.unsqueeze(0).expand(k, b, d).reshape(k * b, d)
    lv_r = logvar.unsqueeze(0).expand(k, b, d).reshape(k * b, d)
    z = eps.reshape(k * b, d) * torch.exp(0.5 * lv_r) + mu_r
    return z, unit_gaussian_log_pdf(z) - gaussian_log_pdf(z, mu_r, lv_r)


def lhood_style_sample(mu, logvar, eps, style_mu, style_logvar, style_eps):
    with torch.no_grad():
        z, t_c = _draw(mu, logvar, eps)
        zs, t_s = _draw(style_mu, style_logvar, style_eps)
        return torch.cat((zs, z), dim=1), t_c, t_s


def lhood_estimates(lp, t_c, t_s, n_samples, subset_mask):
    with torch.no_grad():
        b = t_c.shape[0] // n_samples
        ts = torch.zeros_like(t_c) if t_s is None else t_s
        ws = [lp[m] + t_c + (ts if (subset_mask >> m) & 1 else 0.0) for m in range(3)]
        ws.append(lp[0] + lp[1] + lp[2] + t_c + 3.0 * ts)
        # the reference's view of the sample-major [K*B] vector as (batch_size, K)
        return torch.stack([torch.mean(log_mean_exp(w.view(b, n_samples), dim=1)) for w in ws])
