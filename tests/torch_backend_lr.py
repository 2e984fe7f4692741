"""TEST INFRASTRUCTURE: plain-PyTorch float64 restatement of ops.logreg_fit / ops.logreg_predict (the latent-representation
classifiers of --eval_lr), with the same signatures.  Used on CPU in place of the HIP ops (install) and on the GPU box as
the comparison partner of the kernels.  Never imported by the product package.

Reference: mimic/evaluation/eval_metrics/representation.py:147-187 (LogisticRegression(solver='lbfgs', max_iter=1000) per
subset and label); the problem its defaults pose is solved here to the exact optimum by a damped Newton iteration."""
from __future__ import annotations

import torch

import torch_backend_lhood
from mimic_amd import ops as real_ops

OP_NAMES = ["logreg_fit", "logreg_predict"]
CALLS = {"logreg_fit": 0, "logreg_predict": 0}


def install(monkeypatch):
    """torch_backend_lhood.install (every other op) plus the two classifier ops (pytest monkeypatch; undone after the test)."""
    import sys
    torch_backend_lhood.install(monkeypatch)
    me = sys.modules[__name__]
    for name in OP_NAMES:
        monkeypatch.setattr(real_ops, name, getattr(me, name))


def _f_grad(wb, xa, y, c):
    m = xa @ wb
    f = c * (torch.logaddexp(torch.zeros_like(m), m) - y * m).sum() + 0.5 * (wb[:-1] ** 2).sum()
    p = torch.sigmoid(m)
    g = c * (xa.T @ (p - y))
    g[:-1] += wb[:-1]
    return f, g, p


def _fit_one(x, y, c, max_iter, tol):
    n, d = x.shape
    xa = torch.cat([x, torch.ones(n, 1, dtype=x.dtype, device=x.device)], dim=1)
    reg = torch.diag(torch.cat([torch.ones(d, dtype=x.dtype, device=x.device), torch.zeros(1, dtype=x.dtype, device=x.device)]))
    wb = torch.zeros(d + 1, dtype=x.dtype, device=x.device)
    steps = 0
    for it in range(max_iter + 1):
        f, g, p = _f_grad(wb, xa, y, c)
        gn = g.abs().max().item()
        if not gn > tol or it == max_iter:
            break
        h = c * (xa.T * (p * (1 - p))) @ xa + reg
        step = -torch.linalg.solve(h, g)
        t, gd, ok = 1.0, (g @ step).item(), False
        for _ in range(60):
            if _f_grad(wb + t * step, xa, y, c)[0].item() <= f.item() + 1e-4 * t * gd + 1e-13 * abs(f.item()):
                ok = True
                break
            t *= 0.5
        if not ok:
            break
        wb = wb + t * step
        steps += 1
    return wb, steps, gn


def logreg_fit(x, y, c: float = 1.0, max_iter: int = 100, tol: float = 1e-5):
    """float64 optimum; W [S, L, D+1] float64, info [S, L, 2] float64.  (tol is tightened to at most 1e-10: this is the
    yardstick, not a model of the kernel's stopping rule.)"""
    CALLS["logreg_fit"] += 1
    with torch.no_grad():
        x64, y64 = x.double(), y.double()
        s_n, _n, d = x.shape
        l_n = y.shape[1]
        w = torch.empty(s_n, l_n, d + 1, dtype=torch.float64, device=x.device)
        info = torch.empty(s_n, l_n, 2, dtype=torch.float64, device=x.device)
        for s in range(s_n):
            for l in range(l_n):
                wb, steps, gn = _fit_one(x64[s], (y64[:, l] > 0.5).double(), float(c), int(max_iter), min(float(tol), 1e-10))
                w[s, l], info[s, l, 0], info[s, l, 1] = wb, steps, gn
        return w, info


def logreg_predict(x, w, want_decision: bool = False):
    CALLS["logreg_predict"] += 1
    with torch.no_grad():
        xs = torch.stack(list(x)) if not isinstance(x, torch.Tensor) else x
        dec = torch.einsum("smd,sld->sml", xs.double(), w[:, :, :-1].double()) + w[:, None, :, -1].double()
        pred = (dec > 0).float()
        return (pred, dec) if want_decision else pred
