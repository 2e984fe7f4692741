"""TEST INFRASTRUCTURE for the latent-representation evaluation (--eval_lr): the seeded logistic-regression problems of the
g11_lr_* fixtures (inputs are regenerated here, the fixtures store the reference's results and a fingerprint), the
objective's float64 gradient and a float64 damped Newton that goes to the exact optimum.

The problem sklearn's LogisticRegression defaults pose, per (subset s, label l), y in {0, 1}, intercept not penalised:
    f(w, b) = C sum_i [log(1 + exp(m_i)) - y_i m_i] + 1/2 |w|^2,   m_i = x_i . w + b
"""
from __future__ import annotations

import numpy as np

# name -> list of cases; a case: seed, N train rows, M test rows, D, S subsets, per-label kinds, feature offset
#   kind 'std': labels Bernoulli(0.4), shift 0.2 + 0.1 s along the label's direction for subset s
#        'sep': the same labels, shift 2.0 (linearly separable)
#        'rare': Bernoulli(0.05) labels          'one': exactly one positive training row
CASES = {
    "c2": [dict(seed=1101, N=500, M=240, D=128, S=7, kinds=("std", "std", "std"), offset=0.0)],
    "small": [dict(seed=1201, N=37, M=240, D=8, S=7, kinds=("std",), offset=0.0),
              dict(seed=1202, N=2000, M=240, D=64, S=7, kinds=("std", "std", "std"), offset=0.0),
              dict(seed=1203, N=500, M=240, D=256, S=7, kinds=("std", "std", "std"), offset=0.0)],
    "hard": [dict(seed=1301, N=500, M=240, D=128, S=7, kinds=("sep", "rare", "one"), offset=0.5)],
}
SIGMA = 0.7
LABEL_NAMES = ["Lung Opacity", "Pleural Effusion", "Support Devices"]
SUBSET_KEYS = ["PA", "Lateral", "text", "Lateral_PA", "PA_text", "Lateral_text", "Lateral_PA_text"]


def _labels(rs, kind, n, train):
    if kind in ("std", "sep"):
        return (rs.random_sample(n) < 0.4).astype(np.float32)
    if kind == "rare" or not train:
        y = (rs.random_sample(n) < 0.05).astype(np.float32)
        if y.sum() == 0:
            y[rs.randint(n)] = 1.0
        return y
    y = np.zeros(n, dtype=np.float32)          # 'one'
    y[rs.randint(n)] = 1.0
    return y


def make_case(spec):
    """-> dict: x_train [S,N,D] f32, y_train [N,L] f32, x_test [S,M,D] f32, y_test [M,L] f32"""
    rs = np.random.RandomState(int(spec["seed"]))
    n, m, d, s_n, kinds = spec["N"], spec["M"], spec["D"], spec["S"], spec["kinds"]
    l_n = len(kinds)
    dirs = rs.standard_normal((l_n, d))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    out = {}
    for split, rows in (("train", n), ("test", m)):
        y = np.stack([_labels(rs, k, rows, split == "train") for k in kinds], axis=1)
        x = np.empty((s_n, rows, d), dtype=np.float64)
        for s in range(s_n):
            x[s] = SIGMA * rs.standard_normal((rows, d)) + spec["offset"]
            for l, k in enumerate(kinds):
                shift = 2.0 if k == "sep" else 0.2 + 0.1 * s
                x[s] += (2.0 * y[:, l:l + 1] - 1.0) * shift * dirs[l][None, :]
        out["x_" + split], out["y_" + split] = x.astype(np.float32), y.astype(np.float32)
    return out


def fingerprint(case):
    """a few float64 sums of the regenerated inputs: the fixture's results belong to exactly these numbers"""
    return np.array([case[k].astype(np.float64).sum() for k in ("x_train", "y_train", "x_test", "y_test")]
                    + [np.square(case["x_train"].astype(np.float64)).sum(), float(case["x_train"][-1, -1, -1])])


def f_and_grad(wb, x, y, c=1.0):
    """float64 objective and gradient at wb = [w; b]; x [N,D], y [N]"""
    x, y, wb = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(wb, np.float64)
    m = x @ wb[:-1] + wb[-1]
    f = c * np.sum(np.logaddexp(0.0, m) - y * m) + 0.5 * wb[:-1] @ wb[:-1]
    e = np.exp(-np.abs(m))
    p = np.where(m >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    g = np.concatenate([c * (x.T @ (p - y)) + wb[:-1], [c * np.sum(p - y)]])
    return f, g, p


def grad_inf(w_all, x_all, y_all, c=1.0):
    """|grad f|_inf in float64 for every problem: w_all [S,L,D+1], x_all [S,N,D], y_all [N,L] -> [S,L]"""
    s_n, l_n = w_all.shape[:2]
    return np.array([[np.abs(f_and_grad(w_all[s, l], x_all[s], y_all[:, l], c)[1]).max() for l in range(l_n)]
                     for s in range(s_n)])


def newton_exact(x, y, c=1.0, tol=1e-10, max_iter=200):
    """float64 damped Newton to |grad f|_inf <= tol -> [w; b]"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n, d = x.shape
    xa = np.concatenate([x, np.ones((n, 1))], axis=1)
    reg = np.diag(np.concatenate([np.ones(d), [0.0]]))
    wb = np.zeros(d + 1)
    for _ in range(max_iter):
        f, g, p = f_and_grad(wb, x, y, c)
        if np.abs(g).max() <= tol:
            return wb
        h = c * (xa.T * (p * (1.0 - p))) @ xa + reg
        step = -np.linalg.solve(h, g)
        t = 1.0
        for _h in range(60):
            if f_and_grad(wb + t * step, x, y, c)[0] <= f + 1e-4 * t * (g @ step) + 1e-13 * abs(f):
                break
            t *= 0.5
        wb = wb + t * step
    raise RuntimeError(f"newton_exact: |grad|_inf {np.abs(g).max():.3e} after {max_iter} iterations")


def decisions(w_all, x_all):
    """float64 decision values [S,M,L] of w_all [S,L,D+1] on x_all [S,M,D]"""
    w_all, x_all = np.asarray(w_all, np.float64), np.asarray(x_all, np.float64)
    return np.einsum("smd,sld->sml", x_all, w_all[:, :, :-1]) + w_all[:, None, :, -1]


def load_cases(name):
    """-> list of (tag, spec, regenerated inputs, fixture arrays of the case) with the fingerprint checked"""
    from golden_util import load
    g = load(f"g11_lr_{name}")
    out = []
    for i, spec in enumerate(CASES[name]):
        case = make_case(spec)
        np.testing.assert_allclose(fingerprint(case), g[f"{i}/fingerprint"], rtol=1e-12, atol=0,
                                   err_msg="lr_util.make_case no longer regenerates the fixture's inputs")
        fx = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(f"{i}/")}
        out.append((f"{name}{i}", spec, case, fx))
    return out


def unpack_pred(fx, spec):
    s_n, m, l_n = spec["S"], spec["M"], len(spec["kinds"])
    return np.unpackbits(fx["pred_ref"])[: s_n * m * l_n].reshape(s_n, m, l_n).astype(np.float32)
