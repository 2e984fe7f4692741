"""TEST INFRASTRUCTURE: the hostile-value input sets of tests/test_guarded_ops_gpu.py, built in one place so that the CPU file
(tests/test_arena_cpu.py) pins them -- the fp32 reference arithmetic has to stay within half of the GPU bar on each set when
compared with its own fp64 evaluation -- and the GPU tests then use exactly those sets."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import torch_backend as TB
from mimic_amd.ops import BN_EPS, Bn

# BatchNorm at shifted means: rows x 64 activations randn + r
BN_SHIFT_ROWS = (65536, 4096)
BN_SHIFTS = (0, 10, 30, 100)          # r <= 30 is gated, r = 100 logged
BN_GATED_SHIFT = 30
# latent kernels: mu ~ 3 randn, logvar uniform in this range
WIDE_LOGVAR = (-8.0, 8.0)
DEGENERATE_CASES = ("const_col", "gamma0_mode1", "gamma0_mode3", "rvar0_mode2")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def bn_shift_inputs(rows, c, r, narrow):
    """narrow: channel 5 is the same draw scaled by 1e-2 (variance 1e-4 against eps = 1e-5, the same mean / spread ratio)"""
    gen = _gen(rows + 7 * r + int(narrow))
    x = torch.randn(rows, c, generator=gen) + float(r)
    if narrow:
        x[:, 5] *= 1e-2
    return dict(x=x, dy=torch.randn(rows, c, generator=gen), gamma=1 + 0.3 * torch.randn(c, generator=gen),
                beta=0.2 * torch.randn(c, generator=gen), w1=torch.randn(1, c, c, generator=gen) / 8)


def _relerr(a, ref64):
    return float((a.double() - ref64).abs().max() / ref64.abs().max().clamp_min(1e-30))


def bn_reference_errors(h):
    """-> dict(fp64 = the fp64 evaluation of every quantity the shifted-mean test measures, ref_err = the error against it of
    torch.nn.functional.batch_norm and its autograd in fp32 on the CPU)"""
    x, dy, gamma, beta, w1 = h["x"], h["dy"], h["gamma"], h["beta"], h["w1"]
    rows, c = x.shape
    x64, dy64, g64, b64 = x.double(), dy.double(), gamma.double(), beta.double()
    mean = x64.mean(0)
    var = x64.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    xhat = (x64 - mean) * rstd
    act = torch.relu(xhat * g64 + b64)
    sums = torch.stack([dy64.sum(0), (dy64 * xhat).sum(0)])
    dx = g64 * rstd * (dy64 - sums[0] / rows - xhat * (sums[1] / rows))
    t64 = dict(stats=torch.stack([x64.sum(0), (x64 * x64).sum(0)]), mean=mean, var=var, act=act, conv=act @ w1.double().view(c, c),
               sums=sums, dx=dx, run=torch.stack([0.1 * mean, 0.9 + 0.1 * var * (rows / (rows - 1))]))
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = torch.zeros(c), torch.ones(c)
    y = F.batch_norm(xr, rm, rv, gr, br, training=True, momentum=0.1, eps=BN_EPS)
    y.backward(dy)
    a32 = torch.relu(y.detach())
    v32, m32 = torch.var_mean(x, dim=0, unbiased=False)
    err = dict(conv_fwd_stats=_relerr(torch.stack([x.sum(0), (x * x).sum(0)]), t64["stats"]), mean=_relerr(m32, mean),
               var=float(((v32.double() - var).abs() / var).max()), bn_relu_apply=_relerr(a32, act),
               conv_bn_on_load=_relerr(a32 @ w1.view(c, c), t64["conv"]), bn_bwd_reduce=_relerr(torch.stack([br.grad, gr.grad]), sums),
               bn_bwd_apply=_relerr(xr.grad, dx), bn_running_update=_relerr(torch.stack([rm, rv]), t64["run"]))
    return dict(fp64=t64, ref_err=err)


# the floor of tests/test_hip_ops_gpu.check for each measured quantity (its atol_rel: a fraction of the tensor's scale)
BN_FLOOR = dict(conv_fwd_stats=1e-4, bn_relu_apply=2e-4, conv_bn_on_load=2e-4, bn_bwd_reduce=2e-4, bn_bwd_apply=2e-4, bn_running_update=1e-5)


def degenerate_inputs(g, case):
    """channel 3 (and 7) of the BatchNorm in front of conv geometry g made degenerate"""
    gen = _gen(50 + DEGENERATE_CASES.index(case) + g.Cin)
    c = g.Cin
    x = torch.randn(g.in_shape, generator=gen)
    if case == "const_col":
        x[..., 3] = 1.7
    gamma, beta = 1 + 0.3 * torch.randn(c, generator=gen), 0.2 * torch.randn(c, generator=gen)
    beta[3], beta[7] = 0.25, -0.25                    # (away from zero: the ReLU mask of a constant channel is the sign of beta)
    if case.startswith("gamma0"):
        gamma[3], gamma[7] = 0.0, 0.0
    rows = x.numel() // c
    if case == "rvar0_mode2":
        rvar = 0.5 + torch.rand(c, generator=gen)
        rvar[3] = 0.0
        bn = Bn(gamma, beta, 2, rmean=0.1 * torch.randn(c, generator=gen), rvar=rvar)
    else:
        x2 = x.reshape(-1, c).double()
        bn = Bn(gamma, beta, 1, sums=torch.stack([x2.sum(0), (x2 * x2).sum(0)]), count=rows)
    gx = torch.randn(g.in_shape, generator=gen)
    mean, rstd = TB.bn_coef(bn)[:2]
    sums_x = torch.stack([gx.reshape(-1, c).double().sum(0), (gx * ((x - mean) * rstd)).reshape(-1, c).double().sum(0)])
    return dict(x=x, wp=torch.randn(g.taps, g.Cin, g.Cout, generator=gen) / math.sqrt(g.taps * g.Cin), bias=0.1 * torch.randn(g.Cout, generator=gen),
                dy=torch.randn(g.out_shape, generator=gen), bn=bn, gx=gx, sums_x=sums_x, act=TB.bn_relu_apply(x, bn))


def _uniform(gen, shape, lo, hi):
    return (torch.rand(shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo).float()


def wide_latent_inputs(b, d, present):
    gen = _gen(60 + b + d)
    lo, hi = WIDE_LOGVAR
    mu = [3 * torch.randn(b, d, generator=gen) if p else None for p in present]
    lv = [_uniform(gen, (b, d), lo, hi) if p else None for p in present]
    return mu, lv, torch.randn(b, d, generator=gen)


def wide_style_inputs(b, d, dims):
    gen = _gen(61 + b + d)
    lo, hi = WIDE_LOGVAR
    smu = [3 * torch.randn(b, s, generator=gen) for s in dims]
    slv = [_uniform(gen, (b, s), lo, hi) for s in dims]
    return smu, slv, [torch.randn(b, s, generator=gen) for s in dims], 3 * torch.randn(b, d, generator=gen)
