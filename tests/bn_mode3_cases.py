"""TEST INFRASTRUCTURE: inputs and fp64 references of the mode-3 accuracy test (include/mopoe_hip.h, mopoe_bn_ref mode 3: conv2's
input gradient reads its ReLU mask and x-hat off the stored activation a2 = relu(bn2(d1)) instead of d1), at small |gamma| and
large |beta|.  tests/test_bn_ref_cpu.py runs the fp32 emulation and tests/test_bn_modes_gpu.py the bf16 kernel on exactly
these numbers, against exactly these references and bounds.

The bound (derived, not measured): a2 is y = relu(gamma xhat + beta) rounded to nearest bf16, |a2 - y| <= 2^-9 |y|, hence
|y| <= |a2| (1 + 2^-8) and the rebuilt x-hat (a2 - beta) / gamma is off by at most 2^-9 |a2| (1 + 2^-8) / |gamma| where the mask
is set.  sums[1] = sum_rows dx xhat of a channel therefore moves by at most sum_rows |dx| 2^-9 |a2| (1 + 2^-8) / |gamma_c|."""
import torch

import torch_backend as TB
from mimic_amd.ops import Bn, Geom

BF = torch.bfloat16
ULP = 2.0 ** -7      # one bf16 rounding step, relative
GEOM = Geom(2, 1, 32, 1, 64, 64, 128, 1, 4, 1, 2, 0, 1, False)
SETTINGS = [(gabs, beta) for gabs in (1.0, 0.05, 0.01) for beta in (0.1, 2.0)]
# the project's present bars of a bf16 input gradient (tests/plan_cases.py: bars): (rtol, atol_rel) of
# |got - ref| <= atol_rel max|ref| + rtol |ref|
DX_BAR = (1.01 * ULP, 2e-4)
SUMS_BAR = (2e-3, 2e-3)


class Mode3Case:
    """d1 random (fp64), bn2 mode 1 from d1's own statistics with |gamma| = gabs (mixed signs) and beta = beta, a2 computed in
    fp64 and rounded to bf16; dy and the packed weight are bf16 values.
      ref_stored: fp64 on the SAME stored a2 (mask a2 > 0, x-hat (a2 - beta) / gamma) -> dx (as stored: rounded to bf16), sums
      ref_exact:  fp64 with the exact x-hat from d1                                    -> dx (the same mask), sums
      slack:      per channel, the derived bound on |sums[1] of ref_stored - sums[1] of ref_exact|"""

    def __init__(self, gabs, beta):
        g, c = GEOM, GEOM.Cin
        gen = torch.Generator().manual_seed(4242)      # (the same d1, dy and weight at every setting)
        self.d1 = torch.randn(g.in_shape, generator=gen, dtype=torch.float64)
        self.w = (torch.randn(g.taps, c, g.Cout, generator=gen) / 16).to(BF)
        self.dy = torch.randn(g.out_shape, generator=gen).to(BF)
        sign = torch.where(torch.rand(c, generator=gen) < 0.5, -1.0, 1.0)
        gamma, betav = (gabs * sign).float(), torch.full((c,), float(beta))
        x2 = self.d1.reshape(-1, c)
        rows = x2.shape[0]
        sums = torch.stack([x2.sum(0), (x2 * x2).sum(0)])
        self.bn2 = Bn(gamma, betav, 1, sums=sums, count=rows)            # mode 1, on d1
        self.bn2y = Bn(gamma, betav, 3)                                  # mode 3, on a2: gamma and beta alone
        mean = sums[0] / rows
        rstd = 1.0 / torch.sqrt((sums[1] / rows - mean * mean).clamp_min(0) + self.bn2.eps)
        xhat = (self.d1 - mean) * rstd
        y = torch.relu(gamma.double() * xhat + betav.double())
        self.a2 = y.to(BF)
        a2 = self.a2.double()
        assert torch.equal(a2 > 0, y > 0)                                # the stored activation keeps the ReLU mask
        dx = (TB.conv_dgrad(self.dy.double(), self.w.double(), g) * (a2 > 0)).to(BF).double()
        xhat_a2 = (a2 - betav.double()) / gamma.double()

        def sums_of(xh):
            return torch.stack([dx.reshape(-1, c).sum(0), (dx * xh).reshape(-1, c).sum(0)])

        self.ref_stored = dict(dx=dx, sums=sums_of(xhat_a2))
        self.ref_exact = dict(dx=dx, sums=sums_of(xhat))
        self.slack = (dx.abs() * (2.0 ** -9) * a2 * (1 + 2.0 ** -8)).reshape(-1, c).sum(0) / gamma.double().abs()


def worst(got, ref, bar, slack=None):
    """worst |got - ref| / bound over the elements, bound = atol_rel max|ref| + rtol |ref| (+ slack)"""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    bound = bar[1] * max(ref.abs().max().item(), 1e-6) + bar[0] * ref.abs()
    if slack is not None:
        bound = bound + slack
    return ((got - ref).abs() / bound).max().item()


def assert_mode3(case: Mode3Case, dx, sums, tag):
    """the assertions of the mode-3 accuracy test on one result (dx bf16 [in_shape], sums double [2, C]); returns the figures"""
    fig = dict(dx=worst(dx.float(), case.ref_stored["dx"], DX_BAR),
               sums_stored=worst(sums, case.ref_stored["sums"], SUMS_BAR),
               sums0_exact=worst(sums[0], case.ref_exact["sums"][0], SUMS_BAR),
               sums1_exact=worst(sums[1], case.ref_exact["sums"][1], SUMS_BAR, case.slack))
    print(f"mode3 {tag}: " + " ".join(f"{k}={v:.3f}" for k, v in fig.items()) + " (worst error / bound)")
    assert all(v <= 1.0 for v in fig.values()), (tag, fig)
    return fig


def sums1_error(sums, case: Mode3Case):
    """max over the channels of |sums[1] - exact| on the scale of max|exact| (the figure the ratio table is made of)"""
    ref = case.ref_exact["sums"][1]
    return ((sums[1].detach().double().cpu() - ref).abs().max() / ref.abs().max()).item()
