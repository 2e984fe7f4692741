"""The BatchNorm-mode x path matrix of the HIP kernels, closed (running statistics = mode 2 = a backward pass taken in eval mode;
mode 3 = conv2's input gradient reading its ReLU mask and x-hat off the stored activation, include/mopoe_hip.h):

  * every entry point that takes a mopoe_bn_ref refuses a broken one with MOPOE_ERR_ARG before anything is enqueued
    (csrc/bn_ref_check.hpp; tests/test_bn_ref_cpu.py holds the check itself against its rules on the CPU);
  * the streaming block front (csrc/pointwise.hip) of both storage families with running statistics in bn1 and / or bn2, and
    conv2's input gradient through a mode-3 reference that carries no statistics at all;
  * mode 3 at small |gamma| and large |beta| against fp64, at the derived bound (tests/bn_mode3_cases.py);
  * the whole model in eval mode WITH gradients at 64 channels (fixtures G7 eval64_b8 / eval64_b8_bf16, oracle/gen_g7.py), on the
    default switches and with the fp32 forward front (MOPOE_BLOCK_FRONT_F32_FWD=1), each with a recorder around ops.conv_dgrad
    and ops.block_front_bwd that proves the paths in question ran.

(The bf16 glue and the weight gradients under mode 2 are loops inside their sibling tests: test_block_glue_bf16,
test_conv_family, test_conv_family_bf16.)
"""
import ctypes as C

import pytest
import torch

import bn_mode3_cases as M3
from g7_util import check_bf16_case, check_fp32_case
from mimic_amd import ops
from mimic_amd.ops import Bn, Geom
from test_bf16_gpu import front_case_bf16
from test_hip_ops_gpu import _log, front_case_f32, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ERR_ARG = -1
SENTINEL = 7.0


# ---------------------------------------------------------------------------------------------------------------
# refusals: nothing is launched, every output keeps its sentinel
# ---------------------------------------------------------------------------------------------------------------
def _refs(c, rows):
    """(a good mode-1 reference, {label: broken reference}) on the GPU"""
    gamma, beta = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    sums = torch.stack([torch.zeros(c, dtype=torch.float64, device=DEV), torch.full((c,), float(rows), dtype=torch.float64, device=DEV)])
    rmean, rvar = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    good = Bn(gamma, beta, 1, sums=sums, count=rows)
    broken = {"mode 1 without sums": Bn(gamma, beta, 1, sums=None, count=rows),
              "mode 2 without rvar": Bn(gamma, beta, 2, rmean=rmean, rvar=None),
              "mode 7": Bn(gamma, beta, 7, sums=sums, count=rows, rmean=rmean, rvar=rvar),
              "mode 3": Bn(gamma, beta, 3)}
    return good, broken


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
def test_every_entry_point_refuses_a_broken_bn_ref(dt):
    lib, p, bn, nomask, st = ops.lib(), ops._p, ops._bn, ops._mask(None), ops._stream()
    h = dt == BF
    sfx = "_bf16" if h else ""
    c, g = 64, Geom(2, 4, 4, 4, 4, 64, 64, 1, 1, 1, 1, 0, 0, False)
    rows = g.N * g.Hs * g.Ws
    gc = g.c()
    gr, R, nil, f = C.byref(gc), C.c_int64(rows), C.c_size_t(0), C.c_float
    good, broken = _refs(c, rows)
    x = torch.randn(rows, c, device=DEV).to(dt)                        # every activation-like input
    w = (torch.randn(1, c, c, device=DEV) / 8).to(dt)
    bias = torch.zeros(c, device=DEV)
    sums_in = torch.zeros(2, c, dtype=torch.float64, device=DEV)
    # outputs, pre-filled: activation-typed, fp32 activation-shaped, fp64 [2, C], fp32 [C] x 4, fp32 weight gradient
    out = {k: torch.full((rows, c), SENTINEL, device=DEV).to(dt) for k in ("y", "y2")}
    out.update(d0=torch.full((2, c), SENTINEL, dtype=torch.float64, device=DEV), d1=torch.full((2, c), SENTINEL, dtype=torch.float64, device=DEV),
               small=torch.full((4, c), SENTINEL, device=DEV), dw=torch.full((1, c, c), SENTINEL, device=DEV))
    before = {k: v.clone() for k, v in out.items()}
    y, y2, d0, d1, small, dw = (out[k] for k in ("y", "y2", "d0", "d1", "small", "dw"))
    f32flag = (C.c_int32(0),) if h else ()                             # (the bf16 conv entry points take the result's type)

    def mix(b):
        return C.byref(ops._MixRef(x.data_ptr(), b.c(), ops.RES_A, ops.RES_B))

    # entry point -> (number of references it takes, call(*references))
    sites = {
        "conv_fwd": (1, lambda a: getattr(lib, "mopoe_conv_fwd" + sfx)(p(x), p(w), p(bias), p(y), *f32flag, gr, bn(a), nomask, p(d0), None, None, nil, st)),
        "conv_fwd_mix": (2, lambda a, b: getattr(lib, "mopoe_conv_fwd_mix" + sfx)(p(x), p(w), p(bias), p(y), gr, bn(a), nomask, mix(b), p(d0), None, None, nil, st)),
        "conv_dgrad": (1, lambda a: getattr(lib, "mopoe_conv_dgrad" + sfx)(p(x), p(w), p(y), *f32flag, gr, bn(a), p(x), p(d0), None, None, nil, st)),
        "conv_wgrad": (1, lambda a: getattr(lib, "mopoe_conv_wgrad" + sfx)(p(x), p(x), p(dw), gr, bn(a), C.c_int32(0), None, st)),
        "block_out_fwd": (1, lambda a: getattr(lib, "mopoe_block_out_fwd" + sfx)(p(x), p(x), p(y), R, c, bn(a), f(2.0), f(0.3), p(d0), st)),
        "bn_relu_apply": (1, lambda a: getattr(lib, "mopoe_bn_relu_apply" + sfx)(p(x), p(y), R, c, bn(a), st)),
        "bn_bwd_reduce": (1, lambda a: getattr(lib, "mopoe_bn_bwd_reduce" + sfx)(p(x), p(x), R, c, bn(a), p(d0), st)),
        "block_out_bwd": (1, lambda a: getattr(lib, "mopoe_block_out_bwd" + sfx)(p(x), p(x), p(y), p(y2), R, c, bn(a), p(sums_in), nomask, f(2.0), f(0.3),
                                                                                p(small[0]), p(small[1]), p(small[2]), p(small[3]), st)),
        "bn_bwd_apply": (2, lambda a, b: getattr(lib, "mopoe_bn_bwd_apply" + sfx)(p(x), p(x), None, p(y), R, c, bn(a), p(sums_in), nomask, p(small[0]), p(small[1]),
                                                                                  p(small[2]), p(x), bn(b), p(d0), st)),
        "block_front_stats": (1, lambda a: getattr(lib, "mopoe_block_front_stats" + sfx)(p(x), p(w), p(bias), R, c, bn(a), nomask, p(d0), st)),
        "block_front_apply": (2, lambda a, b: getattr(lib, "mopoe_block_front_apply" + sfx)(p(x), p(w), p(bias), p(y), R, c, bn(a), bn(b), nomask, st)),
        "block_front_bwd": (2, lambda a, b: getattr(lib, "mopoe_block_front_bwd" + sfx)(p(x), p(x), p(w), p(bias), p(y), R, c, bn(a), bn(b), nomask, p(sums_in), p(d1),
                                                                                        p(dw), p(small[2]), p(small[0]), p(small[1]), st)),
    }
    for name, (nref, call) in sites.items():
        for slot in range(nref):
            for label, bad in broken.items():
                if name == "conv_dgrad" and label == "mode 3":
                    continue                                           # (allowed there; below: refused without xin)
                refs = [good] * nref
                refs[slot] = bad
                rc = call(*refs)
                msg = lib.mopoe_last_error().decode()
                assert rc == ERR_ARG, (name + sfx, slot, label, rc, msg)
                assert f"mopoe_{name}{sfx}" in msg, (name + sfx, slot, label, msg)
        for k, v in out.items():
            assert torch.equal(v, before[k]), (name + sfx, k)
    # relu_bn of the input gradient: any present mode needs xin, mode 3 included; a mode-1 reference needs a count
    for label, ref in (("mode 3", broken["mode 3"]), ("mode 1", good)):
        rc = getattr(lib, "mopoe_conv_dgrad" + sfx)(p(x), p(w), p(y), *f32flag, gr, bn(ref), None, p(d0), None, None, nil, st)
        assert rc == ERR_ARG and "xin" in lib.mopoe_last_error().decode(), (label, rc, lib.mopoe_last_error().decode())
    rc = getattr(lib, "mopoe_conv_dgrad" + sfx)(p(x), p(w), p(y), *f32flag, gr, bn(Bn(good.gamma, good.beta, 1, sums=good.sums, count=0)), p(x), p(d0),
                                                None, None, nil, st)
    assert rc == ERR_ARG and "inv_count" in lib.mopoe_last_error().decode(), (rc, lib.mopoe_last_error().decode())
    # ... and through the Python layer a refusal is a MopoeHipError
    with pytest.raises(ops.MopoeHipError):
        ops.bn_relu_apply(x, broken["mode 1 without sums"])
    with pytest.raises(ops.MopoeHipError):
        ops.conv_wgrad(x.view(g.in_shape), x.view(g.out_shape), g, bn_in=broken["mode 3"])
    torch.cuda.synchronize()
    for k, v in out.items():
        assert torch.equal(v, before[k]), k


# ---------------------------------------------------------------------------------------------------------------
# the block front with running statistics
# ---------------------------------------------------------------------------------------------------------------
FRONT_MODES = [(2, 2), (2, 1), (1, 2)]       # (bn1, bn2); (2, 2) is what a step in eval mode does
FRONT_SHAPES = [(3, 64, True), (5, 32, True)]


@pytest.mark.parametrize("mode1,mode2", FRONT_MODES, ids=[f"bn1mode{a}_bn2mode{b}" for a, b in FRONT_MODES])
@pytest.mark.parametrize("n,rps,drop", FRONT_SHAPES)
def test_block_front_running_statistics_f32(n, rps, drop, mode1, mode2):
    front_case_f32(n, rps, drop, mode1, mode2)


@pytest.mark.parametrize("mode1,mode2", FRONT_MODES, ids=[f"bn1mode{a}_bn2mode{b}" for a, b in FRONT_MODES])
@pytest.mark.parametrize("n,rps,drop", FRONT_SHAPES)
def test_block_front_running_statistics_bf16(n, rps, drop, mode1, mode2):
    front_case_bf16(n, rps, drop, mode1, mode2)


# ---------------------------------------------------------------------------------------------------------------
# mode 3 at small |gamma| and large |beta|
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gabs,beta", M3.SETTINGS, ids=[f"gamma{g}_beta{b}" for g, b in M3.SETTINGS])
def test_mode3_bound_at_small_gamma_large_beta_bf16(gabs, beta):
    """conv_dgrad_bf16 with a mode-3 reference on the stored a2 against fp64: on the same a2 at the project's bars (the
    kernel's arithmetic at awkward coefficients), and against the exact x-hat from d1 at the DERIVED bound of what the
    bf16-rounded a2 can cost (tests/bn_mode3_cases.py; the CPU half runs the emulation on the same numbers).
    Logged, not gated: that error against the error of the mode-1 path reading a bf16 d1."""
    case, g = M3.Mode3Case(gabs, beta), M3.GEOM
    dy, w = case.dy.to(DEV), case.w.to(DEV)
    sums = torch.zeros(2, g.Cin, dtype=torch.float64, device=DEV)
    dx = ops.conv_dgrad(dy, w, g, relu_bn=to_dev(case.bn2y), xin=case.a2.to(DEV), bwd_sums=sums)
    assert dx.dtype == BF
    M3.assert_mode3(case, dx.cpu(), sums.cpu(), f"kernel |gamma|={gabs} beta={beta}")
    sums1 = torch.zeros(2, g.Cin, dtype=torch.float64, device=DEV)
    ops.conv_dgrad(dy, w, g, relu_bn=to_dev(case.bn2), xin=case.d1.to(BF).to(DEV), bwd_sums=sums1)
    e3, e1 = M3.sums1_error(sums, case), M3.sums1_error(sums1, case)
    _log(f"mode3_vs_mode1 |gamma|={gabs} beta={beta}: sums[1] error / max|sums[1]|: mode 3 on a2 {e3:.3e}, mode 1 on bf16 d1 {e1:.3e}, "
         f"ratio {e3 / max(e1, 1e-30):.2f}")


# ---------------------------------------------------------------------------------------------------------------
# the whole model in eval mode, with gradients, at 64 channels
# ---------------------------------------------------------------------------------------------------------------
class Recorder:
    """wraps ops.conv_dgrad and ops.block_front_bwd (the real functions still run) and notes the references they were handed"""

    def __init__(self, monkeypatch):
        self.relu_bn, self.front_bn2 = [], []
        real_dgrad, real_front = ops.conv_dgrad, ops.block_front_bwd

        def conv_dgrad(dy, wp, g, relu_bn=None, xin=None, bwd_sums=None, out_dtype=None):
            if relu_bn is not None:
                self.relu_bn.append((relu_bn.mode, relu_bn.sums is None))
            return real_dgrad(dy, wp, g, relu_bn=relu_bn, xin=xin, bwd_sums=bwd_sums, out_dtype=out_dtype)

        def block_front_bwd(x, dh2, w1, bias, bn1, bn2, *args, **kw):
            self.front_bn2.append(bn2.mode)
            return real_front(x, dh2, w1, bias, bn1, bn2, *args, **kw)

        monkeypatch.setattr(ops, "conv_dgrad", conv_dgrad)
        monkeypatch.setattr(ops, "block_front_bwd", block_front_bwd)

    def mode3_without_sums(self):
        return (3, True) in self.relu_bn


def test_eval64_fp32_gradients_vs_reference(monkeypatch):
    """eval mode with gradients at 64 channels, fp32 family, default switches: d1 is written, the fused front backward runs
    with running statistics in bn2"""
    rec = Recorder(monkeypatch)
    check_fp32_case("eval64_b8")
    assert 2 in rec.front_bn2, rec.front_bn2
    assert not any(m == 3 for m, _ in rec.relu_bn)       # (no forward front in fp32 by default: conv2's gradient reads d1)


def test_eval64_fp32_forward_front_gradients_vs_reference(monkeypatch):
    """... with the fp32 forward front (MOPOE_BLOCK_FRONT_F32_FWD=1): d1 is never written, conv2's input gradient takes the
    mode-3 reference without statistics -- the fp32 mode-3 path"""
    monkeypatch.setattr(ops, "BLOCK_FRONT_F32_FWD", True)
    rec = Recorder(monkeypatch)
    check_fp32_case("eval64_b8")
    assert rec.mode3_without_sums(), rec.relu_bn
    assert 2 in rec.front_bn2, rec.front_bn2


def test_c2_fp32_forward_front_train_mode_vs_reference(monkeypatch):
    """the fp32 forward front in train mode at model level (BASELINE config #2's shape, B = 8)"""
    monkeypatch.setattr(ops, "BLOCK_FRONT_F32_FWD", True)
    rec = Recorder(monkeypatch)
    check_fp32_case("c2_b8")
    assert rec.mode3_without_sums(), rec.relu_bn
    assert rec.front_bn2 and set(rec.front_bn2) == {1}, rec.front_bn2      # (train mode: batch statistics)


def test_eval64_bf16_gradients_vs_oracle(monkeypatch):
    """eval mode with gradients at 64 channels, bf16 family (the streaming front is its default path)"""
    rec = Recorder(monkeypatch)
    check_bf16_case("eval64_b8_bf16", small_batch=True)
    assert rec.mode3_without_sums(), rec.relu_bn
    assert 2 in rec.front_bn2, rec.front_bn2


def test_small_bf16_eval_gradients_vs_oracle(monkeypatch):
    """the DIM 32 eval case, now with gradients (its second blocks have 64 channels: the front and mode 3 run there too)"""
    rec = Recorder(monkeypatch)
    check_bf16_case("small_bf16_eval", small_batch=True)
    assert rec.mode3_without_sums(), rec.relu_bn
    assert 2 in rec.front_bn2, rec.front_bn2
