"""Likelihood estimates of the factorized representation on the GPU: the two estimator kernels (ops.lhood_style_sample /
ops.lhood_estimates) against their torch restatement (tests/torch_backend_lhood.py), the whole estimator against the
reference's estimates (tests/golden/g10_lhood_style_*), and --calc_nll through the launcher."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import torch_backend_lhood as TBL
from golden_util import load
from test_lhood_style_cpu import MODS, lhood_exp, run_fixture
from mimic_amd import ops

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _rand(gen, *shape, lo=-1.0, hi=1.0):
    return (torch.rand(*shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo).float().to(DEV)


def _sample_inputs(gen, b, k, d, s):
    return (_rand(gen, b, d, lo=-2, hi=2), _rand(gen, b, d, lo=-6, hi=4), torch.randn(k, b, d, generator=gen).to(DEV),
            _rand(gen, b, s, lo=-2, hi=2), _rand(gen, b, s, lo=-6, hi=4), torch.randn(k, b, s, generator=gen).to(DEV))


def _check(name, got, ref, rtol, atol):
    np.testing.assert_allclose(got.double().cpu().numpy(), ref.double().cpu().numpy(), rtol=rtol, atol=atol, err_msg=name)


def test_lhood_style_sample_vs_restatement():
    """B in {1, 30, 65}, K in {1, 6, 10}, D in {8, 128}, S in {1, 8, 32, 64}, logvar in [-6, 4]"""
    gen = torch.Generator().manual_seed(3)
    for b, k, d, s in itertools.product((1, 30, 65), (1, 6, 10), (8, 128), (1, 8, 32, 64)):
        args = _sample_inputs(gen, b, k, d, s)
        zcat, t_c, t_s = ops.lhood_style_sample(*args)
        torch.cuda.synchronize()
        r_zcat, r_tc, r_ts = TBL.lhood_style_sample(*args)
        tag = f"B{b} K{k} D{d} S{s}"
        assert tuple(zcat.shape) == (k * b, s + d) and tuple(t_c.shape) == (k * b,) and tuple(t_s.shape) == (k * b,)
        _check("zcat " + tag, zcat, r_zcat, 2e-6, 1e-6)
        # (sums of D / S terms of magnitude up to ~exp(4) * 4: fp32 summation order)
        _check("t_c " + tag, t_c, r_tc, 1e-5, 2e-5 * float(r_tc.abs().max()) + 1e-4 * d)
        _check("t_s " + tag, t_s, r_ts, 1e-5, 2e-5 * float(r_ts.abs().max()) + 1e-4 * s)
        zcat2, t_c2, t_s2 = ops.lhood_style_sample(*args)
        assert torch.equal(zcat, zcat2) and torch.equal(t_c, t_c2) and torch.equal(t_s, t_s2), tag


def _est_inputs(gen, b, k):
    r = k * b
    lp = [_rand(gen, r, lo=-3000, hi=-1000) for _ in range(3)]
    return lp, _rand(gen, r, lo=-30, hi=30), _rand(gen, r, lo=-20, hi=20)


def test_lhood_estimates_vs_restatement():
    """every membership mask, t_s given and NULL; bit-identical on a second run"""
    gen = torch.Generator().manual_seed(5)
    for b, k in itertools.product((1, 30, 65), (1, 6, 10)):
        lp, t_c, t_s = _est_inputs(gen, b, k)
        for mask, ts in itertools.product(range(8), (t_s, None)):
            got = ops.lhood_estimates(lp, t_c, ts, k, mask)
            again = ops.lhood_estimates(lp, t_c, ts, k, mask)
            ref = TBL.lhood_estimates(lp, t_c, ts, k, mask)
            tag = f"B{b} K{k} mask{mask} t_s {'null' if ts is None else 'given'}"
            _check(tag, got, ref, 1e-6, 2e-3)
            assert torch.equal(got, again), tag


def test_lhood_estimates_keep_the_view_rule():
    """the importance weights are viewed as (batch_size, K) over the sample-major [K*B] vector, as the reference does:
    with weights that depend only on b, every view row mixes samples of different b -- the (K, B) grouping would give
    another answer"""
    b, k = 4, 6
    rows = torch.arange(k * b, device=DEV)
    per_b = torch.tensor([-100.0, -40.0, -10.0, -70.0], device=DEV)
    lp = [per_b[rows % b].contiguous() for _ in range(3)]
    zero = torch.zeros(k * b, device=DEV)
    got = ops.lhood_estimates(lp, zero, None, k, 7)
    ref = TBL.lhood_estimates(lp, zero, None, k, 7)
    _check("view rule", got, ref, 1e-6, 1e-4)
    lme = lambda x: torch.logsumexp(x, dim=1) - float(np.log(x.shape[1]))
    per_sample = lme(lp[0].view(k, b).t()).mean()          # what grouping the K samples of each b would give
    assert abs(got[0].item() - per_sample.item()) > 1.0
    assert abs(got[0].item() - lme(lp[0].view(b, k)).mean().item()) < 1e-3


@pytest.mark.parametrize("name", ["s64", "jsd_s64", "c2"])
def test_g10_estimator(name):
    """the estimator on the device (eval mode) against the reference's calc_log_likelihood_batch: every subset of the
    fixture x {PA, Lateral, text, joint}, 1e-4 rel + 1e-3 (G4's GPU tolerance)"""
    g = load(f"g10_lhood_style_{name}")
    exp, batch, k = lhood_exp(g, DEV)
    got = run_fixture(g, exp, batch, k, DEV)
    for key, (v, ref) in got.items():
        assert abs(v - ref) <= 1e-4 * abs(ref) + 1e-3, (key, v, ref)


def test_g10_estimator_bf16():
    """bf16 storage family (style dims 32) against g10_lhood_style_c2.  Loose tolerance, 2e-3 relative: the decoders run
    bf16 activations and bf16 MFMA products (fp32 accumulation) against the reference's fp32 decode (measured: at most
    1.8e-4 relative, on the image marginals)"""
    g = load("g10_lhood_style_c2")
    exp, batch, k = lhood_exp(g, DEV, compute_dtype="bf16")
    got = run_fixture(g, exp, batch, k, DEV)
    errs = {key: abs(v - ref) / abs(ref) for key, (v, ref) in got.items()}
    print("bf16 relative errors:", json.dumps({f"{s}/{m}": e for (s, m), e in errs.items()}))
    for key, (v, ref) in got.items():
        assert np.isfinite(v) and abs(v - ref) <= 2e-3 * abs(ref), (key, v, ref)


def test_char_encoding_factorized(monkeypatch):
    """text_encoding='char' (dense rows kernel for the text marginal): finite, and the same as the estimator with the two
    new ops replaced by their torch restatement"""
    from mimic_amd.evaluation.eval_metrics.likelihood import calc_log_likelihood_batch
    from mimic_amd.utils.experiment import HotPathExperiment, default_flags
    torch.manual_seed(0)
    b, k = 5, 6
    flags = default_flags(img_size=64, class_dim=16, DIM_img=8, DIM_text=8, batch_size=b, device=torch.device(DEV),
                          text_encoding="char", len_sequence=1024, num_features=71, factorized_representation=True,
                          style_pa_dim=8, style_lat_dim=8, style_text_dim=8)
    exp = HotPathExperiment(flags)
    exp.mm_vae.to(DEV).eval()
    ids = torch.randint(0, 71, (b, 1024))
    batch = {"PA": torch.rand(b, 1, 64, 64, device=DEV), "Lateral": torch.rand(b, 1, 64, 64, device=DEV),
             "text": torch.nn.functional.one_hot(ids, 71).float().to(DEV)}
    gen = torch.Generator().manual_seed(1)
    eps = torch.randn(k, b, 16, generator=gen).to(DEV)
    eps_style = {m: torch.randn(k, b, 8, generator=gen).to(DEV) for m in MODS}
    with torch.no_grad():
        lat = exp.mm_vae.inference(dict(batch))
        outs = []
        for patch in (False, True):
            if patch:
                for name in TBL.OP_NAMES:
                    monkeypatch.setattr(ops, name, getattr(TBL, name))
            outs.append({s: calc_log_likelihood_batch(exp, lat, s, exp.subsets[s], batch, k, eps=eps, eps_style=eps_style)
                         for s in ("text", "Lateral_PA", "Lateral_PA_text")})
    for s in outs[0]:
        for m in outs[0][s]:
            v, ref = outs[0][s][m].item(), outs[1][s][m].item()
            assert np.isfinite(v) and abs(v - ref) <= 1e-5 * abs(ref) + 1e-3, (s, m, v, ref)


def _launcher(tmp_path, *extra, timeout=600):
    env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0").split(",")[0],
               PYTHONPATH=os.pathsep.join([os.path.join(REPO, "mopoe-mimic_amd"), os.environ.get("PYTHONPATH", "")]))
    argv = [sys.executable, "-m", "mimic_amd.main_mimic", "--img_size", "64", "--class_dim", "64", "--DIM_img", "64",
            "--batch_size", "8", "--initial_learning_rate", "1e-5",
            "--dir_experiment_run", str(tmp_path / "run"), *extra]
    out = subprocess.run(["timeout", "-k", "10", str(timeout), *argv], env=env, cwd=REPO, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def _check_lhoods(lh):
    assert set(lh) == {"PA", "Lateral", "text", "Lateral_PA", "PA_text", "Lateral_text", "Lateral_PA_text"}
    for d in lh.values():
        assert set(d) == {"PA", "Lateral", "text", "joint"} and all(np.isfinite(v) for v in d.values())


def test_launcher_factorized_calc_nll(tmp_path):
    """2 epochs at eval_freq 1: the estimate after each epoch, and epoch 1 still replays the captured train step"""
    res = _launcher(tmp_path, "--end_epoch", "2", "--eval_freq", "1", "--factorized_representation", "true",
                    "--style_pa_dim", "8", "--style_lat_dim", "8", "--style_text_dim", "8", "--calc_nll", "true")
    assert res["epochs"] == 2 and res["graphed_steps_last_epoch"] > 0
    _check_lhoods(res["last_lhoods"])
    with open(tmp_path / "run" / "history.json") as f:
        hist = json.load(f)
    assert all("lhoods" in h["test"] for h in hist)


def test_launcher_calc_nll_non_factorized(tmp_path):
    res = _launcher(tmp_path, "--end_epoch", "1", "--calc_nll", "true")
    _check_lhoods(res["last_lhoods"])
