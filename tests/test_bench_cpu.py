"""bench.py --dump-outputs on CPU: the files stay within the 64 MB budget, small arrays are written whole, large ones as
the same seeded sample on every run; the extra measurements are behind --full."""
import os

import numpy as np
import pytest
import torch

import bench


def _arrays():
    g = torch.Generator().manual_seed(0)
    return {"total_loss": torch.tensor(1.5), "latents.z": torch.randn(64, 128, generator=g),
            "state.big": torch.randn(3, 1000, 1000, generator=g), "grad.big": torch.randn(2_000_000, generator=g),
            "rec.PA.loc": torch.rand(64, 1, 128, 128, generator=g).to(torch.bfloat16)}


def test_dump_budget_and_determinism(tmp_path):
    arrays = _arrays()
    budget = 4 * 2 ** 20
    n, whole = bench.write_outputs(arrays, str(tmp_path / "a"), budget=budget)
    bench.write_outputs(_arrays(), str(tmp_path / "b"), budget=budget)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(k + ".npy" for k in arrays) and n == len(arrays) and whole == 2
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b), f
    assert np.load(tmp_path / "a" / "total_loss.npy").shape == () and float(np.load(tmp_path / "a" / "total_loss.npy")) == 1.5
    z = np.load(tmp_path / "a" / "latents.z.npy")
    assert np.array_equal(z, arrays["latents.z"].numpy())
    big = np.load(tmp_path / "a" / "grad.big.npy")
    assert big.ndim == 1 and 0 < big.size < 2_000_000
    assert np.isin(big, arrays["grad.big"].numpy()).all()       # a sample of the array's own elements
    loc = np.load(tmp_path / "a" / "rec.PA.loc.npy")
    assert np.isin(loc, arrays["rec.PA.loc"].float().numpy()).all()


def test_dump_fits_the_budget_at_the_default_size(tmp_path):
    arrays = {f"a{i}": torch.zeros(n) for i, n in enumerate([1, 100, 10 ** 5, 10 ** 7, 3 * 10 ** 7])}
    bench.write_outputs(arrays, str(tmp_path))
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 * 10 ** 6


def test_full_is_off_by_default():
    """a plain run measures only the headline; the roofline pass, the CPU baseline and the host-cost steps need --full"""
    plain = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert plain.full is False and (plain.steps, plain.warmup, plain.dump_outputs) == (5, 2, None)
    full = bench.parse_args(["--full", "--no-cpu-baseline"])
    assert full.full is True and full.no_cpu_baseline is True and full.no_roofline is False
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def _one_step_outputs(monkeypatch):
    import mopoe_ref as R
    import torch_backend
    from model_util import build_exp
    from mimic_amd import run_epochs as RE
    torch_backend.install(monkeypatch)
    cfg = R.Cfg(img_size=64, class_dim=8, DIM_img=4, DIM_text=4, vocab_size=50, batch_size=4)
    exp = build_exp(cfg, R.init_state(cfg, seed=1), "cpu", "train")
    exp.mm_vae.set_mask_replay(None)
    exp.set_optimizer()
    pack = RE.ScalarPack(torch.device("cpu"))
    torch.manual_seed(3)
    routine = RE.train_step(exp, (R.synthetic_batch(cfg, 4, seed=2)[0], None), None, pack)
    with torch.no_grad():
        return bench.step_outputs(routine), pack.read(), exp


def test_step_outputs_of_a_train_step(monkeypatch, tmp_path):
    """what --dump-outputs collects from one train step (HIP ops replaced by their torch emulation): the loss terms, latents
    and reconstructions the step returns; the same seeds give the same files"""
    out, scalars, exp = _one_step_outputs(monkeypatch)
    assert float(out["total_loss"]) == pytest.approx(scalars["total_loss"], rel=1e-6)
    for k in ("joint_divergence", "latents.z", "latents.joint.mu", "latents.PA.mu", "rec.PA.loc", "rec.Lateral.loc"):
        assert k in out, k
    assert {k for k in out if k.startswith("klds.") or k.startswith("log_probs.")} == \
        {n.replace("/", ".") for n in scalars if n.startswith("klds/") or n.startswith("log_probs/")}
    assert out["rec.text.logits"].shape == (4, exp.flags.len_sequence, 50)
    assert all("/" not in k for k in out)
    n, _ = bench.write_outputs(out, str(tmp_path / "a"))
    assert n == len(out) == len(os.listdir(tmp_path / "a"))
    bench.write_outputs(_one_step_outputs(monkeypatch)[0], str(tmp_path / "b"))
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
