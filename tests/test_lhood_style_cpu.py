"""Likelihood estimates of the factorized representation and the --calc_nll epoch hook, on CPU: host logic with the HIP
ops replaced by their torch restatements (tests/torch_backend*.py, torch_backend_lhood.py), against the reference's own
estimates (tests/golden/g10_lhood_style_*, written by tests/tools/gen_golden_lhood_style.py); the flags; run_epochs."""
import numpy as np
import pytest
import torch

import model_util
import mopoe_ref as R
import style_util as SU
import torch_backend_lhood
from golden_util import cfg_from, load
from mimic_amd import main_mimic as MM
from mimic_amd import run_epochs as RE
from mimic_amd.plugins import FusedLaplace
from mimic_amd.utils.experiment import HotPathExperiment, default_flags

MODS = ("PA", "Lateral", "text")
FLAG_NAMES = ("style_pa_dim", "style_lat_dim", "style_text_dim")


def lhood_exp(g, device="cpu", compute_dtype="fp32"):
    """the fixture's factorized model in eval mode, its test batch and its K"""
    cfg = cfg_from(g["cfg"])
    sd, dims = SU.g9_state(g, cfg)
    with SU.style_flags(dims, str(g["method"])):
        exp = model_util.build_exp(cfg, sd, device, "eval", compute_dtype=compute_dtype)
    batch, _ = R.synthetic_batch(cfg, cfg.batch_size, seed=int(g["seed_batch"]))
    return exp, {m: v.to(device) for m, v in batch.items()}, int(g["K"])


def run_fixture(g, exp, batch, k, device="cpu"):
    """-> {(subset, value): (estimate, reference)} for every subset of the fixture"""
    from mimic_amd.evaluation.eval_metrics.likelihood import calc_log_likelihood_batch
    out = {}
    with torch.no_grad():
        lat = exp.mm_vae.inference(dict(batch))
        for s_key in [str(s) for s in g["subsets"]]:
            eps_style = {m: torch.from_numpy(g[f"{s_key}/eps_style/{m}"]).to(device) for m in MODS}
            ll = calc_log_likelihood_batch(exp, lat, s_key, exp.subsets[s_key], batch, num_imp_samples=k,
                                           eps=torch.from_numpy(g[f"{s_key}/eps"]).to(device), eps_style=eps_style)
            assert list(ll) == ["PA", "Lateral", "text", "joint"]
            for m_key, v in ll.items():
                out[(s_key, m_key)] = (v.item(), float(g[f"{s_key}/{m_key}"]))
    return out


@pytest.mark.parametrize("name", ["s64", "jsd_s64"])
def test_g10_estimator_host(monkeypatch, name):
    """every subset x {PA, Lateral, text, joint} against the reference's calc_log_likelihood_batch (G4's tolerance)"""
    torch_backend_lhood.install(monkeypatch)
    g = load(f"g10_lhood_style_{name}")
    exp, batch, k = lhood_exp(g)
    got = run_fixture(g, exp, batch, k)
    assert len(got) == 7 * 4
    for key, (v, ref) in got.items():
        assert abs(v - ref) <= 2e-5 * abs(ref) + 2e-4, (key, v, ref)


def test_g10_quirk_is_visible():
    """the fixture pins the reference's quirk: a subset's marginal of a NON-member modality still differs between subsets
    whose last members differ (the decoders read the last member's style sample)"""
    g = load("g10_lhood_style_s64")
    assert float(g["PA/text"]) != float(g["Lateral/text"])
    assert len({float(g[f"{s}/joint"]) for s in g["subsets"]}) == 7


def _unequal_exp():
    cfg = R.Cfg(img_size=64, class_dim=8, DIM_img=4, DIM_text=4, vocab_size=50, batch_size=4)
    dims = (3, 5, 2)
    sd = SU.style_state(cfg, R.init_state(cfg, seed=1), dims, 5)
    return SU.build_exp(cfg, sd, "cpu", "eval", dims=dims), cfg


def test_unequal_style_dims_raise_in_estimator(monkeypatch):
    torch_backend_lhood.install(monkeypatch)
    from mimic_amd.evaluation.eval_metrics.likelihood import calc_log_likelihood_batch
    exp, cfg = _unequal_exp()
    batch, _ = R.synthetic_batch(cfg, 4, seed=3)
    with torch.no_grad():
        lat = exp.mm_vae.inference(dict(batch))
        with pytest.raises(ValueError) as e:
            calc_log_likelihood_batch(exp, lat, "PA", exp.subsets["PA"], batch, num_imp_samples=3)
    assert all(f in str(e.value) for f in FLAG_NAMES)


def test_unequal_style_dims_raise_at_set_up_with_calc_nll():
    kw = dict(img_size=64, class_dim=8, DIM_img=4, DIM_text=4, vocab_size=50, batch_size=4, device=torch.device("cpu"),
              factorized_representation=True, style_pa_dim=3, style_lat_dim=5, style_text_dim=2)
    HotPathExperiment(default_flags(**kw))        # training alone runs with unequal dims
    with pytest.raises(ValueError) as e:
        HotPathExperiment(default_flags(calc_nll=True, **kw))
    assert all(f in str(e.value) for f in FLAG_NAMES)
    argv = ["--factorized_representation", "true", "--calc_nll", "true", "--style_pa_dim", "8", "--style_lat_dim", "8",
            "--style_text_dim", "16"]
    with pytest.raises(ValueError) as e:
        MM.Main(MM.parse_flags(argv))
    assert all(f in str(e.value) for f in FLAG_NAMES)


def test_public_functions_with_style_dicts(monkeypatch):
    """utils.likelihood.get_latent_samples / log_marginal_estimate / log_joint_estimate with style dicts against the
    reference's functions on the same tensors"""
    torch_backend_lhood.install(monkeypatch)
    from types import SimpleNamespace
    from mimic_amd.utils.likelihood import get_latent_samples, log_joint_estimate, log_marginal_estimate
    g = load("g10_lhood_style_pub")
    t = lambda k: torch.from_numpy(g["in/" + k])
    k, b = int(g["K"]), int(g["B"])
    flags = SimpleNamespace(batch_size=b, factorized_representation=True, device=torch.device("cpu"))
    lat = get_latent_samples(flags, {"content": (t("mu"), t("logvar")),
                                     "style": {m: (t(f"style/{m}/mu"), t(f"style/{m}/logvar")) for m in MODS}},
                             k, MODS, eps=t("eps"), eps_style={m: t(f"style/{m}/eps") for m in MODS})
    assert list(lat["style"]) == list(MODS) and tuple(lat["style"]["text"]["z"].shape) == (k, b, 4)
    flat = lambda d: {key: v.reshape(k * b, -1) for key, v in d.items()}
    content = flat(lat["content"])
    styles = {m: flat(lat["style"][m]) for m in MODS}
    scale = float(g["scale"])
    lh = {m: FusedLaplace(t(f"loc/{m}"), scale) for m in MODS}
    got = {"marginal/PA": log_marginal_estimate(flags, k, lh["PA"], t("target/PA"), styles["PA"], content),
           "marginal/Lateral_nostyle": log_marginal_estimate(flags, k, lh["Lateral"], t("target/Lateral"), None, content),
           "joint": log_joint_estimate(flags, k, lh, {m: t(f"target/{m}") for m in MODS}, styles, content)}
    for key, v in got.items():
        ref = float(g[key])
        assert abs(v.item() - ref) <= 2e-5 * abs(ref) + 2e-4, (key, v.item(), ref)


def test_calc_nll_flag():
    assert MM.parse_flags([]).calc_nll is False
    assert MM.parse_flags(["--calc_nll", "true"]).calc_nll is True
    assert default_flags(device=None).calc_nll is False


def test_launcher_result_line():
    """the default output is unchanged; last_lhoods comes from the latest epoch that estimated"""
    h = lambda e, **t: {"epoch": e, "train": {"graphed_steps": 3}, "test": {"total_loss": 1.5, **t}}
    assert MM.result_line([h(0), h(1)]) == {"epochs": 2, "last_test_loss": 1.5, "graphed_steps_last_epoch": 3}
    lh = {"PA": {"PA": -1.0, "Lateral": -2.0, "text": -3.0, "joint": -6.0}}
    assert MM.result_line([h(0, lhoods=lh), h(1)])["last_lhoods"] == lh


def _run_exp(tmp_path, **kw):
    cfg = R.Cfg(img_size=64, class_dim=8, DIM_img=4, DIM_text=4, vocab_size=50, batch_size=4)
    dims = (4, 4, 4)
    sd = SU.style_state(cfg, R.init_state(cfg, seed=1), dims, 5)
    exp = SU.build_exp(cfg, sd, "cpu", "train_nodrop", dims=dims)
    f = exp.flags
    f.calc_nll, f.dataloader_workers, f.dir_checkpoints = True, 0, str(tmp_path / "ckpt")
    f.__dict__.update(kw)
    return exp


def test_run_epochs_calc_nll(monkeypatch, tmp_path):
    """eval_freq 2, end_epoch 3: the estimate runs after epochs 1 and 2 (every eval_freq-th and the last epoch), over
    the synthetic test split at batch size 30; flags.batch_size comes back"""
    torch_backend_lhood.install(monkeypatch)
    exp = _run_exp(tmp_path, eval_freq=2, end_epoch=3)
    history = RE.run_epochs("cpu", exp)
    assert [h["epoch"] for h in history] == [0, 1, 2]
    assert ["lhoods" in h["test"] for h in history] == [False, True, True]
    for h in history[1:]:
        lh = h["test"]["lhoods"]
        assert set(lh) == {"PA", "Lateral", "text", "Lateral_PA", "PA_text", "Lateral_text", "Lateral_PA_text"}
        vals = [v for d in lh.values() for v in d.values()]
        assert all(set(d) == {"PA", "Lateral", "text", "joint"} for d in lh.values())
        assert len(vals) == 28 and all(np.isfinite(vals))
    assert exp.flags.batch_size == 4


def test_calc_nll_skips_a_small_test_split(monkeypatch, tmp_path, capsys):
    torch_backend_lhood.install(monkeypatch)
    exp = _run_exp(tmp_path, testing_batches=0)
    assert RE.estimate_test_likelihoods(exp, 0) is None
    assert "skipped" in capsys.readouterr().out
    assert exp.flags.batch_size == 4
