"""method='moe' (MMVAE) and method='jsd' (mixture of experts with a dynamic prior): host logic on CPU, with the HIP ops
replaced by their torch restatements (tests/torch_backend.py, tests/torch_backend_methods.py), against the reference's
own outputs for the two methods (tests/golden/g8_*, written by tests/tools/gen_golden_methods.py); the --method switch;
the compact fixture format (tests/methods_util.py)."""
import numpy as np
import pytest
import torch

import mopoe_ref as R
import torch_backend_methods
from golden_util import load, cfg_from, g0_masks
from methods_util import METHODS, build_exp, check_against_g8_g0, g8_batch, g8_state
from test_host_logic_cpu import close
from mimic_amd import main_mimic as MM
from mimic_amd import run_epochs as RE
from mimic_amd.utils.experiment import default_flags


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("mode", ["eval", "train_nodrop", "train"])
def test_g8_g0_host_logic(monkeypatch, method, mode):
    torch_backend_methods.install(monkeypatch)
    g = load(f"g8_{method}_g0_s64")
    cfg = cfg_from(g["cfg"])
    exp = build_exp(method, cfg, g8_state(g, cfg), "cpu", mode,
                    masks=g0_masks(g) if mode == "train" else None, eps=torch.from_numpy(g[f"{mode}/eps"]))
    out = check_against_g8_g0(exp, g, mode, g8_batch(g, cfg))
    res = out["results"]
    n_comp = 3 + (method == "jsd")
    assert tuple(res["individual_divs"].shape) == (n_comp,) and tuple(res["latents"]["mus"].shape) == (n_comp, 4, 8)
    assert len(out["klds"]) == 7
    if method == "moe":
        assert res["dyn_prior"] is None
    else:
        pd_mu, pd_lv = res["dyn_prior"]
        assert tuple(pd_mu.shape) == tuple(pd_lv.shape) == (4, 8)
        # the prior component is N(0, I) and the joint's rows taken from it are z = eps
        lat = res["latents"]
        assert float(lat["mus"][3].detach().abs().max()) == 0.0 and float(lat["logvars"][3].detach().abs().max()) == 0.0


@pytest.mark.parametrize("method", METHODS)
def test_g8_partial_modalities_inference(monkeypatch, method):
    torch_backend_methods.install(monkeypatch)
    g = load(f"g8_{method}_partial")
    cfg = cfg_from(g["partial/cfg"])
    sd = R.init_state(cfg, seed=int(g["partial/seed_weights"]))
    batch, _ = R.synthetic_batch(cfg, cfg.batch_size, seed=int(g["partial/seed_batch"]))
    exp = build_exp(method, cfg, sd, "cpu", "eval")
    for combo in (("PA",), ("text",), ("PA", "text"), ("Lateral", "text"), ("PA", "Lateral")):
        tag = "+".join(combo)
        with torch.no_grad():
            lat = exp.mm_vae.inference({m: batch[m] for m in combo})
        assert list(lat["subsets"].keys()) == list(g[f"partial/{tag}/keys"])
        close(lat["mus"], g[f"partial/{tag}/mus"])
        close(lat["logvars"], g[f"partial/{tag}/logvars"])
        close(lat["weights"], g[f"partial/{tag}/weights"])
        close(lat["joint"][0], g[f"partial/{tag}/joint_mu"])
        close(lat["joint"][1], g[f"partial/{tag}/joint_logvar"])


@pytest.mark.parametrize("method", METHODS)
def test_g8_adam_trajectory_host(monkeypatch, method):
    torch_backend_methods.install(monkeypatch)
    g = load(f"g8_{method}_traj")
    cfg = cfg_from(g["cfg"])
    exp = build_exp(method, cfg, R.init_state(cfg, seed=int(g["seed_weights"])), "cpu", "train_nodrop")
    exp.flags.initial_learning_rate = float(g["lr"])
    exp.set_optimizer()
    losses = []
    for step in range(3):
        batch, _ = R.synthetic_batch(cfg, cfg.batch_size, seed=20 + step)
        e = torch.from_numpy(g["eps"][step])
        exp.mm_vae.eps_source = lambda b, d, dev, e=e: e
        out = RE.train_step(exp, (batch, None))
        losses.append(out["total_loss"].item())
    np.testing.assert_allclose(losses, g["losses"], rtol=2e-5)
    sd = exp.mm_vae.state_dict()
    close(sd["encoder_pa.feature_extractor.conv1.weight"], g["final/encoder_pa.feature_extractor.conv1.weight"],
          1e-4, 1e-6)


@pytest.mark.parametrize("method", METHODS)
def test_g8_likelihood_estimator_host(monkeypatch, method):
    torch_backend_methods.install(monkeypatch)
    from mimic_amd.evaluation.eval_metrics.likelihood import calc_log_likelihood_batch
    g = load(f"g8_{method}_likelihood")
    cfg = cfg_from(g["cfg"])
    sd = R.init_state(cfg, seed=int(g["seed_weights"]))
    batch, _ = R.synthetic_batch(cfg, cfg.batch_size, seed=int(g["seed_batch"]))
    exp = build_exp(method, cfg, sd, "cpu", "eval")
    with torch.no_grad():
        lat = exp.mm_vae.inference(dict(batch))
        for s_key in ("PA", "text", "Lateral_text", "Lateral_PA_text"):
            ll = calc_log_likelihood_batch(exp, lat, s_key, exp.subsets[s_key], batch, num_imp_samples=int(g["K"]),
                                           eps=torch.from_numpy(g[f"{s_key}/eps"]))
            for m_key, v in ll.items():
                ref = float(g[f"{s_key}/{m_key}"])
                assert abs(v.item() - ref) <= 2e-5 * abs(ref) + 2e-4, (s_key, m_key, v.item(), ref)


@pytest.mark.parametrize("method", ["poe", "moe", "jsd", "joint_elbo"])
def test_parse_flags_method(method):
    f = MM.parse_flags(["--method", method])
    flags = {"poe": f.modality_poe, "moe": f.modality_moe, "jsd": f.modality_jsd, "joint_elbo": f.joint_elbo}
    assert flags == {m: m == method for m in flags}
    assert f.poe_unimodal_elbos == (method == "poe")
    assert f.device is None


def test_get_method_through_the_alias_package():
    from mimic.utils.filehandling import get_method
    from mimic_amd.utils import filehandling
    assert get_method is filehandling.get_method
    f = default_flags(device=torch.device("cpu"), method="jsd")
    get_method(f)
    assert f.modality_jsd and not (f.joint_elbo or f.modality_moe or f.modality_poe)
    f.method = "mvae"
    with pytest.raises(NotImplementedError):
        get_method(f)


def test_default_flags_still_mean_joint_elbo():
    f = default_flags(device=torch.device("cpu"))
    assert f.method == "joint_elbo" and f.joint_elbo
    assert not (f.modality_poe or f.modality_moe or f.modality_jsd or f.poe_unimodal_elbos)
    f = MM.parse_flags([])
    assert f.method == "joint_elbo" and f.joint_elbo and not (f.modality_poe or f.modality_moe or f.modality_jsd)


def test_poe_raises_with_the_reason(monkeypatch):
    torch_backend_methods.install(monkeypatch)
    g = load("g8_moe_g0_s64")
    cfg = cfg_from(g["cfg"])
    with pytest.raises(NotImplementedError, match="KeyError"):
        build_exp("poe", cfg, g8_state(g, cfg), "cpu")


def test_restatement_matches_the_fixture_latents():
    """the torch restatement itself against the reference's latent outputs (the GPU tests compare the kernels with it)"""
    from mimic_amd.mmvae import kl_weights, mixture_row_starts
    for method in METHODS:
        g = load(f"g8_{method}_g0_s64")
        mu_in = [torch.from_numpy(g[f"eval/enc/{m}/mu"]) for m in R.MOD_ORDER]
        lv_in = [torch.from_numpy(g[f"eval/enc/{m}/logvar"]) for m in R.MOD_ORDER]
        b = mu_in[0].shape[0]
        c = 3 + (method == "jsd")
        w = kl_weights(3) if method == "moe" else [0.25] * 4
        outs = torch_backend_methods.latent_mixture_fwd(method, mu_in, lv_in, torch.from_numpy(g["eval/eps"]),
                                                        [mixture_row_starts(b, m) for m in (1, 2, 3)],
                                                        mixture_row_starts(b, c), w, float(b))
        close(outs[2], g["eval/mus"])
        close(outs[4], g["eval/joint/mu"])
        close(outs[8], g["eval/individual_divs"])
        close(outs[9], g["eval/joint_divergence"])


def test_compact_gradient_check_catches_a_wrong_gradient():
    """methods_util.check_grads (sketched gradients of the G0 fixtures) passes the reference's own gradients and fails a
    gradient with one element off by 30 % of its tensor's largest, sketched or exact"""
    import methods_util as MU
    gen = torch.Generator().manual_seed(3)
    grads = {"a.weight": torch.randn(4, 8, generator=gen), "a.bias": torch.randn(4, generator=gen) * 1e-3,
             "b.weight": torch.randn(64, 40, generator=gen), "c.weight": torch.randn(5, 3, generator=gen)}
    names = sorted(grads)
    store = {"grad_names": np.array(names), "grad_numel": np.array([grads[n].numel() for n in names])}
    MU.pack_grads(store, "m", grads, names)
    assert store["m/grad_sketch"].shape == (1, MU.GRAD_SKETCH)
    MU.check_grads(store, "m", {n: t * (1 + 1e-5) for n, t in grads.items()})
    for bad in ("b.weight", "c.weight"):
        wrong = dict(grads)
        wrong[bad] = grads[bad].clone()
        wrong[bad][1] += 0.3 * grads[bad].abs().max()
        with pytest.raises(AssertionError):
            MU.check_grads(store, "m", wrong)


@pytest.mark.parametrize("method", METHODS)
def test_g8_fixture_inputs_regenerate(method):
    """the compact fixtures' weights and images come back from their seeds (fingerprint and checksum checked inside)"""
    for name in ("g0_s64", "c2"):
        g = load(f"g8_{method}_{name}")
        cfg = cfg_from(g["cfg"])
        if "seed_weights" in g.files and "sd_fingerprint" in g.files:
            sd = g8_state(g, cfg)
            assert len(sd) > 500
        batch = g8_batch(g, cfg)
        assert tuple(batch["PA"].shape) == (int(g["cfg"][5]), 1, cfg.img_size, cfg.img_size)
