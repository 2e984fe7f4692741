"""method='moe' (MMVAE) and method='jsd' (mixture of experts with a dynamic prior) on the GPU: the fused mixture latent
kernels (ops.latent_mixture_fwd / _bwd) against their torch restatement (tests/torch_backend_methods.py), and the whole
model against the reference's own outputs for the two methods (tests/golden/g8_*), with the tolerances of the joint_elbo
tests (test_model_gpu.py, test_bf16_gpu.py)."""
import numpy as np
import pytest
import torch

import mopoe_ref as R
import torch_backend_methods as TBM
from golden_util import load, cfg_from, g0_masks
from methods_util import METHODS, build_exp, check_against_g8_g0, g8_batch, g8_state
from test_host_logic_cpu import close
from mimic_amd import ops, run_epochs as RE
from mimic_amd.mmvae import kl_weights, mixture_row_starts

pytestmark = pytest.mark.gpu

SLOTS = ("PA", "Lateral", "text")
PRESENCE = [("PA",), ("text",), ("PA", "text"), ("Lateral", "text"), ("PA", "Lateral"), ("PA", "Lateral", "text")]
SHAPES = [(64, 128), (7, 8), (65, 64), (4, 8)]


def _mixture_args(method, n, b):
    c = n + (method == "jsd")
    w = kl_weights(n) if method == "moe" else [float(torch.tensor(1 / float(c)))] * c
    return [mixture_row_starts(b, m) for m in (1, 2, 3)], mixture_row_starts(b, c), w


def _cuda(ts):
    return [None if t is None else t.cuda() for t in ts]


def _close(name, got, ref, rtol=1e-5, atol_rel=1e-5):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    scale = max(ref.abs().max().item(), 1e-6)
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=rtol, atol=atol_rel * scale, err_msg=name)


@pytest.mark.parametrize("method", METHODS)
def test_latent_mixture_kernels_vs_restatement(method):
    names = ("sub_mu", "sub_lv", "comp_mu", "comp_lv", "joint_mu", "joint_lv", "z", "klds", "individual_divs",
             "joint_div", "pd_mu", "pd_lv")
    for combo in PRESENCE:
        for b, d in SHAPES:
            tag = f"{method} {'+'.join(combo)} B={b} D={d}"
            gen = torch.Generator().manual_seed(1000 * b + d + 7 * len(combo))
            rnd = lambda *shape, s=1.0: torch.randn(*shape, generator=gen) * s
            mu_in = [rnd(b, d) if m in combo else None for m in SLOTS]
            lv_in = [rnd(b, d, s=0.7) if m in combo else None for m in SLOTS]
            eps = rnd(b, d)
            mrs, crs, w = _mixture_args(method, len(combo), b)
            norm = 64.0
            got = ops.latent_mixture_fwd(method, _cuda(mu_in), _cuda(lv_in), eps.cuda(), mrs, crs, w, norm)
            ref = TBM.latent_mixture_fwd(method, mu_in, lv_in, eps, mrs, crs, w, norm)
            assert (got[10] is None) == (ref[10] is None) == (method == "moe"), tag
            for name, a, r in zip(names, got, ref):
                if r is None:
                    continue
                assert tuple(a.shape) == tuple(r.shape), (tag, name, a.shape, r.shape)
                if name in ("sub_mu", "sub_lv", "comp_mu", "comp_lv", "joint_mu", "joint_lv"):
                    # mixture selection copies rows: bit-identical to the members' (and the prior's zeros)
                    assert torch.equal(a.cpu(), r), (tag, name)
                elif name in ("klds", "individual_divs", "joint_div"):
                    np.testing.assert_allclose(a.cpu().numpy(), r.numpy(), rtol=2e-5, atol=1e-6, err_msg=f"{tag} {name}")
                else:
                    _close(f"{tag} {name}", a, r)
            # a second forward starts from a clean workspace (the first one left it zero)
            again = ops.latent_mixture_fwd(method, _cuda(mu_in), _cuda(lv_in), eps.cuda(), mrs, crs, w, norm)
            for i in (7, 8, 9):
                np.testing.assert_allclose(again[i].cpu().numpy(), got[i].cpu().numpy(), rtol=1e-6, atol=1e-7,
                                           err_msg=f"{tag} second forward {names[i]}")
            # backward: every upstream gradient, then only the ones a training step sends (z and joint_divergence)
            gs = [None if r is None else rnd(*r.shape) for r in ref]
            only = [None] * 6 + [gs[6], None, None, gs[9], None, None]
            for kind, g in (("all", gs), ("z+jd", only)):
                dmu, dlv = ops.latent_mixture_bwd(method, _cuda(mu_in), _cuda(lv_in), eps.cuda(), mrs, crs, w, norm,
                                                  *_cuda(g))
                rmu, rlv = TBM.latent_mixture_bwd(method, mu_in, lv_in, eps, mrs, crs, w, norm, *g)
                for s, m in enumerate(SLOTS):
                    assert (dmu[s] is None) == (m not in combo), (tag, kind, m)
                    if m in combo:
                        _close(f"{tag} {kind} d_mu/{m}", dmu[s], rmu[s], rtol=1e-4, atol_rel=1e-5)
                        _close(f"{tag} {kind} d_logvar/{m}", dlv[s], rlv[s], rtol=1e-4, atol_rel=1e-5)
    torch.cuda.synchronize()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("mode", ["eval", "train_nodrop", "train"])
def test_g8_g0_full_model_on_gpu(method, mode):
    g = load(f"g8_{method}_g0_s64")
    cfg = cfg_from(g["cfg"])
    exp = build_exp(method, cfg, g8_state(g, cfg), "cuda", mode,
                    masks=g0_masks(g) if mode == "train" else None, eps=torch.from_numpy(g[f"{mode}/eps"]))
    out = check_against_g8_g0(exp, g, mode, g8_batch(g, cfg), device="cuda", rtol=2e-4, atol=2e-5)
    assert (out["results"]["dyn_prior"] is None) == (method == "moe")


def _checksums(t):
    """golden_util.checksums with its sample positions clamped to the tensor (as tests/tools/gen_golden_methods.py wrote
    them: config #2's text logits have more elements than the fp32 linspace behind the positions resolves)"""
    t = t.detach().double().flatten().cpu()
    idx = torch.linspace(0, t.numel() - 1, 16).long().clamp(max=t.numel() - 1)
    return np.concatenate([[t.sum().item(), (t * t).sum().item()], t[idx].numpy()])


def _check_g1_like(g, method):
    cfg = cfg_from(g["cfg"])
    exp = build_exp(method, cfg, R.init_state(cfg, seed=int(g["seed_weights"])), "cuda", "train_nodrop",
                    eps=torch.from_numpy(g["eps"]))
    out = RE.basic_routine_epoch(exp, ({k: v.cuda() for k, v in g8_batch(g, cfg).items()}, None))
    close(out["total_loss"], g["total_loss"], 1e-4, 0)
    close(out["results"]["joint_divergence"], g["joint_divergence"], 1e-4, 0)
    close(out["results"]["individual_divs"], g["individual_divs"], 1e-4, 1e-6)
    for k, v in out["log_probs"].items():
        close(v, g[f"log_probs/{k}"], 1e-4, 0)
    for k, v in out["klds"].items():
        close(v, g[f"klds/{k}"], 1e-4, 1e-6)
    lat = out["results"]["latents"]
    for m in R.MOD_ORDER:
        np.testing.assert_allclose(_checksums(lat["modalities"][m][0]), g[f"chk/enc/{m}/mu"], rtol=1e-3, atol=1e-4)
        np.testing.assert_allclose(_checksums(lat["modalities"][m][1]), g[f"chk/enc/{m}/logvar"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(_checksums(lat["joint"][0]), g["chk/joint/mu"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(_checksums(out["results"]["rec"]["PA"].loc), g["chk/rec/PA"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(_checksums(out["results"]["rec"]["text"].logits), g["chk/rec/text"], rtol=1e-3, atol=1e-2)
    exp.mm_vae.zero_grad()
    out["total_loss"].backward()
    norms = {}
    for name, gr in exp.mm_vae.reference_named_grads().items():
        top = name.split(".")[0]
        norms[top] = norms.get(top, 0.0) + gr.double().pow(2).sum().item()
    for k, v in norms.items():
        np.testing.assert_allclose(np.sqrt(v), g[f"gradnorm/{k}"], rtol=2e-3, err_msg=k)
    dead = [n for n, p in exp.mm_vae.named_parameters() if p.grad is None]
    assert len(dead) == int(g["n_dead_params"])


@pytest.mark.parametrize("method", METHODS)
def test_g8_c1_on_gpu(method):
    """config #1 stand-in (64 px, class_dim 64, B = 8, DIM_img 64)"""
    _check_g1_like(load(f"g8_{method}_c1"), method)


@pytest.mark.parametrize("method", METHODS)
def test_g8_c2_shape_on_gpu(method, table_plans):
    """config #2's shape (128 px, class_dim 128, B = 64, DIM_img 64) on the committed launch plans"""
    _check_g1_like(load(f"g8_{method}_c2"), method)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ["eager", "graph"])
def test_g8_adam_trajectory_on_gpu(method, kind):
    """the reference's 3-step Adam trajectory of each method, eager and replayed from the captured hipGraph (as
    test_model_gpu.test_g3_adam_trajectory_on_gpu does for joint_elbo)"""
    g = load(f"g8_{method}_traj")
    cfg = cfg_from(g["cfg"])
    exp = build_exp(method, cfg, R.init_state(cfg, seed=int(g["seed_weights"])), "cuda", "train_nodrop")
    exp.flags.initial_learning_rate = float(g["lr"])
    exp.set_optimizer(capturable=(kind == "graph"))
    eps_static = torch.zeros(cfg.batch_size, cfg.class_dim, device="cuda")
    exp.mm_vae.eps_source = lambda b, d, dev: eps_static
    pack = RE.ScalarPack(exp.flags.device)
    dev = lambda b: ({k: v.cuda() for k, v in b.items()}, None)
    losses, step = [], None
    for i in range(3):
        batch, _ = R.synthetic_batch(cfg, cfg.batch_size, seed=20 + i)
        eps_static.copy_(torch.from_numpy(g["eps"][i]))
        if kind == "eager":
            RE.train_step(exp, dev(batch), None, pack)
        elif step is None:
            step = RE.GraphedTrainStep(exp, dev(batch), pack, warmup=1)
        else:
            step(dev(batch))
        losses.append(pack.read()["total_loss"])
    torch.cuda.synchronize()
    np.testing.assert_allclose(losses, g["losses"], rtol=1e-4)
    sd = exp.mm_vae.state_dict()
    lr = float(g["lr"])
    for name in ("encoder_pa.feature_extractor.conv1.weight", "decoder_text.feature_generator.bias"):
        ref = g["final/" + name]
        d = np.abs(sd[name].cpu().numpy() - ref)
        assert d.max() <= 6 * lr + 1e-6, (name, d.max())
        assert np.quantile(d, 0.98) <= 1e-4 * np.abs(ref).max() + 2e-6, (name, np.quantile(d, 0.98), d.max())


@pytest.mark.parametrize("method", METHODS)
def test_g8_partial_modalities_and_likelihood_on_gpu(method):
    g = load(f"g8_{method}_partial")
    cfg = cfg_from(g["partial/cfg"])
    sd = R.init_state(cfg, seed=int(g["partial/seed_weights"]))
    batch, _ = R.synthetic_batch(cfg, cfg.batch_size, seed=int(g["partial/seed_batch"]))
    exp = build_exp(method, cfg, sd, "cuda", "eval")
    for combo in PRESENCE[:-1]:
        tag = "+".join(combo)
        with torch.no_grad():
            lat = exp.mm_vae.inference({m: batch[m].cuda() for m in combo})
        assert list(lat["subsets"].keys()) == list(g[f"partial/{tag}/keys"])
        close(lat["mus"].cpu(), g[f"partial/{tag}/mus"], 1e-4, 1e-4)
        close(lat["logvars"].cpu(), g[f"partial/{tag}/logvars"], 1e-4, 1e-4)
        close(lat["weights"].cpu(), g[f"partial/{tag}/weights"])
        close(lat["joint"][0].cpu(), g[f"partial/{tag}/joint_mu"], 1e-4, 1e-4)
        close(lat["joint"][1].cpu(), g[f"partial/{tag}/joint_logvar"], 1e-4, 1e-4)
    from mimic_amd.evaluation.eval_metrics.likelihood import calc_log_likelihood_batch
    g = load(f"g8_{method}_likelihood")
    cfg = cfg_from(g["cfg"])
    sd = R.init_state(cfg, seed=int(g["seed_weights"]))
    batch, _ = R.synthetic_batch(cfg, cfg.batch_size, seed=int(g["seed_batch"]))
    exp = build_exp(method, cfg, sd, "cuda", "eval")
    dbatch = {k: v.cuda() for k, v in batch.items()}
    with torch.no_grad():
        lat = exp.mm_vae.inference(dict(dbatch))
        for s_key in ("PA", "text", "Lateral_text", "Lateral_PA_text"):
            ll = calc_log_likelihood_batch(exp, lat, s_key, exp.subsets[s_key], dbatch, num_imp_samples=int(g["K"]),
                                           eps=torch.from_numpy(g[f"{s_key}/eps"]))
            for m_key, v in ll.items():
                ref = float(g[f"{s_key}/{m_key}"])
                assert abs(v.item() - ref) <= 1e-4 * abs(ref) + 1e-3, (s_key, m_key, v.item(), ref)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


@pytest.mark.parametrize("method", METHODS)
def test_g8_bf16_family_vs_fp32_reference(method):
    """the bf16 family (bf16 storage and MFMA; the latents stay fp32) runs both methods: its scalars against the
    reference's fp32 run at the bf16 tolerance of test_bf16_gpu.py (rtol 2e-2), and its backward is finite.  On the C1
    fixture: the smallest one whose channel counts the bf16 kernels take (multiples of 32; G0's are 4)."""
    g = load(f"g8_{method}_c1")
    cfg = cfg_from(g["cfg"])
    exp = build_exp(method, cfg, R.init_state(cfg, seed=int(g["seed_weights"])), "cuda", "train_nodrop",
                    eps=torch.from_numpy(g["eps"]), compute_dtype="bf16")
    out = RE.basic_routine_epoch(exp, ({k: v.cuda() for k, v in g8_batch(g, cfg).items()}, None))
    res = out["results"]
    assert res["latents"]["mus"].dtype == torch.float32

    def near(v, r, what):
        assert _rel(v, r) <= 2e-2 + 1e-3 / max(abs(r), 1e-3), (what, v, r)

    near(out["total_loss"].item(), float(g["total_loss"]), "total_loss")
    near(res["joint_divergence"].item(), float(g["joint_divergence"]), "joint_divergence")
    for i, v in enumerate(res["individual_divs"].tolist()):
        near(v, float(g["individual_divs"][i]), f"individual_divs[{i}]")
    for k, v in out["klds"].items():
        near(v.item(), float(g[f"klds/{k}"]), f"klds/{k}")
    for k, v in out["log_probs"].items():
        near(v.item(), float(g[f"log_probs/{k}"]), f"log_probs/{k}")
    exp.mm_vae.zero_grad()
    out["total_loss"].backward()
    for name, gr in exp.mm_vae.reference_named_grads().items():
        assert bool(torch.isfinite(gr).all()), name


def test_jsd_two_epochs_on_tensor_files_through_the_launcher(tmp_path):
    """`--method jsd` through the launcher (as test_launcher_gpu.test_two_epochs_on_tensor_files_through_the_launcher
    runs joint_elbo): spawned rank process, captured train steps and the eager short last batch, test(), checkpoint"""
    from golden_util import make_mimic_files
    from mimic_amd import main_mimic as MM
    data = tmp_path / "data"
    make_mimic_files(str(data), img_size=64, n_train=100, n_eval=30, seed=5)
    run_dir = tmp_path / "run"
    flags = MM.parse_flags(["--method", "jsd", "--dataset", "mimic", "--dir_data", str(data), "--img_size", "64",
                            "--class_dim", "32", "--DIM_img", "64", "--DIM_text", "32", "--batch_size", "8",
                            "--len_sequence", "128", "--end_epoch", "2", "--initial_learning_rate", "1e-5",
                            "--dir_experiment_run", str(run_dir)])
    assert flags.modality_jsd and not flags.joint_elbo
    m = MM.Main(flags)
    m.setup_distributed = lambda: (setattr(m.flags, "world_size", 1), setattr(m.flags, "distributed", False))
    assert m.main() is True and m.current_tries == 0
    hist = m.history
    n_train = hist[0]["train"]["steps"]
    assert n_train >= 8 and [h["epoch"] for h in hist] == [0, 1]
    assert hist[1]["train"]["graphed_steps"] >= n_train - 1
    for h in hist:
        assert len(h["train"]["last"]) == 18     # the seven subset KLs are still seven
        assert all(v == v and abs(v) < 1e9 for v in h["train"]["last"].values()) and "total_loss" in h["test"]
    assert (run_dir / "checkpoints" / "0001" / "mm_vae").exists()
