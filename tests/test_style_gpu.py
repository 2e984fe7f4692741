"""Style latents (factorized_representation=True) on the GPU: the style kernels (ops.latent_style_fwd / _bwd) against their
torch restatement (tests/torch_backend_style.py), and the whole factorized model against the reference's own outputs
(tests/golden/g9_style_*), with the tolerances of the joint_elbo / method tests (test_model_gpu.py, test_methods_gpu.py)."""
import itertools

import numpy as np
import pytest
import torch

import model_util
import mopoe_ref as R
import style_util as SU
import torch_backend_style as TBS
from golden_util import load, g0_masks
from methods_util import check_against_g8_g0, g8_batch
from test_host_logic_cpu import close
from test_methods_gpu import _checksums, _rel
from test_style_cpu import check_style
from mimic_amd import ops, run_epochs as RE
from mimic_amd.nets import ZCAT

pytestmark = pytest.mark.gpu

PRESENCE = [p for p in itertools.product((False, True), repeat=3) if any(p)]
S_LIST = (1, 5, 8, 32, 64)


def _np(t):
    return t.detach().double().cpu().numpy()


def _close(name, got, ref, rtol=1e-5, atol_rel=1e-5):
    scale = max(float(ref.detach().abs().max()), 1e-6)
    np.testing.assert_allclose(_np(got), _np(ref), rtol=rtol, atol=atol_rel * scale, err_msg=name)


def test_latent_style_kernels_vs_restatement():
    """every presence pattern, B in {1, 7, 64, 65, 256}, S in {1, 5, 8, 32, 64} mixed per slot, D in {8, 64, 128}; the four
    gradient patterns (g_zcat only, g_klds_style only, both, neither)"""
    gen = torch.Generator().manual_seed(11)
    case = 0
    for b in (1, 7, 64, 65, 256):
        for d in (8, 64, 128):
            for pres in PRESENCE:
                case += 1
                dims = [S_LIST[(case + k) % len(S_LIST)] for k in range(3)]
                mk = lambda s, f=1.0: (torch.randn(b, s, generator=gen) * f).cuda()
                smu = [mk(dims[m]) if pres[m] else None for m in range(3)]
                slv = [mk(dims[m], 0.5) if pres[m] else None for m in range(3)]
                eps = [mk(dims[m]) if pres[m] else None for m in range(3)]
                z = mk(d)
                norm = float(max(b, 2))
                zcat, klds = ops.latent_style_fwd(smu, slv, eps, z, norm)
                rz, rk = TBS.latent_style_fwd(smu, slv, eps, z, norm)
                for m in range(3):
                    assert (zcat[m] is None) == (not pres[m])
                    if pres[m]:
                        assert bool(torch.isfinite(zcat[m]).all())
                        _close(f"zcat {b} {d} {pres} {m}", zcat[m], rz[m])
                        ref64 = -0.5 * torch.sum(1 - slv[m].double().exp() - smu[m].double() ** 2 + slv[m].double()) / norm
                        assert abs(klds[m].item() - ref64.item()) <= 2e-6 * (abs(ref64.item()) + 1e-3) * dims[m] ** 0.5 \
                            + 1e-6, (b, d, pres, m, klds[m].item(), ref64.item())
                    else:
                        assert klds[m].item() == 0.0
                g_zcat = [torch.randn(t.shape, generator=gen).cuda() if t is not None else None for t in zcat]
                g_kl = torch.randn(3, generator=gen).cuda()
                for gz_on, gk_on in ((True, False), (False, True), (True, True), (False, False)):
                    gzc = g_zcat if gz_on else [None] * 3
                    gk = g_kl if gk_on else None
                    dmu, dlv, gz = ops.latent_style_bwd(smu, slv, eps, d, norm, gzc, gk)
                    rmu, rlv, rgz = TBS.latent_style_bwd(smu, slv, eps, d, norm, gzc, gk)
                    _close("g_z", gz, rgz)
                    for m in range(3):
                        if pres[m]:
                            assert bool(torch.isfinite(dmu[m]).all()) and bool(torch.isfinite(dlv[m]).all())
                            _close(f"dmu {b} {d} {pres} {m} {gz_on} {gk_on}", dmu[m], rmu[m])
                            _close(f"dlv {b} {d} {pres} {m} {gz_on} {gk_on}", dlv[m], rlv[m])
                        else:
                            assert dmu[m] is None and dlv[m] is None
    torch.cuda.synchronize()
    assert float(ops._ws(torch.device("cuda", torch.cuda.current_device()), 4).abs().sum()) == 0.0   # left zero


def test_latent_style_refuses_inconsistent_arguments():
    x = torch.zeros(4, 3, device="cuda")
    z = torch.zeros(4, 8, device="cuda")
    with pytest.raises(ops.MopoeHipError):
        ops.latent_style_fwd([x, None, None], [None, None, None], [x, None, None], z, 4.0)
    with pytest.raises(ops.MopoeHipError):
        ops.latent_style_fwd([None] * 3, [None] * 3, [None] * 3, z, 4.0)


def _exp(g, mode, method="joint_elbo", device="cuda", compute_dtype="fp32", eps=None):
    cfg = SU.cfg_of(g)
    sd, dims = SU.g9_state(g, cfg)
    sw = [float(v) for v in g["style_weights"]]
    with SU.style_flags(dims, method, beta_m1_style=sw[0], beta_m2_style=sw[1], beta_m3_style=sw[2]):
        exp = model_util.build_exp(cfg, sd, device, mode, g0_masks(g) if mode == "train" else None,
                                   compute_dtype=compute_dtype)
    SU.set_eps(exp.mm_vae, eps if eps is not None else SU.fixture_eps(g, mode + "/"), device)
    return exp, cfg


@pytest.mark.parametrize("method", ["joint_elbo", "jsd"])
@pytest.mark.parametrize("mode", ["eval", "train_nodrop", "train"])
def test_g9_g0_full_model_on_gpu(method, mode):
    g = load({"joint_elbo": "g9_style_g0_s64", "jsd": "g9_style_jsd_g0_s64"}[method])
    exp, cfg = _exp(g, mode, method)
    out = check_against_g8_g0(exp, g, mode, g8_batch(g, cfg), device="cuda", rtol=2e-4, atol=2e-5)
    check_style(out, g, mode)


def _c2_eps(g):
    return [torch.from_numpy(g["eps"])] + [torch.from_numpy(g[f"eps_style/{m}"]) for m, *_ in SU.MODS]


def _check_c2(g, out, exp):
    close(out["total_loss"], g["total_loss"], 1e-4, 0)
    close(out["results"]["joint_divergence"], g["joint_divergence"], 1e-4, 0)
    for k, v in out["log_probs"].items():
        close(v, g[f"log_probs/{k}"], 1e-4, 0)
    for k, v in out["klds"].items():
        close(v, g[f"klds/{k}"], 1e-4, 1e-6)
    lat = out["results"]["latents"]["modalities"]
    for m, *_ in SU.MODS:
        close(out["klds_style"][m + "_style"], g[f"klds_style/{m}_style"], 1e-4, 1e-6)
        np.testing.assert_allclose(_checksums(lat[m + "_style"][0]), g[f"chk/enc/{m}_style/mu"], rtol=1e-3, atol=1e-4)
        np.testing.assert_allclose(_checksums(lat[m + "_style"][1]), g[f"chk/enc/{m}_style/logvar"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(_checksums(out["results"]["rec"]["PA"].loc), g["chk/rec/PA"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(_checksums(out["results"]["rec"]["text"].logits), g["chk/rec/text"], rtol=1e-3, atol=1e-2)


def test_g9_c2_shape_on_gpu(table_plans):
    """config #2's shape (128 px, class_dim 128, B = 64, DIM_img 64) with style dims 32 / 16 / 64, on the committed launch
    plans (the style heads and widened feature generators are not in the table: static heuristic)"""
    g = load("g9_style_c2")
    exp, cfg = _exp(g, "train_nodrop", eps=_c2_eps(g))
    out = RE.basic_routine_epoch(exp, ({k: v.cuda() for k, v in g8_batch(g, cfg).items()}, None))
    _check_c2(g, out, exp)
    exp.mm_vae.zero_grad()
    out["total_loss"].backward()
    norms = {}
    for name, gr in exp.mm_vae.reference_named_grads().items():
        top = name.split(".")[0]
        norms[top] = norms.get(top, 0.0) + gr.double().pow(2).sum().item()
    for k, v in norms.items():
        np.testing.assert_allclose(np.sqrt(v), g[f"gradnorm/{k}"], rtol=2e-3, err_msg=k)
    assert len([n for n, p in exp.mm_vae.named_parameters() if p.grad is None]) == int(g["n_dead_params"])


@pytest.mark.parametrize("kind", ["eager", "graph"])
def test_g9_adam_trajectory_on_gpu(kind):
    """the reference's 3-step Adam trajectory of the factorized model, eager and replayed from the captured hipGraph"""
    g = load("g9_style_traj")
    cfg = SU.cfg_of(g)
    dims = tuple(int(v) for v in g["style_dims"])
    sd = SU.style_state(cfg, R.init_state(cfg, seed=int(g["seed_weights"])), dims, int(g["seed_style"]))
    sw = [float(v) for v in g["style_weights"]]
    with SU.style_flags(dims, beta_m1_style=sw[0], beta_m2_style=sw[1], beta_m3_style=sw[2]):
        exp = model_util.build_exp(cfg, sd, "cuda", "train_nodrop")
    exp.flags.initial_learning_rate = float(g["lr"])
    exp.set_optimizer(capturable=(kind == "graph"))
    eps_static = [torch.zeros(cfg.batch_size, cfg.class_dim, device="cuda")] + \
        [torch.zeros(cfg.batch_size, s, device="cuda") for s in dims]
    exp.mm_vae.eps_source = lambda b, d, dev: eps_static[0]
    exp.mm_vae.style_eps_source = lambda m, b, s, dev: eps_static[1 + ("PA", "Lateral", "text").index(m)]
    pack = RE.ScalarPack(exp.flags.device)
    dev = lambda b: ({k: v.cuda() for k, v in b.items()}, None)
    losses, step = [], None
    for i in range(3):
        batch, _ = R.synthetic_batch(cfg, cfg.batch_size, seed=20 + i)
        eps_static[0].copy_(torch.from_numpy(g["eps"][i]))
        for k, (m, *_) in enumerate(SU.MODS):
            eps_static[1 + k].copy_(torch.from_numpy(g[f"eps_style/{m}"][i]))
        if kind == "eager":
            RE.train_step(exp, dev(batch), None, pack)
        elif step is None:
            step = RE.GraphedTrainStep(exp, dev(batch), pack, warmup=1)
        else:
            step(dev(batch))
        scal = pack.read()
        losses.append(scal["total_loss"])
        assert all(f"klds_style/{m}_style" in scal for m, *_ in SU.MODS)
    torch.cuda.synchronize()
    np.testing.assert_allclose(losses, g["losses"], rtol=1e-4)
    sd = exp.mm_vae.state_dict()
    lr = float(g["lr"])
    for name in ("encoder_pa.feature_extractor.conv1.weight", "decoder_text.feature_generator.bias",
                 "encoder_text.feature_compressor.style_mu.weight", "decoder_lat.feature_generator.weight"):
        ref = g["final/" + name]
        d = np.abs(sd[name].cpu().numpy() - ref)
        assert d.max() <= 6 * lr + 1e-6, (name, d.max())
        assert np.quantile(d, 0.98) <= 1e-4 * np.abs(ref).max() + 2e-6, (name, np.quantile(d, 0.98), d.max())


def test_g9_bf16_family_vs_fp32_reference():
    """the bf16 family runs the factorized model (style latents fp32, as the content ones): its scalars against the
    reference's fp32 run at the tolerance of test_bf16_gpu.py, and its backward is finite"""
    g = load("g9_style_c2")
    exp, cfg = _exp(g, "train_nodrop", compute_dtype="bf16", eps=_c2_eps(g))
    out = RE.basic_routine_epoch(exp, ({k: v.cuda() for k, v in g8_batch(g, cfg).items()}, None))
    lat = out["results"]["latents"]["modalities"]
    assert all(lat[m + "_style"][i].dtype == torch.float32 for m, *_ in SU.MODS for i in (0, 1))

    def near(v, r, what):
        assert _rel(v, r) <= 2e-2 + 1e-3 / max(abs(r), 1e-3), (what, v, r)

    near(out["total_loss"].item(), float(g["total_loss"]), "total_loss")
    for k, v in out["klds_style"].items():
        near(v.item(), float(g[f"klds_style/{k}"]), f"klds_style/{k}")
    for k, v in out["klds"].items():
        near(v.item(), float(g[f"klds/{k}"]), f"klds/{k}")
    exp.mm_vae.zero_grad()
    out["total_loss"].backward()
    for name, gr in exp.mm_vae.reference_named_grads().items():
        assert bool(torch.isfinite(gr).all()), name


def test_g9_eval_step_checkpoint_and_generation(tmp_path):
    """an eval step, a checkpoint round trip with the style keys, and generate / cond_generation with injected style noise:
    the decoders see [z_style | z] (the reference's torch.cat((z_style, z_content), dim=1))"""
    g = load("g9_style_g0_s64")
    exp, cfg = _exp(g, "eval")
    batch = {k: v.cuda() for k, v in g8_batch(g, cfg).items()}
    with torch.no_grad():
        out = RE.basic_routine_epoch(exp, ({k: v.clone() for k, v in batch.items()}, None))
    close(out["total_loss"], g["eval/total_loss"], 2e-4, 2e-5)
    path = tmp_path / "model.pt"
    torch.save(exp.mm_vae.state_dict(), path)
    exp2, _ = _exp(g, "eval")
    exp2.mm_vae.load_state_dict(torch.load(path), strict=True)
    assert any(".style_mu." in k for k in exp2.mm_vae.state_dict())
    with torch.no_grad():
        out2 = RE.basic_routine_epoch(exp2, ({k: v.clone() for k, v in batch.items()}, None))
    close(out2["total_loss"], out["total_loss"].item(), 1e-6, 1e-6)
    model = exp2.mm_vae
    dims = tuple(int(v) for v in g["style_dims"])
    gen = torch.Generator().manual_seed(4)
    n = 3
    zs = {m: torch.randn(n, s, generator=gen).cuda() for (m, *_), s in zip(SU.MODS, dims)}
    torch.manual_seed(5)
    z = torch.randn(n, cfg.class_dim, device="cuda")     # (what generate() draws for its content after the same seed)
    model.style_eps_source = lambda m, b, s, dev: zs[m]
    model.eps_source = lambda b, d, dev: z
    with torch.no_grad():
        styles = model.get_random_styles(n)
        assert all(torch.equal(styles[m], zs[m]) for m in zs)
        cond = model.cond_generation({"Lateral_text": [torch.zeros_like(z), torch.zeros_like(z)]}, n)["Lateral_text"]
        # the model's own decoder path (the kernel-written input), fed the reference's torch.cat((z_style, z_content))
        ref = {"PA": model.decoder_pa(ZCAT, torch.cat((zs["PA"], z), dim=1))[0],
               "Lateral": model.decoder_lat(ZCAT, torch.cat((zs["Lateral"], z), dim=1))[0],
               "text": model.lhood_text(logits=model.decoder_text(ZCAT, torch.cat((zs["text"], z), dim=1))[0]).mean}
        torch.manual_seed(5)
        gen_out = model.generate(n)
    for m in ("PA", "Lateral", "text"):
        close(cond[m], ref[m].cpu(), 1e-5, 1e-6)
        close(gen_out[m], ref[m].cpu(), 1e-5, 1e-6)


@pytest.mark.parametrize("method", ["joint_elbo", "moe", "jsd"])
def test_factorized_two_epochs_through_the_launcher(tmp_path, method):
    """`--factorized_representation true` with three style dims through the launcher, for each method: spawned rank
    process, captured train steps and the eager short last batch, test(), checkpoint"""
    from golden_util import make_mimic_files
    from mimic_amd import main_mimic as MM
    data = tmp_path / "data"
    make_mimic_files(str(data), img_size=64, n_train=60, n_eval=20, seed=5)
    run_dir = tmp_path / "run"
    flags = MM.parse_flags(["--method", method, "--dataset", "mimic", "--dir_data", str(data), "--img_size", "64",
                            "--class_dim", "32", "--DIM_img", "64", "--DIM_text", "32", "--batch_size", "8",
                            "--len_sequence", "128", "--end_epoch", "2", "--initial_learning_rate", "1e-5",
                            "--factorized_representation", "true", "--style_pa_dim", "32", "--style_lat_dim", "16",
                            "--style_text_dim", "64", "--dir_experiment_run", str(run_dir)])
    m = MM.Main(flags)
    m.setup_distributed = lambda: (setattr(m.flags, "world_size", 1), setattr(m.flags, "distributed", False))
    assert m.main() is True and m.current_tries == 0
    hist = m.history
    assert [h["epoch"] for h in hist] == [0, 1]
    assert hist[1]["train"]["graphed_steps"] >= hist[0]["train"]["steps"] - 1
    for h in hist:
        last = h["train"]["last"]
        assert all(f"klds_style/{m}_style" in last for m in ("PA", "Lateral", "text"))
        assert all(v == v and abs(v) < 1e9 for v in last.values()) and "total_loss" in h["test"]
    assert (run_dir / "checkpoints" / "0001" / "mm_vae").exists()
