"""Build the mimic_amd model for method='moe' / 'jsd' fixtures (tests/golden/g8_*): model_util.build_exp with the flags
passed through utils.filehandling.get_method (shared by the CPU and GPU tests of the two methods)."""
import contextlib

import model_util
from mimic_amd.utils.filehandling import get_method

METHODS = ("moe", "jsd")


@contextlib.contextmanager
def method_flags(method):
    orig = model_util.default_flags

    def flags(**kw):
        f = orig(**kw)
        f.method = method
        return get_method(f)

    model_util.default_flags = flags
    try:
        yield
    finally:
        model_util.default_flags = orig


def build_exp(method, *args, **kw):
    with method_flags(method):
        exp = model_util.build_exp(*args, **kw)
    assert exp.mm_vae.method == method
    return exp


# ---------------------------------------------------------------------------------------------------------------
# Compact fixture format of g8_*_g0_s64 and g8_*_c2 (tests/tools/gen_golden_methods.py writes it, the tests read it).
#   * weights: not stored; regenerated from `seed_weights` (mopoe_ref.init_state, plus the embedding padding row G0 sets)
#     and checked against `sd_fingerprint`;
#   * images of a seeded batch (c2): the few pixels the tie-breaking pass moved, as a patch on mopoe_ref.synthetic_batch;
#   * reconstructions (g0): full-tensor checksums plus REC_SAMPLE seeded elements;
#   * parameter gradients (g0), per mode, in flat arrays over the parameters in `grad_names` order: every element of a
#     tensor of at most GRAD_EXACT elements, otherwise its L2 norm, max |g| and a GRAD_SKETCH-bucket count sketch (element i
#     to bucket i mod GRAD_SKETCH with a seeded sign): ||S a - S t|| estimates ||a - t|| for any a (relative standard
#     deviation sqrt(2 / GRAD_SKETCH) = 25 %), enough to tell fp32 rounding (~1e-5 of ||t||) from a wrong gradient.
# ---------------------------------------------------------------------------------------------------------------
import numpy as np  # noqa: E402
import torch  # noqa: E402
import zlib  # noqa: E402

GRAD_EXACT, GRAD_SKETCH, REC_SAMPLE = 32, 32, 256
G0_PAD_ROW = ("encoder_text.feature_extractor.embedding.weight", 0.25)   # oracle/gen_golden.gen_g0


def _gen(n, salt):
    return torch.Generator().manual_seed(salt + n % 1000003)


def grad_sketch(t):
    t = t.detach().double().cpu().flatten()
    n = t.numel()
    signs = torch.randint(0, 2, (n,), generator=_gen(n, 0x5EED1000), dtype=torch.int8) * 2 - 1
    v = t * signs
    pad = (-n) % GRAD_SKETCH
    if pad:
        v = torch.cat([v, v.new_zeros(pad)])
    return v.view(-1, GRAD_SKETCH).sum(0)


def rec_sample_index(n):
    return torch.randperm(n, generator=_gen(n, 0x5EED2000))[:REC_SAMPLE].sort().values


def pack_grads(store, prefix, grads, names):
    exact, norms, sketches = [], [], []
    for name in names:
        t = torch.as_tensor(grads[name]).detach().double().cpu().flatten()
        if t.numel() <= GRAD_EXACT:
            exact.append(t)
        else:
            norms.append([t.norm().item(), t.abs().max().item()])
            sketches.append(grad_sketch(t))
    store[prefix + "/grad_exact"] = torch.cat(exact).float().numpy()
    store[prefix + "/grad_norm"] = np.array(norms, dtype=np.float64)
    store[prefix + "/grad_sketch"] = torch.stack(sketches).numpy()


def check_grads(g, prefix, grads, rtol=1e-3, atol=1e-3):
    """every parameter gradient against a packed fixture: exact tensors element-wise as test_host_logic_cpu.check_against_g0
    does (rtol, atol * the tensor's scale), sketched ones in L2 (|| error || <= 2 (rtol ||t|| + atol sqrt(n) scale), the
    factor 2 covering the sketch's spread)"""
    names, numel = [str(s) for s in g["grad_names"]], [int(v) for v in g["grad_numel"]]
    assert set(names) == set(grads.keys()), set(names) ^ set(grads.keys())
    exact, norms, sk = g[prefix + "/grad_exact"], g[prefix + "/grad_norm"], g[prefix + "/grad_sketch"]
    absmax = {}
    pe = pn = 0
    for name, n in zip(names, numel):
        if n <= GRAD_EXACT:
            absmax[name] = float(np.abs(exact[pe:pe + n]).max()) if n else 0.0
            pe += n
        else:
            absmax[name] = float(norms[pn][1])
            pn += 1
    pe = pn = 0
    for name, n in zip(names, numel):
        got = grads[name].detach().double().cpu().flatten()
        assert got.numel() == n, (name, got.numel(), n)
        scale = max(absmax[name], 1e-3)
        if name.endswith(".bias") and name[:-4] + "weight" in absmax:
            scale = max(scale, absmax[name[:-4] + "weight"])
        if n <= GRAD_EXACT:
            np.testing.assert_allclose(got.numpy(), exact[pe:pe + n], rtol=rtol, atol=atol * scale, err_msg=name)
            pe += n
        else:
            err = (grad_sketch(got) - torch.from_numpy(sk[pn])).norm().item()
            bound = 2 * (rtol * norms[pn][0] + atol * np.sqrt(n) * scale)
            assert err <= bound, (name, err, bound, norms[pn][0])
            assert abs(got.norm().item() - norms[pn][0]) <= bound, (name, got.norm().item(), norms[pn][0])
            pn += 1


def u8_crc(u8):
    return zlib.crc32(np.ascontiguousarray(u8).tobytes())


def g8_state(g, cfg):
    """the fixture's weights, regenerated from their seed"""
    import mopoe_ref as R
    from golden_util import weights_fingerprint
    sd = R.init_state(cfg, seed=int(g["seed_weights"]))
    if "pad_row" in g.files:
        sd[G0_PAD_ROW[0]][0] = float(g["pad_row"])
    np.testing.assert_allclose(weights_fingerprint(sd), g["sd_fingerprint"], rtol=1e-6)
    return sd


def g8_batch(g, cfg):
    """the fixture's inputs: stored as they are (g0) or as a patch on the seeded synthetic batch (c2)"""
    import mopoe_ref as R
    from golden_util import g0_batch
    if "in/PA_u8" in g.files:
        return g0_batch(g)
    nrow = int(g["cfg"][5])
    batch, _ = R.synthetic_batch(cfg, nrow, seed=int(g["seed_batch"]))
    out = {"text": torch.from_numpy(g["in/text"]).float()}
    for m in ("PA", "Lateral"):
        u8 = (batch[m] * 255.0).round().to(torch.uint8).numpy().copy()
        u8.reshape(-1)[g[f"in/{m}_patch_idx"]] = g[f"in/{m}_patch_val"]
        assert u8_crc(u8) == int(g[f"in/{m}_crc"]), m
        out[m] = torch.from_numpy(u8).float() / 255.0
    return out


def check_against_g8_g0(exp, g, mode, batch, device="cpu", grad_rtol=1e-3, grad_atol=1e-3, rtol=1e-4, atol=1e-5):
    """test_host_logic_cpu.check_against_g0 on the compact G0 format: every output, the reconstructions through their
    checksums and samples, every parameter gradient through check_grads"""
    import mopoe_ref as R
    from golden_util import checksums
    from mimic_amd import run_epochs as RE

    def close(a, b, rt=rtol, at=atol, msg=""):
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        np.testing.assert_allclose(a, b, rtol=rt, atol=at, err_msg=msg)

    out = RE.basic_routine_epoch(exp, ({k: v.clone().to(device) for k, v in batch.items()}, None))
    res, lat = out["results"], out["results"]["latents"]
    for m in R.MOD_ORDER:
        close(lat["modalities"][m][0], g[f"{mode}/enc/{m}/mu"], msg=m)
        close(lat["modalities"][m][1], g[f"{mode}/enc/{m}/logvar"], msg=m)
    assert list(lat["subsets"].keys()) == ["PA", "Lateral", "text", "Lateral_PA", "PA_text", "Lateral_text",
                                           "Lateral_PA_text"]
    for key, (mu, lv) in lat["subsets"].items():
        close(mu, g[f"{mode}/subset/{key}/mu"], msg=key)
        close(lv, g[f"{mode}/subset/{key}/logvar"], msg=key)
    close(lat["mus"], g[f"{mode}/mus"])
    close(lat["logvars"], g[f"{mode}/logvars"])
    close(lat["weights"], g[f"{mode}/weights"], 1e-4, 1e-5)
    close(lat["joint"][0], g[f"{mode}/joint/mu"])
    close(lat["joint"][1], g[f"{mode}/joint/logvar"])
    close(res["individual_divs"], g[f"{mode}/individual_divs"])
    close(res["joint_divergence"], g[f"{mode}/joint_divergence"])
    recs = {"PA": res["rec"]["PA"].loc, "Lateral": res["rec"]["Lateral"].loc, "text": res["rec"]["text"].logits}
    for m, t in recs.items():
        flat = t.detach().cpu().flatten()
        close(flat[rec_sample_index(flat.numel())], g[f"{mode}/rec/{m}/sample"], 10 * rtol, 10 * atol, m)
        np.testing.assert_allclose(checksums(t), g[f"{mode}/recchk/{m}"], rtol=10 * rtol, atol=1e-3, err_msg=m)
    for k, v in out["klds"].items():
        close(v, g[f"{mode}/klds/{k}"], msg=k)
    for k, v in out["log_probs"].items():
        close(v, g[f"{mode}/log_probs/{k}"], msg=k)
    close(out["total_loss"], g[f"{mode}/total_loss"])
    exp.mm_vae.zero_grad()
    out["total_loss"].backward()
    check_grads(g, mode, exp.mm_vae.reference_named_grads(), grad_rtol, grad_atol)
    return out
