"""Generate tests/golden/g10_lhood_style_*.npz: the reference's importance-sampled likelihood estimates with
factorized_representation=True (mimic/evaluation/eval_metrics/likelihood.py:17-96, mimic/utils/likelihood.py:13-220).

Built on tests/tools/gen_golden_style.py: its install() gives the reference networks their style dims and the seeded style
weights of tests/style_util.py, and sets exp.style_weights.  Per subset the reference's calc_log_likelihood_batch draws
four times through utils.reparameterize -- the content noise [K,B,D], then one style draw [K,B,S] for PA, Lateral and
text -- and StyleCapture counts them; the draws themselves are re-made from the seed set before the call (the values
utils.reparameterize took from the global generator), so they are stored exactly.  Only seeds, noise and scalars are
written; the weights come from their seeds (R.init_state, style_util.style_weights) and are checked by fingerprint.

Fixtures:
  g10_lhood_style_s64       tiny model (64 px, class_dim 8, DIM 4, B 4, K 6, style dims 4/4/4), all 7 subsets, joint_elbo
  g10_lhood_style_jsd_s64   the same for method='jsd'
  g10_lhood_style_c2        128 px, class_dim 128, DIM_img 64, style dims 32/32/32, B 4, K 6, three subsets
  g10_lhood_style_pub       the reference's log_marginal_estimate / log_joint_estimate on stored random tensors with
                            style dicts (Laplace likelihoods)
Usage:  python tests/tools/gen_golden_lhood_style.py [--only s64 jsd_s64 c2 pub]
"""
from __future__ import annotations

import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(REPO, "tests"), os.path.join(REPO, "oracle"), os.path.join(REPO, "mopoe-mimic_amd")]

import gen_golden_methods as GM  # noqa: E402
import gen_golden_style as GS  # noqa: E402
import style_util as SU  # noqa: E402

MODS = ("PA", "Lateral", "text")
K, B = 6, 4
SEED_WEIGHTS, SEED_BATCH = 31, 9
ALL = ("PA", "Lateral", "text", "Lateral_PA", "PA_text", "Lateral_text", "Lateral_PA_text")
FIXTURES = {
    "s64": dict(cfg=(64, 8, 4, 4, 50, B), dims=(4, 4, 4), method="joint_elbo", subsets=ALL),
    "jsd_s64": dict(cfg=(64, 8, 4, 4, 50, B), dims=(4, 4, 4), method="jsd", subsets=ALL),
    "c2": dict(cfg=(128, 128, 64, 128, 3517, B), dims=(32, 32, 32), method="joint_elbo",
               subsets=("PA", "Lateral_text", "Lateral_PA_text")),
}


def gen_estimates(G, name, spec):
    import mopoe_ref as R
    from mimic.evaluation.eval_metrics.likelihood import calc_log_likelihood_batch
    GS._state.dims, GS._state.caps = spec["dims"], []
    GM.select_method(G, spec["method"])
    cfg = R.Cfg(img_size=spec["cfg"][0], class_dim=spec["cfg"][1], DIM_img=spec["cfg"][2], DIM_text=spec["cfg"][3],
                vocab_size=spec["cfg"][4], batch_size=spec["cfg"][5])
    sd = R.init_state(cfg, seed=SEED_WEIGHTS)
    batch, _ = R.synthetic_batch(cfg, B, seed=SEED_BATCH)
    exp = G.build_reference(cfg, sd)
    exp.mm_vae.eval()
    store = {"cfg": np.array(spec["cfg"]), "seed_weights": np.array(SEED_WEIGHTS), "seed_batch": np.array(SEED_BATCH),
             "K": np.array(K), "method": np.array(spec["method"]), "subsets": np.array(spec["subsets"])}
    with torch.no_grad():
        lat = exp.mm_vae.inference({m: v.clone() for m, v in batch.items()})
        for i, s_key in enumerate(spec["subsets"]):
            seed = 700 + i
            torch.manual_seed(seed)
            cap = GS.StyleCapture(exp.mm_vae)
            try:
                ll = calc_log_likelihood_batch(exp, lat, s_key, exp.subsets[s_key],
                                               {m: v.clone() for m, v in batch.items()}, num_imp_samples=K)
            finally:
                cap.close()
            assert len(cap.eps) == 4, (s_key, len(cap.eps))
            # utils.reparameterize draws std.data.new(std.size()).normal_(): the same four draws, re-made from the seed
            torch.manual_seed(seed)
            draws = [torch.empty(e.shape).normal_() for e in cap.eps]
            for e, d in zip(cap.eps, draws):
                np.testing.assert_allclose(e.numpy(), d.numpy(), rtol=1e-4, atol=1e-4)
            store[f"{s_key}/eps"] = draws[0].numpy()
            for m, d in zip(MODS, draws[1:]):
                store[f"{s_key}/eps_style/{m}"] = d.numpy()
            for m_key, v in ll.items():
                assert np.isfinite(float(v)), (s_key, m_key)
                store[f"{s_key}/{m_key}"] = np.array(float(v))
    store["style_dims"] = np.array(spec["dims"])
    store["seed_style"] = np.array(GS.SEED_STYLE)
    store["style_fingerprint"] = SU.fingerprint(SU.style_weights(cfg, spec["dims"], GS.SEED_STYLE))
    return store


def gen_public():
    """the reference's log_marginal_estimate / log_joint_estimate with style dicts on seeded random tensors"""
    from mimic.utils.likelihood import log_joint_estimate, log_marginal_estimate
    gen = torch.Generator().manual_seed(77)
    d, s, side = 8, 4, 4
    rnd = lambda *shape: torch.randn(*shape, generator=gen)
    store = {"K": np.array(K), "B": np.array(B), "scale": np.array(0.75)}
    t = {"mu": rnd(B, d), "logvar": rnd(B, d).clamp(-3, 2), "eps": rnd(K, B, d)}
    for m in MODS:
        t[f"style/{m}/mu"], t[f"style/{m}/logvar"] = rnd(B, s), rnd(B, s).clamp(-3, 2)
        t[f"style/{m}/eps"] = rnd(K, B, s)
        t[f"target/{m}"] = torch.rand(B, 1, side, side, generator=gen)
        t[f"loc/{m}"] = torch.rand(K * B, 1, side, side, generator=gen)
    draw = lambda mu, lv, e: {"mu": mu.unsqueeze(0).repeat(K, 1, 1).view(K * B, -1),
                              "logvar": lv.unsqueeze(0).repeat(K, 1, 1).view(K * B, -1),
                              "z": (e * torch.exp(0.5 * lv.unsqueeze(0)) + mu.unsqueeze(0)).view(K * B, -1)}
    content = draw(t["mu"], t["logvar"], t["eps"])
    styles = {m: draw(t[f"style/{m}/mu"], t[f"style/{m}/logvar"], t[f"style/{m}/eps"]) for m in MODS}
    lh = {m: torch.distributions.Laplace(t[f"loc/{m}"], torch.tensor(0.75)) for m in MODS}
    flags = SimpleNamespace(batch_size=B, device=torch.device("cpu"))
    store["marginal/PA"] = np.array(float(log_marginal_estimate(flags, K, lh["PA"], t["target/PA"], styles["PA"], content)))
    store["marginal/Lateral_nostyle"] = np.array(float(log_marginal_estimate(flags, K, lh["Lateral"], t["target/Lateral"],
                                                                             None, content)))
    store["joint"] = np.array(float(log_joint_estimate(flags, K, lh, {m: t[f"target/{m}"] for m in MODS}, styles, content)))
    for k, v in t.items():
        store["in/" + k] = v.numpy()
    return store


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    G = GM.load_generator()
    G.checksums = GM.checksums
    if not os.path.isdir(G.REF):
        print("reference not present; nothing to do")
        return
    torch.set_num_threads(8)
    G.import_reference()
    GS.install(G)
    outdir = os.path.join(REPO, "tests", "golden")
    for name in ("s64", "jsd_s64", "c2", "pub"):
        if args.only and name not in args.only:
            continue
        store = gen_public() if name == "pub" else gen_estimates(G, name, FIXTURES[name])
        path = os.path.join(outdir, f"g10_lhood_style_{name}.npz")
        np.savez_compressed(path, **store)
        print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(store)} arrays", flush=True)


if __name__ == "__main__":
    main()
