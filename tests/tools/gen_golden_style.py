"""Generate tests/golden/g9_style_*.npz: the reference's own outputs with factorized_representation=True (a private style
latent per modality besides the shared content latent).

oracle/gen_golden.py is imported as a module and left as it is (as tests/tools/gen_golden_methods.py does).  Three of its
pieces are wrapped here:
  * make_flags: factorized_representation, the three style dims and the style weights beta_m{1,2,3}_style are set;
  * build_reference: the reference networks get their style dims, and the state dict of mopoe_ref.init_state gets the
    seeded style heads and widened feature_generators of tests/style_util.py;
  * Capture: gen_golden.Capture keeps only the last utils.reparameterize draw and replays one shape.  The forward draws
    four times (content, then the PA, Lateral and text styles): StyleCapture records and replays the ordered list.
Only inputs, seeds and numeric outputs are written.

Fixtures:
  g9_style_g0_s64        tiny full model (as g0_s64), joint_elbo: every output, klds_style, the loss and every parameter
                         gradient, eval / train_nodrop / train, in the compact form of tests/methods_util.py
  g9_style_jsd_g0_s64    the same for method='jsd'
  g9_style_c2            config #2's shape (128 px, D 128, B 64, DIM_img 64): scalars, checksums, per-network gradient norms
  g9_style_traj          three Adam steps (train_nodrop), as g3_traj
Usage:  python tests/tools/gen_golden_style.py [--only g0_s64 jsd_g0_s64 c2 traj]
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
import style_util as SU  # noqa: E402

MODS = ("PA", "Lateral", "text")
# style dims per fixture: three distinct values, some not multiples of 4
DIMS = {"g0_s64": (3, 5, 2), "jsd_g0_s64": (3, 5, 2), "c2": (32, 16, 64), "traj": (3, 5, 2)}
STYLE_WEIGHTS = (1.0, 0.5, 2.0)   # beta_m1_style, beta_m2_style, beta_m3_style
SEED_STYLE = 901

_state = SimpleNamespace(dims=None, caps=[], exp=None)


class StyleCapture:
    """gen_golden.Capture for the four draws of a factorized forward: eps is the ordered list [content, PA, Lateral, text]
    (eps.numpy() gives the content draw, so gen_golden's own packing code keeps working); force_eps replays such a list."""

    class EpsList(list):
        def numpy(self):
            return self[0].numpy()

    def __init__(self, model, force_eps=None):
        import mimic.utils.utils as U
        self.inner = _BaseCapture(model, None)       # dropout masks (its reparameterize wrapper is replaced below)
        self.U, self.orig = U, self.inner.orig
        self.masks = self.inner.masks
        self.eps, self.z = StyleCapture.EpsList(), []
        cap = self

        def wrapped(mu, logvar):
            i = len(cap.eps)
            if force_eps is not None:
                e = force_eps[i].to(mu.dtype)
                z = e * torch.exp(0.5 * logvar) + mu
            else:
                z = cap.orig(mu, logvar)
                e = ((z - mu) / torch.exp(0.5 * logvar)).detach()
            cap.eps.append(e.detach())
            cap.z.append(z.detach())
            return z

        U.reparameterize = wrapped
        _state.caps.append(self)

    def close(self):
        self.inner.close()


_BaseCapture = None
_last_out = [None]


def install(G):
    global _BaseCapture
    base_make_flags = G.make_flags

    def make_flags(cfg):
        f = base_make_flags(cfg)
        f.factorized_representation = True
        f.style_pa_dim, f.style_lat_dim, f.style_text_dim = _state.dims
        f.beta_m1_style, f.beta_m2_style, f.beta_m3_style = STYLE_WEIGHTS
        return f

    def build_reference(cfg, sd):
        from mimic.networks.ConvNetworksImgMimic import EncoderImg, DecoderImg
        from mimic.networks.ConvNetworksTextMimic import EncoderText, DecoderText
        from mimic.modalities.MimicPA import MimicPA
        from mimic.modalities.MimicLateral import MimicLateral
        from mimic.modalities.MimicText import MimicText
        from mimic.utils.BaseExperiment import BaseExperiment
        from mimic.networks.VAEtrimodalMimic import VAEtrimodalMimic
        f = G.make_flags(cfg)
        s = _state.dims
        mods = {"PA": MimicPA(EncoderImg(f, s[0]), DecoderImg(f, s[0]), f),
                "Lateral": MimicLateral(EncoderImg(f, s[1]), DecoderImg(f, s[1]), f),
                "text": MimicText(EncoderText(f, s[2]), DecoderText(f, s[2]), cfg.len_sequence, None, None, f)}
        exp = SimpleNamespace(flags=f, modalities=mods)
        exp.subsets = BaseExperiment.set_subsets(exp)
        exp.mm_vae = VAEtrimodalMimic(f, mods, exp.subsets)
        exp.mm_vae.load_state_dict(SU.style_state(cfg, sd, s, SEED_STYLE), strict=True)
        exp.rec_weights = {m: 0.33 for m in mods}
        exp.style_weights = dict(zip(MODS, STYLE_WEIGHTS))
        _state.exp = exp
        return exp

    base_pack = G.pack_outputs

    def pack_outputs(prefix, out, cap, model, store, rec_stride=1):
        base_pack(prefix, out, cap, model, store, rec_stride)
        pack_style(prefix + "/", out, cap, store)

    base_run = G.run_reference

    def run_reference(*a, **kw):
        out, cap = base_run(*a, **kw)
        _last_out[0] = out
        return out, cap

    _BaseCapture = G.Capture
    G.make_flags, G.build_reference, G.Capture, G.pack_outputs = make_flags, build_reference, StyleCapture, pack_outputs
    G.run_reference = run_reference


def pack_style(prefix, out, cap, store, full=True):
    """the style stage of one reference step: its noise, the style posteriors, klds_style and the decoder inputs"""
    from mimic.evaluation.losses import calc_klds_style
    lat = out["results"]["latents"]["modalities"]
    assert len(cap.eps) == 4, len(cap.eps)
    ks = calc_klds_style(_state.exp, out["results"])
    z = cap.z[0]
    for i, m in enumerate(MODS):
        store[f"{prefix}eps_style/{m}"] = cap.eps[1 + i].numpy()
        store[f"{prefix}klds_style/{m}_style"] = ks[m + "_style"].detach().numpy()
        mu, lv = lat[m + "_style"]
        if full:
            store[f"{prefix}enc/{m}_style/mu"] = mu.detach().numpy()
            store[f"{prefix}enc/{m}_style/logvar"] = lv.detach().numpy()
            store[f"{prefix}zcat/{m}"] = torch.cat((cap.z[1 + i], z), dim=1).numpy()
        else:
            store[f"{prefix}chk/enc/{m}_style/mu"] = GM.checksums(mu)
            store[f"{prefix}chk/enc/{m}_style/logvar"] = GM.checksums(lv)


def common(store, name):
    store["style_dims"] = np.array(_state.dims)
    store["style_weights"] = np.array(STYLE_WEIGHTS)
    store["seed_style"] = np.array(SEED_STYLE)
    store["style_fingerprint"] = SU.fingerprint(SU.style_weights(SU.cfg_of(store), _state.dims, SEED_STYLE))
    sd = _state.exp.mm_vae.state_dict()
    store["sd_keys"] = np.array(list(sd.keys()))
    store["sd_shapes"] = np.array([",".join(str(v) for v in t.shape) for t in sd.values()])
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
    run_epochs = G.import_reference()
    install(G)
    outdir = os.path.join(REPO, "tests", "golden")
    for name in ("g0_s64", "jsd_g0_s64", "c2", "traj"):
        if args.only and name not in args.only:
            continue
        _state.dims, _state.caps = DIMS[name], []
        GM.select_method(G, "jsd" if name.startswith("jsd") else "joint_elbo")
        if name.endswith("g0_s64"):
            store = GM.compact_g0(G.gen_g0(run_epochs, 64, 4))
        elif name == "c2":
            raw = G.gen_g1(run_epochs, 128, 128, 64, 64)
            pack_style("", _last_out[0], _state.caps[-1], raw, full=False)
            store = GM.compact_c2(raw)
        else:
            store = G.gen_g3(run_epochs)
            caps = _state.caps[-3:]
            for i, m in enumerate(MODS):
                store[f"eps_style/{m}"] = np.stack([c.eps[1 + i].numpy() for c in caps])
            final = _state.exp.mm_vae.state_dict()
            for k in ("encoder_text.feature_compressor.style_mu.weight", "decoder_lat.feature_generator.weight"):
                store["final/" + k] = final[k].numpy()
        store["method"] = np.array("jsd" if name.startswith("jsd") else "joint_elbo")
        common(store, name)
        path = os.path.join(outdir, f"g9_style_{name}.npz")
        np.savez_compressed(path, **store)
        print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(store)} arrays", flush=True)


if __name__ == "__main__":
    main()
