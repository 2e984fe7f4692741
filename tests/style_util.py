"""Factorized-representation (style latents) fixtures tests/golden/g9_style_*: the seeded extra weights, the flags and the
model builder shared by tests/tools/gen_golden_style.py and the CPU / GPU tests.

oracle/mopoe_ref.init_state knows no style parameters and gives each decoder's feature_generator the non-factorized
[5 * DIM, class_dim] shape.  style_state() adds the six style heads and replaces the three feature_generators with the
widened [5 * DIM, S_m + class_dim] ones, drawn by the rule of nn.Linear's default init (uniform in +-1/sqrt(fan_in), weight
and bias) from one seeded generator in sorted-key order.  The fixtures store the seed and a fingerprint, not the tensors."""
import contextlib

import numpy as np
import torch

import model_util
import mopoe_ref as R

MODS = (("PA", "encoder_pa", "decoder_pa", "style_pa_dim"), ("Lateral", "encoder_lat", "decoder_lat", "style_lat_dim"),
        ("text", "encoder_text", "decoder_text", "style_text_dim"))


def style_shapes(cfg, dims):
    """{state_dict key: shape} of the parameters the factorized model adds or widens; dims = (S_PA, S_Lateral, S_text)"""
    out = {}
    for (m, enc, dec, _), s in zip(MODS, dims):
        cin = 5 * (cfg.DIM_text if m == "text" else cfg.DIM_img)
        for head in ("style_mu", "style_logvar"):
            out[f"{enc}.feature_compressor.{head}.weight"] = (s, cin)
            out[f"{enc}.feature_compressor.{head}.bias"] = (s,)
        out[f"{dec}.feature_generator.weight"] = (cin, s + cfg.class_dim)
        out[f"{dec}.feature_generator.bias"] = (cin,)
    return out


def style_weights(cfg, dims, seed):
    gen = torch.Generator().manual_seed(int(seed))
    shapes = style_shapes(cfg, dims)
    out = {}
    for key in sorted(shapes):
        shape = shapes[key]
        w_shape = shapes[key[:-len("bias")] + "weight"] if key.endswith(".bias") else shape
        bound = 1.0 / float(np.sqrt(w_shape[1]))
        out[key] = (torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1).mul(bound).float()
    return out


def style_state(cfg, base_sd, dims, seed):
    """the reference-layout state dict of the factorized model: base_sd (mopoe_ref.init_state) + style_weights"""
    sd = dict(base_sd)
    sd.update(style_weights(cfg, dims, seed))
    return sd


def fingerprint(tensors):
    """[sum, sum of squares, sum of index-weighted values] over the tensors in sorted-key order"""
    out = []
    for k in sorted(tensors):
        t = tensors[k].double().flatten()
        out.append([t.sum().item(), (t * t).sum().item(), (t * torch.arange(1, t.numel() + 1, dtype=torch.float64)).sum().item()])
    return np.array(out)


@contextlib.contextmanager
def style_flags(dims, method="joint_elbo", **extra):
    """model_util.default_flags with factorized_representation and the three style dims (and `method`)"""
    from mimic_amd.utils.filehandling import get_method
    orig = model_util.default_flags

    def flags(**kw):
        kw.update(factorized_representation=True, style_pa_dim=int(dims[0]), style_lat_dim=int(dims[1]),
                  style_text_dim=int(dims[2]), **extra)
        f = orig(**kw)
        f.method = method
        return get_method(f)

    model_util.default_flags = flags
    try:
        yield
    finally:
        model_util.default_flags = orig


def build_exp(cfg, sd, device, mode="train_nodrop", masks=None, eps=None, dims=(3, 5, 2), method="joint_elbo",
              compute_dtype="fp32"):
    """model_util.build_exp for the factorized model; eps: None or the reference's four draws [content, PA, Lateral, text]
    (replayed through eps_source / style_eps_source)"""
    with style_flags(dims, method):
        exp = model_util.build_exp(cfg, sd, device, mode, masks, None, compute_dtype)
    if eps is not None:
        set_eps(exp.mm_vae, eps, device)
    return exp


def set_eps(model, eps, device):
    e = [torch.as_tensor(t).float().to(device) for t in eps]
    model.eps_source = lambda b, d, dev: e[0]
    model.style_eps_source = lambda m, b, s, dev: e[1 + ("PA", "Lateral", "text").index(m)]


def fixture_eps(g, prefix):
    """the four draws of a fixture: [content, PA, Lateral, text]"""
    return [torch.from_numpy(g[f"{prefix}eps"])] + [torch.from_numpy(g[f"{prefix}eps_style/{m}"]) for m, *_ in MODS]


def g9_state(g, cfg):
    """the fixture's weights: the base state regenerated from its seed (methods_util.g8_state) + the seeded style weights,
    both checked against their fingerprints"""
    import methods_util as MU
    dims = tuple(int(v) for v in g["style_dims"])
    sd = MU.g8_state(g, cfg) if "sd_fingerprint" in g.files else R.init_state(cfg, seed=int(g["seed_weights"]))
    extra = style_weights(cfg, dims, int(g["seed_style"]))
    np.testing.assert_allclose(fingerprint(extra), g["style_fingerprint"], rtol=1e-6)
    sd.update(extra)
    return sd, dims


def cfg_of(g):
    from golden_util import cfg_from
    return cfg_from(g["cfg"])
