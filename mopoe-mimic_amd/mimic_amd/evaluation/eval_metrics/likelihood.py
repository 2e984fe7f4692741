"""Likelihood evaluation: the reference's mimic/evaluation/eval_metrics/likelihood.py
(calc_log_likelihood_batch :17-96, estimate_likelihoods :99-140).

Per subset: K importance samples per row from the subset posterior, ONE batched decode of the K*B latents through the
three decoders (eval mode; the reference's DecoderText chunks inputs larger than flags.batch_size,
ConvNetworksTextMimic.py:59-66 -- with running statistics the chunking does not change the result, so it is not
needed here), per-row log p(x|z) reductions on the device, log-mean-exp of the importance weights.

factorized_representation=True (_factorized_batch) keeps the reference's quirk: its lines :49-52 read
l_style_rep[mod.name] with `mod` left over from the loop at :29, i.e. the LAST subset member in sorted-name order, so
every modality is decoded from that member's style sample [z_style_last | z]; the prior draws of the other modalities
are never used.  A marginal adds that style term only for a subset member (:77), the joint adds it once per modality
key (3x).  This needs style_pa_dim == style_lat_dim == style_text_dim (otherwise the reference's decoders fail on the
shape).  Device work per subset: mopoe_lhood_style_sample (draws, decoder input, Gaussian terms), the three decodes,
three *_logprob_rows launches, mopoe_lhood_estimates (the four log-mean-exp estimates); no ATen elementwise op.
"""
from __future__ import annotations

import numpy as np
import torch

from ... import ops
from ...utils.likelihood import get_latent_samples, log_joint_estimate, log_marginal_estimate

MODS = ("PA", "Lateral", "text")
STYLE_FLAGS = ("style_pa_dim", "style_lat_dim", "style_text_dim")


def check_style_dims(flags):
    """the factorized estimator decodes every modality from one style sample: the three style dims must agree"""
    dims = [int(getattr(flags, k)) for k in STYLE_FLAGS]
    if len(set(dims)) != 1:
        raise ValueError("the likelihood estimator of factorized_representation decodes every modality from the last "
                         "subset member's style sample (the reference's eval_metrics/likelihood.py:49-52), so it needs "
                         f"style_pa_dim == style_lat_dim == style_text_dim; got {', '.join(f'{k}={v}' for k, v in zip(STYLE_FLAGS, dims))}")


def _factorized_batch(exp, latents, subset_key, subset, batch, num_imp_samples, eps, eps_style):
    from ...nets import ZCAT
    flags, model = exp.flags, exp.mm_vae
    check_style_dims(flags)
    mu, logvar = latents["subsets"][subset_key]
    b, d = mu.shape
    last = subset[-1].name                       # subsets are sorted by name: Lateral < PA < text
    s_mu, s_lv = latents["modalities"].get(last + "_style", [None, None])
    if s_mu is None or s_lv is None:             # (get_random_style_dists: the style stays N(0, 0))
        s_mu = s_lv = torch.zeros(b, int(flags.style_pa_dim), device=mu.device)
    if eps is None:
        eps = torch.randn(num_imp_samples, b, d, device=mu.device)
    e_s = eps_style[last] if eps_style is not None else torch.randn(num_imp_samples, b, s_mu.shape[1], device=mu.device)
    c = lambda t: t.to(mu.device, torch.float32).contiguous()
    zcat, t_c, t_s = ops.lhood_style_sample(c(mu), c(logvar), c(eps), c(s_mu), c(s_lv), c(e_s))
    gen = model.generate_sufficient_statistics_from_latents({"content": zcat, "style": {m: ZCAT for m in MODS}})
    lp = [gen[m].log_prob_rows(batch[m]) for m in MODS]
    mask = sum(1 << MODS.index(mod.name) for mod in subset)
    est = ops.lhood_estimates(lp, t_c, t_s, num_imp_samples, mask)
    return {"PA": est[0], "Lateral": est[1], "text": est[2], "joint": est[3]}


def calc_log_likelihood_batch(exp, latents, subset_key, subset, batch, num_imp_samples=10, eps=None, eps_style=None):
    """-> {modality name: log p(x_m) estimate, ..., 'joint': log p(x_1..x_M) estimate} (0-dim tensors).
    batch: dict of device tensors (text as float ids [B,L]); eps (tests): the [K,B,D] noise; eps_style (tests,
    factorized_representation): {m: [K,B,S]} style noise, of which the last subset member's is used."""
    flags, model, mods = exp.flags, exp.mm_vae, exp.modalities
    if getattr(flags, "factorized_representation", False):
        return _factorized_batch(exp, latents, subset_key, subset, batch, num_imp_samples, eps, eps_style)
    s_dist = latents["subsets"][subset_key]
    n_total = s_dist[0].shape[0] * num_imp_samples
    lat = get_latent_samples(flags, {"content": s_dist, "style": None}, num_imp_samples, mods.keys(), eps=eps)
    c = {k: v.view(n_total, -1) for k, v in lat["content"].items()}
    styles = {m_key: None for m_key in mods}
    gen = model.generate_sufficient_statistics_from_latents({"content": c["z"].contiguous(), "style": dict(styles)})
    ll = {}
    for m_key, mod in mods.items():
        ll[mod.name] = log_marginal_estimate(flags, num_imp_samples, gen[mod.name], batch[mod.name], None, c)
    ll["joint"] = log_joint_estimate(flags, num_imp_samples, gen, batch, styles, c)
    return ll


def estimate_likelihoods(exp, loader=None, num_imp_samples=6):
    """Mean estimates over a test loader for every non-empty subset (likelihood.py:99-140).  loader yields
    ((dict of tensors), labels) with exactly flags.batch_size rows (the reference drops the last partial batch)."""
    model, mods = exp.mm_vae, exp.modalities
    if loader is None:
        raise ValueError("pass the test loader (dataset plumbing is outside the hot path)")
    subsets = {k: v for k, v in exp.subsets.items() if k != ""}
    lhoods = {s_key: {**{m_key: [] for m_key in mods}, "joint": []} for s_key in subsets}
    was_training = model.training
    model.eval()
    with torch.no_grad():
        for batch in loader:
            batch_d = {k: v.to(exp.flags.device) for k, v in batch[0].items()}
            latents = model.inference(batch_d)
            pending = {}
            for s_key, subset in subsets.items():
                pending[s_key] = calc_log_likelihood_batch(exp, latents, s_key, subset, batch_d, num_imp_samples)
            # one device->host transfer per batch for all 7 x 4 scalars (the reference: 28 .item() syncs)
            keys = [(s, m) for s in pending for m in pending[s]]
            vals = torch.stack([pending[s][m].reshape(()) for s, m in keys]).tolist()
            for (s, m), v in zip(keys, vals):
                lhoods[s][m].append(v)
    model.train(was_training)
    return {s: {m: float(np.mean(np.array(v))) for m, v in d.items()} for s, d in lhoods.items()}
