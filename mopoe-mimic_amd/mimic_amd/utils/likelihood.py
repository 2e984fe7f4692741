"""Importance-sampled likelihood estimates: the reference's mimic/utils/likelihood.py (get_latent_samples :13-32,
log_mean_exp :41-53, gaussian_log_pdf :56-67, unit_gaussian_log_pdf :70-80, log_marginal_estimate :83-147,
log_joint_estimate :150-220).

Same names, arguments and return values.  What changes is the data path of log p(x|z): the reference repeats the target
K times, builds the elementwise log_prob tensor ([K*B,1,S,S], or a [K*B,L,V] product with an int64 one-hot for text)
and sums it; here the decoders' output objects reduce per row in one HIP launch against the un-repeated target
(`log_prob_rows`, include/mopoe_hip.h: mopoe_laplace_logprob_rows / mopoe_token_logprob_rows).  `image` / `targets`
are therefore passed UN-repeated ([B,...]; text as float ids [B,L]).  The Gaussian terms are [K*B, D] torch ops.

factorized_representation=True: get_latent_samples also draws every style entry of latents['style'] ({m: (mu, logvar)}),
and the two estimates add each given style dict's log N(z_s; 0, I) - log q(z_s) as the reference does.  These public
mirrors stay torch arithmetic; the estimator itself (evaluation/eval_metrics/likelihood.py) runs the factorized case
through mopoe_lhood_style_sample / mopoe_lhood_estimates.
"""
from __future__ import annotations

import math

import torch

LOG2PI = float(math.log(2.0 * math.pi))


def _draw(mu, logvar, n_imp_samples, eps):
    mu_rep = mu.unsqueeze(0).repeat(n_imp_samples, 1, 1)
    lv_rep = logvar.unsqueeze(0).repeat(n_imp_samples, 1, 1)
    if eps is None:
        eps = torch.randn_like(mu_rep)
    z = eps.to(mu_rep.device) * torch.exp(0.5 * lv_rep) + mu_rep
    return {"mu": mu_rep, "logvar": lv_rep, "z": z}


def get_latent_samples(flags, latents, n_imp_samples, mod_names=None, eps=None, eps_style=None):
    """latents['content'] = (mu, logvar) [B,D] -> {'content': {'mu','logvar','z'} [K,B,D], 'style': {m: None}}.
    eps (tests): the [K,B,D] noise utils.reparameterize would draw.
    factorized_representation: latents['style'] = {m: (mu, logvar) [B,S_m]} -> 'style': {m: {'mu','logvar','z'} [K,B,S_m]},
    drawn after the content in the dict's key order (likelihood.py:21-28); eps_style (tests): {m: [K,B,S_m]}."""
    if not getattr(flags, "factorized_representation", False):
        mu, logvar = latents["content"]
        return {"content": _draw(mu, logvar, n_imp_samples, eps), "style": {key: None for key in (mod_names or [])}}
    content = _draw(latents["content"][0], latents["content"][1], n_imp_samples, eps)
    styles = {}
    for key, (s_mu, s_lv) in latents["style"].items():
        styles[key] = _draw(s_mu, s_lv, n_imp_samples, None if eps_style is None else eps_style[key])
    return {"content": content, "style": styles}


def log_mean_exp(x, dim=1):
    m = torch.max(x, dim=dim, keepdim=True)[0]
    return m + torch.log(torch.mean(torch.exp(x - m), dim=dim, keepdim=True))


def gaussian_log_pdf(x, mu, logvar):
    return torch.sum(-0.5 * LOG2PI - logvar / 2. - torch.pow(x - mu, 2) / (2. * torch.exp(logvar)), dim=1)


def unit_gaussian_log_pdf(x):
    return torch.sum(-0.5 * LOG2PI - torch.pow(x, 2) / 2., dim=1)


def _rows_log_prob(likelihood, target):
    if hasattr(likelihood, "log_prob_rows"):
        return likelihood.log_prob_rows(target)
    raise TypeError("the decoder output must be one of mimic_amd.plugins' fused distributions")


def _weights_to_estimate(flags, n_samples, log_weight_2d):
    # the reference views the sample-major [K*B] vector as (batch_size, n_samples) (likelihood.py:140,217): kept
    log_weight = log_weight_2d.view(flags.batch_size, n_samples)
    return torch.mean(log_mean_exp(log_weight, dim=1))


def log_marginal_estimate(flags, n_samples, likelihood, image, style, content, dynamic_prior=None):
    """log p(x_m) estimate for one modality.  likelihood: the decoder's distribution over [K*B,...]; image: the
    UN-repeated target [B,...]; content: {'mu','logvar','z'} [K*B,D]."""
    z, mu, logvar = content["z"], content["mu"], content["logvar"]
    log_p_x_given_z_2d = _rows_log_prob(likelihood, image)
    log_q_z_given_x_2d = gaussian_log_pdf(z, mu, logvar)
    if dynamic_prior is None:
        log_p_z_2d = unit_gaussian_log_pdf(z)
    else:
        log_p_z_2d = gaussian_log_pdf(z, dynamic_prior["mu"], dynamic_prior["logvar"])
    if style is not None:
        # style: {'mu','logvar','z'} [K*B,S] (likelihood.py:98-104,132-134)
        log_p_z_2d = unit_gaussian_log_pdf(style["z"]) + log_p_z_2d
        log_q_z_given_x_2d = gaussian_log_pdf(style["z"], style["mu"], style["logvar"]) + log_q_z_given_x_2d
    return _weights_to_estimate(flags, n_samples, log_p_x_given_z_2d + log_p_z_2d - log_q_z_given_x_2d)


def log_joint_estimate(flags, n_samples, likelihoods, targets, styles, content, dynamic_prior=None):
    """log p(x_1, ..., x_M) estimate; likelihoods / targets are dicts keyed like `styles` (the modality names)."""
    z, mu, logvar = content["z"], content["mu"], content["logvar"]
    log_joint_zs_2d = None
    for key in styles.keys():
        lp = _rows_log_prob(likelihoods[key], targets[key])
        log_joint_zs_2d = lp if log_joint_zs_2d is None else log_joint_zs_2d + lp
    if dynamic_prior is None:
        log_p_z_2d = unit_gaussian_log_pdf(z)
    else:
        log_p_z_2d = gaussian_log_pdf(z, dynamic_prior["mu"], dynamic_prior["logvar"])
    log_q_z_given_x_2d = gaussian_log_pdf(z, mu, logvar)
    # every given style dict adds its terms once per modality key (likelihood.py:160-175,211-215)
    for key in styles.keys():
        if styles[key] is not None:
            log_p_z_2d = log_p_z_2d + unit_gaussian_log_pdf(styles[key]["z"])
            log_q_z_given_x_2d = log_q_z_given_x_2d + gaussian_log_pdf(styles[key]["z"], styles[key]["mu"],
                                                                       styles[key]["logvar"])
    return _weights_to_estimate(flags, n_samples, log_joint_zs_2d + log_p_z_2d - log_q_z_given_x_2d)
