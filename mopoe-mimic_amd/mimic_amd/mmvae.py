"""MoPoE model: encoders -> fused latent kernel -> decoders.

API of the reference's ``BaseMMVae`` (mimic/utils/BaseMMVae.py:16-231) and ``VAEtrimodalMimic``
(mimic/networks/VAEtrimodalMimic.py:12-163) for ``method`` 'joint_elbo' (MoPoE), 'moe' (the MMVAE baseline) and 'jsd'
(mixture of experts with a dynamic prior); results-dict schema as in SURVEY.md §8(a3,a7).  The 7-subset Python loop, the
fusion (PoE for joint_elbo, mixture selection for moe/jsd), the joint mixture selection, the KL passes (and the dynamic
prior of jsd) and the reparameterisation of the reference are ONE kernel here (ops.latent_fwd, ops.latent_mixture_fwd)
and one autograd node.  'poe' (the MVAE baseline) has no path: the reference cannot train it (set_fusion_functions).
"""
from __future__ import annotations

import contextlib
import os
from abc import ABC, abstractmethod
from functools import lru_cache
from itertools import combinations
from typing import Dict, List, Mapping, Optional, Tuple

import torch
import torch.nn as nn

from . import ops

MOD_SLOT = {"PA": 0, "Lateral": 1, "text": 2}

from .nets import run_group
from .lanes import NET_STREAMS, NET_STREAM_SET, ModalityLanes as _ModalityLanes, _net_streams  # noqa: F401


def reweight_weights(w):
    return w / w.sum()


@lru_cache(maxsize=None)
def mixture_row_starts(num_samples: int, k: int) -> List[int]:
    """Row offsets of the batch partition over k mixture components
    (utils.mixture_component_selection, mimic/utils/utils.py:55-77, with weights 1/k re-normalised in
    fp32 exactly as BaseMMVae.inference/moe_fusion do: BaseMMVae.py:185-187,104).  Host integers: the
    reference's six device->host syncs per step (utils.py:69) disappear."""
    w = reweight_weights((1 / float(k)) * torch.ones(k))
    starts, start = [0], 0
    for i in range(k):
        end = num_samples if i == k - 1 else start + int(torch.floor(num_samples * w[i]))
        starts.append(end)
        start = end
    return starts


@lru_cache(maxsize=None)
def kl_weights(k: int) -> List[float]:
    """weights of calc_group_divergence_moe after divergence_static_prior's reweighting
    (BaseMMVae.py:71-85): 1/k re-normalised twice in fp32."""
    w = reweight_weights(reweight_weights((1 / float(k)) * torch.ones(k)))
    return [float(v) for v in w]


def subset_keys(names=("PA", "Lateral", "text")) -> List[Tuple[str, Tuple[str, ...]]]:
    out = []
    for n in range(1, len(names) + 1):
        for combo in combinations(names, n):
            members = tuple(sorted(combo))
            out.append(("_".join(members), members))
    return out


class _LatentFuse(torch.autograd.Function):
    """(mu, logvar) of the present modalities + eps -> mus, logvars [K,B,D], joint (mu, logvar), z,
    klds [K], joint_divergence."""

    @staticmethod
    def forward(ctx, present, row_start, w, norm, eps, *enc):
        mu_in, lv_in, j = [None] * 3, [None] * 3, 0
        for slot in range(3):
            if present[slot]:
                mu_in[slot], lv_in[slot] = enc[j].contiguous(), enc[j + 1].contiguous()
                j += 2
        outs = ops.latent_fwd(mu_in, lv_in, eps, row_start, w, norm)
        ctx.args = (mu_in, lv_in, eps, row_start, w, norm, present)
        ctx.set_materialize_grads(False)   # outputs the loss never touches arrive as None (the kernel takes null
        return outs                        # pointers), not as five zero-filled tensors per step

    @staticmethod
    def backward(ctx, g_mus, g_lvs, g_jm, g_jl, g_z, g_klds, g_jd):
        mu_in, lv_in, eps, row_start, w, norm, present = ctx.args
        c = lambda t: None if t is None else t.contiguous()
        dmu, dlv = ops.latent_bwd(mu_in, lv_in, eps, row_start, w, norm, c(g_mus), c(g_lvs), c(g_jm), c(g_jl),
                                  c(g_z), c(g_klds), c(g_jd))
        grads = []
        for slot in range(3):
            if present[slot]:
                grads += [dmu[slot], dlv[slot]]
        return (None, None, None, None, None, *grads)


class _LatentMixture(torch.autograd.Function):
    """method 'moe' / 'jsd': (mu, logvar) of the present modalities + eps -> subset (mu, logvar) [K,B,D], component
    (mu, logvar) [C,B,D], joint (mu, logvar), z, klds [K], individual_divs [C], joint_divergence (+ the dynamic prior's
    (mu, logvar) for jsd)."""

    @staticmethod
    def forward(ctx, method, present, member_rs, comp_rs, w, norm, eps, *enc):
        mu_in, lv_in, j = [None] * 3, [None] * 3, 0
        for slot in range(3):
            if present[slot]:
                mu_in[slot], lv_in[slot] = enc[j].contiguous(), enc[j + 1].contiguous()
                j += 2
        outs = ops.latent_mixture_fwd(method, mu_in, lv_in, eps, member_rs, comp_rs, w, norm)
        ctx.args = (method, mu_in, lv_in, eps, member_rs, comp_rs, w, norm, present)
        ctx.set_materialize_grads(False)
        return outs if method == "jsd" else outs[:10]   # (no dynamic prior for moe)

    @staticmethod
    def backward(ctx, *g):
        method, mu_in, lv_in, eps, member_rs, comp_rs, w, norm, present = ctx.args
        g = [None if t is None else t.contiguous() for t in g] + [None] * (12 - len(g))
        dmu, dlv = ops.latent_mixture_bwd(method, mu_in, lv_in, eps, member_rs, comp_rs, w, norm, *g)
        grads = []
        for slot in range(3):
            if present[slot]:
                grads += [dmu[slot], dlv[slot]]
        return (None, None, None, None, None, None, None, *grads)


class _LatentStyle(torch.autograd.Function):
    """style stage of the factorized representation, after the content latent node: z + the present modalities' style
    (mu, logvar) + their noise -> the decoder inputs zcat_m = [z_style_m | z] (3, None for absent modalities) and
    klds_style [3]."""

    @staticmethod
    def forward(ctx, present, eps_s, norm, z, *enc):
        smu, slv, j = [None] * 3, [None] * 3, 0
        for slot in range(3):
            if present[slot]:
                smu[slot], slv[slot] = enc[j].contiguous(), enc[j + 1].contiguous()
                j += 2
        z = z.contiguous()
        zcat, klds = ops.latent_style_fwd(smu, slv, eps_s, z, norm)
        ctx.args = (smu, slv, eps_s, z.shape[1], norm, present)
        ctx.set_materialize_grads(False)
        return (*zcat, klds)

    @staticmethod
    def backward(ctx, g0, g1, g2, g_klds):
        smu, slv, eps_s, d, norm, present = ctx.args
        c = lambda t: None if t is None else t.contiguous()
        dmu, dlv, g_z = ops.latent_style_bwd(smu, slv, eps_s, d, norm, [c(g0), c(g1), c(g2)], c(g_klds))
        grads = []
        for slot in range(3):
            if present[slot]:
                grads += [dmu[slot], dlv[slot]]
        return (None, None, None, g_z, *grads)


class BaseMMVae(ABC, nn.Module):
    def __init__(self, flags, modalities, subsets):
        super().__init__()
        self.num_modalities = len(modalities.keys())
        self.flags = flags
        self.modalities = modalities
        self.subsets = subsets
        self.eps_source = None  # tests inject the reference's noise here: callable (B, D, device) -> tensor
        # ... and the style noise of the factorized representation here: callable (m_key, B, S, device) -> tensor
        self.style_eps_source = None
        self.set_fusion_functions()

    @abstractmethod
    def forward(self, input_batch):
        ...

    @abstractmethod
    def encode(self, input_batch):
        ...

    def set_fusion_functions(self):
        """BaseMMVae.py:51-69, in its order of precedence: moe, jsd, poe, joint_elbo (utils.filehandling.get_method sets
        the one flag of a method).  self.method names the latent kernel the model runs."""
        f = self.flags
        if getattr(f, "modality_moe", False):
            self.method = "moe"
        elif getattr(f, "modality_jsd", False):
            self.method = "jsd"
        elif getattr(f, "modality_poe", False):
            raise NotImplementedError(
                "method='poe' (MVAE) has no HIP path: the reference cannot train it either -- calc_poe_loss "
                "(mimic/evaluation/losses.py:66) calls the model with a one-modality dict, and VAEtrimodalMimic.forward "
                "then indexes input_batch for all three modalities (mimic/networks/VAEtrimodalMimic.py:46): KeyError")
        elif getattr(f, "joint_elbo", False):
            self.method = "joint_elbo"
        else:
            raise NotImplementedError("no method selected: set flags.method to 'joint_elbo', 'moe' or 'jsd' and apply "
                                      "utils.filehandling.get_method")
        w = reweight_weights(torch.Tensor(self.flags.alpha_modalities))
        self.weights = w.to(self.flags.device)

    def _draw_eps(self, b, d, device):
        if self.eps_source is not None:
            return self.eps_source(b, d, device).contiguous()
        return torch.randn(b, d, device=device)

    def _draw_style_eps(self, m_key, b, s, device):
        if self.style_eps_source is not None:
            return self.style_eps_source(m_key, b, s, device).contiguous()
        return torch.randn(b, s, device=device)

    def inference(self, input_batch, num_samples=None) -> Mapping[str, any]:
        """BaseMMVae.inference (:139-196): accepts partial modality dicts."""
        enc_mods = self.encode(input_batch)
        latents = {"modalities": enc_mods}
        present = tuple(name in input_batch for name in ("PA", "Lateral", "text"))
        avail = sum(1 << i for i, p in enumerate(present) if p)
        active = [(key, members) for (key, members), m in zip(subset_keys(), ops.SUBSET_MASKS) if (m & ~avail) == 0]
        k = len(active)
        first = enc_mods[[n for n, p in zip(("PA", "Lateral", "text"), present) if p][0]][0]
        b, d = first.shape
        enc_flat = []
        for name, p in zip(("PA", "Lateral", "text"), present):
            if p:
                enc_flat += [enc_mods[name][0], enc_mods[name][1]]
        eps = self._draw_eps(b, d, first.device)
        if self.method != "joint_elbo":
            return self._mixture_inference(latents, present, active, enc_flat, eps, first)
        row_start = mixture_row_starts(b, k)
        mus, lvs, jm, jl, z, klds, jd = _LatentFuse.apply(present, row_start, kl_weights(k),
                                                          float(self.flags.batch_size), eps, *enc_flat)
        latents["mus"], latents["logvars"] = mus, lvs
        latents["weights"] = (1 / float(k)) * torch.ones(k, device=first.device)
        latents["joint"] = [jm, jl]
        latents["subsets"] = {key: [mus[i], lvs[i]] for i, (key, _m) in enumerate(active)}
        # by-products of the fused kernel, consumed by forward() / losses.calc_klds
        latents["_z"], latents["_klds"], latents["_joint_divergence"] = z, klds, jd
        latents["_subset_order"] = [key for key, _m in active]
        return latents

    def _mixture_inference(self, latents, present, active, enc_flat, eps, first):
        """moe / jsd (BaseMMVae.py:139-196 with moe_fusion): every subset is a mixture selection of its members' rows,
        the components are the singletons (+ the N(0,I) prior for jsd, BaseMMVae.py:178-184, built with the ACTUAL
        batch size where the reference uses flags.batch_size), the joint is a mixture selection over the components."""
        b = first.shape[0]
        n = sum(present)
        c = n + (self.method == "jsd")
        # subset members and components carry weights 1/m re-normalised (moe_fusion): the floor(B*w) partitions
        member_rs = [mixture_row_starts(b, m) for m in (1, 2, 3)]
        # joint divergence weights: divergence_static_prior re-normalises 1/n (moe); calc_alphaJSD_modalities takes the
        # alphas 1/(n+1) as they are (jsd)
        w = kl_weights(n) if self.method == "moe" else [float(torch.tensor(1 / float(c)))] * c
        outs = _LatentMixture.apply(self.method, present, member_rs, mixture_row_starts(b, c), w,
                                    float(self.flags.batch_size), eps, *enc_flat)
        sub_mu, sub_lv, comp_mu, comp_lv, jm, jl, z, klds, indiv, jd = outs[:10]
        latents["mus"], latents["logvars"] = comp_mu, comp_lv
        latents["weights"] = (1 / float(c)) * torch.ones(c, device=first.device)
        latents["joint"] = [jm, jl]
        latents["subsets"] = {key: [sub_mu[i], sub_lv[i]] for i, (key, _m) in enumerate(active)}
        latents["_z"], latents["_klds"], latents["_joint_divergence"] = z, klds, jd
        latents["_subset_order"] = [key for key, _m in active]
        latents["_individual_divs"] = indiv
        latents["_dyn_prior"] = list(outs[10:12]) if self.method == "jsd" else None
        return latents

    def generate(self, num_samples=None):
        if num_samples is None:
            num_samples = self.flags.batch_size
        z_class = torch.randn(num_samples, self.flags.class_dim, device=self.flags.device)
        return self.generate_from_latents({"content": z_class, "style": self.get_random_styles(num_samples)})

    def generate_from_latents(self, latents):
        suff_stats = self.generate_sufficient_statistics_from_latents(latents)
        return {m_key: suff_stats[m_key].mean for m_key in latents["style"].keys()}

    def cond_generation(self, latent_distributions, num_samples=None):
        if num_samples is None:
            num_samples = self.flags.batch_size
        style_latents = self.get_random_styles(num_samples)
        out = {}
        for key, (mu, logvar) in latent_distributions.items():
            eps = self._draw_eps(mu.shape[0], mu.shape[1], mu.device)   # (tests inject the noise through eps_source)
            content = eps * torch.exp(0.5 * logvar) + mu  # off the training path: plain torch on device
            out[key] = self.generate_from_latents({"content": content, "style": style_latents})
        return out


class VAEtrimodalMimic(BaseMMVae, nn.Module):
    def __init__(self, flags, modalities, subsets):
        super().__init__(flags, modalities, subsets)
        dims = {"style_pa_dim": flags.style_pa_dim, "style_lat_dim": flags.style_lat_dim,
                "style_text_dim": flags.style_text_dim}
        self.factorized = bool(getattr(flags, "factorized_representation", False))
        # the two combinations the reference cannot run: encode() stores no '<m>_style' pair (forward: KeyError), or the
        # decoders' feature_generator expects [z_style | z] and gets z (shape mismatch)
        if self.factorized and any(v <= 0 for v in dims.values()):
            bad = ", ".join(k for k, v in dims.items() if v <= 0)
            raise ValueError(f"factorized_representation needs style_pa_dim, style_lat_dim and style_text_dim > 0; "
                             f"{bad} = 0")
        if not self.factorized and any(v > 0 for v in dims.values()):
            bad = ", ".join(f"{k}={v}" for k, v in dims.items() if v > 0)
            raise ValueError(f"{bad} without factorized_representation: the style latents are used only with "
                             "factorized_representation=True")
        dev = flags.device
        self.encoder_pa = modalities["PA"].encoder.to(dev)
        self.encoder_lat = modalities["Lateral"].encoder.to(dev)
        self.encoder_text = modalities["text"].encoder.to(dev)
        self.decoder_pa = modalities["PA"].decoder.to(dev)
        self.decoder_lat = modalities["Lateral"].decoder.to(dev)
        self.decoder_text = modalities["text"].decoder.to(dev)
        self.lhood_pa = modalities["PA"].likelihood
        self.lhood_lat = modalities["Lateral"].likelihood
        self.lhood_text = modalities["text"].likelihood
        # the word decoder's head stays factored (logits + row log-sum-exp) on this model's own forward: the [B, L, V] fp32
        # log-softmax tensor is made only on demand (nets.DecoderText.lazy_head, plugins.LogitsWithLse; MOPOE_LAZY_HEAD=0:
        # the dense form of rounds 1-3)
        self.decoder_text.lazy_head = os.environ.get("MOPOE_LAZY_HEAD", "1") != "0"
        # prefixes let a replayed dropout-mask dict use whole-model names (tests)
        for name in ("encoder_pa", "encoder_lat", "encoder_text", "decoder_pa", "decoder_lat", "decoder_text"):
            getattr(self, name)._net_name = name

    def forward(self, input_batch) -> Mapping[str, any]:
        latents = self.inference(input_batch)
        results = {"latents": latents, "group_distr": latents["joint"],
                   "joint_divergence": latents["_joint_divergence"].view(()),
                   "individual_divs": latents.get("_individual_divs", latents["_klds"]),
                   "dyn_prior": latents.get("_dyn_prior")}
        z = latents["_z"]
        dec_in = {m_key: (None, z) for m_key in MOD_SLOT}
        if self.factorized:
            dec_in = self._style_stage(latents, input_batch, z)
        # the decoders are independent: one grouped autograd node, each network on its modality's stream (nets.run_group)
        items = [(m_key, net, dec_in[m_key])
                 for m_key, net in (("Lateral", self.decoder_lat), ("PA", self.decoder_pa), ("text", self.decoder_text))
                 if m_key in self.modalities and input_batch[m_key] is not None]
        dec = dict(zip([m for m, _, _ in items], run_group(items)))
        rec = {}
        for m_key in self.modalities:
            if m_key not in dec:
                continue
            if m_key == "Lateral":
                rec[m_key] = self.lhood_lat(*dec[m_key])
            elif m_key == "PA":
                rec[m_key] = self.lhood_pa(*dec[m_key])
            elif m_key == "text":
                rec[m_key] = self.lhood_text(logits=dec[m_key][0])
        results["rec"] = rec
        return results

    def _style_stage(self, latents, input_batch, z):
        """style draws (after the content noise, in the order PA, Lateral, text: VAEtrimodalMimic.py:31-62) and the
        decoder inputs [z_style_m | z], in one node (_LatentStyle); latents['_klds_style'] [3] is its KL by-product"""
        from .nets import ZCAT
        mods = latents["modalities"]
        present = tuple(name in input_batch and mods.get(name + "_style", [None])[0] is not None for name in MOD_SLOT)
        eps_s, enc = [None] * 3, []
        for name, slot in MOD_SLOT.items():
            if present[slot]:
                mu, lv = mods[name + "_style"]
                eps_s[slot] = self._draw_style_eps(name, mu.shape[0], mu.shape[1], mu.device)
                enc += [mu, lv]
        outs = _LatentStyle.apply(present, eps_s, float(self.flags.batch_size), z, *enc)
        latents["_klds_style"] = outs[3]
        return {name: (ZCAT, outs[slot]) for name, slot in MOD_SLOT.items()}

    def encode(self, input_batch):
        """{'PA', 'PA_style', 'Lateral', 'Lateral_style', 'text', 'text_style'} in the reference's key order
        (VAEtrimodalMimic.py:64-93); the '<m>_style' pairs exist when the encoders have style heads, and are [None, None]
        for an absent modality"""
        items = [(name, enc, (input_batch[name],))
                 for name, enc in (("PA", self.encoder_pa), ("Lateral", self.encoder_lat), ("text", self.encoder_text))
                 if name in input_batch.keys()]
        outs = {name: list(out) for (name, _, _), out in zip(items, run_group(items))}
        latents = {}
        for name in MOD_SLOT:
            if name not in outs:
                latents[name + "_style"] = [None, None]
                latents[name] = [None, None]
                continue
            latents[name] = outs[name][:2]
            if len(outs[name]) == 4:
                latents[name + "_style"] = outs[name][2:]
        return latents

    def get_random_styles(self, num_samples):
        """N(0, I) styles for generation (VAEtrimodalMimic.py:95-107; tests inject them through style_eps_source)"""
        if not self.factorized:
            return {"PA": None, "Lateral": None, "text": None}
        f, dev = self.flags, self.flags.device
        return {m: self._draw_style_eps(m, num_samples, s, dev)
                for m, s in (("PA", f.style_pa_dim), ("Lateral", f.style_lat_dim), ("text", f.style_text_dim))}

    def get_random_style_dists(self, num_samples):
        dev, f = self.flags.device, self.flags
        z = lambda d: [torch.zeros(num_samples, d, device=dev), torch.zeros(num_samples, d, device=dev)]
        return {"PA": z(f.style_pa_dim), "Lateral": z(f.style_lat_dim), "text": z(f.style_text_dim)}

    def generate_sufficient_statistics_from_latents(self, latents):
        content = latents["content"]
        return {"PA": self.lhood_pa(*self.decoder_pa(latents["style"]["PA"], content)),
                "Lateral": self.lhood_lat(*self.decoder_lat(latents["style"]["Lateral"], content)),
                "text": self.lhood_text(logits=self.decoder_text(latents["style"]["text"], content)[0])}

    def save_networks(self):
        f = self.flags
        for net, fn in ((self.encoder_pa, f.encoder_save_m1), (self.decoder_pa, f.decoder_save_m1),
                        (self.encoder_lat, f.encoder_save_m2), (self.decoder_lat, f.decoder_save_m2),
                        (self.encoder_text, f.encoder_save_m3), (self.decoder_text, f.decoder_save_m3)):
            torch.save(net.state_dict(), os.path.join(f.dir_checkpoints, fn))

    # ---- helpers used by the tests / DP glue ------------------------------------------------------
    def set_mask_replay(self, masks: Optional[Dict[str, torch.Tensor]]):
        from .trunk import MaskSource
        for name in ("encoder_pa", "encoder_lat", "encoder_text", "decoder_pa", "decoder_lat", "decoder_text"):
            net = getattr(self, name)
            net.mask_source = MaskSource(masks, prefix=name + ".") if masks is not None else MaskSource()

    def reference_named_grads(self) -> Dict[str, torch.Tensor]:
        """parameter gradients keyed by the reference's parameter names, in the reference's layouts."""
        from .layout import PackedConv
        out, packed = {}, set()
        for mname, mod in self.named_modules():
            if isinstance(mod, PackedConv):
                packed.add(mname + ".weight")
                if mod.weight.grad is not None:
                    out[mname + ".weight"] = mod.ref_grad()
        for pname, p in self.named_parameters():
            if pname not in packed and p.grad is not None:
                out[pname] = p.grad
        return out
