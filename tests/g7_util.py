"""The GPU side of the G7 fixtures (oracle/gen_g7.py): rebuild a case's seeded weights / inputs / noise, run the HIP path,
compare forward scalars, reconstructions and EVERY parameter gradient with the stored full-size truths (the reference's own
fp32 / fp64 passes; the oracle's bf16-mode pass for the bf16 family).  No CPU forward or backward runs on the GPU box."""
import os

import numpy as np
import torch

import mopoe_ref as R
from golden_util import (GOLDEN, load, cfg_from, PackedGrad, unpack_mask, weights_fingerprint, rec_sample_index)
from model_util import build_exp
from mimic_amd import run_epochs as RE


def _log(path, line):
    os.makedirs("gpurun_out", exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def g7_inputs(g):
    """(cfg, state dict, batch, eps, masks) of a G7 case, regenerated from its seeds + the fixture's moved pixels / mask bits"""
    cfg = cfg_from(g["cfg"])
    seed, nrow = int(g["seed"]), cfg.batch_size
    sd = R.init_state(cfg, seed=seed)
    np.testing.assert_allclose(weights_fingerprint(sd), g["weights_fingerprint"], rtol=1e-12,
                               err_msg="the seeded weights differ from the ones the fixture was made with")
    batch, eps = R.synthetic_batch(cfg, nrow, seed=seed + 1)
    for m in ("PA", "Lateral"):
        idx = torch.from_numpy(g[f"in/{m}_moved_idx"]).long()
        if idx.numel():
            batch[m].view(-1)[idx] = torch.from_numpy(g[f"in/{m}_moved_u8"]).float() / 255.0
    fp = np.array([batch["PA"].double().sum().item(), batch["Lateral"].double().sum().item(),
                   batch["text"].double().sum().item(), eps.double().sum().item()])
    np.testing.assert_allclose(fp, g["in/fingerprint"], rtol=1e-12, err_msg="the seeded inputs differ from the fixture's")
    masks = None
    if str(g["mode"]) == "train":
        masks = {k[5:-5]: unpack_mask(g[k], tuple(int(v) for v in g[k[:-5] + "/shape"]))
                 for k in g.files if k.startswith("mask/") and k.endswith("/bits")}
    return cfg, sd, batch, eps, masks


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


def _scalars(got):
    out = {"total_loss": got["total_loss"].item()}
    out.update({f"klds/{k}": v.item() for k, v in got["klds"].items()})
    out.update({f"log_probs/{k}": v.item() for k, v in got["log_probs"].items()})
    return out


def _rec_samples(got, m):
    t = got["results"]["rec"][m].loc.flatten()
    return t[rec_sample_index(t.numel()).to(t.device)].double().cpu()


# Parameters whose gradient is analytically (almost) zero: a per-channel constant added in front of a BatchNorm is removed by
# it, so the bias of a conv that feeds a BN (shortcut conv -> BN_s; conv1 -> bn2) only sees rounding noise, and the shortcut
# BatchNorm's own bias is (up to zero-padding effects at the borders) a constant in front of the next block's bn1 / shortcut
# BN.  Their "relative" error is noise over noise; they are held to an absolute bound instead.
def near_zero_grad(name):
    return (name.endswith("sample.0.bias") or name.endswith(".conv1.bias") and ("resblock_" in name or ".generator." in name)
            or name.endswith("sample.1.bias"))


def check_fp32_case(case, q90_tol=2e-3, trim_tol=4e-3, l2_tol=5e-2, zero_tol=5e-2):
    """fp32 HIP path against a G7 case: forward scalars rtol 1e-4, reconstruction samples 2e-4 of max|ref|, and the
    whole-model gradient gates of round 2/3 (derived from gpurun_out/grad_err_*.log: median relative L2 3e-5, worst regular
    tensor 8e-3, worst analytically-zero bias 1.7e-2):
      * every tensor finite;
      * 90 % of the (sampled) elements within 2e-3 of the layer scale;
      * relative L2 error with the 1 % largest element errors set aside <= 4e-3, of the whole tensor (count sketch) <= 5e-2
        -- two fp32 implementations that sum in different orders disagree on a handful of BN->ReLU masks, each of which
        moves one row / channel of a weight gradient (tests/tools/debug_trace.py);
      * analytically-zero biases: relative L2 (noise-floor denominator) <= 5e-2;
      * each bound is relaxed to 3x the reference's own fp32-vs-fp64 deviation where the fixture holds an fp64 truth."""
    g = load(f"g7_{case}")
    cfg, sd, batch, eps, masks = g7_inputs(g)
    mode = str(g["mode"])
    exp = build_exp(cfg, sd, "cuda", mode, masks=masks, eps=eps)
    got = RE.basic_routine_epoch(exp, ({k: v.cuda() for k, v in batch.items()}, None))
    for k, v in _scalars(got).items():
        ref = float(g[f"fp32/{k}"])
        assert abs(v - ref) <= 1e-4 * abs(ref) + (1e-6 if k.startswith("klds") else 0.0), (case, k, v, ref)
    for m in ("PA", "Lateral"):
        err = (_rec_samples(got, m) - torch.from_numpy(g[f"fp32/rec/{m}"]).double()).abs().max().item()
        assert err <= 2e-4 * float(g[f"fp32/recmax/{m}"]) + 1e-5, (case, m, err)
    exp.mm_vae.zero_grad()
    got["total_loss"].backward()
    grads = exp.mm_vae.reference_named_grads()
    names, numel, meta = [str(n) for n in g["grad_names"]], g["grad_numel"], g["grad_meta"]
    assert set(grads) == set(names)
    log = f"gpurun_out/grad_err_{case}.log"
    if os.path.exists(log):
        os.remove(log)
    failures = []
    for name, n, (scale, e_cpu, cpu_l2) in zip(names, numel, meta):
        gr = grads[name]
        pg = PackedGrad(g, f"g/{name}", int(n))
        l2, elem, _ = pg.diff(gr)
        err = elem / scale
        floor = 1e-2 * scale * int(n) ** 0.5
        denom = max(pg.norm, floor)
        k = max(2, err.numel() // 100)
        keep = elem.topk(err.numel() - k, largest=False).values if err.numel() > k else elem[:0]
        m = dict(max=err.max().item(), q90=torch.quantile(err, 0.9).item(), rel_l2=l2 / denom,
                 rel_l2_trim=keep.norm().item() * pg.sample_scale() / denom)
        finite = bool(torch.isfinite(gr).all())
        _log(log, f"{name}: max={m['max']:.3e} q90={m['q90']:.3e} relL2={m['rel_l2']:.3e} trimL2={m['rel_l2_trim']:.3e} "
                  f"cpu32max={e_cpu:.3e} cpu32L2={cpu_l2:.3e} scale={scale:.3e} finite={finite}")
        if near_zero_grad(name):
            ok = finite and m["rel_l2"] <= max(zero_tol, 3 * cpu_l2)
        else:
            ok = (finite and m["q90"] <= max(q90_tol, 3 * e_cpu) and m["rel_l2_trim"] <= max(trim_tol, 3 * cpu_l2)
                  and m["rel_l2"] <= max(l2_tol, 3 * cpu_l2))
        if not ok:
            failures.append((name, m))
    assert not failures, failures[:10]
    return exp, cfg


def check_bf16_case(case, small_batch=False, grads=True):
    """bf16 HIP path against a G7 case: forward scalars against the bf16-mode oracle (3e-3) and the REFERENCE's fp32 run
    (rtol 2e-2); reconstruction samples; every parameter gradient against the bf16-mode oracle's and the
    reference's fp32 gradient.  Gates (derived from gpurun_out/bf16_parity.log, round 3: C3 at B = 256, tensors above the
    bf16 noise floor: median rel-L2 2.5e-2, p90 7.2e-2, max 1.2e-1 -- the decoders' bn1 / conv1, the deepest points of the
    backward chain).  Two bf16 implementations that round at the same points but sum in different orders differ by about the
    noise bf16 itself adds, so the second yardstick is the FP32 gradient: the HIP gradient must be as close to it as the
    bf16-mode oracle's is.
      regular tensor:   rel-L2 vs the bf16-mode oracle <= 0.15, cosine >= 0.985;
                        rel-L2 vs the fp32 reference <= 1.5 x the bf16-mode oracle's own + 2e-2;
                        over all regular tensors: median <= 4e-2, 90th percentile <= 0.11, median cosine >= 0.998
      analytically zero gradients (both sides hold pure rounding noise): |error| <= half the bf16 noise floor of the tensor
    A gradient that is wrong by 20 % in one tensor fails the first line.  (Norms of differences are count-sketch estimates,
    8.8 % relative standard deviation: tests/golden_util.py.)  small_batch (B <= 16: fewer rows per gradient, measured in round 3:
    median 3.0e-2, p90 9.1e-2, max 1.5e-1): 0.22 / 0.975 / 6e-2 / 0.15.  grads=False: an eval-mode case, forward only."""
    g = load(f"g7_{case}")
    cfg, sd, batch, eps, masks = g7_inputs(g)
    exp = build_exp(cfg, sd, "cuda", str(g["mode"]), masks=masks, eps=eps, compute_dtype="bf16")
    got = RE.basic_routine_epoch(exp, ({k: v.cuda() for k, v in batch.items()}, None))
    log = "gpurun_out/bf16_parity.log"
    for k, v in _scalars(got).items():
        r16, r32 = float(g[f"bf16/{k}"]), float(g[f"fp32/{k}"])
        _log(log, f"{case} {k}: hip={v:.6g} oracle_bf16={r16:.6g} reference_fp32={r32:.6g} rel16={_rel(v, r16):.2e} rel32={_rel(v, r32):.2e}")
        assert _rel(v, r32) <= 2e-2 + 1e-3 / max(abs(r32), 1e-3), (case, k, v, r32)
        assert _rel(v, r16) <= 3e-3 + 1e-3 / max(abs(r16), 1e-3), (case, k, v, r16)
    for m in ("PA", "Lateral"):
        err = (_rec_samples(got, m) - torch.from_numpy(g[f"bf16/rec/{m}"]).double()).abs()
        assert err.mean().item() <= 2e-3 * float(g[f"bf16/recmax/{m}"]), (case, m, err.mean().item())
    if not grads:
        return exp, cfg, g
    exp.mm_vae.zero_grad()
    got["total_loss"].backward()
    grads = exp.mm_vae.reference_named_grads()
    names, numel, meta = [str(n) for n in g["grad_names"]], g["grad_numel"], g["grad_meta"]
    assert set(grads) == set(names)
    g32 = load(f"g7_{case}_g32") if os.path.exists(os.path.join(GOLDEN, f"g7_{case}_g32.npz")) else g    # (oracle/gen_g7.py: SPLIT_G32)
    cap, cos_min, med_max, p90_max = (0.22, 0.975, 6e-2, 0.15) if small_batch else (0.15, 0.985, 4e-2, 0.11)
    bad, cos_all, rel_reg = [], [], []
    for name, n, (scale, e_ref32) in zip(names, numel, meta):
        gr = grads[name]
        assert torch.isfinite(gr).all(), name
        b, c = PackedGrad(g, f"g16/{name}", int(n)), PackedGrad(g32, f"g32/{name}", int(n))
        floor = 2e-2 * scale * int(n) ** 0.5          # bf16 noise floor for (near-)zero gradients
        below = b.norm <= floor
        d16, _, na = b.diff(gr)
        d32, _, _ = c.diff(gr)
        rel_l2 = d16 / max(b.norm, floor)
        cos = 1.0 if below else (na * na + b.norm * b.norm - d16 * d16) / max(2 * na * b.norm, 1e-30)
        e_hip32 = d32 / max(c.norm, floor)
        _log(log, f"{case} grad {name}: relL2={rel_l2:.3e} cos={cos:.5f} scale={scale:.3e} vs_fp32: hip={e_hip32:.3e} "
                  f"oracle_bf16={e_ref32:.3e}" + (" (below the noise floor)" if below else ""))
        if below:
            ok = rel_l2 <= 0.5
        else:
            cos_all.append(cos)
            rel_reg.append(rel_l2)
            # (the fp32 yardstick needs a gradient well above the noise floor: within 3 x the floor both bf16 results are
            # mostly rounding noise and their distances to the fp32 gradient are two independent draws of it)
            ok = rel_l2 <= cap and cos >= cos_min and (b.norm <= 3 * floor or e_hip32 <= 1.5 * e_ref32 + 2e-2)
        if not ok:
            bad.append((name, round(rel_l2, 4), round(cos, 5), round(e_hip32, 4), round(float(e_ref32), 4), below))
    q = np.quantile(rel_reg, [0.5, 0.9])
    _log(log, f"{case} grads: {len(rel_reg)} regular tensors: rel-L2 median={q[0]:.3e} p90={q[1]:.3e} max={max(rel_reg):.3e}; "
              f"median cos={np.median(cos_all):.6f} min cos={min(cos_all):.5f}")
    assert not bad, bad[:10]
    assert q[0] <= med_max and q[1] <= p90_max, q
    assert np.median(cos_all) >= 0.998, np.median(cos_all)
    return exp, cfg, g
