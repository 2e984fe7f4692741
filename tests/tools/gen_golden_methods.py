"""Generate tests/golden/g8_{moe,jsd}_*.npz: the reference's own outputs for method='moe' (MMVAE) and method='jsd'
(mixture of experts with a dynamic prior).

oracle/gen_golden.py is imported as a module and left as it is.  Its `make_flags` is wrapped so that `method` and the
four method booleans are set through the reference's own `get_method` (the three it does not select are cleared first,
since the wrapped call has already selected joint_elbo); every generator below then builds the reference model through
that wrapper.  Only inputs, seeds and numeric outputs are written.

Fixtures, per method m in {moe, jsd}:
  g8_m_g0_s64       tiny full model (as g0_s64): every output and every parameter gradient, eval / train_nodrop / train
  g8_m_c1           config #1 stand-in (64 px, D=64, B=8, DIM_img=64): scalars, checksums, per-network gradient norms
  g8_m_c2           config #2 shape (128 px, D=128, B=64, DIM_img=64): as c1
  g8_m_partial      partial-modality inference of the tiny model (as g2_edges)
  g8_m_traj         three Adam steps (as g3_traj)
  g8_m_likelihood   importance-sampled likelihood estimates (as g4_likelihood)
g8_m_g0_s64 and g8_m_c2 are written in the compact form of tests/methods_util.py (weights regenerated from their seed,
seeded images as a patch, sampled reconstructions, sketched gradients): the reference's numbers, in a few hundred KiB.
Usage:  python tests/tools/gen_golden_methods.py [--only moe_c2 jsd_g0_s64 ...]
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "oracle"), os.path.join(REPO, "mopoe-mimic_amd")]


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(REPO, "oracle", "gen_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    return G


def select_method(G, method):
    """route G.make_flags through the reference's get_method for `method`"""
    base = getattr(G, "_make_flags_joint_elbo", G.make_flags)
    G._make_flags_joint_elbo = base

    def make_flags(cfg):
        from mimic.utils.filehandling import get_method
        f = base(cfg)
        f.method = method
        f.modality_poe = f.modality_moe = f.modality_jsd = f.joint_elbo = False
        return get_method(f)

    G.make_flags = make_flags


def checksums(t: torch.Tensor):
    """gen_golden.checksums with its 16 sample positions clamped to the tensor: the fp32 linspace behind them rounds its
    last position past the end once a tensor has more than 2^24 elements (config #2's text logits).  Identical to the
    original below that size."""
    t = t.detach().double().flatten()
    idx = torch.linspace(0, t.numel() - 1, 16).long().clamp(max=t.numel() - 1)
    return np.concatenate([[t.sum().item(), (t * t).sum().item()], t[idx].numpy()])


def compact_g0(store, size=64):
    """the G0 store of gen_golden.gen_g0 in the compact form (tests/methods_util.py)"""
    import mopoe_ref as R
    import methods_util as MU
    from golden_util import cfg_from, weights_fingerprint
    cfg = cfg_from(store["cfg"])
    sd = {k[3:]: torch.from_numpy(v) for k, v in store.items() if k.startswith("sd/")}
    for attempt in range(30):   # (gen_g0's seed schedule: the first well-conditioned attempt was kept)
        seed = 100 + size + 1000 * attempt
        regen = R.init_state(cfg, seed=seed)
        regen[MU.G0_PAD_ROW[0]][0] = MU.G0_PAD_ROW[1]
        if all(torch.equal(regen[k], v) for k, v in sd.items()):
            break
    else:
        raise RuntimeError("G0 weights do not come from gen_g0's seeds")
    out = {"seed_weights": np.array(seed), "pad_row": np.array(MU.G0_PAD_ROW[1]),
           "sd_fingerprint": weights_fingerprint(regen)}
    names = sorted(k[len("eval/grad/"):] for k in store if k.startswith("eval/grad/"))
    out["grad_names"] = np.array(names)
    out["grad_numel"] = np.array([store["eval/grad/" + n].size for n in names])
    for k, v in store.items():
        if k.startswith("sd/") or "/grad/" in k or "/buf/" in k or "/rec/" in k:
            continue
        out[k] = v
    for mode in ("eval", "train_nodrop", "train"):
        assert sorted(k[len(mode) + 6:] for k in store if k.startswith(mode + "/grad/")) == names, mode
        MU.pack_grads(out, mode, {n: torch.from_numpy(store[f"{mode}/grad/{n}"]) for n in names}, names)
        out[f"{mode}/recchk/text"] = checksums(torch.from_numpy(store[f"{mode}/rec/text"]))
        for m in ("PA", "Lateral", "text"):
            t = torch.from_numpy(store[f"{mode}/rec/{m}"]).flatten()
            out[f"{mode}/rec/{m}/sample"] = t[MU.rec_sample_index(t.numel())].numpy()
    return out


def compact_c2(store):
    """the config #2 store of gen_golden.gen_g1 with its images as a patch on the seeded synthetic batch"""
    import mopoe_ref as R
    import methods_util as MU
    from golden_util import cfg_from
    cfg = cfg_from(store["cfg"])
    batch, _ = R.synthetic_batch(cfg, int(store["cfg"][5]), seed=int(store["seed_batch"]))
    out = {k: v for k, v in store.items() if k not in ("in/PA_u8", "in/Lateral_u8")}
    for m in ("PA", "Lateral"):
        u8 = store[f"in/{m}_u8"]
        base = (batch[m] * 255.0).round().to(torch.uint8).numpy()
        idx = np.flatnonzero(base.reshape(-1) != u8.reshape(-1)).astype(np.int32)
        out[f"in/{m}_patch_idx"], out[f"in/{m}_patch_val"] = idx, u8.reshape(-1)[idx]
        out[f"in/{m}_crc"] = np.array(MU.u8_crc(u8), dtype=np.int64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    G = load_generator()
    G.checksums = checksums
    if not os.path.isdir(G.REF):
        print("reference not present; nothing to do")
        return
    torch.set_num_threads(8)
    run_epochs = G.import_reference()
    outdir = os.path.join(REPO, "tests", "golden")
    for method in ("moe", "jsd"):
        jobs = {
            "g0_s64": lambda: G.gen_g0(run_epochs, 64, 4),
            "c1": lambda: G.gen_g1(run_epochs, 64, 64, 8, 64),
            "c2": lambda: G.gen_g1(run_epochs, 128, 128, 64, 64),
            "partial": lambda: G.gen_g2(run_epochs),
            "traj": lambda: G.gen_g3(run_epochs),
            "likelihood": lambda: G.gen_g4(run_epochs),
        }
        for name, job in jobs.items():
            if args.only and f"{method}_{name}" not in args.only:
                continue
            select_method(G, method)
            store = job()
            store = {"g0_s64": compact_g0, "c2": compact_c2}.get(name, dict)(store)
            store["method"] = np.array(method)
            path = os.path.join(outdir, f"g8_{method}_{name}.npz")
            np.savez_compressed(path, **store)
            print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(store)} arrays", flush=True)


if __name__ == "__main__":
    main()
