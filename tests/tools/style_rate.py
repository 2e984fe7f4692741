"""Training-step rate with the style latents of the factorized representation off and on, at bench.py configurations,
alternated in one process: each arm gets its own model, HipAdam and captured step (run_epochs.GraphedTrainStep, as
bench.py runs it), then the arms take turns, `--rounds` times, each turn `--steps` timed replays after a synchronisation.
The 'style' arm sets factorized_representation with every style dim `--style-dim`; the 'plain' arm is bench.py's model.

    python tests/tools/style_rate.py [--configs c2 c3] [--rounds 5] [--steps 50] [--style-dim 32] [--out FILE]
Prints one JSON line: per config and arm, the samples/s of every round and their median, and the style arm's cost.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "mopoe-mimic_amd")]

import torch  # noqa: E402

import bench  # noqa: E402  (CONFIGS, synthetic_batches: the benchmark's own workload)
from mimic_amd import run_epochs as RE  # noqa: E402
from mimic_amd.utils.experiment import HotPathExperiment, default_flags  # noqa: E402


def setup(arm, config, device, style_dim):
    size, cdim, dimg, bsz, cdtype = bench.CONFIGS[config]
    torch.manual_seed(0)
    s = style_dim if arm == "style" else 0
    flags = default_flags(img_size=size, class_dim=cdim, DIM_img=dimg, batch_size=bsz, device=device,
                          initial_learning_rate=1e-5, compute_dtype=cdtype, factorized_representation=(arm == "style"),
                          style_pa_dim=s, style_lat_dim=s, style_text_dim=s)
    exp = HotPathExperiment(flags)
    exp.mm_vae.to(device)
    exp.mm_vae.train()
    exp.set_optimizer()
    batches = bench.synthetic_batches(flags, 4, device, seed=1)
    pack = RE.ScalarPack(device)
    step = RE.GraphedTrainStep(exp, batches[0], pack, None)
    return {"exp": exp, "step": step, "batches": batches, "pack": pack, "bsz": bsz, "i": 0}


def run(s, n):
    for _ in range(n):
        s["step"](s["batches"][s["i"] % len(s["batches"])])
        s["i"] += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"], choices=sorted(bench.CONFIGS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--style-dim", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    arms = ("plain", "style")
    out = {"style_dim": args.style_dim, "steps_per_round": args.steps, "rounds": args.rounds, "configs": {}}
    for config in args.configs:
        runs = {a: setup(a, config, device, args.style_dim) for a in arms}
        for s in runs.values():
            run(s, args.warmup)
        torch.cuda.synchronize()
        rates = {a: [] for a in arms}
        for r in range(args.rounds):
            for a in (arms if r % 2 == 0 else arms[::-1]):
                s = runs[a]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(s, args.steps)
                torch.cuda.synchronize()
                rates[a].append(s["bsz"] * args.steps / (time.perf_counter() - t0))
        med = {a: statistics.median(v) for a, v in rates.items()}
        out["configs"][config] = {
            "samples_per_sec": {a: {"median": round(med[a], 1), "rounds": [round(x, 1) for x in v]} for a, v in rates.items()},
            "style_cost_pct": round(100.0 * (med["plain"] / med["style"] - 1.0), 2),
            "last_total_loss": {a: s["pack"].read().get("total_loss") for a, s in runs.items()}}
        del runs
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
