"""Training-step rate of method='joint_elbo', 'moe' and 'jsd' at a bench.py configuration, the three alternated in one
process: each method gets its own model, HipAdam and captured step (run_epochs.GraphedTrainStep, as bench.py runs it),
then the methods take turns, `--rounds` times, each turn `--steps` timed replays after a synchronisation.  Everything
outside the latent stage is the same work in the three methods, so their step times should agree within noise.

    python tests/tools/method_rate.py [--config c2] [--rounds 5] [--steps 50] [--methods joint_elbo moe jsd] [--out FILE]
Prints one JSON line: per method, the samples/s of every round and their median.
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
from mimic_amd.utils.filehandling import get_method  # noqa: E402


def setup(method, config, device):
    size, cdim, dimg, bsz, cdtype = bench.CONFIGS[config]
    torch.manual_seed(0)
    flags = default_flags(img_size=size, class_dim=cdim, DIM_img=dimg, batch_size=bsz, device=device,
                          initial_learning_rate=1e-5, compute_dtype=cdtype, method=method)
    get_method(flags)
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
    ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--methods", nargs="+", default=["joint_elbo", "moe", "jsd"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    runs = {m: setup(m, args.config, device) for m in args.methods}
    for s in runs.values():
        run(s, args.warmup)
    torch.cuda.synchronize()
    rates = {m: [] for m in args.methods}
    for r in range(args.rounds):
        order = args.methods if r % 2 == 0 else args.methods[::-1]
        for m in order:
            s = runs[m]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(s, args.steps)
            torch.cuda.synchronize()
            rates[m].append(s["bsz"] * args.steps / (time.perf_counter() - t0))
    losses = {m: s["pack"].read().get("total_loss") for m, s in runs.items()}
    out = {"config": args.config, "steps_per_round": args.steps, "rounds": args.rounds,
           "samples_per_sec": {m: {"median": round(statistics.median(v), 1), "rounds": [round(x, 1) for x in v]}
                               for m, v in rates.items()},
           "last_total_loss": losses}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
