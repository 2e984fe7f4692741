"""Training-step rate with --ema_decay off and on, at bench.py configurations, alternated in one process: each arm gets its
own model, HipAdam and captured step (run_epochs.GraphedTrainStep, as bench.py runs it), then the arms take turns, `--rounds`
times, each turn `--steps` timed replays after a synchronisation.  Arms:

    off   bench.py's step: no average, every network's Adam update right behind its backward (MOPOE_EARLY_ADAM)
    on    ema_decay = --decay: the same step with one EMA update launch behind every Adam launch, on that launch's stream

so on - off is the cost of the average: 12 bytes per live parameter (p read, ema read and written) and the extra launches.

    python tests/tools/ema_rate.py [--configs c2 c3] [--rounds 5] [--steps 50] [--decay 0.999] [--out FILE]
         [--bench-parent DIR --bench-runs 3]
Prints one JSON line: per config and arm, the samples/s of every round and their median, and the cost.
--bench-parent DIR (a checkout of the parent commit with its library built): `python bench.py --config c2` of this tree and of
DIR alternated, --bench-runs each, in child processes; both series go into the line under "bench_c2_off" with the verdict
`median_within_parent_spread`.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "mopoe-mimic_amd"), os.path.dirname(os.path.abspath(__file__))]

ARMS = ("off", "on")


def setup(arm, config, device, decay):
    import torch
    import bench
    from mimic_amd import run_epochs as RE
    from mimic_amd.utils.experiment import HotPathExperiment, default_flags
    size, cdim, dimg, bsz, cdtype = bench.CONFIGS[config]
    torch.manual_seed(0)
    flags = default_flags(img_size=size, class_dim=cdim, DIM_img=dimg, batch_size=bsz, device=device,
                          initial_learning_rate=1e-5, compute_dtype=cdtype, ema_decay=decay if arm == "on" else 0.0)
    exp = HotPathExperiment(flags)
    exp.mm_vae.to(device)
    exp.mm_vae.train()
    exp.set_optimizer()
    batches = bench.synthetic_batches(flags, 4, device, seed=1)
    pack = RE.ScalarPack(device)
    step = RE.GraphedTrainStep(exp, batches[0], pack, None)
    n_live = sum(p.numel() for p in exp.mm_vae.parameters() if p.grad is not None)
    return {"exp": exp, "step": step, "batches": batches, "pack": pack, "bsz": bsz, "i": 0, "live_elements": n_live}


def run(s, n):
    for _ in range(n):
        s["step"](s["batches"][s["i"] % len(s["batches"])])
        s["i"] += 1


def main():
    from grad_clip_rate import bench_off       # (the same alternated bench.py series, parent against this tree)
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["c2", "c3"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"ema_decay": args.decay, "steps_per_round": args.steps, "rounds": args.rounds, "configs": {}}
    if args.bench_parent:      # (before this process opens the GPU: the children then have the device to themselves)
        out["bench_c2_off"] = bench_off(os.path.abspath(args.bench_parent), args.bench_runs)
    if args.configs:
        import torch
        device = torch.device("cuda", 0)
        torch.cuda.set_device(device)
    for config in args.configs:
        runs = {a: setup(a, config, device, args.decay) for a in ARMS}
        for s in runs.values():
            run(s, args.warmup)
        torch.cuda.synchronize()
        rates = {a: [] for a in ARMS}
        for r in range(args.rounds):
            for a in (ARMS if r % 2 == 0 else ARMS[::-1]):
                s = runs[a]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(s, args.steps)
                torch.cuda.synchronize()
                rates[a].append(s["bsz"] * args.steps / (time.perf_counter() - t0))
        med = {a: statistics.median(v) for a, v in rates.items()}
        ms = {a: 1e3 * runs[a]["bsz"] / med[a] for a in ARMS}
        opt = runs["on"]["exp"].optimizer
        lag = max(float((e - p.detach()).abs().max()) for e, p in zip(opt.ema_tensors(), opt._params))
        out["configs"][config] = {
            "samples_per_sec": {a: {"median": round(med[a], 1), "rounds": [round(x, 1) for x in v]} for a, v in rates.items()},
            "step_ms": {a: round(ms[a], 4) for a in ARMS},
            "ema_cost_pct": round(100.0 * (med["off"] / med["on"] - 1.0), 2),
            "ema_cost_ms": round(ms["on"] - ms["off"], 4),
            "ema_megabytes_moved": round(12e-6 * runs["on"]["live_elements"], 1),
            "optimiser_steps": float(opt._step), "max_abs_ema_minus_p": lag,
            "last_total_loss": {a: s["pack"].read().get("total_loss") for a, s in runs.items()}}
        del runs, opt
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
