"""Training-step rate with --max_grad_norm off and on, at bench.py configurations, alternated in one process: each arm gets
its own model, HipAdam and captured step (run_epochs.GraphedTrainStep, as bench.py runs it), then the arms take turns,
`--rounds` times, each turn `--steps` timed replays after a synchronisation.  Arms:

    off           bench.py's step: no clipping, every network's Adam update right behind its backward (MOPOE_EARLY_ADAM)
    off_one_adam  no clipping, ONE Adam update behind the last backward (what MOPOE_EARLY_ADAM=0 runs)
    on            max_grad_norm = --max-norm: the norm kernels, then one clipped Adam update behind the last backward

so on - off_one_adam is the cost of the norm pass (one more read of all gradients) and off_one_adam - off the cost of giving
up the early updates, which clipping implies.

    python tests/tools/grad_clip_rate.py [--configs c2 c3] [--rounds 5] [--steps 50] [--max-norm 1.0] [--out FILE]
         [--bench-parent DIR --bench-runs 3]
Prints one JSON line: per config and arm, the samples/s of every round and their median, and the two costs.
--bench-parent DIR (a checkout of the parent commit with its library built): `python bench.py --config c2` of this tree and of
DIR alternated, --bench-runs each, in child processes; both series go into the line under "bench_c2_off" with the verdict
`median_within_parent_spread`.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "mopoe-mimic_amd")]

ARMS = ("off", "off_one_adam", "on")


def setup(arm, config, device, max_norm):
    import torch
    import bench
    from mimic_amd import run_epochs as RE
    from mimic_amd.utils.experiment import HotPathExperiment, default_flags
    size, cdim, dimg, bsz, cdtype = bench.CONFIGS[config]
    torch.manual_seed(0)
    flags = default_flags(img_size=size, class_dim=cdim, DIM_img=dimg, batch_size=bsz, device=device,
                          initial_learning_rate=1e-5, compute_dtype=cdtype, max_grad_norm=max_norm if arm == "on" else 0.0)
    exp = HotPathExperiment(flags)
    exp.mm_vae.to(device)
    exp.mm_vae.train()
    exp.set_optimizer()
    batches = bench.synthetic_batches(flags, 4, device, seed=1)
    pack = RE.ScalarPack(device)
    early = RE.EARLY_ADAM
    RE.EARLY_ADAM = early and arm != "off_one_adam"       # (read by train_step while the step is captured)
    try:
        step = RE.GraphedTrainStep(exp, batches[0], pack, None)
    finally:
        RE.EARLY_ADAM = early
    n_grad = sum(p.numel() for p in exp.mm_vae.parameters() if p.grad is not None)
    return {"exp": exp, "step": step, "batches": batches, "pack": pack, "bsz": bsz, "i": 0, "grad_elements": n_grad}


def run(s, n):
    for _ in range(n):
        s["step"](s["batches"][s["i"] % len(s["batches"])])
        s["i"] += 1


def bench_value(tree, config):
    """one `python bench.py --config <config>` of the tree in a fresh process -> the value of its JSON line"""
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--config", config], cwd=tree, capture_output=True,
                         text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f"bench.py of {tree} failed ({out.returncode}):\n{out.stderr[-3000:]}")
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    return float(line["value"])


def bench_off(parent, runs, config="c2"):
    series = {"this": [], "parent": []}
    for r in range(runs):
        for who in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            series[who].append(round(bench_value(REPO if who == "this" else parent, config), 1))
            print(f"[grad_clip_rate] bench {config} {who}: {series[who][-1]}", file=sys.stderr, flush=True)
    med = statistics.median(series["this"])
    return {"config": config, "unit": "samples/s", "this": series["this"], "parent": series["parent"],
            "this_median": med, "parent_min": min(series["parent"]), "parent_max": max(series["parent"]),
            "median_within_parent_spread": min(series["parent"]) <= med <= max(series["parent"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["c2", "c3"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"max_grad_norm": args.max_norm, "steps_per_round": args.steps, "rounds": args.rounds, "configs": {}}
    if args.bench_parent:      # (before this process opens the GPU: the children then have the device to themselves)
        out["bench_c2_off"] = bench_off(os.path.abspath(args.bench_parent), args.bench_runs)
    if args.configs:
        import torch
        device = torch.device("cuda", 0)
        torch.cuda.set_device(device)
    for config in args.configs:
        runs = {a: setup(a, config, device, args.max_norm) for a in ARMS}
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
        last = runs["on"]["pack"].read()
        out["configs"][config] = {
            "samples_per_sec": {a: {"median": round(med[a], 1), "rounds": [round(x, 1) for x in v]} for a, v in rates.items()},
            "step_ms": {a: round(ms[a], 4) for a in ARMS},
            "clip_cost_pct": round(100.0 * (med["off"] / med["on"] - 1.0), 2),
            "norm_pass_cost_pct": round(100.0 * (med["off_one_adam"] / med["on"] - 1.0), 2),
            "early_adam_loss_pct": round(100.0 * (med["off"] / med["off_one_adam"] - 1.0), 2),
            "norm_pass_ms": round(ms["on"] - ms["off_one_adam"], 4),
            "gradient_megabytes": round(4e-6 * runs["on"]["grad_elements"], 1),
            "last_grad_norm": last.get("grad_norm"), "skipped_steps": last.get("skipped_steps"),
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
