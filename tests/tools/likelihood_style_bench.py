"""Time per test batch of the importance-sampled likelihood estimator with and without style latents (measurement aid,
not a test): config #2 shapes (128 px, class_dim 128, DIM_img 64), eval mode, the launcher's --calc_nll batch of
B = 30 rows, K = 6 samples per row, all 7 subsets per batch.  'style' is factorized_representation with style dims 32/32/32
(mopoe_lhood_style_sample + mopoe_lhood_estimates per subset), 'none' the non-factorized estimator.
Prints one JSON line; --out also writes it to a file.
--only style / none measures one of the two (a kernel trace of the factorized estimator alone).
Usage:  python tests/tools/likelihood_style_bench.py [--batches 6] [--only style|none] [--out results.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "mopoe-mimic_amd"))
import torch  # noqa: E402
from mimic_amd.evaluation.eval_metrics.likelihood import estimate_likelihoods  # noqa: E402
from mimic_amd.utils.experiment import HotPathExperiment, default_flags  # noqa: E402

B, K, S = 30, 6, 32


def measure(style, n_batches, dev):
    torch.manual_seed(0)
    kw = dict(factorized_representation=True, style_pa_dim=S, style_lat_dim=S, style_text_dim=S) if style else {}
    flags = default_flags(img_size=128, class_dim=128, DIM_img=64, batch_size=B, device=dev, **kw)
    exp = HotPathExperiment(flags)
    exp.mm_vae.to(dev).eval()
    mk = lambda: ({"PA": torch.rand(B, 1, 128, 128, device=dev), "Lateral": torch.rand(B, 1, 128, 128, device=dev),
                   "text": torch.randint(0, 3517, (B, 128), device=dev).float()}, None)
    loader = [mk() for _ in range(n_batches)]
    estimate_likelihoods(exp, loader[:2], num_imp_samples=K)      # warm-up: launch plans are tuned here
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = estimate_likelihoods(exp, loader, num_imp_samples=K)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"ms_per_batch": dt / n_batches * 1e3, "joint_all_given": out["Lateral_PA_text"]["joint"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--only", choices=("style", "none"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    res = {"shapes": f"128 px, class_dim 128, DIM_img 64, B {B}, K {K}, 7 subsets per batch", "batches": args.batches}
    if args.only != "style":
        res["none"] = measure(False, args.batches, dev)
    if args.only != "none":
        res[f"style_{S}"] = measure(True, args.batches, dev)
    if args.only is None:
        res["style_over_none"] = res[f"style_{S}"]["ms_per_batch"] / res["none"]["ms_per_batch"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
