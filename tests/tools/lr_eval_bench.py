"""Times and accuracy of the latent-representation evaluation (--eval_lr) on one MI355X (measurement aid, not a test):

  * ops.logreg_fit for the 21 problems (7 subsets x 3 labels) at N 500, D 128 and D 256 (the problems of
    tests/golden/g11_lr_c2 and g11_lr_small case 2), ops.logreg_predict for one batch of M 30: medians of repeated launches,
    HIP events around each launch, after a warm-up;
  * the accuracy of the fit per fixture: |grad f(W)|_inf / N in float64, |W - w*| / ref_dist, |W - w*| / |w*| (the figures
    tests/test_lr_eval_gpu.py asserts on and DESIGN section 7 quotes);
  * one whole evaluation at config #2 shapes (128 px, class_dim 128, DIM_img 64) on the synthetic split, wall time split
    into encoding + sampling (train side), fitting, and scoring (test side);
  * where scikit-learn is importable: 21 LogisticRegression(random_state=0, solver='lbfgs', max_iter=1000).fit calls on the
    same data on the host; where it is not, the figures of the build machine, labelled as such.
Prints one JSON line; --out also writes it (profiles/lr_eval_bench.json).
--fit_only: launch the D 128 fit a few times and nothing else (for `rocprofv3 --kernel-trace --stats -- python ... --fit_only`).
Usage:  python tests/tools/lr_eval_bench.py [--out profiles/lr_eval_bench.json] [--reps 20] [--fit_only]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(REPO, "mopoe-mimic_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lr_util as LU  # noqa: E402
from mimic_amd import ops  # noqa: E402

BUILD_MACHINE_SKLEARN_MS_PER_FIT = [23, 224]   # one LogisticRegression.fit at N 500, D 128 on the build machine's CPU


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def kernel_times(reps):
    out = {}
    for tag, name, idx in (("fit_21_problems_N500_D128", "c2", 0), ("fit_21_problems_N500_D256", "small", 2)):
        case = LU.make_case(LU.CASES[name][idx])
        x, y = torch.from_numpy(case["x_train"]).cuda(), torch.from_numpy(case["y_train"]).cuda()
        out[tag] = timed(lambda: ops.logreg_fit(x, y), reps)
        out[tag]["newton_steps"] = [int(v) for v in ops.logreg_fit(x, y)[1][..., 0].flatten().tolist()]
        if name == "c2":
            w = ops.logreg_fit(x, y)[0]
            xt = [t.contiguous() for t in torch.from_numpy(case["x_test"][:, :30]).cuda().unbind(0)]
            out["predict_7_subsets_M30_D128"] = timed(lambda: ops.logreg_predict(xt, w), reps)
            out["sklearn_host_21_fits_N500_D128"] = sklearn_times(case)
    return out


def sklearn_times(case):
    try:
        from sklearn.linear_model import LogisticRegression
    except ImportError:
        return {"source": "not measured here (scikit-learn not importable); build machine's CPU, ms per single fit",
                "ms_per_fit_range": BUILD_MACHINE_SKLEARN_MS_PER_FIT}
    torch.set_num_threads(16)
    per_fit = []
    for rep in range(2):                               # the second pass is the one reported
        per_fit = []
        for s in range(case["x_train"].shape[0]):
            for l in range(case["y_train"].shape[1]):
                t0 = time.perf_counter()
                LogisticRegression(random_state=0, solver="lbfgs", max_iter=1000).fit(case["x_train"][s], case["y_train"][:, l])
                per_fit.append((time.perf_counter() - t0) * 1e3)
    return {"source": "measured on this host", "total_ms": sum(per_fit), "ms_per_fit_range": [min(per_fit), max(per_fit)]}


def accuracy():
    from golden_util import load  # noqa: F401  (lr_util.load_cases reads the fixtures through it)
    out = {}
    for name in ("c2", "small", "hard"):
        for tag, spec, case, fx in LU.load_cases(name):
            x, y = torch.from_numpy(case["x_train"]).cuda(), torch.from_numpy(case["y_train"]).cuda()
            w, info = ops.logreg_fit(x, y)
            wn = w.cpu().numpy().astype(np.float64)
            dist = np.linalg.norm(wn - fx["w_star"], axis=2)
            out[tag] = {"N": spec["N"], "D": spec["D"], "problems": int(dist.size),
                        "grad_inf_over_N_max": float(LU.grad_inf(wn, case["x_train"], case["y_train"]).max() / spec["N"]),
                        "dist_over_ref_dist_max": float((dist / fx["ref_dist"]).max()),
                        "dist_over_norm_wstar_max": float((dist / np.linalg.norm(fx["w_star"], axis=2)).max()),
                        "newton_steps_max": int(info[..., 0].max().item())}
    return out


def whole_evaluation():
    from mimic_amd import run_epochs as RE
    from mimic_amd.evaluation.eval_metrics import representation as REP
    from mimic_amd.utils.experiment import HotPathExperiment, default_flags
    dev = torch.device("cuda")
    flags = default_flags(img_size=128, class_dim=128, DIM_img=64, batch_size=REP.LR_BATCH_SIZE, device=dev,
                          testing_batches=20, num_training_samples_lr=500)
    exp = HotPathExperiment(flags)
    exp.mm_vae.to(dev).eval()
    spans = {}

    def stamp(name, fn):
        def wrapped(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            spans[name] = spans.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return out
        return wrapped

    real_fit = ops.logreg_fit
    res = {}
    for rep in ("warm_up", "timed"):
        spans.clear()
        RE.set_random_seed(0)
        ops.logreg_fit = stamp("fit_ms", real_fit)
        try:
            t0 = time.perf_counter()
            clf = stamp("train_side_ms", REP.train_clf_lr_all_subsets)(exp)
            stamp("test_side_ms", REP.test_clf_lr_all_subsets)(clf, exp)
            total = (time.perf_counter() - t0) * 1e3
        finally:
            ops.logreg_fit = real_fit
        res = {"shapes": "128 px, class_dim 128, DIM_img 64, synthetic split of 20 batches of 30 rows on each side, "
                         "500 sampled training rows, 7 subsets x 3 labels",
               "total_ms": total, "fit_ms": spans["fit_ms"],
               "train_side_encoding_and_sampling_ms": spans["train_side_ms"] - spans["fit_ms"],
               "test_side_encoding_and_scoring_ms": spans["test_side_ms"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fit_only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lr_eval_bench needs an MI355X: nothing is measured without one")
    if args.fit_only:
        case = LU.make_case(LU.CASES["c2"][0])
        x, y = torch.from_numpy(case["x_train"]).cuda(), torch.from_numpy(case["y_train"]).cuda()
        for _ in range(5):
            ops.logreg_fit(x, y)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernel_times(args.reps), "accuracy": accuracy(),
           "whole_evaluation": whole_evaluation()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
