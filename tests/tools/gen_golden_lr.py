"""Generate tests/golden/g11_lr_*.npz: the reference's latent-representation classifiers and metrics
(mimic/evaluation/eval_metrics/representation.py:147-187, mimic/networks/classifiers/utils.py:286-413) on the seeded
problems of tests/lr_util.py, next to the exact optimum of each problem.

Built on oracle/gen_golden.py (imported as a module through tests/tools/gen_golden_methods.load_generator and left as it
is): its import_reference() makes the reference importable; train_clf_lr and classify_latent_representations take a
SimpleNamespace with `labels`, `flags.verbose`, `flags.dataset`.  Inputs are NOT stored: lr_util.make_case regenerates them
from the seed and the fixture keeps a fingerprint.  Stored per case i of a fixture (data only):
  i/coef_ref [S,L,D+1] f64   the reference's coef_ / intercept_ (scikit-learn's lbfgs stopping point)
  i/pred_ref                 its predictions on the test rows, packed bits of [S,M,L]
  i/metrics [S,K] f64, metrics_keys [K]   its Metrics dictionaries per subset (on its own predictions)
  i/w_star [S,L,D+1] f64     the exact optimum (float64 damped Newton to |grad f|_inf <= 1e-10)
  i/ref_dist [S,L]           |w_ref - w*|_2            i/ref_gap [S,L]   max over the test rows of |decision_ref - decision*|
  i/band_share [S,L]         share of test rows with |decision*| <= 1.25 ref_gap: ASSERTED <= 5 % here for the c2 and small
                             fixtures (their predictions are compared outside that band); a seed that misses the cap is
                             replaced in lr_util.CASES, before any run of the code under test
g11_lr_metrics: the reference's Metrics on stored random prediction / label matrices (one label column predicted all 0).
Usage:  python tests/tools/gen_golden_lr.py [--only c2 small hard metrics]
"""
from __future__ import annotations

import argparse
import os
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(REPO, "tests"), os.path.join(REPO, "oracle"), os.path.join(REPO, "mopoe-mimic_amd")]

import gen_golden_methods as GM  # noqa: E402
import lr_util as LU  # noqa: E402

BAND, CAP = 1.25, 0.05


def ref_metrics(pred, labels, names):
    from mimic.networks.classifiers.utils import Metrics
    m = Metrics(torch.from_numpy(np.asarray(pred, np.float32)), torch.from_numpy(np.asarray(labels, np.float32)), str_labels=names)
    return m.extract_values(m.evaluate())


def gen_case(spec, enforce_cap):
    from mimic.evaluation.eval_metrics.representation import classify_latent_representations, train_clf_lr
    case = LU.make_case(spec)
    s_n, l_n, d = spec["S"], len(spec["kinds"]), spec["D"]
    names = LU.LABEL_NAMES[:l_n]
    exp = SimpleNamespace(labels=names, flags=SimpleNamespace(verbose=0, dataset="mimic"))
    keys = LU.SUBSET_KEYS[:s_n]
    clf = train_clf_lr(exp, {k: case["x_train"][s] for s, k in enumerate(keys)}, case["y_train"])
    pred = classify_latent_representations(exp, clf, {k: case["x_test"][s] for s, k in enumerate(keys)})
    coef = np.zeros((s_n, l_n, d + 1))
    w_star = np.zeros_like(coef)
    pred_ref = np.zeros((s_n, spec["M"], l_n), dtype=np.uint8)
    for s, k in enumerate(keys):
        for l, name in enumerate(names):
            c = clf[name][k]
            coef[s, l, :-1], coef[s, l, -1] = c.coef_[0], c.intercept_[0]
            pred_ref[s, :, l] = pred[name][k].astype(np.uint8)
            w_star[s, l] = LU.newton_exact(case["x_train"][s], case["y_train"][:, l])
    dec_ref, dec_star = LU.decisions(coef, case["x_test"]), LU.decisions(w_star, case["x_test"])
    assert np.array_equal(pred_ref, (dec_ref > 0).astype(np.uint8))
    ref_gap = np.abs(dec_ref - dec_star).max(axis=1)                   # [S, L]
    band_share = (np.abs(dec_star) <= BAND * ref_gap[:, None, :]).mean(axis=1)
    if enforce_cap:
        assert band_share.max() <= CAP, f"seed {spec['seed']}: {band_share.max():.3f} of a problem's test rows inside the band"
    mets = [ref_metrics(pred_ref[s], case["y_test"], names) for s in range(s_n)]
    mkeys = list(mets[0])
    assert all(list(m) == mkeys for m in mets)
    gi = LU.grad_inf(coef, case["x_train"], case["y_train"]) / spec["N"]
    print(f"  seed {spec['seed']} N {spec['N']} D {d}: ref_dist {np.linalg.norm(coef - w_star, axis=2).min():.2e}.."
          f"{np.linalg.norm(coef - w_star, axis=2).max():.2e}  |w*| {np.linalg.norm(w_star, axis=2).min():.2f}.."
          f"{np.linalg.norm(w_star, axis=2).max():.2f}  ref grad/N {gi.min():.2e}..{gi.max():.2e}  ref_gap max {ref_gap.max():.3f}  "
          f"band share max {band_share.max():.3f}", flush=True)
    return {"fingerprint": LU.fingerprint(case), "coef_ref": coef, "w_star": w_star, "pred_ref": np.packbits(pred_ref),
            "ref_dist": np.linalg.norm(coef - w_star, axis=2), "ref_gap": ref_gap, "band_share": band_share,
            "metrics": np.array([[float(m[k]) for k in mkeys] for m in mets]), "metrics_keys": np.array(mkeys)}


def gen_metrics():
    rs = np.random.RandomState(1401)
    store = {}
    for i, (m, l_n) in enumerate(((240, 3), (97, 1), (60, 3))):
        pred = (rs.random_sample((m, l_n)) < 0.45).astype(np.float32)
        labels = (rs.random_sample((m, l_n)) < 0.4).astype(np.float32)
        if i == 2:
            pred[:, 1] = 0.0                  # a label that is never predicted: average precision 0.0
        names = LU.LABEL_NAMES[:l_n] if l_n > 1 else ["Finding"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            met = ref_metrics(pred, labels, names)
        store[f"{i}/pred"], store[f"{i}/labels"] = pred.astype(np.uint8), labels.astype(np.uint8)
        store[f"{i}/names"] = np.array(names)
        store[f"{i}/metrics_keys"], store[f"{i}/metrics"] = np.array(list(met)), np.array([float(v) for v in met.values()])
    store["n"] = np.array(3)
    return store


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    G = GM.load_generator()
    if not os.path.isdir(G.REF):
        print("reference not present; nothing to do")
        return
    G.import_reference()
    warnings.filterwarnings("ignore", category=FutureWarning)
    outdir = os.path.join(REPO, "tests", "golden")
    for name in ("c2", "small", "hard", "metrics"):
        if args.only and name not in args.only:
            continue
        print(name, flush=True)
        if name == "metrics":
            store = gen_metrics()
        else:
            store = {}
            for i, spec in enumerate(LU.CASES[name]):
                store.update({f"{i}/{k}": v for k, v in gen_case(spec, enforce_cap=name != "hard").items()})
        path = os.path.join(outdir, f"g11_lr_{name}.npz")
        np.savez_compressed(path, **store)
        size = os.path.getsize(path)
        assert size <= 200 * 1024, (path, size)
        print(f"wrote {path}: {size / 1024:.0f} KiB, {len(store)} arrays", flush=True)


if __name__ == "__main__":
    main()
