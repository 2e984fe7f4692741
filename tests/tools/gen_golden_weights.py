"""Generate tests/golden/g12_weights.npz: the sampling weights the reference's own calculateWeights (mimic/dataio/utils.py:
81-94) gives for a few label tables -- what dataio.utils.label_weights must reproduce bit for bit.

oracle/gen_golden.py is imported as a module and left as it is; its import_reference() makes the reference importable.
Only label tables and the float64 weights are written.  Entries, each as `<name>/labels` (float64 [n, 3] or [n, 1]) and
`<name>/weights` (float64 [n]):
  t64, t48, t200   three-label tables of tests/weighted_util.label_table (n, seed 11, p1 0.15)
  bin64            binary table: Finding = any label of t64
Usage:  python tests/tools/gen_golden_weights.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "oracle"), os.path.join(REPO, "mopoe-mimic_amd")]


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(REPO, "oracle", "gen_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    return G


def reference_weights(calculateWeights, table, names, binary):
    """what reference get_data_loaders does with dataset.labels (dataio/utils.py:128-130)"""
    import pandas as pd
    labels_df = pd.DataFrame(table, columns=names)
    label_counts = labels_df[labels_df == 1].count()
    weights, _ = calculateWeights(labels_df, label_counts, binary)
    return weights.numpy().astype(np.float64)


def main():
    from weighted_util import LABEL_NAMES, label_table
    G = load_generator()
    G.import_reference()
    from mimic.dataio.utils import calculateWeights
    store = {}
    for name, n in (("t64", 64), ("t48", 48), ("t200", 200)):
        lab = label_table(n, seed=11, p1=0.15)
        store[name + "/labels"] = lab
        store[name + "/weights"] = reference_weights(calculateWeights, lab, LABEL_NAMES, False)
    finding = (label_table(64) == 1).any(axis=1).astype(np.float64)[:, None]
    store["bin64/labels"] = finding
    store["bin64/weights"] = reference_weights(calculateWeights, finding, ["Finding"], True)
    out = os.path.join(REPO, "tests", "golden", "g12_weights.npz")
    np.savez_compressed(out, **store)
    for k in sorted(store):
        print(k, store[k].shape, store[k].dtype)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
