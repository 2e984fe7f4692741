"""What --weighted_sampler costs on the device-resident input path, at BASELINE config #2 shapes (B 64, 128 px, word text
L 128) on a synthetic resident split of `--rows` rows:

  assemble   one training batch out of the resident split: ops.batch_assemble (one launch) against the torch-op assembly of
             the uniform loader (index_select / float / div_ per modality) on the same indices;
  draw       the epoch's ops.batch_draw at n = `--draw-rows` rows (one launch per epoch);
  train      run_epochs.train() samples/s over the same split with the weighted and with the uniform loader, each arm with
             its own model, HipAdam and captured step.

The arms of a comparison alternate in one process, `--rounds` times (the order flips every round); a turn is timed between
two synchronisations.  Medians over the rounds are reported.

    python tests/tools/weighted_batch_bench.py [--rounds 5] [--batches 200] [--epochs 2] [--out FILE]
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "mopoe-mimic_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (CONFIGS: the benchmark's own shapes)
from mimic_amd import ops  # noqa: E402
from mimic_amd import run_epochs as RE  # noqa: E402
from mimic_amd.dataio.MimicDataset import DeviceResidentMimic  # noqa: E402
from mimic_amd.dataio.utils import get_str_labels, label_weights  # noqa: E402
from mimic_amd.utils.experiment import HotPathExperiment, default_flags  # noqa: E402


class SyntheticSplit:
    """what DeviceResidentMimic reads of a MimicSplit, without files: uint8 images, word ids, a three-label table"""

    def __init__(self, rows, size, length, vocab, seed=0):
        import pandas as pd
        g = torch.Generator().manual_seed(seed)
        self.args = argparse.Namespace(img_size=size)
        self.rows = np.arange(rows, dtype=np.int64)
        self.pa = torch.randint(0, 256, (rows, size, size), generator=g, dtype=torch.uint8)
        self.lat = torch.randint(0, 256, (rows, size, size), generator=g, dtype=torch.uint8)
        self._ids = torch.randint(0, vocab, (rows, length), generator=g, dtype=torch.int32)
        self.sentences = object()       # (word encoding)
        lab = (torch.rand(rows, 3, generator=g) < 0.15).double().numpy()
        self.label_frame = pd.DataFrame(lab, columns=get_str_labels(False))
        self.label_matrix = torch.from_numpy(lab).float()

    def __len__(self):
        return int(self.rows.shape[0])

    def text_ids(self):
        return self._ids


def torch_assemble(src, sel):
    """the uniform loader's batch (DeviceResidentMimic.__iter__), on given indices"""
    pa = src.pa.index_select(0, sel).unsqueeze(1).float().div_(255.0)
    lat = src.lat.index_select(0, sel).unsqueeze(1).float().div_(255.0)
    return pa, lat, src.text.index_select(0, sel).float(), src.labels.index_select(0, sel)


def alternate(arms, rounds, turn):
    """turn(arm) -> seconds of one synchronised turn; -> {arm: [seconds per round]}"""
    names = list(arms)
    out = {a: [] for a in names}
    for r in range(rounds):
        for a in (names if r % 2 == 0 else names[::-1]):
            out[a].append(turn(a))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--draw-rows", type=int, default=200000)
    ap.add_argument("--epochs", type=int, default=2, help="train() epochs per turn")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    size, cdim, dimg, bsz, cdtype = bench.CONFIGS["c2"]
    length, vocab = 128, 3517
    split = SyntheticSplit(args.rows, size, length, vocab)
    weights = label_weights(split.label_frame, False)
    out = {"config": f"c2 shapes: B {bsz}, {size} px, word L {length}, resident split of {args.rows} rows",
           "rounds": args.rounds, "batches_per_round": args.batches}

    # ---- per-batch assembly --------------------------------------------------------------------------------------------
    src = DeviceResidentMimic(split, device, bsz, True, 0, 1, 0, weights=weights)
    order = ops.batch_draw(src.cdf, 0, 0, 0, 0, args.batches * bsz)
    sels = [order[i * bsz:(i + 1) * bsz] for i in range(args.batches)]
    same = all(torch.equal(a, b) for a, b in zip(ops.batch_assemble(src.pa, src.lat, src.text, src.labels, sels[0]),
                                                 torch_assemble(src, sels[0])))
    arms = {"batch_assemble": lambda: [ops.batch_assemble(src.pa, src.lat, src.text, src.labels, s) for s in sels],
            "torch_ops": lambda: [torch_assemble(src, s) for s in sels]}
    for fn in arms.values():
        fn()
    secs = alternate(arms, args.rounds, lambda a: timed(arms[a]))
    us = {a: [1e6 * s / args.batches for s in v] for a, v in secs.items()}
    out["assemble_us_per_batch"] = {a: {"median": round(statistics.median(v), 2), "rounds": [round(x, 2) for x in v]}
                                    for a, v in us.items()}
    out["assemble_bit_identical_to_torch_ops_on_gpu"] = bool(same)

    # ---- the epoch's draw ----------------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(1)
    cdf = torch.cumsum(torch.rand(args.draw_rows, generator=g, dtype=torch.float64) + 0.01, 0).to(device)
    ops.batch_draw(cdf, 0, 0, 0, 0, args.draw_rows)
    draw = [1e6 * timed(lambda: [ops.batch_draw(cdf, 0, e, 0, 0, args.draw_rows) for e in range(args.batches)]) / args.batches
            for _ in range(args.rounds)]
    out["draw_us_per_epoch"] = {"rows": args.draw_rows, "median": round(statistics.median(draw), 2),
                                "rounds": [round(x, 2) for x in draw]}

    # ---- train() over the split ----------------------------------------------------------------------------------------
    if not args.skip_train:
        runs = {}
        for arm in ("uniform", "weighted"):
            torch.manual_seed(0)
            flags = default_flags(img_size=size, class_dim=cdim, DIM_img=dimg, batch_size=bsz, device=device, vocab_size=vocab,
                                  len_sequence=length, initial_learning_rate=1e-5, compute_dtype=cdtype)
            exp = HotPathExperiment(flags)
            exp.mm_vae.to(device)
            exp.set_optimizer()
            loader = DeviceResidentMimic(split, device, bsz, True, 0, 1, 0, weights=weights if arm == "weighted" else None)
            runs[arm] = {"exp": exp, "loader": loader, "epoch": 0, "graphed": 0}
            RE.train(exp, loader)       # (capture + warm-up epoch, not timed)
        torch.cuda.synchronize()

        def turn(arm):
            s, rates = runs[arm], []
            for _ in range(args.epochs):
                s["epoch"] += 1
                s["loader"].set_epoch(s["epoch"])
                torch.cuda.synchronize()
                r = RE.train(s["exp"], s["loader"])
                rates.append(r["samples_per_sec"])
                s["graphed"] += r["graphed_steps"]
            return statistics.median(rates)

        rates = alternate(runs, args.rounds, turn)
        med = {a: statistics.median(v) for a, v in rates.items()}
        out["train_samples_per_sec"] = {a: {"median": round(med[a], 1), "rounds": [round(x, 1) for x in v]} for a, v in rates.items()}
        out["train_weighted_cost_pct"] = round(100.0 * (med["uniform"] / med["weighted"] - 1.0), 2)
        out["train_graphed_steps"] = {a: s["graphed"] for a, s in runs.items()}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
