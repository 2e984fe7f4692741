"""TEST INFRASTRUCTURE for --weighted_sampler (tests/test_weighted_sampler_{cpu,gpu}.py): a Python restatement of one weighted
draw (include/mopoe_hip_data.h: mopoe_batch_draw) in integers and IEEE doubles, and the label table the tests write over the
stock fixture's (whose three-label weights are not valid: the reference's "no finding" denominator is -1 there)."""
import bisect
import os

import numpy as np
import torch

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85

# (counter, key, output) of Philox4x32-10, as words: Random123's known answers
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def uniform(seed, epoch, rank, i):
    """u in [0, 1) of draw i: (x0 >> 5) * 2^26 + (x1 >> 6) is an integer below 2^53, exact as a double"""
    seed &= 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10((i & M32, i >> 32, epoch, rank), (seed & M32, seed >> 32))
    return float((x[0] >> 5) * (1 << 26) + (x[1] >> 6)) * 2.0 ** -53


def draws(weights, seed, epoch, rank, first, count):
    """the rows draws first .. first + count - 1 select: list of ints.  weights: float64 tensor / array [n]"""
    cdf = torch.cumsum(torch.as_tensor(weights, dtype=torch.float64), 0).tolist()   # (the prefix sum the product hands the kernel)
    n, total = len(cdf), cdf[-1]
    return [min(bisect.bisect_right(cdf, uniform(seed, epoch, rank, i) * total), n - 1) for i in range(first, first + count)]


LABEL_NAMES = ["Lung Opacity", "Pleural Effusion", "Support Devices"]


def label_table(n=64, seed=11, p1=0.15):
    """a three-label table with valid weights: no -1 rows, row 0 carries two findings, row 1 none"""
    rng = np.random.RandomState(seed)
    lab = rng.choice([0.0, 1.0], size=(n, 3), p=[1.0 - p1, p1])
    lab[0] = [1, 0, 1]
    lab[1] = [0, 0, 0]
    return lab


def write_train_labels(dir_data, img_size, lab):
    import pandas as pd
    pd.DataFrame(lab, columns=LABEL_NAMES).to_csv(os.path.join(dir_data, f"files_small_{img_size}", "train_labels.csv"), index=False)


def make_weighted_files(dir_data, img_size=16, n_train=64, n_eval=12):
    """golden_util.make_mimic_files(seed 3) with train_labels.csv replaced by label_table(n_train); returns the table"""
    from golden_util import make_mimic_files
    make_mimic_files(str(dir_data), img_size=img_size, n_train=n_train, n_eval=n_eval, seed=3)
    lab = label_table(n_train)
    write_train_labels(str(dir_data), img_size, lab)
    return lab
