"""--weighted_sampler without a GPU: the label weights against the reference's own (fixture g12_weights, written by
tests/tools/gen_golden_weights.py from mimic/dataio/utils.py:81-94 calculateWeights), the up-front refusal of a label table the
reference's formula has no valid weights for, the host loader path, the Python restatement of the device draw
(tests/weighted_util.py) and the coverage of include/mopoe_hip_data.h by the GPU file's guard-band table."""
import argparse
import ctypes
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import weighted_util as WU
from golden_util import load, make_mimic_files
from mimic_amd.dataio.MimicDataset import DeviceResidentMimic, Mimic
from mimic_amd.dataio.utils import get_data_loaders, label_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = WU.LABEL_NAMES


def _args(tmp, **kw):
    a = argparse.Namespace(dir_data=str(tmp), img_size=16, text_encoding="word", len_sequence=12, word_min_occ=3,
                           undersample_dataset=False, feature_extractor_img="resnet", batch_size=8, distributed=False,
                           dataloader_workers=0, world_size=1, binary_labels=False)
    a.__dict__.update(kw)
    return a


# ---- the weights -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t64", "t48", "t200", "bin64"])
def test_label_weights_equal_the_reference_bit_for_bit(name):
    g = load("g12_weights")
    lab = g[name + "/labels"]
    binary = name == "bin64"
    frame = pd.DataFrame(lab, columns=["Finding"] if binary else LABELS)
    w = label_weights(frame, binary)
    assert w.dtype == torch.float64 and tuple(w.shape) == (lab.shape[0],)
    np.testing.assert_array_equal(w.numpy(), g[name + "/weights"])
    if name == "t64":       # the table the other tests train on: the issue's figures
        np.testing.assert_array_equal(lab, WU.label_table(64))
        assert (lab == 1).sum(0).tolist() == [13, 10, 9] and len(set(w.tolist())) == 6
        assert min(w.tolist()) == 0.03125 and abs(max(w.tolist()) - 0.18803) < 1e-5
    if binary:
        assert sorted(set(w.tolist())) == [1 / 35, 1 / 29]


def test_invalid_label_tables_are_refused_up_front(tmp_path):
    """the stock fixture: N 36, counts 17 / 6 / 14, so the no-finding weight would be 1 / -1 for 8 rows"""
    from mimic_amd.utils.experiment import HotPathExperiment, default_flags
    make_mimic_files(str(tmp_path), img_size=16, n_train=40, n_eval=12, seed=3)
    ds = Mimic(_args(tmp_path), LABELS, split="train")
    v = ds.labels[LABELS].to_numpy()
    assert len(ds) == 36 and (v == 1).sum(0).tolist() == [17, 6, 14] and int((v == 0).all(1).sum()) == 8
    with pytest.raises(ValueError, match=r"17.*6.*14.*N = 36"):
        label_weights(ds.labels, False)
    flags = default_flags(dataset="mimic", dir_data=str(tmp_path), img_size=16, len_sequence=12, batch_size=8,
                          weighted_sampler=True, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="N = 36"):
        HotPathExperiment(flags)
    with pytest.raises(ValueError):
        get_data_loaders(_args(tmp_path), ds, "train", weighted_sampler=True)
    # no row without a finding: the non-positive denominator is never used, the table is fine
    busy = pd.DataFrame([[1, 1, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]], columns=LABELS, dtype=float)
    w = label_weights(busy, False)
    np.testing.assert_array_equal(w.numpy(), [(1 / 3 + 1 / 3) + 1 / 3, 1 / 3 + 1 / 3, 1 / 3 + 1 / 3, 1 / 3 + 1 / 3])
    # a zero denominator with a no-finding row, and the binary form's
    with pytest.raises(ValueError, match="N = 3"):
        label_weights(pd.DataFrame([[1, 1, 0], [0, 0, 1], [0, 0, 0]], columns=LABELS, dtype=float), False)
    # a label nobody carries contributes 0 (binary: N - count >= 1 wherever a 0-row exists, so that form is always valid)
    np.testing.assert_array_equal(label_weights(pd.DataFrame([[0.0], [0.0]], columns=["Finding"]), True).numpy(), [0.5, 0.5])
    np.testing.assert_array_equal(label_weights(pd.DataFrame([[1.0], [1.0]], columns=["Finding"]), True).numpy(), [0.5, 0.5])
    w = label_weights(pd.DataFrame([[1, 0, 0], [0, 0, 0], [0, 0, 0]], columns=LABELS, dtype=float), False)
    np.testing.assert_array_equal(w.numpy(), [1.0, 0.5, 0.5])


def test_flag_is_parsed_and_needs_a_label_table(tmp_path):
    from mimic_amd.main_mimic import parse_flags
    from mimic_amd.utils.experiment import HotPathExperiment, check_flags
    assert parse_flags([]).weighted_sampler is False
    flags = parse_flags(["--weighted_sampler", "true"])
    assert flags.weighted_sampler is True and flags.dataset == "testing"
    with pytest.raises(ValueError, match="testing"):
        check_flags(flags)
    flags.device = torch.device("cpu")
    with pytest.raises(ValueError, match="testing"):
        HotPathExperiment(flags)


# ---- the host loader path --------------------------------------------------------------------------------------------------
def test_host_loader_draws_with_the_label_weights(tmp_path):
    lab = WU.make_weighted_files(tmp_path)
    args = _args(tmp_path)
    ds = Mimic(args, LABELS, split="train")
    assert len(ds) == 64
    want = label_weights(ds.labels, False)
    np.testing.assert_array_equal(want.numpy(), load("g12_weights")["t64/weights"])
    sampler, loader = get_data_loaders(args, ds, "train", weighted_sampler=True)
    assert isinstance(sampler, torch.utils.data.WeightedRandomSampler) and sampler.replacement
    assert torch.equal(torch.as_tensor(sampler.weights), want) and sampler.num_samples == len(ds) == 64
    assert loader.sampler is sampler and len(loader) == 8
    batch, labels = next(iter(loader))
    assert tuple(batch["PA"].shape) == (8, 1, 16, 16) and tuple(labels.shape) == (8, 3)
    assert set(map(tuple, labels.tolist())) <= set(map(tuple, lab.tolist()))
    sampler, loader = get_data_loaders(args, ds, "train", weighted_sampler=True, nbr_samples_4_sampler=20)
    assert sampler.num_samples == 20 and len(loader) == 3
    # as in the reference, the weighted sampler takes the distributed sampler's place ...
    dist_args = _args(tmp_path, distributed=True, world_size=2)
    # ... and 'eval' ignores the flag
    ev = Mimic(args, LABELS, split="eval")
    sampler, loader = get_data_loaders(args, ev, "eval", weighted_sampler=True)
    assert sampler is None and isinstance(loader.sampler, torch.utils.data.RandomSampler)
    assert isinstance(get_data_loaders(dist_args, ds, "train", weighted_sampler=True, nbr_samples_4_sampler=16)[0],
                      torch.utils.data.WeightedRandomSampler)
    # the experiment keeps the weights
    from mimic_amd.utils.experiment import HotPathExperiment, default_flags
    seen = {}

    class WeightsOnly(HotPathExperiment):          # (stops after the datasets: no networks at 16 px)
        def set_modalities(self):
            seen["weights"] = self.train_weights
            raise KeyboardInterrupt

    flags = default_flags(dataset="mimic", dir_data=str(tmp_path), img_size=16, len_sequence=12, batch_size=8,
                          weighted_sampler=True, device=torch.device("cpu"))
    with pytest.raises(KeyboardInterrupt):
        WeightsOnly(flags)
    assert torch.equal(seen["weights"], want)
    flags.weighted_sampler = False
    with pytest.raises(KeyboardInterrupt):
        WeightsOnly(flags)
    assert seen["weights"] is None


def test_device_resident_weighted_form_has_no_cpu_fallback(tmp_path):
    from mimic_amd.ops import MopoeHipError
    WU.make_weighted_files(tmp_path)
    ds = Mimic(_args(tmp_path), LABELS, split="train")
    w = label_weights(ds.labels, False)
    with pytest.raises(MopoeHipError, match="no CPU fallback"):
        DeviceResidentMimic(ds, "cpu", batch_size=8, weights=w)
    with pytest.raises(MopoeHipError):
        from mimic_amd import ops
        ops.batch_draw(torch.cumsum(w, 0), 0, 0, 0, 0, 4)
    with pytest.raises(MopoeHipError):
        ops.batch_assemble(torch.zeros(2, 4, 4, dtype=torch.uint8), torch.zeros(2, 4, 4, dtype=torch.uint8),
                           torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3), torch.zeros(1, dtype=torch.int64))
    # without weights: every line as before
    src = DeviceResidentMimic(ds, "cpu", batch_size=8, shuffle=False, weights=None)
    assert src.cdf is None and len(src) == 8
    k = 0
    for data, labels in src:
        for j in range(labels.shape[0]):
            s, lab = ds[k]
            assert torch.equal(data["PA"][j], s["PA"]) and torch.equal(data["text"][j], s["text"]) and torch.equal(labels[j], lab)
            k += 1
    assert k == 64
    sh = DeviceResidentMimic(ds, "cpu", batch_size=8, shuffle=True, seed=0)
    g = torch.Generator()
    g.manual_seed(0)
    assert sh._indices() == torch.randperm(64, generator=g).tolist()


# ---- the restatement of the device draw ------------------------------------------------------------------------------------
def test_philox_restatement_reproduces_the_known_answers():
    for counter, key, out in WU.KNOWN_ANSWERS:
        assert WU.philox4x32_10(counter, key) == out
    us = [WU.uniform(2 ** 40 + 5, 3, 1, i) for i in range(64)]
    assert all(0.0 <= u < 1.0 for u in us) and len(set(us)) == 64
    assert WU.uniform(0, 0, 0, 0) == float((0x6627E8D5 >> 5) * 2 ** 26 + (0xE169C58D >> 6)) * 2.0 ** -53
    # a draw is a function of (seed, epoch, rank, i) alone: pieces of an epoch are the epoch
    w = torch.tensor([0.03125] * 32 + [0.1] * 10 + [0.18] * 6, dtype=torch.float64)
    whole = WU.draws(w, 7, 2, 1, 0, 100)
    assert WU.draws(w, 7, 2, 1, 40, 25) == whole[40:65]
    assert whole != WU.draws(w, 7, 2, 0, 0, 100) and whole != WU.draws(w, 7, 3, 1, 0, 100) and whole != WU.draws(w, 8, 2, 1, 0, 100)


def test_restated_draws_follow_the_weights():
    w = [0.03125] * 32 + [0.1] * 10 + [0.18] * 6
    n_draws, total = 4096, sum(w)
    got = WU.draws(torch.tensor(w, dtype=torch.float64), 0, 0, 0, 0, n_draws)
    counts = np.bincount(got, minlength=48)
    assert counts.sum() == n_draws and len(counts) == 48
    worst = 0.0
    for j, wj in enumerate(w):
        p = wj / total
        sigma = math.sqrt(n_draws * p * (1 - p))
        worst = max(worst, abs(counts[j] - n_draws * p) / sigma)
    print(f"worst deviation {worst:.2f} binomial standard deviations")
    assert worst <= 5.0
    # rows of weight zero never appear: first, last and two middle rows
    wz = torch.tensor(w, dtype=torch.float64)
    wz[[0, 20, 21, 47]] = 0.0
    gz = WU.draws(wz, 0, 0, 0, 0, n_draws)
    assert not {0, 20, 21, 47} & set(gz) and set(gz) == set(range(48)) - {0, 20, 21, 47}
    assert WU.draws(torch.ones(1, dtype=torch.float64), 5, 0, 0, 0, 7) == [0] * 7


# ---- the input-pipeline header against the library and the GPU file's table ------------------------------------------------------
def _declared(header):
    text = open(os.path.join(REPO, "include", header)).read()
    return set(re.findall(r"\b(mopoe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_every_input_pipeline_entry_point_is_exported_and_guarded():
    import test_weighted_sampler_gpu as G
    from mimic_amd import ops
    if not os.path.exists(ops.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    names = _declared("mopoe_hip_data.h")
    assert names == {"mopoe_batch_draw", "mopoe_batch_assemble"}
    lib = ctypes.CDLL(ops.LIB_PATH)
    for fn in names:
        assert hasattr(lib, fn), fn
    assert not names & _declared("mopoe_hip.h"), "the input-pipeline entry points live in their own header"
    assert set(G.GUARDED) == names
    for fn, test in G.GUARDED.items():
        assert callable(getattr(G, test, None)), (fn, test)
        assert hasattr(ops, fn[len("mopoe_"):])
    lib.mopoe_abi_version.restype = ctypes.c_int
    assert lib.mopoe_abi_version() == ops.ABI_VERSION and len(ops.PROF_KINDS) == 144
