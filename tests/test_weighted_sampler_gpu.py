"""--weighted_sampler on the GPU (include/mopoe_hip_data.h, csrc/batch.hip): the device draw against its Python restatement
index for index, the batch assembly bit for bit against CPU-computed expectations, both entry points between the guard bands
of tests/arena.py, and two epochs of run_epochs whose training rows are exactly the restatement's draws.

Guard-band coverage of the input-pipeline header (checked by tests/test_weighted_sampler_cpu.py against the header and against
this table, and below against what the library was really asked for): GUARDED."""
import math

import numpy as np
import pytest
import torch

import weighted_util as WU
from arena import Arena, CALLED_UNDER_ARENA, outputs_in
from golden_util import load

pytestmark = pytest.mark.gpu
DEV = "cuda"

GUARDED = {
    "mopoe_batch_draw": "test_batch_draw_between_guard_bands",
    "mopoe_batch_assemble": "test_batch_assemble_between_guard_bands",
}

W48 = [0.03125] * 32 + [0.1] * 10 + [0.18] * 6
# (seed, epoch, rank): seeds 0 and 2^40 + 5 (both key words in use), epochs 0 and 3, ranks 0 and 1
STREAMS = [(0, 0, 0), (0, 0, 1), (0, 3, 0), (2 ** 40 + 5, 0, 0), (2 ** 40 + 5, 3, 1)]


def _weights(kind):
    if kind == "w48":
        return torch.tensor(W48, dtype=torch.float64)
    if kind == "zeros48":       # rows of weight zero: first, last, two in the middle
        w = torch.tensor(W48, dtype=torch.float64)
        w[[0, 20, 21, 47]] = 0.0
        return w
    if kind == "one":
        return torch.tensor([0.25], dtype=torch.float64)
    return torch.from_numpy(load("g12_weights")["t64/weights"])


# ---- batch_draw ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,count,first", [("w48", 4096, 0), ("w48", 1000, 3), ("w48", 1, 4095), ("one", 7, 0),
                                              ("t64", 64, 0), ("zeros48", 4096, 0)])
def test_batch_draw_equals_the_restatement(kind, count, first):
    from mimic_amd import ops
    w = _weights(kind)
    cdf = torch.cumsum(w, 0).to(DEV)
    got = {}
    for seed, epoch, rank in STREAMS:
        out = ops.batch_draw(cdf, seed, epoch, rank, first, count)
        assert out.dtype == torch.int64 and tuple(out.shape) == (count,)
        got[(seed, epoch, rank)] = out.cpu().tolist()
        assert got[(seed, epoch, rank)] == WU.draws(w, seed, epoch, rank, first, count), (kind, seed, epoch, rank)
    if kind == "zeros48":
        assert not {0, 20, 21, 47} & set(got[(0, 0, 0)])
    if w.numel() > 1 and count > 1:       # ranks, epochs and seeds draw independently
        assert len({tuple(v) for v in got.values()}) == len(STREAMS)
        assert got[(0, 0, 0)] != got[(0, 0, 1)]
    assert tuple(ops.batch_draw(cdf, 0, 0, 0, 5, 0).shape) == (0,)


def test_batch_draw_does_not_depend_on_how_an_epoch_is_cut():
    """more draws than one grid covers in one pass (2048 blocks of 256), drawn whole and in pieces"""
    from mimic_amd import ops
    w = _weights("t64")
    cdf = torch.cumsum(w, 0).to(DEV)
    n_draws = 2048 * 256 + 1000
    whole = ops.batch_draw(cdf, 9, 1, 2, 0, n_draws)
    assert int(whole.min()) >= 0 and int(whole.max()) <= 63
    for first, count in ((0, 300), (2048 * 256 - 7, 1007), (123457, 4096)):
        assert torch.equal(ops.batch_draw(cdf, 9, 1, 2, first, count), whole[first:first + count])
    assert whole[2048 * 256 - 3:2048 * 256 + 3].tolist() == WU.draws(w, 9, 1, 2, 2048 * 256 - 3, 6)
    # the shares follow the weights: 5 binomial standard deviations of 525 288 draws
    counts = torch.bincount(whole, minlength=64).cpu().double()
    p = (w / w.sum())
    assert bool(((counts - n_draws * p).abs() <= 5.0 * torch.sqrt(n_draws * p * (1 - p))).all())


def test_batch_ops_refuse_what_they_cannot_run():
    from mimic_amd import ops
    cdf = torch.cumsum(_weights("w48"), 0).to(DEV)
    for bad in (lambda: ops.batch_draw(cdf.float(), 0, 0, 0, 0, 4), lambda: ops.batch_draw(cdf, 0, 0, 0, -1, 4),
                lambda: ops.batch_draw(cdf, 0, 0, 0, 0, -4), lambda: ops.batch_draw(cdf[:0], 0, 0, 0, 0, 4),
                lambda: ops.batch_draw(cdf, 0, -1, 0, 0, 4), lambda: ops.batch_draw(cdf.cpu(), 0, 0, 0, 0, 4)):
        with pytest.raises(ops.MopoeHipError):
            bad()
    src = _source(4, 16, "word", 3)
    d = {k: v.to(DEV) for k, v in src.items()}
    sel = torch.tensor([1, 2], device=DEV)
    ok = lambda **kw: ops.batch_assemble(*[kw.get(k, d[k]) for k in ("pa", "lat", "text", "labels")], kw.get("sel", sel), kw.get("f"))
    ok()
    for kw in ({"pa": d["pa"].float()}, {"lat": d["lat"][:3]}, {"text": d["text"].long()}, {"f": 7}, {"labels": d["labels"].double()},
               {"sel": sel.int()}, {"sel": sel[:0]}, {"sel": sel.cpu()}, {"labels": d["labels"][:2]}, {"pa": d["pa"][:, :, :8], "lat": d["lat"][:, :, :8]}):
        with pytest.raises(ops.MopoeHipError):
            ok(**kw)


# ---- batch_assemble --------------------------------------------------------------------------------------------------------
def _source(n, s, text, n_labels, seed=0):
    """a resident split on the CPU: row 0 of PA holds every byte value when S = 16"""
    g = torch.Generator().manual_seed(100 * s + seed)
    pa = torch.randint(0, 256, (n, s, s), generator=g, dtype=torch.uint8)
    lat = torch.randint(0, 256, (n, s, s), generator=g, dtype=torch.uint8)
    if s == 16:
        pa[0] = torch.arange(256, dtype=torch.uint8).view(16, 16)
        lat[n - 1] = torch.arange(255, -1, -1, dtype=torch.uint8).view(16, 16)
    if text == "word":
        t = torch.randint(0, 3517, (n, 12), generator=g, dtype=torch.int32)
    else:
        t = torch.randint(0, 7, (n, 5), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 2, (n, n_labels), generator=g).float()
    return {"pa": pa, "lat": lat, "text": t, "labels": labels}


def _expected(src, sel, num_features):
    """what the CPU computes: index gather, u8.float() / 255, one_hot"""
    n = src["pa"].shape[0]
    rows = torch.as_tensor(sel).clamp(0, n - 1)
    text = src["text"][rows]
    text = text.float() if num_features is None else torch.nn.functional.one_hot(text.long(), num_features).float()
    return (src["pa"][rows].unsqueeze(1).float() / 255, src["lat"][rows].unsqueeze(1).float() / 255, text, src["labels"][rows])


SELS = {5: [[3, 0, 3, 8, 0], [-1, 9, 2, -(2 ** 40), 2 ** 40]], 1: [[0], [8], [9]]}      # n = 9: repeats; rows outside [0, n)


@pytest.mark.parametrize("n_labels", [3, 1])
@pytest.mark.parametrize("text", ["word", "char"])
@pytest.mark.parametrize("s", [16, 6])
def test_batch_assemble_is_bit_exact(s, text, n_labels):
    from mimic_amd import ops
    src = _source(9, s, text, n_labels)
    dev = {k: v.to(DEV) for k, v in src.items()}
    f = 7 if text == "char" else None
    for b, sels in SELS.items():
        for sel in sels:
            got = ops.batch_assemble(dev["pa"], dev["lat"], dev["text"], dev["labels"], torch.tensor(sel, device=DEV), f)
            want = _expected(src, sel, f)
            shapes = [(b, 1, s, s), (b, 1, s, s), (b, 5, 7) if f else (b, 12), (b, n_labels)]
            for name, g_, w_, shape in zip(("PA", "Lateral", "text", "labels"), got, want, shapes):
                assert g_.dtype == torch.float32 and tuple(g_.shape) == shape, (name, g_.shape)
                assert torch.equal(g_.cpu(), w_), (s, text, n_labels, sel, name)
    if s == 16:       # every byte value went through the conversion
        got = ops.batch_assemble(dev["pa"], dev["lat"], dev["text"], dev["labels"], torch.tensor([0], device=DEV), f)
        assert torch.equal(got[0].cpu().flatten(), torch.arange(256).float() / 255)


def test_batch_assemble_reaches_rows_past_two_to_the_31_bytes():
    """n * S * S above 2^31: the row offset is 64-bit arithmetic"""
    from mimic_amd import ops
    n, s = 131072 + 9000, 128
    pa = torch.zeros(n, s, s, dtype=torch.uint8, device=DEV)
    rows = [n - 1, 131073, 0, 70000]
    g = torch.Generator().manual_seed(5)
    marks = torch.randint(0, 256, (4, s, s), generator=g, dtype=torch.uint8)
    text = torch.zeros(n, 4, dtype=torch.int32, device=DEV)
    labels = torch.zeros(n, 1, device=DEV)
    for k, r in enumerate(rows):
        pa[r] = marks[k].to(DEV)
        text[r] = k + 1
        labels[r] = k + 2.0
    got = ops.batch_assemble(pa, pa, text, labels, torch.tensor(rows + [n + 5], device=DEV))
    want = marks[[0, 1, 2, 3, 0]].unsqueeze(1).float() / 255
    assert torch.equal(got[0].cpu(), want) and torch.equal(got[1].cpu(), want)
    assert got[2].cpu()[:, 0].tolist() == [1, 2, 3, 4, 1] and got[3].cpu()[:, 0].tolist() == [2, 3, 4, 5, 2]


# ---- between the guard bands -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    return Arena(DEV, capacity=96 << 20, capacity64=24 << 20)


def _bits(t):
    return t.contiguous().view(torch.uint8).cpu()


def _in_arena(arena, inputs, misalign, call):
    """place the inputs, run the call with its results allocated between poisoned guards (the results start as NaN patterns),
    check the guards, that the results are arena views and that no input changed"""
    arena.reset()
    placed = {k: arena.place(v, misalign.get(k, 0), name=k) for k, v in inputs.items()}
    for k, off in misalign.items():
        assert placed[k].data_ptr() % 16 == off
    before = {k: _bits(v) for k, v in placed.items()}
    CALLED_UNDER_ARENA.clear()
    with outputs_in(arena) as px:
        got = call(placed)
    torch.cuda.synchronize()
    arena.assert_untouched()
    got = got if isinstance(got, tuple) else (got,)
    assert len(px.allocated) == len(got) and all(arena.owns(t) for t in got)
    for k, v in placed.items():
        assert torch.equal(_bits(v), before[k]), f"input {k} was modified"
    return got


def test_batch_draw_between_guard_bands(arena):
    from mimic_amd import ops
    for kind, count, first in (("w48", 1000, 3), ("one", 7, 0), ("zeros48", 4097, 0)):
        w = _weights(kind)
        (out,) = _in_arena(arena, {"cdf": torch.cumsum(w, 0)}, {},
                           lambda p: ops.batch_draw(p["cdf"], 2 ** 40 + 5, 3, 1, first, count))
        assert out.cpu().tolist() == WU.draws(w, 2 ** 40 + 5, 3, 1, first, count)
        assert "mopoe_batch_draw" in CALLED_UNDER_ARENA


@pytest.mark.parametrize("s,text,off", [(16, "word", 4), (16, "word", 0), (16, "char", 4), (6, "char", 4), (6, "word", 0)])
def test_batch_assemble_between_guard_bands(arena, s, text, off):
    """off = 4: the uint8 arrays start 4 bytes off a 16-byte boundary (the scalar path, whatever S); off = 0 with S = 16: the
    16-byte path with its stores against the guards"""
    from mimic_amd import ops
    src = _source(9, s, text, 3, seed=1)
    f = 7 if text == "char" else None
    misalign = {k: off for k in ("pa", "lat") + (("text",) if text == "char" else ())} if off else {}
    for sel in ([3, 0, 3, 8, 0], [-1, 9, 2, -(2 ** 40), 2 ** 40], [8]):
        inputs = dict(src, sel=torch.tensor(sel))
        got = _in_arena(arena, inputs, misalign,
                        lambda p: ops.batch_assemble(p["pa"], p["lat"], p["text"], p["labels"], p["sel"], f))
        for name, g_, w_ in zip(("PA", "Lateral", "text", "labels"), got, _expected(src, sel, f)):
            assert torch.equal(g_.cpu(), w_), (s, text, off, sel, name)
        assert "mopoe_batch_assemble" in CALLED_UNDER_ARENA


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _run(tmp_path, monkeypatch, weighted, end_epoch):
    """run_epochs in-process on the 64-row files; returns (history, experiment, per train epoch: the yielded batches)"""
    from mimic_amd import run_epochs as RE
    from mimic_amd.dataio.MimicDataset import DeviceResidentMimic
    from mimic_amd.utils.experiment import HotPathExperiment, default_flags
    flags = default_flags(dataset="mimic", dir_data=str(tmp_path / "data"), img_size=64, class_dim=16, DIM_img=8, DIM_text=8,
                          batch_size=8, len_sequence=128, weighted_sampler=weighted, end_epoch=end_epoch, seed=0,
                          initial_learning_rate=1e-5, dir_checkpoints=str(tmp_path / f"ck{int(weighted)}"),
                          device=torch.device("cuda", 0))
    exp = HotPathExperiment(flags)
    seen = {}
    plain_iter = DeviceResidentMimic.__iter__

    def recording_iter(self):
        for data, labels in plain_iter(self):
            if self.n == 64:          # (the train split; the eval split has 12 rows or fewer)
                seen.setdefault(self.epoch, []).append((data["PA"], data["text"], labels, self.cdf is not None))
            yield data, labels

    monkeypatch.setattr(DeviceResidentMimic, "__iter__", recording_iter)
    history = RE.run_epochs(0, exp)
    monkeypatch.setattr(DeviceResidentMimic, "__iter__", plain_iter)
    return history, exp, seen


def test_two_weighted_epochs_train_on_the_restated_draws(tmp_path, monkeypatch):
    lab = WU.make_weighted_files(tmp_path / "data", img_size=64)
    history, exp, seen = _run(tmp_path, monkeypatch, True, 2)
    files = exp.dataset_train.files
    assert len(files) == 64 and torch.equal(files.label_matrix, torch.from_numpy(lab).float())
    np.testing.assert_array_equal(exp.train_weights.numpy(), load("g12_weights")["t64/weights"])
    assert [h["epoch"] for h in history] == [0, 1]
    assert history[0]["train"]["steps"] == history[1]["train"]["steps"] == 8
    assert history[1]["train"]["graphed_steps"] > 0
    for h in history:
        assert all(math.isfinite(v) for v in h["train"]["last"].values()) and math.isfinite(h["test"]["total_loss"])
        assert math.isfinite(h["train"]["mean"]["total_loss"])
    text_ids = files.text_ids()
    for epoch in (0, 1):
        want = WU.draws(exp.train_weights, 0, epoch, 0, 0, 64)
        assert len(seen[epoch]) == 8 and all(w for *_x, w in seen[epoch])
        for k, (pa, text, labels, _w) in enumerate(seen[epoch]):
            rows = torch.tensor(want[8 * k:8 * k + 8])
            assert torch.equal(labels.cpu(), files.label_matrix[rows]), (epoch, k)
            assert torch.equal(pa.cpu(), files.pa[rows].unsqueeze(1).float() / 255), (epoch, k)
            assert torch.equal(text.cpu(), text_ids[rows].float()), (epoch, k)
    assert WU.draws(exp.train_weights, 0, 0, 0, 0, 64) != WU.draws(exp.train_weights, 0, 1, 0, 0, 64)
    # the same run without the flag: the uniform loader's permutation of the 64 rows, not the draws
    history_u, exp_u, seen_u = _run(tmp_path, monkeypatch, False, 1)
    assert exp_u.train_weights is None and len(seen_u[0]) == 8 and not any(w for *_x, w in seen_u[0])
    g = torch.Generator()
    g.manual_seed(0)
    perm = torch.randperm(64, generator=g)
    got_u = torch.cat([labels.cpu() for _pa, _t, labels, _w in seen_u[0]])
    assert torch.equal(got_u, files.label_matrix[perm])
    assert not torch.equal(got_u, files.label_matrix[torch.tensor(WU.draws(exp.train_weights, 0, 0, 0, 0, 64))])
    assert math.isfinite(history_u[0]["test"]["total_loss"])
