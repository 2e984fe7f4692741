"""Latent-representation evaluation (--eval_lr) on CPU: the Metrics restatement against the reference's dictionaries
(tests/golden/g11_lr_*, written by tests/tools/gen_golden_lr.py), the float64 test backend against the exact optimum, the
resampling loop, the host logic on the tiny model with the HIP ops replaced by tests/torch_backend_lr.py, the flags, the
launcher's result line and the epoch hook."""
import numpy as np
import pytest
import torch

import lr_util as LU
import model_util
import mopoe_ref as R
import torch_backend_lr
from golden_util import load
from mimic_amd import main_mimic as MM
from mimic_amd import run_epochs as RE
from mimic_amd.utils.experiment import default_flags

SUBSETS = {"PA", "Lateral", "text", "Lateral_PA", "PA_text", "Lateral_text", "Lateral_PA_text"}


def metric_keys(names):
    return (["accuracy", "recall", "specificity", "precision", "f1", "jaccard", "dice"] + [f"mean_AP_{n}" for n in names]
            + ["mean_AP_total"] + [f"pred_count_{n}" for n in names] + [f"gt_count_{n}" for n in names])


def check_metrics(pred, labels, names, keys, values, what):
    from mimic_amd.networks.classifiers.utils import Metrics
    m = Metrics(torch.from_numpy(pred), torch.from_numpy(labels), str_labels=names)
    got = m.extract_values(m.evaluate())
    assert list(got) == [str(k) for k in keys] == metric_keys(names), what
    for k, ref in zip(got, values):
        assert abs(float(got[k]) - float(ref)) <= 1e-9, (what, k, got[k], ref)


def test_metrics_against_reference_on_random_matrices():
    g = load("g11_lr_metrics")
    for i in range(int(g["n"])):
        names = [str(n) for n in g[f"{i}/names"]]
        check_metrics(g[f"{i}/pred"].astype(np.float32), g[f"{i}/labels"].astype(np.float32), names, g[f"{i}/metrics_keys"],
                      g[f"{i}/metrics"], i)
    # the fixture holds the case the issue names: a label that is never predicted scores an average precision of 0.0
    keys = [str(k) for k in g["2/metrics_keys"]]
    assert g["2/pred"][:, 1].sum() == 0 and g["2/metrics"][keys.index("mean_AP_Pleural Effusion")] == 0.0


def test_metrics_on_the_reference_predictions_of_c2():
    for tag, spec, case, fx in LU.load_cases("c2"):
        pred = LU.unpack_pred(fx, spec)
        for s in range(spec["S"]):
            check_metrics(pred[s], case["y_test"], LU.LABEL_NAMES, fx["metrics_keys"], fx["metrics"][s], (tag, s))


@pytest.mark.parametrize("name", ["c2", "small", "hard"])
def test_backend_fit_reaches_the_optimum(name):
    """torch_backend_lr.logreg_fit (the GPU tests' comparison partner) against w* of every fixture problem"""
    for tag, spec, case, fx in LU.load_cases(name):
        w, info = torch_backend_lr.logreg_fit(torch.from_numpy(case["x_train"]), torch.from_numpy(case["y_train"]))
        w = w.numpy()
        assert w.shape == fx["w_star"].shape and info.shape == (*w.shape[:2], 2)
        dist = np.linalg.norm(w - fx["w_star"], axis=2)
        assert dist.max() <= 1e-7 * np.linalg.norm(fx["w_star"], axis=2).max(), (tag, dist.max())
        assert LU.grad_inf(w, case["x_train"], case["y_train"]).max() <= 1e-9, tag
        pred = torch_backend_lr.logreg_predict(torch.from_numpy(case["x_test"]), torch.from_numpy(w)).numpy()
        assert np.array_equal(pred, (LU.decisions(fx["w_star"], case["x_test"]) > 0).astype(np.float32)) or name == "hard"


def test_fixture_band_cap():
    """the prediction comparison of the GPU tests leaves out at most 5 % of a problem's test rows"""
    for name in ("c2", "small"):
        for tag, spec, case, fx in LU.load_cases(name):
            dec = LU.decisions(fx["w_star"], case["x_test"])
            share = (np.abs(dec) <= 1.25 * fx["ref_gap"][:, None, :]).mean(axis=1)
            assert share.max() <= 0.05, (tag, share.max())


def test_get_random_labels_redraws(monkeypatch):
    from mimic_amd.evaluation.eval_metrics import representation as REP
    labels = np.zeros((40, 2), dtype=np.float32)
    labels[3, 0] = labels[7, 1] = 1.0
    draws = []
    real = np.random.randint

    def counting(*a, **kw):
        draws.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(np.random, "randint", counting)
    np.random.seed(0)
    got, idx = REP.get_random_labels(40, 10, labels)
    assert len(draws) > 1                              # 10 of 40 rows rarely hold both rare positives at once
    assert got.shape == (10, 2) and np.array_equal(got, labels[idx])
    assert all(len(np.unique(got[:, l])) == 2 for l in range(2))
    np.random.seed(0)
    draws.clear()
    got2, idx2 = REP.get_random_labels(40, 10, labels)
    assert np.array_equal(idx, idx2)                   # numpy's global generator, as set_random_seed seeds it


def test_get_random_labels_assertions():
    from mimic_amd.evaluation.eval_metrics import representation as REP
    with pytest.raises(AssertionError, match="at least two classes"):
        REP.get_random_labels(20, 5, np.ones((20, 3), dtype=np.float32))
    one_sided = np.zeros((20, 2), dtype=np.float32)
    one_sided[:, 0] = np.arange(20) % 2                # column 1 never has a positive: no sample can hold both classes
    with pytest.raises(AssertionError, match="Could not get sample containing both classes"):
        REP.get_random_labels(20, 5, one_sided, max_tries=7)


def tiny_exp(**kw):
    cfg = R.Cfg(img_size=64, class_dim=8, DIM_img=4, DIM_text=4, vocab_size=50, batch_size=4)
    exp = model_util.build_exp(cfg, R.init_state(cfg, seed=1), "cpu", "train_nodrop")
    f = exp.flags
    f.dataloader_workers, f.num_training_samples_lr = 0, 40
    f.__dict__.update(kw)
    return exp


class CountingInference:
    def __init__(self, monkeypatch, model):
        self.n, real = [], model.inference

        def counted(batch, *a, **kw):
            assert not model.training
            self.n.append(next(iter(batch.values())).shape[0])
            return real(batch, *a, **kw)

        monkeypatch.setattr(model, "inference", counted)


@pytest.mark.parametrize("steps, train_batches, test_batches", [(0, 5, 5), (2, 5, 3)])
def test_host_logic_on_the_tiny_model(monkeypatch, steps, train_batches, test_batches):
    """Mimic_testing with 5 batches of 30: the training side reads the whole split in either case (the early exit needs more
    than 150 batches); the test side scores all batches with steps_per_training_epoch 0 and three with a limit of 2"""
    torch_backend_lr.install(monkeypatch)
    exp = tiny_exp(testing_batches=5, steps_per_training_epoch=steps)
    count = CountingInference(monkeypatch, exp.mm_vae)
    RE.set_random_seed(3)
    fits = torch_backend_lr.CALLS["logreg_fit"]
    res = RE.evaluate_latent_representation(exp, 0)
    assert torch_backend_lr.CALLS["logreg_fit"] == fits + 1            # all 7 x 3 problems in one call
    assert count.n == [30] * (train_batches + test_batches)
    assert set(res) == SUBSETS and len(res) == 7
    for sub, d in res.items():
        assert list(d) == metric_keys(exp.labels), sub
        assert all(np.isfinite(float(v)) for v in d.values()), (sub, d)
        assert sum(d[f"gt_count_{n}"] for n in exp.labels) <= 30 * test_batches * 3
    assert len(exp.subsets) == 8 and "" in exp.subsets
    assert exp.flags.batch_size == 4 and exp.mm_vae.training


def test_binary_labels_fit_one_label(monkeypatch):
    torch_backend_lr.install(monkeypatch)
    cfg = R.Cfg(img_size=64, class_dim=8, DIM_img=4, DIM_text=4, vocab_size=50, batch_size=4)
    flags = default_flags(img_size=64, class_dim=8, DIM_img=4, DIM_text=4, vocab_size=50, batch_size=4, binary_labels=True,
                          device=torch.device("cpu"), testing_batches=3, num_training_samples_lr=30)
    from mimic_amd.utils.experiment import HotPathExperiment
    exp = HotPathExperiment(flags)
    exp.mm_vae.load_state_dict(R.init_state(cfg, seed=1))
    RE.set_random_seed(1)
    res = RE.evaluate_latent_representation(exp, 0)
    assert all(list(d) == metric_keys(["Finding"]) for d in res.values())


def test_state_comes_back_when_the_evaluation_raises(monkeypatch):
    torch_backend_lr.install(monkeypatch)
    from mimic_amd import ops
    exp = tiny_exp(testing_batches=2)

    def boom(*a, **kw):
        raise RuntimeError("boom")

    monkeypatch.setattr(ops, "logreg_fit", boom)
    for training in (True, False):
        exp.mm_vae.train(training)
        with pytest.raises(RuntimeError, match="boom"):
            RE.evaluate_latent_representation(exp, 0)
        assert exp.flags.batch_size == 4 and exp.mm_vae.training is training


def test_one_class_label_column_never_reaches_the_kernel(monkeypatch):
    torch_backend_lr.install(monkeypatch)
    from mimic_amd.evaluation.eval_metrics import representation as REP
    exp = tiny_exp()
    fits = torch_backend_lr.CALLS["logreg_fit"]
    labels = np.zeros((12, 3), dtype=np.float32)
    labels[::2, 0] = labels[::3, 1] = 1.0
    with pytest.raises(ValueError, match="Support Devices"):
        REP.train_clf_lr(exp, {"PA": torch.randn(12, 8)}, labels)
    assert torch_backend_lr.CALLS["logreg_fit"] == fits


def test_train_and_classify_shapes(monkeypatch):
    """train_clf_lr / classify_latent_representations with the reference's call shapes on a fixture problem: the backend's
    classifiers predict what the exact optimum predicts"""
    torch_backend_lr.install(monkeypatch)
    from mimic_amd.evaluation.eval_metrics import representation as REP
    (tag, spec, case, fx), = LU.load_cases("c2")
    exp = tiny_exp(dataset="mimic")
    keys = LU.SUBSET_KEYS
    clf = REP.train_clf_lr(exp, {k: torch.from_numpy(case["x_train"][s]) for s, k in enumerate(keys)}, case["y_train"])
    assert clf.subsets == keys and clf.labels == exp.labels and tuple(clf.W.shape) == (7, 3, 129)
    assert tuple(clf["Lung Opacity"]["PA_text"].shape) == (129,)
    out = REP.classify_latent_representations(exp, clf, {k: torch.from_numpy(case["x_test"][s]) for s, k in enumerate(keys)})
    assert list(out) == exp.labels and all(list(v) == keys for v in out.values())
    want = LU.decisions(fx["w_star"], case["x_test"]) > 0
    for l, name in enumerate(exp.labels):
        for s, k in enumerate(keys):
            assert np.array_equal(out[name][k].numpy() > 0.5, want[s, :, l])


def test_flags():
    f = MM.parse_flags([])
    assert f.eval_lr is False and f.num_training_samples_lr == 500
    f = MM.parse_flags(["--eval_lr", "true", "--num_training_samples_lr", "120"])
    assert f.eval_lr is True and f.num_training_samples_lr == 120
    d = default_flags(device=None)
    assert d.eval_lr is False and d.num_training_samples_lr == 500


def test_result_line():
    h = lambda e, **t: {"epoch": e, "train": {"graphed_steps": 3}, "test": {"total_loss": 1.5, **t}}
    assert MM.result_line([h(0), h(1)]) == {"epochs": 2, "last_test_loss": 1.5, "graphed_steps_last_epoch": 3}
    lr = {"PA": {"accuracy": 0.5}}
    line = MM.result_line([h(0, lr_eval=lr), h(1)])
    assert line["last_lr_eval"] == lr and "last_lhoods" not in line
    both = MM.result_line([h(0, lr_eval=lr, lhoods={"PA": {"joint": -1.0}})])
    assert list(both) == ["epochs", "last_test_loss", "graphed_steps_last_epoch", "last_lhoods", "last_lr_eval"]


def test_run_epochs_eval_lr_with_calc_nll(monkeypatch, tmp_path):
    """eval_freq 2, end_epoch 3: both hooks run after epochs 1 and 2 only, the representation evaluation first"""
    torch_backend_lr.install(monkeypatch)
    exp = tiny_exp(eval_lr=True, calc_nll=True, eval_freq=2, end_epoch=3, testing_batches=8,
                   dir_checkpoints=str(tmp_path / "ckpt"))
    order = []
    real_lr, real_nll = RE.evaluate_latent_representation, RE.estimate_test_likelihoods
    monkeypatch.setattr(RE, "evaluate_latent_representation", lambda e, ep: (order.append(("lr", ep)), real_lr(e, ep))[1])
    monkeypatch.setattr(RE, "estimate_test_likelihoods", lambda e, ep: (order.append(("nll", ep)), real_nll(e, ep))[1])
    history = RE.run_epochs("cpu", exp)
    assert ["lr_eval" in h["test"] for h in history] == [False, True, True]
    assert ["lhoods" in h["test"] for h in history] == [False, True, True]
    assert order == [("lr", 1), ("nll", 1), ("lr", 2), ("nll", 2)]
    for h in history[1:]:
        assert set(h["test"]["lr_eval"]) == SUBSETS
    assert exp.flags.batch_size == 4
    import json
    json.dumps(history)                                # the launcher writes the history as JSON
