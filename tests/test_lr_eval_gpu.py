"""Latent-representation evaluation (--eval_lr) on the GPU: csrc/logreg.hip against the exact optimum of every fixture
problem and against the reference's own predictions (tests/golden/g11_lr_*, tests/tools/gen_golden_lr.py), determinism,
info, refusals, the whole path at model level against tests/torch_backend_lr.py, and the launcher.

The bars of the fit come from the reference, not from the kernel: (a) |grad f(W)|_inf evaluated in float64 <= 1e-4 N is
lbfgs' own stopping rule (tol 1e-4 on the mean loss); (b) |W - w*|_2 <= ref_dist: at least as close to the optimum as the
reference's result is.  (c) is the tighter float32 expectation: the worst |W - w*|_2 / |w*|_2 measured over all fixture
problems is 5.1e-6 (g11_lr_hard; recorded per fixture in profiles/lr_eval_bench.json by tests/tools/lr_eval_bench.py),
asserted with a 4x margin."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lr_util as LU
import methods_util
import mopoe_ref as R
import torch_backend_lr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_BAR = 4 * 5.1e-6
SUBSETS = {"PA", "Lateral", "text", "Lateral_PA", "PA_text", "Lateral_text", "Lateral_PA_text"}


def fit(case):
    from mimic_amd import ops
    x, y = torch.from_numpy(case["x_train"]).cuda(), torch.from_numpy(case["y_train"]).cuda()
    w, info = ops.logreg_fit(x, y)
    return x, y, w, info


@pytest.mark.parametrize("name", ["c2", "small", "hard"])
def test_fit_against_the_optimum(name):
    for tag, spec, case, fx in LU.load_cases(name):
        _x, _y, w, info = fit(case)
        wn, inf = w.cpu().numpy().astype(np.float64), info.cpu().numpy()
        assert np.isfinite(wn).all(), tag
        gi = LU.grad_inf(wn, case["x_train"], case["y_train"])
        dist = np.linalg.norm(wn - fx["w_star"], axis=2)
        rel = dist / np.linalg.norm(fx["w_star"], axis=2)
        print(f"{tag}: |grad|_inf / N max {gi.max() / spec['N']:.3e} (bar 1e-4); |W - w*| / ref_dist max "
              f"{(dist / fx['ref_dist']).max():.3e} (bar 1); |W - w*| / |w*| max {rel.max():.3e} (bar {REL_BAR:.2e}); "
              f"Newton steps {inf[..., 0].min():.0f}..{inf[..., 0].max():.0f}")
        assert (gi <= 1e-4 * spec["N"]).all(), (tag, gi.max())                       # (a)
        assert (dist <= fx["ref_dist"]).all(), (tag, (dist / fx["ref_dist"]).max())    # (b)
        assert (rel <= REL_BAR).all(), (tag, rel.max())                              # (c)


@pytest.mark.parametrize("name", ["c2", "small"])
def test_predictions_against_the_reference(name):
    from mimic_amd import ops
    from mimic_amd.networks.classifiers.utils import Metrics
    for tag, spec, case, fx in LU.load_cases(name):
        _x, _y, w, _info = fit(case)
        xt = torch.from_numpy(case["x_test"]).cuda()
        pred, dec = ops.logreg_predict(xt, w, want_decision=True)
        pred_list = ops.logreg_predict(list(xt.unbind(0)), w)
        assert torch.equal(pred, pred_list)
        pred, dec = pred.cpu().numpy(), dec.cpu().numpy()
        assert np.array_equal(pred, (dec > 0).astype(np.float32))
        dec_star = LU.decisions(fx["w_star"], case["x_test"])
        outside = np.abs(dec_star) > 1.25 * fx["ref_gap"][:, None, :]             # [S, M, L]
        assert ((~outside).mean(axis=1) <= 0.05).all(), (tag, (~outside).mean(axis=1).max())
        ref = LU.unpack_pred(fx, spec)
        assert np.array_equal(pred[outside], ref[outside]), (tag, int((pred != ref)[outside].sum()))
        names = LU.LABEL_NAMES[:len(spec["kinds"])]
        keys = [str(k) for k in fx["metrics_keys"]]
        for s in range(spec["S"]):
            m = Metrics(pred[s], case["y_test"], names)
            acc = m.extract_values(m.evaluate())["accuracy"]
            left_out = int((~outside[s]).sum())
            assert abs(acc - fx["metrics"][s][keys.index("accuracy")]) <= left_out / (spec["M"] * len(names)) + 1e-12, (tag, s)


def test_fit_is_deterministic_and_reports_info():
    from mimic_amd import ops
    (tag, spec, case, fx), = LU.load_cases("c2")
    x, y, w, info = fit(case)
    w2, info2 = ops.logreg_fit(x, y)
    assert torch.equal(w, w2) and torch.equal(info, info2)
    inf = info.cpu().numpy()
    assert inf.shape == (7, 3, 2) and (inf[..., 0] >= 1).all() and (inf[..., 0] <= 100).all()
    # the reported gradient is the float32 gradient at the returned W: it agrees with the float64 one to float32 rounding
    gi = LU.grad_inf(w.cpu().numpy().astype(np.float64), case["x_train"], case["y_train"])
    assert np.abs(inf[..., 1] - gi).max() <= 1e-6 * spec["N"]
    tol = 1e-5
    w1, info1 = ops.logreg_fit(x, y, max_iter=1, tol=tol)
    inf1 = info1.cpu().numpy()
    assert np.isfinite(w1.cpu().numpy()).all() and (inf1[..., 0] == 1).all()
    assert (inf1[..., 1] > tol).all()                    # one Newton step from zero has not converged, and info says so
    w0, info0 = ops.logreg_fit(x, y, max_iter=0)
    assert (w0 == 0).all() and (info0[..., 0] == 0).all()


def test_refusals():
    from mimic_amd import ops
    from mimic_amd.evaluation.eval_metrics import representation as REP
    from types import SimpleNamespace
    dev = "cuda"
    with pytest.raises(ops.MopoeHipError):
        ops.logreg_fit(torch.zeros(1, 8, 257, device=dev), torch.zeros(8, 1, device=dev))
    with pytest.raises(ops.MopoeHipError):
        ops.logreg_fit(torch.zeros(1, 1, 8, device=dev), torch.zeros(1, 1, device=dev))
    with pytest.raises(ops.MopoeHipError):
        ops.logreg_fit(torch.zeros(1, 8, 4), torch.zeros(8, 1))
    with pytest.raises(ops.MopoeHipError):
        ops.logreg_fit(torch.zeros(1, 8, 4, device=dev), torch.zeros(7, 1, device=dev))
    with pytest.raises(ops.MopoeHipError):
        ops.logreg_predict(torch.zeros(2, 8, 4), torch.zeros(2, 1, 5))
    with pytest.raises(ops.MopoeHipError):
        ops.logreg_predict(torch.zeros(2, 8, 4, device=dev), torch.zeros(2, 1, 6, device=dev))
    with pytest.raises(ops.MopoeHipError):
        ops.logreg_predict(torch.zeros(3, 8, 4, device=dev), torch.zeros(2, 1, 5, device=dev))
    torch.cuda.synchronize()
    exp = SimpleNamespace(labels=["a", "b"], flags=SimpleNamespace(device=torch.device(dev), dataset="mimic"))
    labels = np.zeros((8, 2), dtype=np.float32)
    labels[::2, 0] = 1.0
    with pytest.raises(ValueError):
        REP.train_clf_lr(exp, {"PA": torch.randn(8, 4, device=dev)}, labels)


@pytest.mark.parametrize("method", ["joint_elbo", "moe"])
@pytest.mark.parametrize("compute_dtype", ["fp32", "bf16"])
def test_whole_path_at_model_level(monkeypatch, method, compute_dtype):
    """train_clf_lr_all_subsets + test_clf_lr_all_subsets on cuda; the float64 backend fits the SAME gathered latents"""
    from mimic_amd import ops
    from mimic_amd import run_epochs as RE
    from mimic_amd.evaluation.eval_metrics import representation as REP
    cfg = R.Cfg(img_size=64, class_dim=32, DIM_img=32, DIM_text=32, vocab_size=200, batch_size=8)
    exp = methods_util.build_exp(method, cfg, R.init_state(cfg, seed=4), "cuda", "train_nodrop", compute_dtype=compute_dtype)
    f = exp.flags
    f.testing_batches, f.num_training_samples_lr, f.dataloader_workers = 8, 200, 0
    fits, preds = [], []
    real_fit, real_predict = ops.logreg_fit, ops.logreg_predict

    def spy_fit(x, y, *a, **kw):
        out = real_fit(x, y, *a, **kw)
        fits.append((x, y, out[0]))
        return out

    def spy_predict(xs, w, *a, **kw):
        out = real_predict(xs, w, *a, **kw)
        preds.append((torch.stack([t.clone() for t in xs]), out))
        return out

    monkeypatch.setattr(ops, "logreg_fit", spy_fit)
    monkeypatch.setattr(ops, "logreg_predict", spy_predict)
    RE.set_random_seed(5)
    f.batch_size = REP.LR_BATCH_SIZE
    try:
        clf = REP.train_clf_lr_all_subsets(exp)
        res = REP.test_clf_lr_all_subsets(clf, exp)
    finally:
        f.batch_size = 8
    assert len(fits) == 1 and len(preds) == 8                 # ONE fit launch for the 21 problems; 8 test batches of 30
    assert exp.mm_vae.training and len(exp.subsets) == 8
    assert set(res) == SUBSETS and all(np.isfinite(float(v)) for d in res.values() for v in d.values())
    x, y, w = fits[0]
    assert tuple(x.shape) == (7, 200, 32) and tuple(y.shape) == (200, 3) and x.is_cuda
    xn, yn, wn = x.cpu().numpy(), y.cpu().numpy(), w.cpu().numpy().astype(np.float64)
    gi = LU.grad_inf(wn, xn, yn)
    assert (gi <= 1e-4 * 200).all(), gi.max()                                       # bar (a) on the path's own data
    wb, _ = torch_backend_lr.logreg_fit(x, y)
    wb = wb.cpu().numpy()
    wdiff = np.linalg.norm(wn - wb, axis=2)                                          # [S, L]
    xt = torch.cat([p[0] for p in preds], 1).cpu().numpy().astype(np.float64)        # [S, 240, D]
    got = torch.cat([p[1] for p in preds], 1).cpu().numpy()
    dec = LU.decisions(wb, xt)
    mag = np.einsum("smd,sld->sml", np.abs(xt), np.abs(wb[:, :, :-1])) + np.abs(wb[:, None, :, -1])
    blur = (32 + 1) * 2.0 ** -23 * mag + np.linalg.norm(xt, axis=2)[:, :, None] * wdiff[:, None, :]
    clear = np.abs(dec) > blur
    print(f"{method} {compute_dtype}: |grad|_inf/N max {gi.max() / 200:.3e}; |W - W_backend| max {wdiff.max():.3e}; "
          f"rows inside the float32 blur {(~clear).mean():.4f}")
    assert ((~clear).mean(axis=1) <= 0.05).all()
    assert np.array_equal(got[clear], (dec > 0).astype(np.float32)[clear])


def test_fit_is_one_launch_and_nothing_crosses_to_the_host(monkeypatch):
    """structure: between the first inference() and the end of the fit the only device->host copies are label matrices,
    and the fit of all problems is one call of the C entry point (one kernel launch, csrc/logreg.hip)"""
    from mimic_amd import ops
    from mimic_amd.evaluation.eval_metrics import representation as REP
    cfg = R.Cfg(img_size=64, class_dim=32, DIM_img=32, DIM_text=32, vocab_size=200, batch_size=8)
    exp = methods_util.build_exp("joint_elbo", cfg, R.init_state(cfg, seed=4), "cuda", "eval")
    f = exp.flags
    f.testing_batches, f.num_training_samples_lr, f.dataloader_workers, f.batch_size = 4, 100, 0, REP.LR_BATCH_SIZE
    copies, launches = [], []
    real_fit = ops.lib().mopoe_logreg_fit
    real = {name: getattr(torch.Tensor, name) for name in ("cpu", "to", "item", "tolist")}

    def spy(name):
        def wrapped(self, *a, **kw):
            out = real[name](self, *a, **kw)
            if self.is_cuda and not (isinstance(out, torch.Tensor) and out.is_cuda):
                copies.append(tuple(self.shape))
            return out
        return wrapped

    class Lib:
        def __getattr__(self, name):
            if name == "mopoe_logreg_fit":
                return lambda *a: (launches.append(1), real_fit(*a))[1]
            return getattr(ops._lib, name)

    for name in real:
        monkeypatch.setattr(torch.Tensor, name, spy(name))
    monkeypatch.setattr(ops, "lib", lambda: Lib())
    clf = REP.train_clf_lr_all_subsets(exp)
    monkeypatch.undo()
    assert launches == [1]
    assert all(len(shape) == 2 and shape[1] == 3 for shape in copies), copies     # label matrices only
    assert clf.W.is_cuda and tuple(clf.W.shape) == (7, 3, 33)


def test_real_split_is_evaluated_from_hbm(tmp_path, monkeypatch):
    """dataset != 'testing' on a GPU: both splits are read through DeviceResidentMimic (uploaded once, kept between
    evaluations); what crosses to the host is label matrices and, once, the prediction matrix"""
    from golden_util import make_mimic_files
    from mimic_amd import main_mimic as MM
    from mimic_amd import run_epochs as RE
    from mimic_amd.dataio.MimicDataset import DeviceResidentMimic
    from mimic_amd.utils.experiment import HotPathExperiment
    data = tmp_path / "data"
    make_mimic_files(str(data), img_size=64, n_train=100, n_eval=30, seed=5)
    flags = MM.parse_flags(["--dataset", "mimic", "--dir_data", str(data), "--img_size", "64", "--class_dim", "32",
                            "--DIM_img", "64", "--DIM_text", "32", "--batch_size", "8", "--len_sequence", "128",
                            "--num_training_samples_lr", "50"])
    flags.device = torch.device("cuda")
    exp = HotPathExperiment(flags)
    exp.mm_vae.to(flags.device)
    RE.set_random_seed(2)
    first = RE.evaluate_latent_representation(exp, 0)
    residents = dict(exp._lr_resident)
    assert len(residents) == 2 and all(isinstance(v, DeviceResidentMimic) for v in residents.values())
    copies = []
    real = {name: getattr(torch.Tensor, name) for name in ("cpu", "to", "item", "tolist")}

    def spy(name):
        def wrapped(self, *a, **kw):
            out = real[name](self, *a, **kw)
            if self.is_cuda and not (isinstance(out, torch.Tensor) and out.is_cuda):
                copies.append(tuple(self.shape))
            return out
        return wrapped

    for name in real:
        monkeypatch.setattr(torch.Tensor, name, spy(name))
    RE.set_random_seed(2)
    second = RE.evaluate_latent_representation(exp, 1)
    monkeypatch.undo()
    assert exp._lr_resident == residents                      # no second upload of the splits
    n_test = len(exp.dataset_test)
    assert all((len(c) == 2 and c[1] == 3) or c == (7, n_test, 3) for c in copies), copies
    assert [c for c in copies if len(c) == 3] == [(7, n_test, 3)]
    assert set(first) == SUBSETS and first == second          # same seed, same sample, deterministic fit
    assert all(np.isfinite(float(v)) for d in first.values() for v in d.values())
    assert exp.flags.batch_size == 8


def test_eval_lr_through_the_launcher(tmp_path):
    """python -m mimic_amd.main_mimic --eval_lr true on the synthetic split: last_lr_eval in the result line, and the
    captured train step keeps replaying after the evaluation (graphed_steps_last_epoch as without the flag)"""
    env = dict(os.environ)
    env["PYTHONPATH"] = os.path.join(REPO, "mopoe-mimic_amd") + os.pathsep + env.get("PYTHONPATH", "")
    lines = {}
    for flag in ("false", "true"):
        cmd = [sys.executable, "-m", "mimic_amd.main_mimic", "--img_size", "64", "--class_dim", "64", "--DIM_img", "64",
               "--batch_size", "8", "--end_epoch", "2", "--eval_freq", "1", "--testing_batches", "12",
               "--initial_learning_rate", "1e-5", "--num_training_samples_lr", "60", "--eval_lr", flag,
               "--dir_experiment_run", str(tmp_path / f"run_{flag}")]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines[flag] = json.loads(out.stdout.strip().splitlines()[-1])
    assert "last_lr_eval" not in lines["false"]
    lr = lines["true"]["last_lr_eval"]
    assert set(lr) == SUBSETS
    assert all(np.isfinite(float(v)) for d in lr.values() for v in d.values())
    assert lines["true"]["graphed_steps_last_epoch"] == lines["false"]["graphed_steps_last_epoch"] == 12
