"""Latent-representation evaluation (--eval_lr): the reference's mimic/evaluation/eval_metrics/representation.py
(train_clf_lr_all_subsets :20-69, get_random_labels :72-88, test_clf_lr_all_subsets :91-145,
classify_latent_representations :147-166, train_clf_lr :169-187) with the reference's names and call shapes.

A logistic-regression classifier per label and per non-empty modality subset is fitted on the subset posteriors' means of
flags.num_training_samples_lr training rows and scored on the test split.  What the reference does with 21 scikit-learn
fits on the host happens on the device: the means are appended into a device buffer as inference() produces them, the
sampled rows are gathered by index there, ops.logreg_fit solves all subsets x labels problems in one launch
(csrc/logreg.hip: the exact optimum of the problem LogisticRegression's defaults pose), ops.logreg_predict classifies a
batch's seven subset means in one launch.  Only the label matrix (the resampling loop of get_random_labels runs on the
host, on numpy's global generator as in the reference) and the final prediction matrix cross to the host.

Kept from the reference: the loop bounds (training side: the early exit needs `it > training_steps`, two classes in some
label column and `it > 150`; test side: `iteration > training_steps` with training_steps = flags.steps_per_training_epoch,
so a limit of 2 scores three batches), sampling with replacement, np.nan_to_num of the training data on the synthetic
dataset, Metrics with its swapped average-precision arguments.  Deliberately different: exp.subsets is
not mutated; on dataset == 'testing' the test-side latents get the same nan_to_num; scikit-learn is not imported.
"""
from __future__ import annotations

import typing

import numpy as np
import torch

from ... import ops
from ...networks.classifiers.utils import Metrics

LR_BATCH_SIZE = 30      # run_epochs.test sets flags.batch_size = 30 before the evaluation (mimic/run_epochs.py:186-188)
C_DEFAULT = 1.0         # LogisticRegression's default inverse regularisation strength


class LatentClassifiers:
    """what the reference's {label: {subset: LogisticRegression}} holds, on the device: W [S, L, D+1] (coefficients, then
    intercept) for `subsets` x `labels`; info [S, L, 2] = (Newton steps, |grad f|_inf) as the fit left it"""

    def __init__(self, subsets, labels, w, info):
        self.subsets, self.labels, self.W, self.info = list(subsets), list(labels), w, info

    def __getitem__(self, label):
        """clf_lr[label][subset] -> that classifier's [D+1] weights (the reference's indexing order)"""
        l = self.labels.index(label)
        return {s_key: self.W[s, l] for s, s_key in enumerate(self.subsets)}


def _subset_keys(exp):
    return [k for k in exp.subsets if k != ""]


def _loader(exp, dataset, shuffle: bool):
    """batches of 30 as ((dict of tensors), labels): a real split on a GPU through DeviceResidentMimic as in run_epochs (the
    split stays in HBM between evaluations), the synthetic split through its DataLoader"""
    from torch.utils.data import DataLoader
    from ...dataio.MimicDataset import DeviceResidentMimic, Mimic
    flags = exp.flags
    if (isinstance(dataset, Mimic) and flags.device.type == "cuda" and getattr(flags, "device_resident_data", True)):
        cache = exp.__dict__.setdefault("_lr_resident", {})
        key = (id(dataset), shuffle)
        if key not in cache:
            cache[key] = DeviceResidentMimic(dataset, flags.device, flags.batch_size, shuffle, 0, 1, flags.seed)
        cache[key].batch_size = int(flags.batch_size)
        return cache[key]
    if shuffle:
        from ...dataio.utils import get_data_loaders
        single = dict(vars(flags), distributed=False)      # every rank evaluates the whole split on its own device
        return get_data_loaders(type(flags)(**single), dataset, which_set="train")[1]
    return DataLoader(dataset, batch_size=flags.batch_size, shuffle=False,
                      num_workers=int(getattr(flags, "dataloader_workers", 0)), drop_last=False)


def _inference(exp, batch_d):
    batch_d = {k: v.to(exp.flags.device, non_blocking=True) for k, v in batch_d.items()}
    return exp.mm_vae.inference(batch_d)["subsets"]


def _two_classes(col) -> bool:
    return len(np.unique(col)) > 1


def train_clf_lr_all_subsets(exp, weighted_sampler: bool = False) -> LatentClassifiers:
    """Encodes the training split (eval mode) and fits the classifiers on a random sample of its rows."""
    if weighted_sampler:
        raise NotImplementedError("label-weighted sampling is outside the hot path")
    flags, model = exp.flags, exp.mm_vae
    subsets = _subset_keys(exp)
    n_train_samples = int(flags.num_training_samples_lr)
    was_training = model.training
    model.eval()
    try:
        loader = _loader(exp, exp.dataset_train, shuffle=True)
        training_steps = flags.steps_per_training_epoch if flags.steps_per_training_epoch > 0 else len(loader)
        rows_max = len(loader) * int(flags.batch_size)
        buf, n_rows, labels = None, 0, []
        with torch.no_grad():
            for it, (batch_d, batch_l) in enumerate(loader):
                if it > training_steps and it > 150:
                    # (labels seen so far: a small copy, and only once the reference's early exit is in reach)
                    seen = torch.cat(labels, 0).cpu().numpy()
                    if any(_two_classes(seen[:, l]) for l in range(seen.shape[-1])):
                        break
                lr_subsets = _inference(exp, batch_d)
                b = batch_l.shape[0]
                if buf is None:
                    d = lr_subsets[subsets[0]][0].shape[1]
                    buf = torch.empty(len(subsets), rows_max, d, dtype=torch.float32, device=flags.device)
                for s, key in enumerate(subsets):
                    buf[s, n_rows:n_rows + b].copy_(lr_subsets[key][0])
                labels.append(batch_l)
                n_rows += b
        all_labels = torch.cat([t.to("cpu") for t in labels], 0).numpy()
        sampled, rand_ind_train = get_random_labels(n_rows, n_train_samples, all_labels)
        index = torch.from_numpy(np.asarray(rand_ind_train, dtype=np.int64)).to(flags.device)
        data_train = buf[:, :n_rows].index_select(1, index)           # [S, n_train_samples, D], on the device
        return train_clf_lr(exp, {key: data_train[s] for s, key in enumerate(subsets)}, sampled)
    finally:
        model.train(was_training)


def get_random_labels(n_samples, n_train_samples, all_labels, max_tries=1000):
    """The classifiers need both classes of every label: row indices are drawn with replacement (numpy's global generator,
    which set_random_seed seeds) until every label column of the sample holds two classes."""
    all_labels = np.asarray(all_labels)
    assert any(_two_classes(all_labels[:, l]) for l in range(all_labels.shape[-1])), \
        'The labels must contain at least two classes to train the classifier'
    rand_ind_train = np.random.randint(n_samples, size=n_train_samples)
    labels = all_labels[rand_ind_train, :]
    tries = 1
    while any(not _two_classes(labels[:, l]) for l in range(labels.shape[-1])):
        rand_ind_train = np.random.randint(n_samples, size=n_train_samples)
        labels = all_labels[rand_ind_train, :]
        tries += 1
        assert max_tries >= tries, f'Could not get sample containing both classes to train ' \
                                   f'the classifier in {tries} tries. Might need to increase batch_size'
    return labels, rand_ind_train


def _stack(exp, data, subsets):
    x = data if isinstance(data, torch.Tensor) else torch.stack([torch.as_tensor(data[k]) for k in subsets])
    x = x.to(exp.flags.device, torch.float32)
    if exp.flags.dataset == "testing":
        # the synthetic dataset's latents may hold NaNs (the reference replaces them on the training side, :180-182)
        x = torch.nan_to_num(x)
    return x.contiguous()


def train_clf_lr(exp, data, labels, max_iter: int = 100, tol: float = 1e-5) -> LatentClassifiers:
    """data: {subset: [n, D] tensor}; labels: [n, len(exp.labels)] -> the fitted classifiers of every subset and label"""
    subsets = list(data.keys())
    labels = np.reshape(np.asarray(labels, dtype=np.float32), (np.shape(labels)[0], len(exp.labels)))
    for l, label_str in enumerate(exp.labels):
        if not _two_classes(labels[:, l] > 0.5):
            raise ValueError(f"label '{label_str}' holds a single class in the training sample: a logistic regression "
                             "with a free intercept has no optimum there")
    x = _stack(exp, data, subsets)
    y = torch.from_numpy(labels).to(exp.flags.device)
    w, info = ops.logreg_fit(x, y, C_DEFAULT, max_iter, tol)
    return LatentClassifiers(subsets, exp.labels, w, info)


def _predict(exp, clf_lr: LatentClassifiers, data) -> torch.Tensor:
    """-> predictions [S, M, L] on the device (1.0 where the decision value is > 0)"""
    if exp.flags.dataset == "testing":
        xs = list(_stack(exp, data, clf_lr.subsets).unbind(0))
    else:
        xs = [data[k].to(exp.flags.device, torch.float32).contiguous() for k in clf_lr.subsets]
    return ops.logreg_predict(xs, clf_lr.W)


def classify_latent_representations(exp, clf_lr: LatentClassifiers, data) -> typing.Mapping[str, typing.Mapping[str, torch.Tensor]]:
    """{label: {subset: predictions [M]}} as the reference, the arrays being device tensors (views of one [S, M, L] result)"""
    pred = _predict(exp, clf_lr, data)
    return {label: {key: pred[s, :, l] for s, key in enumerate(clf_lr.subsets)} for l, label in enumerate(clf_lr.labels)}


def test_clf_lr_all_subsets(clf_lr: LatentClassifiers, exp):
    """Scores the classifiers on the test split -> {subset: {metric: value}}"""
    flags, model = exp.flags, exp.mm_vae
    was_training = model.training
    model.eval()
    try:
        loader = _loader(exp, exp.dataset_test, shuffle=False)
        training_steps = flags.steps_per_training_epoch if flags.steps_per_training_epoch > 0 else len(loader)
        preds, labels = [], []
        with torch.no_grad():
            for iteration, (batch_d, batch_l) in enumerate(loader):
                if iteration > training_steps:
                    break
                labels.append(batch_l)
                lr_subsets = _inference(exp, batch_d)
                preds.append(_predict(exp, clf_lr, {key: lr_subsets[key][0] for key in clf_lr.subsets}))
        predictions = torch.cat(preds, 1).cpu().numpy()            # [S, rows, L]: the one copy of results to the host
        batch_labels = torch.cat([t.to("cpu") for t in labels], 0).numpy()
        results = {}
        for s, subset in enumerate(clf_lr.subsets):
            metrics = Metrics(predictions[s], batch_labels, str_labels=exp.labels)
            results[subset] = metrics.extract_values(metrics.evaluate())
        return results
    finally:
        model.train(was_training)


test_clf_lr_all_subsets.__test__ = False      # (the reference's name; not a pytest test)
