"""`Metrics` under the reference's import path (mimic/networks/classifiers/utils.py:286-413): the scores the
latent-representation evaluation reports per modality subset, same keys in the same order.  Restated on integer counts in
numpy; scikit-learn is not imported (average precision is written out below).  The MIMIC label classifiers that live in the
reference's module are out of scope."""
from __future__ import annotations

import typing

import numpy as np


def _to_numpy(t) -> np.ndarray:
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def average_precision_score(y_true, y_score) -> float:
    """sklearn.metrics.average_precision_score for binary y_true: AP = sum_k (R_k - R_{k-1}) P_k over the thresholds at the
    distinct score values, highest first; 0.0 when y_true holds no positive (scikit-learn 1.7.2's answer)."""
    y_true = _to_numpy(y_true).ravel() > 0.5
    y_score = _to_numpy(y_score).ravel()
    n_pos = int(y_true.sum())
    if n_pos == 0 or y_true.size == 0:
        return 0.0
    order = np.argsort(-y_score, kind="mergesort")
    y_true, y_score = y_true[order], y_score[order]
    last_of_value = np.r_[np.nonzero(np.diff(y_score))[0], y_true.size - 1]
    tps = np.cumsum(y_true)[last_of_value].astype(np.float64)
    precision = tps / (last_of_value + 1.0)
    recall = tps / n_pos
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


class Metrics(object):
    """Metrics(prediction [M, L], groundtruth [M, L], str_labels).evaluate() -> {metric: [value]}; extract_values unwraps."""

    def __init__(self, prediction, groundtruth, str_labels):
        self.str_labels = list(str_labels)
        self.prediction = _to_numpy(prediction)
        self.groundtruth = _to_numpy(groundtruth)
        self.prediction_bin = (self.prediction > 0.5).astype(np.int64)
        self.groundtruth_bin = (self.groundtruth > 0.5).astype(np.int64)
        self.class_pred_bin = {name: self.prediction_bin[:, i] for i, name in enumerate(self.str_labels)}
        self.class_gt_bin = {name: self.groundtruth_bin[:, i] for i, name in enumerate(self.str_labels)}

    def _confusion(self):
        p, g = self.prediction_bin, self.groundtruth_bin
        self.TP = self.INTER = int((p * g).sum())
        self.TN = self.INTER_NEG = int(((1 - p) * (1 - g)).sum())
        self.FP = int((p * (1 - g)).sum())
        self.FN = int(((1 - p) * g).sum())
        self.TOTAL = int(p.size)

    def evaluate(self) -> typing.Dict[str, list]:
        """accuracy, recall, specificity, precision, f1, jaccard, dice over all M * L entries (the reference's 1e-6 terms in
        the denominators; f1 is built from the rounded-off recall and precision, dice from the counts), then mean_AP_<label>,
        mean_AP_total, pred_count_<label>, gt_count_<label>"""
        self._confusion()
        tp, tn, fp, fn = float(self.TP), float(self.TN), float(self.FP), float(self.FN)
        self.RC = tp / ((tp + fn) + 1e-6)
        self.SP = tn / ((tn + fp) + 1e-6)
        self.PC = tp / ((tp + fp) + 1e-6)
        out = {"accuracy": [(tp + tn) / float(self.TOTAL)],
               "recall": [self.RC],
               "specificity": [self.SP],
               "precision": [self.PC],
               "f1": [2 * (self.RC * self.PC) / (self.RC + self.PC + 1e-6)],
               "jaccard": [tp / ((tp + fp + fn) + 1e-6)],
               "dice": [2 * tp / ((2 * tp + fp + fn) + 1e-6)]}
        out.update(self.mean_AP())
        out.update(self.counts())
        return out

    def extract_values(self, results: dict):
        return {k: v[0] for k, v in results.items()}

    def mean_AP(self) -> dict:
        """The reference calls average_precision_score(prediction, groundtruth): the PREDICTIONS take the place of y_true and
        the labels that of the score (mimic/networks/classifiers/utils.py:400-405).  Kept: its result tables hold this number."""
        ap = {f"mean_AP_{name}": [average_precision_score(self.prediction[:, i], self.groundtruth[:, i])]
              for i, name in enumerate(self.str_labels)}
        ap["mean_AP_total"] = [average_precision_score(self.prediction.ravel(), self.groundtruth.ravel())]
        return ap

    def counts(self) -> dict:
        pred = {f"pred_count_{name}": [int(self.class_pred_bin[name].sum())] for name in self.str_labels}
        gt = {f"gt_count_{name}": [int(self.class_gt_bin[name].sum())] for name in self.str_labels}
        return {**pred, **gt}
