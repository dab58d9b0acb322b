"""Linear-probe evaluation head on the GPU (reproducibility/evaluation/linear_probing/linear_classifier.py).

The reference fits ``SGDClassifier(loss="log_loss", penalty="l2", alpha, class_weight="balanced", max_iter=10000)``: one-vs-rest
sequential SGD on one CPU core, stopped when the epoch loss has not improved by 1e-3 for five epochs.  ``LinearProber`` here minimises
the SAME objective, with the same class weights and the same prediction rule, by a full-batch L-BFGS solve whose loss-and-gradient
pass is one fused HIP kernel over the cached embeddings (``Engine.probe_fit``, csrc/probe.hip) -- converged instead of
early-stopped, deterministic, and ``seed`` has no effect (INTEGRATION.md lists this with the heads' other deviations).  Labels of
any sortable kind are encoded as ``LabelEncoder`` does (sorted unique values); predictions come back as [N] int32 from the GPU.
"""
from __future__ import annotations

import logging
from typing import Optional

import numpy as np
import torch

from ..engine import Engine, heads_engine
from .metrics import eval_metrics


def _encode(classes: np.ndarray, labels, what: str) -> np.ndarray:
    """``LabelEncoder.transform``: index of every label in the sorted ``classes``; ValueError on one that was not fitted."""
    arr = np.asarray(labels)
    idx = np.searchsorted(classes, arr)
    idx = np.clip(idx, 0, len(classes) - 1)
    bad = classes[idx] != arr
    if bad.any():
        raise ValueError(f"{what} contains previously unseen labels: {sorted(set(np.asarray(arr)[bad].tolist()))!r}")
    return idx.astype(np.int64)


class ProbeClassifier:
    """What ``train_and_test`` returns in place of the fitted ``SGDClassifier``: ``coef_`` [K, D] (``[1, D]`` for two classes),
    ``intercept_`` [K], ``classes_``, ``n_iter_``, ``predict`` and ``decision_function`` with scikit-learn's shapes."""

    def __init__(self, engine: Engine, coef: torch.Tensor, intercept: torch.Tensor, classes: np.ndarray, info: dict):
        self._engine = engine
        self._coef, self._intercept = coef, intercept
        self.coef_ = coef.cpu().numpy().astype(np.float64)
        self.intercept_ = intercept.cpu().numpy().astype(np.float64)
        self.classes_ = classes
        self.n_iter_ = int(info["iterations"])
        self.info_ = info

    def predict_index(self, x) -> np.ndarray:
        return self._engine.probe_predict(x, self._coef, self._intercept).cpu().numpy().astype(np.int64)

    def predict(self, x) -> np.ndarray:
        return self.classes_[self.predict_index(x)]

    def decision_function(self, x) -> np.ndarray:
        _, dec = self._engine.probe_predict(x, self._coef, self._intercept, return_decision=True)
        dec = dec.cpu().numpy()
        return dec[:, 0] if dec.shape[1] == 1 else dec


class LinearProber:
    def __init__(self, alpha, seed=7, engine: Optional[Engine] = None, max_iter: int = 1000, gtol: float = 2e-8):
        self.alpha = alpha
        self.seed = seed            # kept for the reference's signature: the solver is deterministic
        self._engine = engine
        self.max_iter, self.gtol = max_iter, gtol

    def train_and_test(self, train_x, train_y, test_x, test_y):
        eng = self._engine or heads_engine()
        classes = np.unique(np.asarray(train_y))                    # LabelEncoder.fit: sorted unique labels
        if len(classes) < 2:
            raise ValueError("the probe needs at least two classes in train_y")
        ytr = _encode(classes, train_y, "train_y")
        yte = _encode(classes, test_y, "test_y")
        if len(ytr) != len(train_x) or len(yte) != len(test_x):
            raise ValueError("embeddings and labels differ in length")
        with torch.cuda.device(eng.device):
            xtr = eng._probe_x(train_x if torch.is_tensor(train_x) else np.asarray(train_x, dtype=np.float32), "LinearProber")
        coef, intercept, info = eng.probe_fit(xtr, ytr, len(classes), float(self.alpha), class_weight="balanced",
                                              max_iter=self.max_iter, gtol=self.gtol)
        classifier = ProbeClassifier(eng, coef, intercept, classes, info)
        test_pred = classifier.predict_index(test_x if torch.is_tensor(test_x) else np.asarray(test_x, dtype=np.float32))
        train_pred = classifier.predict_index(xtr)
        test_metrics = eval_metrics(yte, test_pred, average_method="macro")
        train_metrics = eval_metrics(ytr, train_pred, average_method="macro")
        test_metrics["split"] = "test"
        train_metrics["split"] = "train"
        logging.info("LinearProber Done")
        return classifier, (test_metrics, train_metrics)
