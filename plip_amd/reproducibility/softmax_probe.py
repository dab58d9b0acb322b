"""Softmax linear probe on the GPU: the CLIP paper's linear-probe protocol (``LogisticRegression(C=0.316, max_iter=1000)``, multinomial,
L-BFGS) and, equally, the reference's fine-tuning head with the tower frozen (``LinearClassifier`` + ``nn.CrossEntropyLoss()``,
reproducibility/fine_tuning/finetune.py).

``SoftmaxProber`` has ``LinearProber``'s ``train_and_test`` signature and return value (macro metrics) and minimises ONE softmax over all
classes instead of K one-vs-rest sigmoids (``plip_amd.softmax_probe.softmax_fit``, csrc/probe_softmax.hip): a full-batch L-BFGS solve,
converged and deterministic -- ``seed`` has no effect.  Give scikit-learn's ``C`` (default: the CLIP protocol's 0.316) or ``alpha = 1 /
(C N)``, not both.  With three or more classes the fitted point is ``LogisticRegression(C, class_weight)``'s; with two classes ``coef_``
stays [2, D], and ``coef_[1] - coef_[0]`` / ``intercept_[1] - intercept_[0]`` are ``LogisticRegression(C=2 C)``'s binary solution (the
two-row softmax is the binary problem at half the penalty).  Intercepts are determined up to a common constant: compare ``b - b.mean()``.
"""
from __future__ import annotations

import logging
from typing import Optional

import numpy as np
import torch

from ..engine import Engine, heads_engine
from ..softmax_probe import DEFAULT_GTOL, softmax_fit
from .linear_probe import ProbeClassifier, _encode
from .metrics import eval_metrics


class SoftmaxClassifier(ProbeClassifier):
    """``ProbeClassifier`` with ``coef_`` [C, D] for every C >= 2, plus ``predict_proba``: the softmax of the decision values."""

    def predict_proba(self, x) -> np.ndarray:
        _, dec = self._engine.probe_predict(x, self._coef, self._intercept, return_decision=True)
        z = dec.cpu().numpy().astype(np.float64)
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)


class SoftmaxProber:
    def __init__(self, alpha: Optional[float] = None, C: Optional[float] = 0.316, class_weight: Optional[str] = None, seed=7,
                 engine: Optional[Engine] = None, max_iter: int = 1000, gtol: float = DEFAULT_GTOL):
        if alpha is not None and C == 0.316:
            C = None                # alpha takes the place of the DEFAULT C; any other C beside an alpha is refused below
        if (alpha is None) == (C is None):
            raise ValueError("give exactly one of alpha and C")
        if class_weight not in ("balanced", None):
            raise ValueError("class_weight must be 'balanced' or None")
        self.alpha, self.C, self.class_weight = alpha, C, class_weight
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
            xtr = eng._probe_x(train_x if torch.is_tensor(train_x) else np.asarray(train_x, dtype=np.float32), "SoftmaxProber")
        coef, intercept, info = softmax_fit(eng, xtr, ytr, len(classes), alpha=self.alpha, C=self.C, class_weight=self.class_weight,
                                            max_iter=self.max_iter, gtol=self.gtol)
        classifier = SoftmaxClassifier(eng, coef, intercept, classes, info)
        test_pred = classifier.predict_index(test_x if torch.is_tensor(test_x) else np.asarray(test_x, dtype=np.float32))
        train_pred = classifier.predict_index(xtr)
        test_metrics = eval_metrics(yte, test_pred, average_method="macro")
        train_metrics = eval_metrics(ytr, train_pred, average_method="macro")
        test_metrics["split"] = "test"
        train_metrics["split"] = "train"
        logging.info("SoftmaxProber Done")
        return classifier, (test_metrics, train_metrics)
