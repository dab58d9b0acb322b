"""Softmax (multinomial) linear probe on cached embeddings: one softmax over all classes, the objective of the CLIP paper's linear-probe
protocol (``LogisticRegression(C=0.316, max_iter=1000)``) and of a cross-entropy head on a frozen tower (include/plipmi.h
plipmi_softmax_fit; csrc/probe_softmax.hip).  A function on an engine, not a method of it: ``softmax_fit(engine, x, y, n_classes, C=0.316)``;
``plip_amd.reproducibility.SoftmaxProber`` routes here.  Predictions and decision values are ``Engine.probe_predict`` on the returned
``coef`` / ``intercept``.  Runs on the given engine alone and keeps no state.

    f(W, b) = (1/N) sum_i cw[y_i] (logsumexp_k(x_i.w_k + b_k) - (x_i.w_{y_i} + b_{y_i})) + alpha/2 |W|_F^2,    alpha = 1 / (C N)

* Three or more classes: the minimiser is ``LogisticRegression(C=1/(alpha N), class_weight=...)``'s (coef_ within 1.1e-7, centred
  intercepts within 1.7e-7 in float64 on the ``ragged3`` fixture: scikit-learn's own stopping floor).
* The optimum is not unique in b: a constant added to every intercept changes nothing.  The gradient with respect to b sums to zero, so
  the fit from zeros stays on sum(b) = 0 up to rounding; compare ``b - b.mean()``.  The columns of the optimal W sum to zero.
* Two classes: still two rows (``coef`` is [2, D]).  ``W[1] - W[0]`` and ``b[1] - b[0]`` equal ``LogisticRegression(C=2/(alpha N))``'s
  binary ``coef_`` / ``intercept_``: the two-row softmax is scikit-learn's binary problem at HALF the penalty.
"""
from __future__ import annotations

import ctypes as C_
import math
import warnings
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import _ptr

DEFAULT_GTOL = 2e-8      # LinearProber's: above the measured gradient noise of the kernel at the fixtures' optima (profiles/softmax_probe_parity.txt)


def softmax_fit(engine, x, y, n_classes: int, alpha: Optional[float] = None, C: Optional[float] = None,
                class_weight: Optional[str] = None, max_iter: int = 1000, gtol: float = DEFAULT_GTOL, coef_init=None,
                intercept_init=None):
    """Minimise f on embeddings ``x`` [N, D] with integer labels ``y`` in [0, n_classes): a full-batch L-BFGS solve inside libplipmi.so,
    converged to ``|grad f|_inf <= gtol``, deterministic (no seed).  Exactly one of ``alpha`` (the penalty's weight) and ``C``
    (scikit-learn's inverse strength, ``alpha = 1 / (C N)``) is given.  ``x`` / ``y`` may be host numpy arrays or torch tensors on either
    side.  Returns ``(coef [n_classes, D], intercept [n_classes], info)`` as device tensors; ``info`` = dict(iterations, evaluations,
    converged (bool), grad_norm, loss (float), alpha).  A fit that stops at ``max_iter`` is reported through ``info["converged"]`` and a
    RuntimeWarning, not raised."""
    K = int(n_classes)
    if K < 2:
        raise ValueError("the probe needs at least two classes")
    if K > _lib.PROBE_MAX_K:
        raise ValueError(f"at most {_lib.PROBE_MAX_K} classes, got {K}")
    if (alpha is None) == (C is None):
        raise ValueError("give exactly one of alpha and C")
    if class_weight not in ("balanced", None):
        raise ValueError("class_weight must be 'balanced' or None")
    if int(max_iter) < 1 or not (math.isfinite(gtol) and gtol > 0):
        raise ValueError("need max_iter >= 1 and a finite gtol > 0")
    n_rows, width = engine._probe_shape(x, "softmax_fit")
    if alpha is None:
        if not (math.isfinite(C) and C > 0):
            raise ValueError(f"C must be finite and > 0, got {C}")
        alpha = 1.0 / (float(C) * n_rows)
    if not (math.isfinite(alpha) and alpha > 0):
        raise ValueError(f"alpha must be finite and > 0, got {alpha}")
    if not (torch.is_tensor(x) and x.device == engine.device):
        engine._probe_fits(n_rows, width, "softmax_fit", " (chunked fitting is not provided)")
    yh = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
    if yh.ndim != 1 or yh.shape[0] != n_rows:
        raise ValueError(f"y must be [N = {n_rows}], got {tuple(yh.shape)}")
    if not np.issubdtype(yh.dtype, np.integer):
        raise ValueError("y must hold integer class indices")
    if yh.size and (yh.min() < 0 or yh.max() >= K):
        raise ValueError(f"label out of range [0, {K})")
    cw = None
    if class_weight == "balanced":
        counts = np.bincount(yh, minlength=K).astype(np.float64)
        if (counts == 0).any():
            raise ValueError("class_weight='balanced' needs every class in y")
        cw = len(yh) / (K * counts)
    with torch.cuda.device(engine.device):
        xd = engine._probe_x(x, "softmax_fit")
        D = xd.shape[1]
        yd = torch.from_numpy(yh.astype(np.int32)).to(engine.device)
        cwd = None if cw is None else torch.tensor(cw, dtype=torch.float32, device=engine.device)
        wb = torch.zeros((K, D + 1), dtype=torch.float32, device=engine.device)
        if coef_init is not None:
            wb[:, :D] = torch.as_tensor(coef_init, dtype=torch.float32).reshape(K, D).to(engine.device)
        if intercept_init is not None:
            wb[:, D] = torch.as_tensor(intercept_init, dtype=torch.float32).reshape(K).to(engine.device)
        info = _lib.ProbeInfo()
        rc = engine.lib.plipmi_softmax_fit(engine._h, _ptr(xd), xd.shape[0], D, _ptr(yd), K, _ptr(cwd), float(alpha), int(max_iter),
                                           float(gtol), _ptr(wb), C_.byref(info), engine._stream())
        if rc not in (0, _lib.ERR_NOT_CONVERGED):
            _lib.check(rc, "plipmi_softmax_fit")
        if rc == _lib.ERR_NOT_CONVERGED:
            warnings.warn(_lib.last_error(), RuntimeWarning, stacklevel=2)
    out = dict(iterations=int(info.iterations), evaluations=int(info.evaluations), converged=rc == 0,
               grad_norm=float(info.grad_norm), loss=float(info.loss[0]), alpha=float(alpha))
    return wb[:, :D].contiguous(), wb[:, D].contiguous(), out
