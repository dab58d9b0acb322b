"""What runs on embeddings the caller already holds: normalisation, logits, top-k, similarity top-k and the linear-probe head.  Mixed into
``plip_amd.engine.Engine``; none of it uses tower weights or keeps per-engine state."""
from __future__ import annotations

import ctypes as C
import math
import warnings
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import _ptr


class HeadsMixin:
    def l2_normalize_(self, x: torch.Tensor) -> torch.Tensor:
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
        with torch.cuda.device(self.device):
            _lib.check(self.lib.plipmi_l2_normalize(self._h, _ptr(x), x.shape[0], x.shape[1], self._stream()), "plipmi_l2_normalize")
        return x

    def logits(self, image_embeds: torch.Tensor, text_embeds: torch.Tensor, scale: float = 1.0,
               want_text: bool = True, want_argmax: bool = False):
        """scale * image_embeds @ text_embeds.T -> (logits_per_image, logits_per_text|None, argmax|None)."""
        with torch.cuda.device(self.device):
            img = image_embeds.to(device=self.device, dtype=torch.float32).contiguous()
            txt = text_embeds.to(device=self.device, dtype=torch.float32).contiguous()
            ni, nt, d = img.shape[0], txt.shape[0], img.shape[1]
            if txt.shape[1] != d:
                raise ValueError("embedding widths differ")
            lpi = torch.empty((ni, nt), dtype=torch.float32, device=self.device)
            lpt = torch.empty((nt, ni), dtype=torch.float32, device=self.device) if want_text else None
            am = torch.empty((ni,), dtype=torch.int32, device=self.device) if want_argmax else None
            _lib.check(self.lib.plipmi_logits(self._h, _ptr(img), ni, _ptr(txt), nt, d, float(scale), _ptr(lpi), _ptr(lpt),
                                              _ptr(am), self._stream()), "plipmi_logits")
        return lpi, lpt, am

    def topk(self, scores: torch.Tensor, k: int) -> torch.Tensor:
        with torch.cuda.device(self.device):
            sc = scores.to(device=self.device, dtype=torch.float32).contiguous()
            idx = torch.empty((sc.shape[0], k), dtype=torch.int64, device=self.device)
            _lib.check(self.lib.plipmi_topk(self._h, _ptr(sc), sc.shape[0], sc.shape[1], int(k), _ptr(idx), self._stream()), "plipmi_topk")
        return idx

    def similarity_topk(self, keys: torch.Tensor, space: torch.Tensor, k: int, return_values: bool = False):
        """Top-k rows of ``space`` by dot product for every row of ``keys`` -- ``(keys @ space.T).argsort()[:, -k:][:, ::-1]``
        (plip.py:83-84, retrieval.py:13-16) without the [Nq, Ns] matrix: scores exist only as [<=4096, <=8192] panels."""
        with torch.cuda.device(self.device):
            q = keys.to(device=self.device, dtype=torch.float32).contiguous()
            sp = space.to(device=self.device, dtype=torch.float32).contiguous()
            if q.dim() != 2 or sp.dim() != 2 or q.shape[1] != sp.shape[1]:
                raise ValueError("keys [Nq,D] and space [Ns,D] must share D")
            idx = torch.empty((q.shape[0], int(k)), dtype=torch.int64, device=self.device)
            vals = torch.empty((q.shape[0], int(k)), dtype=torch.float32, device=self.device) if return_values else None
            _lib.check(self.lib.plipmi_similarity_topk(self._h, _ptr(q), q.shape[0], _ptr(sp), sp.shape[0], q.shape[1],
                                                       int(k), _ptr(idx), _ptr(vals), self._stream()), "plipmi_similarity_topk")
        return (idx, vals) if return_values else idx

    # ---- linear-probe head (include/plipmi.h plipmi_probe_fit / plipmi_probe_predict) -------------------------------------
    @staticmethod
    def _probe_shape(x, what: str):
        shape = tuple(x.shape)
        if len(shape) != 2 or shape[0] < 1:
            raise ValueError(f"{what}: x must be [N >= 1, D], got {shape}")
        if shape[1] % 4 or not 4 <= shape[1] <= 1024:
            raise ValueError(f"{what}: embedding width {shape[1]} unsupported (D % 4 == 0, 4 <= D <= 1024)")
        return shape

    def _probe_fits(self, n: int, d: int, what: str, hint: str = "") -> None:
        """ValueError when an fp32 [n, d] copy of ``x`` would not fit the device's free memory"""
        free, _ = torch.cuda.mem_get_info(self.device)
        need = n * d * 4
        if need > free:
            raise ValueError(f"{what}: x [{n}, {d}] needs {need / 2**20:.0f} MiB of device memory, {free / 2**20:.0f} MiB are free{hint}")

    def _probe_x(self, x, what: str) -> torch.Tensor:
        """``x`` (host numpy / host or device torch) as a contiguous fp32 [N, D] tensor on this engine's device; ValueError before
        anything is allocated when it has the wrong shape or would not fit the device's free memory."""
        n, d = self._probe_shape(x, what)
        resident = (torch.is_tensor(x) and x.device == self.device and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0)
        if resident:
            return x
        self._probe_fits(n, d, what)
        t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()

    def probe_fit(self, x, y, n_classes: int, alpha: float, class_weight: Optional[str] = "balanced", max_iter: int = 1000,
                  gtol: float = 2e-8, coef_init=None, intercept_init=None):
        """Fit the reference's linear probe (``SGDClassifier(loss="log_loss", penalty="l2", alpha, class_weight)``'s objective,
        one-vs-rest; two classes: ONE problem for class 1) on embeddings ``x`` [N, D] with integer labels ``y`` in [0, n_classes):
        a full-batch L-BFGS solve inside libplipmi.so, converged to ``|grad|_inf <= gtol`` per problem, deterministic (no seed).
        ``x`` / ``y`` may be host numpy arrays or torch tensors on either side.  Returns ``(coef [K, D], intercept [K], info)`` as
        device tensors, K = n_classes (1 for two classes); ``info`` = dict(iterations, evaluations, converged (bool), grad_norm,
        loss [K]).  A fit that stops at ``max_iter`` is reported through ``info["converged"]`` and a RuntimeWarning, not raised."""
        C_ = int(n_classes)
        if C_ < 2:
            raise ValueError("the probe needs at least two classes")
        K = 1 if C_ == 2 else C_
        if K > _lib.PROBE_MAX_K:
            raise ValueError(f"at most {_lib.PROBE_MAX_K} classes, got {C_}")
        if class_weight not in ("balanced", None):
            raise ValueError("class_weight must be 'balanced' or None")
        if not (math.isfinite(alpha) and alpha > 0):
            raise ValueError(f"alpha must be finite and > 0, got {alpha}")
        if int(max_iter) < 1 or not (math.isfinite(gtol) and gtol > 0):
            raise ValueError("need max_iter >= 1 and a finite gtol > 0")
        n_rows, width = self._probe_shape(x, "probe_fit")
        if not (torch.is_tensor(x) and x.device == self.device):
            self._probe_fits(n_rows, width, "probe_fit", " (chunked fitting is not provided)")
        yh = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
        if yh.ndim != 1 or yh.shape[0] != x.shape[0]:
            raise ValueError(f"y must be [N = {x.shape[0]}], got {tuple(yh.shape)}")
        if not np.issubdtype(yh.dtype, np.integer):
            raise ValueError("y must hold integer class indices")
        if yh.size and (yh.min() < 0 or yh.max() >= C_):
            raise ValueError(f"label out of range [0, {C_})")
        counts = np.bincount(yh, minlength=C_).astype(np.float64)
        if class_weight == "balanced":
            if (counts == 0).any():
                raise ValueError("class_weight='balanced' needs every class in y")
            cw = len(yh) / (C_ * counts)
        else:
            cw = np.ones(C_)
        pos_w, neg_w = (cw[1:2], cw[0:1]) if C_ == 2 else (cw, np.ones(C_))
        with torch.cuda.device(self.device):
            xd = self._probe_x(x, "probe_fit")
            D = xd.shape[1]
            yd = torch.from_numpy(yh.astype(np.int32)).to(self.device)
            pw = torch.tensor(pos_w, dtype=torch.float32, device=self.device)
            nw = torch.tensor(neg_w, dtype=torch.float32, device=self.device)
            wb = torch.zeros((K, D + 1), dtype=torch.float32, device=self.device)
            if coef_init is not None:
                wb[:, :D] = torch.as_tensor(coef_init, dtype=torch.float32).reshape(K, D).to(self.device)
            if intercept_init is not None:
                wb[:, D] = torch.as_tensor(intercept_init, dtype=torch.float32).reshape(K).to(self.device)
            info = _lib.ProbeInfo()
            rc = self.lib.plipmi_probe_fit(self._h, _ptr(xd), xd.shape[0], D, _ptr(yd), K, _ptr(pw), _ptr(nw), float(alpha),
                                           int(max_iter), float(gtol), _ptr(wb), C.byref(info), self._stream())
            if rc not in (0, _lib.ERR_NOT_CONVERGED):
                _lib.check(rc, "plipmi_probe_fit")
            if rc == _lib.ERR_NOT_CONVERGED:
                warnings.warn(_lib.last_error(), RuntimeWarning, stacklevel=2)
        out = dict(iterations=int(info.iterations), evaluations=int(info.evaluations), converged=rc == 0,
                   grad_norm=float(info.grad_norm), loss=np.array(info.loss[:K], dtype=np.float64))
        return wb[:, :D].contiguous(), wb[:, D].contiguous(), out

    def probe_predict(self, x, coef, intercept, return_decision: bool = False, chunk_rows: Optional[int] = None):
        """``argmax_k (x . coef_k + intercept_k)`` (one problem: 1 if the decision value is > 0 else 0) as int32 [N] on the device, and
        with ``return_decision`` the fp32 decision values [N, K] too.  A host ``x`` travels in chunks (``chunk_rows``, default what a
        quarter of the free device memory holds), so it need not fit the device."""
        with torch.cuda.device(self.device):
            w = torch.as_tensor(coef, dtype=torch.float32).to(self.device)
            b = torch.as_tensor(intercept, dtype=torch.float32).to(self.device).reshape(-1)
            if w.dim() != 2 or b.shape[0] != w.shape[0] or not 1 <= w.shape[0] <= _lib.PROBE_MAX_K:
                raise ValueError(f"coef must be [1 <= K <= {_lib.PROBE_MAX_K}, D] and intercept [K]")
            K, D = int(w.shape[0]), int(w.shape[1])
            if len(x.shape) != 2 or x.shape[1] != D:
                raise ValueError(f"x must be [N, {D}], got {tuple(x.shape)}")
            N = int(x.shape[0])
            wb = torch.cat([w, b[:, None]], dim=1).contiguous()
            pred = torch.empty((N,), dtype=torch.int32, device=self.device)
            dec = torch.empty((N, K), dtype=torch.float32, device=self.device) if return_decision else None
            on_device = torch.is_tensor(x) and x.device == self.device
            if chunk_rows is None:
                free, _ = torch.cuda.mem_get_info(self.device)
                chunk_rows = N if on_device else max(1, min(N, int(free // 4) // (D * 4)))
            for a in range(0, N, max(1, int(chunk_rows))):
                e = min(N, a + int(chunk_rows))
                xd = self._probe_x(x[a:e], "probe_predict")
                _lib.check(self.lib.plipmi_probe_predict(self._h, _ptr(xd), e - a, D, _ptr(wb), K, _ptr(None if dec is None else dec[a:e]),
                                                         _ptr(pred[a:e]), self._stream()), "plipmi_probe_predict")
                xd.record_stream(torch.cuda.current_stream(self.device))
        return (pred, dec) if return_decision else pred
