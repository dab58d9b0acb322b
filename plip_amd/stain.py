"""Macenko stain normalisation on the GPU (include/plipmi.h "stain normalisation"; csrc/stain.hip).  Functions on an engine, not methods
of it, like ``engine_region``: ``stain_fit(engine, images, ...)`` and ``stain_apply(engine, images, fit, ...)``.  They run on the given
engine and the caller's current stream, keep no state and never synchronise; ``PLIP.fit_stain`` / ``PLIP.normalize_stain`` and the
``stain=`` keyword of ``PLIP.encode_region`` route here.  The definition -- what is tissue, which percentile, which rounding -- is
``preprocess.stain_fit_reference`` / ``stain_apply_reference``, the float64 numpy oracle the kernels are tested against.

* A fit lives on the device (``StainFit.fits``, float64 [F, 16]: HE 6, P 6, maxC 2, n, valid); ``.numpy()`` is the caller's
  synchronisation.  An invalid fit (too little tissue, a degenerate stain plane) is flagged in its row and ``stain_apply`` copies such an
  image unchanged.
* ``images`` is uint8 [B,H,W,3] or [H,W,3] with last strides (3, 1); a device view (a crop of a larger array, every other image of a
  batch) is read where it lies.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import _ptr
from .preprocess import STAIN_ALPHA, STAIN_BETA, STAIN_IO, stain_lut, stain_target

_LUTS = {}        # (device, Io) -> float64 [256] on the device: the optical density of a byte, built by numpy (preprocess.stain_lut)
_TARGETS = {}     # device -> the default target, float64 [8]


@dataclass
class StainFit:
    """``fits``: float64 [F, 16] on the device, one row per fit (F = 1 for a pooled fit); the parameters it was made with."""
    fits: torch.Tensor
    pooled: bool
    step: int
    Io: float = STAIN_IO
    alpha: float = STAIN_ALPHA
    beta: float = STAIN_BETA

    def __len__(self) -> int:
        return int(self.fits.shape[0])

    def numpy(self) -> np.ndarray:
        """the rows on the host, float64 [F, 16] (synchronises): ``stain_fields`` names their parts"""
        return self.fits.detach().cpu().numpy()

    def as_target(self) -> torch.Tensor:
        """this ONE fit as the ``target`` of ``stain_apply``: float64 [8] on the device = its HE and maxC (no synchronisation).  An
        invalid fit makes a target of zeros: every pixel normalised to it comes out as ``min(255, Io)``."""
        if len(self) != 1:
            raise ValueError(f"a target is one fit, this holds {len(self)}")
        return torch.cat([self.fits[0, 0:6], self.fits[0, 12:14]])


def stain_fields(rows) -> dict:
    """float64 [F, 16] -> ``{"HE": [F,3,2], "P": [F,2,3], "maxC": [F,2], "n": int64 [F], "valid": bool [F]}``"""
    r = np.asarray(rows, np.float64).reshape(-1, 16)
    return {"HE": r[:, 0:6].reshape(-1, 3, 2), "P": r[:, 6:12].reshape(-1, 2, 3), "maxC": r[:, 12:14], "n": r[:, 14].astype(np.int64),
            "valid": r[:, 15] != 0.0}


def _check_params(step, Io, alpha, beta) -> None:
    if int(step) != step or int(step) < 1:
        raise ValueError(f"step must be an integer >= 1, got {step!r}")
    if not (math.isfinite(Io) and Io > 0):
        raise ValueError(f"Io must be positive, got {Io!r}")
    if not (0.0 < alpha < 50.0):
        raise ValueError(f"alpha must lie in (0, 50), got {alpha!r}")
    if not (math.isfinite(beta) and beta > 0):
        raise ValueError(f"beta must be positive, got {beta!r}")


def _check_images(images):
    """The caller's images as a uint8 tensor [B,H,W,3] (on whichever side it is) and whether it came as one [H,W,3] image."""
    if isinstance(images, np.ndarray):
        if images.dtype != np.uint8:
            raise ValueError(f"stain images are uint8 [B,H,W,3] or [H,W,3], got {images.dtype} {tuple(images.shape)}")
        images = np.ascontiguousarray(images)
        images = torch.from_numpy(images if images.flags.writeable else images.copy())
    if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() not in (3, 4) or images.shape[-1] != 3:
        what = f"{images.dtype} {tuple(images.shape)}" if torch.is_tensor(images) else type(images).__name__
        raise ValueError(f"stain images are uint8 [B,H,W,3] or [H,W,3], got {what}")
    single = images.dim() == 3
    x = images[None] if single else images
    B, H, W = (int(v) for v in x.shape[:3])
    if H < 1 or W < 1:
        raise ValueError(f"stain images need H, W >= 1, got {H} x {W}")
    st = x.stride()
    if tuple(st[2:]) != (3, 1) or (H > 1 and st[1] < 3 * W) or (B > 1 and st[0] < 0):
        raise ValueError(f"stain images are packed RGB rows: the last two strides must be (3, 1) and the row stride at least 3 W, got strides {tuple(st)}")
    return x, single


def _source_args(engine, x: torch.Tensor):
    """``x`` on the engine's device (a device view stays where it lies, a host tensor is uploaded densely) and (B, H, W, pitch, stride)"""
    if x.device != engine.device:
        x = x.contiguous().to(engine.device)
    B, H, W = (int(v) for v in x.shape[:3])
    pitch = int(x.stride(1)) if H > 1 else 3 * W
    image_stride = int(x.stride(0)) if B > 1 else H * pitch
    return x, (B, H, W, pitch, image_stride)


def _lut(engine, Io: float) -> torch.Tensor:
    key = (engine.device, float(Io))
    if key not in _LUTS:
        _LUTS[key] = torch.from_numpy(stain_lut(Io)).to(engine.device)
    return _LUTS[key]


def _target(engine, target) -> torch.Tensor:
    if target is None:
        if engine.device not in _TARGETS:
            _TARGETS[engine.device] = torch.from_numpy(stain_target(None)).to(engine.device)
        return _TARGETS[engine.device]
    if isinstance(target, StainFit):
        return target.as_target().to(engine.device)
    if torch.is_tensor(target):
        if target.numel() != 8:
            raise ValueError(f"a stain target is 8 values (HE [3,2], maxC [2]), got {target.numel()}")
        return target.to(device=engine.device, dtype=torch.float64).reshape(8).contiguous()
    return torch.from_numpy(stain_target(target)).to(engine.device)


def stain_fit(engine, images, pooled: bool = False, step: int = 1, Io: float = STAIN_IO, alpha: float = STAIN_ALPHA,
              beta: float = STAIN_BETA) -> StainFit:
    """Macenko fits of ``images`` over the pixels with ``y % step == 0 and x % step == 0``: one per image, or ONE over all of them with
    ``pooled``.  Enqueues on the caller's stream and returns a ``StainFit`` whose rows are on the device."""
    _check_params(step, Io, alpha, beta)
    x, _ = _check_images(images)
    step = int(step)
    with torch.cuda.device(engine.device):
        x, (B, H, W, pitch, image_stride) = _source_args(engine, x)
        F = 1 if pooled else B
        fits = torch.zeros((F, 16), dtype=torch.float64, device=engine.device)
        if B == 0:
            return StainFit(fits, bool(pooled), step, float(Io), float(alpha), float(beta))
        nbytes = int(engine.lib.plipmi_stain_workspace(B, H, W, step))
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=engine.device)
        _lib.check(engine.lib.plipmi_stain_fit(engine._h, _ptr(x), B, H, W, pitch, image_stride, step, int(bool(pooled)), float(Io), float(alpha),
                                               float(beta), _ptr(_lut(engine, Io)), _ptr(ws), _ptr(fits), engine._stream()), "plipmi_stain_fit")
    return StainFit(fits, bool(pooled), step, float(Io), float(alpha), float(beta))


def stain_apply(engine, images, fit: StainFit, target=None) -> torch.Tensor:
    """``images`` normalised by ``fit`` (one row for all, or one per image) to ``target``: None = Macenko's reference
    (``preprocess.HE_REF`` / ``MAXC_REF``), a one-row ``StainFit`` (normalise one slide to another), or 8 values.  uint8 on the device,
    contiguous, in the shape of ``images``; an image whose fit is invalid comes back unchanged.  Enqueues only."""
    if not isinstance(fit, StainFit):
        raise ValueError(f"fit must be a StainFit, got {type(fit).__name__}")
    x, single = _check_images(images)
    B = int(x.shape[0])
    if len(fit) not in (1, B):
        raise ValueError(f"need a fit of 1 row or of {B} (one per image), got {len(fit)}")
    if isinstance(target, StainFit) and len(target) != 1:
        raise ValueError(f"a target is one fit, got {len(target)}")
    with torch.cuda.device(engine.device):
        x, (B, H, W, pitch, image_stride) = _source_args(engine, x)
        dst = torch.empty((B, H, W, 3), dtype=torch.uint8, device=engine.device)
        if B:
            rows = fit.fits.to(engine.device)
            _lib.check(engine.lib.plipmi_stain_apply(engine._h, _ptr(x), B, H, W, pitch, image_stride, _ptr(rows), len(fit),
                                                     _ptr(_target(engine, target)), float(fit.Io), _ptr(_lut(engine, fit.Io)), _ptr(dst),
                                                     engine._stream()), "plipmi_stain_apply")
    return dst[0] if single else dst
