"""The two resize front ends: Pillow-exact bicubic resize + centre crop on the GPU, for batches of one image size and for batches of
mixed sizes.  Mixed into ``plip_amd.engine.Engine``; the per-engine state they keep (``_resize_plans``, ``_ragged_ws``) is declared
in ``Engine._init_own_state``."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import _ptr
from .preprocess import _as_rgb_u8, pack_ragged, ragged_ksize, resize_crop_plan


def ragged_blob(images, out: Optional[torch.Tensor] = None):
    """Images of differing sizes -> ``(blob, offsets, hw)`` for :meth:`Engine.resize_crop_ragged`: ``blob`` = 1-D uint8 tensor holding
    the descriptors the kernels read (offsets int64 [B], then hw int32 [B,2]) followed by the images' RGB bytes end to end
    (``preprocess.pack_ragged``), so that ONE host-to-device copy carries a batch; ``offsets`` / ``hw`` are the host copies the C entry
    validates.  ``out``: a 1-D uint8 tensor to pack into (a pinned staging buffer of at least :func:`ragged_blob_bytes` bytes)."""
    arrs = [_as_rgb_u8(im) for im in images]
    head = 16 * len(arrs)
    total = head + sum(a.size for a in arrs)
    if out is None:
        out = torch.empty((total,), dtype=torch.uint8)
    elif out.numel() < total:
        raise ValueError(f"ragged_blob: the buffer holds {out.numel()} bytes, the batch needs {total}")
    view = out.numpy()
    _, offsets, hw = pack_ragged(arrs, out=view[head:total])
    view[:head // 2].view(np.int64)[:] = offsets
    view[head // 2:head].view(np.int32)[:] = hw.reshape(-1)
    return out[:total], offsets, hw


def ragged_blob_bytes(images) -> int:
    """Bytes :func:`ragged_blob` needs for these images (arrays / PIL images; nothing is decoded or converted)."""
    total = 16 * len(images)
    for im in images:
        h, w = (im.shape[0], im.shape[1]) if isinstance(im, np.ndarray) else (im.size[1], im.size[0])
        total += h * w * 3
    return total


class ResizeMixin:
    def _square_tile(self, what: str) -> int:
        n, n_w = self.image_hw
        if n != n_w:
            raise ValueError(f"{what} makes square tiles; this engine takes {n} x {n_w} images")
        return n

    def resize_crop_u8(self, images_u8: torch.Tensor, crop: str = "torchvision") -> torch.Tensor:
        """uint8 [B,H,W,3] images of one size -> uint8 [B,n,n,3] tiles at the model resolution: Pillow-exact bicubic
        resize (shortest edge -> n) + centre crop on the GPU; feed the result to :meth:`encode_image_u8`.
        ``crop`` = "torchvision" (OpenAI ``_transform``) or "hf" (``CLIPImageProcessor``), preprocess.crop_offset."""
        n = self._square_tile("resize_crop_u8")
        if images_u8.dim() != 4 or images_u8.shape[-1] != 3 or images_u8.dtype != torch.uint8:
            raise ValueError("expected uint8 [B,H,W,3]")
        B, H, Wd = int(images_u8.shape[0]), int(images_u8.shape[1]), int(images_u8.shape[2])
        cache = self._resize_plans
        if (Wd, H, crop) not in cache:
            plan = resize_crop_plan(Wd, H, n, crop)
            dev = {k: (None if plan[k] is None else torch.from_numpy(plan[k]).to(self.device)) for k in ("xb", "xk", "yb", "yk")}
            if plan["yb"] is not None:
                r0 = int(plan["yb"][:, 0].min())
                r1 = int((plan["yb"][:, 0] + plan["yb"][:, 1]).max())
            else:
                r0, r1 = plan["top"], plan["top"] + n
            cache[(Wd, H, crop)] = (plan, dev, r0, r1 - r0)
        plan, dev, r0, R = cache[(Wd, H, crop)]
        with torch.cuda.device(self.device):
            src = images_u8.to(self.device).contiguous()
            tmp = torch.empty((B, R, n, 3), dtype=torch.uint8, device=self.device)
            dst = torch.empty((B, n, n, 3), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.plipmi_resize_crop_u8(
                self._h, _ptr(src), B, H, Wd, n, _ptr(dev["xb"]), _ptr(dev["xk"]),
                0 if plan["xk"] is None else plan["xk"].shape[1], plan["left"], _ptr(dev["yb"]), _ptr(dev["yk"]),
                0 if plan["yk"] is None else plan["yk"].shape[1], plan["top"], r0, R, _ptr(tmp), _ptr(dst),
                self._stream()), "plipmi_resize_crop_u8")
        return dst

    def resize_crop_ragged(self, images, crop: str = "torchvision", n_px: Optional[int] = None) -> torch.Tensor:
        """uint8 RGB images of DIFFERING sizes -> uint8 [B,n,n,3] tiles on the device, each bit-identical to Pillow's bicubic resize
        (shortest edge -> n) + centre crop of that image; feed the result to :meth:`encode_image_u8`.  ``images``: a list of arrays /
        PIL images (packed here, one pageable H2D copy), or a :func:`ragged_blob` result ``(blob, offsets, hw)`` whose blob may sit in
        pinned memory or already on the device.  One copy carries the pixels and their descriptors; geometry and coefficient tables are
        computed on the device (include/plipmi.h ``plipmi_resize_crop_u8_ragged``), in a workspace this engine keeps and grows.
        Everything is enqueued on the current stream, nothing synchronises.  ``n_px``: the tile size (default: the engine's)."""
        if crop not in ("torchvision", "hf"):
            raise ValueError(f"unknown crop rule {crop!r} (expected 'hf' or 'torchvision')")
        n = self._square_tile("resize_crop_ragged") if n_px is None else int(n_px)
        blob, offsets, hw = images if isinstance(images, tuple) else ragged_blob(images)
        B = int(hw.shape[0])
        if B == 0:
            return torch.empty((0, n, n, 3), dtype=torch.uint8, device=self.device)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        hw = np.ascontiguousarray(hw, dtype=np.int32).reshape(B, 2)
        if blob.dtype != torch.uint8 or blob.dim() != 1 or blob.numel() < 16 * B:
            raise ValueError("the packed batch is a 1-D uint8 tensor: descriptors (16 bytes per image) then pixels")
        ks = ragged_ksize(hw, n)
        with torch.cuda.device(self.device):
            need = int(self.lib.plipmi_resize_ragged_workspace(hw.ctypes.data_as(C.c_void_p), B, n, ks))
            ws = self._ragged_ws
            if ws is None or ws.numel() < need:
                if ws is not None:
                    ws.record_stream(torch.cuda.current_stream(self.device))      # its last kernels may still be running there
                ws = self._ragged_ws = torch.empty((max(need, 1) * 5 // 4,), dtype=torch.uint8, device=self.device)
            src = blob.to(self.device, non_blocking=True)
            dst = torch.empty((B, n, n, 3), dtype=torch.uint8, device=self.device)
            base = src.data_ptr()
            _lib.check(self.lib.plipmi_resize_crop_u8_ragged(
                self._h, C.c_void_p(base + 16 * B), src.numel() - 16 * B, C.c_void_p(base), C.c_void_p(base + 8 * B),
                offsets.ctypes.data_as(C.c_void_p), hw.ctypes.data_as(C.c_void_p), B, n, 1 if crop == "hf" else 0, ks,
                _ptr(ws), ws.numel(), _ptr(dst), self._stream()), "plipmi_resize_crop_u8_ragged")
        return dst
