"""The engine layer of slide regions: which tiles of a region on the device hold tissue, and those tiles as the uint8 batch the image
entries take (include/plipmi.h ``plipmi_region_select`` / ``plipmi_region_gather``; csrc/region.hip).  Functions on an engine, not
methods of it, like ``token_similarity``: ``region_select(engine, region, ...)``, ``region_gather(engine, region, kept, ...)``.  They
run on the given engine and the caller's current stream, keep no state, and neither synchronises; ``PLIP.encode_region``
(region_routes.py) is the loop over them."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import _ptr
from .preprocess import TISSUE_DEFAULTS, region_grid, region_min_count

REGION_MAX_BYTES = 2 ** 32 - 1      # rows x pitch of one call (the kernels' 32-bit offsets); larger regions go in bands of rows


def _region_args(engine, region: torch.Tensor, tile_px: int, stride: Optional[int], origin):
    """What both entries take for a region: the checked tensor on the engine's device and (H, W, pitch, y0, x0, tile, stride)."""
    if not torch.is_tensor(region) or region.dtype != torch.uint8 or region.dim() != 3 or region.shape[2] != 3:
        what = f"{region.dtype} {tuple(region.shape)}" if torch.is_tensor(region) else type(region).__name__
        raise ValueError(f"a region is a uint8 [H,W,3] tensor, got {what}")
    if tuple(region.stride()[1:]) != (3, 1):
        raise ValueError(f"a region's pixels are packed RGB: its last two strides must be (3, 1), got {tuple(region.stride()[1:])} "
                         "(any row stride will do)")
    region = region.to(engine.device)
    H, W = int(region.shape[0]), int(region.shape[1])
    pitch = int(region.stride(0)) if H > 1 else 3 * W
    t = int(tile_px)
    s = t if stride is None else int(stride)
    y0, x0 = (int(v) for v in origin)
    return region, (H, W, pitch, y0, x0, t, s)


def region_select(engine, region: torch.Tensor, tile_px: int, stride: Optional[int] = None, origin: Tuple[int, int] = (0, 0),
                  min_tissue: float = 0.5, sat_min: int = TISSUE_DEFAULTS["sat_min"], luma_min: int = TISSUE_DEFAULTS["luma_min"],
                  luma_max: int = TISSUE_DEFAULTS["luma_max"], min_count: Optional[int] = None):
    """``region``: uint8 [H,W,3] on the device, any row stride (a view of a larger array works without a copy) -> ``(counts, kept,
    n_kept)`` on the device: ``counts`` int32 [rows, cols], the tissue pixels (``preprocess.tissue_mask``) of every tile of
    ``preprocess.region_grid``; ``kept`` int32 [rows * cols] whose first ``n_kept`` entries are the flat indices of the tiles with at
    least ``min_count`` of them (default ``ceil(min_tissue * tile_px ** 2)``), ascending; ``n_kept`` int32 [1].  Reading ``n_kept`` on
    the host is the caller's one synchronisation."""
    region, (H, W, pitch, y0, x0, t, s) = _region_args(engine, region, tile_px, stride, origin)
    rows, cols = region_grid(H, W, t, s, (y0, x0))
    if min_count is None:
        min_count = region_min_count(min_tissue, t)
    with torch.cuda.device(engine.device):
        counts = torch.empty((rows, cols), dtype=torch.int32, device=engine.device)
        kept = torch.empty((rows * cols,), dtype=torch.int32, device=engine.device)
        n_kept = torch.empty((1,), dtype=torch.int32, device=engine.device)
        _lib.check(engine.lib.plipmi_region_select(engine._h, _ptr(region), H, W, pitch, y0, x0, t, s, rows, cols, int(sat_min),
                                                   int(luma_min), int(luma_max), int(min_count), _ptr(counts), _ptr(kept), _ptr(n_kept),
                                                   engine._stream()), "plipmi_region_select")
    return counts, kept, n_kept


def region_gather(engine, region: torch.Tensor, kept: torch.Tensor, first: int, B: int, tile_px: int, stride: Optional[int] = None,
                  origin: Tuple[int, int] = (0, 0)) -> torch.Tensor:
    """Tiles ``kept[first : first + B]`` (int32 flat indices on the device, ``region_select``'s or the caller's own) of the same grid
    on ``region`` -> uint8 [B, tile_px, tile_px, 3] on the device, for ``encode_image_u8`` / ``resize_crop_u8``."""
    region, (H, W, pitch, y0, x0, t, s) = _region_args(engine, region, tile_px, stride, origin)
    if not torch.is_tensor(kept) or kept.dtype != torch.int32 or kept.dim() != 1 or not kept.is_contiguous() or kept.device != region.device:
        raise ValueError("kept is a contiguous int32 [n] tensor on the region's device")
    first, B = int(first), int(B)
    if first < 0 or B < 0 or first + B > kept.numel():
        raise ValueError(f"kept[{first}:{first + B}] of {kept.numel()} entries")
    _, cols = region_grid(H, W, t, s, (y0, x0))
    with torch.cuda.device(engine.device):
        dst = torch.empty((B, t, t, 3), dtype=torch.uint8, device=engine.device)
        _lib.check(engine.lib.plipmi_region_gather(engine._h, _ptr(region), H, W, pitch, y0, x0, t, s, cols, _ptr(kept), first, B,
                                                   _ptr(dst), engine._stream()), "plipmi_region_gather")
    return dst
