"""``PLIP.encode_region``: a slide region -- thousands of pixels per side, mostly glass -- to the embeddings of its tissue tiles, with
the grid, the background filter and the stacking on the GPU (engine_region.py) instead of in the caller's numpy.

A region is walked in BANDS of whole tile-rows: a device tensor is one band (a view; more only where it passes the entries' 4 GiB),
a host array / memmap / PIL image is uploaded band by band.  Per band: ``region_select`` on the caller's stream, ONE 4-byte copy of the
number of kept tiles to the host, then the kept tiles in batches of ``max_batch`` through the lane loop -- gather, resize where the
tile size is not the encode resolution, encode, all enqueued inside the lane's call on that lane's engine and stream, the routes
``encode_images`` takes for a host list of the same crops.  Counts and indices stay on the device until the embeddings are copied."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .engine_region import REGION_MAX_BYTES, region_gather, region_select
from .image_routes import _is_pil, lane_loop
from .preprocess import check_tissue_thresholds, region_grid, region_min_count


@dataclass
class RegionEmbeddings:
    """``PLIP.encode_region``: K kept tiles of a ``grid`` = (rows, cols).  ``embeddings`` float32 [K,P], un-normalised, as
    ``encode_images`` returns them; ``coords`` int64 [K,2], the (y, x) of each kept tile's top-left pixel in the region; ``kept`` int64
    [K], their flat grid indices (row * cols + col), ascending; ``tissue`` float32 [rows, cols], the tissue fraction of every tile."""
    embeddings: np.ndarray
    coords: np.ndarray
    kept: np.ndarray
    grid: Tuple[int, int]
    tissue: np.ndarray


def _as_region(region):
    """The caller's region as it will be read: a uint8 [H,W,3] tensor (any device) or numpy array (a memmap stays one)."""
    if _is_pil(region):
        region = np.asarray(region.convert("RGB"), dtype=np.uint8)
    if not torch.is_tensor(region) and not isinstance(region, np.ndarray):
        raise ValueError(f"a region is a uint8 [H,W,3] array, tensor or PIL image, got {type(region).__name__}")
    if region.dtype != (torch.uint8 if torch.is_tensor(region) else np.uint8) or region.ndim != 3 or region.shape[2] != 3:
        raise ValueError(f"a region is uint8 [H,W,3], got {region.dtype} {tuple(region.shape)}")
    return region


def _band_rows(region, eng, pitch: int, t: int, s: int, rows: int, band_rows: Optional[int]) -> int:
    """Tile-rows per band: the caller's, else everything for a device tensor and what a quarter of the free device memory holds for a
    host region -- and never more pixel rows than one call of the entries takes."""
    px_rows = REGION_MAX_BYTES // max(pitch, 1)
    if band_rows is None and not torch.is_tensor(region):
        free, _ = torch.cuda.mem_get_info(eng.device)
        px_rows = min(px_rows, (free // 4) // max(pitch, 1))
    fit = (px_rows - t) // s + 1 if px_rows >= t else 1         # (one tile-row is the least a band can be)
    return max(1, min(rows if band_rows is None else int(band_rows), fit, rows))


@dataclass
class RegionMosaic:
    """``PLIP.region_mosaic``: ``region`` = the ``RegionEmbeddings`` of the kept tiles; per cluster, ``representatives`` int64 [K] (the
    representative tile's index into the kept tiles) and ``rep_coords`` int64 [K,2] = ``region.coords[representatives]`` and ``rep_kept`` int64 [K] = ``region.kept[representatives]``, its
    flat grid index; ``labels`` int32 [tiles], every kept tile's cluster; ``counts`` int32 [K]; ``result``, the ``outputs.KMeansResult`` (None for a region without tissue)."""
    region: RegionEmbeddings
    representatives: np.ndarray
    rep_coords: np.ndarray
    rep_kept: np.ndarray
    labels: np.ndarray
    counts: np.ndarray
    result: Optional[object]


def encode_region(eng, region, n_px: int, projection_dim: int, crop: str, tile_px: Optional[int] = None, stride: Optional[int] = None,
                  origin=(0, 0), min_tissue: float = 0.5, sat_min: int = 18, luma_min: int = 25, luma_max: int = 235,
                  band_rows: Optional[int] = None, stain=None) -> RegionEmbeddings:
    """``region`` on engine ``eng`` (tile size ``n_px``): see ``PLIP.encode_region``.  Every argument is checked before anything is
    uploaded or launched."""
    region = _as_region(region)
    if stain is not None:
        from .stain import StainFit, stain_apply
        if not isinstance(stain, StainFit) or len(stain) != 1:
            raise ValueError("stain must be a StainFit of ONE fit (PLIP.fit_stain(region, pooled=True)), got "
                             + (f"{len(stain)} fits" if isinstance(stain, StainFit) else type(stain).__name__))
    t = int(n_px) if tile_px is None else int(tile_px)
    s = t if stride is None else int(stride)
    y0, x0 = (int(v) for v in origin)
    H, W = int(region.shape[0]), int(region.shape[1])
    rows, cols = region_grid(H, W, t, s, (y0, x0))          # (refuses tile, stride < 1 and a negative origin)
    check_tissue_thresholds(sat_min, luma_min, luma_max)
    min_count = region_min_count(min_tissue, t)
    if torch.is_tensor(region) and tuple(region.stride()[1:]) != (3, 1):
        raise ValueError(f"a region's pixels are packed RGB: its last two strides must be (3, 1), got {tuple(region.stride()[1:])}")
    if band_rows is not None and int(band_rows) < 1:
        raise ValueError(f"band_rows must be at least 1, got {band_rows}")
    ii, jj = np.divmod(np.arange(rows * cols, dtype=np.int64), max(cols, 1))
    if rows * cols == 0:
        return RegionEmbeddings(np.zeros((0, projection_dim), np.float32), np.zeros((0, 2), np.int64), np.zeros((0,), np.int64),
                                (rows, cols), np.zeros((rows, cols), np.float32))
    on_device = torch.is_tensor(region) and region.is_cuda
    if torch.is_tensor(region) and not on_device:
        region = region.numpy()
    pitch = int(region.stride(0)) if on_device and H > 1 else 3 * W
    per = _band_rows(region, eng, pitch, t, s, rows, band_rows)
    caller = torch.cuda.current_stream(eng.device)
    cap = int(eng.max_batch)
    outs, counts_dev, kept_dev = [], [], []

    def step(e, band, kept, first, B):
        """one batch of a band's kept tiles inside its lane: the lane waits for the select (and the upload) on the caller's stream, and
        the allocator is told that the band and the indices are read there (image_routes._encode_parts, ADVICE.md's cross-stream finding)"""
        lane = torch.cuda.current_stream(e.device)
        if lane != caller:
            lane.wait_stream(caller)
            band.record_stream(lane)
            kept.record_stream(lane)
        tiles = region_gather(e, band, kept, first, B, t, s, (0, x0))
        if stain is not None:           # the one fit for every tile, on the gathered bytes: tissue selection has seen the raw pixels
            tiles = stain_apply(e, tiles, stain)
        if t != n_px:
            tiles = e.resize_crop_u8(tiles, crop=crop)
        return e.encode_image_u8(tiles)

    with torch.no_grad(), lane_loop(eng) as run:
        for r0 in range(0, rows, per):
            r1 = min(rows, r0 + per)
            ya, yb = y0 + r0 * s, y0 + (r1 - 1) * s + t         # consecutive bands share t - s pixel rows when the tiles overlap
            band = region[ya:yb]
            if not on_device:
                band = np.ascontiguousarray(band)               # (a band of whole rows of a contiguous array is no copy)
                band = torch.from_numpy(band if band.flags.writeable else band.copy()).to(eng.device)
            counts, kept, n_kept = region_select(eng, band, t, s, (0, x0), min_count=min_count, sat_min=sat_min, luma_min=luma_min,
                                                 luma_max=luma_max)
            k = int(n_kept.item())                              # the band's one synchronisation: 4 bytes
            counts_dev.append(counts.reshape(-1))
            kept_dev.append(kept[:k] + r0 * cols)
            for a in range(0, k, cap):
                outs.append(run(lambda e, band=band, kept=kept, a=a, B=min(cap, k - a): step(e, band, kept, a, B)))
    kept_np = torch.cat(kept_dev).cpu().numpy().astype(np.int64)
    tissue = (torch.cat(counts_dev).cpu().numpy().astype(np.float32) / np.float32(t * t)).reshape(rows, cols)
    emb = torch.cat(outs).detach().cpu().numpy() if outs else np.zeros((0, projection_dim), np.float32)
    coords = np.stack([y0 + ii[kept_np] * s, x0 + jj[kept_np] * s], axis=1).astype(np.int64)
    return RegionEmbeddings(emb, coords, kept_np, (rows, cols), tissue)
