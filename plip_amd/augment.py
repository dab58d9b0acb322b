"""The engine layer of augmented views: Pillow-exact affine / perspective warps of uint8 tiles on the device (include/plipmi.h
``plipmi_warp_u8``; csrc/augment.hip), the reference's train chain as two of them and the eight dihedral views of a tile.  Functions
on an engine, not methods of it, like ``engine_region`` and ``token_similarity``: they run on the given engine and the caller's current
stream, keep no state, and none synchronises; ``PLIP.encode_views`` (``encode_views`` below) is the loop over them.

Coefficient rows and windows are host arrays here (``preprocess.affine_coeffs`` / ``perspective_coeffs`` / ``dihedral_coeffs`` /
``train_params``): they are checked by name before anything is uploaded or launched -- a perspective row whose denominator vanishes
inside the output, a window outside the source -- and the kernel reads them on the device.  (A caller of the C entry who builds rows on
the device gets the device's refusal instead: that image comes out all fill.)"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import _ptr
from .image_routes import _is_pil, lane_loop
from .preprocess import check_perspective, dihedral_coeffs, train_params

TRANSFORMS = ("d4", "train")


def _fill_rgb(fill) -> int:
    rgb = (fill,) * 3 if np.ndim(fill) == 0 else tuple(fill)
    if len(rgb) != 3 or any(int(v) != v or not 0 <= int(v) <= 255 for v in rgb):
        raise ValueError(f"fill is an integer 0 .. 255 or three of them (r, g, b), got {fill!r}")
    return int(rgb[0]) | int(rgb[1]) << 8 | int(rgb[2]) << 16


def _source_args(src: torch.Tensor):
    """``src`` uint8 [H,W,3] (one image for every output) or [B,H,W,3] -> (images or None, H, W, pitch_bytes, image_stride_bytes)."""
    if not torch.is_tensor(src) or src.dtype != torch.uint8 or src.dim() not in (3, 4) or src.shape[-1] != 3:
        what = f"{src.dtype} {tuple(src.shape)}" if torch.is_tensor(src) else type(src).__name__
        raise ValueError(f"a warp's source is a uint8 [H,W,3] or [B,H,W,3] tensor, got {what}")
    if tuple(src.stride()[-2:]) != (3, 1):
        raise ValueError(f"a source's pixels are packed RGB: its last two strides must be (3, 1), got {tuple(src.stride()[-2:])} "
                         "(any row and image stride will do)")
    if not src.is_cuda:
        raise ValueError("a warp's source is on the device (strides are kept: upload it first)")
    H, W = int(src.shape[-3]), int(src.shape[-2])
    if H < 1 or W < 1:
        raise ValueError(f"a source of {H} x {W} pixels")
    pitch = int(src.stride(-3)) if H > 1 else 3 * W
    if src.dim() == 3:
        return None, H, W, pitch, 0
    n = int(src.shape[0])
    stride = int(src.stride(0)) if n > 1 else 0
    if n > 1 and stride < 1:
        raise ValueError(f"the images of a source batch are {stride} bytes apart: pass one [H,W,3] image for views of one image")
    return n, H, W, pitch, stride


def _check_windows(win: np.ndarray, H: int, W: int) -> np.ndarray:
    """integer [..., 5] rows (wy, wx, wh, ww, flip), each inside an H x W source -> the same rows as int32; refused by name otherwise"""
    if win.dtype.kind not in "iu" or win.shape[-1] != 5:
        raise ValueError(f"windows are integer [..., 5] rows (wy, wx, wh, ww, flip), got {win.dtype} {win.shape}")
    w = win.astype(np.int64)
    bad = (w[..., 0] < 0) | (w[..., 1] < 0) | (w[..., 2] < 1) | (w[..., 3] < 1) | (w[..., 0] + w[..., 2] > H) | (w[..., 1] + w[..., 3] > W)
    if bad.any():
        i = np.argwhere(bad)[0].tolist()
        raise ValueError(f"window {i[0] if len(i) == 1 else i} = {w[tuple(i)][:4].tolist()} (wy, wx, wh, ww) does not lie inside the {H} x {W} source")
    return w.astype(np.int32)


def warp_u8(engine, src: torch.Tensor, coeffs, windows=None, perspective: bool = False, out_size=None, fill=127,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``src`` uint8 on the device, [B,H,W,3] (output b samples image b; any row and image stride: views work without a copy) or
    [H,W,3] (every output samples the one image) -> uint8 [B,oh,ow,3] with the bytes of Pillow's ``Image.transform(..., BILINEAR,
    fillcolor=fill)`` (``preprocess.warp_reference``).  ``coeffs`` [B,6] or [B,8] float64 on the host, output -> input rows;
    ``windows`` int32 [B,5] on the host (wy, wx, wh, ww, flip) or None (the whole source, not mirrored); ``out_size`` (oh, ow),
    default the source's; ``fill`` an int or (r, g, b); ``out``: a contiguous uint8 [B,oh,ow,3] on the device to write instead of a
    new tensor.  ValueError before any upload or launch for a perspective row whose denominator vanishes (``check_perspective``) and
    a window that does not lie inside the source.  One launch on the caller's stream."""
    n_src, H, W, pitch, stride = _source_args(src)
    a = np.asarray(coeffs.cpu().numpy() if torch.is_tensor(coeffs) else coeffs, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] not in (6, 8) or (perspective and a.shape[1] != 8):
        raise ValueError(f"coeffs are [B,6] or [B,8] (perspective: [B,8]) float64 rows, got {a.shape}")
    B = int(a.shape[0])
    if n_src is not None and n_src != B:
        raise ValueError(f"{B} coefficient rows for {n_src} source images (pass one [H,W,3] image for B views of it)")
    rows = np.zeros((B, 8), np.float64)
    rows[:, :a.shape[1]] = a
    oh, ow = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if oh < 1 or ow < 1:
        raise ValueError(f"an output of {oh} x {ow} pixels")
    if perspective:
        check_perspective(rows, oh, ow)
    win = None
    if windows is not None:
        win = np.ascontiguousarray(windows.cpu().numpy() if torch.is_tensor(windows) else windows)
        if win.shape != (B, 5):
            raise ValueError(f"windows are integer [B,5] rows (wy, wx, wh, ww, flip) for the {B} outputs, got {win.dtype} {win.shape}")
        win = _check_windows(win, H, W)
    fill_rgb = _fill_rgb(fill)
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (B, oh, ow, 3)
                            or not out.is_contiguous() or not out.is_cuda):
        raise ValueError(f"out is a contiguous uint8 [{B},{oh},{ow},3] tensor on the source's device")
    with torch.cuda.device(engine.device):
        dst = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=engine.device) if out is None else out
        if B == 0:
            return dst
        rows_dev = torch.from_numpy(rows).to(engine.device, non_blocking=True)
        win_dev = None if win is None else torch.from_numpy(win).to(engine.device, non_blocking=True)
        _lib.check(engine.lib.plipmi_warp_u8(engine._h, _ptr(src), B, H, W, pitch, stride, _ptr(win_dev), _ptr(rows_dev),
                                             int(bool(perspective)), oh, ow, fill_rgb, _ptr(dst), engine._stream()), "plipmi_warp_u8")
    return dst


def train_views(engine, src_u8: torch.Tensor, params, fill=127) -> torch.Tensor:
    """The reference's train chain on the device.  ``src_u8`` uint8 [N,H,W,3]; ``params`` = (windows [N,V,5], affine [N,V,8],
    perspective [N,V,8]) of ``preprocess.train_params`` (or [N,5] / [N,8] / [N,8]: one view each) -> uint8 [V,N,n,n,3], VIEW-MAJOR:
    ``out[v, i]`` is view v of tile i, the layout the launches write without a copy.  Per view one launch of crop + flip + affine from
    the source (every tile of the view), then ONE perspective launch over all V * N of them; each stage rounds to bytes, as the PIL
    chain does -- an identity perspective row copies its input exactly.  (One fused pass would not be exact.)"""
    windows, affine, persp = (np.asarray(p) for p in params)
    if windows.ndim == 2:
        windows, affine, persp = windows[:, None], affine[:, None], persp[:, None]
    if src_u8.dim() != 4 or windows.ndim != 3 or windows.shape[:2] != affine.shape[:2] or windows.shape[:2] != persp.shape[:2] \
            or windows.shape[0] != src_u8.shape[0]:
        raise ValueError(f"train_views takes uint8 [N,H,W,3] tiles and params [N,V,5], [N,V,8], [N,V,8]; got {tuple(src_u8.shape)}, "
                         f"{windows.shape}, {affine.shape}, {persp.shape}")
    N, V = windows.shape[:2]
    sizes = np.unique(windows[..., 2:4]) if windows.size else np.zeros(0)
    if sizes.size != 1:
        raise ValueError(f"the crops of one call have one square size, got {sizes.tolist()}")
    n = int(sizes[0])
    # everything the V + 1 launches would refuse, before the first of them
    _, H, W, _, _ = _source_args(src_u8)
    windows = _check_windows(windows, H, W)
    _fill_rgb(fill)
    if affine.shape[2] not in (6, 8) or persp.shape[2] != 8:
        raise ValueError(f"affine rows have 6 or 8 coefficients and perspective rows 8, got {affine.shape} and {persp.shape}")
    check_perspective(persp, n, n)
    with torch.cuda.device(engine.device):
        stage = torch.empty((V, N, n, n, 3), dtype=torch.uint8, device=engine.device)
        for v in range(V):
            warp_u8(engine, src_u8, affine[:, v], windows[:, v], False, (n, n), fill, out=stage[v])
        out = warp_u8(engine, stage.view(V * N, n, n, 3), persp.transpose(1, 0, 2).reshape(V * N, 8), None, True, (n, n), fill)
    return out.view(V, N, n, n, 3)


def dihedral_views(engine, tiles: torch.Tensor, views: int = 8) -> torch.Tensor:
    """uint8 [N,n,n,3] square tiles -> uint8 [V,N,n,n,3], view-major: ``out[k, i]`` is symmetry k of tile i in the order of
    ``preprocess.dihedral_coeffs`` (``np.rot90(t if k < 4 else t[:, ::-1], k % 4)``) -- exact re-indexing, one launch per view."""
    if not torch.is_tensor(tiles) or tiles.dim() != 4 or tiles.shape[1] != tiles.shape[2]:
        raise ValueError(f"dihedral_views takes square uint8 [N,n,n,3] tiles, got {tuple(tiles.shape) if torch.is_tensor(tiles) else type(tiles).__name__}")
    if not 1 <= int(views) <= 8:
        raise ValueError(f"a square has eight symmetries: views = 1 .. 8, got {views}")
    N, n = int(tiles.shape[0]), int(tiles.shape[1])
    with torch.cuda.device(engine.device):
        out = torch.empty((int(views), N, n, n, 3), dtype=torch.uint8, device=engine.device)
        for k in range(int(views)):
            warp_u8(engine, tiles, np.tile(dihedral_coeffs(k, n), (N, 1)), None, False, (n, n), 0, out=out[k])
    return out


# ---- PLIP.encode_views ---------------------------------------------------------------------------------------------------------------
def _as_tiles(images):
    """The caller's tiles as ONE uint8 [N,H,W,3] array or tensor; a list of arrays / PIL images is stacked (mixed sizes are refused)."""
    if torch.is_tensor(images) or isinstance(images, np.ndarray):
        tiles = images
    else:
        arrs = [np.asarray(im.convert("RGB"), dtype=np.uint8) if _is_pil(im) else (im.cpu().numpy() if torch.is_tensor(im) else np.asarray(im))
                for im in images]
        shapes = sorted({a.shape for a in arrs})
        if len(shapes) > 1:
            raise ValueError(f"encode_views takes tiles of one size, got mixed sizes {shapes[:4]} (resize them first: encode_images' "
                             "resize route, Engine.resize_crop_u8 / resize_crop_ragged)")
        tiles = np.stack(arrs) if arrs else np.zeros((0, 0, 0, 3), np.uint8)
    if tiles.dtype != (torch.uint8 if torch.is_tensor(tiles) else np.uint8) or tiles.ndim != 4 or tiles.shape[3] != 3:
        raise ValueError(f"encode_views takes uint8 [N,H,W,3] tiles, got {tiles.dtype} {tuple(tiles.shape)}")
    return tiles


def encode_views(eng, images, batch_size: int, n_px: int, projection_dim: int, views: int = 8, transform: str = "d4", seed: int = 0,
                 reduce: Optional[str] = None, return_params: bool = False):
    """``PLIP.encode_views`` on engine ``eng`` (encode resolution ``n_px``): every argument is checked, and every parameter row is
    drawn and checked, before anything is uploaded or launched."""
    if transform not in TRANSFORMS:
        raise ValueError(f"unknown transform {transform!r}: expected one of {TRANSFORMS}")
    if reduce not in (None, "mean"):
        raise ValueError(f"reduce must be None or 'mean', got {reduce!r}")
    V, step = int(views), int(batch_size)
    if V < 1 or step < 1:
        raise ValueError(f"views {views} and batch_size {batch_size} must be at least 1")
    if transform == "d4" and V > 8:
        raise ValueError(f"transform 'd4' has eight views (the symmetries of the square), got views={views}")
    tiles = _as_tiles(images)
    N, H, W = int(tiles.shape[0]), int(tiles.shape[1]), int(tiles.shape[2])
    if N and transform == "d4" and (H, W) != (n_px, n_px):
        raise ValueError(f"transform 'd4' takes tiles at the encode resolution {n_px} x {n_px}, got {H} x {W}")
    if N and transform == "train" and (H < n_px or W < n_px):
        raise ValueError(f"transform 'train' crops {n_px} x {n_px} windows: tiles of {H} x {W} pixels are smaller than n_px")
    if transform == "train":
        params = train_params(seed, N, V, (H, W), n_px) if N else (np.zeros((0, V, 5), np.int32),) + (np.zeros((0, V, 8)),) * 2
    else:
        rows = np.zeros((V, 8), np.float64)
        rows[:, :6] = [dihedral_coeffs(k, n_px) for k in range(V)]
        params = (np.broadcast_to(np.asarray([0, 0, n_px, n_px, 0], np.int32), (N, V, 5)).copy(),
                  np.broadcast_to(rows, (N, V, 8)).copy(), np.broadcast_to(np.asarray([1.0, 0, 0, 0, 1, 0, 0, 0]), (N, V, 8)).copy())
    on_device = torch.is_tensor(tiles) and tiles.is_cuda
    if torch.is_tensor(tiles) and not on_device:
        tiles = tiles.numpy()
    caller = torch.cuda.current_stream(eng.device) if on_device else None
    outs = []

    def run_chunk(e, a, b):
        """views of tiles a .. b built and encoded inside the lane: upload (or the caller's device tensor, which the lane waits for --
        region_routes.step), the warps, the towers -- one engine, one stream"""
        chunk = tiles[a:b]
        if on_device:
            lane = torch.cuda.current_stream(e.device)
            if lane != caller:
                lane.wait_stream(caller)
                chunk.record_stream(lane)
        else:
            chunk = np.ascontiguousarray(chunk)
            chunk = torch.from_numpy(chunk if chunk.flags.writeable else chunk.copy()).to(e.device)
        if transform == "train":
            v = train_views(e, chunk, tuple(p[a:b] for p in params))
        else:
            v = dihedral_views(e, chunk, V)
        emb = e.encode_image_u8(v.view(V * (b - a), n_px, n_px, 3))
        return emb.view(V, b - a, -1).transpose(0, 1)            # [Nb,V,P]: a view of the view-major rows

    with torch.no_grad(), lane_loop(eng) as run:
        for a in range(0, N, step):
            outs.append(run(lambda e, a=a, b=min(N, a + step): run_chunk(e, a, b)))
    emb = torch.cat(outs).detach().cpu().numpy() if outs else np.zeros((0, V, projection_dim), np.float32)
    if reduce == "mean":       # [N,V,P] is small: the normalised mean in float64 on the host, rounded once
        x = emb.astype(np.float64)
        x = x / np.linalg.norm(x, axis=-1, keepdims=True)
        m = x.mean(axis=1)
        emb = (m / np.linalg.norm(m, axis=-1, keepdims=True)).astype(np.float32)
    return (emb, params) if return_params else emb
