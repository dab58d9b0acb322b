"""Where a batch of images goes, and that decision run on an engine -- shared by ``PLIP.encode_images`` (direct and pipelined, at the
checkpoint's resolution and at ``image_size=``), ``PLIP.attention_maps`` and ``CLIPEmbedder``'s routed loop.

``classify`` is the one place that looks at a batch: native uint8 tiles / uint8 images of one other size (resized on the GPU) / images
of differing sizes (``ragged``: the GPU's ragged resize) / float pixels / whatever is left for host Pillow.  ``open_paths`` is the one
place that opens files.  ``encode_direct`` is the direct host loop, ``prepare_routed_batch`` + ``consume_routed_batch`` the two halves of
the pipelined one (``pipeline.run_batches`` prepares batch k + 1 while batch k runs).

The loops coalesce on the HOST only: a batch stays host arrays (or the caller's own tensors) until it is flushed, and every device-side
step of it -- upload, resize + crop, encode -- is enqueued inside the call of the lane it runs on, on that lane's engine and stream.  A
resize is therefore followed directly by the encode that reads its output, on the same engine and stream.  (One exception in the
sequence, none in the placement: one-size batches of DIFFERENT sizes that share a flush of the direct loop are resized size by size
and encoded together -- a flush per size measured 5.5 ms against 2.9 ms for 8 batches of 8, profiles/plip_routes_ab.txt.)
"""
from __future__ import annotations

import contextlib
import itertools

import numpy as np
import torch

from .preprocess import preprocess_image, preprocess_images, ragged_supported


# ---- what a batch holds ------------------------------------------------------------------------------------------------------------
def _is_pil(im) -> bool:
    return hasattr(im, "size") and hasattr(im, "mode") and not torch.is_tensor(im)      # (a tensor has both, as methods)


def _native_u8_tiles(chunk, n_px):
    """uint8 HWC tiles that are already at the model resolution -> one [B,n,n,3] array, else None."""
    if torch.is_tensor(chunk):
        return None
    if isinstance(chunk, np.ndarray):
        ok = chunk.dtype == np.uint8 and chunk.ndim == 4 and chunk.shape[1:] == (n_px, n_px, 3)
        return np.ascontiguousarray(chunk) if ok else None
    arrs = []
    for im in chunk:
        if isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.shape == (n_px, n_px, 3):
            arrs.append(im)
        elif _is_pil(im) and im.size == (n_px, n_px):
            arrs.append(np.asarray(im.convert("RGB"), dtype=np.uint8))
        else:
            return None
    return np.stack(arrs) if arrs else None


def _all_native_tiles(chunk, n_px) -> bool:
    """every element an n_px x n_px uint8 RGB array or PIL image (what _native_u8_tiles would stack)"""
    if len(chunk) == 0:
        return False
    for im in chunk:
        if isinstance(im, np.ndarray):
            if im.dtype != np.uint8 or im.shape != (n_px, n_px, 3):
                return False
        elif not (_is_pil(im) and im.size == (n_px, n_px)):
            return False
    return True


def _uniform_u8_images(chunk, n_px):
    """Equally sized uint8 RGB images (arrays or PIL) that still need resize/crop -> one [B,H,W,3] array, else None."""
    if torch.is_tensor(chunk) or isinstance(chunk, np.ndarray) or len(chunk) == 0:
        return None
    arrs, shape = [], None
    for im in chunk:
        if isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3:
            a = im
        elif _is_pil(im):
            a = np.asarray(im.convert("RGB"), dtype=np.uint8)
        else:
            return None
        if shape is None:
            shape = a.shape
        if a.shape != shape or min(a.shape[:2]) < 8:
            return None
        arrs.append(a)
    return np.stack(arrs)


def _u8_image_hw(im):
    """(h, w) of a uint8 array (grey, RGB, RGBA) or PIL image -- what ``preprocess.pack_ragged`` takes --, else None."""
    if isinstance(im, np.ndarray):
        ok = im.dtype == np.uint8 and (im.ndim == 2 or (im.ndim == 3 and im.shape[2] in (3, 4)))
        return (int(im.shape[0]), int(im.shape[1])) if ok else None
    if not _is_pil(im):
        return None
    return int(im.size[1]), int(im.size[0])


def _ragged_segments(chunk, n_px):
    """A list of images -> ``[("ragged", [images...]) | ("host", [image]), ...]`` in order: runs of images the device entry takes, and
    one "host" entry per image it does not (a float array, an in / out ratio over the limit), which keeps the Pillow path.  None
    when the chunk is not a list or holds nothing for the device."""
    if not isinstance(chunk, (list, tuple)) or len(chunk) == 0:
        return None
    segs = []
    for im in chunk:
        hw = _u8_image_hw(im)
        if hw is not None and ragged_supported(hw[0], hw[1], n_px):
            if segs and segs[-1][0] == "ragged":
                segs[-1][1].append(im)
            else:
                segs.append(("ragged", [im]))
        else:
            segs.append(("host", [im]))
    return segs if any(k == "ragged" for k, _ in segs) else None


def classify(chunk, n_px, ragged=False, stage=False):
    """One caller batch (paths opened) -> ``(route, payload)``, everything still on the host or the caller's own tensor:

    ``"stage"``   a list of n_px x n_px uint8 arrays / PIL images as it is, for the caller's pinned staging rows (only with ``stage``);
    ``"tiles"``   uint8 [B,n,n,3], array or tensor;
    ``"resize"``  uint8 [B,H,W,3] of one other size, array or tensor: the GPU's resize + crop;
    ``"ragged"``  (only with ``ragged``) the ``_ragged_segments`` of a list of differing sizes;
    ``"pixels"``  a float array or tensor;
    ``"host"``    the batch as a list, for ``preprocess_image(s)``."""
    if stage and isinstance(chunk, (list, tuple)) and _all_native_tiles(chunk, n_px):
        return "stage", list(chunk)
    tiles = _native_u8_tiles(chunk, n_px)
    if tiles is not None:
        return "tiles", tiles
    same = _uniform_u8_images(chunk, n_px)
    if same is not None:
        return "resize", same
    segs = _ragged_segments(chunk, n_px) if ragged else None
    if segs is not None:
        return "ragged", segs
    if torch.is_tensor(chunk) or isinstance(chunk, np.ndarray):
        if chunk.dtype != (torch.uint8 if torch.is_tensor(chunk) else np.uint8):
            return "pixels", chunk
        return ("tiles" if tuple(chunk.shape[1:]) == (n_px, n_px, 3) else "resize"), chunk
    return "host", list(chunk)


# ---- files -------------------------------------------------------------------------------------------------------------------------
def _decode_image(im):
    if isinstance(im, str):            # read where this runs (the pipelined loop: on the worker threads), the file closed again
        from PIL import Image
        im = Image.open(im)
        im.load()
    return im


def open_paths(chunk, pool=None):
    """A list batch with its ``str`` entries opened as PIL images (plip.py:34); arrays and tensors pass through."""
    if not isinstance(chunk, (list, tuple)):
        return chunk
    return list(pool.map(_decode_image, chunk)) if pool is not None else [_decode_image(c) for c in chunk]


# ---- a routed batch on an engine ---------------------------------------------------------------------------------------------------
class PinnedPair:
    """Two page-locked byte buffers used alternately by the batch producer of ``pipeline.run_batches``: batch k + 1 is packed into
    one while the copy of batch k leaves the other (``run_batches`` waits for that copy before the producer runs again)."""

    def __init__(self):
        self.bufs, self.k = [None, None], 0

    def take(self, nbytes: int) -> torch.Tensor:
        i, self.k = self.k, self.k ^ 1
        if self.bufs[i] is None or self.bufs[i].numel() < nbytes:
            self.bufs[i] = torch.empty((max(nbytes, 1) * 5 // 4,), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        return self.bufs[i]


def _encode_segments(e, segs, n_px, crop, normalize=False):
    """The segments of one chunk on engine ``e`` (inside a lane: every device-side step, the copy included, is enqueued here)."""
    outs = []
    for kind, items in segs:
        if kind == "ragged":
            outs.append(e.encode_image_u8(e.resize_crop_ragged(items, crop=crop), normalize=normalize))
        else:
            outs.append(e.encode_image(torch.from_numpy(preprocess_images(items, n_px, crop=crop)), normalize=normalize))
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def _ragged_prepare(chunk, segs, n_px, crop, pool, pinned):
    """One decoded batch and its ``_ragged_segments`` -> ``(("ragged", offsets, hw, rows, host), blob)`` for ``run_batches``: the images
    the device takes, converted to RGB on the workers and packed with their descriptors into a pinned buffer; ``rows`` = their positions
    in the batch (None: all of it) and ``host`` = [(position, fp32 pixels)] of the others, preprocessed on the host."""
    from .engine import ragged_blob
    from .preprocess import _as_rgb_u8
    flags = [k == "ragged" for k, items in segs for _ in items]
    dev = [im for im, f in zip(chunk, flags) if f]
    rgb = list(pool.map(_as_rgb_u8, dev)) if pool is not None else [_as_rgb_u8(im) for im in dev]
    out = pinned.take(16 * len(rgb) + sum(a.size for a in rgb)) if pinned is not None else None
    blob, offsets, hw = ragged_blob(rgb, out=out)
    host = [(i, preprocess_image(chunk[i], n_px, crop)) for i, f in enumerate(flags) if not f]
    rows = None if not host else [i for i, f in enumerate(flags) if f]
    return ("ragged", offsets, hw, rows, host), blob


def _ragged_consume(e, tag, blob, crop, normalize=False):
    _, offsets, hw, rows, host = tag
    u = e.encode_image_u8(e.resize_crop_ragged((blob, offsets, hw), crop=crop), normalize=normalize)
    if not host:
        return u
    out = torch.empty((len(rows) + len(host), u.shape[1]), dtype=u.dtype, device=u.device)
    out[torch.as_tensor(rows, device=u.device)] = u
    for i, px in host:
        out[i:i + 1] = e.encode_image(torch.from_numpy(px[None]), normalize=normalize).to(u.device)
    return out


def prepare_routed_batch(chunk, n_px, crop, pool=None, pinned=None, ragged=True):
    """Decode and route one batch of images the way ``PLIP.encode_images`` does: ``("tiles", uint8 [B,n,n,3])`` already at the model
    resolution, ``("resize", uint8 [B,H,W,3])`` one size, ``(("ragged", ...), blob)`` differing sizes (``ragged``), else
    ``("pixels", fp32 [B,3,n,n])`` from the host's Pillow path.  ``consume_routed_batch`` runs the result on an engine."""
    chunk = open_paths(chunk, pool)
    route, load = classify(chunk, n_px, ragged)
    if route == "ragged":
        return _ragged_prepare(chunk, load, n_px, crop, pool, pinned)
    if route == "host":
        one = lambda im: preprocess_image(im, n_px, crop)
        return "pixels", np.stack(list(pool.map(one, load)) if pool is not None else [one(c) for c in load])
    return route, load


def consume_routed_batch(e, tag, t, crop, normalize=False):
    if isinstance(tag, tuple):
        return _ragged_consume(e, tag, t, crop, normalize)
    if tag == "tiles":
        return e.encode_image_u8(t, normalize=normalize)
    if tag == "resize":
        return e.encode_image_u8(e.resize_crop_u8(t, crop=crop), normalize=normalize)
    return e.encode_image(t, normalize=normalize)


# ---- the direct loop ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def lane_loop(eng):
    """``Engine.lane_loop`` where the engine has one (a PlipModel's); any other engine object: every call on it, in order."""
    loop = getattr(eng, "lane_loop", None)
    if loop is None:
        yield lambda fn: fn(eng)
    else:
        with loop() as run:
            yield run


def _joins(route, load, first) -> bool:
    """May the [B, ...] payload ``load`` share a flush with the pending ones (``first``: the oldest)?  Same Python type, dtype and
    trailing shape; one-size batches of DIFFERENT source sizes also join -- each size is resized by itself, the tiles share the encode."""
    return type(load) is type(first) and load.dtype == first.dtype and (route == "resize" or load.shape[1:] == first.shape[1:])


def _encode_parts(e, route, parts, crop, caller):
    """The pending "tiles" / "resize" / "pixels" payloads of one flush, joined and run on engine ``e`` inside its lane.  Tensors the
    caller made on the device were produced on the ``caller`` stream: the lane's stream waits for it, and the allocator is told."""
    on_device = [p for p in parts if torch.is_tensor(p) and p.is_cuda]
    if on_device:
        lane = torch.cuda.current_stream(e.device)
        lane.wait_stream(caller)
        for p in on_device:
            p.record_stream(lane)

    def join(ps):                      # several payloads: uploaded one by one and joined on the device (no second copy on the host)
        ts = [p if torch.is_tensor(p) else torch.from_numpy(p) for p in ps]
        return ts[0] if len(ts) == 1 else torch.cat([t.to(e.device) for t in ts])

    sizes = [list(g) for _, g in itertools.groupby(parts, key=lambda p: tuple(p.shape[1:]))]
    if len(sizes) == 1:
        return consume_routed_batch(e, route, join(parts), crop)
    ups = [join(g).to(e.device) for g in sizes]        # ("resize", see _joins) every upload first: a synchronous copy enqueued behind a
    return e.encode_image_u8(torch.cat([e.resize_crop_u8(u, crop=crop) for u in ups]))         # resize would wait for its kernels


def encode_direct(images, batch_size, eng, n_px, cap, crop, ragged=False, fill_stage=None):
    """``images`` in caller batches of ``batch_size`` on ``eng`` (tile size ``n_px``) -> the embeddings of the engine calls, in order.
    Consecutive caller batches of one route are joined on the host, up to ``cap`` rows, and flushed when the route, the payload's
    Python type, trailing shape (``_joins``: but for one-size batches) or dtype changes or the rows would pass ``cap``; a flush is ONE
    call of the lane loop (consecutive calls alternate between the engine and a clone on a second stream, ``Engine.lane_loop``; a
    row's bits do not depend on the lane).
    ``fill_stage(tiles, n_px, cap)``: the caller's pinned staging rows for lists of native tiles (None: no such route)."""
    outs, pend, kind, rows, caller = [], [], None, 0, None

    def flush():
        nonlocal pend, kind, rows
        if kind == "stage":            # each tile copied ONCE, into the pinned rows; one H2D (synchronous: the rows may be refilled)
            stage = fill_stage(pend, n_px, cap)
            outs.append(run(lambda e: e.encode_image_u8(stage)))
        elif kind == "ragged":         # packed, copied, resized and encoded inside the lane's call
            outs.append(run(lambda e, imgs=pend: _encode_segments(e, [("ragged", imgs)], n_px, crop)))
        elif pend:
            outs.append(run(lambda e, k=kind, parts=pend: _encode_parts(e, k, parts, crop, caller)))
        pend, kind, rows = [], None, 0

    with torch.no_grad(), lane_loop(eng) as run:
        for s in range(0, len(images), batch_size):
            chunk = open_paths(images[s:s + batch_size])
            route, load = classify(chunk, n_px, ragged, stage=fill_stage is not None and len(chunk) <= cap)
            if route == "ragged" and len(load) > 1:        # some images keep the host path: the segments in order, in one lane call
                flush()
                outs.append(run(lambda e, segs=load: _encode_segments(e, segs, n_px, crop)))
                continue
            if route == "ragged":
                load = load[0][1]
            elif route == "host":
                route, load = "pixels", preprocess_images(load, n_px, crop=crop)
            listed = route in ("stage", "ragged")          # lists of images; the other payloads are [B, ...] arrays or tensors
            if kind is not None and (route != kind or rows + len(load) > cap or not (listed or _joins(route, load, pend[0]))):
                flush()
            if torch.is_tensor(load) and load.is_cuda and caller is None:
                caller = torch.cuda.current_stream(eng.device)
            pend.extend(load) if listed else pend.append(load)
            kind, rows = route, rows + len(load)
        flush()
    return outs
