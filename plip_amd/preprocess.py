"""Input contract of the path: CLIP image preprocessing and the tokenizer hook.

``_transform`` in reproducibility/embedders/transform.py:45-52 and HF
``CLIPImageProcessor`` (image_processing_pil_clip.py:23-34) are the same pipeline:
resize(shortest edge -> n_px, bicubic) -> center crop n_px -> RGB -> /255 ->
normalise with the CLIP mean/std -> CHW float32.  For tiles that are already
n_px x n_px it reduces exactly to ``(u8/255 - mean)/std``.
"""
from __future__ import annotations

from typing import Callable, List, Sequence, Union

import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)   # transform.py:50
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def crop_offset(extent: int, n_px: int, rule: str = "torchvision") -> int:
    """First row/column of the centre crop.  The two preprocessing front ends of the reference disagree by one
    pixel when the excess is odd: torchvision ``CenterCrop`` (OpenAI ``_transform``,
    reproducibility/embedders/transform.py:47) uses ``int(round((extent - n) / 2.0))`` (round-half-to-even), HF
    ``CLIPImageProcessor.center_crop`` behind ``self.preprocess`` (plip.py:27,35) uses ``(extent - n) // 2``."""
    if rule == "hf":
        return (extent - n_px) // 2
    if rule == "torchvision":
        return int(round((extent - n_px) / 2.0))
    raise ValueError(f"unknown crop rule {rule!r} (expected 'hf' or 'torchvision')")


def preprocess_image(img, n_px: int = 224, crop: str = "torchvision") -> np.ndarray:
    """PIL image / path / HWC uint8 array -> float32 [3, n_px, n_px].  ``crop``: see :func:`crop_offset`
    ("torchvision" = ``_transform`` of reproducibility/, "hf" = the ``CLIPProcessor`` of the top-level PLIP)."""
    from PIL import Image
    if isinstance(img, str):
        img = Image.open(img)
    if isinstance(img, np.ndarray):
        img = Image.fromarray(img)
    img = img.convert("RGB")
    w, h = img.size
    if (w, h) != (n_px, n_px):
        short = min(w, h)
        # torchvision Resize(int): shortest edge -> n_px, long edge int(n_px * long / short)
        nw, nh = (n_px, int(n_px * h / w)) if w == short else (int(n_px * w / h), n_px)
        img = img.resize((nw, nh), resample=Image.BICUBIC)
        left, top = crop_offset(nw, n_px, crop), crop_offset(nh, n_px, crop)
        img = img.crop((left, top, left + n_px, top + n_px))
    x = np.asarray(img, dtype=np.float32) / np.float32(255.0)
    x = (x - np.asarray(CLIP_MEAN, dtype=np.float32)) / np.asarray(CLIP_STD, dtype=np.float32)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


# ---------------------------------------------------------------------------------------------------------------
# GPU-side resize + centre crop.  Pillow's ``Image.resize(BICUBIC)`` on 8-bit images is
# integer arithmetic once its coefficient tables exist (libImaging/Resample.c: precompute_coeffs,
# normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc): per output pixel a window [xmin, xmin+n) of
# input pixels, weights = bicubic(a = -0.5) sampled at the window's pixel centres, normalised, rounded to 22-bit fixed
# point; each pass accumulates int32 from 2^21 and shifts right by 22 with a clamp to 0..255, horizontal pass first,
# uint8 in between.  The tables are built here in float64 exactly as published; the two integer passes run in
# libplipmi.so (plipmi_resize_crop_u8) and are therefore bit-identical to Pillow (tests/test_host.py emulates the
# passes in numpy against Pillow itself, tests/test_gpu_api.py checks the kernel against Pillow).
# ---------------------------------------------------------------------------------------------------------------
_PRECISION_BITS = 32 - 8 - 2


def _bicubic(x: np.ndarray) -> np.ndarray:
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0,
                    np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


def resample_coeffs(in_size: int, out_size: int):
    """Pillow's 8-bit bicubic tables for one axis: ``bounds`` int32 [out, 2] = (first input index, tap count) and
    ``kk`` int32 [out, ksize] fixed-point weights (zero beyond the tap count)."""
    scale = float(np.float32(in_size) - np.float32(0.0)) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)           # C (int) cast: truncation of a non-negative value
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = _bicubic((np.arange(xmax, dtype=np.float64) + xmin - center + 0.5) * ss)
        ww = w.sum()
        if ww != 0.0:
            w = w / ww
        fixed = np.where(w < 0, -0.5 + w * (1 << _PRECISION_BITS), 0.5 + w * (1 << _PRECISION_BITS))
        kk[xx, :xmax] = np.trunc(fixed).astype(np.int64).astype(np.int32)
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def resize_crop_plan(w: int, h: int, n_px: int = 224, crop: str = "torchvision"):
    """Everything ``plipmi_resize_crop_u8`` needs for [h, w, 3] uint8 images: torchvision ``Resize(n_px)`` geometry
    (shortest edge -> n_px, long edge ``int(n_px * long / short)``; HF's ``get_resize_output_image_size`` gives the
    same numbers), centre-crop offsets by ``crop`` rule (:func:`crop_offset`), and the two coefficient tables
    restricted to the crop window.  ``None`` entries mean that pass is an identity (Pillow skips it too)."""
    short = min(w, h)
    nw, nh = (n_px, int(n_px * h / w)) if w == short else (int(n_px * w / h), n_px)
    if nw < n_px or nh < n_px:
        raise ValueError(f"image {w}x{h} is too small to crop {n_px}x{n_px} after the resize")
    left, top = crop_offset(nw, n_px, crop), crop_offset(nh, n_px, crop)
    plan = dict(w=w, h=h, n_px=n_px, nw=nw, nh=nh, left=left, top=top, xb=None, xk=None, yb=None, yk=None)
    if nw != w:
        b, k = resample_coeffs(w, nw)
        plan["xb"], plan["xk"] = np.ascontiguousarray(b[left:left + n_px]), np.ascontiguousarray(k[left:left + n_px])
    if nh != h:
        b, k = resample_coeffs(h, nh)
        plan["yb"], plan["yk"] = np.ascontiguousarray(b[top:top + n_px]), np.ascontiguousarray(k[top:top + n_px])
    return plan


def resize_crop_reference(img_u8: np.ndarray, plan) -> np.ndarray:
    """numpy emulation of the two integer passes (what the HIP kernels do); [h, w, 3] uint8 -> [n, n, 3] uint8."""
    n = plan["n_px"]
    src = img_u8.astype(np.int64)
    half = 1 << (_PRECISION_BITS - 1)
    if plan["xb"] is not None:
        tmp = np.empty((src.shape[0], n, 3), np.int64)
        for x in range(n):
            x0, cnt = plan["xb"][x]
            acc = (src[:, x0:x0 + cnt, :] * plan["xk"][x, :cnt].astype(np.int64)[None, :, None]).sum(axis=1) + half
            tmp[:, x, :] = np.clip(acc >> _PRECISION_BITS, 0, 255)
    else:
        tmp = src[:, plan["left"]:plan["left"] + n, :]
    if plan["yb"] is not None:
        out = np.empty((n, n, 3), np.int64)
        for y in range(n):
            y0, cnt = plan["yb"][y]
            acc = (tmp[y0:y0 + cnt, :, :] * plan["yk"][y, :cnt].astype(np.int64)[:, None, None]).sum(axis=0) + half
            out[y] = np.clip(acc >> _PRECISION_BITS, 0, 255)
    else:
        out = tmp[plan["top"]:plan["top"] + n]
    return out.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# Ragged batches (plipmi_resize_crop_u8_ragged): images of differing sizes packed end to end, geometry and coefficient
# tables computed on the device.  The host only packs bytes and sizes buffers; the functions below are that packing, the
# limits the C entry checks, and the CPU oracle of the whole call.
# ---------------------------------------------------------------------------------------------------------------
RAGGED_MAX_RATIO = 64          # largest in / out ratio of an axis the device entry takes (csrc/resize_ragged.h)


def _as_rgb_u8(img) -> np.ndarray:
    """array or PIL image -> uint8 [h, w, 3]; anything that is not RGB uint8 goes through ``.convert("RGB")``, as the
    reference's datasets do (reproducibility/dataset_loading/internal_datasets.py:42)."""
    if isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3:
        return img
    if isinstance(img, np.ndarray):
        if img.dtype != np.uint8:
            raise TypeError(f"pack_ragged takes uint8 arrays or PIL images, got an array of {img.dtype}")
        from PIL import Image
        img = Image.fromarray(img)
    return np.asarray(img.convert("RGB"), dtype=np.uint8)


def resize_output_size(h: int, w: int, n_px: int):
    """(nh, nw) of torchvision ``Resize(n_px)``: shortest edge -> n_px, long edge ``int(n_px * long / short)``."""
    return (int(n_px * h / w), n_px) if w <= h else (n_px, int(n_px * w / h))


def ragged_supported(h: int, w: int, n_px: int) -> bool:
    """Whether the device entry takes an h x w image: both sides at least 1 and no in / out ratio above RAGGED_MAX_RATIO."""
    if h < 1 or w < 1:
        return False
    nh, nw = resize_output_size(h, w, n_px)
    return h / nh <= RAGGED_MAX_RATIO and w / nw <= RAGGED_MAX_RATIO


def ragged_ksize(hw, n_px: int) -> int:
    """Taps per coefficient row for a batch of sizes ``hw`` [B, 2] = (h, w): ``2 * ceil(2 * max(scale, 1)) + 1`` at the batch's
    largest per-axis scale -- the row width ``resample_coeffs`` gives that axis."""
    hw = np.asarray(hw, dtype=np.int64).reshape(-1, 2)
    if hw.shape[0] == 0 or int(hw.min()) < 1:       # (a side below 1 is refused by the C entry whatever the row width)
        return 5
    h, w = hw[:, 0], hw[:, 1]
    tall = w <= h
    nh = np.where(tall, (n_px * h / w).astype(np.int64), n_px)          # int(n_px * long / short): true division, truncated
    nw = np.where(tall, n_px, (n_px * w / h).astype(np.int64))
    scale = np.concatenate([h.astype(np.float32).astype(np.float64) / nh, w.astype(np.float32).astype(np.float64) / nw])
    return int(np.ceil(2.0 * max(float(scale.max()), 1.0))) * 2 + 1


def pack_ragged(images: Sequence, out: "np.ndarray | None" = None):
    """Arrays / PIL images of any sizes -> ``(buf uint8 [sum h*w*3], offsets int64 [B], hw int32 [B, 2])``: the images' RGB bytes
    end to end, image b at ``buf[offsets[b]:]`` with ``hw[b] = (h, w)``.  ``out``: a uint8 buffer to pack into (a pinned staging
    buffer); ``buf`` is then its leading slice."""
    arrs = [_as_rgb_u8(im) for im in images]
    hw = np.asarray([a.shape[:2] for a in arrs], dtype=np.int32).reshape(len(arrs), 2)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    offsets = np.zeros(len(arrs), np.int64)
    if len(arrs) > 1:
        np.cumsum(sizes[:-1], out=offsets[1:])
    total = int(sizes.sum())
    buf = np.empty(total, np.uint8) if out is None else out[:total]
    if buf.shape[0] != total:
        raise ValueError(f"pack_ragged: the output buffer holds {0 if out is None else out.shape[0]} bytes, the images need {total}")
    for a, o, sz in zip(arrs, offsets.tolist(), sizes.tolist()):
        buf[o:o + sz] = a.reshape(-1)
    return buf, offsets, hw


def resize_crop_ragged_reference(images: Sequence, n_px: int = 224, crop: str = "torchvision") -> np.ndarray:
    """CPU oracle of the ragged entry: :func:`resize_crop_reference` per image -> uint8 [B, n_px, n_px, 3]."""
    out = np.zeros((len(images), n_px, n_px, 3), np.uint8)
    for i, im in enumerate(images):
        a = _as_rgb_u8(im)
        out[i] = resize_crop_reference(a, resize_crop_plan(a.shape[1], a.shape[0], n_px, crop))
    return out


# ---------------------------------------------------------------------------------------------------------------
# Slide regions (plipmi_region_select / plipmi_region_gather): the tissue rule and the tile grid, written ONCE here in numpy.  The
# kernels restate them (csrc/region.hip) and the tests hold the kernels to these functions; the rule is integer arithmetic only, so
# there is nothing to round.
# ---------------------------------------------------------------------------------------------------------------
TISSUE_DEFAULTS = dict(sat_min=18, luma_min=25, luma_max=235)


def check_tissue_thresholds(sat_min: int, luma_min: int, luma_max: int) -> None:
    for name, v in (("sat_min", sat_min), ("luma_min", luma_min), ("luma_max", luma_max)):
        if int(v) != v or not 0 <= int(v) <= 255:
            raise ValueError(f"{name} must be an integer in 0 .. 255, got {v!r}")


def tissue_mask(rgb: np.ndarray, sat_min: int = 18, luma_min: int = 25, luma_max: int = 235) -> np.ndarray:
    """uint8 [..., 3] RGB -> bool [...]: a pixel is tissue iff it is coloured enough, ``255 (mx - mn) >= sat_min * mx`` with ``mx`` /
    ``mn`` the largest / smallest of its channels, and neither dark nor blank, ``luma_min <= (77 r + 150 g + 29 b + 128) >> 8 <=
    luma_max``.  Glass is bright and grey, pen marks and the slide's edge are dark."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.shape[-1] != 3:
        raise ValueError(f"tissue_mask takes uint8 [..., 3], got {rgb.dtype} {rgb.shape}")
    check_tissue_thresholds(sat_min, luma_min, luma_max)
    x = rgb.astype(np.int32)
    mx, mn = x.max(axis=-1), x.min(axis=-1)
    luma = (77 * x[..., 0] + 150 * x[..., 1] + 29 * x[..., 2] + 128) >> 8
    return (255 * (mx - mn) >= int(sat_min) * mx) & (luma >= int(luma_min)) & (luma <= int(luma_max))


def region_grid(H: int, W: int, tile_px: int, stride: int, origin=(0, 0)):
    """``(rows, cols)`` of the tiles of ``tile_px`` pixels, one every ``stride``, that fit an ``H x W`` region from ``origin`` =
    (y0, x0): tile (i, j) has its top-left pixel at (y0 + i * stride, x0 + j * stride) and the flat index i * cols + j; tiles that do
    not fit are dropped; either number is 0 when not even one fits."""
    y0, x0 = (int(v) for v in origin)
    t, s = int(tile_px), int(stride)
    if t < 1 or s < 1 or y0 < 0 or x0 < 0:
        raise ValueError(f"tile_px {tile_px}, stride {stride}, origin {origin}: need tile_px >= 1, stride >= 1 and an origin >= (0, 0)")
    rows = (int(H) - y0 - t) // s + 1 if int(H) - y0 - t >= 0 else 0
    cols = (int(W) - x0 - t) // s + 1 if int(W) - x0 - t >= 0 else 0
    return rows, cols


def region_min_count(min_tissue: float, tile_px: int) -> int:
    """The tissue pixels a tile of ``tile_px`` needs to be kept: ``ceil(min_tissue * tile_px ** 2)``, never below 0."""
    import math
    if not min_tissue == min_tissue:
        raise ValueError("min_tissue is NaN")
    return max(0, min(int(math.ceil(float(min_tissue) * int(tile_px) ** 2)), 2 ** 31 - 1))


def region_tile_counts(region: np.ndarray, tile_px: int, stride: int, origin=(0, 0), **thresholds) -> np.ndarray:
    """The oracle of ``plipmi_region_select``'s counts: int32 [rows, cols], tissue pixels per tile of :func:`region_grid`."""
    rows, cols = region_grid(region.shape[0], region.shape[1], tile_px, stride, origin)
    mask = tissue_mask(region, **thresholds)
    out = np.zeros((rows, cols), np.int32)
    for i in range(rows):
        for j in range(cols):
            y, x = origin[0] + i * stride, origin[1] + j * stride
            out[i, j] = int(mask[y:y + tile_px, x:x + tile_px].sum())
    return out


def preprocess_images(images: Sequence, n_px: int = 224, crop: str = "torchvision") -> np.ndarray:
    return np.stack([preprocess_image(i, n_px, crop) for i in images]) if len(images) else \
        np.zeros((0, 3, n_px, n_px), np.float32)


def load_tokenizer(path: str) -> Callable[[List[str], int], "np.ndarray"]:
    """CLIP BPE tokenizer from a local HF model dir (vocab.json + merges.txt).  Returns
    ``fn(texts, context_length) -> (ids int64 [N,ctx], mask int64 [N,ctx])`` padded/truncated
    the way plip.py:57-58 asks (max_length=77, padding="max_length", truncation=True)."""
    from transformers import CLIPTokenizer
    tok = CLIPTokenizer.from_pretrained(path)

    def fn(texts, context_length=77):
        enc = tok(list(texts), return_tensors="np", max_length=context_length, padding="max_length",
                  truncation=True)
        return enc["input_ids"].astype(np.int64), enc["attention_mask"].astype(np.int64)

    return fn
