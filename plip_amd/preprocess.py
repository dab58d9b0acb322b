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


# ---------------------------------------------------------------------------------------------------------------
# Augmented views (include/plipmi.h plipmi_warp_u8, plip_amd/augment.py).  The reference's ``_train_transform``
# (reproducibility/embedders/transform.py:18-38) is RandomCrop -> RandomHorizontalFlip -> RandomAffine -> RandomPerspective on PIL
# images, and torchvision warps a PIL image with ``Image.transform(size, AFFINE | PERSPECTIVE, coeffs, BILINEAR, fillcolor=...)``.
# ``warp_reference`` restates that call (libImaging/Geometry.c: affine_transform / perspective_transform, bilinear_filter8) in numpy
# float64 -- every product and sum rounds once, as in the C -- and is the oracle of the kernel; the builders below are torchvision's
# ``_get_inverse_affine_matrix`` / ``_get_perspective_coeffs`` and the parameter ranges of the reference.  torchvision is not a
# dependency: these functions are the specification, and nothing claims parity with torch's random stream.
def check_perspective(coeffs, out_h: int, out_w: int) -> np.ndarray:
    """float64 [..., 8] perspective rows for an ``out_h x out_w`` output, refused by name (ValueError) when the denominator
    ``(a6 x + a7 y) + 1`` is not > 0 at the four corners (0, 0), (out_w, 0), (0, out_h), (out_w, out_h): it is linear, so it is then
    > 0 at every pixel.  Pillow leaves a denominator that vanishes inside the output undefined; such rows never reach a kernel."""
    a = np.asarray(coeffs, dtype=np.float64)
    if a.shape[-1] != 8:
        raise ValueError(f"perspective rows have 8 coefficients, got {a.shape}")
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.ones(a.shape[:-1], bool)
        for X, Y in ((0.0, 0.0), (float(out_w), 0.0), (0.0, float(out_h)), (float(out_w), float(out_h))):
            ok &= ((a[..., 6] * X + a[..., 7] * Y) + 1.0) > 0.0
    if not ok.all():
        bad = np.argwhere(~np.atleast_1d(ok))[0].tolist()
        raise ValueError(f"vanishing denominator: perspective row {bad} has (a6 x + a7 y) + 1 <= 0 (or not finite) at a corner of the "
                         f"{out_h} x {out_w} output")
    return a


def warp_reference(src: np.ndarray, coeffs, perspective: bool = False, out_size=None, fill=127, window=None) -> np.ndarray:
    """The oracle of ``plipmi_warp_u8`` for one image: uint8 [H,W,3] -> uint8 [oh,ow,3], byte for byte
    ``Image.fromarray(img).transform((ow, oh), AFFINE | PERSPECTIVE, coeffs, BILINEAR, fillcolor=fill)`` where ``img`` is the
    ``window`` = (wy, wx, wh, ww, flip) of ``src``, mirrored left-right when ``flip`` (default: all of ``src``).  ``coeffs``: 6 or 8
    float64 (affine reads the first six), the output -> input map of include/plipmi.h; ``fill`` an int or (r, g, b)."""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3:
        raise ValueError(f"warp_reference takes uint8 [H,W,3], got {src.dtype} {src.shape}")
    a = np.zeros(8, np.float64)
    c = np.asarray(coeffs, dtype=np.float64).reshape(-1)
    if c.size not in (6, 8) or (perspective and c.size != 8):
        raise ValueError(f"{c.size} coefficients: an affine row has 6 (or 8), a perspective row 8")
    a[:c.size] = c
    oh, ow = (src.shape[0], src.shape[1]) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if perspective:
        check_perspective(a, oh, ow)
    wy, wx, wh, ww, flip = (0, 0, src.shape[0], src.shape[1], 0) if window is None else (int(v) for v in window)
    if wy < 0 or wx < 0 or wh < 1 or ww < 1 or wy + wh > src.shape[0] or wx + ww > src.shape[1]:
        raise ValueError(f"window {(wy, wx, wh, ww)} does not lie inside the {src.shape[0]} x {src.shape[1]} source")
    img = src[wy:wy + wh, wx:wx + ww]
    if flip:
        img = img[:, ::-1]
    fill = np.asarray((fill,) * 3 if np.ndim(fill) == 0 else fill, dtype=np.uint8)
    xin = (np.arange(ow, dtype=np.float64) + 0.5)[None, :]
    yin = (np.arange(oh, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xs = (a[0] * xin + a[1] * yin) + a[2]
        ys = (a[3] * xin + a[4] * yin) + a[5]
        if perspective:
            den = (a[6] * xin + a[7] * yin) + 1.0
            xs, ys = xs / den, ys / den
        inside = (xs >= 0.0) & (xs < ww) & (ys >= 0.0) & (ys < wh)
    xs, ys = np.where(inside, xs, 0.5), np.where(inside, ys, 0.5)
    xf, yf = xs - 0.5, ys - 0.5
    x0, y0 = np.floor(xf), np.floor(yf)
    dx, dy = (xf - x0)[..., None], (yf - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    c0, c1 = np.clip(x0, 0, ww - 1), np.clip(x0 + 1, 0, ww - 1)
    r0 = np.clip(y0, 0, wh - 1)
    second = (y0 + 1 >= 0) & (y0 + 1 < wh)              # row y0 + 1 is not clipped: outside, the first row stands for it
    r1 = np.where(second, y0 + 1, r0)
    px = img.astype(np.float64)
    v1 = px[r0, c0] + (px[r0, c1] - px[r0, c0]) * dx
    v2 = np.where(second[..., None], px[r1, c0] + (px[r1, c1] - px[r1, c0]) * dx, v1)
    v = v1 + (v2 - v1) * dy
    return np.where(inside[..., None], v.astype(np.uint8), fill[None, None, :])        # (truncation; v is in [0, 255])


def affine_coeffs(center, angle_deg: float, translate, scale: float, shear_deg) -> np.ndarray:
    """float64 [6]: the output -> input map of a rotation by ``angle_deg`` about ``center`` = (cx, cy), a shear by ``shear_deg`` =
    (sx, sy) degrees, a ``scale`` and a translation by ``translate`` = (tx, ty) pixels -- the inverse of translate . centre .
    rotate-shear-scale . centre^-1, as torchvision's ``_get_inverse_affine_matrix`` writes it (the row ``F.affine`` hands to PIL;
    for an image of w x h pixels the centre is (w * 0.5, h * 0.5))."""
    import math
    cx, cy = (float(v) for v in center)
    tx, ty = (float(v) for v in translate)
    rot, sx, sy = math.radians(angle_deg), math.radians(shear_deg[0]), math.radians(shear_deg[1])
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [v / float(scale) for v in (d, -b, 0.0, -c, a, 0.0)]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty) + cx
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty) + cy
    return np.asarray(m, dtype=np.float64)


def perspective_coeffs(startpoints, endpoints) -> np.ndarray:
    """float64 [8]: the perspective row with ``start = H(end)`` for four point pairs (x, y) -- the output -> input map that
    sends each endpoint to its startpoint, torchvision's ``_get_perspective_coeffs`` as an 8 x 8 float64 solve.  Refused by name
    (ValueError): degenerate points, and a row whose denominator is not > 0 at all four endpoints (the quadrilateral is folded
    over: the denominator vanishes between its corners)."""
    s, e = np.asarray(startpoints, np.float64), np.asarray(endpoints, np.float64)
    if s.shape != (4, 2) or e.shape != (4, 2):
        raise ValueError(f"perspective_coeffs takes four (x, y) start and end points, got {s.shape} and {e.shape}")
    A = np.zeros((8, 8), np.float64)
    for i in range(4):
        A[2 * i] = [e[i, 0], e[i, 1], 1, 0, 0, 0, -s[i, 0] * e[i, 0], -s[i, 0] * e[i, 1]]
        A[2 * i + 1] = [0, 0, 0, e[i, 0], e[i, 1], 1, -s[i, 1] * e[i, 0], -s[i, 1] * e[i, 1]]
    try:
        a = np.linalg.solve(A, s.reshape(-1))
    except np.linalg.LinAlgError as err:
        raise ValueError(f"vanishing denominator: no perspective map sends {e.tolist()} to {s.tolist()} ({err})") from None
    den = (a[6] * e[:, 0] + a[7] * e[:, 1]) + 1.0
    if not (np.isfinite(a).all() and (den > 0.0).all()):
        raise ValueError(f"vanishing denominator: the map from {e.tolist()} to {s.tolist()} has (a6 x + a7 y) + 1 = {den.tolist()} at "
                         "the endpoints, not > 0 at all four")
    return a


def dihedral_coeffs(k: int, n: int) -> np.ndarray:
    """float64 [6], integer entries: symmetry ``k`` = 0 .. 7 of an n x n tile as an affine output -> input row.  View k of ``img`` is
    ``np.rot90(img if k < 4 else img[:, ::-1], k % 4)``: 0 the identity, 1 .. 3 the quarter turns, 4 the left-right flip
    ``[-1,0,n, 0,1,0]``, 5 .. 7 the flip followed by the turns.  Pixel centres map to pixel centres, so the warp is an exact
    re-index (dx = dy = 0 in ``warp_reference``)."""
    k, n = int(k), float(int(n))
    if not 0 <= k <= 7:
        raise ValueError(f"a square has eight symmetries, k = 0 .. 7; got {k}")
    rows = [[1, 0, 0, 0, 1, 0], [0, -1, n, 1, 0, 0], [-1, 0, n, 0, -1, n], [0, 1, 0, -1, 0, n],
            [-1, 0, n, 0, 1, 0], [0, 1, 0, 1, 0, 0], [1, 0, 0, 0, -1, n], [0, -1, n, -1, 0, n]]
    return np.asarray(rows[k], dtype=np.float64)


IDENTITY_ROW = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)     # as an affine and as a perspective row: the input's bytes exactly


def sample_train_params(seed: int, index: int, view: int, src_hw, n_px: int, degrees: float = 10.0, translate: float = 0.1,
                        scale=(0.8, 1.2), shear: float = 15.0, p_flip: float = 0.5, distortion: float = 0.3, p_perspective: float = 0.3):
    """The random draws of the reference's ``_train_transform`` (transform.py:23-38; its ranges are the keyword defaults) for view
    ``view`` of image ``index`` of ``src_hw`` = (H, W) pixels, H, W >= n_px -> ``(window, affine, perspective)``: int32 [5] (top, left,
    n_px, n_px, flip), float64 [8] (an affine row, a6 = a7 = 0) and float64 [8] (a perspective row; the identity when none is drawn).
    Every draw comes from ``np.random.default_rng([seed, index, view])`` in a fixed order, whatever is drawn: a view's bytes depend on
    (seed, index, view) alone, never on the batch size, the order or the lane.
    Crop: top, left uniform over the positions that fit.  Flip: p = ``p_flip``.  Affine about the crop's centre (n/2, n/2): angle
    U(-degrees, degrees); tx, ty = round(U(-translate n, translate n)); scale U(*scale); shears U(-shear, shear) each.  Perspective,
    p = ``p_perspective``: each corner of [[0,0],[n-1,0],[n-1,n-1],[0,n-1]] moves inward by an integer in [0, d] per axis, d =
    int(distortion * (n // 2))."""
    H, W = int(src_hw[0]), int(src_hw[1])
    n = int(n_px)
    if n < 1 or H < n or W < n:
        raise ValueError(f"a crop of {n} px does not fit a source of {H} x {W} pixels")
    rng = np.random.default_rng([int(seed), int(index), int(view)])
    top, left = int(rng.integers(0, H - n + 1)), int(rng.integers(0, W - n + 1))
    flip = int(rng.random() < p_flip)
    angle = float(rng.uniform(-degrees, degrees))
    tx, ty = (int(round(float(rng.uniform(-translate * n, translate * n)))) for _ in range(2))
    sc = float(rng.uniform(scale[0], scale[1]))
    shx, shy = float(rng.uniform(-shear, shear)), float(rng.uniform(-shear, shear))
    warp = bool(rng.random() < p_perspective)
    d = int(distortion * (n // 2))
    move = rng.integers(0, d + 1, size=(4, 2))
    affine = np.zeros(8, np.float64)
    affine[:6] = affine_coeffs((n * 0.5, n * 0.5), angle, (tx, ty), sc, (shx, shy))
    persp = np.asarray(IDENTITY_ROW, np.float64)
    if warp:
        start = np.asarray([[0, 0], [n - 1, 0], [n - 1, n - 1], [0, n - 1]], np.float64)
        end = start + move * np.asarray([[1, 1], [-1, 1], [-1, -1], [1, -1]], np.float64)
        persp = check_perspective(perspective_coeffs(start, end), n, n)
    return np.asarray([top, left, n, n, flip], np.int32), affine, persp


def train_params(seed: int, count: int, views: int, src_hw, n_px: int, first: int = 0, **ranges):
    """``sample_train_params`` for images ``first .. first + count`` and views ``0 .. views`` -> ``(windows int32 [count, views, 5],
    affine float64 [count, views, 8], perspective float64 [count, views, 8])``."""
    rows = [[sample_train_params(seed, first + i, v, src_hw, n_px, **ranges) for v in range(int(views))] for i in range(int(count))]
    shape = (int(count), int(views))
    return (np.asarray([[r[0] for r in row] for row in rows], np.int32).reshape(shape + (5,)),
            np.asarray([[r[1] for r in row] for row in rows], np.float64).reshape(shape + (8,)),
            np.asarray([[r[2] for r in row] for row in rows], np.float64).reshape(shape + (8,)))


def train_view_reference(src: np.ndarray, window, affine, perspective, fill=127) -> np.ndarray:
    """One view of the train chain in numpy, each stage through bytes as the PIL chain goes: crop + flip + affine, then perspective."""
    n = int(window[2])
    return warp_reference(warp_reference(src, affine, False, (n, n), fill, window), perspective, True, (n, n), fill)


# ---- Macenko stain normalisation: the definition csrc/stain.hip implements, in float64 numpy -----------------
STAIN_IO, STAIN_ALPHA, STAIN_BETA = 240.0, 1.0, 0.15
HE_REF = np.array([[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]], np.float64)     # Macenko's target stain vectors (H, E columns)
MAXC_REF = np.array([1.9705, 1.0308], np.float64)                                           # and 99th-percentile concentrations
STAIN_MIN_TISSUE = 16          # a fit over fewer tissue pixels is invalid
STAIN_MIN_DET = 1e-12          # and so is one whose det(HE^T HE) is not above this
STAIN_MAX_SAMPLES = 1 << 22    # PLIP.fit_stain's default step keeps the sampled pixels at or under this


def stain_lut(Io: float = STAIN_IO) -> np.ndarray:
    """float64 [256]: the optical density of a byte, ``-log((v + 1) / Io)``.  Built here and uploaded: the device takes no logarithm."""
    return -np.log((np.arange(256, dtype=np.float64) + 1.0) / np.float64(Io))


def stain_percentile(keys, q: float) -> float:
    """numpy's default (linear) percentile of float32 keys, written out: sort as float32, then in float64 ``r = (q / 100) (m - 1)``,
    ``l = floor(r)``, ``t = r - l`` and numpy's two-sided lerp between ``a[l]`` and ``a[min(l + 1, m - 1)]`` (``a + (b - a) t`` below
    ``t = 0.5``, ``b - (b - a)(1 - t)`` from there on), every operation rounded once.  NaN for no keys."""
    a = np.sort(np.asarray(keys, dtype=np.float32).reshape(-1)).astype(np.float64)
    m = a.size
    if m == 0:
        return float("nan")
    r = (np.float64(q) / np.float64(100.0)) * np.float64(m - 1)
    lo = int(np.floor(r))
    t = r - np.float64(lo)
    va, vb = a[min(lo, m - 1)], a[min(lo + 1, m - 1)]
    d = vb - va
    return float(va + d * t) if t < 0.5 else float(vb - d * (np.float64(1.0) - t))


def _stain_jacobi(cov: np.ndarray):
    """Cyclic Jacobi on a symmetric 3 x 3 (the rotation of Numerical Recipes' jacobi, at most 16 sweeps, pairs (0,1), (0,2), (1,2)) ->
    (eigenvalues [3], eigenvectors as columns [3,3]); the statement order is the kernel's."""
    A = np.array(cov, np.float64)
    V = np.eye(3)
    for _ in range(16):
        if A[0, 1] * A[0, 1] + A[0, 2] * A[0, 2] + A[1, 2] * A[1, 2] == 0.0:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p, q]
            if apq == 0.0:
                continue
            theta = (A[q, q] - A[p, p]) / (2.0 * apq)
            with np.errstate(over="ignore"):                 # (theta^2 may pass the range: then t = 0, as on the device)
                t = 1.0 / (abs(theta) + np.sqrt(theta * theta + 1.0))
            if theta < 0.0:
                t = -t
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            r = 3 - p - q
            A[p, p] = A[p, p] - t * apq
            A[q, q] = A[q, q] + t * apq
            A[p, q] = A[q, p] = 0.0
            arp, arq = A[r, p], A[r, q]
            A[r, p] = A[p, r] = c * arp - s * arq
            A[r, q] = A[q, r] = s * arp + c * arq
            for k in range(3):
                vkp, vkq = V[k, p], V[k, q]
                V[k, p] = c * vkp - s * vkq
                V[k, q] = s * vkp + c * vkq
    return np.array([A[0, 0], A[1, 1], A[2, 2]]), V


def _stain_samples(images: np.ndarray, step: int) -> np.ndarray:
    """uint8 [B,H,W,3] -> the sampled pixels (y % step == 0 and x % step == 0) of every image, in image, row, column order: [B, ns, 3]"""
    x = np.asarray(images)
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3:
        raise ValueError(f"stain images are uint8 [B,H,W,3], got {x.dtype} {tuple(x.shape)}")
    if int(step) < 1:
        raise ValueError(f"step must be at least 1, got {step}")
    x = x[:, ::int(step), ::int(step)]
    return x.reshape(x.shape[0], -1, 3)


def _stain_fit_pixels(px: np.ndarray, Io: float, alpha: float, beta: float) -> np.ndarray:
    """One fit over pixels uint8 [m, 3] -> the float64 [16] row of ``plipmi_stain_fit``: HE [3,2], P [2,3], maxC [2], n, valid."""
    row = np.zeros(16, np.float64)
    od = stain_lut(Io)[px]                                            # [m, 3]
    tissue = ~(od < beta).any(axis=1)
    n = int(tissue.sum())
    row[14] = n
    if n < STAIN_MIN_TISSUE:
        return row
    odt = od[tissue]
    s1 = odt.sum(axis=0)
    cov = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            cov[i, j] = ((odt[:, i] * odt[:, j]).sum() - s1[i] * s1[j] / n) / (n - 1)
    w, V = _stain_jacobi(cov)
    i1 = int(np.argmax(w))                                            # (ties: the lower index, as the kernel)
    rest = [i for i in range(3) if i != i1]
    i2 = rest[0] if w[rest[0]] >= w[rest[1]] else rest[1]
    e = np.stack([V[:, i1], V[:, i2]], axis=1)                        # [3, 2]
    for j in range(2):
        if (e[0, j] + e[1, j]) + e[2, j] < 0.0:
            e[:, j] = -e[:, j]
    t0 = (odt[:, 0] * e[0, 0] + odt[:, 1] * e[1, 0]) + odt[:, 2] * e[2, 0]
    t1 = (odt[:, 0] * e[0, 1] + odt[:, 1] * e[1, 1]) + odt[:, 2] * e[2, 1]
    phi = np.arctan2(t1, t0).astype(np.float32)
    lo, hi = stain_percentile(phi, alpha), stain_percentile(phi, 100.0 - alpha)
    v1 = e[:, 0] * np.cos(lo) + e[:, 1] * np.sin(lo)
    v2 = e[:, 0] * np.cos(hi) + e[:, 1] * np.sin(hi)
    HE = np.stack([v1, v2], axis=1) if v1[0] > v2[0] else np.stack([v2, v1], axis=1)
    a = (HE[0, 0] * HE[0, 0] + HE[1, 0] * HE[1, 0]) + HE[2, 0] * HE[2, 0]
    b = (HE[0, 0] * HE[0, 1] + HE[1, 0] * HE[1, 1]) + HE[2, 0] * HE[2, 1]
    d = (HE[0, 1] * HE[0, 1] + HE[1, 1] * HE[1, 1]) + HE[2, 1] * HE[2, 1]
    det = a * d - b * b
    if not det > STAIN_MIN_DET:
        return row
    P = np.stack([(d * HE[:, 0] - b * HE[:, 1]) / det, (a * HE[:, 1] - b * HE[:, 0]) / det])      # [2, 3]
    maxc = np.zeros(2)
    for j in range(2):
        c = (P[j, 0] * od[:, 0] + P[j, 1] * od[:, 1]) + P[j, 2] * od[:, 2]                         # every sampled pixel, glass included
        maxc[j] = stain_percentile(c.astype(np.float32), 99.0)
    if not (maxc[0] > 0.0 and maxc[1] > 0.0):
        return row
    row[0:6], row[6:12], row[12:14], row[15] = HE.reshape(-1), P.reshape(-1), maxc, 1.0
    return row


def stain_fit_reference(images, pooled: bool = False, step: int = 1, Io: float = STAIN_IO, alpha: float = STAIN_ALPHA,
                        beta: float = STAIN_BETA) -> np.ndarray:
    """Macenko fits of uint8 [B,H,W,3] (or one [H,W,3]) over the sampled pixels -> float64 [F, 16], F = 1 if ``pooled`` else B.  A row:
    HE [3,2] row-major (haematoxylin column first), P = (HE^T HE)^-1 HE^T [2,3], maxC [2], the tissue count n, the valid flag; an
    invalid fit (n < 16, det(HE^T HE) not > 1e-12, a maxC not > 0) keeps n and is zero elsewhere."""
    x = np.asarray(images)
    px = _stain_samples(x[None] if x.ndim == 3 else x, step)
    if pooled:
        px = px.reshape(1, -1, 3)
    return np.stack([_stain_fit_pixels(p, Io, alpha, beta) for p in px]) if len(px) else np.zeros((0, 16), np.float64)


def stain_target(target=None) -> np.ndarray:
    """float64 [8] = target HE [3,2] row-major, then target maxC [2]: None = Macenko's reference, else a fit row [16] / [1,16]"""
    if target is None:
        return np.concatenate([HE_REF.reshape(-1), MAXC_REF])
    t = np.asarray(target, np.float64).reshape(-1)
    if t.size == 16:
        return np.concatenate([t[0:6], t[12:14]])
    if t.size != 8:
        raise ValueError(f"a stain target is 8 values (HE [3,2], maxC [2]) or a fit row of 16, got {t.size}")
    return t.copy()


def stain_apply_reference(images, fits, target=None, Io: float = STAIN_IO, unrounded: bool = False) -> np.ndarray:
    """uint8 [B,H,W,3] normalised by ``fits`` float64 [B,16] (or [1,16] for all) to ``target`` (``stain_target``): per pixel
    C = P . OD, C2 = C * (maxC_target / maxC), out = min(255, Io exp(-(HE_target . C2))) truncated to a byte, each operation rounded
    once in the order written here; an image whose fit is invalid comes back unchanged.  ``unrounded``: the float64 values
    ``Io exp(...)`` before the clip and the truncation instead -- how far a byte is from the next one (an invalid image's are its own
    bytes)."""
    x = np.asarray(images)
    single = x.ndim == 3
    x = x[None] if single else x
    fits = np.asarray(fits, np.float64).reshape(-1, 16)
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3:
        raise ValueError(f"stain images are uint8 [B,H,W,3], got {x.dtype} {tuple(x.shape)}")
    if fits.shape[0] not in (1, x.shape[0]):
        raise ValueError(f"need 1 or {x.shape[0]} fits, got {fits.shape[0]}")
    tg = stain_target(target)
    lut = stain_lut(Io)
    out = np.empty(x.shape, np.float64)
    for b in range(x.shape[0]):
        f = fits[b if fits.shape[0] > 1 else 0]
        if f[15] == 0.0:
            out[b] = x[b]
            continue
        od = lut[x[b]]
        P = f[6:12].reshape(2, 3)
        c2 = [((P[j, 0] * od[..., 0] + P[j, 1] * od[..., 1]) + P[j, 2] * od[..., 2]) * (tg[6 + j] / f[12 + j]) for j in range(2)]
        for ch in range(3):
            v = np.float64(Io) * np.exp(-(tg[2 * ch] * c2[0] + tg[2 * ch + 1] * c2[1]))
            out[b, ..., ch] = v if unrounded else np.where(v < 255.0, v, 255.0)
    if not unrounded:
        out = out.astype(np.uint8)
    return out[0] if single else out


def stain_default_step(B: int, H: int, W: int) -> int:
    """the smallest step at which the sampled pixels of B images of H x W, B * ceil(H / step) * ceil(W / step), are at most 2^22"""
    if B > STAIN_MAX_SAMPLES:
        raise ValueError(f"{B} images: even one sample of each passes {STAIN_MAX_SAMPLES}")
    step = max(1, int(np.sqrt(B * H * W / STAIN_MAX_SAMPLES)) - 1)
    while B * (-(-H // step)) * (-(-W // step)) > STAIN_MAX_SAMPLES:
        step += 1
    return step


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
