"""What the augmented-view tests share (tests/test_augment_host.py, tests/test_gpu_augment.py): random warp rows, the Pillow calls the
numpy oracle is pinned to, and the train chain through PIL.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

from plip_amd.preprocess import affine_coeffs, check_perspective, perspective_coeffs

FILL = (127, 5, 250)          # three different channels: a swapped or dropped channel shows


def pil():
    """PIL.Image, or None where Pillow is not installed"""
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def random_affine_row(rs, w, h, strong=False):
    """an affine output -> input row [8] for a w x h image: RandomAffine's ranges, or well past them"""
    k = 4.0 if strong else 1.0
    row = np.zeros(8, np.float64)
    row[:6] = affine_coeffs((w * 0.5, h * 0.5), rs.uniform(-10 * k, 10 * k), (rs.uniform(-0.1, 0.1) * w * k, rs.uniform(-0.1, 0.1) * h * k),
                            rs.uniform(0.8, 1.2) if not strong else rs.uniform(0.3, 2.5), (rs.uniform(-15, 15) * k / 2, rs.uniform(-15, 15) * k / 2))
    return row


def random_perspective_row(rs, w, h, distortion=0.3):
    """a perspective row [8]: each corner of the w x h image moved inward by up to distortion / 2 of the side, as RandomPerspective"""
    dw, dh = distortion * w / 2, distortion * h / 2
    start = np.asarray([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
    end = start + np.asarray([[rs.uniform(0, dw), rs.uniform(0, dh)], [-rs.uniform(0, dw), rs.uniform(0, dh)],
                              [-rs.uniform(0, dw), -rs.uniform(0, dh)], [rs.uniform(0, dw), -rs.uniform(0, dh)]])
    return perspective_coeffs(start, end)


def pil_warp(src, row, perspective, out_hw, fill=FILL, window=None):
    """the call torchvision makes: (crop -> transpose ->) Image.transform(size, AFFINE | PERSPECTIVE, coeffs, BILINEAR, fillcolor)"""
    Image = pil()
    im = Image.fromarray(np.ascontiguousarray(src))
    if window is not None:
        wy, wx, wh, ww, flip = (int(v) for v in window)
        im = im.crop((wx, wy, wx + ww, wy + wh))
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
    fill = (fill,) * 3 if np.ndim(fill) == 0 else tuple(int(v) for v in fill)
    data = [float(v) for v in (row if perspective else row[:6])]
    out = im.transform((int(out_hw[1]), int(out_hw[0])), Image.PERSPECTIVE if perspective else Image.AFFINE, data, Image.BILINEAR,
                       fillcolor=fill)
    return np.asarray(out, dtype=np.uint8)


def pil_train_view(src, window, affine, persp, fill=127):
    """the reference's chain on a PIL image, each stage through bytes: crop -> flip -> affine -> perspective"""
    n = int(window[2])
    return pil_warp(pil_warp(src, affine, False, (n, n), fill, window), persp, True, (n, n), fill)


def random_cases(seed=11, count=44):
    """(src, row, perspective, (oh, ow)) for ``count`` random warps: sources 5 .. 70 px, non-square outputs 4 .. 48 px, both modes,
    a quarter of them well past the train ranges"""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(count):
        h, w = int(rs.randint(5, 71)), int(rs.randint(5, 71))
        oh, ow = int(rs.randint(4, 49)), int(rs.randint(4, 49))
        if oh == ow:
            ow += 1
        src = rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8)
        perspective = i % 2 == 1
        while True:          # (a strongly distorted quadrilateral may fold over, or its denominator vanish inside a larger output: redraw)
            try:
                row = random_perspective_row(rs, w, h, 0.9 if i % 4 == 3 else 0.3) if perspective else random_affine_row(rs, w, h, strong=i % 4 == 2)
                if perspective:
                    check_perspective(row, oh, ow)
                break
            except ValueError:
                continue
        out.append((src, row, perspective, (oh, ow)))
    return out
