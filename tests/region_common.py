"""What the slide-region tests share (tests/test_region_host.py, tests/test_gpu_region.py): the synthetic region, its four grids and
the numpy oracle of a whole ``encode_region`` call's selection, computed once.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import functools

import numpy as np

from plip_amd.preprocess import region_min_count, region_tile_counts

REGION_HW = (200, 331)                      # 331 pixels: a pitch of 993 bytes, odd -- every row starts at another alignment
BLOCK = (slice(20, 150), slice(40, 250))    # the "tissue": uniform random bytes; everything else is glass
# (origin, tile, stride) -> kept / total at min_tissue = 0.5: every grid has tiles that stay and tiles that go
GRIDS = {((3, 5), 64, 64): (6, 15), ((0, 0), 64, 40): (15, 28), ((3, 5), 64, 80): (4, 8), ((1, 2), 96, 96): (2, 6)}


@functools.lru_cache(maxsize=None)
def synthetic_region() -> np.ndarray:
    """uint8 [200,331,3]: glass = 240 + randint(-3, 4) per channel (bright and grey: never tissue), and a block of uniform random bytes
    (98.5 % of such pixels pass the rule)."""
    rs = np.random.RandomState(2024)
    H, W = REGION_HW
    region = (240 + rs.randint(-3, 4, size=(H, W, 3))).astype(np.uint8)
    region[BLOCK] = rs.randint(0, 256, size=region[BLOCK].shape, dtype=np.uint8)
    region.setflags(write=False)
    return region


@functools.lru_cache(maxsize=None)
def _selection(origin, t, s, min_tissue):
    region = synthetic_region()
    counts = region_tile_counts(region, t, s, origin)
    kept = np.flatnonzero(counts.reshape(-1) >= region_min_count(min_tissue, t)).astype(np.int64)
    rows, cols = counts.shape
    coords = np.stack([origin[0] + (kept // cols) * s, origin[1] + (kept % cols) * s], axis=1).astype(np.int64)
    for a in (counts, kept, coords):
        a.setflags(write=False)
    return counts, kept, coords


def oracle_selection(origin, t, s, min_tissue=0.5):
    """``(counts int32 [rows, cols], kept int64 [K] ascending, coords int64 [K,2])`` of the synthetic region, in numpy (read-only)."""
    return _selection(tuple(origin), int(t), int(s), float(min_tissue))


def host_crops(region: np.ndarray, coords: np.ndarray, t: int):
    """the kept tiles as a host list, what a caller of ``encode_images`` would cut"""
    return [np.ascontiguousarray(region[y:y + t, x:x + t]) for y, x in coords.tolist()]

