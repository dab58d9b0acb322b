"""CPU-side checks of slide regions (include/plipmi.h plipmi_region_select / plipmi_region_gather, PLIP.encode_region): the numpy
oracle of the tissue rule and the grid, the rounding of the threshold, the C-ABI declarations and bindings, and what
``encode_region`` refuses before it touches a device.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest
import torch

import helpers as Hh
from region_common import BLOCK, GRIDS, REGION_HW, oracle_selection, synthetic_region

from plip_amd.preprocess import region_grid, region_min_count, region_tile_counts, tissue_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tissue_rule_on_hand_computed_pixels():
    """(220,160,200) pink: mx - mn = 60, 255 * 60 = 15300 >= 18 * 220 = 3960; luma = (16940 + 24000 + 5800 + 128) >> 8 = 183: tissue.
    Black: saturation passes (0 >= 0) but luma 0 < 25.  White: 0 >= 18 * 255 fails.  (243,238,240) glass: 255 * 5 = 1275 < 18 * 243 =
    4374, and its luma 240 is above 235 too."""
    px = np.array([[220, 160, 200], [0, 0, 0], [255, 255, 255], [243, 238, 240]], np.uint8)
    assert tissue_mask(px).tolist() == [True, False, False, False]
    assert (77 * 220 + 150 * 160 + 29 * 200 + 128) >> 8 == 183 and (77 * 243 + 150 * 238 + 29 * 240 + 128) >> 8 == 240
    # each condition alone decides: the thresholds are arguments
    assert tissue_mask(px, sat_min=0, luma_min=0, luma_max=255).all()
    assert tissue_mask(px, luma_min=0).tolist() == [True, True, False, False]
    assert tissue_mask(px, sat_min=5, luma_max=240).tolist() == [True, False, False, True]       # 1275 >= 5 * 243, luma 240 <= 240
    assert tissue_mask(px, sat_min=5, luma_max=239).tolist() == [True, False, False, False]
    assert tissue_mask(px.reshape(2, 2, 3)).shape == (2, 2)
    for bad in (dict(sat_min=256), dict(luma_min=-1), dict(luma_max=300)):
        with pytest.raises(ValueError):
            tissue_mask(px, **bad)
    with pytest.raises(ValueError):
        tissue_mask(px.astype(np.float32))


def test_region_grid_counts():
    H, W = REGION_HW
    assert [region_grid(H, W, t, s, o) for (o, t, s) in GRIDS] == [(3, 5), (4, 7), (2, 4), (2, 3)]
    assert [r * c for r, c in (region_grid(H, W, t, s, o) for (o, t, s) in GRIDS)] == [n for _, n in GRIDS.values()]
    assert region_grid(64, 64, 64, 64) == (1, 1) and region_grid(64, 63, 64, 64) == (1, 0) and region_grid(63, 64, 64, 1) == (0, 1)
    assert region_grid(64, 64, 64, 64, (1, 0)) == (0, 1) and region_grid(10, 10, 3, 1) == (8, 8) and region_grid(10, 10, 3, 7) == (2, 2)
    assert region_grid(10, 10, 3, 8) == (1, 1) and region_grid(500, 700, 224, 224) == (2, 3)
    for bad in (dict(tile_px=0, stride=1), dict(tile_px=4, stride=0), dict(tile_px=4, stride=4, origin=(-1, 0))):
        with pytest.raises(ValueError):
            region_grid(10, 10, **bad)


def test_min_count_rounds_up():
    assert region_min_count(0.5, 64) == 2048 and region_min_count(0.5, 3) == 5 and region_min_count(0.5, 1) == 1
    assert region_min_count(0.0, 64) == 0 and region_min_count(1.0, 64) == 4096 and region_min_count(1e-9, 64) == 1
    assert region_min_count(0.25, 96) == 2304 and region_min_count(1 / 3, 3) == 3 and region_min_count(-1.0, 8) == 0
    assert region_min_count(1.5, 8) == 96          # above 1: nothing can be kept, and nothing overflows
    with pytest.raises(ValueError):
        region_min_count(float("nan"), 8)


def test_synthetic_region_has_kept_and_dropped_tiles_in_every_grid():
    region = synthetic_region()
    assert region.shape == REGION_HW + (3,) and region.strides[0] == 993
    mask = tissue_mask(region)
    glass = mask.copy()
    glass[BLOCK] = False
    assert glass.sum() == 0                          # 240 +- 3 per channel: at most 6 apart, 255 * 6 < 18 * 237
    assert 0.975 < mask[BLOCK].mean() < 0.99         # uniform random bytes: about 98 % pass
    for (o, t, s), (k, n) in GRIDS.items():
        counts, kept, coords = oracle_selection(o, t, s)
        assert (len(kept), counts.size) == (k, n) and 0 < k < n
        assert np.array_equal(counts, region_tile_counts(region, t, s, o)) and coords.shape == (k, 2)
        assert (coords[:, 0] + t <= REGION_HW[0]).all() and (coords[:, 1] + t <= REGION_HW[1]).all()


def test_header_binding_and_library_agree_on_the_two_entries():
    from plip_amd import _lib
    from plip_amd.build import SOURCES, build
    build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "plipmi.h")).read()
    test_header = open(os.path.join(ROOT, "include", "plipmi_test.h")).read()
    for name, nargs in (("plipmi_region_select", 19), ("plipmi_region_gather", 15)):
        m = re.search(r"\bint %s\(([^;]*?)\);" % name, header, re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert name not in _lib.TEST_SYMBOLS and name not in test_header and hasattr(lib, name)
        assert _lib.SYMBOLS[name][0] is _lib._i and _lib.SYMBOLS[name][1][4] is __import__("ctypes").c_int64       # pitch_bytes
    assert SOURCES[-1] == "region.hip" and lib.plipmi_version() == 412
    assert re.search(r"#define PLIPMI_VERSION\s+412\b", header)


def test_entry_checks_are_clean_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/region_checks.hip, a stand-alone program: every rejection of the two entries (they all come before the handle is
    read or anything is launched), with region.hip's host code compiled under ASan + UBSan; the other objects are the library's own."""
    import subprocess
    from plip_amd import build as B
    try:
        hipcc = B._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    B.build(verbose=False)
    sanitize = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                "-Xarch_host", "-fno-omit-frame-pointer", "-g"]
    objs = []
    for src in (os.path.join(B.CSRC, "region.hip"), os.path.join(ROOT, "tests", "native", "region_checks.hip")):
        objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
        r = subprocess.run([hipcc, *B.FLAGS, *sanitize, "-I", B.CSRC, "-c", src, "-o", objs[-1]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    others = [os.path.join(B.BUILD, s.replace(".hip", ".o")) for s in B.SOURCES if s != "region.hip"]
    exe = str(tmp_path / "region_checks")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", *sanitize[:2], *objs, *others, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"), timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "region checks passed" in r.stdout, out[-6000:]
    for report in ("AddressSanitizer", "runtime error", "LeakSanitizer", "FAILED"):
        assert report not in out, out[-6000:]


@pytest.fixture(scope="module")
def oracle_plip():
    from oracle.make_golden import case_inputs
    from plip_amd.plip import PLIP
    cfg, sd, *_ = case_inputs("tiny_b6")
    plip = object.__new__(PLIP)                  # the constructor insists on a GPU; the argument checks do not need one
    plip.model = Hh.oracle_model(cfg, sd)
    return plip, cfg


@pytest.mark.parametrize("kwargs,match", [
    (dict(region=np.zeros((80, 80, 3), np.float32)), "uint8"),
    (dict(region=np.zeros((80, 80), np.uint8)), "uint8"),
    (dict(region=np.zeros((80, 80, 4), np.uint8)), "uint8"),
    (dict(region=[[1, 2, 3]]), "region"),
    (dict(region=torch.zeros((80, 80, 3))), "uint8"),
    (dict(region=torch.zeros((80, 3, 80), dtype=torch.uint8).permute(0, 2, 1)), "strides"),
    (dict(sat_min=256), "sat_min"), (dict(luma_min=-1), "luma_min"), (dict(luma_max=256), "luma_max"), (dict(sat_min=18.5), "sat_min"),
    (dict(tile_px=0), "tile_px"), (dict(stride=0), "stride"), (dict(origin=(-1, 0)), "origin"), (dict(min_tissue=float("nan")), "NaN"),
    (dict(band_rows=0), "band_rows"),
])
def test_encode_region_refuses_bad_arguments_before_any_device_work(oracle_plip, kwargs, match):
    plip, _ = oracle_plip
    args = dict(region=np.zeros((80, 80, 3), np.uint8))
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        plip.encode_region(**args)
    assert plip.model.engine.calls == []


def test_encode_region_on_an_empty_grid_needs_no_device(oracle_plip):
    plip, cfg = oracle_plip
    for region, kw, grid in ((np.zeros((63, 200, 3), np.uint8), {}, (0, 3)), (np.zeros((200, 40, 3), np.uint8), {}, (3, 0)),
                             (np.zeros((64, 64, 3), np.uint8), dict(origin=(0, 1)), (1, 0)),
                             (np.zeros((100, 100, 3), np.uint8), dict(tile_px=101, stride=7), (0, 0))):
        out = plip.encode_region(region, **kw)
        assert out.grid == grid and out.embeddings.shape == (0, cfg.projection_dim) and out.embeddings.dtype == np.float32
        assert out.coords.shape == (0, 2) and out.coords.dtype == np.int64 and out.kept.shape == (0,) and out.kept.dtype == np.int64
        assert out.tissue.shape == grid and out.tissue.dtype == np.float32
    assert plip.model.engine.calls == []
