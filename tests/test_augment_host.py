"""CPU-side checks of augmented views (include/plipmi.h plipmi_warp_u8, plip_amd/augment.py, PLIP.encode_views): the numpy oracle of
the warp against Pillow, byte for byte; the parameter builders; the C-ABI declaration and binding; the entry's rejections under the
sanitizers; and what ``encode_views`` refuses before it touches a device.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest

import helpers as Hh
from augment_common import FILL, pil, pil_train_view, pil_warp, random_cases

from plip_amd.preprocess import (IDENTITY_ROW, affine_coeffs, check_perspective, dihedral_coeffs, perspective_coeffs, sample_train_params,
                                 train_params, train_view_reference, warp_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_pillow = pytest.mark.skipif(pil() is None, reason="Pillow is not installed")


def _mismatches(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (got.shape, want.shape, got.dtype, want.dtype)
    return int((got != want).sum())


# ---- warp_reference == Pillow -------------------------------------------------------------------------------------------------------
@needs_pillow
def test_warp_reference_equals_pillow_on_random_rows():
    cases = random_cases()
    assert len(cases) >= 40 and {c[2] for c in cases} == {False, True} and all(c[3][0] != c[3][1] for c in cases)
    total = 0
    for i, (src, row, perspective, out_hw) in enumerate(cases):
        want = pil_warp(src, row, perspective, out_hw)
        got = warp_reference(src, row, perspective, out_hw, FILL)
        bad = _mismatches(got, want)
        print(f"warp_reference vs Pillow, case {i}: src {src.shape[:2]} out {out_hw} perspective {perspective}: {bad} of {got.size} bytes differ")
        assert bad == 0, i
        total += got.size
    assert total > 50000


@needs_pillow
def test_warp_reference_identity_and_fill():
    rs = np.random.RandomState(3)
    src = rs.randint(0, 256, size=(19, 31, 3), dtype=np.uint8)
    for perspective in (False, True):
        assert np.array_equal(warp_reference(src, IDENTITY_ROW, perspective), src)
        assert np.array_equal(pil_warp(src, np.asarray(IDENTITY_ROW), perspective, (19, 31)), src)
    # a row that maps every pixel outside: all fill, each channel its own value
    out = warp_reference(src, [1, 0, 1000, 0, 1, 0], False, (7, 9), FILL)
    assert out.shape == (7, 9, 3) and (out == np.asarray(FILL, np.uint8)).all()
    assert np.array_equal(out, pil_warp(src, np.asarray([1.0, 0, 1000, 0, 1, 0, 0, 0]), False, (7, 9)))
    # NaN coefficients are outside everywhere
    assert (warp_reference(src, [np.nan, 0, 0, 0, 1, 0], False, (4, 5), 9) == 9).all()
    # a 1 x 1 source, magnified
    one = np.asarray([[[10, 200, 77]]], np.uint8)
    row = [1 / 6, 0, 0, 0, 1 / 5, 0, 0, 0]
    assert np.array_equal(warp_reference(one, row, False, (5, 6), FILL), pil_warp(one, np.asarray(row), False, (5, 6)))


def test_dihedral_rows_equal_numpy_rotations_and_flips():
    rs = np.random.RandomState(4)
    for n in (1, 2, 7, 24):
        src = rs.randint(0, 256, size=(n, n, 3), dtype=np.uint8)
        seen = set()
        for k in range(8):
            row = dihedral_coeffs(k, n)
            assert row.shape == (6,) and np.array_equal(row, np.round(row))
            want = np.rot90(src if k < 4 else src[:, ::-1], k % 4)
            got = warp_reference(src, row, False, (n, n), FILL)
            assert np.array_equal(got, want), (n, k)
            if pil() is not None:
                assert np.array_equal(pil_warp(src, np.concatenate([row, [0, 0]]), False, (n, n)), want), (n, k)
            seen.add(got.tobytes())
        assert n == 1 or len(seen) == 8
    assert dihedral_coeffs(4, 24).tolist() == [-1, 0, 24, 0, 1, 0]
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            dihedral_coeffs(bad, 8)


@needs_pillow
def test_windows_with_flip_equal_pil_crop_transpose_transform():
    rs = np.random.RandomState(5)
    src = rs.randint(0, 256, size=(40, 52, 3), dtype=np.uint8)
    from augment_common import random_affine_row, random_perspective_row
    n = 0
    for i in range(24):
        wh, ww = (24, 24) if i % 3 else (int(rs.randint(1, 41)), int(rs.randint(1, 53)))
        wy, wx = int(rs.randint(0, 40 - wh + 1)), int(rs.randint(0, 52 - ww + 1))
        if i == 0:
            wy, wx, wh, ww = 0, 0, 40, 52
        if i == 1:
            wy, wx, wh, ww = 39, 51, 1, 1
        window = (wy, wx, wh, ww, i % 2)
        perspective = i % 4 >= 2
        row = random_perspective_row(rs, ww, wh) if perspective else random_affine_row(rs, ww, wh)
        out_hw = (wh, ww) if i % 3 else (17, 22)
        if perspective:
            try:
                check_perspective(row, *out_hw)
            except ValueError:
                continue
        got = warp_reference(src, row, perspective, out_hw, FILL, window)
        assert _mismatches(got, pil_warp(src, row, perspective, out_hw, FILL, window)) == 0, window
        n += 1
    assert n >= 20
    for bad in ((-1, 0, 5, 5, 0), (0, 0, 41, 5, 0), (0, 48, 5, 5, 1), (0, 0, 0, 5, 0)):
        with pytest.raises(ValueError, match="window"):
            warp_reference(src, IDENTITY_ROW, False, (5, 5), 0, bad)


@needs_pillow
def test_train_chain_reference_equals_the_pil_chain():
    rs = np.random.RandomState(6)
    src = rs.randint(0, 256, size=(40, 52, 3), dtype=np.uint8)
    drew = set()
    for v in range(20):
        window, affine, persp = sample_train_params(7, 0, v, (40, 52), 24)
        drew.add(bool((persp != np.asarray(IDENTITY_ROW)).any()))
        got = train_view_reference(src, window, affine, persp)
        assert _mismatches(got, pil_train_view(src, window, affine, persp)) == 0, v
    assert drew == {False, True}


# ---- the builders -------------------------------------------------------------------------------------------------------------------
def test_affine_coeffs_is_the_inverse_of_the_forward_matrix():
    import math
    rs = np.random.RandomState(8)
    assert np.array_equal(affine_coeffs((12.0, 9.5), 0.0, (0, 0), 1.0, (0.0, 0.0)), [1, 0, 0, 0, 1, 0])
    for _ in range(50):
        cx, cy = rs.uniform(1, 112, 2)               # (tiles up to 224 px: the entries stay below a few hundred, 1e-12 is ~1e4 ulp of them)
        ang, sc = rs.uniform(-180, 180), rs.uniform(0.7, 1.4)
        tx, ty = rs.uniform(-25, 25, 2)
        shx, shy = rs.uniform(-20, 20, 2)
        rot, sx, sy = math.radians(ang), math.radians(shx), math.radians(shy)
        rss = np.asarray([[math.cos(rot - sy) / math.cos(sy), -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot), 0],
                          [math.sin(rot - sy) / math.cos(sy), -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot), 0],
                          [0, 0, 1]]) * np.asarray([[sc], [sc], [1.0]])
        T = np.asarray([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])
        C = np.asarray([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]])
        Ci = np.asarray([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]])
        inv = np.linalg.inv(T @ C @ rss @ Ci)
        got = affine_coeffs((cx, cy), ang, (tx, ty), sc, (shx, shy))
        assert np.abs(got - inv[:2].reshape(-1)).max() <= 1e-12, (got, inv)


def test_an_integer_translation_shifts_bytes_exactly():
    rs = np.random.RandomState(9)
    src = rs.randint(0, 256, size=(20, 30, 3), dtype=np.uint8)
    for tx, ty in ((3, 0), (-4, 2), (0, -5), (7, 6)):
        row = affine_coeffs((15.0, 10.0), 0.0, (tx, ty), 1.0, (0.0, 0.0))
        assert row.tolist() == [1, 0, -tx, 0, 1, -ty]
        got = warp_reference(src, row, False, None, FILL)
        want = np.empty_like(src)
        want[:] = np.asarray(FILL, np.uint8)
        ys, xs = np.arange(20), np.arange(30)
        oky, okx = (ys - ty >= 0) & (ys - ty < 20), (xs - tx >= 0) & (xs - tx < 30)
        want[np.ix_(oky, okx)] = src[np.ix_((ys - ty)[oky], (xs - tx)[okx])]
        assert np.array_equal(got, want), (tx, ty)


def test_perspective_coeffs_maps_endpoints_to_startpoints_and_refuses_vanishing_denominators():
    rs = np.random.RandomState(10)
    for _ in range(30):
        w, h = rs.randint(8, 300, 2)
        start = np.asarray([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
        end = start + rs.uniform(0, 0.3, (4, 2)) * [w / 2, h / 2] * np.asarray([[1, 1], [-1, 1], [-1, -1], [1, -1]])
        a = perspective_coeffs(start, end)
        den = a[6] * end[:, 0] + a[7] * end[:, 1] + 1
        got = np.stack([(a[0] * end[:, 0] + a[1] * end[:, 1] + a[2]) / den, (a[3] * end[:, 0] + a[4] * end[:, 1] + a[5]) / den], axis=1)
        assert np.abs(got - start).max() <= 1e-9
        check_perspective(a, h, w)
    sq = [[0, 0], [9, 0], [9, 9], [0, 9]]
    assert np.abs(perspective_coeffs(sq, sq) - np.asarray(IDENTITY_ROW)).max() <= 1e-12
    # a folded-over quadrilateral (two endpoints swapped): the denominator changes sign between its corners
    with pytest.raises(ValueError, match="vanishing denominator"):
        perspective_coeffs(sq, [[0, 0], [9, 9], [9, 0], [0, 9]])
    with pytest.raises(ValueError, match="vanishing denominator"):
        perspective_coeffs(sq, [[0, 0], [5, 5], [9, 9], [2, 2]])        # collinear: singular
    # a valid row used for an output larger than the one it was made for
    row = np.asarray([1, 0, 0, 0, 1, 0, -0.02, 0.0])
    check_perspective(row, 40, 49)
    for bad, hw in ((row, (40, 50)), (row, (40, 64)), (np.asarray([1, 0, 0, 0, 1, 0, np.nan, 0]), (4, 4)), (np.asarray([1, 0, 0, 0, 1, 0, 0, np.inf]), (4, 4))):
        with pytest.raises(ValueError, match="vanishing denominator"):
            check_perspective(bad, *hw)
        with pytest.raises(ValueError, match="vanishing denominator"):
            warp_reference(np.zeros((8, 8, 3), np.uint8), bad, True, hw)
    with pytest.raises(ValueError, match=r"row \[1, 2\]"):
        rows = np.tile(np.asarray(IDENTITY_ROW), (2, 3, 1))
        rows[1, 2, 7] = -1.0
        check_perspective(rows, 4, 4)


def test_sample_train_params_ranges_reproducibility_and_independence():
    import math
    n, hw = 64, (96, 80)
    d = int(0.3 * (n // 2))
    seen_flip, seen_persp, tops, lefts = set(), 0, set(), set()
    for i in range(40):
        for v in range(3):
            window, affine, persp = sample_train_params(5, i, v, hw, n)
            assert window.dtype == np.int32 and window.shape == (5,) and affine.shape == persp.shape == (8,) and affine.dtype == persp.dtype == np.float64
            top, left, wh, ww, flip = window.tolist()
            assert 0 <= top <= hw[0] - n and 0 <= left <= hw[1] - n and (wh, ww) == (n, n) and flip in (0, 1)
            tops.add(top), lefts.add(left), seen_flip.add(flip)
            # the affine row back to its parameters: [d, -b, ., -c, a, .] / scale
            a6 = affine[:6]
            assert affine[6] == affine[7] == 0.0
            fwd = np.linalg.inv(np.asarray([[a6[0], a6[1], a6[2]], [a6[3], a6[4], a6[5]], [0, 0, 1]]))
            # forward = T C RSS C^-1: its translation part gives tx, ty as integers within 0.1 n
            lin = fwd[:2, :2]
            t = fwd[:2, 2] - (np.asarray([n * 0.5, n * 0.5]) - lin @ np.asarray([n * 0.5, n * 0.5]))
            assert np.abs(t - np.round(t)).max() < 1e-9 and np.abs(t).max() <= round(0.1 * n) + 1e-9
            # a = cos(rot - sy) / cos(sy) * s, c = sin(rot - sy) / cos(sy) * s: |(a, c)| = s / cos(sy), within the scale and shear ranges
            s_over = math.hypot(lin[0, 0], lin[1, 0])
            assert 0.8 - 1e-9 <= s_over <= 1.2 / math.cos(math.radians(15)) + 1e-9
            ang = math.degrees(math.atan2(lin[1, 0], lin[0, 0]))           # rot - sy
            assert -25 - 1e-9 <= ang <= 25 + 1e-9
            if (persp != np.asarray(IDENTITY_ROW)).any():
                seen_persp += 1
                # the endpoints (corners moved inward by integers in [0, d]) map to the corners
                corners = np.asarray([[0, 0], [n - 1, 0], [n - 1, n - 1], [0, n - 1]], np.float64)
                A = np.asarray([[persp[0], persp[1], persp[2]], [persp[3], persp[4], persp[5]], [persp[6], persp[7], 1.0]])
                ends = (np.linalg.inv(A) @ np.concatenate([corners, np.ones((4, 1))], axis=1).T).T
                ends = ends[:, :2] / ends[:, 2:]
                move = (ends - corners) * np.asarray([[1, 1], [-1, 1], [-1, -1], [1, -1]])
                assert np.abs(move - np.round(move)).max() < 1e-6 and move.min() > -1e-6 and move.max() < d + 1e-6
                check_perspective(persp, n, n)
            again = sample_train_params(5, i, v, hw, n)
            assert all(np.array_equal(x, y) for x, y in zip((window, affine, persp), again))
    assert seen_flip == {0, 1} and 15 <= seen_persp <= 60 and len(tops) > 10 and len(lefts) > 8         # p = 0.3 of 120: 36 +- 5
    # independent across (index, view), and of how many are drawn together
    rows = {(i, v): sample_train_params(5, i, v, hw, n)[1].tobytes() for i in range(6) for v in range(4)}
    assert len(set(rows.values())) == 24
    assert sample_train_params(6, 0, 0, hw, n)[1].tobytes() != rows[(0, 0)]
    w, a, p = train_params(5, 4, 3, hw, n, first=2)
    assert w.shape == (4, 3, 5) and a.shape == p.shape == (4, 3, 8) and a[1, 2].tobytes() == rows[(3, 2)]
    with pytest.raises(ValueError, match="does not fit"):
        sample_train_params(0, 0, 0, (63, 80), 64)


# ---- header, binding, library -------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_entry():
    import ctypes
    from plip_amd import _lib
    from plip_amd.build import SOURCES, build
    build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "plipmi.h")).read()
    test_header = open(os.path.join(ROOT, "include", "plipmi_test.h")).read()
    name = "plipmi_warp_u8"
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, header, re.S)
    assert m and len(m.group(1).split(",")) == 15 == len(_lib.SYMBOLS[name][1])
    assert name not in _lib.TEST_SYMBOLS and name not in test_header and hasattr(lib, name)
    args = _lib.SYMBOLS[name][1]
    assert _lib.SYMBOLS[name][0] is _lib._i and args[5] is ctypes.c_int64 and args[6] is ctypes.c_int64 and args[12] is ctypes.c_uint32
    # every plipmi_* function the header declares is bound, and nothing else is
    declared = set(re.findall(r"\b(plipmi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    assert SOURCES[-1] == "region.hip" and SOURCES[-2] == "augment.hip" and lib.plipmi_version() == 412
    assert re.search(r"#define PLIPMI_VERSION\s+412\b", header)


def test_engine_surface_is_unchanged():
    from test_host import ENGINE_SURFACE
    from plip_amd.engine import Engine
    assert {k for k in dir(Engine) if not k.startswith("_")} == set(ENGINE_SURFACE)
    import inspect
    from plip_amd.plip import PLIP
    assert str(inspect.signature(PLIP.encode_images)) == ("(self, images: 'Union[List[str], list, np.ndarray, torch.Tensor]', batch_size: 'int', "
                                                          "num_workers: 'int' = 0, image_size: 'Optional[int]' = None)")
    sig = inspect.signature(PLIP.encode_views)
    assert list(sig.parameters) == ["self", "images", "batch_size", "views", "transform", "seed", "reduce", "return_params"]
    assert [sig.parameters[k].default for k in ("views", "transform", "seed", "reduce", "return_params")] == [8, "d4", 0, None, False]


def test_entry_checks_are_clean_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/augment_checks.hip, a stand-alone program: every rejection of the entry (they all come before the handle is read
    or anything is launched), with augment.hip's host code compiled under ASan + UBSan; the other objects are the library's own."""
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
    for src in (os.path.join(B.CSRC, "augment.hip"), os.path.join(ROOT, "tests", "native", "augment_checks.hip")):
        objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
        r = subprocess.run([hipcc, *B.FLAGS, *sanitize, "-I", B.CSRC, "-c", src, "-o", objs[-1]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    others = [os.path.join(B.BUILD, s.replace(".hip", ".o")) for s in B.SOURCES if s != "augment.hip"]
    exe = str(tmp_path / "augment_checks")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", *sanitize[:2], *objs, *others, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"), timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "augment checks passed" in r.stdout, out[-6000:]
    for report in ("AddressSanitizer", "runtime error", "LeakSanitizer", "FAILED"):
        assert report not in out, out[-6000:]


# ---- what encode_views refuses without a device -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_plip():
    from oracle.make_golden import case_inputs
    from plip_amd.plip import PLIP
    cfg, sd, *_ = case_inputs("tiny_b6")
    plip = object.__new__(PLIP)                  # the constructor insists on a GPU; the argument checks do not need one
    plip.model = Hh.oracle_model(cfg, sd)
    return plip, cfg


@pytest.mark.parametrize("kwargs,match", [
    (dict(images=np.zeros((2, 63, 80, 3), np.uint8), transform="train"), "smaller than n_px"),
    (dict(images=np.zeros((2, 80, 63, 3), np.uint8), transform="train"), "smaller than n_px"),
    (dict(views=9), "eight views"),
    (dict(images=np.zeros((2, 80, 80, 3), np.uint8)), "encode resolution"),
    (dict(images=[np.zeros((64, 64, 3), np.uint8), np.zeros((64, 65, 3), np.uint8)]), "mixed sizes"),
    (dict(transform="rot"), "unknown transform"),
    (dict(reduce="sum"), "reduce"),
    (dict(views=0), "at least 1"),
    (dict(images=np.zeros((2, 64, 64, 3), np.float32)), "uint8"),
    (dict(images=np.zeros((2, 64, 64), np.uint8)), "uint8"),
])
def test_encode_views_refuses_bad_arguments_before_any_device_work(oracle_plip, kwargs, match):
    plip, cfg = oracle_plip
    assert cfg.image_size == 64
    args = dict(images=np.zeros((2, 64, 64, 3), np.uint8), batch_size=4)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        plip.encode_views(**args)
    assert plip.model.engine.calls == []


def test_encode_views_of_no_tiles_needs_no_device(oracle_plip):
    plip, cfg = oracle_plip
    out = plip.encode_views(np.zeros((0, 64, 64, 3), np.uint8), batch_size=4, views=3)
    assert out.shape == (0, 3, cfg.projection_dim) and out.dtype == np.float32
    out, params = plip.encode_views([], batch_size=4, views=2, transform="train", reduce="mean", return_params=True)
    assert out.shape == (0, cfg.projection_dim) and [p.shape for p in params] == [(0, 2, 5), (0, 2, 8), (0, 2, 8)]
    assert plip.model.engine.calls == []
