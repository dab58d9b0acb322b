"""Stain normalisation without a GPU: the numpy oracle of plip_amd/preprocess.py pinned against a transcription of the published Macenko
script and against its own rules, the header / binding / build agreement, and every bad argument refused from Python before anything
touches a device."""
import os
import re

import numpy as np
import pytest

import stain_common as SC
from plip_amd import preprocess as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the generator -----------------------------------------------------------------------------------------------------------------------
def test_generator_gives_tissue_and_glass():
    for seed in range(12):
        t = SC.he_tile(seed)
        od = PP.stain_lut()[t]
        tissue = int((~(od < PP.STAIN_BETA).any(axis=2)).sum())
        assert t.shape == (64, 64, 3) and t.dtype == np.uint8 and tissue >= 2000 and 0.2 < 1 - tissue / 4096 < 0.45, (seed, tissue)
    assert np.abs(SC.HE_SOURCE - PP.HE_REF).max() > 0.1


# ---- the oracle against the published script ---------------------------------------------------------------------------------------------
def test_oracle_equals_the_published_macenko_script():
    worst_he = worst_maxc = 0.0
    differing = total = 0
    for seed in range(12):
        t = SC.he_tile(seed)
        row = PP.stain_fit_reference(t)[0]
        ref_img, ref_he, ref_maxc = SC.published_macenko(t)
        out = PP.stain_apply_reference(t, row[None])
        assert row[15] == 1.0 and row[14] >= 2000
        worst_he = max(worst_he, float(np.abs(row[0:6].reshape(3, 2) - ref_he).max()))
        worst_maxc = max(worst_maxc, float((np.abs(row[12:14] - ref_maxc) / ref_maxc).max()))
        differing += int((out != ref_img).sum())
        total += out.size
        P = row[6:12].reshape(2, 3)
        assert np.abs(P @ row[0:6].reshape(3, 2) - np.eye(2)).max() <= 1e-12            # P is the pseudo-inverse of HE
    print(f"stain oracle vs the published script: HE {worst_he:.3g}, maxC (relative) {worst_maxc:.3g}, bytes differing {differing} of {total}")
    assert worst_he <= 1e-6 and worst_maxc <= 1e-6 and differing == 0 and total == 12 * 64 * 64 * 3


# ---- the percentile ----------------------------------------------------------------------------------------------------------------------
def test_stain_percentile_is_numpys_linear_percentile_of_the_float32_keys():
    rs = np.random.RandomState(4)
    cases = [np.asarray([1.5]), np.asarray([2.0, -3.0]), np.asarray([0.0, -0.0, 0.0]), np.round(rs.standard_normal(200) * 3) / 3,       # m = 1, 2; ties
             -np.abs(rs.standard_normal(101)), rs.standard_normal(101), rs.standard_normal(1000) * 1e-3 + 0.7371, np.pi * rs.uniform(-1, 1, 577)]
    checked = 0
    for keys in cases:
        m = keys.size
        qs = [0, 1, 25, 50, 75, 99, 100, 37.3, 99.9] + ([100.0 * k / (m - 1) for k in (1, m // 2, m - 2)] if m > 2 else [])      # integer ranks too
        for q in qs:
            want = np.percentile(keys.astype(np.float32).astype(np.float64), q)
            got = PP.stain_percentile(keys, q)
            assert got == want, (m, q, got, want)
            checked += 1
    assert checked > 70 and np.isnan(PP.stain_percentile(np.zeros(0), 50))


# ---- behaviour ---------------------------------------------------------------------------------------------------------------------------
def test_refitting_a_normalised_tile_finds_the_target_stains():
    """Measured with the oracle on seeds 0 .. 3: HE within 0.0196 of HE_REF, maxC within 5.09 % of MAXC_REF (the tile's own stains are
    0.13 and 50 % away); the bars are twice that."""
    worst_he = worst_maxc = 0.0
    for seed in range(4):
        t = SC.he_tile(seed)
        before = PP.stain_fit_reference(t)[0]
        assert np.abs(before[0:6].reshape(3, 2) - PP.HE_REF).max() > 0.1
        again = PP.stain_fit_reference(PP.stain_apply_reference(t, before[None]))[0]
        assert again[15] == 1.0
        worst_he = max(worst_he, float(np.abs(again[0:6].reshape(3, 2) - PP.HE_REF).max()))
        worst_maxc = max(worst_maxc, float((np.abs(again[12:14] - PP.MAXC_REF) / PP.MAXC_REF).max()))
    print(f"stain refit: HE within {worst_he:.4f}, maxC within {100 * worst_maxc:.2f} %")
    assert worst_he <= 0.04 and worst_maxc <= 0.102
    # normalising one tile to another's fit moves it to that tile's stains
    other = PP.stain_fit_reference(SC.he_tile(7, he=PP.HE_REF, strength=(1.2, 0.9)))[0]
    moved = PP.stain_fit_reference(PP.stain_apply_reference(SC.he_tile(0), PP.stain_fit_reference(SC.he_tile(0)), target=other))[0]
    assert np.abs(moved[0:6] - other[0:6]).max() <= 0.04 and (np.abs(moved[12:14] - other[12:14]) / other[12:14]).max() <= 0.102


def test_an_all_glass_tile_is_an_invalid_fit_and_comes_back_unchanged():
    g = SC.glass_tile(0)
    row = PP.stain_fit_reference(g)
    assert row.shape == (1, 16) and row[0, 14] == 0 and row[0, 15] == 0 and not row[0, :14].any()
    assert np.array_equal(PP.stain_apply_reference(g, row), g)
    batch = np.stack([SC.he_tile(0), g])
    rows = PP.stain_fit_reference(batch)
    out = PP.stain_apply_reference(batch, rows)
    assert rows[:, 15].tolist() == [1, 0] and np.array_equal(out[1], g) and not np.array_equal(out[0], batch[0])
    few = g.copy()
    few[0, :15] = SC.he_tile(0)[SC.he_tile(0).max(axis=2) <= 200][:15]                 # 15 tissue pixels: one short of a fit
    row = PP.stain_fit_reference(few)[0]
    assert row[14] == 15 and row[15] == 0
    flat = np.full((8, 8, 3), 120, np.uint8)                                            # tissue of ONE colour: no stain plane
    row = PP.stain_fit_reference(flat)[0]
    assert row[14] == 64 and row[15] == 0 and np.isfinite(row).all()


def test_host_subsampling_and_step_give_identical_fits():
    imgs = np.stack([SC.he_tile(s, 61, 70) for s in (3, 4)])
    for step in (2, 3, 7):
        for pooled in (False, True):
            a = PP.stain_fit_reference(imgs, pooled=pooled, step=step)
            b = PP.stain_fit_reference(np.ascontiguousarray(imgs[:, ::step, ::step]), pooled=pooled, step=1)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (step, pooled)
    assert np.array_equal(PP._stain_samples(imgs, 3), imgs[:, ::3, ::3].reshape(2, -1, 3))
    assert PP.stain_default_step(1, 8192, 8192) == 4 and PP.stain_default_step(256, 224, 224) == 2 and PP.stain_default_step(4, 64, 64) == 1
    for B, H, W in ((1, 8192, 8192), (3, 5000, 7001), (256, 224, 224)):
        s = PP.stain_default_step(B, H, W)
        assert B * -(-H // s) * -(-W // s) <= 1 << 22 and (s == 1 or B * -(-H // (s - 1)) * -(-W // (s - 1)) > 1 << 22)


# ---- headers, symbols and the build ------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_entries():
    from plip_amd import _lib
    from plip_amd import build as BLD
    BLD.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "plipmi.h")).read()
    test_header = open(os.path.join(ROOT, "include", "plipmi_test.h")).read()
    for name, ret, nargs in (("plipmi_stain_workspace", "size_t", 4), ("plipmi_stain_fit", "int", 16), ("plipmi_stain_apply", "int", 14)):
        m = re.search(r"\b%s %s\(([^;]*?)\);" % (ret, name), header, re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert name not in _lib.TEST_SYMBOLS and not re.search(r"\b%s %s\s*\(" % (ret, name), test_header) and hasattr(lib, name)    # (declared in one header)
    m = re.search(r"\bint plipmi_stain_percentile\(([^;]*?)\);", test_header, re.S)
    assert m and len(m.group(1).split(",")) == 10 == len(_lib.TEST_SYMBOLS["plipmi_stain_percentile"][1])
    assert "plipmi_stain_percentile" not in _lib.SYMBOLS and "plipmi_stain_percentile" not in header and hasattr(lib, "plipmi_stain_percentile")
    # the new unit: compiled and linked last, behind kmeans.hip, in neither pinned list
    order = BLD.SOURCES + BLD.LATER_SOURCES + BLD.STAIN_SOURCES
    assert order[-1] == "stain.hip" and order[-2] == "kmeans.hip" and BLD.LATER_SOURCES == ["kmeans.hip"] and BLD.SOURCES[-1] == "region.hip"
    assert "stain.hip" not in BLD.SOURCES and "stain.hip" not in BLD.LATER_SOURCES and len(set(order)) == len(order)
    assert lib.plipmi_version() == 412 and re.search(r"#define PLIPMI_VERSION\s+412\b", header)
    # the workspace: zero for sizes the fit refuses, and it grows with the samples
    ws = lib.plipmi_stain_workspace
    assert ws(0, 64, 64, 1) == 0 and ws(1, 0, 64, 1) == 0 and ws(1, 64, 64, 0) == 0
    assert ws(1, 64, 64, 1) > 4 * 64 * 64 and ws(4, 64, 64, 1) > ws(1, 64, 64, 1) > ws(1, 64, 64, 2)


# ---- what Python refuses before any device work ------------------------------------------------------------------------------------------
def _engine():
    class NoDevice:
        @property
        def device(self):
            raise AssertionError("a refused call asked for the device")

        @property
        def lib(self):
            raise AssertionError("a refused call asked for the library")
    return NoDevice()


def _fit(rows: int):
    import torch
    from plip_amd.stain import StainFit
    return StainFit(torch.zeros((rows, 16), dtype=torch.float64), rows == 1, 1)


_TILES = np.zeros((3, 8, 8, 3), np.uint8)


@pytest.mark.parametrize("call,message", [
    (lambda st, e: st.stain_fit(e, _TILES.astype(np.float32)), "uint8 [B,H,W,3]"),
    (lambda st, e: st.stain_fit(e, np.zeros((3, 8, 8, 4), np.uint8)), "uint8 [B,H,W,3]"),
    (lambda st, e: st.stain_fit(e, np.zeros((8, 8), np.uint8)), "uint8 [B,H,W,3]"),
    (lambda st, e: st.stain_fit(e, [1, 2, 3]), "uint8 [B,H,W,3]"),
    (lambda st, e: st.stain_fit(e, _t(_TILES).permute(0, 2, 1, 3)), "strides"),
    (lambda st, e: st.stain_fit(e, _t(np.zeros((3, 8, 8, 6), np.uint8))[..., ::2]), "strides"),
    (lambda st, e: st.stain_fit(e, _TILES, step=0), "step must be an integer >= 1"),
    (lambda st, e: st.stain_fit(e, _TILES, step=1.5), "step must be an integer >= 1"),
    (lambda st, e: st.stain_fit(e, _TILES, alpha=0.0), "alpha must lie in (0, 50)"),
    (lambda st, e: st.stain_fit(e, _TILES, alpha=50.0), "alpha must lie in (0, 50)"),
    (lambda st, e: st.stain_fit(e, _TILES, Io=0.0), "Io must be positive"),
    (lambda st, e: st.stain_fit(e, _TILES, beta=-1.0), "beta must be positive"),
    (lambda st, e: st.stain_apply(e, _TILES, _fit(2)), "a fit of 1 row or of 3"),
    (lambda st, e: st.stain_apply(e, _TILES, np.zeros((3, 16))), "fit must be a StainFit"),
    (lambda st, e: st.stain_apply(e, _TILES.astype(np.int16), _fit(3)), "uint8 [B,H,W,3]"),
    (lambda st, e: st.stain_apply(e, _TILES, _fit(3), target=_fit(3)), "a target is one fit"),
])
def test_bad_arguments_are_refused_with_a_message_that_names_them(call, message):
    import plip_amd.stain as st
    with pytest.raises(ValueError) as err:
        call(st, _engine())
    assert message in str(err.value), str(err.value)


def _t(a):
    import torch
    return torch.from_numpy(a)


def test_encode_region_refuses_a_stain_that_is_not_one_fit():
    from plip_amd.region_routes import encode_region
    region = np.zeros((64, 64, 3), np.uint8)
    for bad, message in ((_fit(2), "2 fits"), (np.zeros(16), "ndarray")):
        with pytest.raises(ValueError) as err:
            encode_region(_engine(), region, 64, 8, "hf", stain=bad)
        assert "ONE fit" in str(err.value) and message in str(err.value)
    assert len(_fit(1)) == 1 and _fit(1).as_target().shape == (8,)
    with pytest.raises(ValueError, match="a target is one fit"):
        _fit(2).as_target()
