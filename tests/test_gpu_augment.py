"""Augmented views on the MI355X (include/plipmi.h plipmi_warp_u8, plip_amd/augment.py, PLIP.encode_views): the warp kernel against
the numpy oracle ``preprocess.warp_reference`` (pinned to Pillow in tests/test_augment_host.py, and compared with Pillow here too where
it imports), the two-launch train chain against the PIL chain, and the embeddings of the views against ``PLIP.encode_images`` on the
oracle's bytes -- all exact: bytes and bit-equal floats, zero mismatches allowed.  Every count is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from augment_common import FILL, pil, pil_train_view, pil_warp, random_affine_row, random_perspective_row

from plip_amd.preprocess import (IDENTITY_ROW, check_perspective, dihedral_coeffs, train_params, train_view_reference, warp_reference)

pytestmark = pytest.mark.gpu

CASE = "tiny_b6"          # 64 px tiles, 16 px patches
H, W, B = 37, 53, 5
SENTINEL, GUARD = 0xA5, 64


def _report(what, *diffs):
    print(f"augment parity: {what}: " + ", ".join(f"{k} {v}" for k, v in diffs))


@pytest.fixture(scope="module")
def engine(engines):
    return engines(CASE, "f32")[0].engine


@functools.lru_cache(maxsize=None)
def _sources():
    """uint8 [5,41,57,3]; the sources are its [:, 2:39, 3:56]: a pitch of 171 bytes (odd: rows start at every alignment) and images
    7011 bytes apart, not H * pitch"""
    big = np.random.RandomState(21).randint(0, 256, size=(B, 41, 57, 3), dtype=np.uint8)
    big.setflags(write=False)
    return big


def _source_view(engine):
    big = torch.from_numpy(_sources().copy()).to(engine.device)
    view = big[:, 2:39, 3:56]
    assert tuple(view.shape) == (B, H, W, 3) and view.stride() == (41 * 171, 171, 3, 1) and 41 * 171 != H * 171
    return view


@functools.lru_cache(maxsize=None)
def _rows(perspective, out_hw):
    """five differing rows of one mode: two in the train ranges, one far past them (a strongly distorted quadrilateral), one that maps
    every pixel outside the source, and a translated identity"""
    rs = np.random.RandomState(31 + int(perspective))
    while True:
        try:                 # (a strongly distorted quadrilateral may fold over: drawn again)
            if perspective:
                rows = [random_perspective_row(rs, W, H), random_perspective_row(rs, W, H, 0.95), np.asarray([1, 0, 1000.0, 0, 1, 0, 0, 0]),
                        np.asarray([1, 0, 0.25, 0, 1, -0.5, 1e-3, 2e-3]), random_perspective_row(rs, W, H)]
                check_perspective(np.stack(rows), *out_hw)
            else:
                rows = [random_affine_row(rs, W, H), random_affine_row(rs, W, H, strong=True), np.asarray([1, 0, 0, 0, 1, -1000.0, 0, 0]),
                        np.asarray([1, 0, 0.25, 0, 1, -0.5, 0, 0]), random_affine_row(rs, W, H)]
            return np.stack(rows)
        except ValueError:
            continue


WINDOWS = np.asarray([[0, 0, 20, 30, 0], [0, 23, 37, 30, 1], [17, 0, 20, 53, 0], [36, 52, 1, 1, 1], [0, 0, 37, 53, 1]], np.int32)


def _guarded(engine, n_out, offset=0):
    """a sentinel-filled destination of n_out bytes starting ``offset`` bytes into its allocation, guard bytes behind (and in front)"""
    buf = torch.full((offset + n_out + GUARD,), SENTINEL, dtype=torch.uint8, device=engine.device)
    return buf, buf[offset:offset + n_out]


def _check_warp(engine, what, src_dev, src_np, rows, perspective, out_hw, windows=None, offset=0, fill=FILL):
    from plip_amd.augment import warp_u8
    n = rows.shape[0]
    oh, ow = out_hw
    buf, out = _guarded(engine, n * oh * ow * 3, offset)
    got = warp_u8(engine, src_dev, rows, windows, perspective, out_hw, fill, out=out.view(n, oh, ow, 3))
    torch.cuda.synchronize(engine.device)
    got, buf = got.cpu().numpy(), buf.cpu().numpy()
    imgs = [src_np] * n if src_np.ndim == 3 else list(src_np)
    want = np.stack([warp_reference(imgs[b], rows[b], perspective, out_hw, fill, None if windows is None else windows[b]) for b in range(n)])
    bad = int((got != want).sum())
    diffs = [("bytes", want.size), ("mismatches vs oracle", bad)]
    if pil() is not None:
        pw = np.stack([pil_warp(imgs[b], rows[b], perspective, out_hw, fill, None if windows is None else windows[b]) for b in range(n)])
        diffs.append(("mismatches vs Pillow", int((got != pw).sum())))
    guard = int((buf[:offset] != SENTINEL).sum() + (buf[offset + want.size:] != SENTINEL).sum())
    _report(what, *diffs, ("guard bytes touched", guard))
    assert all(v == 0 for k, v in diffs[1:]) and guard == 0, what
    return got


# ---- 1. kernel == oracle, every byte --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perspective", [False, True], ids=["affine", "perspective"])
@pytest.mark.parametrize("out_hw", [(24, 24), (20, 33), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_warp_equals_the_oracle_on_a_strided_source(engine, perspective, out_hw):
    """24 x 24 takes the four-pixel kernel (and, from a destination one byte off, the byte kernel); 20 x 33 and 1 x 1 fit no wide store"""
    src = _source_view(engine)
    src_np = _sources()[:, 2:39, 3:56]
    rows = _rows(perspective, out_hw)
    got = _check_warp(engine, f"strided source, {out_hw}, perspective={perspective}", src, src_np, rows, perspective, out_hw)
    assert (got[2] == np.asarray(FILL, np.uint8)).all()                     # the row that maps wholly outside: all fill, channel by channel
    assert out_hw == (1, 1) or len({got[b].tobytes() for b in range(B)}) == B
    _check_warp(engine, f"the same, destination one byte off, {out_hw}", src, src_np, rows, perspective, out_hw, offset=1)
    # windows touching each border, mirrored and not
    _check_warp(engine, f"windows, {out_hw}, perspective={perspective}", src, src_np, rows, perspective, out_hw, windows=WINDOWS)
    # image_stride_bytes = 0: five views of ONE image (itself a view: row 2, column 3 of the buffer)
    _check_warp(engine, f"one source image, {out_hw}, perspective={perspective}", src[1], src_np[1], rows, perspective, out_hw, windows=WINDOWS)


@pytest.mark.parametrize("perspective", [False, True], ids=["affine", "perspective"])
def test_a_one_pixel_source(engine, perspective):
    one = np.asarray([[[10, 200, 77]]], np.uint8)
    rows = np.asarray([[1 / 6, 0, 0, 0, 1 / 5, 0, 0, 0], [1, 0, 0, 0, 1, 0, 0, 0], [0.3, 0.1, -0.2, 0.05, 0.2, 0.1, 1e-3, -1e-3]], np.float64)
    got = _check_warp(engine, f"1 x 1 source, perspective={perspective}", torch.from_numpy(one).to(engine.device), one, rows, perspective, (5, 6))
    assert (got[0] == one[0, 0]).all() and (got[1, 0, 0] == one[0, 0]).all() and (got[1, 1:] == np.asarray(FILL, np.uint8)).all()


# ---- 2. identity and the dihedral rows ------------------------------------------------------------------------------------------------
def test_identity_row_is_an_exact_copy(engine):
    from plip_amd.augment import warp_u8
    src, src_np = _source_view(engine), _sources()[:, 2:39, 3:56]
    rows = np.tile(np.asarray(IDENTITY_ROW), (B, 1))
    for perspective in (False, True):
        got = warp_u8(engine, src, rows, perspective=perspective).cpu().numpy()
        _report(f"identity, perspective={perspective}", ("mismatches", int((got != src_np).sum())))
        assert got.shape == (B, H, W, 3) and np.array_equal(got, src_np)


@pytest.mark.parametrize("n", [24, 7])
def test_dihedral_views_equal_numpy(engine, n):
    from plip_amd.augment import dihedral_views
    tiles = np.random.RandomState(n).randint(0, 256, size=(3, n, n, 3), dtype=np.uint8)
    got = dihedral_views(engine, torch.from_numpy(tiles).to(engine.device)).cpu().numpy()
    want = np.stack([np.stack([np.rot90(t if k < 4 else t[:, ::-1], k % 4) for t in tiles]) for k in range(8)])
    _report(f"dihedral views, n={n}", ("mismatches", int((got != want).sum())))
    assert got.shape == (8, 3, n, n, 3) and np.array_equal(got, want)
    assert dihedral_views(engine, torch.from_numpy(tiles).to(engine.device), views=3).shape == (3, 3, n, n, 3)


# ---- 3. the train chain ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _train_case():
    """8 tiles of 96 px, 3 views of 64 px each, and the oracle's bytes [8,3,64,64,3], computed once"""
    tiles = np.random.RandomState(41).randint(0, 256, size=(8, 96, 96, 3), dtype=np.uint8)
    params = train_params(3, 8, 3, (96, 96), 64)
    want = np.stack([np.stack([train_view_reference(tiles[i], params[0][i, v], params[1][i, v], params[2][i, v]) for v in range(3)]) for i in range(8)])
    for a in (tiles, want) + params:
        a.setflags(write=False)
    return tiles, params, want


def test_train_chain_equals_the_pil_chain(engine):
    from plip_amd.augment import train_views
    tiles, params, want = _train_case()
    assert (params[2] != np.asarray(IDENTITY_ROW)).any(axis=-1).sum() >= 3 and (params[2] == np.asarray(IDENTITY_ROW)).all(axis=-1).sum() >= 3
    assert set(params[0][..., 4].reshape(-1).tolist()) == {0, 1}
    got = train_views(engine, torch.from_numpy(tiles.copy()).to(engine.device), params).cpu().numpy().transpose(1, 0, 2, 3, 4)
    diffs = [("bytes", want.size), ("mismatches vs oracle", int((got != want).sum()))]
    if pil() is not None:
        pw = np.stack([np.stack([pil_train_view(tiles[i], params[0][i, v], params[1][i, v], params[2][i, v]) for v in range(3)]) for i in range(8)])
        diffs.append(("mismatches vs the PIL chain", int((got != pw).sum())))
    _report("train chain, 8 tiles x 3 views, 96 -> 64 px", *diffs)
    assert got.shape == want.shape and all(v == 0 for _, v in diffs[1:])


# ---- 4. encode_views ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plips(engines):
    from plip_amd.plip import PLIP
    return {dt: (PLIP(model=engines(CASE, dt)[0]), engines(CASE, dt)[1]) for dt in ("f32", "bf16")}


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, b.shape, a.dtype, b.dtype)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_encode_views_d4_equals_encode_images_on_the_oracle_bytes(plips, dtype):
    plip, cfg = plips[dtype]
    tiles = np.random.RandomState(51).randint(0, 256, size=(8, 64, 64, 3), dtype=np.uint8)
    got, params = plip.encode_views(tiles, batch_size=8, return_params=True)
    assert got.shape == (8, 8, cfg.projection_dim) and got.dtype == np.float32
    plain = plip.encode_images(tiles, batch_size=8)
    oracle = np.stack([np.stack([warp_reference(t, dihedral_coeffs(k, 64)) for k in range(8)]) for t in tiles])
    regenerated = np.stack([np.stack([warp_reference(t, params[1][i, k]) for k in range(8)]) for i, t in enumerate(tiles)])
    want = plip.encode_images(oracle.reshape(64, 64, 64, 3), batch_size=32).reshape(8, 8, -1)
    _report(f"encode_views d4 {dtype}", ("view 0 elements with other bits", _bits(got[:, 0], plain)), ("all views, elements with other bits", _bits(got, want)),
            ("bytes regenerated from the returned rows that differ", int((regenerated != oracle).sum())))
    assert _bits(got[:, 0], plain) == 0 and _bits(got, want) == 0 and np.array_equal(regenerated, oracle)
    assert np.array_equal(oracle[:, 4], tiles[:, :, ::-1])
    few = plip.encode_views(tiles, batch_size=8, views=3)
    assert few.shape == (8, 3, cfg.projection_dim) and _bits(few, got[:, :3]) == 0
    # reduce="mean": the normalised mean of the normalised rows, against float64
    mean = plip.encode_views(tiles, batch_size=8, reduce="mean")
    x = got.astype(np.float64)
    x /= np.linalg.norm(x, axis=-1, keepdims=True)
    m = x.mean(axis=1)
    m /= np.linalg.norm(m, axis=-1, keepdims=True)
    err = float(np.abs(mean.astype(np.float64) - m).max())
    _report(f"reduce=mean {dtype}", ("max |mean - float64 mean|", err))
    assert mean.shape == (8, cfg.projection_dim) and mean.dtype == np.float32 and err <= 1e-6


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_encode_views_train_equals_encode_images_on_the_oracle_bytes(plips, dtype):
    plip, cfg = plips[dtype]
    tiles, params, oracle = _train_case()
    got, used = plip.encode_views(tiles, batch_size=8, views=3, transform="train", seed=3, return_params=True)
    assert all(np.array_equal(a, b) for a, b in zip(used, params))           # the returned rows are the seed's: they regenerate the oracle's bytes
    want = plip.encode_images(oracle.reshape(24, 64, 64, 3).copy(), batch_size=24).reshape(8, 3, -1)
    _report(f"encode_views train {dtype}", ("elements with other bits", _bits(got, want)))
    assert got.shape == (8, 3, cfg.projection_dim) and _bits(got, want) == 0
    other = plip.encode_views(tiles, batch_size=8, views=3, transform="train", seed=4)
    assert _bits(other, got) > 0


def test_encode_views_does_not_depend_on_batch_size_residence_or_lanes(engines, monkeypatch):
    from plip_amd.engine import Engine
    from plip_amd.plip import PLIP
    import plip_amd.augment as A
    model, cfg, *_ = engines(CASE, "f32", 4)
    plip, eng = PLIP(model=model), model.engine
    tiles, _, _ = _train_case()
    used, warps = [], []
    inner, inner_warp = Engine.encode_image_u8, A.warp_u8
    here = lambda e: (id(e), torch.cuda.current_stream(e.device).cuda_stream)
    monkeypatch.setattr(Engine, "encode_image_u8", lambda self, x, normalize=False: (used.append(here(self)), inner(self, x, normalize))[1])
    monkeypatch.setattr(A, "warp_u8", lambda e, *a, **k: (warps.append(here(e)), inner_warp(e, *a, **k))[1])
    assert eng.use_lanes
    for transform, src in (("train", tiles), ("d4", np.ascontiguousarray(tiles[:, 16:80, 16:80]))):
        del used[:], warps[:]
        base = plip.encode_views(src, batch_size=3, views=3, transform=transform, seed=3)
        assert len(used) == 3 and len(set(used)) == 2, used                      # chunks of 3, 3, 2 tiles on two lanes
        per = 4 if transform == "train" else 3                                   # launches per chunk: V affine + 1 perspective, or V
        assert [w for i, w in enumerate(warps) if i % per == 0] == used           # every warp inside its lane: the engine and stream of its encode
        assert all(warps[i] == warps[i - i % per] for i in range(len(warps))) and len(warps) == 3 * per
        forms = {"batch_size=8": lambda: plip.encode_views(src, batch_size=8, views=3, transform=transform, seed=3),
                 "device tensor": lambda: plip.encode_views(torch.from_numpy(src.copy()).to(eng.device), batch_size=3, views=3, transform=transform, seed=3),
                 "list": lambda: plip.encode_views(list(src), batch_size=5, views=3, transform=transform, seed=3)}
        results = {k: fn() for k, fn in forms.items()}
        try:
            eng.use_lanes = False
            del used[:]
            results["lanes off"] = plip.encode_views(src, batch_size=3, views=3, transform=transform, seed=3)
            assert len(set(used)) == 1
        finally:
            eng.use_lanes = True
        for name, out in results.items():
            _report(f"invariance, {transform}, {name}", ("elements with other bits", _bits(out, base)))
            assert _bits(out, base) == 0, (transform, name)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch(engine, plips, monkeypatch):
    from plip_amd import _lib
    from plip_amd._lib import _ptr
    from plip_amd.engine import Engine
    import plip_amd.augment as A
    plip, cfg = plips["f32"]
    launched = []
    inner = Engine.encode_image_u8
    monkeypatch.setattr(Engine, "encode_image_u8", lambda self, x, normalize=False: (launched.append("encode"), inner(self, x, normalize))[1])
    tiles = np.zeros((2, 64, 64, 3), np.uint8)
    for kwargs, match in ((dict(images=np.zeros((2, 63, 80, 3), np.uint8), transform="train"), "smaller than n_px"),
                          (dict(views=9), "eight views"), (dict(images=[tiles[0], np.zeros((64, 65, 3), np.uint8)]), "mixed sizes"),
                          (dict(transform="rot"), "unknown transform"), (dict(images=np.zeros((2, 80, 80, 3), np.uint8)), "encode resolution")):
        args = dict(images=tiles, batch_size=4)
        args.update(kwargs)
        with pytest.raises(ValueError, match=match):
            plip.encode_views(**args)
    # a vanishing denominator: refused by name on the host, the destination untouched
    src = _source_view(engine)
    buf, out = _guarded(engine, B * 24 * 24 * 3)
    rows = _rows(True, (24, 24)).copy()
    rows[3, 6] = -1.0 / 12                      # den = 0 at x = 12
    with pytest.raises(ValueError, match="vanishing denominator"):
        A.warp_u8(engine, src, rows, None, True, (24, 24), FILL, out=out.view(B, 24, 24, 3))
    with pytest.raises(ValueError, match="vanishing denominator"):
        A.train_views(engine, torch.zeros((B, 24, 24, 3), dtype=torch.uint8, device=engine.device),
                      (np.tile(np.asarray([0, 0, 24, 24, 0], np.int32), (B, 1)), np.tile(np.asarray(IDENTITY_ROW), (B, 1)), rows))
    with pytest.raises(ValueError, match="window 1"):
        A.warp_u8(engine, src, rows[:, :6], np.asarray([[0, 0, 5, 5, 0], [30, 0, 8, 5, 0]] + [[0, 0, 1, 1, 0]] * 3, np.int32), False, (24, 24), FILL,
                  out=out.view(B, 24, 24, 3))
    for bad_src, match in ((src.float(), "uint8"), (src.permute(0, 2, 1, 3), "strides"), (src.cpu(), "on the device")):
        with pytest.raises(ValueError, match=match):
            A.warp_u8(engine, bad_src, rows[:, :6])
    with pytest.raises(ValueError, match="coefficient rows"):
        A.warp_u8(engine, src, rows[:3, :6])
    with pytest.raises(ValueError, match="fill"):
        A.warp_u8(engine, src, rows[:, :6], fill=256)
    # the entry's own checks, through the binding
    lib, h, st = engine.lib, engine._h, engine._stream()
    co = torch.from_numpy(_rows(False, (24, 24))).to(engine.device)
    call = lambda **k: lib.plipmi_warp_u8(h, _ptr(src), k.get("B", B), H, W, k.get("pitch", 171), k.get("stride", 7011), None, _ptr(co), k.get("persp", 0),
                                          24, k.get("ow", 24), k.get("fill", 127), _ptr(out), st)
    for kw, msg in ((dict(pitch=158), "pitch_bytes 158"), (dict(stride=-1), "image_stride_bytes -1"), (dict(persp=2), "perspective 2"),
                    (dict(ow=0), "an output of 24 x 0"), (dict(fill=1 << 24), "fill_rgb"), (dict(B=-2), "B -2"), (dict(pitch=2 ** 31), "2 GiB")):
        rc = call(**kw)
        assert rc == 1 and msg in _lib.last_error(), (kw, rc, _lib.last_error())
    torch.cuda.synchronize(engine.device)
    assert launched == [] and bool((buf == SENTINEL).all())           # nothing was launched


def test_train_views_checks_every_view_before_its_first_launch(engine, monkeypatch):
    """a bad window, fill or row in the LAST view raises before the first view's launch"""
    import plip_amd.augment as A
    tiles, params, _ = _train_case()
    src = torch.from_numpy(tiles.copy()).to(engine.device)
    launches = []
    inner = A.warp_u8
    monkeypatch.setattr(A, "warp_u8", lambda e, *a, **k: (launches.append(1), inner(e, *a, **k))[1])
    windows, affine, persp = (p.copy() for p in params)
    bad_window = windows.copy()
    bad_window[5, 2, :2] = (40, 0)                        # 40 + 64 > 96
    bad_persp = persp.copy()
    bad_persp[7, 2] = [1, 0, 0, 0, 1, 0, -1.0 / 32, 0]
    for bad, kw, match in (((bad_window, affine, persp), {}, r"window \[5, 2\]"), ((windows, affine, bad_persp), {}, "vanishing denominator"),
                           ((windows, affine, persp), dict(fill=300), "fill"), ((windows.astype(np.float32), affine, persp), {}, "integer"),
                           ((windows, affine[..., :5], persp), {}, "coefficients")):
        with pytest.raises(ValueError, match=match):
            A.train_views(engine, src, bad, **kw)
    with pytest.raises(ValueError, match="on the device"):
        A.train_views(engine, src.cpu(), (windows, affine, persp))
    assert launches == []


def test_rows_and_windows_built_on_the_device_are_refused_there(engine):
    """what the host layers never pass on, given to the entry itself: a perspective row whose denominator vanishes inside the output
    and windows outside the source come out all fill -- no fault, no address outside the source, the other images untouched by it"""
    from plip_amd import _lib
    from plip_amd._lib import _ptr
    src, src_np = _source_view(engine), _sources()[:, 2:39, 3:56]
    rows = _rows(True, (24, 24)).copy()
    rows[0, 6] = -1.0 / 12
    rows[4, 7] = float("nan")
    wins = np.tile(np.asarray([0, 0, H, W, 0], np.int32), (B, 1))
    wins[2] = [30, 0, 8, 5, 0]                                        # 30 + 8 > 37
    wins[3] = [0, -1, 5, 5, 1]
    buf, out = _guarded(engine, B * 24 * 24 * 3)
    co, wi = torch.from_numpy(rows).to(engine.device), torch.from_numpy(wins).to(engine.device)
    fill = FILL[0] | FILL[1] << 8 | FILL[2] << 16
    _lib.check(engine.lib.plipmi_warp_u8(engine._h, _ptr(src), B, H, W, 171, 7011, _ptr(wi), _ptr(co), 1, 24, 24, fill, _ptr(out), engine._stream()),
               "plipmi_warp_u8")
    torch.cuda.synchronize(engine.device)
    got = out.view(B, 24, 24, 3).cpu().numpy()
    for b in (0, 2, 3, 4):
        assert (got[b] == np.asarray(FILL, np.uint8)).all(), b
    assert np.array_equal(got[1], warp_reference(src_np[1], rows[1], True, (24, 24), FILL)) and (got[1] != np.asarray(FILL, np.uint8)).any()
    assert bool((buf[B * 24 * 24 * 3:] == SENTINEL).all())
