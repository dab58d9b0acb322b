"""Macenko stain normalisation on the GPU (csrc/stain.hip) against the float64 numpy oracle of plip_amd/preprocess.py: the exact
percentile kernel, the apply kernel on oracle fits, the fit, fit + apply end to end, the routes through ``PLIP`` and the refusals.
Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

import stain_common as SC
from plip_amd import preprocess as PP

pytestmark = pytest.mark.gpu

CASE = "tiny_b6"          # 64 px tiles, 16 px patches
H, W, B = 37, 53, 5
SENTINEL, GUARD = 0xA5, 64


def _report(what, *figures):
    print(f"stain parity: {what}: " + ", ".join(f"{k} {v}" for k, v in figures))


@pytest.fixture(scope="module")
def engine(engines):
    return engines(CASE, "f32")[0].engine


# ---- 1. the percentile kernel, exact -----------------------------------------------------------------------------------------------------
def _percentile_keys(n=5000):
    """[3, n] float32: ties, negatives, both zeros, subnormals, neighbours in the lowest key bits; segment 1 about 40 % absent,
    segment 2 one key present"""
    rs = np.random.RandomState(7)
    k = rs.standard_normal((3, n)).astype(np.float32)
    k[:, 0:400] = np.round(k[:, 0:400] * 4) / 4                                   # ties
    k[:, 400:420] = 0.0
    k[:, 420:440] = -0.0
    k[:, 440:470] = (rs.randint(1, 1 << 22, (3, 30)).astype(np.uint32)).view(np.float32)                   # subnormals
    k[:, 470:500] = -(rs.randint(1, 1 << 22, (3, 30)).astype(np.uint32)).view(np.float32)
    base = np.float32(0.7371).view(np.uint32)
    k[:, 500:900] = (base + rs.randint(0, 5, (3, 400)).astype(np.uint32)).view(np.float32)                 # differ in the last bits only
    k[:, 900:1300] = -(base + rs.randint(0, 2000, (3, 400)).astype(np.uint32)).view(np.float32)            # and across the 10-bit pass
    for s in range(3):
        k[s] = k[s][rs.permutation(n)]
    k[1, rs.random_sample(n) < 0.4] = np.nan
    keep = k[2, 1234]
    k[2] = np.nan
    k[2, 1234] = keep
    return k


def _check_percentiles(engine, keys, qs, what):
    from plip_amd.kernel_entries import stain_percentile
    S, Q = keys.shape[0], len(qs)
    buf = torch.full((GUARD + S * Q + GUARD,), float(SENTINEL), dtype=torch.float64, device=engine.device)
    out, counts = stain_percentile(engine, torch.from_numpy(keys).to(engine.device), qs, out=buf[GUARD:GUARD + S * Q])
    torch.cuda.synchronize(engine.device)
    got, cnt, buf = out.cpu().numpy().reshape(S, Q), counts.cpu().numpy(), buf.cpu().numpy()
    want = np.array([[PP.stain_percentile(keys[s][~np.isnan(keys[s])], q) for q in qs] for s in range(S)])
    want_np = np.array([[np.percentile(keys[s][~np.isnan(keys[s])].astype(np.float64), q) for q in qs] for s in range(S)])
    want_cnt = (~np.isnan(keys)).sum(axis=1)
    bad = int((got != want).sum())
    guard = int((buf[:GUARD] != SENTINEL).sum() + (buf[GUARD + S * Q:] != SENTINEL).sum())
    _report(what, ("values", S * Q), ("unequal to the oracle", bad), ("oracle unequal to np.percentile", int((want != want_np).sum())),
            ("counts", cnt.tolist()), ("want", want_cnt.tolist()), ("guard values touched", guard))
    assert bad == 0 and np.array_equal(want, want_np) and np.array_equal(cnt, want_cnt) and guard == 0, what


def test_percentile_kernel_is_exact(engine):
    keys = _percentile_keys()
    assert 0.3 < np.isnan(keys[1]).mean() < 0.5 and (~np.isnan(keys[2])).sum() == 1
    _check_percentiles(engine, keys, [0, 1, 50, 99, 100], "percentile 3 x 5000")
    _check_percentiles(engine, np.asarray([[-2.5]], np.float32), [0, 1, 50, 99, 100], "percentile n = 1")
    _check_percentiles(engine, np.asarray([[3.0, -1.0], [np.nan, 0.25]], np.float32), [0, 37.5, 50, 100], "percentile n = 2")


# ---- shared sources and oracle fits ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sources():
    """uint8 [5,41,57,3] of synthetic H&E (image 3 glass); the sources are its [:, 2:39, 3:56]: a pitch of 171 bytes (odd) and images
    7011 bytes apart, not H * pitch -- the layout of test_gpu_augment._sources"""
    big = np.stack([SC.glass_tile(b, 41, 57) if b == 3 else SC.he_tile(40 + b, 41, 57, strength=(1.0 + 0.2 * b, 1.0 - 0.1 * b)) for b in range(B)])
    big.setflags(write=False)
    return big


def _source_view(engine):
    big = torch.from_numpy(_sources().copy()).to(engine.device)
    view = big[:, 2:39, 3:56]
    assert tuple(view.shape) == (B, H, W, 3) and view.stride() == (41 * 171, 171, 3, 1)
    return view


@functools.lru_cache(maxsize=None)
def _tiles():
    """uint8 [4,64,64,3]: three H&E tiles of differing strength and one all-glass tile (index 2)"""
    t = np.stack([SC.he_tile(0), SC.he_tile(1, strength=(1.3, 0.8)), SC.glass_tile(5), SC.he_tile(2, strength=(0.8, 1.2))])
    t.setflags(write=False)
    return t


def _stainfit(engine, rows):
    from plip_amd.stain import StainFit
    return StainFit(torch.from_numpy(np.ascontiguousarray(rows)).to(engine.device), rows.shape[0] == 1, 1)


# ---- 2. the apply kernel alone, on the oracle's fits --------------------------------------------------------------------------------------
def _compare_bytes(got, want, unrounded, eps, what, max_exempt, copied=()):
    """mismatches outside / inside the exempt set = the bytes whose unrounded oracle value lies within eps of an integer; the images
    ``copied`` (an invalid fit: the source's bytes) have no exempt bytes"""
    with np.errstate(invalid="ignore"):
        near = np.abs(unrounded - np.rint(unrounded)) <= eps
    for b in copied:
        near[b] = False
    diff = got != want
    by_more = int((np.abs(got.astype(np.int32) - want.astype(np.int32)) > 1).sum())
    _report(what, ("bytes", want.size), ("exempt", int(near.sum())), ("differing", int(diff.sum())), ("differing outside the exempt", int((diff & ~near).sum())),
            ("differing by more than one", by_more))
    assert int((diff & ~near).sum()) == 0 and by_more == 0 and near.sum() <= max_exempt * want.size, what


@pytest.mark.parametrize("n_fits", [5, 1])
@pytest.mark.parametrize("target", ["default", "fit"])
def test_apply_kernel_equals_the_oracle_on_a_strided_source(engine, n_fits, target):
    from plip_amd.kernel_entries import stain_apply_into
    from plip_amd.stain import _lut
    src_np = _sources()[:, 2:39, 3:56]
    rows = PP.stain_fit_reference(src_np)
    assert rows[:, 15].tolist() == [1, 1, 1, 0, 1]
    if n_fits == 1:
        rows = rows[3:4] if target == "fit" else rows[1:2]            # (one invalid fit for all: every image copied; one valid for all)
    tg = PP.stain_target(None if target == "default" else PP.stain_fit_reference(SC.he_tile(9, he=PP.HE_REF))[0])
    want = PP.stain_apply_reference(src_np, rows, tg)
    unrounded = PP.stain_apply_reference(src_np, rows, tg, unrounded=True)
    src = _source_view(engine)
    n = B * H * W * 3
    for offset in (0, 1):                                             # (37 x 53 fits no wide store; the offset moves dst's alignment all the same)
        buf = torch.full((offset + n + GUARD,), SENTINEL, dtype=torch.uint8, device=engine.device)
        stain_apply_into(engine, src, torch.from_numpy(rows).to(engine.device), torch.from_numpy(tg).to(engine.device), _lut(engine, 240.0),
                         buf[offset:offset + n])
        torch.cuda.synchronize(engine.device)
        host = buf.cpu().numpy()
        got = host[offset:offset + n].reshape(B, H, W, 3)
        guard = int((host[:offset] != SENTINEL).sum() + (host[offset + n:] != SENTINEL).sum())
        _report(f"apply {n_fits} fits, {target} target, offset {offset}", ("guard bytes touched", guard))
        copied = [b for b in range(B) if rows[b if n_fits == 5 else 0, 15] == 0]
        _compare_bytes(got, want, unrounded, 1e-9, f"apply {n_fits} fits, {target} target, offset {offset}", 1e-4, copied)
        assert guard == 0 and copied == ([3] if n_fits == 5 else list(range(B)) if target == "fit" else [])
        for b in copied:
            assert np.array_equal(got[b], src_np[b])                  # an invalid fit: the source's bytes


def test_apply_wide_paths_equal_the_byte_path(engine):
    """64 x 64 contiguous takes dword loads and stores; the same tiles one byte into an allocation take byte loads and dword stores"""
    from plip_amd.stain import stain_apply
    tiles = _tiles()
    rows = PP.stain_fit_reference(tiles)
    want = PP.stain_apply_reference(tiles, rows)
    unrounded = PP.stain_apply_reference(tiles, rows, unrounded=True)
    dev = torch.from_numpy(tiles.copy()).to(engine.device)
    shifted = torch.empty((tiles.size + 1,), dtype=torch.uint8, device=engine.device)[1:].view(tiles.shape)
    shifted.copy_(dev)
    for what, x in (("wide", dev), ("byte loads", shifted)):
        got = stain_apply(engine, x, _stainfit(engine, rows)).cpu().numpy()
        _compare_bytes(got, want, unrounded, 1e-9, f"apply 64 x 64 {what}", 1e-4, [2])
        assert np.array_equal(got[2], tiles[2])


# ---- 3. the fit --------------------------------------------------------------------------------------------------------------------------
def _fit_errors(got, want):
    he = float(np.abs(got[:, 0:12] - want[:, 0:12]).max())
    valid = want[:, 15] != 0
    mc = float((np.abs(got[valid, 12:14] - want[valid, 12:14]) / want[valid, 12:14]).max()) if valid.any() else 0.0
    return he, mc


@pytest.mark.parametrize("pooled", [False, True], ids=["per tile", "pooled"])
@pytest.mark.parametrize("step", [1, 3])
def test_fit_equals_the_oracle(engine, step, pooled):
    from plip_amd.stain import stain_fit
    cases = {"64 x 64": (torch.from_numpy(_tiles().copy()).to(engine.device), _tiles()),
             "37 x 53 strided": (_source_view(engine)[1:2], _sources()[1:2, 2:39, 3:56])}
    for name, (dev, host) in cases.items():
        want = PP.stain_fit_reference(host, pooled=pooled, step=step)
        a = stain_fit(engine, dev, pooled=pooled, step=step).numpy()
        b = stain_fit(engine, dev, pooled=pooled, step=step).numpy()
        he, mc = _fit_errors(a, want)
        _report(f"fit {name} step {step} {'pooled' if pooled else 'per tile'}", ("n", a[:, 14].tolist()), ("want", want[:, 14].tolist()),
                ("valid", a[:, 15].tolist()), ("want", want[:, 15].tolist()), ("max |HE, P - oracle|", he), ("max rel maxC error", mc),
                ("elements with other bits on a second run", int((a.view(np.uint64) != b.view(np.uint64)).sum())))
        assert a.shape == want.shape and np.array_equal(a[:, 14], want[:, 14]) and np.array_equal(a[:, 15], want[:, 15])
        assert he <= 1e-6 and mc <= 1e-6
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        assert np.isfinite(a).all()
    if not pooled:
        assert stain_fit(engine, cases["64 x 64"][0], step=step).numpy()[:, 15].tolist() == [1, 1, 0, 1]


def test_fit_stain_on_the_host_and_on_the_device_gives_the_same_bits(engines):
    from plip_amd.plip import PLIP
    plip = PLIP(model=engines(CASE, "f32")[0])
    region = SC.he_tile(77, 200, 264)
    on_host = plip.fit_stain(region, step=3)
    on_dev = plip.fit_stain(torch.from_numpy(region.copy()).to(plip.model.engine.device), step=3)
    a, b = on_host.numpy(), on_dev.numpy()
    want = PP.stain_fit_reference(region, pooled=True, step=3)
    he, mc = _fit_errors(a, want)
    _report("fit_stain host vs device, step 3", ("elements with other bits", int((a.view(np.uint64) != b.view(np.uint64)).sum())), ("max |HE, P - oracle|", he),
            ("max rel maxC error", mc))
    assert len(on_host) == 1 and on_host.step == 3 and np.array_equal(a.view(np.uint64), b.view(np.uint64)) and a[0, 15] == 1
    assert he <= 1e-6 and mc <= 1e-6
    tiles = _tiles()
    per = plip.fit_stain(tiles, pooled=False)
    assert len(per) == 4 and per.step == 1 and np.array_equal(per.numpy()[:, 14], PP.stain_fit_reference(tiles)[:, 14])


# ---- 4. fit then apply, end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooled", [False, True], ids=["per tile", "pooled"])
def test_fit_then_apply_equals_the_oracle_end_to_end(engine, pooled):
    from plip_amd.stain import stain_apply, stain_fit
    tiles = _tiles()
    dev = torch.from_numpy(tiles.copy()).to(engine.device)
    got = stain_apply(engine, dev, stain_fit(engine, dev, pooled=pooled)).cpu().numpy()
    rows = PP.stain_fit_reference(tiles, pooled=pooled)
    want = PP.stain_apply_reference(tiles, rows)
    unrounded = PP.stain_apply_reference(tiles, rows, unrounded=True)
    _compare_bytes(got, want, unrounded, 2e-3, f"fit + apply {'pooled' if pooled else 'per tile'}", 1e-2, [] if pooled else [2])
    if not pooled:
        assert np.array_equal(got[2], tiles[2])


# ---- 5. routes ---------------------------------------------------------------------------------------------------------------------------
def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, b.shape, a.dtype, b.dtype)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


@functools.lru_cache(maxsize=None)
def _region():
    r = SC.he_tile(31, 200, 264, glass=0.15)
    r.setflags(write=False)
    return r


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_encode_region_with_stain_equals_encode_images_on_the_normalised_crops(engines, dtype):
    from plip_amd.plip import PLIP
    from plip_amd.stain import stain_apply
    model, cfg, *_ = engines(CASE, dtype, 4)
    plip, eng = PLIP(model=model), model.engine
    region = _region()
    fit = plip.fit_stain(region, step=2)
    plain = plip.encode_region(region)
    assert plain.grid == (3, 4) and len(plain.kept) >= 8, (plain.grid, plain.kept)          # several batches of max_batch 4, two lanes
    crops = np.stack([region[y:y + 64, x:x + 64] for y, x in plain.coords])
    normalised = stain_apply(eng, torch.from_numpy(crops).to(eng.device), fit)
    want = plip.encode_images(normalised, batch_size=4)
    want_oracle = PP.stain_apply_reference(crops, PP.stain_fit_reference(region, pooled=True, step=2))
    _report(f"routes {dtype}", ("normalised bytes differing from the oracle's", int((normalised.cpu().numpy() != want_oracle).sum())), ("of", want_oracle.size))
    forms = {"host": lambda: plip.encode_region(region, stain=fit),
             "host, band_rows=1": lambda: plip.encode_region(region, stain=fit, band_rows=1),
             "device": lambda: plip.encode_region(torch.from_numpy(region.copy()).to(eng.device), stain=fit),
             "device, band_rows=2": lambda: plip.encode_region(torch.from_numpy(region.copy()).to(eng.device), stain=fit, band_rows=2)}
    results = {k: fn() for k, fn in forms.items()}
    try:
        eng.use_lanes = False
        results["lanes off"] = plip.encode_region(region, stain=fit)
    finally:
        eng.use_lanes = True
    for name, out in results.items():
        _report(f"routes {dtype}, {name}", ("elements with other bits", _bits(out.embeddings, want)))
        assert _bits(out.embeddings, want) == 0 and np.array_equal(out.kept, plain.kept) and np.array_equal(out.tissue, plain.tissue), name
    assert _bits(want, plain.embeddings) > 0                                                  # the normalisation changed the tiles
    none = plip.encode_region(region, stain=None)
    assert _bits(none.embeddings, plain.embeddings) == 0 and np.array_equal(none.kept, plain.kept)


def test_normalize_stain_routes(engines):
    from plip_amd.plip import PLIP
    plip = PLIP(model=engines(CASE, "f32")[0])
    tiles = _tiles()
    per_tile = plip.normalize_stain(tiles, fit="tile").cpu().numpy()
    each = np.stack([plip.normalize_stain(tiles[i:i + 1], fit="tile").cpu().numpy()[0] for i in range(len(tiles))])
    pooled = plip.normalize_stain(list(tiles), fit="pooled").cpu().numpy()
    one = plip.fit_stain(tiles, pooled=True, step=1)
    given = plip.normalize_stain(torch.from_numpy(tiles.copy()), fit=one).cpu().numpy()
    to_other = plip.normalize_stain(tiles, fit="tile", target=plip.fit_stain(tiles[3], step=1)).cpu().numpy()
    _report("normalize_stain", ("tile vs per-image calls, bytes differing", int((per_tile != each).sum())), ("pooled vs given fit", int((pooled != given).sum())))
    assert per_tile.dtype == np.uint8 and per_tile.shape == tiles.shape and np.array_equal(per_tile, each) and np.array_equal(pooled, given)
    assert np.array_equal(per_tile[2], tiles[2]) and not np.array_equal(per_tile[0], tiles[0]) and not np.array_equal(to_other, per_tile)
    assert plip.encode_images(plip.normalize_stain(tiles), batch_size=4).shape[0] == 4


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(engine):
    from plip_amd import _lib
    from plip_amd._lib import _ptr
    from plip_amd.stain import _lut, stain_apply, stain_fit
    src = _source_view(engine)
    lib, h, st = engine.lib, engine._h, engine._stream()
    lut = _lut(engine, 240.0)
    fits = torch.full((B, 16), float(SENTINEL), dtype=torch.float64, device=engine.device)
    dst = torch.full((B * H * W * 3,), SENTINEL, dtype=torch.uint8, device=engine.device)
    ws = torch.full((int(lib.plipmi_stain_workspace(B, H, W, 1)),), SENTINEL, dtype=torch.uint8, device=engine.device)
    tg = torch.from_numpy(PP.stain_target(None)).to(engine.device)
    odd = torch.zeros((40,), dtype=torch.uint8, device=engine.device)[4:]           # a double buffer 4 bytes off
    fit_call = lambda **k: lib.plipmi_stain_fit(h, k.get("src", _ptr(src)), k.get("B", B), k.get("H", H), W, k.get("pitch", 171), k.get("stride", 7011),
                                                k.get("step", 1), k.get("pooled", 0), k.get("Io", 240.0), k.get("alpha", 1.0), k.get("beta", 0.15),
                                                k.get("lut", _ptr(lut)), k.get("ws", _ptr(ws)), k.get("fits", _ptr(fits)), st)
    for kw, msg in ((dict(pitch=158), "pitch_bytes 158"), (dict(stride=-1), "image_stride_bytes -1"), (dict(B=-2), "B -2"), (dict(H=0), "0 x 53"),
                    (dict(step=0), "step 0"), (dict(pitch=2 ** 31), "2 GiB"), (dict(alpha=0.0), "alpha 0"), (dict(alpha=50.0), "alpha 50"),
                    (dict(Io=0.0), "Io 0"), (dict(beta=-0.1), "beta -0.1"), (dict(src=None), "null src"), (dict(lut=None), "null lut_dev"),
                    (dict(ws=None), "null workspace"), (dict(fits=None), "null fits_out"), (dict(fits=_ptr(odd)), "8-byte aligned"),
                    (dict(pooled=2), "pooled 2")):
        rc = fit_call(**kw)
        assert rc == 1 and msg in _lib.last_error(), (kw, rc, _lib.last_error())
    apply_call = lambda **k: lib.plipmi_stain_apply(h, k.get("src", _ptr(src)), k.get("B", B), H, k.get("W", W), k.get("pitch", 171), k.get("stride", 7011),
                                                    k.get("fits", _ptr(fits)), k.get("n_fits", B), k.get("tg", _ptr(tg)), k.get("Io", 240.0),
                                                    k.get("lut", _ptr(lut)), k.get("dst", _ptr(dst)), st)
    for kw, msg in ((dict(pitch=158), "pitch_bytes 158"), (dict(n_fits=2), "n_fits 2"), (dict(n_fits=0), "n_fits 0"), (dict(W=0), "37 x 0"),
                    (dict(Io=-1.0), "Io -1"), (dict(dst=None), "null dst"), (dict(fits=None), "null fits"), (dict(tg=None), "null target_dev"),
                    (dict(tg=_ptr(odd)), "8-byte aligned"), (dict(pitch=2 ** 31), "2 GiB")):
        rc = apply_call(**kw)
        assert rc == 1 and msg in _lib.last_error(), (kw, rc, _lib.last_error())
    assert fit_call(B=0) == 0 and apply_call(B=0) == 0                                  # B == 0 launches nothing
    # the Python layer, on a live engine
    with pytest.raises(ValueError, match="uint8"):
        stain_fit(engine, src.float())
    with pytest.raises(ValueError, match="strides"):
        stain_fit(engine, src.permute(0, 2, 1, 3))
    with pytest.raises(ValueError, match="1 row or of 5"):
        stain_apply(engine, src, _stainfit(engine, np.zeros((2, 16))))
    torch.cuda.synchronize(engine.device)
    assert bool((fits == float(SENTINEL)).all()) and bool((dst == SENTINEL).all()) and bool((ws == SENTINEL).all())      # nothing was launched
