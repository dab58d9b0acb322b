"""Slide regions on the MI355X (include/plipmi.h plipmi_region_select / plipmi_region_gather, plip_amd/engine_region.py,
PLIP.encode_region): the selection against the numpy oracle (plip_amd/preprocess.py), the gather against numpy slicing, and the
embeddings against ``PLIP.encode_images`` on the same tiles cut on the host -- all exact: integers, bytes and bit-equal floats.  Every
difference is printed before it is asserted (profiles/region_parity.txt keeps the output of one run)."""
import numpy as np
import pytest
import torch

from region_common import GRIDS, REGION_HW, host_crops, oracle_selection, synthetic_region

from plip_amd.preprocess import region_grid, region_min_count, region_tile_counts, tissue_mask

pytestmark = pytest.mark.gpu

CASE = "tiny_b6"          # 64 px tiles, 16 px patches


def _report(what, *diffs):
    print(f"region parity: {what}: " + ", ".join(f"{k} {v}" for k, v in diffs))


def _float_diff(a, b):
    """largest |a - b| of two float arrays of one shape, and how many elements differ in their bits"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, b.shape, a.dtype, b.dtype)
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) if a.size else 0.0, int((a.view(np.uint32) != b.view(np.uint32)).sum())


@pytest.fixture(scope="module")
def engine(engines):
    return engines(CASE, "f32")[0].engine


@pytest.fixture(scope="module")
def region_dev(engine):
    return torch.from_numpy(synthetic_region().copy()).to(engine.device)


def _strided_view(engine):
    """the same region as rows 7 .. 207, columns 11 .. 342 of a larger tensor: a row stride of 400 * 3 bytes, a base that is no multiple of 4"""
    big = torch.randint(0, 256, (230, 400, 3), dtype=torch.uint8, device=engine.device)
    big[7:207, 11:342] = torch.from_numpy(synthetic_region().copy()).to(engine.device)
    view = big[7:207, 11:342]
    assert view.stride() == (1200, 3, 1) and not view.is_contiguous()
    return view


# ---- 1. select == oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "row_strided_view"])
@pytest.mark.parametrize("grid", list(GRIDS), ids=lambda g: f"o{g[0][0]}_{g[0][1]}_t{g[1]}_s{g[2]}")
def test_select_equals_the_numpy_oracle(engine, region_dev, grid, strided):
    from plip_amd.engine_region import region_select
    origin, t, s = grid
    want_counts, want_kept, _ = oracle_selection(origin, t, s)
    region = _strided_view(engine) if strided else region_dev
    counts, kept, n_kept = region_select(engine, region, t, s, origin)
    K = int(n_kept.item())
    counts, kept = counts.cpu().numpy(), kept.cpu().numpy()
    _report(f"select {grid} strided={strided}", ("count differences", int((counts != want_counts).sum())), ("K", K),
            ("kept differences", int(K != len(want_kept) or (kept[:K] != want_kept).sum())))
    assert counts.dtype == np.int32 and counts.shape == want_counts.shape and np.array_equal(counts, want_counts)
    assert K == len(want_kept) == GRIDS[grid][0] and np.array_equal(kept[:K], want_kept)


def test_select_with_other_thresholds_and_an_odd_tile(engine, region_dev):
    """thresholds are arguments, and a tile size that is no multiple of 4 takes the row tail's byte loads: t = 37, stride 29"""
    from plip_amd.engine_region import region_select
    region = synthetic_region()
    for t, s, origin, th, min_tissue in ((37, 29, (2, 1), dict(sat_min=18, luma_min=25, luma_max=235), 0.5),
                                         (64, 64, (3, 5), dict(sat_min=120, luma_min=60, luma_max=200), 0.3),
                                         (64, 64, (0, 0), dict(sat_min=0, luma_min=0, luma_max=255), 1.0),
                                         (1, 1, (0, 0), dict(sat_min=18, luma_min=25, luma_max=235), 0.5)):
        want = region_tile_counts(region, t, s, origin, **th)
        want_kept = np.flatnonzero(want.reshape(-1) >= region_min_count(min_tissue, t))
        counts, kept, n_kept = region_select(engine, region_dev, t, s, origin, min_tissue=min_tissue, **th)
        K = int(n_kept.item())
        _report(f"select t={t} s={s} {th}", ("count differences", int((counts.cpu().numpy() != want).sum())), ("K", K))
        assert np.array_equal(counts.cpu().numpy(), want) and K == len(want_kept) and np.array_equal(kept.cpu().numpy()[:K], want_kept)
    assert K > 256      # the 1-pixel grid: 66200 tiles, more kept indices than the compaction has threads


# ---- 2. threshold boundary ----------------------------------------------------------------------------------------------------------
def test_a_tile_with_exactly_min_count_is_kept_and_one_below_is_dropped(engine):
    from plip_amd.engine_region import region_select
    t = 64
    min_count = region_min_count(0.5, t)
    assert min_count == 2048
    region = np.full((t + 5, 2 * t + 9, 3), 240, np.uint8)               # glass
    flat = np.zeros((t * t, 3), np.uint8)
    flat[:] = 240
    for j, n in enumerate((min_count, min_count - 1)):                  # tile 0: exactly min_count pink pixels, tile 1: one fewer
        tile = flat.copy()
        tile[np.random.RandomState(j).permutation(t * t)[:n]] = (220, 160, 200)
        region[3:3 + t, 7 + j * t:7 + (j + 1) * t] = tile.reshape(t, t, 3)
    assert tissue_mask(region).sum() == 2 * min_count - 1
    counts, kept, n_kept = region_select(engine, torch.from_numpy(region).to(engine.device), t, t, (3, 7))
    K = int(n_kept.item())
    _report("threshold boundary", ("counts", counts.cpu().numpy().tolist()), ("kept", kept.cpu().numpy()[:K].tolist()))
    assert counts.cpu().numpy().tolist() == [[min_count, min_count - 1]] and K == 1 and int(kept[0]) == 0


# ---- 3. gather == slicing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x0", [0, 1, 2, 5])
def test_gather_equals_numpy_slicing(engine, region_dev, x0):
    """every source alignment: the pitch is odd, so the rows of one tile already start at every byte offset mod 16; x0 moves the tile's
    own base.  t = 64 and 96 take the 16-byte kernel, t = 37 the byte kernel; ``first`` > 0 and a ``B`` short of the list both occur."""
    from plip_amd.engine_region import region_gather, region_select
    region = synthetic_region()
    for t, s, y0 in ((64, 40, 0), (96, 96, 1), (37, 29, 2)):
        origin = (y0, x0)
        _, kept, n_kept = region_select(engine, region_dev, t, s, origin)
        K = int(n_kept.item())
        rows, cols = region_grid(*REGION_HW, t, s, origin)
        idx = kept.cpu().numpy()[:K]
        assert K >= 2
        for first, B in ((0, K), (1, K - 1), (1, max(K - 2, 1)), (K - 1, 1), (0, 0)):
            got = region_gather(engine, region_dev, kept, first, B, t, s, origin).cpu().numpy()
            want = np.stack([region[y0 + (i // cols) * s:, x0 + (i % cols) * s:][:t, :t] for i in idx[first:first + B]]) if B else \
                np.zeros((0, t, t, 3), np.uint8)
            _report(f"gather t={t} s={s} origin={origin} first={first} B={B}", ("byte differences", int((got != want).sum())))
            assert got.dtype == np.uint8 and got.shape == (B, t, t, 3) and np.array_equal(got, want)
    # the caller's own list, with indices outside the grid: clamped to its first / last tile
    own = torch.tensor([rows * cols + 7, -3, 0], dtype=torch.int32, device=engine.device)
    got = region_gather(engine, region_dev, own, 0, 3, t, s, origin).cpu().numpy()
    last = region[y0 + (rows - 1) * s:, x0 + (cols - 1) * s:][:t, :t]
    assert np.array_equal(got[0], last) and np.array_equal(got[1], region[y0:y0 + t, x0:x0 + t]) and np.array_equal(got[1], got[2])


def test_gather_from_a_row_strided_view(engine):
    from plip_amd.engine_region import region_gather, region_select
    view, region = _strided_view(engine), synthetic_region()
    origin, t, s = (3, 5), 64, 64
    _, want_kept, coords = oracle_selection(origin, t, s)
    _, kept, n_kept = region_select(engine, view, t, s, origin)
    got = region_gather(engine, view, kept, 0, int(n_kept.item()), t, s, origin).cpu().numpy()
    want = np.stack(host_crops(region, coords, t))
    _report("gather from a view", ("byte differences", int(got.shape != want.shape or (got != want).sum())))
    assert np.array_equal(got, want)


# ---- 4 / 5. embeddings == encode_images on the host crops ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plips(engines):
    from plip_amd.plip import PLIP
    return {dt: (PLIP(model=engines(CASE, dt)[0]), engines(CASE, dt)[1]) for dt in ("f32", "bf16")}


def _check_against_host_crops(plip, cfg, grid, what, **kw):
    origin, t, s = grid
    region = synthetic_region()
    counts, kept, coords = oracle_selection(origin, t, s)
    want = plip.encode_images(host_crops(region, coords, t), batch_size=4)
    out = plip.encode_region(region, tile_px=t, stride=s, origin=origin, **kw)
    d, nbits = _float_diff(out.embeddings, want)
    tissue = (counts.astype(np.float32) / np.float32(t * t))
    _report(f"{what} {grid}", ("max |encode_region - encode_images|", d), ("elements with other bits", nbits),
            ("kept differences", int(len(out.kept) != len(kept) or (out.kept != kept).sum())),
            ("coords differences", int(out.coords.shape != coords.shape or (out.coords != coords).sum())),
            ("tissue differences", int(out.tissue.shape != tissue.shape or (out.tissue != tissue).sum())))
    assert out.embeddings.shape == (len(kept), cfg.projection_dim) and nbits == 0 and d == 0.0
    assert out.kept.dtype == np.int64 and np.array_equal(out.kept, kept)
    assert out.coords.dtype == np.int64 and np.array_equal(out.coords, coords)
    assert out.grid == counts.shape and out.tissue.dtype == np.float32 and np.array_equal(out.tissue, tissue)
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_embeddings_equal_encode_images_on_the_same_tiles(plips, dtype):
    """t = 64, the encode resolution: gather, then encode_image_u8 -- the "tiles" route of the host list"""
    plip, cfg = plips[dtype]
    assert cfg.image_size == 64
    for grid in (((3, 5), 64, 64), ((0, 0), 64, 40)):
        _check_against_host_crops(plip, cfg, grid, f"same size {dtype}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_embeddings_of_resized_tiles_equal_the_resize_route(plips, dtype, monkeypatch):
    """t = 96 on a 64 px engine: gather, resize_crop_u8(crop="hf"), encode_image_u8 -- the "resize" route of the host list, which is
    checked to be the route the host crops took"""
    from plip_amd.engine import Engine
    plip, cfg = plips[dtype]
    crops = []
    inner = Engine.resize_crop_u8
    monkeypatch.setattr(Engine, "resize_crop_u8", lambda self, x, crop="torchvision": (crops.append((tuple(x.shape), crop)), inner(self, x, crop=crop))[1])
    _check_against_host_crops(plip, cfg, ((1, 2), 96, 96), f"resized {dtype}")
    assert crops == [((2, 96, 96, 3), "hf")] * 2          # once for the host list, once inside encode_region
    # and at image_size = 96 the same tiles are native: no resize, the at_resolution engine
    del crops[:]
    region, (_, _, coords) = synthetic_region(), oracle_selection((1, 2), 96, 96)
    want = plip.encode_images(host_crops(region, coords, 96), batch_size=4, image_size=96)
    out = plip.encode_region(region, stride=96, origin=(1, 2), image_size=96)           # tile_px defaults to the encode resolution
    d, nbits = _float_diff(out.embeddings, want)
    _report(f"image_size=96 {dtype}", ("max |encode_region - encode_images|", d), ("elements with other bits", nbits))
    assert nbits == 0 and crops == [] and np.array_equal(out.coords, coords)


# ---- 6. invariance ------------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_bands_residence_or_lanes(engines, monkeypatch):
    """the 15-kept grid (overlapping tiles: bands share rows) on an engine of max_batch 4: four batches per call"""
    from plip_amd.engine import Engine
    from plip_amd.plip import PLIP
    model, cfg, *_ = engines(CASE, "f32", 4)
    plip, eng = PLIP(model=model), model.engine
    origin, t, s = (0, 0), 64, 40
    region = synthetic_region()
    kw = dict(tile_px=t, stride=s, origin=origin)
    used = []
    inner = Engine.encode_image_u8
    monkeypatch.setattr(Engine, "encode_image_u8", lambda self, x, normalize=False: (
        used.append((id(self), torch.cuda.current_stream(self.device).cuda_stream, int(x.shape[0]))), inner(self, x, normalize))[1])
    import plip_amd.region_routes as routes
    gathers, selects = [], []
    inner_gather, inner_select = routes.region_gather, routes.region_select
    here = lambda e: (id(e), torch.cuda.current_stream(e.device).cuda_stream)
    monkeypatch.setattr(routes, "region_gather", lambda e, *a, **k: (gathers.append(here(e) + (int(a[3]),)), inner_gather(e, *a, **k))[1])
    monkeypatch.setattr(routes, "region_select", lambda e, *a, **k: (selects.append(here(e)), inner_select(e, *a, **k))[1])
    assert eng.use_lanes
    whole = plip.encode_region(region, **kw)
    calls = list(used)
    assert [c[2] for c in calls] == [4, 4, 4, 3] and len({c[:2] for c in calls}) == 2, calls       # batches of max_batch, on two lanes
    assert gathers == calls                 # every gather inside its lane's call: the engine and the stream of the encode that reads it
    assert selects == [(id(eng), torch.cuda.current_stream(eng.device).cuda_stream)]      # one select per band, on the caller's stream
    forms = {"band_rows=1": lambda: plip.encode_region(region, band_rows=1, **kw),
             "band_rows=3": lambda: plip.encode_region(region, band_rows=3, **kw),
             "device tensor": lambda: plip.encode_region(torch.from_numpy(region.copy()).to(eng.device), **kw),
             "device tensor, band_rows=2": lambda: plip.encode_region(torch.from_numpy(region.copy()).to(eng.device), band_rows=2, **kw),
             "device view": lambda: plip.encode_region(_strided_view(eng), **kw)}
    try:
        eng.use_lanes = False
        del used[:]
        forms_off = plip.encode_region(region, **kw)
        assert len({c[:2] for c in used}) == 1
    finally:
        eng.use_lanes = True
    results = {"lanes off": forms_off}
    results.update({name: fn() for name, fn in forms.items()})
    _, kept, coords = oracle_selection(origin, t, s)
    assert len(kept) == 15 and np.array_equal(whole.kept, kept)
    for name, out in results.items():
        d, nbits = _float_diff(out.embeddings, whole.embeddings)
        _report(f"invariance, {name}", ("max |difference|", d), ("elements with other bits", nbits))
        assert nbits == 0 and np.array_equal(out.kept, kept) and np.array_equal(out.coords, coords), name
        assert out.grid == whole.grid and np.array_equal(out.tissue, whole.tissue), name


# ---- 7. empty results ---------------------------------------------------------------------------------------------------------------
def test_empty_grid_and_all_background_give_no_rows(plips, engine):
    from plip_amd.engine_region import region_gather, region_select
    plip, cfg = plips["f32"]
    glass = (240 + np.random.RandomState(5).randint(-3, 4, size=(150, 210, 3))).astype(np.uint8)
    for region in (glass, torch.from_numpy(glass).to(engine.device)):
        out = plip.encode_region(region)
        assert out.embeddings.shape == (0, cfg.projection_dim) and out.embeddings.dtype == np.float32
        assert out.grid == (2, 3) and out.kept.shape == (0,) and out.coords.shape == (0, 2) and not out.tissue.any()
        out = plip.encode_region(region, tile_px=211)
        assert out.embeddings.shape == (0, cfg.projection_dim) and out.grid == (0, 0) and out.tissue.shape == (0, 0)
    # the entries themselves: an empty grid writes n_kept = 0 and launches nothing; no tiles asked for, none returned
    small = torch.from_numpy(glass[:40]).to(engine.device)
    counts, kept, n_kept = region_select(engine, small, 64)
    assert counts.shape == (0, 3) and kept.numel() == 0 and int(n_kept.item()) == 0
    assert region_gather(engine, small, kept, 0, 0, 64).shape == (0, 64, 64, 3)


# ---- 8. bad arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch(engine, region_dev, plips):
    from plip_amd import _lib
    from plip_amd._lib import PlipmiError, _ptr
    from plip_amd.engine_region import region_gather, region_select
    H, W = REGION_HW
    lib, h, st = engine.lib, engine._h, engine._stream()
    out = torch.full((64,), -7, dtype=torch.int32, device=engine.device)      # counts | kept | n_kept: must stay as they are
    counts, kept, n_kept = out[:16], out[16:32], out[32:33]
    dst = torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=engine.device)

    def select(H=H, W=W, pitch=3 * W, y0=0, x0=0, t=64, s=64, rows=1, cols=1, sat=18, lo=25, hi=235, mc=1, region=region_dev):
        return lib.plipmi_region_select(h, _ptr(region), H, W, pitch, y0, x0, t, s, rows, cols, sat, lo, hi, mc, _ptr(counts), _ptr(kept),
                                        _ptr(n_kept), st)

    def gather(H=H, W=W, pitch=3 * W, y0=0, x0=0, t=64, s=64, cols=1, first=0, B=1, region=region_dev, kept=kept):
        return lib.plipmi_region_gather(h, _ptr(region), H, W, pitch, y0, x0, t, s, cols, _ptr(kept), first, B, _ptr(dst), st)

    assert select() == 0 and gather() == 0              # the arguments the bad ones below differ from by one thing each
    torch.cuda.synchronize(engine.device)
    out.fill_(-7)
    dst.zero_()
    for what, call, msg in (
            ("window below the region", lambda: select(rows=4, cols=1), "outside the 200 x 331 region"),
            ("window right of the region", lambda: select(rows=1, cols=6), "outside the 200 x 331 region"),
            ("origin pushes the window out", lambda: select(y0=137, rows=1), "outside the 200 x 331 region"),
            ("pitch < 3W", lambda: select(pitch=3 * W - 1), "pitch_bytes 992"),
            ("threshold 256", lambda: select(sat=256), "0 .. 255"), ("threshold 256", lambda: select(hi=256), "0 .. 255"),
            ("threshold -1", lambda: select(lo=-1), "0 .. 255"), ("negative min_count", lambda: select(mc=-1), "min_count"),
            ("stride 0", lambda: select(s=0), "stride"), ("negative origin", lambda: select(x0=-1), "origin"), ("null region", lambda: select(region=None), "null region"),
            ("4 GiB", lambda: select(H=70000, pitch=70000), "4 GiB"), ("null handle", lambda: lib.plipmi_region_select(
                None, _ptr(region_dev), H, W, 3 * W, 0, 0, 64, 64, 1, 1, 18, 25, 235, 1, _ptr(counts), _ptr(kept), _ptr(n_kept), st), "null handle"),
            ("gather: columns outside", lambda: gather(cols=6), "outside the 200 x 331 region"),
            ("gather: tile taller than the region", lambda: gather(t=201, s=201), "empty grid"),
            ("gather: pitch < 3W", lambda: gather(pitch=3 * W - 1), "pitch_bytes 992"),
            ("gather: past the list", lambda: gather(cols=5, first=10, B=6), "kept[10 .. 16)"),
            ("gather: negative first", lambda: gather(first=-1), "first -1"), ("gather: null kept", lambda: gather(kept=None), "null kept/dst")):
        rc = call()
        assert rc == 1 and msg in _lib.last_error(), (what, rc, _lib.last_error())
    torch.cuda.synchronize(engine.device)
    assert bool((out == -7).all()) and not dst.any()      # nothing was launched
    # the Python layer: what it refuses itself, and what it passes on
    with pytest.raises(ValueError, match="uint8"):
        region_select(engine, region_dev.float(), 64)
    with pytest.raises(ValueError, match="strides"):
        region_select(engine, region_dev.permute(1, 0, 2), 64)
    with pytest.raises(PlipmiError, match="pitch_bytes"):
        region_select(engine, torch.as_strided(region_dev, (H, W, 3), (3 * W - 3, 3, 1)), 64)
    with pytest.raises(PlipmiError, match="0 .. 255"):
        region_select(engine, region_dev, 64, luma_max=256)
    with pytest.raises(ValueError, match="kept"):
        region_gather(engine, region_dev, kept.long(), 0, 1, 64)
    with pytest.raises(ValueError, match="kept"):
        region_gather(engine, region_dev, kept, 10, 7, 64)
    plip, _ = plips["f32"]
    for bad, match in ((dict(region=region_dev.float()), "uint8"), (dict(sat_min=256), "sat_min"), (dict(origin=(0, -2)), "origin"),
                       (dict(region=torch.as_strided(region_dev, (H, W, 3), (3 * W - 3, 3, 1))), "pitch_bytes")):
        args = dict(region=region_dev)
        args.update(bad)
        with pytest.raises((ValueError, PlipmiError), match=match):
            plip.encode_region(**args)


# ---- 9. the 224 px route: ends in the uint8 patch-gather GEMM ---------------------------------------------------------------------------
def test_vitb32_region_equals_encode_images_on_its_crops(engines):
    from plip_amd.plip import PLIP
    model, cfg, *_ = engines("vitb32_b4", "bf16")
    assert cfg.image_size == 224 and cfg.patch_size == 32
    rs = np.random.RandomState(9)
    region = (240 + rs.randint(-3, 4, size=(500, 700, 3))).astype(np.uint8)
    region[100:420, 150:560] = rs.randint(0, 256, size=(320, 410, 3), dtype=np.uint8)
    counts = region_tile_counts(region, 224, 224)
    kept = np.flatnonzero(counts.reshape(-1) >= region_min_count(0.5, 224))
    assert counts.shape == (2, 3) and 0 < len(kept) < 6
    coords = np.stack([(kept // 3) * 224, (kept % 3) * 224], axis=1)
    plip = PLIP(model=model)
    want = plip.encode_images(host_crops(region, coords, 224), batch_size=4)
    for name, r in (("host", region), ("device", torch.from_numpy(region).to(model.engine.device))):
        out = plip.encode_region(r)
        d, nbits = _float_diff(out.embeddings, want)
        _report(f"vitb32_b4 bf16 224 px, {name} region, kept {kept.tolist()} of 6", ("max |encode_region - encode_images|", d),
                ("elements with other bits", nbits))
        assert nbits == 0 and np.array_equal(out.kept, kept) and np.array_equal(out.coords, coords) and out.grid == (2, 3)
        assert np.array_equal(out.tissue, counts.astype(np.float32) / np.float32(224 * 224))
