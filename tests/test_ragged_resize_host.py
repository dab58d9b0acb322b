"""Host side of the ragged resize (plipmi_resize_crop_u8_ragged): packing, sizing, the CPU oracle against Pillow, and the routing
of ``PLIP`` / ``CLIPEmbedder`` with ``ragged_resize=True`` over a recording stand-in engine.  No GPU."""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers as Hh  # noqa: E402

# (h, w): native size, one pixel of odd crop excess on each axis (where the two crop rules differ), upscaling, one axis already
# right, both aspect extremes, a scale above 4
SIZES = [(64, 64), (65, 64), (64, 65), (67, 64), (63, 63), (40, 100), (100, 40), (96, 96), (71, 64), (129, 200), (300, 77), (20, 20),
         (64, 200), (257, 301), (33, 500)]
N = 64


def _image(h, w, seed=0):
    return np.random.RandomState(1000 * h + w + seed).randint(0, 256, (h, w, 3), dtype=np.uint8)


def _pillow(img, n, rule):
    from PIL import Image
    from plip_amd.preprocess import crop_offset, resize_output_size
    h, w = img.shape[:2]
    nh, nw = resize_output_size(h, w, n)
    im = Image.fromarray(img).resize((nw, nh), resample=Image.BICUBIC)
    left, top = crop_offset(nw, n, rule), crop_offset(nh, n, rule)
    return np.asarray(im.crop((left, top, left + n, top + n)))


def test_pack_ragged_offsets_and_sizes():
    from PIL import Image
    from plip_amd.engine import ragged_blob, ragged_blob_bytes
    from plip_amd.preprocess import pack_ragged
    rs = np.random.RandomState(3)
    rgb = _image(5, 7)
    grey = rs.randint(0, 256, (4, 6), dtype=np.uint8)
    rgba = Image.fromarray(rs.randint(0, 256, (3, 9, 4), dtype=np.uint8), "RGBA")
    pil = Image.fromarray(_image(8, 2))
    images = [rgb, grey, rgba, pil]
    buf, offsets, hw = pack_ragged(images)
    assert buf.dtype == np.uint8 and offsets.dtype == np.int64 and hw.dtype == np.int32
    np.testing.assert_array_equal(hw, [[5, 7], [4, 6], [3, 9], [8, 2]])
    sizes = [5 * 7 * 3, 4 * 6 * 3, 3 * 9 * 3, 8 * 2 * 3]
    np.testing.assert_array_equal(offsets, np.cumsum([0] + sizes[:-1]))
    assert buf.shape == (sum(sizes),)
    want = [rgb, np.asarray(Image.fromarray(grey).convert("RGB")), np.asarray(rgba.convert("RGB")), np.asarray(pil)]
    for o, s, a in zip(offsets, sizes, want):
        np.testing.assert_array_equal(buf[o:o + s], a.reshape(-1))
    assert (want[1][..., 0] == grey).all()                      # grey -> three equal channels
    # into a caller's buffer (the pinned staging rows): the leading slice of it, nothing past it touched
    out = np.full(sum(sizes) + 5, 77, np.uint8)
    buf2, _, _ = pack_ragged(images, out=out)
    assert np.shares_memory(buf2, out) and np.array_equal(buf2, buf) and (out[-5:] == 77).all()
    with pytest.raises(ValueError):
        pack_ragged(images, out=np.zeros(10, np.uint8))
    with pytest.raises(TypeError):
        pack_ragged([np.zeros((4, 4, 3), np.float32)])
    empty = pack_ragged([])
    assert empty[0].shape == (0,) and empty[1].shape == (0,) and empty[2].shape == (0, 2)
    # the one-copy form: descriptors in front of the pixels
    blob, o2, hw2 = ragged_blob(images)
    assert blob.dtype == torch.uint8 and blob.numel() == ragged_blob_bytes(images) == 16 * 4 + sum(sizes)
    raw = blob.numpy()
    np.testing.assert_array_equal(raw[:32].view(np.int64), offsets)
    np.testing.assert_array_equal(raw[32:64].view(np.int32).reshape(4, 2), hw)
    np.testing.assert_array_equal(raw[64:], buf)
    np.testing.assert_array_equal(o2, offsets)
    np.testing.assert_array_equal(hw2, hw)


@pytest.mark.parametrize("n", [64, 224])
def test_ragged_ksize_is_the_row_width_of_resample_coeffs(n):
    from plip_amd.preprocess import ragged_ksize, resample_coeffs, resize_output_size
    widths = []
    for h, w in SIZES:
        nh, nw = resize_output_size(h, w, n)
        per_axis = [resample_coeffs(h, nh)[1].shape[1], resample_coeffs(w, nw)[1].shape[1]]
        assert ragged_ksize(np.asarray([[h, w]]), n) == max(per_axis), (h, w)
        widths += per_axis
    assert ragged_ksize(np.asarray(SIZES), n) == max(widths)
    if n == 64:
        assert max(widths) == 19
    assert ragged_ksize(np.zeros((0, 2), np.int32), n) == 5


@pytest.mark.parametrize("rule", ["torchvision", "hf"])
def test_ragged_reference_is_pillow(rule):
    from PIL import Image
    from plip_amd.preprocess import resize_crop_ragged_reference
    images = [_image(h, w) for h, w in SIZES]
    got = resize_crop_ragged_reference(images, N, rule)
    assert got.shape == (len(SIZES), N, N, 3) and got.dtype == np.uint8
    for i, im in enumerate(images):
        np.testing.assert_array_equal(got[i], _pillow(im, N, rule), err_msg=str(SIZES[i]))
    # PIL inputs of other modes are converted first, as the datasets of the reference do
    grey = Image.fromarray(_image(40, 100)[..., 0])
    np.testing.assert_array_equal(resize_crop_ragged_reference([grey], N, rule)[0],
                                  _pillow(np.asarray(grey.convert("RGB")), N, rule))


@pytest.mark.parametrize("n", [32, 64, 224])
def test_scale_one_table_is_a_single_tap(n):
    """An axis that already has the right size needs no special case in the kernels: its table is one tap of 2^22 at the centre, and
    (p * 2^22 + 2^21) >> 22 == p for every byte."""
    from plip_amd.preprocess import resample_coeffs
    bounds, kk = resample_coeffs(n, n)
    np.testing.assert_array_equal(bounds[:, 1] > 0, True)
    for x in range(n):
        taps = kk[x, :bounds[x, 1]]
        nz = np.nonzero(taps)[0]
        assert len(nz) == 1 and taps[nz[0]] == 1 << 22 and bounds[x, 0] + nz[0] == x
    p = np.arange(256, dtype=np.int64)
    np.testing.assert_array_equal((p * (1 << 22) + (1 << 21)) >> 22, p)


def test_ragged_supported_limit():
    from plip_amd.preprocess import ragged_supported
    assert ragged_supported(64 * 64, 64 * 64, 64) and ragged_supported(64, 100000, 64)      # the ratio is taken per axis, in / out
    assert not ragged_supported(64 * 64 + 1, 64 * 64 + 1, 64)
    assert ragged_supported(8 * 64, 8 * 64, 8) and not ragged_supported(8 * 65, 8 * 65, 8)
    assert not ragged_supported(0, 5, 64)


# ---- routing over a recording stand-in ---------------------------------------------------------------------------------------------
class RecordingEngine(Hh.OracleEngine):
    """The oracle-backed stand-in plus the ragged entry (the CPU oracle of it) and the lane loop the embedder uses."""
    use_lanes = False

    def resize_crop_ragged(self, images, crop="torchvision", n_px=None):
        from plip_amd.preprocess import resize_crop_ragged_reference
        n = self.cfg.image_size if n_px is None else n_px
        if isinstance(images, tuple):            # the packed form of the pipelined path: (blob, offsets, hw)
            blob, offsets, hw = images
            raw = blob.numpy()[16 * len(hw):]
            images = [raw[o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(offsets.tolist(), hw.tolist())]
        self.calls.append(("resize_crop_ragged", tuple(tuple(int(v) for v in np.asarray(im).shape[:2]) if isinstance(im, np.ndarray)
                                                       else (im.size[1], im.size[0]) for im in images), crop))
        return torch.from_numpy(resize_crop_ragged_reference(list(images), n, crop))

    @contextlib.contextmanager
    def lane_loop(self):
        yield lambda fn: fn(self)

    def at_resolution(self, height, width):      # encode_images(image_size=N): the stand-in serves its own size only
        assert (height, width) == (self.cfg.image_size, self.cfg.image_size)
        return self


@pytest.fixture(scope="module")
def tiny():
    from oracle.make_golden import case_inputs
    cfg, sd, *_ = case_inputs("tiny_b6")
    assert cfg.image_size == N
    return cfg, sd


def _plip(tiny, ragged):
    from plip_amd.model import PlipModel
    from plip_amd.plip import PLIP
    cfg, sd = tiny
    m = object.__new__(PlipModel)
    m.config, m.engine, m.device, m.dtype, m.training = cfg, RecordingEngine(cfg, sd, 8), torch.device("cpu"), torch.float32, False
    ours = object.__new__(PLIP)                  # the constructor insists on a GPU; the host loops do not need one
    ours.device, ours.model_name, ours.model, ours.tokenizer = "cpu", "local", m, None
    ours.model_hash, ours.image_vectors = hash, None
    if ragged is not None:
        ours.ragged_resize = ragged
    return ours, m.engine


def _calls(engine):
    """the recorded calls without the inner encode_image of the stand-in's u8 route (it logs one per encode_image_u8)"""
    out, skip = [], False
    for c in engine.calls:
        if skip and c[0] == "encode_image":
            skip = False
            continue
        skip = c[0] == "encode_image_u8"
        out.append(c)
    return out


def _encode_both_ways(ours, eng, seq, batch_size):
    """``encode_images(seq)`` at the checkpoint's resolution and with ``image_size=`` that very size: ONE loop serves both, so the
    stand-in records the same calls (shapes and crop rules included) and the arrays are equal.  -> the embeddings, the calls"""
    eng.calls.clear()
    at = ours.encode_images(seq, batch_size=batch_size, image_size=N)
    calls_at = list(eng.calls)
    eng.calls.clear()
    got = ours.encode_images(seq, batch_size=batch_size)
    assert eng.calls == calls_at and len(calls_at) > 0
    np.testing.assert_array_equal(got, at)
    return got, _calls(eng)


def test_plip_routing_with_ragged_resize(tiny):
    from plip_amd.preprocess import preprocess_images
    cfg, sd = tiny
    ours, eng = _plip(tiny, True)
    mixed = [_image(h, w) for h, w in SIZES[:12]]
    # chunks of 4 of differing sizes: coalesced into ragged calls of up to max_batch = 8 images, in order
    got, calls = _encode_both_ways(ours, eng, mixed, 4)
    assert [c[0] for c in calls] == ["resize_crop_ragged", "encode_image_u8"] * 2
    assert calls[0][1] == tuple(SIZES[:8]) and calls[2][1] == tuple(SIZES[8:12]) and calls[0][2] == calls[2][2] == "hf"
    host, heng = _plip(tiny, False)
    want = host.encode_images(mixed, batch_size=4)
    assert {c[0] for c in heng.calls} == {"encode_image"}            # the parent's route for such lists: host Pillow
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
    # a chunk entirely at n x n takes the tiles route, a chunk of one size keeps resize_crop_u8, the rest is ragged; order kept
    tiles = [_image(N, N, s) for s in range(4)]
    same = [_image(96, 130, s) for s in range(4)]
    seq = tiles + mixed[4:8] + same + mixed[8:12]
    got, calls = _encode_both_ways(ours, eng, seq, 4)
    # (every resize is enqueued in the flush that encodes its rows: the pending ragged images leave when the one-size chunk arrives,
    # and that chunk is resized when IT is flushed, directly in front of its own encode)
    assert [c[0] for c in calls] == ["encode_image_u8", "resize_crop_ragged", "encode_image_u8", "resize_crop_u8", "encode_image_u8",
                                     "resize_crop_ragged", "encode_image_u8"]
    want = host.encode_images(seq, batch_size=4)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
    # an image over the ratio limit and a float image keep the host path, one by one, and the order is kept
    big = np.random.RandomState(5).randint(0, 256, (N * 64 + 6, N * 64 + 1, 3), dtype=np.uint8)
    flt = _image(50, 70)[..., 0].astype(np.float32)          # (a 2-D float array is Pillow's mode F: the host path takes it)
    seq = [mixed[1], big, mixed[2], mixed[3], flt]
    got, calls = _encode_both_ways(ours, eng, seq, 5)
    assert [c[0] for c in calls] == ["resize_crop_ragged", "encode_image_u8", "encode_image", "resize_crop_ragged", "encode_image_u8",
                                     "encode_image"]
    assert calls[0][1] == (SIZES[1],) and calls[3][1] == (SIZES[2], SIZES[3]) and calls[2][1][0] == 1 and calls[5][1][0] == 1
    want = np.concatenate([host.encode_images([im], batch_size=1) for im in seq[:4]])
    np.testing.assert_allclose(got[:4], want, rtol=0, atol=2e-6)
    px = torch.from_numpy(preprocess_images([seq[1]], N, crop="hf"))
    np.testing.assert_allclose(got[1:2], heng.encode_image(px).numpy(), rtol=0, atol=2e-6)
    # the pipelined loop routes the same way (workers decode and convert, the batch is packed with its descriptors)
    eng.calls.clear()
    piped = ours.encode_images(mixed, batch_size=4, num_workers=3)
    calls = _calls(eng)
    assert [c[0] for c in calls] == ["resize_crop_ragged", "encode_image_u8"] * 3
    assert [c[1] for c in calls[::2]] == [tuple(SIZES[i:i + 4]) for i in range(0, 12, 4)]
    np.testing.assert_allclose(piped, host.encode_images(mixed, batch_size=4), rtol=0, atol=2e-6)
    eng.calls.clear()
    piped = ours.encode_images([mixed[1], big, mixed[2]], batch_size=3, num_workers=2)
    assert [c[0] for c in _calls(eng)] == ["resize_crop_ragged", "encode_image_u8", "encode_image"]
    np.testing.assert_allclose(piped, got[:3], rtol=0, atol=2e-6)


def test_default_routes_are_unchanged(tiny):
    """ragged_resize=False -- and a PLIP object that never heard of the keyword -- take the routes and return the arrays the host loops
    did before the ragged route existed: a list of differing sizes goes through host Pillow, and the stand-in of tests/helpers.py
    (which has no ragged entry, no lanes and no ``at_resolution``) keeps working.  What moved: the direct loop used to resize a
    one-size chunk when it ROUTED it, ahead of the pending batches; now, as the pipelined loop always did, the resize is enqueued in
    the flush that encodes its rows, so both loops record the same sequence."""
    from plip_amd.plip import PLIP
    cfg, sd = tiny
    seq = [_image(h, w) for h, w in SIZES[:4]] + [_image(N, N, s) for s in range(4)] + [_image(96, 130, s) for s in range(4)]
    # host pixels flushed when the native tiles arrive, the staged tiles when the one-size chunk arrives, then its resize and encode
    want_calls = [("encode_image", 4), ("encode_image_u8", 4), ("resize_crop_u8", 4), ("encode_image_u8", 4)]
    outs = []
    for attr in (False, None):
        model = Hh.oracle_model(cfg, sd)
        assert not hasattr(model.engine, "resize_crop_ragged")
        ours = object.__new__(PLIP)
        ours.device, ours.model_name, ours.model, ours.tokenizer = "cpu", "local", model, None
        ours.model_hash, ours.image_vectors = hash, None
        if attr is not None:
            ours.ragged_resize = attr
        a = ours.encode_images(seq, batch_size=4)
        assert [(c[0], c[1][0]) for c in _calls(model.engine)] == want_calls
        model.engine.calls.clear()
        b = ours.encode_images(seq, batch_size=4, num_workers=2)
        assert [(c[0], c[1][0]) for c in _calls(model.engine)] == want_calls
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-6)
        outs.append(a)
    np.testing.assert_array_equal(outs[0], outs[1])
    # image_size= runs the same loop: the same calls on an engine that has ``at_resolution``, and the same arrays
    ours, eng = _plip(tiny, False)
    got, calls = _encode_both_ways(ours, eng, seq, 4)
    assert [(c[0], c[1][0]) for c in calls] == want_calls
    np.testing.assert_array_equal(got, outs[0])
    # one-size chunks of two sizes share a flush: each size resized by itself inside it, the eight tiles encoded together
    other = [_image(80, 72, s) for s in range(4)]
    got, calls = _encode_both_ways(ours, eng, seq[8:] + other, 4)
    assert [c[:2] for c in calls] == [("resize_crop_u8", (4, 96, 130, 3)), ("resize_crop_u8", (4, 80, 72, 3)), ("encode_image_u8", (8, N, N, 3))]
    np.testing.assert_allclose(got, np.concatenate([outs[0][8:], ours.encode_images(other, batch_size=4)]), rtol=0, atol=2e-6)


def test_plip_class_default_is_off():
    import inspect
    from plip_amd.plip import PLIP
    from plip_amd.reproducibility import CLIPEmbedder
    assert inspect.signature(PLIP.__init__).parameters["ragged_resize"].default is False
    assert inspect.signature(CLIPEmbedder.__init__).parameters["ragged_resize"].default is False


def test_clip_embedder_routing_with_ragged_resize(tiny):
    from plip_amd.model import PlipModel
    from plip_amd.reproducibility import CLIPEmbedder
    cfg, sd = tiny

    def embedder(**kw):
        m = object.__new__(PlipModel)
        m.config, m.engine, m.device, m.dtype, m.training = cfg, RecordingEngine(cfg, sd, 8), torch.device("cpu"), torch.float32, False
        return CLIPEmbedder(m, **kw), m.engine

    mixed = [_image(h, w) for h, w in SIZES[:10]]
    tiles = [_image(N, N, s) for s in range(4)]
    same = [_image(96, 130, s) for s in range(4)]
    seq = mixed[:4] + tiles + same + mixed[4:10]
    emb, eng = embedder(ragged_resize=True)
    got = emb.embed_images(seq, batch_size=4)
    calls = _calls(eng)
    assert [c[0] for c in calls] == ["resize_crop_ragged", "encode_image_u8", "encode_image_u8", "resize_crop_u8", "encode_image_u8",
                                     "resize_crop_ragged", "encode_image_u8", "resize_crop_ragged", "encode_image_u8"]
    assert all(c[2] == "torchvision" for c in calls if c[0].startswith("resize"))        # _transform's crop rule
    ref, reng = embedder()
    want = ref.embed_images(seq, batch_size=4)
    assert {c[0] for c in reng.calls} == {"encode_image"}            # the default: every image through the host's preprocess
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
    eng.calls.clear()
    np.testing.assert_allclose(emb.embed_images(seq, batch_size=4, num_workers=3), want, rtol=0, atol=2e-6)
    assert [c[0] for c in _calls(eng)] == [c[0] for c in calls]
    # an over-limit image falls back alone; a caller's own preprocess switches the route off altogether
    big = np.random.RandomState(5).randint(0, 256, (N * 64 + 6, N * 64 + 1, 3), dtype=np.uint8)
    eng.calls.clear()
    got = emb.embed_images([mixed[1], big, mixed[2]], batch_size=4)
    assert [c[0] for c in _calls(eng)] == ["resize_crop_ragged", "encode_image_u8", "encode_image"]
    np.testing.assert_allclose(got, ref.embed_images([mixed[1], big, mixed[2]], batch_size=4), rtol=0, atol=2e-6)
    from plip_amd.preprocess import preprocess_image
    own, oeng = embedder(preprocess=lambda im: preprocess_image(im, N), ragged_resize=True)
    own.embed_images(mixed[:3], batch_size=4)
    assert {c[0] for c in oeng.calls} == {"encode_image"}
    assert emb.embed_images([], batch_size=4).shape == (0, cfg.projection_dim)
