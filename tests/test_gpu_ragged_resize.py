"""The ragged resize on the GPU (plipmi_resize_crop_u8_ragged, csrc/resize_ragged.hip): the device-built coefficient tables against
``resample_coeffs`` integer for integer, the tiles against Pillow bit for bit, and the routes that use it end to end.

Measured on an MI355X (profiles/ragged_resize_parity.txt): every table and every tile below differs from its reference by 0; the
end-to-end embeddings differ from the host-Pillow route's by 7.2e-7 (PLIP, also at image_size=96) and 7.5e-8 (CLIPEmbedder), under the
2e-5 bar."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (65, 64), (64, 65), (67, 64), (63, 63), (40, 100), (100, 40), (96, 96), (71, 64), (129, 200), (300, 77), (20, 20),
         (64, 200), (257, 301), (33, 500)]
SIZES_224 = [(224, 224), (256, 256), (225, 224), (300, 500), (150, 170), (1000, 700)]


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


@pytest.mark.parametrize("size,out", [(64, 64), (65, 64), (20, 64), (63, 97), (500, 969), (301, 64), (4096, 64), (1000, 224)])
def test_table_kernel_equals_resample_coeffs(size, out):
    """Bounds and 22-bit coefficients computed on the device (float64, no fused multiply-add) == the host's Pillow tables, on the full
    axis and on a cropped window, also with a row width above the axis's own (a batch's ksize is its largest)."""
    from plip_amd.kernel_entries import resize_ragged_tables
    from plip_amd.preprocess import resample_coeffs
    bounds, kk = resample_coeffs(size, out)
    ks = kk.shape[1]
    for first, count, width in ((0, out, ks), (out // 3, min(out - out // 3, 37), ks + 4)):
        b, k = resize_ragged_tables(size, out, first, count, width)
        b, k = b.cpu().numpy(), k.cpu().numpy()
        print(f"table {size}->{out} rows {first}..{first + count} ks {width}: max |bounds diff| "
              f"{np.abs(b - bounds[first:first + count]).max()}, max |coef diff| {np.abs(k[:, :ks] - kk[first:first + count]).max()}")
        np.testing.assert_array_equal(b, bounds[first:first + count])
        np.testing.assert_array_equal(k[:, :ks], kk[first:first + count])
        assert not k[:, ks:].any()


@pytest.mark.parametrize("n,sizes", [(None, SIZES), (224, SIZES_224)])
def test_ragged_batch_is_pillow_exact(engines, n, sizes):
    model, cfg, *_ = engines("tiny_b6", "f32")
    images = [_image(h, w) for h, w in sizes]
    for rule in ("torchvision", "hf"):
        got = model.engine.resize_crop_ragged(images, crop=rule, n_px=n).cpu().numpy()
        px = cfg.image_size if n is None else n
        assert got.shape == (len(sizes), px, px, 3) and got.dtype == np.uint8
        want = np.stack([_pillow(im, px, rule) for im in images])
        print(f"ragged n={px} {rule}: max |tile - Pillow| {np.abs(got.astype(int) - want.astype(int)).max()}")
        for i in range(len(sizes)):
            np.testing.assert_array_equal(got[i], want[i], err_msg=f"{sizes[i]} {rule}")


def test_ragged_equals_uniform(engines):
    model, cfg, *_ = engines("tiny_b6", "f32")
    imgs = np.stack([_image(96, 130, s) for s in range(5)])
    for rule in ("torchvision", "hf"):
        a = model.engine.resize_crop_ragged(list(imgs), crop=rule).cpu().numpy()
        b = model.engine.resize_crop_u8(torch.from_numpy(imgs), crop=rule).cpu().numpy()
        np.testing.assert_array_equal(a, b)


def test_edge_batches(engines):
    from plip_amd._lib import PlipmiError
    from plip_amd.engine import ragged_blob
    model, cfg, *_ = engines("tiny_b6", "f32")
    eng, n = model.engine, cfg.image_size
    one = _image(129, 200)
    np.testing.assert_array_equal(eng.resize_crop_ragged([one], crop="hf").cpu().numpy()[0], _pillow(one, n, "hf"))
    empty = eng.resize_crop_ragged([])
    assert tuple(empty.shape) == (0, n, n, 3) and empty.dtype == torch.uint8 and empty.is_cuda
    native = [_image(n, n, s) for s in range(3)]
    np.testing.assert_array_equal(eng.resize_crop_ragged(native).cpu().numpy(), np.stack(native))     # identity tables: the bytes themselves
    # PIL inputs of other modes are converted to RGB when they are packed
    from PIL import Image
    grey = Image.fromarray(_image(40, 100)[..., 0])
    np.testing.assert_array_equal(eng.resize_crop_ragged([grey, one])[0].cpu().numpy(), _pillow(np.asarray(grey.convert("RGB")), n, "torchvision"))
    # a ratio above 64 (520 -> 8) and an offset past the buffer are refused before any launch; the handle stays good
    big = _image(8 * 65, 8 * 65)
    with pytest.raises(PlipmiError, match=r"code 1\).*ratio"):
        eng.resize_crop_ragged([one, big], n_px=8)
    blob, offsets, hw = ragged_blob([one, native[0]])
    bad = offsets.copy()
    bad[1] += 1
    with pytest.raises(PlipmiError, match=r"code 1\).*src_bytes"):
        eng.resize_crop_ragged((blob, bad, hw))
    with pytest.raises(PlipmiError, match=r"code 1\)"):
        eng.resize_crop_ragged((blob, offsets, np.asarray([[129, 200], [0, 64]], np.int32)))
    np.testing.assert_array_equal(eng.resize_crop_ragged([big, one], n_px=16).cpu().numpy()[1], _pillow(one, 16, "torchvision"))
    np.testing.assert_array_equal(eng.resize_crop_ragged((blob, offsets, hw), crop="hf").cpu().numpy()[0], _pillow(one, n, "hf"))


def test_ragged_entry_in_a_captured_graph(engines):
    """The entry only enqueues: it can be captured into a graph and replayed on new pixels of the same sizes."""
    model, cfg, *_ = engines("tiny_b6", "f32")
    from plip_amd.engine import ragged_blob
    eng, n = model.engine, cfg.image_size
    imgs = [_image(h, w) for h, w in SIZES[5:10]]
    blob, offsets, hw = ragged_blob(imgs)
    dev = blob.to(eng.device)
    eng.resize_crop_ragged((dev, offsets, hw))                       # the workspace exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng.resize_crop_ragged((dev, offsets, hw), crop="hf")
    other = [_image(h, w, 7) for h, w in SIZES[5:10]]
    dev.copy_(ragged_blob(other)[0])
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack([_pillow(im, n, "hf") for im in other]))


def test_end_to_end_plip_and_embedder(engines):
    from PIL import Image
    from plip_amd.plip import PLIP
    from plip_amd.preprocess import preprocess_images
    from plip_amd.reproducibility import CLIPEmbedder
    model, cfg, *_ = engines("tiny_b6", "f32")
    eng, n = model.engine, cfg.image_size
    imgs = [_image(*SIZES[i % len(SIZES)], seed=i) for i in range(13)]
    imgs[3], imgs[9] = Image.fromarray(imgs[3]), Image.fromarray(imgs[9])
    plip = PLIP(model=model, ragged_resize=True)
    assert PLIP(model=model).ragged_resize is False
    a = plip.encode_images(imgs, batch_size=4)
    ref = eng.encode_image(torch.from_numpy(preprocess_images(imgs, n, crop="hf"))).cpu().numpy()     # host Pillow path, PLIP's (HF) rule
    print(f"PLIP ragged vs host route: max |diff| {np.abs(a - ref).max():.3e}")
    assert np.abs(a - ref).max() < 2e-5
    alone = np.concatenate([plip.encode_images([im], batch_size=1) for im in imgs])
    np.testing.assert_array_equal(a, alone)
    np.testing.assert_array_equal(a, plip.encode_images(imgs, batch_size=4, num_workers=3))
    many = imgs * 3                                                   # 39 > max_batch = 32: the second lane runs
    assert len(many) > eng.max_batch and eng.use_lanes
    on = plip.encode_images(many, batch_size=4)
    on_piped = plip.encode_images(many, batch_size=4, num_workers=3)
    eng.use_lanes = False
    try:
        off = plip.encode_images(many, batch_size=4)
        off_piped = plip.encode_images(many, batch_size=4, num_workers=3)
    finally:
        del eng.use_lanes
    np.testing.assert_array_equal(on, off)
    np.testing.assert_array_equal(on_piped, off_piped)
    np.testing.assert_array_equal(on, on_piped)
    np.testing.assert_array_equal(on[:13], a)
    # encode_images(image_size=): the same route on the derived engine, direct and pipelined
    at = plip.encode_images(imgs, batch_size=4, image_size=96)
    host_at = PLIP(model=model).encode_images(imgs, batch_size=4, image_size=96)
    print(f"PLIP ragged vs host route at image_size=96: max |diff| {np.abs(at - host_at).max():.3e}")
    assert np.abs(at - host_at).max() < 2e-5
    np.testing.assert_array_equal(at, plip.encode_images(imgs, batch_size=4, image_size=96, num_workers=3))
    # the embedder: torchvision's crop rule, unit rows, against its default (host preprocess) route
    emb = CLIPEmbedder(model, ragged_resize=True)
    e = emb.embed_images(imgs, batch_size=4)
    d = CLIPEmbedder(model).embed_images(imgs, batch_size=4)
    print(f"CLIPEmbedder ragged vs default route: max |diff| {np.abs(e - d).max():.3e}")
    assert np.abs(e - d).max() < 2e-5
    np.testing.assert_array_equal(e, np.concatenate([emb.embed_images([im], batch_size=1) for im in imgs]))
    np.testing.assert_array_equal(e, emb.embed_images(imgs, batch_size=4, num_workers=3))
    em = emb.embed_images(many, batch_size=4)
    eng.use_lanes = False
    try:
        np.testing.assert_array_equal(em, emb.embed_images(many, batch_size=4))
        np.testing.assert_array_equal(em, emb.embed_images(many, batch_size=4, num_workers=3))
    finally:
        del eng.use_lanes
    np.testing.assert_array_equal(em[:13], e)
