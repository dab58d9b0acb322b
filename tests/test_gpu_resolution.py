"""Images at other resolutions (include/plipmi.h plipmi_clone_resolution, Engine.at_resolution, HF's
``interpolate_pos_encoding=True``): the position-table resampler against torch, the derived handle against HF CLIPModel
(tests/golden/vitb32_b4_resolutions.npz, tools/make_resolution_golden.py), and the kernel paths a derived handle takes."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.make_golden import case_inputs
from plip_amd import _lib
from plip_amd import weights as W

pytestmark = pytest.mark.gpu

# the bars of tests/test_gpu_parity.py (f32: fp32 round-off; bf16: the north-star 1e-3 on cosines, 6e-4 on embeddings; f16: its row)
TOL = {
    "f32": dict(feat=2e-4, cos=1e-5, emb=1e-5),
    "bf16": dict(feat=6e-2, cos=1e-3, emb=6e-4),
    "f16": dict(feat=1.5e-2, cos=2.5e-4, emb=4e-4),
}
SIZES = ["448x448", "288x256", "250x250", "230x224", "160x160"]


def _fixture_pixels(g, name):
    b, c, h, w = (int(v) for v in g[f"{name}/shape"])
    return np.random.RandomState(int(g[f"{name}/seed"])).standard_normal((b, c, h, w)).astype(np.float32)


def _kernels(eng, fn):
    rows = []
    with eng.profile(rows):
        fn()
    torch.cuda.synchronize()
    return " ".join(r["name"] for r in rows)


def test_resampler_matches_torch_bicubic():
    """plipmi_resample_pos against torch.nn.functional.interpolate(bicubic, align_corners=False) in fp64 on the CPU, ViT-B/32's table
    to up-, down-, non-square and same-size grids; 7 -> 7 is an exact copy, the CLS row always is."""
    from plip_amd.kernel_entries import resample_pos
    _, sd, *_ = case_inputs("vitb32_b4")
    tab = np.asarray(sd["vision_model.embeddings.position_embedding.weight"], np.float32)      # [50, 768]
    n0, D = 7, tab.shape[1]
    dev = torch.from_numpy(tab).cuda()
    bound = 1e-6 * np.abs(tab).max()
    for gh, gw in ((14, 14), (9, 8), (5, 5), (7, 7), (32, 32)):
        got = resample_pos(dev, gh, gw).cpu().numpy()
        patch = torch.from_numpy(tab[1:].astype(np.float64)).reshape(1, n0, n0, D).permute(0, 3, 1, 2)
        ref = torch.nn.functional.interpolate(patch, size=(gh, gw), mode="bicubic", align_corners=False)
        ref = ref.permute(0, 2, 3, 1).reshape(gh * gw, D).numpy()
        assert got.shape == (1 + gh * gw, D)
        np.testing.assert_array_equal(got[0], tab[0])
        err = np.abs(got[1:] - ref).max()
        assert err <= bound, ((gh, gw), err, bound)
        if (gh, gw) == (7, 7):
            np.testing.assert_array_equal(got, tab)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_parity_against_hf_interpolate_pos_encoding(dtype, engines, golden):
    """get_image_features / forward with interpolate_pos_encoding=True against HF CLIPModel at five sizes: upscale (197 tokens, the
    streamed attention), non-square (73 tokens, the fused q/k/v + attention kernel on the 16-bit engines), a size that floors to the
    native grid (HF keeps its table), the native grid on a non-square image (HF interpolates 7 -> 7) and a downscale."""
    g = golden("vitb32_b4_resolutions")
    model, cfg, sd, _, ids, mask = engines("vitb32_b4", dtype)
    t = TOL[dtype]
    scale = np.exp(np.float64(sd["logit_scale"]))
    for name in SIZES:
        px = torch.from_numpy(_fixture_pixels(g, name))
        feats = model.get_image_features(pixel_values=px, interpolate_pos_encoding=True).cpu().numpy()
        out = model(input_ids=torch.from_numpy(ids), pixel_values=px, attention_mask=torch.from_numpy(mask), interpolate_pos_encoding=True)
        e_feat = np.abs(feats - g[f"{name}/image_features"]).max()
        e_emb = np.abs(out.image_embeds.cpu().numpy() - g[f"{name}/image_embeds"]).max()
        e_cos = np.abs(out.logits_per_image.cpu().numpy() - g[f"{name}/logits_per_image"]).max() / scale
        print(f"{dtype} {name}: features {e_feat:.2e}, image_embeds {e_emb:.2e}, cosine {e_cos:.2e}")
        assert e_feat < t["feat"] and e_emb < t["emb"] and e_cos < t["cos"], (dtype, name, e_feat, e_emb, e_cos)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_derived_handle_at_native_size_is_bit_identical(dtype, engines):
    model, cfg, *_ = engines("vitb32_b4", dtype)
    eng = model.engine
    d = eng.at_resolution(224, 224)
    assert d is not eng and d.image_hw == (224, 224)
    px = torch.from_numpy(W.synthetic_pixels(cfg, 12, 5))
    tiles = torch.from_numpy(W.synthetic_tiles(cfg, 12, 6))
    assert torch.equal(eng.encode_image(px), d.encode_image(px))
    assert torch.equal(eng.encode_image_u8(tiles), d.encode_image_u8(tiles))


@pytest.mark.parametrize("hw", [(448, 448), (288, 256)])
def test_patch_gather_matches_unfold_at_other_sizes(hw, engines):
    """At the batches where the patch GEMM gathers its operand itself (the ring tile: 64 images at 448 x 448, 175 at 288 x 256 on 256
    CUs), the H x W gather gives the bits of the unfold pass + plain patch GEMM, from uint8 tiles and from fp32 pixels; uint8 tiles
    agree with the same tiles normalised on the host within the bf16 bar."""
    from plip_amd import kernel_entries  # noqa: F401  (binds the test header)
    from plip_amd.preprocess import CLIP_MEAN, CLIP_STD
    model, cfg, *_ = engines("vitb32_b4", "bf16", 256)
    h, w = hw
    d = model.engine.at_resolution(h, w)
    B = d.max_batch
    assert B == 256 * 50 // (1 + (h // 32) * (w // 32))
    rs = np.random.RandomState(7)
    tiles = torch.from_numpy(rs.randint(0, 256, size=(B, h, w, 3), dtype=np.uint8)).cuda()
    x = tiles.float().cpu().numpy() / np.float32(255.0)
    px = torch.from_numpy(np.ascontiguousarray(((x - np.asarray(CLIP_MEAN, np.float32)) / np.asarray(CLIP_STD, np.float32))
                                               .transpose(0, 3, 1, 2))).cuda()
    lib = _lib.load()
    try:
        k_u8 = _kernels(d, lambda: d.encode_image_u8(tiles))
        k_px = _kernels(d, lambda: d.encode_image(px))
        assert "patch_gather_u8" in k_u8 and "patch_gather>" in k_px, (k_u8, k_px)
        g_u8, g_px = d.encode_image_u8(tiles), d.encode_image(px)
        _lib.check(lib.plipmi_test_patch_gather(0), "plipmi_test_patch_gather")
        k_u8 = _kernels(d, lambda: d.encode_image_u8(tiles))
        assert "unfold_patches_u8" in k_u8 and "patch_gather" not in k_u8, k_u8
        u_u8, u_px = d.encode_image_u8(tiles), d.encode_image(px)
    finally:
        lib.plipmi_test_reset_hooks()
    assert torch.equal(g_u8, u_u8)
    assert torch.equal(g_px, u_px)
    a = torch.nn.functional.normalize(g_u8, dim=-1).cpu().numpy()
    b = torch.nn.functional.normalize(g_px, dim=-1).cpu().numpy()
    assert np.abs(a - b).max() < TOL["bf16"]["emb"]


def test_fused_qkv_attention_matches_two_kernels_in_the_vision_tower(engines):
    """288 x 256 on ViT-B/32: 73 vision tokens, inside the fused q/k/v + attention kernel's 65 .. 80 -- its first non-causal use.
    Fused (hook 2) and the q/k/v GEMM + attention kernel (hook 0) give the same bits."""
    from plip_amd import kernel_entries  # noqa: F401
    model, cfg, *_ = engines("vitb32_b4", "bf16")
    d = model.engine.at_resolution(288, 256)
    assert d.v_tokens == 73
    px = torch.from_numpy(np.random.RandomState(8).standard_normal((d.max_batch, 3, 288, 256)).astype(np.float32))
    lib = _lib.load()
    try:
        _lib.check(lib.plipmi_test_fused_qkv_attention(2), "plipmi_test_fused_qkv_attention")
        names = _kernels(d, lambda: d.encode_image(px))
        assert "qkv_attention" in names, names
        fused = d.encode_image(px)
        _lib.check(lib.plipmi_test_fused_qkv_attention(0), "plipmi_test_fused_qkv_attention")
        names = _kernels(d, lambda: d.encode_image(px))
        assert "qkv_attention" not in names and "attention_mfma" in names, names
        two = d.encode_image(px)
    finally:
        lib.plipmi_test_reset_hooks()
    assert torch.equal(fused, two)


def test_row_does_not_depend_on_its_batch(engines):
    model, cfg, *_ = engines("vitb32_b4", "bf16")
    eng = model.engine
    d = eng.at_resolution(448, 448)
    mb = d.max_batch
    assert mb == 32 * 50 // 197
    n = 2 * mb + 3
    px = torch.from_numpy(np.random.RandomState(9).standard_normal((n, 3, 448, 448)).astype(np.float32)).cuda()
    torch.cuda.synchronize()                    # inputs fully written before any call
    many_lanes = d.encode_image(px)             # > max_batch rows: chunks alternate between d and a clone of it (lanes)
    d.use_lanes = False
    try:
        many = d.encode_image(px)
    finally:
        d.use_lanes = True
    full = d.encode_image(px[:mb])
    one = d.encode_image(px[:1])
    assert torch.equal(many_lanes, many)
    assert torch.equal(many[:mb], full)
    assert torch.equal(many[:1], one)
    assert torch.equal(many[mb:2 * mb], d.encode_image(px[mb:2 * mb]))


def test_handle_lifetime_lru_and_errors():
    from plip_amd.model import PlipModel
    from plip_amd.config import get_config
    cfg = get_config("ViT-B/32")
    model = PlipModel(cfg, W.synthetic_state_dict(cfg, 0), dtype="bf16", max_batch=8)
    eng = model.engine
    lib = _lib.load()
    px448 = torch.from_numpy(W.synthetic_pixels(cfg.replace(image_size=448), 3, 11)).cuda()
    px160 = torch.from_numpy(W.synthetic_pixels(cfg.replace(image_size=160), 3, 12)).cuda()
    try:
        # two resolutions alive together, each keeps its own table and workspace
        a, b = eng.at_resolution(448, 448), eng.at_resolution(160, 160)
        ea, eb = a.encode_image(px448), b.encode_image(px160)
        assert torch.equal(a.encode_image(px448), ea) and torch.equal(b.encode_image(px160), eb)
        assert eng.at_resolution(448, 448) is a
        # the source destroyed before a derived handle (C ABI): the shared weights and its own table live on
        h = C.c_void_p()
        _lib.check(lib.plipmi_clone_resolution(eng._h, 448, 448, 4, C.byref(h)), "plipmi_clone_resolution")
        h2 = C.c_void_p()
        _lib.check(lib.plipmi_clone(h, C.byref(h2)), "plipmi_clone")      # a clone keeps the size and the table
        # LRU: a fifth size closes the least recently used
        eng.at_resolution(448, 448)
        for s in (192, 256, 320):
            eng.at_resolution(s, s)
        assert not b._h.value and a._h.value and len(eng._resolutions) == 4
        assert a.max_batch == 8 * 50 // 197        # the derived workspace: about the source's vision rows
        rc = lib.plipmi_clone_resolution(eng._h, 16, 224, 0, C.byref(C.c_void_p()))
        assert rc == 1 and "patch" in _lib.last_error(), _lib.last_error()
        with pytest.raises(ValueError):
            model.get_image_features(pixel_values=px448, interpolate_pos_encoding=False)
        with pytest.raises(ValueError):
            model(input_ids=torch.zeros((3, cfg.context_length), dtype=torch.int64), pixel_values=px448)
        model.engine.close()
        assert not a._h.value                    # derived engines close with their parent
        for hh in (h, h2):
            out = torch.empty((3, cfg.projection_dim), dtype=torch.float32, device="cuda")
            _lib.check(lib.plipmi_encode_image(hh, C.c_void_p(px448.data_ptr()), 3, C.c_void_p(out.data_ptr()), 0,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), "plipmi_encode_image")
            torch.cuda.synchronize()
            assert torch.equal(out, ea)
        lib.plipmi_destroy(h)
        lib.plipmi_destroy(h2)
    finally:
        model.engine.close()
    # ViT-L/14@336 at 448 px: a 32 x 32 grid of 14-pixel patches is 1025 tokens
    big = get_config("ViT-L/14@336px")
    m = PlipModel(big, W.synthetic_state_dict(big, 0), dtype="bf16", max_batch=1)
    try:
        rc = lib.plipmi_clone_resolution(m.engine._h, 448, 448, 0, C.byref(C.c_void_p()))
        assert rc == 1 and "1025 tokens" in _lib.last_error(), _lib.last_error()
        with pytest.raises(_lib.PlipmiError, match="1024"):
            m.engine.at_resolution(448, 448)
    finally:
        m.engine.close()


def test_plip_encode_images_at_image_size(engines):
    """PLIP.encode_images(image_size=448) on 600 x 500 uint8 images: the GPU resize + crop to 448 and the derived engine, direct and
    through the worker pipeline (identical), against host Pillow preprocessing + the derived engine (within the bf16 bar)."""
    from plip_amd.plip import PLIP, _CROP
    from plip_amd.preprocess import preprocess_images
    model, cfg, *_ = engines("vitb32_b4", "bf16")
    rs = np.random.RandomState(10)
    base = rs.randint(0, 256, size=(4, 4, 3)).astype(np.float32)
    imgs = [np.clip(np.kron(base + rs.randint(-40, 40, size=(4, 4, 3)), np.ones((125, 150, 1))) +
                    rs.randint(-20, 20, size=(500, 600, 3)), 0, 255).astype(np.uint8) for _ in range(13)]
    p = PLIP(model=model)
    direct = p.encode_images(imgs, batch_size=4, image_size=448)
    workers = p.encode_images(imgs, batch_size=4, num_workers=2, image_size=448)
    assert direct.shape == (13, cfg.projection_dim)
    np.testing.assert_array_equal(direct, workers)
    d = model.engine.at_resolution(448, 448)
    ref = d.encode_image(torch.from_numpy(preprocess_images(imgs, n_px=448, crop=_CROP))).cpu().numpy()
    nrm = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    assert np.abs(nrm(direct) - nrm(ref)).max() < TOL["bf16"]["emb"]
