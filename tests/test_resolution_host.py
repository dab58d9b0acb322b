"""CPU side of the other-resolution feature (Engine.at_resolution): the committed HF fixture and the FLOP count per grid."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resolution_fixture_matches_live_hf():
    """tests/golden/vitb32_b4_resolutions.npz is what HF CLIPModel (interpolate_pos_encoding=True) computes on the inputs the
    GPU test regenerates from the recorded seeds and shapes."""
    pytest.importorskip("transformers")
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_resolution_golden as M
    from oracle import hf_reference as H
    from oracle.make_golden import case_inputs
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "vitb32_b4_resolutions.npz")))
    cfg, sd, _, ids, mask = case_inputs(M.CASE)
    model = H.build_model(cfg, sd, "sdpa")
    assert sorted({k.split("/")[0] for k in g}) == sorted(M.SIZES)
    with torch.no_grad():
        for name, (h, w, seed) in M.SIZES.items():
            assert int(g[f"{name}/seed"]) == seed and tuple(g[f"{name}/shape"]) == (M.BATCH, 3, h, w)
            px = np.random.RandomState(seed).standard_normal((M.BATCH, 3, h, w)).astype(np.float32)
            tp = torch.from_numpy(px)
            feats = H._tensor(model.get_image_features(pixel_values=tp, interpolate_pos_encoding=True)).numpy()
            out = model(input_ids=torch.from_numpy(ids), pixel_values=tp, attention_mask=torch.from_numpy(mask),
                        interpolate_pos_encoding=True)
            np.testing.assert_allclose(feats, g[f"{name}/image_features"], rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(out.image_embeds.numpy(), g[f"{name}/image_embeds"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(out.logits_per_image.numpy(), g[f"{name}/logits_per_image"], rtol=1e-5, atol=1e-4)
    # the sizes differ in what HF does with the table: the 250 px and 230 x 224 rows share the native grid with different pixels
    assert g["448x448/image_embeds"].shape == (M.BATCH, cfg.projection_dim)


def test_image_flops_at():
    from plip_amd.config import get_config
    c = get_config("ViT-B/32")
    assert c.image_flops_at(224, 224) == c.image_flops()
    assert abs(c.image_flops() - 8.8176e9) < 1e5
    # shape-level count at 448 x 448: 14 x 14 patches + CLS = 197 tokens
    n, S, D, F, K = 196, 197, 768, 3072, 3 * 32 * 32
    block = 2 * S * D * 3 * D + 2 * S * D * D + 2 * 2 * S * D * F + 2 * 2 * S * S * D
    want = 2 * n * K * D + 12 * block + 2 * D * 512
    assert c.image_flops_at(448, 448) == pytest.approx(want, rel=1e-12)
    assert c.image_flops_at(448, 448) == pytest.approx(35.8e9, rel=2e-3)
    # pixels past the grid do not count (HF's strided conv floors): 250 x 250 is the native 7 x 7 grid
    assert c.image_flops_at(250, 250) == c.image_flops()
    assert c.image_flops_at(288, 256) == pytest.approx(c.image_flops_at(256, 288))
