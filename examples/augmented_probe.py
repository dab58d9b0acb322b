"""Augmented views on the GPU: ``PLIP.encode_views`` for test-time augmentation and for a probe trained on K views per tile.

    python examples/augmented_probe.py

Two uses, neither needs a backward pass:

* D4 test-time augmentation: a tile has no canonical orientation, so its embedding is averaged over the eight symmetries of the square
  (``transform="d4"``, ``reduce="mean"``); the cosine between a tile and its views is the invariance report.
* A ``SoftmaxProber`` fitted on K views per tile of the reference's train transform (``transform="train"``: random crop, flip, affine,
  perspective, Pillow's bytes) and tested on the D4-averaged embeddings of held-out tiles.

The tiles are synthetic (two "classes": stripes of two orientations over stain-coloured noise) and so are the weights; a real caller
passes their tiles and a real checkpoint (``PLIP("path/to/plip")``).  The train transform crops n_px windows: tiles of another size
than the one to crop from are resized first, by the resize route ``encode_images`` already has (``Engine.resize_crop_u8``)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_tiles(n, side, seed):
    """uint8 [n, side, side, 3] and labels [n]: class 0 has stripes along x, class 1 along the diagonal"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:side, :side]
    tiles, labels = [], rs.randint(0, 2, n)
    for lab in labels:
        period = rs.uniform(14, 22)
        phase = (yy if lab == 0 else (yy + xx) * 0.7071) / period + rs.uniform(0, 1)
        stripes = (np.sin(2 * np.pi * phase) > 0)[..., None]
        stain = np.stack([rs.randint(150, 240, (side, side)), rs.randint(60, 170, (side, side)), rs.randint(130, 220, (side, side))], axis=-1)
        tiles.append(np.where(stripes, stain, 235 + rs.randint(-4, 5, (side, side, 3))).astype(np.uint8))
    return np.stack(tiles), labels


def main():
    from plip_amd import weights as W
    from plip_amd.config import get_config
    from plip_amd.model import PlipModel
    from plip_amd.plip import PLIP
    from plip_amd.reproducibility.softmax_probe import SoftmaxProber
    cfg = get_config("ViT-B/32")
    plip = PLIP(model=PlipModel(cfg, W.synthetic_state_dict(cfg, 0), dtype="bf16", max_batch=256))
    n_px = cfg.image_size

    # 1. D4 test-time augmentation and the invariance report
    test_tiles, test_y = synthetic_tiles(64, n_px, seed=1)
    views = plip.encode_views(test_tiles, batch_size=32)                                    # [64, 8, P]: view 0 is the tile itself
    unit = views / np.linalg.norm(views, axis=-1, keepdims=True)
    cos = (unit[:, :1] * unit).sum(axis=-1)                                                 # cosine of every view with its tile
    print(f"D4 views {views.shape}; cosine(tile, view k), mean over {len(test_tiles)} tiles: " + " ".join(f"{c:.3f}" for c in cos.mean(axis=0)))
    test_x = plip.encode_views(test_tiles, batch_size=32, reduce="mean")                     # [64, P]: the D4-averaged embedding
    print(f"D4-averaged embeddings {test_x.shape}, unit norm: {np.allclose(np.linalg.norm(test_x, axis=-1), 1.0, atol=1e-5)}")

    # 2. a probe on K train views per tile (tiles of 320 px: the crops are n_px windows of them)
    K = 4
    train_tiles, train_y = synthetic_tiles(96, 320, seed=2)
    train_views, params = plip.encode_views(train_tiles, batch_size=32, views=K, transform="train", seed=0, return_params=True)
    flips = int(params[0][..., 4].sum())
    warped = int((params[2] != np.asarray([1.0, 0, 0, 0, 1, 0, 0, 0])).any(axis=-1).sum())
    print(f"train views {train_views.shape}: {flips} of {train_views.shape[0] * K} flipped, {warped} with a perspective")
    train_x = train_views.reshape(-1, train_views.shape[-1])
    train_x = train_x / np.linalg.norm(train_x, axis=-1, keepdims=True)
    # (C far above the CLIP protocol's 0.316: the synthetic towers spread these tiles over a tiny part of the unit sphere)
    classifier, (test_metrics, train_metrics) = SoftmaxProber(C=1000.0, engine=plip.model.engine).train_and_test(
        train_x.astype(np.float32), np.repeat(train_y, K), test_x, test_y)
    print("probe on the views, tested on D4-averaged held-out tiles:",
          {k: round(float(v), 3) for k, v in test_metrics.items() if isinstance(v, (int, float, np.floating))})


if __name__ == "__main__":
    main()
