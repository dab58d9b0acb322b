"""Embed the tissue of a slide region: ``PLIP.encode_region`` on a synthetic region.

    python examples/embed_region.py

The region is uint8 RGB, thousands of pixels per side and mostly glass.  The grid, the background filter and the stacking of the kept
tiles run on the GPU; what comes back is one embedding per kept tile with its place in the region.  A real caller passes the array
their slide reader gives them (numpy, ``np.memmap`` or a PIL image: uploaded in bands; or a tensor already on the device) and a real
checkpoint (``PLIP("path/to/plip")``); weights here are synthetic.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_region(side=4096, seed=0):
    """glass (bright, grey) with three stained blobs (random pink-to-purple pixels)"""
    rs = np.random.RandomState(seed)
    region = (240 + rs.randint(-3, 4, size=(side, side, 3))).astype(np.uint8)
    yy, xx = np.mgrid[:side, :side]
    for cy, cx, r in ((900, 1200, 700), (2600, 2900, 1000), (3300, 800, 500)):
        blob = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        stain = np.stack([rs.randint(150, 240, blob.sum()), rs.randint(60, 170, blob.sum()), rs.randint(130, 220, blob.sum())], axis=1)
        region[blob] = stain.astype(np.uint8)
    return region


def main():
    from plip_amd import weights as W
    from plip_amd.config import get_config
    from plip_amd.model import PlipModel
    from plip_amd.plip import PLIP
    cfg = get_config("ViT-B/32")
    plip = PLIP(model=PlipModel(cfg, W.synthetic_state_dict(cfg, 0), dtype="bf16", max_batch=256))
    region = synthetic_region()
    out = plip.encode_region(region)                                   # 224 px tiles, side by side, kept at >= 50 % tissue
    rows, cols = out.grid
    print(f"region {region.shape[0]} x {region.shape[1]}: grid {rows} x {cols}, {len(out.kept)} tiles kept, embeddings {out.embeddings.shape}")
    print("tissue fraction per tile (rows of the grid):")
    for row in out.tissue:
        print("  " + " ".join(f"{int(round(9 * v))}" for v in row))
    print("first kept tiles (y, x):", out.coords[:4].tolist())
    # half-overlapping 448 px tiles, resized on the GPU to the model's 224 px exactly as encode_images resizes such crops
    big = plip.encode_region(region, tile_px=448, stride=224, min_tissue=0.75)
    print(f"448 px tiles every 224 px, >= 75 % tissue: grid {big.grid}, {len(big.kept)} kept")
    # stain-normalised: ONE Macenko fit over a subsample of the region (every step-th pixel of every step-th row, taken on the host
    # before the upload), then every gathered batch normalised to the reference stains on the GPU before it is encoded
    fit = plip.fit_stain(region)
    row = fit.numpy()[0]
    print(f"stain fit on every {fit.step}th pixel: {int(row[14])} tissue pixels, valid {bool(row[15])}, maxC {row[12]:.3f} {row[13]:.3f}")
    normed = plip.encode_region(region, stain=fit)
    cos = (normed.embeddings * out.embeddings).sum(axis=1) / (np.linalg.norm(normed.embeddings, axis=1) * np.linalg.norm(out.embeddings, axis=1))
    print(f"with stain=: the same {len(normed.kept)} tiles, cosine to the raw tiles' embeddings {cos.min():.3f} .. {cos.max():.3f}")


if __name__ == "__main__":
    main()
