"""The "mosaic" of a slide region: ``PLIP.region_mosaic`` on a synthetic region.

    python examples/region_mosaic.py

``encode_region`` finds and embeds the tissue tiles; spherical k-means on the GPU then groups the L2-normalised embeddings and keeps ONE
representative tile per cluster -- the handful of tiles a slide-retrieval system indexes instead of the thousands it was cut into.
``PLIP.cluster_embeddings`` does the same on any cached embeddings (a corpus to curate or de-duplicate, a codebook).  A real caller
passes their slide reader's array and a real checkpoint (``PLIP("path/to/plip")``); weights here are synthetic.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from embed_region import synthetic_region  # noqa: E402


def main():
    from plip_amd import weights as W
    from plip_amd.config import get_config
    from plip_amd.model import PlipModel
    from plip_amd.plip import PLIP
    cfg = get_config("ViT-B/32")
    plip = PLIP(model=PlipModel(cfg, W.synthetic_state_dict(cfg, 0), dtype="bf16", max_batch=256))
    region = synthetic_region()
    mosaic = plip.region_mosaic(region, 9)                              # 224 px tiles, kept at >= 50 % tissue, nine clusters
    reg, res = mosaic.region, mosaic.result
    print(f"region {region.shape[0]} x {region.shape[1]}: {len(reg.kept)} tissue tiles of a {reg.grid[0]} x {reg.grid[1]} grid -> "
          f"{len(mosaic.counts)} clusters in {res.n_iter} iterations (converged: {res.converged}, inertia {res.inertia:.4f})")
    for k, (n, (y, x), flat) in enumerate(zip(mosaic.counts.tolist(), mosaic.rep_coords.tolist(), mosaic.rep_kept.tolist())):
        print(f"  cluster {k}: {n:3d} tiles, representative at (y, x) = ({y}, {x}), grid tile {flat}")
    # where each cluster lies on the grid ('.' = background)
    rows, cols = reg.grid
    grid = np.full(rows * cols, -1)
    grid[reg.kept] = mosaic.labels
    for row in grid.reshape(rows, cols):
        print("  " + " ".join("." if v < 0 else str(v) for v in row))
    # the same clustering of embeddings already at hand, Euclidean this time, best of three k-means++ restarts
    res = plip.cluster_embeddings(reg.embeddings, 4, metric="euclidean", n_init=3)
    print(f"cluster_embeddings (euclidean, K = 4, n_init = 3): counts {res.counts.tolist()}, inertia {res.inertia:.3f}")


if __name__ == "__main__":
    main()
