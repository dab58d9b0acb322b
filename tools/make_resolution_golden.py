"""Generate tests/golden/vitb32_b4_resolutions.npz: HF ``CLIPModel`` at other image sizes -- TEST INFRASTRUCTURE.

    python tools/make_resolution_golden.py          # needs ``transformers``; CPU, no GPU

Weights and captions are those of the ``vitb32_b4`` golden case (``oracle.make_golden.case_inputs``); the pixels of each
size are ``np.random.RandomState(seed).standard_normal((4, 3, H, W))`` in fp32 (what ``weights.synthetic_pixels`` draws),
so a test regenerates them from the recorded seed and shape without this script or ``transformers``.  For every size the
file holds HF's ``image_features`` (get_image_features), ``image_embeds`` and ``logits_per_image`` (forward), all with
``interpolate_pos_encoding=True`` (modeling_clip.py CLIPVisionEmbeddings.interpolate_pos_encoding), under the keys
``<name>/<field>``, plus ``<name>/seed`` and ``<name>/shape``.  No pixels are stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "vitb32_b4_resolutions.npz")
CASE = "vitb32_b4"
# name -> (height, width, pixel seed): what each size exercises on a ViT-B/32 (32-pixel patches, native 7 x 7 grid)
SIZES = {
    "448x448": (448, 448, 101),   # upscale to 14 x 14: 197 tokens, the streamed MFMA attention
    "288x256": (288, 256, 102),   # non-square 9 x 8: 73 tokens, the fused q/k/v + attention kernel (non-causal)
    "250x250": (250, 250, 103),   # not a multiple of the patch: floors to 7 x 7 on a square image -- HF keeps its table
    "230x224": (230, 224, 104),   # same 7 x 7 grid but height != width: HF interpolates 7 -> 7 (an exact copy)
    "160x160": (160, 160, 105),   # downscale to 5 x 5
}
BATCH = 4


def pixels(seed: int, height: int, width: int) -> np.ndarray:
    return np.random.RandomState(seed).standard_normal((BATCH, 3, height, width)).astype(np.float32)


def main() -> None:
    import torch

    from oracle import hf_reference as H
    from oracle.make_golden import case_inputs
    cfg, sd, _, ids, mask = case_inputs(CASE)
    model = H.build_model(cfg, sd, "sdpa")
    save = {}
    with torch.no_grad():
        ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
        for name, (h, w, seed) in SIZES.items():
            tp = torch.from_numpy(pixels(seed, h, w))
            feats = H._tensor(model.get_image_features(pixel_values=tp, interpolate_pos_encoding=True))
            out = model(input_ids=ti, pixel_values=tp, attention_mask=tm, interpolate_pos_encoding=True)
            save[f"{name}/image_features"] = feats.float().numpy()
            save[f"{name}/image_embeds"] = out.image_embeds.float().numpy()
            save[f"{name}/logits_per_image"] = out.logits_per_image.float().numpy()
            save[f"{name}/seed"] = np.int64(seed)
            save[f"{name}/shape"] = np.asarray([BATCH, 3, h, w], np.int64)
    np.savez_compressed(OUT, **save)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KB, {len(SIZES)} sizes)")


if __name__ == "__main__":
    main()
