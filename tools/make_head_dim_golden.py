"""Generate tests/golden/head_dim_*.npz: HF ``CLIPModel`` with attention heads that are not 64 wide -- TEST INFRASTRUCTURE.

    python tools/make_head_dim_golden.py [case ...]        # needs ``transformers``; CPU, no GPU

Every case is ``PRESETS["tiny"]`` with other tower shapes (``CASES`` below), weights ``synthetic_state_dict(cfg, 0)``, pixels
``synthetic_pixels(cfg, B, 1)`` and ids ``synthetic_ids(cfg, B, 2)`` -- seeds only, a test regenerates them (``case_inputs``).  A file
holds HF's outputs (``image_features`` ... ``logits_per_image``), hidden states as listed per case -- "all": every depth and token,
"rows": the CLS / last-token (vision) or BOS / first-token (text) rows of every depth --, the weight / pixel fingerprints and ids / mask.

* ``head_dim_hd80``        vision 640 wide, 8 heads of 80, 17 tokens; also ``res96/image_features``: HF with
                           ``interpolate_pos_encoding=True`` on 96 x 96 pixels (37 tokens; ``RES_SEED``, ``RES_B`` images)
* ``head_dim_hd88_p4``     vision 1408 wide, 16 heads of 88, 4-pixel patches: 257 tokens, three key chunks; 88 is no multiple of 16
* ``head_dim_text80``      both towers 640 wide with 8 heads of 80: the text tower runs causal with a padding mask
* ``head_dim_hd128``       vision 256 wide, 2 heads of 128: the padded size 128 with no padding
* ``head_dim_hd80_twin64`` the hd80 WEIGHTS AND INPUTS (the head count changes no tensor's shape) run as 10 heads of 64: what an engine
                           on the head-64 kernels is measured against; ``head_dim_hd80`` also stores the distance of its fields from this
                           run (``gap64/<field>``) -- what a loader that guesses ``heads = width // 64`` gets wrong
* ``head_dim_vith14_b2``   ``PRESETS["ViT-H/14"]`` with GELU towers at full size, B = 2, embeddings and logits only (for tools/head_dim_report.py, not
                           for the suite; about 4 GB of weights: made on request only)
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED, PIXEL_SEED, IDS_SEED = 0, 1, 2
# case -> (base preset, config changes, batch, vision hidden states, text hidden states)
CASES = {
    "hd80": ("tiny", dict(v_width=640, v_heads=8, v_mlp=1280), 3, "all", "all"),
    "hd88_p4": ("tiny", dict(v_width=1408, v_heads=16, v_mlp=2816, patch_size=4), 2, "rows", None),
    "text80": ("tiny", dict(v_width=640, v_heads=8, v_mlp=1280, t_width=640, t_heads=8, t_mlp=1280), 3, "rows", "all"),
    "hd128": ("tiny", dict(v_width=256, v_heads=2, v_mlp=512), 3, "all", None),
    "hd80_twin64": ("tiny", dict(v_width=640, v_heads=10, v_mlp=1280), 3, "all", None),
    "vith14_b2": ("ViT-H/14", dict(v_hidden_act="gelu", t_hidden_act="gelu"), 2, None, None),      # the published checkpoints' activation
}
DEFAULT = [c for c in CASES if c != "vith14_b2"]
RES_HW, RES_B, RES_SEED = (96, 96), 3, 301      # the at_resolution field of hd80: 6 x 6 + 1 = 37 vision tokens on 16-pixel patches
F32_EMB_BAR = 1e-5     # tests/test_gpu_parity.py TOL["f32"]["emb"]


def case_config(name):
    from plip_amd.config import get_config
    base, changes, *_ = CASES[name]
    cfg = get_config(base).replace(**changes)
    cfg.validate()
    return cfg


def case_inputs(name):
    """-> (cfg, state dict, pixels, ids, mask) of a case: what the maker ran HF on and what a test builds its engine from"""
    from plip_amd import weights as W
    cfg = case_config(name)
    B = CASES[name][2]
    ids, mask = W.synthetic_ids(cfg, B, IDS_SEED)
    return cfg, W.synthetic_state_dict(cfg, WEIGHT_SEED), W.synthetic_pixels(cfg, B, PIXEL_SEED), ids, mask


def hf_model(cfg, sd):
    """``oracle.hf_reference.build_model`` with the towers' ``hidden_act`` of the config"""
    import torch
    from transformers import CLIPModel

    from oracle import hf_reference as H
    hc = H.hf_config(cfg, "sdpa")
    hc.vision_config.hidden_act, hc.text_config.hidden_act = cfg.v_hidden_act, cfg.t_hidden_act
    model = CLIPModel(hc)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(np.array(v, dtype=np.float32, copy=True)) for k, v in sd.items()},
                                                strict=False)
    bad = [k for k in missing if "position_ids" not in k] + list(unexpected)
    if bad:
        raise RuntimeError(f"state dict does not fit CLIPModel: {bad[:6]}")
    heads = {m.num_heads for m in model.vision_model.modules() if hasattr(m, "num_heads")}
    assert heads == {cfg.v_heads}, (heads, cfg.v_heads)
    return model.eval()


def res_pixels():
    return np.random.RandomState(RES_SEED).standard_normal((RES_B, 3) + RES_HW).astype(np.float32)


def outputs(cfg, sd, px, ids, mask, v_hidden, t_hidden, res=False):
    import torch

    from oracle import hf_reference as H
    model = hf_model(cfg, sd)
    out = H.run(model, px, ids, mask, output_hidden_states=bool(v_hidden or t_hidden))
    if res:
        with torch.no_grad():
            out["res96/image_features"] = H._tensor(model.get_image_features(
                pixel_values=torch.from_numpy(res_pixels()), interpolate_pos_encoding=True)).float().numpy()
    res = {k: out[k] for k in ("image_features", "text_features", "image_embeds", "text_embeds", "logits_per_image", "res96/image_features")
           if k in out}
    if v_hidden == "all":
        res["vision_hidden"] = np.stack(out["vision_hidden"])
    elif v_hidden == "rows":
        res["vision_hidden_cls"] = np.stack([h[:, 0, :] for h in out["vision_hidden"]])
        res["vision_hidden_last_token"] = np.stack([h[:, -1, :] for h in out["vision_hidden"]])
    if t_hidden == "all":
        res["text_hidden"] = np.stack(out["text_hidden"])
    return res


def main(only=None) -> None:
    from oracle.make_golden import fingerprint
    for name in only or DEFAULT:
        _, _, B, v_hidden, t_hidden = CASES[name]
        cfg, sd, px, ids, mask = case_inputs(name)
        res = outputs(cfg, sd, px, ids, mask, v_hidden, t_hidden, res=name == "hd80")
        save = dict(res)
        if name == "hd80":
            # the same tensors as 10 heads of 64: how far HF itself moves
            wrong = outputs(case_config("hd80_twin64"), sd, px, ids, mask, None, None)
            for k in ("image_features", "image_embeds", "logits_per_image"):
                div = np.exp(np.float64(sd["logit_scale"])) if k == "logits_per_image" else 1.0
                save[f"gap64/{k}"] = np.float64(np.abs(res[k].astype(np.float64) - wrong[k]).max() / div)
            d = float(save["gap64/image_embeds"])
            print(f"  hd80 run as 10 x 64 instead of 8 x 80: image_embeds move by {d:.3e} = {d / F32_EMB_BAR:.0f} x the fp32 bar")
            assert d > 100 * F32_EMB_BAR, d
        save["weights_fingerprint"] = fingerprint(sd) if name != "vith14_b2" else np.zeros((0, 2))
        save["pixels_fingerprint"] = np.array([px.astype(np.float64).sum(), (px.astype(np.float64) ** 2).sum()])
        save["ids"], save["mask"] = ids, mask
        path = os.path.join(GOLDEN_DIR, f"head_dim_{name}.npz")
        np.savez_compressed(path, **save)
        heads = f"vision {cfg.v_width} = {cfg.v_heads} x {cfg.head_dim}, text {cfg.t_width} = {cfg.t_heads} x {cfg.t_head_dim}"
        print(f"head_dim_{name}: {heads}, {cfg.v_tokens} vision tokens, B = {B}; wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")
        assert os.path.getsize(path) < 1024 * 1024, "a committed file stays below 1 MiB"


if __name__ == "__main__":
    main(sys.argv[1:] or None)
