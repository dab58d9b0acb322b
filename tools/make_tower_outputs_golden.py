"""Generate tests/golden/tower_outputs_*.npz: HF ``CLIPModel`` per-token tower outputs -- TEST INFRASTRUCTURE.

    python tools/make_tower_outputs_golden.py       # needs ``transformers``; CPU, no GPU

HF ``CLIPModel(attn_implementation="eager")`` on the weights and inputs of the existing golden cases
(``oracle.make_golden.case_inputs``): ``model.vision_model(pixel_values, output_attentions=True, output_hidden_states=True)`` and
``model.text_model(input_ids, attention_mask, ...)``.  Keys are ``<run>/<tower>_<field>``: ``last_hidden_state``, ``pooler_output``,
``hidden_states`` [n, B, S, D] and ``attentions`` [n, B, H, S, S] at the indices ``<run>/<tower>_hidden_idx`` /
``<run>/<tower>_attn_idx``.  Runs:

* tower_outputs_tiny.npz -- the ``tiny`` arch, every layer: ``eos_masked`` (tiny_b6: both towers, the captions with their attention
  mask: padded keys), and the text tower alone for ``eos_nomask`` (the same captions, no mask) and ``zero``
  (tiny_b5_zero_pad_ln100, zero padding, no mask, argmax pooling).
* tower_outputs_vitb32_b2_{vision,text}_{attn,hidden}.npz, tower_outputs_vitb32_b2_last.npz -- ViT-B/32, the first two samples of
  vitb32_b4 (captions with their mask), hidden states / attentions of layers {0, 5, 11}; split so that every file stays under 1 MiB.
* tower_outputs_vitb32_160.npz -- ViT-B/32 vision at 160 x 160 with ``interpolate_pos_encoding=True`` (a 5 x 5 grid, 26 tokens),
  pixels ``RandomState(SEED_160).standard_normal((2, 3, 160, 160))``; layers {0, 5, 11}.
No inputs are stored: the tests rebuild them from the case names and seeds.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")
LAYERS_B32 = (0, 5, 11)
SEED_160 = 160


def pixels_160() -> np.ndarray:
    return np.random.RandomState(SEED_160).standard_normal((2, 3, 160, 160)).astype(np.float32)


def _tower(model, tower, idx_h, idx_a, **kw):
    out = (model.vision_model if tower == "vision" else model.text_model)(output_attentions=True, output_hidden_states=True, **kw)
    hs = [h.float().numpy() for h in out.hidden_states]
    at = [a.float().numpy() for a in out.attentions]
    idx_h = range(len(hs)) if idx_h is None else idx_h
    idx_a = range(len(at)) if idx_a is None else idx_a
    return {f"{tower}_last_hidden_state": out.last_hidden_state.float().numpy(),
            f"{tower}_pooler_output": out.pooler_output.float().numpy(),
            f"{tower}_hidden_states": np.stack([hs[i] for i in idx_h]), f"{tower}_hidden_idx": np.asarray(list(idx_h), np.int64),
            f"{tower}_attentions": np.stack([at[i] for i in idx_a]), f"{tower}_attn_idx": np.asarray(list(idx_a), np.int64)}


def _save(name, d):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    assert size < 1 << 20, (name, size)
    print(f"wrote {path} ({size / 1024:.1f} KB)")


def main() -> None:
    import torch

    from oracle import hf_reference as H
    from oracle.make_golden import case_inputs
    with torch.no_grad():
        tiny = {}
        for run, case, use_mask in (("eos_masked", "tiny_b6", True), ("eos_nomask", "tiny_b6", False), ("zero", "tiny_b5_zero_pad_ln100", False)):
            cfg, sd, px, ids, mask = case_inputs(case)
            model = H.build_model(cfg, sd, "eager")
            d = _tower(model, "vision", None, None, pixel_values=torch.from_numpy(px)) if run == "eos_masked" else {}
            d.update(_tower(model, "text", None, None, input_ids=torch.from_numpy(ids),
                            attention_mask=torch.from_numpy(mask) if use_mask else None))
            tiny.update({f"{run}/{k}": v for k, v in d.items()})
        _save("tower_outputs_tiny", tiny)

        cfg, sd, px, ids, mask = case_inputs("vitb32_b4")
        model = H.build_model(cfg, sd, "eager")
        v = _tower(model, "vision", LAYERS_B32, LAYERS_B32, pixel_values=torch.from_numpy(px[:2]))
        t = _tower(model, "text", LAYERS_B32, LAYERS_B32, input_ids=torch.from_numpy(ids[:2]), attention_mask=torch.from_numpy(mask[:2]))
        for tower, d in (("vision", v), ("text", t)):
            _save(f"tower_outputs_vitb32_b2_{tower}_attn", {f"b2/{k}": d[k] for k in (f"{tower}_attentions", f"{tower}_attn_idx")})
            _save(f"tower_outputs_vitb32_b2_{tower}_hidden", {f"b2/{k}": d[k] for k in (f"{tower}_hidden_states", f"{tower}_hidden_idx")})
        _save("tower_outputs_vitb32_b2_last", {f"b2/{k}": d[k] for d in (v, t) for k in d
                                               if k.endswith(("last_hidden_state", "pooler_output"))})
        d = _tower(model, "vision", LAYERS_B32, LAYERS_B32, pixel_values=torch.from_numpy(pixels_160()), interpolate_pos_encoding=True)
        _save("tower_outputs_vitb32_160", {f"160/{k}": val for k, val in d.items()})


if __name__ == "__main__":
    main()
