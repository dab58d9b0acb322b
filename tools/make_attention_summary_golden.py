"""Generate tests/golden/attention_summary_*.npz: HF ``CLIPModel`` attention summaries -- TEST INFRASTRUCTURE.

    python tools/make_attention_summary_golden.py       # needs ``transformers``; CPU, no GPU

HF ``CLIPModel(attn_implementation="eager")`` through ``oracle.hf_reference.build_model`` on the weights and inputs of the existing golden
cases (``oracle.make_golden.case_inputs``), as tools/make_tower_outputs_golden.py runs it; from every block's ``attentions`` [B, H, S, S]:

* ``<tower>_pooled_attention`` fp32 [L, B, H, S] -- the pooled query row r_b of every block and head (vision: row 0; text: the row the
  case's ``eos_token_id`` rule pools),
* ``<tower>_rollout_matrix`` [B, S, S] -- ``tests/attention_summary_refs.rollout_ref`` of all L blocks, computed in float64 and stored
  as fp32 (the rounding, 6e-8, is far below every tolerance it is used with),
* ``<tower>_rollout`` [B, S] -- row r_b of it, and ``<tower>_rows`` int64 [B] = r_b.

Files (each under 1 MiB):

* attention_summary_vitb32_b2.npz  -- ViT-B/32, the first two samples of vitb32_b4: ``vision_*`` and ``text_*`` (captions under their mask)
* attention_summary_vitb32_160.npz -- ViT-B/32 vision on the 160 x 160 pixels of tools/make_tower_outputs_golden.py (``pixels_160``),
  ``interpolate_pos_encoding=True``: 26 tokens
* attention_summary_tinyp4.npz     -- the ``tiny-p4`` arch, tinyp4_b3 vision: 257 tokens
The ``tiny`` arch needs no file of its own: tower_outputs_tiny.npz holds every block's attentions.  No inputs are stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _summary(model, tower, rows_of, **kw):
    from attention_summary_refs import rollout_ref
    out = (model.vision_model if tower == "vision" else model.text_model)(output_attentions=True, **kw)
    att = [a.float().numpy() for a in out.attentions]
    B = att[0].shape[0]
    rows = rows_of(B)
    R = rollout_ref(att)
    idx = np.arange(B)
    return {f"{tower}_pooled_attention": np.stack([a[idx, :, rows, :] for a in att]).astype(np.float32),
            f"{tower}_rollout_matrix": R.astype(np.float32),
            f"{tower}_rollout": R[idx, rows].astype(np.float32),
            f"{tower}_rows": rows.astype(np.int64)}


def _save(name, d):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    assert size < 1 << 20, (name, size)
    print(f"wrote {path} ({size / 1024:.1f} KB)")


def main() -> None:
    import torch

    from attention_summary_refs import pooled_rows
    from make_tower_outputs_golden import pixels_160
    from oracle import hf_reference as H
    from oracle.make_golden import case_inputs
    cls = lambda B: pooled_rows("vision", B)
    with torch.no_grad():
        cfg, sd, px, ids, mask = case_inputs("vitb32_b4")
        model = H.build_model(cfg, sd, "eager")
        d = _summary(model, "vision", cls, pixel_values=torch.from_numpy(px[:2]))
        d.update(_summary(model, "text", lambda B: pooled_rows("text", B, ids[:2], cfg.eos_token_id),
                          input_ids=torch.from_numpy(ids[:2]), attention_mask=torch.from_numpy(mask[:2])))
        _save("attention_summary_vitb32_b2", d)
        _save("attention_summary_vitb32_160", _summary(model, "vision", cls, pixel_values=torch.from_numpy(pixels_160()),
                                                       interpolate_pos_encoding=True))
        cfg, sd, px, ids, mask = case_inputs("tinyp4_b3")
        model = H.build_model(cfg, sd, "eager")
        _save("attention_summary_tinyp4", _summary(model, "vision", cls, pixel_values=torch.from_numpy(px)))


if __name__ == "__main__":
    main()
