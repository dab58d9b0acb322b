"""Generate tests/golden/token_similarity_*.npz: HF ``CLIPModel`` per-token image-text similarity -- TEST INFRASTRUCTURE.

    python tools/make_token_similarity_golden.py       # needs ``transformers``; CPU, no GPU

HF ``CLIPModel(attn_implementation="eager")`` through ``oracle.hf_reference.build_model`` on the weights and inputs of the existing golden
cases (``oracle.make_golden.case_inputs``), as tools/make_attention_summary_golden.py runs it.  Per file, in fp32 as HF computes them:

* ``token_embeds`` [B, S, P] = ``visual_projection(vision_model.post_layernorm(vision_model(pixel_values).last_hidden_state))``
* ``similarity``   [B, S, C] = <E / |E|, t / |t|> at scale 1 against the case's own HF ``text_embeds`` (tests/golden/<case>.npz; C = the
  case's caption count)

Files (each under 1 MiB; tests/token_similarity_refs.py FIXTURES):

* token_similarity_tiny.npz        -- tiny_b6: 17 tokens, P 64, C 6
* token_similarity_tinyp4.npz      -- tinyp4_b3: 257 tokens, C 3; also ``last_hidden_state`` [B, S, Dv] (no other fixture holds it)
* token_similarity_vitb32_b2.npz   -- the first two images of vitb32_b4, all four captions: 50 tokens, P 512, C 4
* token_similarity_vitb32_160.npz  -- ViT-B/32 on the 160 x 160 pixels of tools/make_tower_outputs_golden.py (``pixels_160``),
  ``interpolate_pos_encoding=True``: 26 tokens
Where the case has all its images (and for the first two of vitb32_b4) row 0 times exp(logit_scale) is checked against the case's stored
``logits_per_image`` before anything is written.  No inputs are stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _head(model, text_embeds, **kw):
    import torch
    out = model.vision_model(**kw)
    E = model.visual_projection(model.vision_model.post_layernorm(out.last_hidden_state))
    T = torch.from_numpy(text_embeds)
    sim = (E / E.norm(dim=-1, keepdim=True)) @ (T / T.norm(dim=-1, keepdim=True)).t()
    return {"token_embeds": E.float().numpy().astype(np.float32), "similarity": sim.float().numpy().astype(np.float32)}, out.last_hidden_state


def _save(name, d):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    assert size < 1 << 20, (name, size)
    print(f"wrote {path} ({size / 1024:.1f} KB)  min |E| = {np.linalg.norm(d['token_embeds'], axis=-1).min():.2f}")


def main() -> None:
    import torch

    from make_tower_outputs_golden import pixels_160
    from oracle import hf_reference as H
    from oracle.make_golden import case_inputs
    from token_similarity_refs import FIXTURES
    models = {}
    with torch.no_grad():
        for name, (case, n_img, shape) in FIXTURES.items():
            cfg, sd, px, ids, mask = case_inputs(case)
            g = dict(np.load(os.path.join(GOLDEN, case + ".npz")))
            if case not in models:
                models[case] = H.build_model(cfg, sd, "eager")
            model = models[case]
            if n_img is None:
                d, last = _head(model, g["text_embeds"], pixel_values=torch.from_numpy(pixels_160()), interpolate_pos_encoding=True)
            else:
                d, last = _head(model, g["text_embeds"], pixel_values=torch.from_numpy(px[:n_img]))
                cls = d["similarity"][:, 0, :].astype(np.float64) * float(np.exp(float(sd["logit_scale"])))
                err = np.abs(cls - g["logits_per_image"][:n_img]).max()
                print(f"{name}: CLS row x exp(logit_scale) against logits_per_image: {err:.2e}")
                assert err <= 2e-6 * float(np.exp(float(sd["logit_scale"]))), (name, err)
            B, S, P, C = shape
            assert d["token_embeds"].shape == (B, S, P) and d["similarity"].shape == (B, S, C), (name, d["token_embeds"].shape)
            if name == "token_similarity_tinyp4":
                d["last_hidden_state"] = last.float().numpy().astype(np.float32)
            _save(name, d)


if __name__ == "__main__":
    main()
