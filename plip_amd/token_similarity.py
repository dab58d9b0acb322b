"""Dense image-text similarity: one score per token (CLS + every patch) and text prompt -- "where in this tile is <prompt>?"
(include/plipmi.h plipmi_encode_token_similarity; csrc/token_scores.hip).  A function on an engine, not a method of it:
``token_similarity(engine, pixels, text_embeds)``; ``PlipModel.vision_model.token_similarity`` and ``PLIP.similarity_maps`` route here.
Runs on the given engine alone and keeps no state."""
from __future__ import annotations

import torch

from . import _lib
from ._lib import TOKEN_SIM_MAX_C, _ptr
from .outputs import TokenSimilarity, token_similarity_bytes


def token_similarity(engine, pixels: torch.Tensor, text_embeds: torch.Tensor, scale: float = 1.0, softmax: bool = False,
                     return_embeds: bool = False) -> TokenSimilarity:
    """``similarity`` [B,S,C] = scale * cosine(E[b,s], text_embeds[c]) with E = visual_projection(post_layernorm(last_hidden_state)) on
    every token of ``pixels`` (fp32 [B,3,H,W] at the engine's image size; row 0 = CLS, then the patch grid row-major), or with
    ``softmax`` its softmax over the C text rows; ``return_embeds``: also ``token_embeds`` [B,S,P], E itself.  ``text_embeds`` [C,P]
    float, rows of any norm (what ``encode_text(..., normalize=False)`` returns will do), 1 <= C <= 64; a model whose ``projection_dim``
    is no multiple of 32 is refused with ValueError (the per-token projection has no kernel for it).  fp32 on the GPU; runs in chunks
    of ``max_batch`` images.  Raises ValueError before allocating anything when outputs and scratch would not fit the device's free
    memory."""
    code, (S, D, H, L), B, chunks = engine._tower_input_check("vision", pixels, None)
    P = engine.cfg.projection_dim
    if P % 32:      # refused here as in the C entry, before anything is allocated or launched: there is no kernel for such a head
        raise ValueError(f"projection_dim = {P}: the per-token head takes multiples of 32 (the encode paths take any width)")
    if not torch.is_tensor(text_embeds):
        text_embeds = torch.as_tensor(text_embeds)
    if text_embeds.dim() != 2 or text_embeds.shape[1] != P or not text_embeds.is_floating_point():
        raise ValueError(f"text_embeds must be a float [C,{P}] array, got {tuple(text_embeds.shape)} {text_embeds.dtype}")
    Cn = int(text_embeds.shape[0])
    if Cn < 1 or Cn > TOKEN_SIM_MAX_C:
        raise ValueError(f"text_embeds holds {Cn} rows: 1 .. {TOKEN_SIM_MAX_C} prompts per call (the limit of the scores kernel)")
    nb = token_similarity_bytes(B, S, D, P, Cn, return_embeds)
    per_chunk = token_similarity_bytes(min(B, engine.max_batch), S, D, P, Cn, return_embeds)
    need = nb["similarity"] + nb["token_embeds"] + per_chunk["scratch"] + 4 * Cn * P + pixels.numel() * 4
    free, _ = torch.cuda.mem_get_info(engine.device)
    if need > free:
        raise ValueError(f"token similarity for {B} images needs {need / 2**20:.0f} MiB of device memory, {free / 2**20:.0f} MiB are "
                         "free: pass fewer images" + (" or drop return_embeds" if return_embeds else ""))
    dev = dict(device=engine.device, dtype=torch.float32)
    with torch.cuda.device(engine.device):
        txt = text_embeds.to(**dev).contiguous()
        x = pixels.to(**dev).contiguous()
        sim = torch.empty((B, S, Cn), **dev)
        emb = torch.empty((B, S, P), **dev) if return_embeds else None
        for a, b in chunks:
            _lib.check(engine.lib.plipmi_encode_token_similarity(engine._h, _ptr(x[a:b]), b - a, _ptr(txt), Cn, float(scale),
                                                                 int(bool(softmax)), _ptr(None if emb is None else emb[a:b]),
                                                                 _ptr(sim[a:b]), engine._stream()), "plipmi_encode_token_similarity")
    return TokenSimilarity(similarity=sim, token_embeds=emb)
