"""CPU restatement (numpy) of the arithmetic behind PLIP.encode_images /
PLIP.encode_text / CLIPModel.forward -- TEST INFRASTRUCTURE, not product code.

Where the algorithm lives
-------------------------
/root/reference/plip.py:50,68 delegate every FLOP to HuggingFace
``transformers`` ``CLIPModel`` -- a third-party dependency that is NOT vendored
in the reference tree and is NOT pinned there (requirements.txt is empty,
setup.py:3-4,33).  The version restated here is transformers **5.15.0**
(the one installed in this image); ``$HF`` below =
``transformers/models/clip/modeling_clip.py`` of that version.  The
reproducibility/ scripts call the OpenAI ``clip`` package for the same network
(reproducibility/embedders/plip.py:48,66), un-pinned and not installed.

Pinning
-------
The reference ships no tests, golden vectors or known-answer values for this
path -- at the level of the reference repository parity is
therefore "unpinned".  This oracle is instead pinned against the reference's
actual arithmetic run in this container: ``oracle/make_golden.py`` loads the
same synthetic weights into HF ``CLIPModel`` (CPU, fp32, eager and sdpa
attention) and stores its outputs under tests/golden/; tests/test_oracle.py
checks every function here against those fixtures (and against a live HF model
when ``transformers`` is importable).

All functions take/return numpy arrays; ``dtype`` selects float32 (the
reference precision) or float64 (error budgeting).
"""
from __future__ import annotations

import numpy as np


def _f(sd, key, dtype):
    return np.asarray(sd[key], dtype=dtype)


def layer_norm(x, weight, bias, eps):
    """``nn.LayerNorm`` over the last axis, biased variance ($HF:358,360,559,605,608)."""
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    var = (xc * xc).mean(axis=-1, keepdims=True)
    return xc / np.sqrt(var + x.dtype.type(eps)) * weight + bias


def quick_gelu(x):
    """``x * sigmoid(1.702 x)`` -- hidden_act="quick_gelu"
    (transformers/activations.py:117-123, configuration_clip.py:54,105)."""
    return x / (1.0 + np.exp(x.dtype.type(-1.702) * x))


def gelu(x):
    """``0.5 x (1 + erf(x / sqrt 2))`` -- hidden_act="gelu" (transformers/activations.py GELUActivation = ``nn.functional.gelu``,
    the erf form; CLIP has no tanh form).  erf is evaluated in float64 by torch's CPU kernel whatever the working dtype, so the
    float32 oracle's activation carries one rounding, not an approximation of erf."""
    import torch
    e = torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64) / np.sqrt(2.0))).numpy()
    return (0.5 * np.asarray(x, dtype=np.float64) * (1.0 + e)).astype(x.dtype)


ACTIVATIONS = {"quick_gelu": quick_gelu, "gelu": gelu}


def activation(name):
    """HF ``hidden_act`` name -> function; any other name is an error, never QuickGELU by default"""
    try:
        return ACTIVATIONS[name]
    except KeyError:
        raise ValueError(f"hidden_act = {name!r}: the oracle restates {sorted(ACTIVATIONS)}") from None


def linear(x, w, b=None):
    """``nn.Linear``: x @ w.T + b, w stored [out, in]."""
    y = x @ w.T
    return y if b is None else y + b


def attention(x, sd, prefix, heads, causal, key_mask, dtype, probs=None):
    """CLIPAttention.forward ($HF:298-335) with eager_attention_forward ($HF:259-277).

    x [B,S,D]; ``causal`` adds the text tower's causal mask; ``key_mask`` is the
    tokenizer's attention_mask [B,S] (1 = keep) combined with it the way
    ``create_causal_mask`` does ($HF:543-548).  Softmax in the working dtype
    (HF computes it in float32, $HF:271).  ``probs``: a list that receives the probabilities [B,H,S,S] (HF ``attentions``):
    a masked entry is exp(finfo.min - max) = exactly 0, as in HF's eager attention, under the causal and the key mask.
    """
    B, S, D = x.shape
    dh = D // heads
    scale = dtype(dh ** -0.5)
    q = linear(x, _f(sd, f"{prefix}.q_proj.weight", dtype), _f(sd, f"{prefix}.q_proj.bias", dtype))
    k = linear(x, _f(sd, f"{prefix}.k_proj.weight", dtype), _f(sd, f"{prefix}.k_proj.bias", dtype))
    v = linear(x, _f(sd, f"{prefix}.v_proj.weight", dtype), _f(sd, f"{prefix}.v_proj.bias", dtype))
    q = q.reshape(B, S, heads, dh).transpose(0, 2, 1, 3)
    k = k.reshape(B, S, heads, dh).transpose(0, 2, 1, 3)
    v = v.reshape(B, S, heads, dh).transpose(0, 2, 1, 3)
    scores = (q @ k.transpose(0, 1, 3, 2)) * scale               # [B,H,S,S]
    neg = np.finfo(dtype).min
    if causal:
        keep = np.tril(np.ones((S, S), dtype=bool))
        scores = np.where(keep[None, None], scores, neg)
    if key_mask is not None:
        scores = np.where(np.asarray(key_mask, dtype=bool)[:, None, None, :], scores, neg)
    scores = scores - scores.max(axis=-1, keepdims=True)
    p = np.exp(scores)
    p = p / p.sum(axis=-1, keepdims=True)
    if probs is not None:
        probs.append(p)
    o = (p @ v).transpose(0, 2, 1, 3).reshape(B, S, D)
    return linear(o, _f(sd, f"{prefix}.out_proj.weight", dtype), _f(sd, f"{prefix}.out_proj.bias", dtype))


def encoder_layer(x, sd, p, heads, causal, key_mask, eps, dtype, act=quick_gelu, probs=None):
    """CLIPEncoderLayer.forward, pre-LN residual block ($HF:362-383) with
    CLIPMLP fc1 -> ``act`` -> fc2 ($HF:346-350; ``act``: the tower's ``hidden_act``, QuickGELU unless said)."""
    h = layer_norm(x, _f(sd, f"{p}.layer_norm1.weight", dtype), _f(sd, f"{p}.layer_norm1.bias", dtype), eps)
    x = x + attention(h, sd, f"{p}.self_attn", heads, causal, key_mask, dtype, probs)
    h = layer_norm(x, _f(sd, f"{p}.layer_norm2.weight", dtype), _f(sd, f"{p}.layer_norm2.bias", dtype), eps)
    h = act(linear(h, _f(sd, f"{p}.mlp.fc1.weight", dtype), _f(sd, f"{p}.mlp.fc1.bias", dtype)))
    h = linear(h, _f(sd, f"{p}.mlp.fc2.weight", dtype), _f(sd, f"{p}.mlp.fc2.bias", dtype))
    return x + h


def unfold_patches(pixels, patch):
    """Conv2d(kernel=stride=patch) as a re-index: [B,3,H,W] -> [B, gh*gw, 3*patch*patch],
    row (i,j) row-major over the grid, column (c,u,v) -- the order of
    ``conv.weight.reshape(out, -1)`` ($HF:148-154,209-210)."""
    B, C, H, W = pixels.shape
    gh, gw = H // patch, W // patch
    x = pixels.reshape(B, C, gh, patch, gw, patch).transpose(0, 2, 4, 1, 3, 5)
    return x.reshape(B, gh * gw, C * patch * patch)


def vision_positions(sd, cfg, image_hw=None, dtype=np.float32):
    """The position table [1 + gh*gw, Dv] of ``image_hw`` = (height, width) pixels: HF's ``interpolate_pos_encoding`` ($HF:158-198).
    The grid floors to (height // patch, width // patch); the checkpoint's own table, untouched, for its own grid on a square image
    (and for ``image_hw`` None); otherwise the CLS row is kept and the patch rows are resampled by torch's CPU bicubic
    (``align_corners=False``) -- the very call HF makes, in the working dtype."""
    table = _f(sd, "vision_model.embeddings.position_embedding.weight", dtype)
    if image_hw is None:
        return table
    h, w = int(image_hw[0]), int(image_hw[1])
    gh, gw = h // cfg.patch_size, w // cfg.patch_size
    n = table.shape[0] - 1
    if gh * gw == n and h == w:
        return table
    import torch
    n0 = int(n ** 0.5)
    grid = torch.from_numpy(np.ascontiguousarray(table[1:])).reshape(1, n0, n0, -1).permute(0, 3, 1, 2)
    grid = torch.nn.functional.interpolate(grid, size=(gh, gw), mode="bicubic", align_corners=False)
    rows = grid.permute(0, 2, 3, 1).reshape(gh * gw, -1).numpy()
    return np.concatenate([table[:1], rows.astype(dtype)], axis=0)


def vision_outputs(pixels, sd, cfg, dtype=np.float32, image_hw=None, attentions=False):
    """CLIPVisionModel.forward ($HF:613-656) + visual_projection ($HF:674,751), every field: ``hidden_states`` (L+1 arrays [B,S,Dv],
    the first after pre_layrnorm), ``last_hidden_state`` (the encoder's output: HF applies post_layernorm to the pooled row only),
    ``pooler_output`` [B,Dv], ``image_features`` [B,P] and, with ``attentions``, L arrays [B,H,S,S].  ``image_hw``: the pixels are
    that size and the tower runs with ``interpolate_pos_encoding=True`` (``vision_positions``); the Conv2d drops the pixels past
    the last whole patch."""
    pixels = np.asarray(pixels, dtype=dtype)
    B = pixels.shape[0]
    Dv = cfg.v_width
    if image_hw is not None:
        assert tuple(pixels.shape[2:]) == (int(image_hw[0]), int(image_hw[1])), (pixels.shape, image_hw)
        P = cfg.patch_size
        pixels = pixels[:, :, :pixels.shape[2] // P * P, :pixels.shape[3] // P * P]
    w = _f(sd, "vision_model.embeddings.patch_embedding.weight", dtype).reshape(Dv, -1)
    patches = unfold_patches(pixels, cfg.patch_size) @ w.T                      # [B,Np,Dv], bias=False
    cls = np.broadcast_to(_f(sd, "vision_model.embeddings.class_embedding", dtype), (B, 1, Dv))
    x = np.concatenate([cls, patches], axis=1)
    x = x + vision_positions(sd, cfg, image_hw, dtype)[None]                   # $HF:212-217
    x = layer_norm(x, _f(sd, "vision_model.pre_layrnorm.weight", dtype),
                   _f(sd, "vision_model.pre_layrnorm.bias", dtype), cfg.layer_norm_eps)  # $HF:642
    hidden = [x]
    probs = [] if attentions else None
    act = activation(cfg.v_hidden_act)
    for i in range(cfg.v_layers):
        x = encoder_layer(x, sd, f"vision_model.encoder.layers.{i}", cfg.v_heads, False, None,
                          cfg.layer_norm_eps, dtype, act, probs)
        hidden.append(x)
    pooled = layer_norm(x[:, 0, :], _f(sd, "vision_model.post_layernorm.weight", dtype),
                        _f(sd, "vision_model.post_layernorm.bias", dtype), cfg.layer_norm_eps)  # $HF:650-651
    emb = pooled @ _f(sd, "visual_projection.weight", dtype).T
    return {"image_features": emb, "pooler_output": pooled, "last_hidden_state": x, "hidden_states": hidden, "attentions": probs}


def _tower_result(out, emb_key, return_hidden, return_attentions):
    res = (out[emb_key],) + ((out["hidden_states"],) if return_hidden else ()) + ((out["attentions"],) if return_attentions else ())
    return res[0] if len(res) == 1 else res


def vision_tower(pixels, sd, cfg, dtype=np.float32, return_hidden=False, image_hw=None, return_attentions=False):
    """CLIPModel.get_image_features ($HF:719-753) = CLIPVisionModel.forward
    ($HF:613-656) + visual_projection ($HF:674,751).  Returns un-normalised
    [B,P] embeddings (what plip.py:50 hands back); with ``return_hidden`` / ``return_attentions`` a tuple
    (embeddings[, hidden states][, attention probabilities]) -- ``vision_outputs`` has the fields by name."""
    return _tower_result(vision_outputs(pixels, sd, cfg, dtype, image_hw, return_attentions), "image_features",
                         return_hidden, return_attentions)


def eos_positions(ids, eos_token_id):
    """Pooled-row rule of CLIPTextModel.forward ($HF:561-581): ``eos_token_id == 2``
    (legacy configs, and the OpenAI ``text.argmax(dim=-1)`` rule) -> first
    arg-max of the ids; otherwise the first position equal to ``eos_token_id``
    (0 when absent, as ``(ids == eos).int().argmax()`` gives)."""
    ids = np.asarray(ids)
    if eos_token_id == 2 or eos_token_id < 0:
        return ids.argmax(axis=-1)
    return (ids == eos_token_id).astype(np.int32).argmax(axis=-1)


def text_outputs(ids, sd, cfg, attention_mask=None, dtype=np.float32, attentions=False):
    """CLIPTextModel.forward ($HF:513-586) + text_projection ($HF:675,713), every field: ``hidden_states`` (L+1 arrays [B,S,Dt], the
    first the embeddings), ``last_hidden_state`` (after final_layer_norm), ``pooler_output`` [B,Dt] (its ``eos_positions`` row),
    ``text_features`` [B,P] and, with ``attentions``, L arrays [B,H,S,S] under the causal and the key mask."""
    ids = np.asarray(ids)
    B, S = ids.shape
    x = _f(sd, "text_model.embeddings.token_embedding.weight", dtype)[ids]       # $HF:251
    x = x + _f(sd, "text_model.embeddings.position_embedding.weight", dtype)[None, :S]  # $HF:253-254
    hidden = [x]
    probs = [] if attentions else None
    act = activation(cfg.t_hidden_act)
    for i in range(cfg.t_layers):
        x = encoder_layer(x, sd, f"text_model.encoder.layers.{i}", cfg.t_heads, True, attention_mask,
                          cfg.layer_norm_eps, dtype, act, probs)
        hidden.append(x)
    x = layer_norm(x, _f(sd, "text_model.final_layer_norm.weight", dtype),
                   _f(sd, "text_model.final_layer_norm.bias", dtype), cfg.layer_norm_eps)  # $HF:559
    pooled = x[np.arange(B), eos_positions(ids, cfg.eos_token_id)]
    emb = pooled @ _f(sd, "text_projection.weight", dtype).T
    return {"text_features": emb, "pooler_output": pooled, "last_hidden_state": x, "hidden_states": hidden, "attentions": probs}


def text_tower(ids, sd, cfg, attention_mask=None, dtype=np.float32, return_hidden=False, return_attentions=False):
    """CLIPModel.get_text_features ($HF:683-715) = CLIPTextModel.forward
    ($HF:513-586) + text_projection ($HF:675,713); the optional returns as ``vision_tower``'s."""
    return _tower_result(text_outputs(ids, sd, cfg, attention_mask, dtype, return_attentions), "text_features",
                         return_hidden, return_attentions)


def l2_normalize(x):
    """``x / sqrt(sum(x^2))`` with no epsilon ($HF:57-65,810-811; plip.py:75)."""
    return x / np.sqrt((x * x).sum(axis=-1, keepdims=True))


def clip_forward(pixels, ids, sd, cfg, attention_mask=None, dtype=np.float32, image_hw=None):
    """CLIPModel.forward ($HF:757-831): both towers, L2 normalise both sides,
    ``logits_per_text = text @ image.T * exp(logit_scale)``, ``logits_per_image`` its transpose.
    ``image_hw``: ``interpolate_pos_encoding=True`` on pixels of that size (``vision_outputs``)."""
    img_raw = vision_tower(pixels, sd, cfg, dtype, image_hw=image_hw)
    txt_raw = text_tower(ids, sd, cfg, attention_mask, dtype)
    img, txt = l2_normalize(img_raw), l2_normalize(txt_raw)
    scale = np.exp(dtype(sd["logit_scale"]))
    lpt = (txt @ img.T) * scale
    return {"image_features": img_raw, "text_features": txt_raw, "image_embeds": img,
            "text_embeds": txt, "logits_per_text": lpt, "logits_per_image": lpt.T.copy()}


def plip_cosine_similarity(key_vectors, space_vectors, normalize=True):
    """PLIP._cosine_similarity (plip.py:73-76): only the KEY side is normalised."""
    if normalize:
        key_vectors = key_vectors / np.linalg.norm(key_vectors, ord=2, axis=-1, keepdims=True)
    return key_vectors @ space_vectors.T


def token_similarity(last_hidden_state, sd, cfg, text_rows, scale=1.0, softmax=False, dtype=np.float32):
    """The dense image-text head (include/plipmi.h plipmi_encode_token_similarity), in HF's terms
    ``visual_projection(post_layernorm(last_hidden_state))`` for EVERY token -- HF applies the two to the CLS row only --, then per
    token and text row the cosine (text rows of any norm, no epsilon) times ``scale``, optionally softmax over the text rows.
    -> (token_embeds [B,S,P], similarity [B,S,C])."""
    x = np.asarray(last_hidden_state, dtype=dtype)
    e = layer_norm(x, _f(sd, "vision_model.post_layernorm.weight", dtype), _f(sd, "vision_model.post_layernorm.bias", dtype),
                   cfg.layer_norm_eps) @ _f(sd, "visual_projection.weight", dtype).T
    s = (l2_normalize(e) @ l2_normalize(np.asarray(text_rows, dtype=dtype)).T) * dtype(scale)
    if softmax:
        s = np.exp(s - s.max(axis=-1, keepdims=True))
        s = s / s.sum(axis=-1, keepdims=True)
    return e, s
