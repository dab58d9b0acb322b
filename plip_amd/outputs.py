"""Per-token tower outputs: the ``BaseModelOutputWithPooling`` of HF ``CLIPVisionTransformer`` / ``CLIPTextTransformer``
(``last_hidden_state``, ``pooler_output``, ``hidden_states``, ``attentions``) and the buffer arithmetic of
``plipmi_encode_tower_outputs`` (include/plipmi.h); the attention summaries of ``plipmi_encode_attention_summary``; the per-token
image-text scores of ``plipmi_encode_token_similarity``.  No GPU needed here."""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Optional, Tuple

import torch


@dataclass
class TowerOutput:
    """HF ``BaseModelOutputWithPooling`` semantics: ``to_tuple()`` holds the fields that are not None, in declaration order;
    an int index or slice reads that tuple, a str key reads a field that is set (KeyError for one that is None)."""
    last_hidden_state: Optional[torch.Tensor] = None
    pooler_output: Optional[torch.Tensor] = None
    hidden_states: Optional[Tuple[torch.Tensor, ...]] = None
    attentions: Optional[Tuple[torch.Tensor, ...]] = None

    def keys(self):
        return [f.name for f in fields(self) if getattr(self, f.name) is not None]

    def to_tuple(self):
        return tuple(getattr(self, k) for k in self.keys())

    def __getitem__(self, k):
        if isinstance(k, str):
            if getattr(self, k, None) is None:
                raise KeyError(k)
            return getattr(self, k)
        return self.to_tuple()[k]

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())


def tower_output_bytes(B: int, S: int, D: int, H: int, L: int, last_hidden: bool = True, pooled: bool = True,
                       hidden_states: bool = False, attentions: bool = False) -> dict:
    """fp32 bytes of each buffer ``plipmi_encode_tower_outputs`` writes for B samples of a tower of S tokens, width D, H heads and
    L blocks (0 for one that is not asked for): last_hidden [B,S,D], pooled [B,D], hidden_states [L+1,B,S,D], attentions [L,B,H,S,S]."""
    return {"last_hidden": 4 * B * S * D if last_hidden else 0,
            "pooled": 4 * B * D if pooled else 0,
            "hidden_states": 4 * (L + 1) * B * S * D if hidden_states else 0,
            "attentions": 4 * L * B * H * S * S if attentions else 0}


@dataclass
class AttentionSummary:
    """``Engine.attention_summary`` (include/plipmi.h plipmi_encode_attention_summary), fp32 on the GPU; a field that was not asked
    for is None.  ``pooled_attention``: L tensors [B,H,S], the pooled query row (CLS / EOS) of every head's probabilities;
    ``rollout``: [B,S], the pooled row of the attention rollout; ``rollout_matrix``: [B,S,S], the whole rollout."""
    pooled_attention: Optional[Tuple[torch.Tensor, ...]] = None
    rollout: Optional[torch.Tensor] = None
    rollout_matrix: Optional[torch.Tensor] = None


def attention_summary_bytes(B: int, S: int, H: int, L: int, pooled_attention: bool = True, rollout: bool = True,
                            rollout_matrix: bool = False) -> dict:
    """fp32 bytes of each buffer ``plipmi_encode_attention_summary`` writes for B samples (0 for one that is not asked for) and of the
    handle scratch one call of B samples reserves: pooled_attention [L,B,H,S], rollout [B,S], rollout_matrix [B,S,S]; scratch = the
    rollout's [B,S,S] buffers the caller does not bring (two, one beside a rollout_matrix) plus the row indices."""
    roll = rollout or rollout_matrix
    return {"pooled_attention": 4 * L * B * H * S if pooled_attention else 0,
            "rollout": 4 * B * S if rollout else 0,
            "rollout_matrix": 4 * B * S * S if rollout_matrix else 0,
            "scratch": 4 * B + (4 * B * S * S * (1 if rollout_matrix else 2) if roll else 0)}


@dataclass
class TokenSimilarity:
    """``plip_amd.token_similarity.token_similarity`` (include/plipmi.h plipmi_encode_token_similarity), fp32 on the GPU.
    ``similarity``: [B,S,C], per token (row 0 = CLS, then the patches row-major) and text row the scaled cosine, or its softmax over C;
    ``token_embeds``: [B,S,P], the un-normalised projected embedding of every token -- None unless asked for."""
    similarity: Optional[torch.Tensor] = None
    token_embeds: Optional[torch.Tensor] = None


def token_similarity_bytes(B: int, S: int, D: int, P: int, C: int, token_embeds: bool = False) -> dict:
    """fp32 bytes of each buffer ``plipmi_encode_token_similarity`` writes for B images of S tokens (vision width D, projection P, C text
    rows; 0 for a token_embeds nobody asked for) and of the handle scratch one call of B images reserves: similarity [B,S,C],
    token_embeds [B,S,P]; scratch = the post_layernorm'd rows [B,S,D] (rounded up to 256 bytes) plus E [B,S,P] when the caller takes
    no token_embeds."""
    ln = (4 * B * S * D + 255) // 256 * 256
    return {"similarity": 4 * B * S * C,
            "token_embeds": 4 * B * S * P if token_embeds else 0,
            "scratch": ln + (0 if token_embeds else 4 * B * S * P)}


@dataclass
class KMeansResult:
    """``plip_amd.kmeans.kmeans_fit`` (include/plipmi.h plipmi_kmeans_fit): device tensors and Python scalars.  ``centers`` fp32 [K,D];
    ``labels`` int32 [N]; ``scores`` fp32 [N], each row's ``x . c + h`` at its own centre; ``counts`` int32 [K]; ``representatives`` int32
    [K], the member of each cluster with the largest score (-1 for an empty cluster); ``inertia``; ``n_iter``; ``converged``;
    ``relocations``, the empty clusters that were given a new centre.  Everything belongs to the returned ``centers``."""
    centers: torch.Tensor
    labels: torch.Tensor
    scores: torch.Tensor
    counts: torch.Tensor
    representatives: torch.Tensor
    inertia: float
    n_iter: int
    converged: bool
    relocations: int
