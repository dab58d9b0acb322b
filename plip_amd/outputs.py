"""Per-token tower outputs: the ``BaseModelOutputWithPooling`` of HF ``CLIPVisionTransformer`` / ``CLIPTextTransformer``
(``last_hidden_state``, ``pooler_output``, ``hidden_states``, ``attentions``) and the buffer arithmetic of
``plipmi_encode_tower_outputs`` (include/plipmi.h).  No GPU needed here."""
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
