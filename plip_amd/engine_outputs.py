"""Every-token outputs of a tower: HF's ``last_hidden_state`` / ``hidden_states`` / ``attentions``, the attention summaries that do
without the [L,B,H,S,S] tensor, and ``hidden`` -- the parity tests' window on one block (include/plipmi_test.h, the one test hook a
product class carries).  Mixed into ``plip_amd.engine.Engine``; all of it runs on this engine alone and keeps no state."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import _ptr, _tower_code
from .outputs import AttentionSummary, TowerOutput, attention_summary_bytes, tower_output_bytes


class OutputsMixin:
    def tower_shape(self, tower: str):
        """(S tokens, D width, H heads, L blocks) of ``tower`` ("vision" / "text") on this engine (include/plipmi.h plipmi_tower_shape)."""
        shape = (C.c_int32 * 4)()
        _lib.check(self.lib.plipmi_tower_shape(self._h, _tower_code(tower), shape), "plipmi_tower_shape")
        return tuple(int(v) for v in shape)

    def _tower_input_check(self, tower: str, inp: torch.Tensor, attention_mask):
        """the input checks ``tower_outputs`` and ``attention_summary`` share -> (tower code, (S, D, H, L), B, the chunk list)"""
        cfg, code = self.cfg, _tower_code(tower)
        if code == _lib.VISION:
            if attention_mask is not None:
                raise ValueError("the vision tower takes no attention_mask")
            ih, iw = self.image_hw
            if inp.dim() != 4 or tuple(inp.shape[1:]) != (3, ih, iw):
                raise ValueError(f"Input image size ({tuple(inp.shape)}) doesn't match model ([B,3,{ih},{iw}]).")
        elif inp.dim() != 2 or inp.shape[1] != cfg.context_length:
            raise ValueError(f"input_ids must be [B,{cfg.context_length}], got {tuple(inp.shape)}")
        elif inp.device.type == "cpu" and inp.numel() and (int(inp.min()) < 0 or int(inp.max()) >= cfg.vocab_size):
            raise IndexError(f"token id out of range [0,{cfg.vocab_size})")
        return code, self.tower_shape(tower), int(inp.shape[0]), self._chunks(int(inp.shape[0]))

    def _tower_chunks(self, code: int, inp, attention_mask, chunks, staged, call) -> None:
        """What ``tower_outputs`` and ``attention_summary`` share once their memory checks have passed: input and mask go to the
        device, then ``call(x rows, mask rows, a, b, *parts)`` runs for rows a..b of every chunk.  ``staged``: the outputs laid out
        [L, B, ...] (None = not asked for) -- a chunk's rows are not contiguous in them, so one chunk writes the caller's tensor
        itself, and several chunks each write a [L, b - a, ...] part that is copied into place and freed before the next one."""
        x = inp.to(device=self.device, dtype=torch.float32 if code == _lib.VISION else torch.int64).contiguous()
        mask = None if attention_mask is None else attention_mask.to(device=self.device, dtype=torch.int64).contiguous()
        one = len(chunks) == 1
        for a, b in chunks:
            parts = [t if one or t is None else torch.empty((t.shape[0], b - a) + t.shape[2:], dtype=t.dtype, device=t.device)
                     for t in staged]
            call(_ptr(x[a:b]), _ptr(None if mask is None else mask[a:b]), a, b, *parts)
            if not one:
                for t, part in zip(staged, parts):
                    if t is not None:
                        t[:, a:b].copy_(part)
                parts = part = None

    def tower_outputs(self, tower: str, inp: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                      output_hidden_states: bool = False, output_attentions: bool = False,
                      eos_token_id: Optional[int] = None) -> TowerOutput:
        """HF ``CLIPModel.vision_model(pixel_values)`` / ``.text_model(input_ids, attention_mask)`` (include/plipmi.h
        plipmi_encode_tower_outputs): ``last_hidden_state`` [B,S,D], ``pooler_output`` [B,D] and, when asked for, ``hidden_states``
        (L+1 tensors [B,S,D]) and ``attentions`` (L tensors [B,H,S,S]), fp32 on the GPU.  Runs in chunks of ``max_batch`` samples on
        this engine.  Raises ValueError before allocating anything when the outputs (and, over several chunks, one chunk's staging)
        would not fit the device's free memory -- ViT-L/14@336 attentions alone are 511 MB per image."""
        code, (S, D, H, L), B, chunks = self._tower_input_check(tower, inp, attention_mask)
        nb = tower_output_bytes(B, S, D, H, L, hidden_states=output_hidden_states, attentions=output_attentions)
        staged = tower_output_bytes(min(B, self.max_batch), S, D, H, L, False, False, output_hidden_states, output_attentions)
        need = sum(nb.values()) + (sum(staged.values()) if len(chunks) > 1 else 0)
        free, _ = torch.cuda.mem_get_info(self.device)
        if need > free:
            raise ValueError(f"{tower} tower outputs for {B} samples need {need / 2**20:.0f} MiB of device memory, {free / 2**20:.0f} MiB "
                             f"are free (attentions: {nb['attentions'] / 2**20:.0f} MiB): pass fewer samples or drop output_attentions / "
                             "output_hidden_states")
        eos = self.cfg.eos_token_id if eos_token_id is None else int(eos_token_id)
        dev = dict(device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            last = torch.empty((B, S, D), **dev)
            pooled = torch.empty((B, D), **dev)
            hs = torch.empty((L + 1, B, S, D), **dev) if output_hidden_states else None
            att = torch.empty((L, B, H, S, S), **dev) if output_attentions else None
            self._tower_chunks(code, inp, attention_mask, chunks, (hs, att), lambda x, mask, a, b, hs_c, att_c: _lib.check(
                self.lib.plipmi_encode_tower_outputs(self._h, code, x, mask, b - a, eos, _ptr(last[a:b]), _ptr(pooled[a:b]),
                                                     _ptr(hs_c), _ptr(att_c), self._stream()), "plipmi_encode_tower_outputs"))
        return TowerOutput(last_hidden_state=last, pooler_output=pooled, hidden_states=None if hs is None else tuple(hs.unbind(0)),
                           attentions=None if att is None else tuple(att.unbind(0)))

    def attention_summary(self, tower: str, inp: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                          pooled_attention: bool = True, rollout: bool = True, rollout_matrix: bool = False,
                          eos_token_id: Optional[int] = None) -> AttentionSummary:
        """What attention maps are mostly pulled for, without the [L,B,H,S,S] tensor (include/plipmi.h plipmi_encode_attention_summary):
        ``pooled_attention`` -- L tensors [B,H,S], the pooled query row (CLS; the caption's EOS row) of every head, the bits
        ``tower_outputs(..., output_attentions=True).attentions`` holds there --, ``rollout`` [B,S] -- the pooled row of the attention
        rollout (residual weight 1/2, head mean) -- and ``rollout_matrix`` [B,S,S], the whole rollout; fp32 on the GPU.  Inputs as
        ``tower_outputs``; runs in chunks of ``max_batch`` samples on this engine.  Raises ValueError before allocating anything when
        outputs and scratch would not fit the device's free memory."""
        code, (S, D, H, L), B, chunks = self._tower_input_check(tower, inp, attention_mask)
        if not (pooled_attention or rollout or rollout_matrix):
            raise ValueError("attention_summary: nothing asked for (pooled_attention, rollout and rollout_matrix are all off)")
        nb = attention_summary_bytes(B, S, H, L, pooled_attention, rollout, rollout_matrix)
        per_chunk = attention_summary_bytes(min(B, self.max_batch), S, H, L, pooled_attention, rollout, rollout_matrix)
        need = nb["pooled_attention"] + nb["rollout"] + nb["rollout_matrix"] + per_chunk["scratch"] + \
            (per_chunk["pooled_attention"] if len(chunks) > 1 else 0)
        free, _ = torch.cuda.mem_get_info(self.device)
        if need > free:
            raise ValueError(f"{tower} attention summary for {B} samples needs {need / 2**20:.0f} MiB of device memory, "
                             f"{free / 2**20:.0f} MiB are free: pass fewer samples or drop rollout_matrix")
        eos = self.cfg.eos_token_id if eos_token_id is None else int(eos_token_id)
        dev = dict(device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            pa = torch.empty((L, B, H, S), **dev) if pooled_attention else None
            ro = torch.empty((B, S), **dev) if rollout else None
            rm = torch.empty((B, S, S), **dev) if rollout_matrix else None
            self._tower_chunks(code, inp, attention_mask, chunks, (pa,), lambda x, mask, a, b, pa_c: _lib.check(
                self.lib.plipmi_encode_attention_summary(self._h, code, x, mask, b - a, eos, _ptr(pa_c), _ptr(None if ro is None else ro[a:b]),
                                                         _ptr(None if rm is None else rm[a:b]), self._stream()),
                "plipmi_encode_attention_summary"))
        return AttentionSummary(pooled_attention=None if pa is None else tuple(pa.unbind(0)), rollout=ro, rollout_matrix=rm)

    def hidden(self, tower: str, layer: int, inp: torch.Tensor) -> torch.Tensor:
        """HF ``hidden_states[layer]`` of a tower (parity tests)."""
        code = _tower_code(tower)
        vision = code == _lib.VISION
        S, D = (self.v_tokens, self.cfg.v_width) if vision else (self.cfg.context_length, self.cfg.t_width)
        with torch.cuda.device(self.device):
            x = inp.to(device=self.device, dtype=torch.float32 if vision else torch.int64).contiguous()
            if x.shape[0] > self.max_batch:
                raise ValueError("batch larger than max_batch")
            out = torch.empty((x.shape[0], S, D), dtype=torch.float32, device=self.device)
            _lib.check(self.lib.plipmi_debug_hidden(self._h, code, int(layer), _ptr(x), x.shape[0], _ptr(out), self._stream()),
                       "plipmi_debug_hidden")
        return out
