"""``PlipModel`` -- the object that replaces ``self.model`` in the reference.

It answers to the three call surfaces SURVEY.md section 8b lists:

* HF ``CLIPModel`` (plip.py:18,50,68; README.md:45-50): ``.to()``, ``.eval()``,
  ``.get_image_features(pixel_values=)``, ``.get_text_features(input_ids=, attention_mask=)``
  returning plain tensors (transformers-4.x semantics, which plip.py:50,68 relies on via
  ``.detach().cpu().numpy()``), and ``model(input_ids=, pixel_values=, attention_mask=)`` ->
  an output with ``logits_per_image / logits_per_text / image_embeds / text_embeds``.
* OpenAI ``clip`` model (reproducibility/embedders/plip.py:48,66; scripts/extract_embedding.py:33,52):
  ``.encode_image(images)``, ``.encode_text(tokens)``, ``.logit_scale``, ``model(images, tokens)``
  -> ``(logits_per_image, logits_per_text)``.

All arithmetic runs in libplipmi.so on the MI355X; there is no CPU path.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Mapping, Optional

import numpy as np
import torch

from . import weights as W
from .config import PlipConfig, get_config
from .engine import Engine
from .outputs import AttentionSummary, TokenSimilarity, TowerOutput
from .token_similarity import token_similarity


@dataclass
class PlipOutput:
    """Fields of HF ``CLIPOutput`` (modeling_clip.py:106-135) that the hot path produces."""
    logits_per_image: torch.Tensor
    logits_per_text: torch.Tensor
    text_embeds: torch.Tensor
    image_embeds: torch.Tensor
    loss: Optional[torch.Tensor] = None
    # forward(..., output_hidden_states= / output_attentions=True): the two towers' per-token outputs (CLIPOutput's fields of those names)
    text_model_output: Optional[TowerOutput] = None
    vision_model_output: Optional[TowerOutput] = None

    def __getitem__(self, k):
        return getattr(self, k)

    def to_tuple(self):
        towers = tuple(o.to_tuple() for o in (self.text_model_output, self.vision_model_output) if o is not None)
        return (self.logits_per_image, self.logits_per_text, self.text_embeds, self.image_embeds) + towers


class _Tower:
    """``CLIPModel.vision_model`` / ``.text_model``: called with the tower's input, returns a :class:`TowerOutput`."""

    def __init__(self, model: "PlipModel", vision: bool):
        self._model, self._vision = model, vision

    @torch.no_grad()
    def forward(self, *args, **kw) -> TowerOutput:
        return self._model._vision_outputs(*args, **kw) if self._vision else self._model._text_outputs(*args, **kw)

    __call__ = forward

    @torch.no_grad()
    def attention_summary(self, *args, **kw) -> AttentionSummary:
        """``vision_model.attention_summary(pixel_values, interpolate_pos_encoding=False, ...)`` /
        ``text_model.attention_summary(input_ids, attention_mask=None, ...)``: ``Engine.attention_summary`` of this tower (keywords
        ``pooled_attention``, ``rollout``, ``rollout_matrix``, ``eos_token_id``)."""
        return self._model._vision_summary(*args, **kw) if self._vision else self._model._text_summary(*args, **kw)

    @torch.no_grad()
    def token_similarity(self, *args, **kw) -> TokenSimilarity:
        """``vision_model.token_similarity(pixel_values, text_embeds, interpolate_pos_encoding=False, ...)``: per token and text row the
        scaled cosine of the token's projected embedding with the text embedding (``plip_amd.token_similarity.token_similarity``;
        keywords ``scale``, ``softmax``, ``return_embeds``).  The vision tower only."""
        if not self._vision:
            raise ValueError("token_similarity scores image tokens against text embeddings: call it on vision_model")
        return self._model._vision_token_similarity(*args, **kw)


class PlipModel:
    def __init__(self, cfg: PlipConfig, state_dict: Mapping[str, object], device="cuda:0", dtype="bf16",
                 max_batch: int = 256, **engine_options):
        """``dtype``: "bf16", "f16" (the reference's own GPU type; 8x smaller operand rounding at the same speed) or "f32".
        ``engine_options``: the per-handle switches of :class:`plip_amd.engine.Engine` (ln_fold, pooled_last_block,
        pack_captions, mfma_attention, graph_batch, text_f16, text_f16_layers, latency_batch)."""
        self.config = cfg
        self.engine = Engine(cfg, state_dict, device=device, dtype=dtype, max_batch=max_batch, **engine_options)
        self.device = self.engine.device
        self.dtype = torch.float32          # I/O dtype; the compute dtype is engine.dtype_name
        self.training = False
        # OpenAI-clip exposes the parameter itself (training_model/clip.py:206 clamps it)
        self.logit_scale = torch.tensor(self.engine.logit_scale, dtype=torch.float32, device=self.device)
        # HF CLIPVisionTransformer / CLIPTextTransformer: per-token outputs (Engine.tower_outputs)
        self.vision_model = _Tower(self, vision=True)
        self.text_model = _Tower(self, vision=False)

    # ---- construction -----------------------------------------------------
    @classmethod
    def from_state_dict(cls, state_dict, cfg: Optional[PlipConfig] = None, hidden_act=None, **kw) -> "PlipModel":
        """``hidden_act``: "gelu" / "quick_gelu" / a ``(vision, text)`` pair, overriding the config's (weights.normalize_state_dict)."""
        sd, cfg = W.normalize_state_dict(state_dict, cfg, hidden_act)
        return cls(cfg, sd, **kw)

    @classmethod
    def from_pretrained(cls, path: str, arch: Optional[str] = None, hidden_act=None, **kw) -> "PlipModel":
        """Local HF directory (what ``CLIPModel.from_pretrained`` takes, plip.py:26) or an
        OpenAI-clip ``.pt`` state dict (factory.py:23-25).  No hub download: this box has no network.
        ``hidden_act``: the towers' MLP activation where the checkpoint cannot say it (an open_clip ``.pt``: "gelu") or to
        override its ``config.json`` -- "gelu", "quick_gelu" or a ``(vision, text)`` pair (weights.load_checkpoint)."""
        sd, cfg = W.load_checkpoint(path, arch, hidden_act=hidden_act)
        return cls(cfg, sd, **kw)

    @classmethod
    def from_synthetic(cls, arch: str = "ViT-B/32", seed: int = 0, logit_scale=None, hidden_act=None, **kw) -> "PlipModel":
        cfg = (get_config(arch) if isinstance(arch, str) else arch).with_hidden_act(hidden_act)
        return cls(cfg, W.synthetic_state_dict(cfg, seed, logit_scale), **kw)

    # ---- nn.Module-ish no-ops the callers use ---------------------------------
    def to(self, device=None, *a, **kw):
        if device is not None and torch.device(device).type != "cuda":
            raise RuntimeError("PlipModel lives on the MI355X it was created on; there is no CPU path")
        return self

    def eval(self):
        return self

    def float(self):
        return self

    def parameters(self):
        return iter(())

    # ---- HF surface ---------------------------------------------------------
    def _image_engine(self, pixel_values, interpolate_pos_encoding: bool) -> Engine:
        """The engine for these pixels: with ``interpolate_pos_encoding`` (HF modeling_clip.py CLIPVisionEmbeddings) images of
        another size run on ``Engine.at_resolution`` -- the checkpoint's own size stays on this engine, as HF keeps its table there;
        without it the engine's own shape check raises HF's ValueError."""
        if not interpolate_pos_encoding or not torch.is_tensor(pixel_values) or pixel_values.dim() != 4:
            return self.engine
        hw = tuple(pixel_values.shape[1:3]) if pixel_values.dtype == torch.uint8 else tuple(pixel_values.shape[2:4])
        return self.engine if hw == self.engine.image_hw else self.engine.at_resolution(*hw)

    @torch.no_grad()
    def get_image_features(self, pixel_values=None, interpolate_pos_encoding: bool = False, **_ignored) -> torch.Tensor:
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        return self._image_engine(pixel_values, interpolate_pos_encoding).encode_image(pixel_values, normalize=False)

    @torch.no_grad()
    def get_text_features(self, input_ids=None, attention_mask=None, **_ignored) -> torch.Tensor:
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        return self.engine.encode_text(input_ids, attention_mask, normalize=False)

    def _vision_outputs(self, pixel_values=None, output_attentions: bool = False, output_hidden_states: bool = False,
                        interpolate_pos_encoding: bool = False, **_ignored) -> TowerOutput:
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        return self._image_engine(pixel_values, interpolate_pos_encoding).tower_outputs(
            "vision", pixel_values, output_hidden_states=bool(output_hidden_states), output_attentions=bool(output_attentions))

    def _text_outputs(self, input_ids=None, attention_mask=None, output_attentions: bool = False, output_hidden_states: bool = False,
                      **_ignored) -> TowerOutput:
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        return self.engine.tower_outputs("text", input_ids, attention_mask, output_hidden_states=bool(output_hidden_states),
                                         output_attentions=bool(output_attentions))

    def _vision_summary(self, pixel_values=None, interpolate_pos_encoding: bool = False, **summary_options) -> AttentionSummary:
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        return self._image_engine(pixel_values, interpolate_pos_encoding).attention_summary("vision", pixel_values, **summary_options)

    def _vision_token_similarity(self, pixel_values=None, text_embeds=None, interpolate_pos_encoding: bool = False,
                                 **options) -> TokenSimilarity:
        if pixel_values is None or text_embeds is None:
            raise ValueError("You have to specify pixel_values and text_embeds")
        return token_similarity(self._image_engine(pixel_values, interpolate_pos_encoding), pixel_values, text_embeds, **options)

    def _text_summary(self, input_ids=None, attention_mask=None, **summary_options) -> AttentionSummary:
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        return self.engine.attention_summary("text", input_ids, attention_mask, **summary_options)

    @torch.no_grad()
    def forward(self, input_ids=None, pixel_values=None, attention_mask=None, interpolate_pos_encoding: bool = False,
                output_attentions: bool = False, output_hidden_states: bool = False, **_ignored):
        # OpenAI calling convention: model(images, tokens) -> (logits_per_image, logits_per_text)
        openai_style = (input_ids is not None and torch.is_tensor(input_ids) and input_ids.is_floating_point()
                        and pixel_values is not None and not pixel_values.is_floating_point())
        if openai_style:
            input_ids, pixel_values = pixel_values, input_ids
        if input_ids is None or pixel_values is None:
            raise ValueError("You have to specify input_ids and pixel_values")
        # modeling_clip.py:793-811: the two towers, here side by side on two HIP streams (Engine.encode_pair: the bits of the
        # one-stream order, the bench's step -- 4.4 -> 4.2 ms at bs = 256)
        # (interpolate_pos_encoding: both towers on the derived engine -- same weights, the text tower as this engine's)
        eng = self._image_engine(pixel_values, interpolate_pos_encoding)
        img, txt = eng.encode_pair(pixel_values, input_ids, attention_mask, normalize=True)
        lpi, lpt, _ = self.engine.logits(img, txt, scale=float(np.exp(float(self.logit_scale))))  # :814-817
        if openai_style:
            return lpi, lpt
        out = PlipOutput(logits_per_image=lpi, logits_per_text=lpt, text_embeds=txt, image_embeds=img)
        if output_attentions or output_hidden_states:
            # modeling_clip.py CLIPModel.forward: the towers' own outputs ride along (a separate dense, eager walk of each tower;
            # the embeddings above are the encode path's)
            out.text_model_output = self._text_outputs(input_ids, attention_mask, output_attentions, output_hidden_states)
            out.vision_model_output = self._vision_outputs(pixel_values, output_attentions, output_hidden_states, interpolate_pos_encoding)
        return out

    __call__ = forward

    # ---- OpenAI-clip surface --------------------------------------------------
    def encode_image(self, image: torch.Tensor) -> torch.Tensor:
        return self.engine.encode_image(image, normalize=False)

    def encode_text(self, text: torch.Tensor) -> torch.Tensor:
        # clip.tokenize pads with 0 and OpenAI pools at text.argmax(-1): the legacy rule (eos id 2 / <0)
        return self.engine.encode_text(text, None, normalize=False, eos_token_id=-1)
