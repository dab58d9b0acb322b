"""Thin host-side owner of one plipmi handle.  PyTorch-ROCm is used for device
memory, streams and tensors only -- all arithmetic happens inside libplipmi.so.

Here: the handle, the per-engine state, derived engines, the encode entries and the setters; the other concerns of ``Engine`` are mixed
in from ``engine_streams`` (pair stream, lanes), ``engine_heads``, ``engine_resize`` and ``engine_outputs`` (every-token outputs)."""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import math
from typing import Mapping, Optional

import numpy as np
import torch

from . import _lib
from ._lib import _TORCH_DTYPE, _code, _ptr, _stream_ptr  # noqa: F401  (this module is their import point too)
from .config import PlipConfig, get_config
from .engine_heads import HeadsMixin
from .engine_outputs import OutputsMixin
from .engine_resize import ResizeMixin, ragged_blob, ragged_blob_bytes  # noqa: F401  (this module is their import point)
from .engine_streams import _PAIR_STREAMS, _SIDE_STREAMS, StreamsMixin  # noqa: F401
from .weights import synthetic_state_dict

# bf16 engine: leading text blocks that run on f16 operands by default.  The bf16 engine's cosine error is mostly operand rounding
# in the FIRST text blocks, where the residual stream is small; eight of them cost what four do (-2.7 % of the step) and land at
# cosine 3.8e-4, text_embeds 4.2e-4 (profiles/r04_text_layer_precision.txt, profiles/r05_text_f16_layers.txt).
# text_f16_layers=0 is the pure bf16 engine, =t_layers the TEXT_TOWER_F16 one.
DEFAULT_TEXT_F16_LAYERS = 8


def _activation_flags(cfg: PlipConfig) -> int:
    """The plipmi_config.flags bits that say which MLP activation each tower runs: ``cfg.v_hidden_act`` / ``cfg.t_hidden_act`` ==
    "gelu" -> PLIPMI_FLAG_VISION_GELU / PLIPMI_FLAG_TEXT_GELU, "quick_gelu" -> no bit (the engine's default kernels)."""
    cfg.validate()      # any other name is refused, never run as QuickGELU
    return ((_lib.FLAG_VISION_GELU if cfg.v_hidden_act == "gelu" else 0) |
            (_lib.FLAG_TEXT_GELU if cfg.t_hidden_act == "gelu" else 0))


class Engine(StreamsMixin, HeadsMixin, ResizeMixin, OutputsMixin):
    """One MI355X engine = packed weights + workspace for ``max_batch`` images/captions."""

    max_resolutions = 4     # derived engines (at_resolution) kept alive per engine; the least recently used one beyond is closed

    def __init__(self, cfg: PlipConfig, state_dict: Mapping[str, object], device="cuda:0", dtype="bf16",
                 max_batch: int = 256, *, ln_fold: bool = True, pooled_last_block: bool = True,
                 pack_captions: bool = False, mfma_attention: bool = True, graph_batch: Optional[int] = None,
                 text_f16: bool = False, text_f16_layers: Optional[int] = None, latency_batch: int = 0,
                 pass_batch: Optional[int] = None, _config_struct_size: Optional[int] = None):
        """``ln_fold`` / ``pooled_last_block`` / ``mfma_attention`` = False select the A/B forms of the 16-bit engines
        (separate LayerNorm kernels, the last block on every token, the exact VALU attention kernel);
        ``text_f16`` (bf16 engine only): the text tower runs on IEEE-half operands, the image tower stays bf16;
        ``text_f16_layers`` (bf16 engine only): only that many LEADING text blocks do (None = the engine default,
        ``DEFAULT_TEXT_F16_LAYERS``; 0 = a pure bf16 engine) -- plipmi_config.text_f16_layers;
        ``graph_batch``: None = default small-batch hipGraph replay (<= 32 samples), 0 = never, n = up to n samples.
        ``pass_batch``: calls of at least twice that many samples run as equal back-to-back passes of at most that many
        (plipmi_config.pass_batch: None = automatic -- 256 for ViT-B/32 --, 0 / negative = never split); same bits either way.
        ``latency_batch``: batches of at most that many samples run on the split-K small-M GEMMs (plipmi_set_latency_batch;
        faster up to batch 8, embeddings then differ from the big-batch path's by up to 6e-4 -- off by default).
        The MLP activation of each tower (QuickGELU or the erf GELU) is the config's: ``cfg.v_hidden_act`` / ``cfg.t_hidden_act``.
        All of it is per-handle configuration (include/plipmi.h plipmi_config.flags): no environment variables.
        (``_config_struct_size``: ABI tests only -- announce a plipmi_config of that many bytes, as a caller compiled against
        an older, shorter header would.)"""
        self._init_own_state()      # first: close() -- and with it __del__ -- works on an engine whose construction raised
        # ---- what a derived engine shares with this one (_derive copies it): everything assigned from here on, and whatever the
        # caller sets on the instance later (use_lanes, max_resolutions, pair_vision_priority)
        cfg.validate()
        if not torch.cuda.is_available():
            raise RuntimeError("plip_amd needs a ROCm GPU (MI355X / gfx950): torch.cuda.is_available() is False and there is no CPU fallback")
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"device must be a cuda(ROCm) device, got {device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.dtype_code = _code(dtype)
        self.dtype_name = {_lib.BF16: "bf16", _lib.F32: "f32", _lib.F16: "f16"}[self.dtype_code]
        self.flags = ((0 if ln_fold else _lib.FLAG_SEPARATE_LAYERNORM) | (0 if pooled_last_block else _lib.FLAG_DENSE_LAST_BLOCK) |
                      (_lib.FLAG_PACK_CAPTIONS if pack_captions else 0) | (0 if mfma_attention else _lib.FLAG_VALU_ATTENTION) |
                      (_lib.FLAG_TEXT_TOWER_F16 if text_f16 else 0) | _activation_flags(cfg))
        gb = 0 if graph_batch is None else (-1 if int(graph_batch) <= 0 else int(graph_batch))
        if text_f16_layers is None:
            text_f16_layers = min(DEFAULT_TEXT_F16_LAYERS, cfg.t_layers) if (self.dtype_code == _lib.BF16 and not text_f16) else 0
        if text_f16_layers and (self.dtype_code != _lib.BF16 or text_f16):
            raise ValueError("text_f16_layers is a mode of the bf16 engine (and excludes text_f16, which is all of them)")
        self.text_f16_layers = int(text_f16_layers)
        self.max_batch = int(max_batch)
        self.pair_vision_priority = False   # experiment (tools/gpu_diag.py prio): encode_pair's vision tower on a high-priority stream
        self.lib = _lib.load()
        self.logit_scale = float(np.asarray(state_dict["logit_scale"], dtype=np.float64)) \
            if not torch.is_tensor(state_dict["logit_scale"]) else float(state_dict["logit_scale"])
        with torch.cuda.device(self.device):
            dev = {}
            for k, v in state_dict.items():
                if k == "logit_scale":
                    continue
                t = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
                dev[k] = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
            c = _lib.Config(C.sizeof(_lib.Config), cfg.image_size, cfg.patch_size, cfg.v_width, cfg.v_layers, cfg.v_heads, cfg.v_mlp,
                            cfg.vocab_size, cfg.context_length, cfg.t_width, cfg.t_layers, cfg.t_heads, cfg.t_mlp,
                            cfg.projection_dim, cfg.layer_norm_eps, self.dtype_code, self.max_batch, self.flags, gb,
                            self.text_f16_layers, 0 if pass_batch is None else (int(pass_batch) if int(pass_batch) > 0 else -1))
            if _config_struct_size is not None:
                c.struct_size = int(_config_struct_size)
            w = _lib.Weights()

            def layers(prefix, n):
                arr = (_lib.LayerWeights * n)()
                for i in range(n):
                    for short, long in _lib.LAYER_KEYS.items():
                        for suf, key in (("w", "weight"), ("b", "bias")):
                            setattr(arr[i], f"{short}_{suf}", dev[f"{prefix}.encoder.layers.{i}.{long}.{key}"].data_ptr())
                return arr

            vl, tl = layers("vision_model", cfg.v_layers), layers("text_model", cfg.t_layers)     # (the names keep the arrays alive)
            w.v_layers, w.t_layers = vl, tl
            for field, key in _lib.WEIGHT_KEYS.items():
                setattr(w, field, dev[key].data_ptr())
            stream = torch.cuda.current_stream(self.device)
            _lib.check(self.lib.plipmi_create(C.byref(c), C.byref(w), C.c_void_p(stream.cuda_stream), C.byref(self._h)), "plipmi_create")
            stream.synchronize()  # packing done -> the fp32 upload copies can go
            del dev
        self.device_name = self.lib.plipmi_device_name(self._h).decode()
        if self.device not in _SIDE_STREAMS:                                # as early as possible: the first ordinary stream of the process
            _SIDE_STREAMS[self.device] = torch.cuda.Stream(device=self.device)
        self.pass_batch = int(self.lib.plipmi_get_pass_batch(self._h))     # plipmi_config.pass_batch as resolved (0 = never split)
        if latency_batch:
            self.set_latency_batch(latency_batch)

    def _init_own_state(self) -> None:
        """Every attribute that is ONE engine's: ``__init__`` and ``_derive`` both start from this, so a derived engine (a clone, a
        lane, another resolution) never shares one of them with its source.  A new per-engine cache is declared HERE."""
        self._h = C.c_void_p()                              # the plipmi handle
        self._lanes = None                                  # [clone] once ``lanes`` has made it
        self._no_lanes = 0                                  # > 0 while encode_pair owns the second stream or profile counts this handle's launches
        self._vis = None                                    # encode_pair's high-priority vision stream (pair_vision_priority)
        self.pair_stream_ratio = None                       # what ``pair_stream`` measured for the stream it chose, if this engine chose
        self._resolutions = collections.OrderedDict()       # (height, width) -> derived engine, least recently used first
        self._res_root = None                               # the engine whose ``at_resolution`` made this one
        self._image_hw = None                               # (height, width) of an ``at_resolution`` engine
        self._resize_plans = {}                             # resize_crop_u8: (width, height, crop) -> tables on the device
        self._ragged_ws = None                              # resize_crop_ragged's workspace

    def _derive(self, what: str, make_handle, **differ) -> "Engine":
        """An engine on this one's packed weights: the shared attributes as they are now, own state fresh, the handle from
        ``make_handle(byref(handle))`` (a plipmi_clone* call), then the attributes in ``differ``."""
        other = object.__new__(Engine)
        vars(other).update(vars(self))
        other._init_own_state()
        with torch.cuda.device(self.device):
            _lib.check(make_handle(C.byref(other._h)), what)
        vars(other).update(differ)
        return other

    def clone(self) -> "Engine":
        """A second engine on the SAME packed weights with a workspace of its own (include/plipmi.h plipmi_clone): an engine runs one
        batch per tower at a time, two engines on two streams run consecutive batches of a corpus side by side (``lanes``)."""
        return self._derive("plipmi_clone", lambda h: self.lib.plipmi_clone(self._h, h),
                            use_lanes=False,        # a clone is a lane, it does not fan out itself
                            _image_hw=self._image_hw, _res_root=self._res_root)     # plipmi_clone keeps the source's size and table

    @property
    def image_hw(self):
        """(height, width) of the images this engine's vision tower takes: the checkpoint's ``image_size`` square, or the size an
        ``at_resolution`` engine was made for."""
        return self._image_hw if self._image_hw is not None else (self.cfg.image_size, self.cfg.image_size)

    @property
    def v_tokens(self) -> int:
        h, w = self.image_hw
        return 1 + (h // self.cfg.patch_size) * (w // self.cfg.patch_size)

    def at_resolution(self, height: int, width: int) -> "Engine":
        """An engine on the SAME packed weights whose vision tower runs on ``height x width`` images (include/plipmi.h
        ``plipmi_clone_resolution``): HF's ``interpolate_pos_encoding=True`` -- the patch grid floors to (height // patch) x
        (width // patch), the position table is resampled bicubically to it (the checkpoint's own table for its own grid on a square
        image).  Its ``max_batch`` keeps the vision workspace about this engine's: the largest B with B * tokens <= max_batch *
        this engine's tokens.  Cached by size: at most ``max_resolutions`` stay alive (least recently used closed), and all close
        with this engine.  Text tower, heads and setters' state are this engine's."""
        if self._res_root is not None:
            return self._res_root.at_resolution(height, width)
        key = h, w = int(height), int(width)
        cache = self._resolutions
        if key in cache and cache[key]._h.value:
            cache.move_to_end(key)
            return cache[key]
        cache.pop(key, None)            # (closed by its caller)
        p = self.cfg.patch_size
        tokens = 1 + (h // p) * (w // p) if h >= p and w >= p else 0
        mb = max(1, (self.max_batch * self.v_tokens) // tokens) if tokens else 1
        other = self._derive("plipmi_clone_resolution", lambda hd: self.lib.plipmi_clone_resolution(self._h, h, w, mb, hd),
                             _image_hw=key, _res_root=self, max_batch=mb)
        other.pass_batch = int(self.lib.plipmi_get_pass_batch(other._h))
        cache[key] = other
        while len(cache) > self.max_resolutions:
            cache.popitem(last=False)[1].close()
        return other

    def close(self):
        for other in (self._lanes or []) + list(self._resolutions.values()):
            other.close()
        self._lanes, self._res_root = None, None
        self._resolutions.clear()
        if self._h.value:
            self.lib.plipmi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return _stream_ptr(self.device)

    def _chunks(self, n):
        return [(s, min(n, s + self.max_batch)) for s in range(0, n, self.max_batch)]

    def _handles(self):
        """this engine and its lanes: what a setter reaches and ``check_async`` asks"""
        return [self] + (self._lanes or [])

    def _encode(self, n: int, call) -> torch.Tensor:
        """What the encode entries share once their input is checked and on the device: the fp32 [n, P] output and ``call(engine, a,
        b, out)`` over the chunks (``_run_chunks``)."""
        out = torch.empty((n, self.cfg.projection_dim), dtype=torch.float32, device=self.device)
        self._run_chunks(n, call, out)
        return out

    def encode_image(self, pixels: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """fp32 [B,3,H,W] (any device) -> fp32 [B,P] on the GPU."""
        ih, iw = self.image_hw
        if pixels.dim() != 4 or pixels.shape[1] != 3 or pixels.shape[2] != ih or pixels.shape[3] != iw:
            raise ValueError(f"Input image size ({tuple(pixels.shape)}) doesn't match model ([B,3,{ih},{iw}]).")
        with torch.cuda.device(self.device):
            px = pixels.to(device=self.device, dtype=torch.float32).contiguous()
            return self._encode(px.shape[0], lambda e, a, b, out: _lib.check(
                e.lib.plipmi_encode_image(e._h, _ptr(px[a:b]), b - a, _ptr(out[a:b]), int(normalize), e._stream()), "plipmi_encode_image"))

    def encode_image_u8(self, tiles: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """uint8 [B,H,W,3] RGB tiles already at the model resolution -> fp32 [B,P]; the CLIP
        normalisation is fused into the patch unfold on the GPU."""
        ih, iw = self.image_hw
        if tiles.dtype != torch.uint8 or tiles.dim() != 4 or tuple(tiles.shape[1:]) != (ih, iw, 3):
            raise ValueError(f"tiles must be uint8 [B,{ih},{iw},3], got {tiles.dtype} {tuple(tiles.shape)}")
        with torch.cuda.device(self.device):
            t = tiles.to(device=self.device).contiguous()
            return self._encode(t.shape[0], lambda e, a, b, out: _lib.check(
                e.lib.plipmi_encode_image_u8(e._h, _ptr(t[a:b]), b - a, _ptr(out[a:b]), int(normalize), e._stream()), "plipmi_encode_image_u8"))

    def encode_text(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                    normalize: bool = False, eos_token_id: Optional[int] = None) -> torch.Tensor:
        """int [B,ctx] token ids -> fp32 [B,P] on the GPU."""
        cfg = self.cfg
        if input_ids.dim() != 2 or input_ids.shape[1] != cfg.context_length:
            raise ValueError(f"input_ids must be [B,{cfg.context_length}], got {tuple(input_ids.shape)} "
                             "(pad/truncate to the context length like the reference, plip.py:58)")
        if input_ids.device.type == "cpu" and input_ids.numel():
            lo, hi = int(input_ids.min()), int(input_ids.max())
            if lo < 0 or hi >= cfg.vocab_size:
                raise IndexError(f"token id out of range [0,{cfg.vocab_size}): min {lo}, max {hi}")
        # device-resident ids are range-checked BY the embedding kernel; the outcome is known once that work has run:
        # check_async() after a synchronisation, or the next encode_text on this engine, raises IndexError
        # (PLIPMI_ERR_TOKEN_ID) -- also from a later chunk of THIS call when B > max_batch: the rows written so far are
        # then not to be used.  Image-side calls never report it.
        eos = cfg.eos_token_id if eos_token_id is None else int(eos_token_id)
        with torch.cuda.device(self.device):
            ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
            mask = None if attention_mask is None else attention_mask.to(device=self.device, dtype=torch.int64).contiguous()
            for other in self._lanes or []:       # an id a clone's embedding kernel flagged is this engine's to report
                if self.lib.plipmi_check_async(other._h) != 0:
                    raise IndexError(_lib.last_error())
            return self._encode(ids.shape[0], lambda e, a, b, out: _lib.check(
                e.lib.plipmi_encode_text(e._h, _ptr(ids[a:b]), _ptr(None if mask is None else mask[a:b]), b - a, eos, _ptr(out[a:b]),
                                         int(normalize), e._stream()), "plipmi_encode_text"))

    def check_async(self, synchronize: bool = True) -> None:
        """Raise IndexError if an earlier ``encode_text`` was given a token id outside the vocabulary -- the reference's
        embedding lookup raises there (plip.py:68; on a GPU at the next synchronisation, like here)."""
        if synchronize:
            torch.cuda.synchronize(self.device)
        for e in self._handles():
            if self.lib.plipmi_check_async(e._h) != 0:
                raise IndexError(_lib.last_error())

    def set_graph_batch(self, max_batch: int):
        """Batches of at most ``max_batch`` samples replay a captured hipGraph (0 = always launch eagerly)."""
        for e in self._handles():
            _lib.check(self.lib.plipmi_set_graph_batch(e._h, int(max_batch)), "plipmi_set_graph_batch")

    def set_latency_batch(self, max_batch: int):
        """Batches of at most ``max_batch`` samples (0 = never, the default) run their GEMMs on the split-K small-M kernel
        (include/plipmi.h plipmi_set_latency_batch): same arithmetic, fp32 summation order of its own."""
        for e in self._handles():
            _lib.check(self.lib.plipmi_set_latency_batch(e._h, int(max_batch)), "plipmi_set_latency_batch")

    def set_text_packing(self, on: bool):
        """Captions packed to their live rows (0 .. EOS): bit-identical text_embeds, cost proportional to the caption
        lengths instead of the padded 77 (include/plipmi.h plipmi_set_text_packing).  Off by default."""
        for e in self._handles():
            _lib.check(self.lib.plipmi_set_text_packing(e._h, int(bool(on))), "plipmi_set_text_packing")

    @contextlib.contextmanager
    def profile(self, result: list):
        """Per-kernel HIP-event timing of everything launched inside the block; rows are appended to ``result``."""
        _lib.check(self.lib.plipmi_profile_enable(self._h, 1), "plipmi_profile_enable")
        self._no_lanes += 1         # the rows are THIS handle's launches: every chunk of a call stays on it
        try:
            yield
        finally:
            self._no_lanes -= 1
            _lib.check(self.lib.plipmi_profile_enable(self._h, 0), "plipmi_profile_enable")
            rows = (_lib.KernelStat * 128)()
            n = C.c_int(0)
            _lib.check(self.lib.plipmi_profile_read(self._h, rows, 128, C.byref(n)), "plipmi_profile_read")
            for r in rows[: n.value]:
                result.append({"name": r.name.decode(), "calls": int(r.calls), "total_ms": float(r.total_ms),
                               "flops": float(r.flops), "bytes": float(r.bytes)})

    @property
    def logit_scale_exp(self) -> float:
        return math.exp(self.logit_scale)


_HEADS = {}


def heads_engine(device="cuda:0") -> Engine:
    """A handle for callers that only need the evaluation heads (l2_normalize / logits / topk / similarity_topk on
    embeddings they already hold -- reproducibility.evaluation): those entry points use no tower weights, so a
    minimal synthetic configuration is enough to own the scratch memory and the stream plumbing."""
    key = str(torch.device(device))
    if key not in _HEADS:
        cfg = get_config("tiny")
        _HEADS[key] = Engine(cfg, synthetic_state_dict(cfg, 0), device=device, dtype="f32", max_batch=1)
    return _HEADS[key]
