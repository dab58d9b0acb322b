"""ctypes binding of libplipmi.so (include/plipmi.h).  No fallback: if the HIP
extension is missing or fails to load, importing callers get a RuntimeError."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

# torch ships its own libamdhip64; imported FIRST so that libplipmi.so binds to the same HIP runtime instance
# (two runtimes in one process do not share devices/streams: plipmi_create then sees "no device")
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libplipmi.so")

F32, BF16, F16 = 0, 1, 2
# plipmi_config.flags
FLAG_SEPARATE_LAYERNORM, FLAG_DENSE_LAST_BLOCK, FLAG_PACK_CAPTIONS, FLAG_VALU_ATTENTION, FLAG_TEXT_TOWER_F16 = 1, 2, 4, 8, 16
FLAG_VISION_GELU, FLAG_TEXT_GELU = 32, 64     # a tower's MLP activation is the erf GELU (HF hidden_act "gelu"), not QuickGELU
VISION, TEXT = 0, 1


class Config(C.Structure):
    # first member = sizeof(Config) as this binding knows it (plipmi_create copies that many bytes: the struct may grow)
    _fields_ = [(n, C.c_int32) for n in (
        "struct_size", "image_size", "patch_size", "v_width", "v_layers", "v_heads", "v_mlp", "vocab_size",
        "context_length", "t_width", "t_layers", "t_heads", "t_mlp", "projection_dim")] + [
        ("layer_norm_eps", C.c_float), ("compute_dtype", C.c_int32), ("max_batch", C.c_int32), ("flags", C.c_int32),
        ("graph_batch", C.c_int32), ("text_f16_layers", C.c_int32), ("pass_batch", C.c_int32)]


_LAYER_FIELDS = ("ln1_w", "ln1_b", "q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "o_w", "o_b",
                 "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")


class LayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _LAYER_FIELDS]


class Weights(C.Structure):
    _fields_ = [
        ("v_class_embedding", C.c_void_p), ("v_patch_weight", C.c_void_p), ("v_pos_embedding", C.c_void_p),
        ("v_pre_ln_w", C.c_void_p), ("v_pre_ln_b", C.c_void_p), ("v_post_ln_w", C.c_void_p),
        ("v_post_ln_b", C.c_void_p), ("visual_projection", C.c_void_p), ("v_layers", C.POINTER(LayerWeights)),
        ("t_token_embedding", C.c_void_p), ("t_pos_embedding", C.c_void_p), ("t_final_ln_w", C.c_void_p),
        ("t_final_ln_b", C.c_void_p), ("text_projection", C.c_void_p), ("t_layers", C.POINTER(LayerWeights)),
    ]


# which tensor of an HF CLIP state dict each pointer is: the members of Weights, and the members ln1_w .. fc2_b of LayerWeights by
# their stem (under <tower>.encoder.layers.<i>.<name>.weight / .bias)
WEIGHT_KEYS = {
    "v_class_embedding": "vision_model.embeddings.class_embedding", "v_patch_weight": "vision_model.embeddings.patch_embedding.weight",
    "v_pos_embedding": "vision_model.embeddings.position_embedding.weight", "v_pre_ln_w": "vision_model.pre_layrnorm.weight",
    "v_pre_ln_b": "vision_model.pre_layrnorm.bias", "v_post_ln_w": "vision_model.post_layernorm.weight",
    "v_post_ln_b": "vision_model.post_layernorm.bias", "visual_projection": "visual_projection.weight",
    "t_token_embedding": "text_model.embeddings.token_embedding.weight", "t_pos_embedding": "text_model.embeddings.position_embedding.weight",
    "t_final_ln_w": "text_model.final_layer_norm.weight", "t_final_ln_b": "text_model.final_layer_norm.bias",
    "text_projection": "text_projection.weight"}
LAYER_KEYS = {"ln1": "layer_norm1", "ln2": "layer_norm2", "q": "self_attn.q_proj", "k": "self_attn.k_proj",
              "v": "self_attn.v_proj", "o": "self_attn.out_proj", "fc1": "mlp.fc1", "fc2": "mlp.fc2"}


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("calls", C.c_int64), ("total_ms", C.c_double),
                ("flops", C.c_double), ("bytes", C.c_double)]


PROBE_MAX_K = 64     # include/plipmi.h PLIPMI_PROBE_MAX_K
TOKEN_SIM_MAX_C = 64   # include/plipmi.h PLIPMI_TOKEN_SIM_MAX_C


class ProbeInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("evaluations", C.c_int32), ("converged", C.c_int32), ("reserved", C.c_int32),
                ("grad_norm", C.c_double), ("loss", C.c_double * PROBE_MAX_K)]


KMEANS_MAX_K = 4096    # include/plipmi.h PLIPMI_KMEANS_MAX_K
KMEANS_METRICS = {"euclidean": 0, "cosine": 1}   # PLIPMI_KMEANS_EUCLIDEAN / PLIPMI_KMEANS_COSINE


class KMeansInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("relocations", C.c_int32), ("reserved", C.c_int32),
                ("inertia", C.c_double), ("center_shift", C.c_double)]


BAG_MAX_K, BAG_MAX_KS, BAG_MAX_CLASSES = 1024, 8, 64    # include/plipmi.h PLIPMI_BAG_MAX_K / _KS / _CLASSES

_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
# kernel-level test entries and A/B hooks (include/plipmi_test.h): tests/, tools/ and bench.py's side fields only
TEST_SYMBOLS = {
    "plipmi_debug_hidden": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp]),
    "plipmi_gemm_nt": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp]),
    "plipmi_gemm_variant_name": (C.c_char_p, [_i]),
    "plipmi_test_force_gemm_tile": (_i, [_i]),
    "plipmi_test_remap_gemm_tile": (_i, [_i, _i]),
    "plipmi_test_fused_qkv_attention": (_i, [_i]),
    "plipmi_test_patch_gather": (_i, [_i]),
    "plipmi_test_reset_hooks": (None, []),
    "plipmi_gemm_variant_built": (_i, [_i, _i]),
    "plipmi_recode_planes": (_i, [_vp, _vp, C.c_size_t, _i, _i, _i, _vp]),
    "plipmi_gemm_nt_ln": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp]),
    "plipmi_gemm_nt_ld": (_i, [_i, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _f, _vp, _vp]),
    "plipmi_gemm_nt_traced": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp]),
    "plipmi_attention": (_i, [_i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "plipmi_qkv_attention": (_i, [_i, _vp, _vp, _vp, _vp, _i, _f, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "plipmi_resample_pos": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "plipmi_probe_loss_grad": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    "plipmi_attention_probs": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "plipmi_attention_pooled_rows": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "plipmi_attention_rollout_step": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "plipmi_layernorm": (_i, [_vp, C.c_size_t, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "plipmi_layernorm_emit": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "plipmi_fold_ln": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "plipmi_text_embed_emit": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "plipmi_pool_rows": (_i, [_i, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _f, _vp, _i, _i, _vp, _vp]),
    "plipmi_pool_gather": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "plipmi_head_gemm": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "plipmi_resize_ragged_tables": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "plipmi_unfold_patches": (_i, [_i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "plipmi_cls_rows": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "plipmi_gemm_patch": (_i, [_i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "plipmi_gemm_patch_gather": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "plipmi_gemm_nt_ln_rows": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "plipmi_attention_packed": (_i, [_i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "plipmi_gemm_nt_gelu": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp]),
    "plipmi_attention_hd": (_i, [_i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "plipmi_attention_probs_hd": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "plipmi_attention_pooled_rows_hd": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "plipmi_attention_rollout_step_hd": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "plipmi_token_scores": (_i, [_vp, _i, _i, _vp, _i, _f, _i, _vp, _vp]),
    "plipmi_softmax_loss_grad": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _f, _vp, _vp, _vp, _vp]),
    "plipmi_kmeans_update": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "plipmi_stain_percentile": (_i, [_vp, _vp, _i, _i, C.POINTER(C.c_double), _i, _vp, _vp, _vp, _vp]),
}
# every symbol include/plipmi.h declares (the product interface): (restype, argtypes)
SYMBOLS = {
    "plipmi_create": (_i, [C.POINTER(Config), C.POINTER(Weights), _vp, C.POINTER(_vp)]),
    "plipmi_destroy": (None, [_vp]),
    "plipmi_version": (_i, []),
    "plipmi_last_error": (C.c_char_p, []),
    "plipmi_device_name": (C.c_char_p, [_vp]),
    "plipmi_encode_image": (_i, [_vp, _vp, _i, _vp, _i, _vp]),
    "plipmi_encode_image_u8": (_i, [_vp, _vp, _i, _vp, _i, _vp]),
    "plipmi_encode_text": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp]),
    "plipmi_check_async": (_i, [_vp]),
    "plipmi_set_latency_batch": (_i, [_vp, _i]),
    "plipmi_set_graph_batch": (_i, [_vp, _i]),
    "plipmi_get_pass_batch": (_i, [_vp]),
    "plipmi_clone": (_i, [_vp, C.POINTER(_vp)]),
    "plipmi_clone_resolution": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "plipmi_streams_overlap": (_i, [_vp, _vp, _vp, C.POINTER(_f)]),
    "plipmi_l2_normalize": (_i, [_vp, _vp, _i, _i, _vp]),
    "plipmi_logits": (_i, [_vp, _vp, _i, _vp, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "plipmi_topk": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "plipmi_resize_crop_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "plipmi_resize_crop_u8_ragged": (_i, [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, C.c_size_t, _vp, _vp]),
    "plipmi_resize_ragged_workspace": (C.c_size_t, [_vp, _i, _i, _i]),
    "plipmi_region_select": (_i, [_vp, _vp, _i, _i, C.c_int64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "plipmi_region_gather": (_i, [_vp, _vp, _i, _i, C.c_int64, _i, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    "plipmi_warp_u8": (_i, [_vp, _vp, _i, _i, _i, C.c_int64, C.c_int64, _vp, _vp, _i, _i, _i, C.c_uint32, _vp, _vp]),
    "plipmi_similarity_topk": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "plipmi_set_text_packing": (_i, [_vp, _i]),
    "plipmi_tower_shape": (_i, [_vp, _i, C.POINTER(C.c_int32)]),
    "plipmi_encode_tower_outputs": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "plipmi_encode_attention_summary": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "plipmi_encode_token_similarity": (_i, [_vp, _vp, _i, _vp, _i, _f, _i, _vp, _vp, _vp]),
    "plipmi_probe_fit": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _f, _i, _f, _vp, C.POINTER(ProbeInfo), _vp]),
    "plipmi_probe_predict": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "plipmi_softmax_fit": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _f, _i, _f, _vp, C.POINTER(ProbeInfo), _vp]),
    "plipmi_kmeans_seed": (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(C.c_double), _vp, _vp, _vp]),
    "plipmi_kmeans_assign": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "plipmi_kmeans_fit": (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.c_double, _vp, _vp, _vp, _vp, _vp, C.POINTER(KMeansInfo), _vp]),
    "plipmi_stain_workspace": (C.c_size_t, [_i, _i, _i, _i]),
    "plipmi_stain_fit": (_i, [_vp, _vp, _i, _i, _i, C.c_int64, C.c_int64, _i, _i, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, _vp]),
    "plipmi_stain_apply": (_i, [_vp, _vp, _i, _i, _i, C.c_int64, C.c_int64, _vp, _i, _vp, C.c_double, _vp, _vp, _vp]),
    "plipmi_bag_workspace": (C.c_size_t, [_i, _i, _i, _i]),
    "plipmi_bag_topk_pool": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _f, C.POINTER(C.c_int32), _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "plipmi_bag_pool_scores": (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, _i, C.POINTER(C.c_int32), _i, _vp, _vp, _vp, _vp, _vp]),
    "plipmi_bag_mean": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "plipmi_profile_enable": (_i, [_vp, _i]),
    "plipmi_profile_read": (_i, [_vp, C.POINTER(KernelStat), _i, C.POINTER(_i)]),
}

_lib = None


def load():
    """Load libplipmi.so once.  Fails loudly -- there is no CPU/eager fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP engine is not built. Run `python -m plip_amd.build` "
            "(needs hipcc / ROCm). plip_amd has no fallback path.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise RuntimeError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in {**SYMBOLS, **TEST_SYMBOLS}.items():
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load().plipmi_last_error().decode(errors="replace")


class PlipmiError(RuntimeError):
    pass


ERR_TOKEN_ID = 5     # include/plipmi.h PLIPMI_ERR_TOKEN_ID
ERR_NOT_CONVERGED = 6   # include/plipmi.h PLIPMI_ERR_NOT_CONVERGED (plipmi_probe_fit; Engine.probe_fit reports it in its info)


def check(rc: int, what: str) -> None:
    if rc == ERR_TOKEN_ID:      # what the reference's embedding lookup raises on an out-of-range id (plip.py:68)
        raise IndexError(f"{what}: {last_error()}")
    if rc != 0:
        raise PlipmiError(f"{what} failed (code {rc}): {last_error()}")


# ---- Python values -> arguments of the entries ----------------------------------------------------------------------------------
_DTYPES = {"fp32": F32, "f32": F32, "float32": F32, torch.float32: F32,
           "bf16": BF16, "bfloat16": BF16, torch.bfloat16: BF16,
           # IEEE half operands: same matrix-core rate as bf16, 8x smaller operand rounding; the reference's own GPU dtype
           "f16": F16, "fp16": F16, "float16": F16, "half": F16, torch.float16: F16}
_TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}


def _code(dt) -> int:
    return _DTYPES[dt]


def _tower_code(tower: str) -> int:
    if tower not in ("vision", "text"):
        raise ValueError(f"tower must be 'vision' or 'text', got {tower!r}")
    return VISION if tower == "vision" else TEXT


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream_ptr(device):
    """the hipStream_t argument of an entry: the caller's current stream on ``device``"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
