"""Shared by tests/test_token_similarity_host.py, tests/test_gpu_token_similarity.py and tools/make_token_similarity_golden.py: the plain
restatement of what include/plipmi.h plipmi_encode_token_similarity defines, written from the definition and not from the kernels.

    E   = LayerNorm(X; ln_w, ln_b, eps) . proj^T                      on every row of X [..., D]  -> [..., P]
    sim = scale * <E / |E|, T / |T|>  (softmax: its softmax over C)                                 -> [..., C]

``dtype`` float64 is the reference; float32 is the plain unfused CPU computation the fp32 tolerances are measured on
(tests/small_kernel_refs.py ``fp32_bound``)."""
import numpy as np
import torch

from small_kernel_refs import layer_norm

F64 = torch.float64


def _t(a, dtype):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dtype)


def scores_ref(E, T, scale=1.0, softmax=False, dtype=F64):
    """the score part alone: E [..., P], T [C, P] (rows of any norm, no epsilon) -> [..., C] in ``dtype``"""
    E, T = _t(E, dtype), _t(T, dtype)
    En = E / torch.sqrt((E * E).sum(-1, keepdim=True))
    Tn = T / torch.sqrt((T * T).sum(-1, keepdim=True))
    s = (En @ Tn.transpose(0, 1)) * scale
    if softmax:
        e = torch.exp(s - s.amax(-1, keepdim=True))
        s = e / e.sum(-1, keepdim=True)
    return s


def head_ref(X, ln_w, ln_b, eps, proj, T, scale=1.0, softmax=False, dtype=F64):
    """-> (token_embeds [..., P], similarity [..., C]) of the encoder output X [..., D] in ``dtype``; proj [P, D] (the HF layout)"""
    E = layer_norm(_t(X, dtype), _t(ln_w, dtype), _t(ln_b, dtype), eps, dtype) @ _t(proj, dtype).transpose(0, 1)
    return E, scores_ref(E, T, scale, softmax, dtype)


def head_weights(sd):
    """(post_layernorm weight, bias, visual_projection weight [P, Dv]) of an HF CLIP state dict, as float32 numpy"""
    get = lambda k: np.asarray(sd[k].float().numpy() if torch.is_tensor(sd[k]) else sd[k], dtype=np.float32)
    return get("vision_model.post_layernorm.weight"), get("vision_model.post_layernorm.bias"), get("visual_projection.weight")


# fixture name -> (golden case whose weights, captions and logits it uses, images of that case or None for other pixels, (B, S, P, C))
FIXTURES = {
    "token_similarity_tiny": ("tiny_b6", 6, (6, 17, 64, 6)),
    "token_similarity_tinyp4": ("tinyp4_b3", 3, (3, 257, 64, 3)),
    "token_similarity_vitb32_b2": ("vitb32_b4", 2, (2, 50, 512, 4)),
    "token_similarity_vitb32_160": ("vitb32_b4", None, (2, 26, 512, 4)),
}
