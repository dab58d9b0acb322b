"""Host side of the attention head sizes other than 64: the presets, where a vision head count comes from for an OpenAI-layout state dict,
what ``PlipConfig.validate`` accepts and refuses, and that header, binding and library agree on the new kernel-level entries.  No GPU."""
import os
import re

import numpy as np
import pytest

from plip_amd import weights as W
from plip_amd.config import MAX_HEAD_DIM, PRESETS, from_hf_config, get_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD_ENTRIES = ("plipmi_attention_hd", "plipmi_attention_probs_hd", "plipmi_attention_pooled_rows_hd", "plipmi_attention_rollout_step_hd")


def test_presets_of_the_two_open_clip_towers():
    h, g = PRESETS["ViT-H/14"], PRESETS["ViT-g/14"]
    assert (h.v_width, h.v_layers, h.v_heads, h.v_mlp, h.patch_size, h.head_dim) == (1280, 32, 16, 5120, 14, 80)
    assert (g.v_width, g.v_layers, g.v_heads, g.v_mlp, g.patch_size, g.head_dim) == (1408, 40, 16, 6144, 14, 88)
    for cfg in (h, g):
        assert (cfg.t_width, cfg.t_layers, cfg.t_heads, cfg.t_mlp, cfg.t_head_dim) == (1024, 24, 16, 4096, 64)
        assert (cfg.projection_dim, cfg.image_size, cfg.v_tokens, cfg.context_length, cfg.vocab_size) == (1024, 224, 257, 77, 49408)
        cfg.validate()
        cfg.with_hidden_act("gelu").validate()          # the published checkpoints' activation: from config.json or hidden_act=
    # every preset that existed keeps heads of 64
    for name, cfg in PRESETS.items():
        if name not in ("ViT-H/14", "ViT-g/14"):
            assert (cfg.head_dim, cfg.t_head_dim) == (64, 64), name
    # the FLOP model follows the width, so it needs no head size: 4 S^2 D per block for the two attention products
    assert h.image_flops() > 3.0e11


def _openai_shapes(cfg):
    """shape-only stand-in for an OpenAI-layout state dict of ``cfg``: arrays of zero strides, no memory behind them"""
    def z(*shape):
        return np.broadcast_to(np.float32(0), shape)
    sd = {"visual.conv1.weight": z(cfg.v_width, 3, cfg.patch_size, cfg.patch_size), "visual.positional_embedding": z(cfg.v_tokens, cfg.v_width),
          "visual.proj": z(cfg.v_width, cfg.projection_dim), "ln_final.weight": z(cfg.t_width),
          "positional_embedding": z(cfg.context_length, cfg.t_width), "token_embedding.weight": z(cfg.vocab_size, cfg.t_width),
          "text_projection": z(cfg.t_width, cfg.projection_dim)}
    for l in range(cfg.v_layers):
        sd[f"visual.transformer.resblocks.{l}.mlp.c_fc.weight"] = z(cfg.v_mlp, cfg.v_width)
    for l in range(cfg.t_layers):
        sd[f"transformer.resblocks.{l}.mlp.c_fc.weight"] = z(cfg.t_mlp, cfg.t_width)
    return sd


@pytest.mark.parametrize("arch,heads,head", [("ViT-H/14", 16, 80), ("ViT-g/14", 16, 88), ("ViT-B/32", 12, 64), ("ViT-L/14", 16, 64)])
def test_vision_heads_of_an_openai_layout_state_dict(arch, heads, head):
    """FAILS WITHOUT THE FEATURE: ``width // 64`` made ViT-H/14 20 heads of 64 -- it loaded, ran and gave wrong embeddings"""
    cfg = get_config(arch)
    got = W.config_from_openai_state_dict(_openai_shapes(cfg))
    assert (got.v_heads, got.head_dim) == (heads, head)
    assert (got.v_width, got.v_layers, got.v_mlp, got.patch_size, got.t_width, got.t_heads, got.t_layers) == \
        (cfg.v_width, cfg.v_layers, cfg.v_mlp, cfg.patch_size, cfg.t_width, cfg.t_heads, cfg.t_layers)
    got.validate()


def test_the_head_table_is_keyed_by_width_and_depth():
    assert W.OPENCLIP_VISION_HEADS == {(1280, 32): 16, (1408, 40): 16, (1664, 48): 16}
    # a 1280-wide tower of another depth is nobody's published model: OpenAI's rule
    odd = get_config("ViT-H/14").replace(v_layers=4)
    assert W.config_from_openai_state_dict(_openai_shapes(odd)).v_heads == 20


def test_validate_accepts_and_refuses_by_the_rule():
    tiny = get_config("tiny")
    assert MAX_HEAD_DIM == {"v": 128, "t": 120}
    for head in range(64, 129, 8):                                   # 16 heads of `head`: the width is a multiple of 128
        cfg = tiny.replace(v_width=16 * head, v_heads=16)
        assert cfg.head_dim == head
        cfg.validate()
        if head <= 120:
            tiny.replace(t_width=16 * head, t_heads=16).validate()
    refused = {"vision head 32": dict(v_width=128, v_heads=4), "vision head 56": dict(v_width=896, v_heads=16),
               "vision head 136": dict(v_width=1088, v_heads=8), "vision head 100": dict(v_width=1600, v_heads=16),
               "vision head 192": dict(v_width=768, v_heads=4), "text head 128": dict(t_width=256, t_heads=2),
               "text head 32": dict(t_width=128, t_heads=4), "no vision heads": dict(v_heads=0), "negative text heads": dict(t_heads=-2),
               "width not a multiple of heads": dict(v_width=640, v_heads=12)}
    for what, changes in refused.items():
        with pytest.raises(ValueError, match="head_dim|must be a multiple of"):
            tiny.replace(**changes).validate()
    # an HF config of such a tower passes through from_hf_config unchanged
    from test_gelu_host import _hf_dict
    hd80 = tiny.replace(v_width=640, v_heads=8, v_mlp=1280)
    assert from_hf_config(_hf_dict(hd80)) == hd80


def test_header_binding_and_library_agree_on_the_new_entries():
    from plip_amd import _lib
    header = open(os.path.join(ROOT, "include", "plipmi_test.h")).read()
    product = open(os.path.join(ROOT, "include", "plipmi.h")).read()
    lib = _lib.load()
    for name in HD_ENTRIES:
        m = re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert name in _lib.TEST_SYMBOLS and name not in _lib.SYMBOLS and hasattr(lib, name)
        assert not re.search(r"\b%s\s*\(" % name, product)                       # test entries: no product signature changed
        res, argtypes = _lib.TEST_SYMBOLS[name]
        assert len(argtypes) == len(args), (name, args)
        assert sum(a == "int head_dim" for a in args) == 1
        old = name[:-3]                                                          # the entry without the argument keeps its signature
        assert len(_lib.TEST_SYMBOLS[old][1]) == len(argtypes) - 1
        i = args.index("int head_dim")
        assert _lib.TEST_SYMBOLS[old][1] == argtypes[:i] + argtypes[i + 1:]
    # the wrappers pass head_dim through and the old ones do not take it
    import inspect

    from plip_amd import kernel_entries as K
    for fn in (K.attention, K.attention_probs, K.attention_pooled_rows, K.attention_rollout_step):
        assert inspect.signature(fn).parameters["head_dim"].default is None


def test_entries_refuse_a_bad_head_size_before_any_launch():
    """argument checks run on the host: no GPU is needed to be refused"""
    import ctypes as C

    from plip_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(16)       # never dereferenced: refused first
    for head in (0, 32, 60, 100, 136):
        assert lib.plipmi_attention_hd(_lib.BF16, 1, one, one, 1, 4, 1, head, 0, None, None) != 0
        assert "head_dim" in _lib.last_error()
        assert lib.plipmi_attention_probs_hd(_lib.BF16, one, one, 1, 4, 1, head, 0, None, None) != 0 and "head_dim" in _lib.last_error()
        assert lib.plipmi_attention_pooled_rows_hd(_lib.BF16, one, one, one, 1, 4, 1, head, 0, None, None) != 0 and "head_dim" in _lib.last_error()
        assert lib.plipmi_attention_rollout_step_hd(_lib.BF16, one, None, one, 1, 4, 1, head, 0, None, None) != 0 and "head_dim" in _lib.last_error()
