"""Host side of the exact-GELU towers (HF ``hidden_act="gelu"``): where the activation is read, overridden and refused, how it reaches
``plipmi_config.flags``, and that header, binding and library agree on the new bits and the new kernel-level entry.  No GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from plip_amd import weights as W
from plip_amd.config import PRESETS, PlipConfig, from_hf_config, get_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hf_dict(cfg, v_act=None, t_act=None):
    """an HF CLIPConfig dict written here (not helpers.hf_config_dict): ``hidden_act`` present only where given"""
    d = {"projection_dim": cfg.projection_dim, "logit_scale_init_value": cfg.logit_scale_init,
         "text_config": {"vocab_size": cfg.vocab_size, "hidden_size": cfg.t_width, "intermediate_size": cfg.t_mlp,
                         "num_hidden_layers": cfg.t_layers, "num_attention_heads": cfg.t_heads,
                         "max_position_embeddings": cfg.context_length, "eos_token_id": cfg.eos_token_id, "bos_token_id": cfg.bos_token_id},
         "vision_config": {"hidden_size": cfg.v_width, "intermediate_size": cfg.v_mlp, "num_hidden_layers": cfg.v_layers,
                           "num_attention_heads": cfg.v_heads, "image_size": cfg.image_size, "patch_size": cfg.patch_size,
                           "layer_norm_eps": cfg.layer_norm_eps}}
    if v_act is not None:
        d["vision_config"]["hidden_act"] = v_act
    if t_act is not None:
        d["text_config"]["hidden_act"] = t_act
    return d


def test_from_hf_config_reads_defaults_and_rejects_hidden_act():
    cfg = get_config("tiny")
    got = from_hf_config(_hf_dict(cfg))
    assert (got.v_hidden_act, got.t_hidden_act) == ("quick_gelu", "quick_gelu") and got == cfg     # absent = HF's default
    for v, t in (("gelu", "gelu"), ("gelu", "quick_gelu"), ("quick_gelu", "gelu"), ("gelu", None), (None, "gelu")):
        got = from_hf_config(_hf_dict(cfg, v, t))
        assert (got.v_hidden_act, got.t_hidden_act) == (v or "quick_gelu", t or "quick_gelu")
        assert got.replace(v_hidden_act="quick_gelu", t_hidden_act="quick_gelu") == cfg            # nothing else moved
    for bad in ("gelu_new", "gelu_pytorch_tanh", "relu", "GELU"):
        with pytest.raises(ValueError, match="v_hidden_act"):
            from_hf_config(_hf_dict(cfg, bad, None))
        with pytest.raises(ValueError, match="t_hidden_act"):
            from_hf_config(_hf_dict(cfg, "gelu", bad))


def test_from_hf_config_reads_a_transformers_clipconfig():
    transformers = pytest.importorskip("transformers")
    from oracle.hf_reference import hf_config
    hc = hf_config(get_config("tiny"))
    assert from_hf_config(hc).v_hidden_act == "quick_gelu"
    hc.vision_config.hidden_act = "gelu"
    got = from_hf_config(hc)
    assert (got.v_hidden_act, got.t_hidden_act) == ("gelu", "quick_gelu")
    assert type(transformers.activations.ACT2FN["gelu"]).__name__ == "GELUActivation"       # the erf form, not the tanh one


def test_config_fields_are_appended_validated_and_presets_unchanged():
    import dataclasses
    names = [f.name for f in dataclasses.fields(PlipConfig)]
    assert names[-2:] == ["v_hidden_act", "t_hidden_act"] and names[0] == "image_size" and names[-3] == "logit_scale_init"
    for name, cfg in PRESETS.items():
        assert (cfg.v_hidden_act, cfg.t_hidden_act) == ("quick_gelu", "quick_gelu"), name
        cfg.validate()
    assert PRESETS["ViT-B/32"] == PlipConfig()
    ok = get_config("tiny").replace(v_hidden_act="gelu", t_hidden_act="gelu")
    ok.validate()
    for field in ("v_hidden_act", "t_hidden_act"):
        with pytest.raises(ValueError, match=field):
            get_config("tiny").replace(**{field: "gelu_new"}).validate()
    tiny = get_config("tiny")
    assert tiny.with_hidden_act(None) is tiny
    assert tiny.with_hidden_act("gelu") == ok
    assert tiny.with_hidden_act(("gelu", "quick_gelu")) == tiny.replace(v_hidden_act="gelu")
    assert ok.with_hidden_act((None, "quick_gelu")) == tiny.replace(v_hidden_act="gelu")
    with pytest.raises(ValueError, match="t_hidden_act"):
        tiny.with_hidden_act(("gelu", "swish"))


def test_load_checkpoint_reads_hidden_act_from_an_hf_directory(tmp_path):
    from safetensors.numpy import save_file
    cfg = get_config("tiny")
    sd = W.synthetic_state_dict(cfg, 0)
    save_file({k: np.ascontiguousarray(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(_hf_dict(cfg, "gelu", "gelu")))
    sd2, got = W.load_checkpoint(str(tmp_path))
    assert (got.v_hidden_act, got.t_hidden_act) == ("gelu", "gelu") and got.with_hidden_act("quick_gelu") == cfg
    np.testing.assert_array_equal(sd2["visual_projection.weight"], sd["visual_projection.weight"])
    # the keyword overrides the file, per tower; an explicit architecture keeps the file's activation
    assert W.load_checkpoint(str(tmp_path), hidden_act="quick_gelu")[1] == cfg
    assert W.load_checkpoint(str(tmp_path), hidden_act=(None, "quick_gelu"))[1] == cfg.replace(v_hidden_act="gelu")
    assert W.load_checkpoint(str(tmp_path), arch="tiny")[1] == got
    (tmp_path / "config.json").write_text(json.dumps(_hf_dict(cfg, "gelu", "gelu_new")))
    with pytest.raises(ValueError, match="t_hidden_act"):
        W.load_checkpoint(str(tmp_path))
    (tmp_path / "config.json").write_text(json.dumps(_hf_dict(cfg)))
    assert W.load_checkpoint(str(tmp_path))[1] == cfg


def test_hidden_act_override_for_an_openai_format_state_dict(tmp_path):
    import torch
    cfg = get_config("tiny")
    oa = W.to_openai_state_dict(W.synthetic_state_dict(cfg, 0), cfg)
    _, plain = W.normalize_state_dict(oa)
    assert (plain.v_hidden_act, plain.t_hidden_act) == ("quick_gelu", "quick_gelu")      # a state dict carries no activation
    _, got = W.normalize_state_dict(oa, hidden_act="gelu")
    assert (got.v_hidden_act, got.t_hidden_act) == ("gelu", "gelu") and got.with_hidden_act("quick_gelu") == plain
    _, got = W.normalize_state_dict(oa, hidden_act=("quick_gelu", "gelu"))
    assert (got.v_hidden_act, got.t_hidden_act) == ("quick_gelu", "gelu")
    with pytest.raises(ValueError, match="hidden_act"):
        W.normalize_state_dict(oa, hidden_act="tanh")
    path = str(tmp_path / "open_clip.pt")
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in oa.items()}, path)
    assert W.load_checkpoint(path, hidden_act="gelu")[1] == plain.with_hidden_act("gelu")
    assert W.load_checkpoint(path)[1] == plain


def test_constructors_take_hidden_act():
    """PlipModel.from_* / PLIP / the reproducibility factory hand the keyword on (signatures: no GPU here to build an engine)"""
    import inspect

    from plip_amd.model import PlipModel
    from plip_amd.plip import PLIP
    for fn in (PlipModel.from_pretrained, PlipModel.from_state_dict, PlipModel.from_synthetic, PLIP.__init__, W.load_checkpoint,
               W.normalize_state_dict):
        p = inspect.signature(fn).parameters
        assert "hidden_act" in p and p["hidden_act"].default is None, fn
    src = open(os.path.join(ROOT, "plip_amd", "reproducibility", "embedders.py")).read()
    assert 'hidden_act=getattr(args, "hidden_act", None)' in src


def test_activation_flags_of_the_four_tower_combinations():
    from plip_amd import _lib
    from plip_amd.engine import _activation_flags
    tiny = get_config("tiny")
    assert (_lib.FLAG_VISION_GELU, _lib.FLAG_TEXT_GELU) == (32, 64)
    want = {("quick_gelu", "quick_gelu"): 0, ("gelu", "quick_gelu"): 32, ("quick_gelu", "gelu"): 64, ("gelu", "gelu"): 96}
    for (v, t), bits in want.items():
        assert _activation_flags(tiny.replace(v_hidden_act=v, t_hidden_act=t)) == bits
    for cfg in PRESETS.values():
        assert _activation_flags(cfg) == 0
    with pytest.raises(ValueError, match="v_hidden_act"):
        _activation_flags(tiny.replace(v_hidden_act="relu"))


def test_engine_surface_is_unchanged():
    import inspect

    from plip_amd.engine import Engine
    params = list(inspect.signature(Engine.__init__).parameters)
    assert "hidden_act" not in params and not any("gelu" in p for p in params)
    assert not [n for n in dir(Engine) if "gelu" in n.lower() or "hidden_act" in n]


def test_header_binding_and_library_agree_on_the_gelu_bits_and_entry():
    from plip_amd import _lib
    from plip_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "plipmi.h")).read()
    flags = dict((n, int(v)) for n, v in re.findall(r"\b(PLIPMI_FLAG_[A-Z0-9_]+)\s*=\s*(\d+)", header))
    assert flags["PLIPMI_FLAG_VISION_GELU"] == _lib.FLAG_VISION_GELU == 32 and flags["PLIPMI_FLAG_TEXT_GELU"] == _lib.FLAG_TEXT_GELU == 64
    assert sorted(flags.values()) == [1, 2, 4, 8, 16, 32, 64]                    # one bit each, none reused
    assert re.search(r"#define PLIPMI_VERSION 412\b", header) and lib.plipmi_version() == 412
    assert C.sizeof(_lib.Config) == 21 * 4
    test_header = open(os.path.join(ROOT, "include", "plipmi_test.h")).read()
    m = re.search(r"int plipmi_gemm_nt_gelu\(([^)]*)\)", test_header)
    assert m and "plipmi_gemm_nt_gelu" in _lib.TEST_SYMBOLS and hasattr(lib, "plipmi_gemm_nt_gelu")
    args = [a.strip() for a in m.group(1).split(",")]
    res, argtypes = _lib.TEST_SYMBOLS["plipmi_gemm_nt_gelu"]
    assert res is C.c_int and len(args) == len(argtypes) == 14
    for a, t in zip(args, argtypes):
        assert t is (C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_int), a
    # epilogue numbers: the new kinds are appended, the old ones keep their values
    gemm_h = open(os.path.join(ROOT, "plip_amd", "csrc", "gemm.h")).read()
    epi = dict((n, int(v)) for n, v in re.findall(r"\b(EPI_[A-Z_]+)\s*=\s*(\d+)", gemm_h))
    assert epi == {"EPI_BIAS": 0, "EPI_BIAS_QGELU": 1, "EPI_BIAS_RESID": 2, "EPI_SCALE": 3, "EPI_PATCH": 4, "EPI_BIAS_LN": 5,
                   "EPI_QGELU_LN": 6, "EPI_RESID_EMIT": 7, "EPI_RESID_SPLIT": 8, "EPI_BIAS_GELU": 9, "EPI_GELU_LN": 10, "EPI_COUNT": 11}


def test_entry_refuses_bad_arguments_before_any_launch():
    """plipmi_gemm_nt_gelu's checks run before the first HIP call: they answer on a machine without a GPU too"""
    from plip_amd import _lib
    from plip_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(dtype, ln, variant, A=p, bias=p, stats=p, ns=2):
        return lib.plipmi_gemm_nt_gelu(dtype, ln, variant, 4, 128, 256, A, p, bias, stats, ns, 1e-5, p, None)

    for args, msg in ((dict(dtype=_lib.F32, ln=1, variant=-1), "16-bit"), (dict(dtype=_lib.BF16, ln=0, variant=-1, A=None), "null pointer"),
                      (dict(dtype=_lib.BF16, ln=0, variant=-1, bias=None), "null pointer"), (dict(dtype=_lib.F16, ln=1, variant=-2), "variant -2"),
                      (dict(dtype=_lib.BF16, ln=1, variant=-1, stats=None), "statistics"), (dict(dtype=_lib.BF16, ln=1, variant=-1, ns=3), "even"),
                      (dict(dtype=_lib.BF16, ln=2, variant=-1), "ln must be"), (dict(dtype=7, ln=0, variant=-1), "bad dtype"),
                      (dict(dtype=_lib.F32, ln=0, variant=-3), "variant -3")):
        assert call(**args) == 1, args                                   # PLIPMI_ERR_INVALID
        assert msg in _lib.last_error(), (args, _lib.last_error())
