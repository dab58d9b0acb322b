"""CPU-side checks of the per-token tower outputs: the output object's HF semantics, the buffer arithmetic of
plipmi_encode_tower_outputs, the C-ABI declaration and binding, and the probability kernel's resource usage."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tower_output_tuple_and_index_semantics():
    """HF BaseModelOutputWithPooling: to_tuple() keeps the fields that are set, in order; ints index that tuple, strs name a field"""
    from plip_amd.outputs import TowerOutput
    last, pooled = torch.zeros(2, 3, 4), torch.ones(2, 4)
    o = TowerOutput(last_hidden_state=last, pooler_output=pooled)
    assert o.to_tuple() == (last, pooled) and len(o) == 2 and o.keys() == ["last_hidden_state", "pooler_output"]
    assert o[0] is last and o[1] is pooled and o[-1] is pooled and o["pooler_output"] is pooled
    with pytest.raises(KeyError):
        o["attentions"]
    with pytest.raises(IndexError):
        o[2]
    att = (torch.zeros(2, 1, 3, 3), torch.zeros(2, 1, 3, 3))
    o = TowerOutput(last_hidden_state=last, pooler_output=pooled, attentions=att)
    assert o[2] is att and o.to_tuple()[2] is att and o["attentions"] is att and o.hidden_states is None
    hs = (last, last, last)
    o = TowerOutput(last, pooled, hs, att)
    assert o[2] is hs and o[3] is att and o[1:] == (pooled, hs, att) and list(o) == ["last_hidden_state", "pooler_output",
                                                                                     "hidden_states", "attentions"]


def test_plip_output_carries_tower_outputs():
    """CLIPOutput's text_model_output / vision_model_output come after loss, default None; to_tuple() appends their tuples"""
    from plip_amd.model import PlipOutput
    from plip_amd.outputs import TowerOutput
    a = torch.zeros(1)
    out = PlipOutput(a, a, a, a)
    assert out.loss is None and out.text_model_output is None and out.vision_model_output is None and len(out.to_tuple()) == 4
    names = list(PlipOutput.__dataclass_fields__)
    assert names[-3:] == ["loss", "text_model_output", "vision_model_output"]
    t = TowerOutput(a, a)
    out = PlipOutput(a, a, a, a, text_model_output=t, vision_model_output=TowerOutput(a, a, attentions=(a,)))
    assert out.to_tuple()[4] == (a, a) and out.to_tuple()[5] == (a, a, (a,))


def test_buffer_size_arithmetic():
    from plip_amd.config import get_config
    from plip_amd.outputs import tower_output_bytes
    b32 = get_config("ViT-B/32")
    # ViT-B/32 vision at bs = 256: 30.7 MB of probabilities per layer
    per_layer = tower_output_bytes(256, 50, b32.v_width, b32.v_heads, 1, False, False, False, True)["attentions"]
    assert per_layer == 256 * 12 * 50 * 50 * 4 == 30_720_000
    # ViT-L/14@336: 577 tokens, 24 blocks of 16 heads -- 511 MB of attentions per image
    l14 = get_config("ViT-L/14@336px")
    S = (l14.image_size // l14.patch_size) ** 2 + 1
    nb = tower_output_bytes(1, S, l14.v_width, l14.v_heads, l14.v_layers, hidden_states=True, attentions=True)
    assert S == 577 and nb["attentions"] == 24 * 16 * 577 * 577 * 4 and 511e6 < nb["attentions"] < 512e6
    assert nb["hidden_states"] == 25 * 577 * 1024 * 4 and nb["last_hidden"] == 577 * 1024 * 4 and nb["pooled"] == 1024 * 4
    # only what is asked for
    nb = tower_output_bytes(4, 77, 512, 8, 12)
    assert nb == {"last_hidden": 4 * 77 * 512 * 4, "pooled": 4 * 512 * 4, "hidden_states": 0, "attentions": 0}


def test_header_declares_and_lib_binds_the_entries():
    from plip_amd import _lib
    header = open(os.path.join(ROOT, "include", "plipmi.h")).read()
    for name, nargs in (("plipmi_encode_tower_outputs", 11), ("plipmi_tower_shape", 3)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert name not in _lib.TEST_SYMBOLS
    assert "plipmi_encode_tower_outputs" in open(os.path.join(ROOT, "plip_amd", "engine_outputs.py")).read()


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_probability_kernel_resources(tmp_path):
    """attention_probs.hip: no scratch, no spills, no inline assembly (so the asynchronous-load rule of test_isa_audit.py has
    nothing to check), its LDS tile dynamic"""
    from plip_amd.build import CSRC, FLAGS, _hipcc
    src = os.path.join(CSRC, "attention_probs.hip")
    assert "asm" not in open(src).read()
    r = subprocess.run([_hipcc(), *FLAGS, "-I", CSRC, "-c", src, "-o", str(tmp_path / "p.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kernels = re.findall(r"Function Name: (\S*attention_probs_kernel\S*)", r.stderr)
    assert len(kernels) == 3, kernels      # fp32, bf16, f16
    padded = re.findall(r"Function Name: (\S*attention_probs_hd_kernel\S*)", r.stderr)
    assert len(padded) == 6, padded        # x the padded head sizes 96 and 128: the same unit, the same rules
    for key in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill", "SGPRs Spill", "LDS Size \\[bytes/block\\]"):
        vals = re.findall(r"%s: (\d+)" % key, r.stderr)
        assert len(vals) == 9 and all(v == "0" for v in vals), (key, vals)
    vgprs = [int(v) for v in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    assert len(vgprs) == 9 and max(vgprs) <= 128, vgprs
