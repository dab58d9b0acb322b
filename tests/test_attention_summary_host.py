"""CPU-side checks of the attention summaries (include/plipmi.h plipmi_encode_attention_summary): the C-ABI declarations and bindings,
the argument checks that need no device, the float64 rollout reference the GPU tests compare with, the fixtures of
tools/make_attention_summary_golden.py, the buffer arithmetic and the summary kernels' resource usage."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from attention_summary_refs import pooled_rows, rollout_bound, rollout_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_entries():
    from plip_amd import _lib
    header = open(os.path.join(ROOT, "include", "plipmi.h")).read()
    m = re.search(r"\bint\s+plipmi_encode_attention_summary\s*\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 10 == len(_lib.SYMBOLS["plipmi_encode_attention_summary"][1])
    assert "plipmi_encode_attention_summary" not in _lib.TEST_SYMBOLS
    test_header = open(os.path.join(ROOT, "include", "plipmi_test.h")).read()
    for name in ("plipmi_attention_pooled_rows", "plipmi_attention_rollout_step"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, test_header)
        assert m, name
        assert len(m.group(1).split(",")) == 10 == len(_lib.TEST_SYMBOLS[name][1]), name
        assert name not in _lib.SYMBOLS and name not in header
    assert "plipmi_encode_attention_summary" in open(os.path.join(ROOT, "plip_amd", "engine_outputs.py")).read()
    # additive: the version number and the entry it extends are as they were
    assert re.search(r"#define PLIPMI_VERSION 412\b", header)
    assert len(_lib.SYMBOLS["plipmi_encode_tower_outputs"][1]) == 11


def test_null_handle_and_missing_outputs_are_invalid():
    """what the entry refuses before it touches a device: a null handle (checked first, whatever else is NULL)"""
    from plip_amd import _lib
    lib = _lib.load()
    assert lib.plipmi_encode_attention_summary(None, _lib.VISION, None, None, 1, -1, None, None, None, None) == 1     # PLIPMI_ERR_INVALID
    assert "null handle" in _lib.last_error()
    assert lib.plipmi_encode_attention_summary(None, _lib.TEXT, None, None, 0, -1, None, None, None, None) == 1
    # the kernel-level entries: null buffers, S outside 1 .. 1024, R_out == R_in
    one = (np.zeros(4, np.float32)).ctypes.data
    for args in ((_lib.F32, None, one, one, 1, 16, 1, 0, None, None), (_lib.F32, one, None, one, 1, 16, 1, 0, None, None),
                 (_lib.F32, one, one, None, 1, 16, 1, 0, None, None), (_lib.F32, one, one, one, 1, 1025, 1, 0, None, None),
                 (7, one, one, one, 1, 16, 1, 0, None, None)):
        assert lib.plipmi_attention_pooled_rows(*args) == 1, args
    for args in ((_lib.F32, None, None, one, 1, 16, 1, 0, None, None), (_lib.F32, one, None, None, 1, 16, 1, 0, None, None),
                 (_lib.F32, one, one, one, 1, 16, 1, 0, None, None), (_lib.F32, one, None, one, 1, 0, 1, 0, None, None),
                 (_lib.F32, one, None, one, 1, 16, 0, 0, None, None)):
        assert lib.plipmi_attention_rollout_step(*args) == 1, args
    assert "R_in" in _lib.last_error() or "bad argument" in _lib.last_error()


def _stochastic_stack(rng, L, B, H, S, dead_row=None):
    P = rng.random((L, B, H, S, S))
    P /= P.sum(-1, keepdims=True)
    if dead_row is not None:
        l, b, i = dead_row
        P[l, b, :, i, :] = 0.0            # a row with no live key: every head's row is zeros
    return P


def _literal_rollout(P):
    """the definition written out: R_L = A^_L A^_{L-1} ... A^_1, associated from the LEFT (rollout_ref multiplies from the right),
    every product an explicit sum over k"""
    L, B, H, S, _ = P.shape
    out = np.empty((B, S, S))
    for b in range(B):
        hats = [0.5 * sum(P[l, b, h] for h in range(H)) / H + 0.5 * np.eye(S) for l in range(L)]
        out[b] = functools.reduce(lambda acc, a: np.einsum("ik,kj->ij", acc, a), hats[::-1][1:], hats[-1])
    return out


@pytest.mark.parametrize("L,B,H,S", [(1, 1, 1, 3), (3, 2, 2, 5), (4, 2, 3, 17)])
def test_rollout_ref_is_the_matrix_product_definition(L, B, H, S):
    rng = np.random.default_rng(100 * L + S)
    P = _stochastic_stack(rng, L, B, H, S)
    R = rollout_ref(list(P))
    assert R.dtype == np.float64 and R.shape == (B, S, S)
    np.testing.assert_allclose(R, _literal_rollout(P), rtol=0, atol=1e-14)
    np.testing.assert_allclose(rollout_ref(P), R, rtol=0, atol=0)          # one stacked array or a list of blocks
    np.testing.assert_allclose(R.sum(-1), 1.0, rtol=0, atol=1e-13)
    assert (R >= 0).all() and (R <= 1).all()
    # one block: R_1 = A^_1 itself
    R1 = rollout_ref(P[:1])
    np.testing.assert_allclose(R1, 0.5 * P[0].mean(1) + 0.5 * np.eye(S), rtol=0, atol=1e-16)


def test_rollout_ref_with_a_dead_row():
    """a dead row i of A_l leaves 1/2 e_i: the rollout row is half the previous block's row i, and no longer sums to 1"""
    rng = np.random.default_rng(5)
    L, B, H, S = 3, 2, 2, 6
    P = _stochastic_stack(rng, L, B, H, S, dead_row=(1, 0, 4))
    R = rollout_ref(P)
    np.testing.assert_allclose(R, _literal_rollout(P), rtol=0, atol=1e-14)
    R2 = rollout_ref(P[:2])
    np.testing.assert_allclose(R2[0, 4], 0.5 * rollout_ref(P[:1])[0, 4], rtol=0, atol=1e-16)
    np.testing.assert_allclose(R2[0, 4].sum(), 0.5, rtol=0, atol=1e-14)
    np.testing.assert_allclose(R2[1].sum(-1), 1.0, rtol=0, atol=1e-13)     # the other sample is untouched
    assert (R >= 0).all() and (R <= 1).all()


def test_rollout_ref_on_hf_tiny_attentions(golden):
    g = golden("tower_outputs_tiny")
    for key in ("eos_masked/vision_attentions", "eos_masked/text_attentions", "eos_nomask/text_attentions", "zero/text_attentions"):
        att = g[key]                      # [L, B, H, S, S], every block
        R = rollout_ref(att)
        assert R.shape == (att.shape[1], att.shape[3], att.shape[3]), key
        np.testing.assert_allclose(R.sum(-1), 1.0, rtol=0, atol=att.shape[0] * 2e-6, err_msg=key)   # HF's fp32 rows sum to 1 within a few ulp
        assert (R >= 0).all() and (R <= 1).all(), key


def test_pooled_rows_rule():
    ids = np.array([[5, 9, 511, 3, 511], [511, 1, 2, 3, 4], [1, 2, 3, 4, 5]])
    assert pooled_rows("vision", 3).tolist() == [0, 0, 0]
    assert pooled_rows("text", 3, ids, 511).tolist() == [2, 0, 0]          # first eos id, 0 when absent
    assert pooled_rows("text", 3, ids, 2).tolist() == [2, 0, 4]            # legacy rule: first arg-max of the ids
    assert pooled_rows("text", 3, ids, -1).tolist() == [2, 0, 4]


FIXTURES = {   # name -> {tower: (B, S, H, L)}
    "attention_summary_vitb32_b2": {"vision": (2, 50, 12, 12), "text": (2, 77, 8, 12)},
    "attention_summary_vitb32_160": {"vision": (2, 26, 12, 12)},
    "attention_summary_tinyp4": {"vision": (3, 257, 2, 2)},
}


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixture_shapes_and_consistency(name, golden):
    from oracle.make_golden import case_inputs
    from plip_amd.config import get_config
    g = golden(name)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1 << 20
    if name == "attention_summary_tinyp4":
        cfg = get_config("tiny-p4")
        assert FIXTURES[name]["vision"] == (3, cfg.v_tokens, cfg.v_heads, cfg.v_layers)
    assert {k.split("_")[0] for k in g} == set(FIXTURES[name])
    for tower, (B, S, H, L) in FIXTURES[name].items():
        pa, ro, rm, rows = (g[f"{tower}_{k}"] for k in ("pooled_attention", "rollout", "rollout_matrix", "rows"))
        assert pa.shape == (L, B, H, S) and ro.shape == (B, S) and rm.shape == (B, S, S) and rows.shape == (B,), (name, tower)
        assert pa.dtype == np.float32
        if tower == "vision":
            assert (rows == 0).all()
        else:
            cfg, sd, px, ids, mask = case_inputs("vitb32_b4")
            assert rows.tolist() == pooled_rows("text", B, ids[:B], cfg.eos_token_id).tolist()
            # under causal + padding mask the pooled row sees nothing behind itself
            for b in range(B):
                assert (pa[:, b, :, rows[b] + 1:] == 0).all() and (rm[b, rows[b], rows[b] + 1:] == 0).all()
        # the rollout is not recomputable from the pooled rows alone: it is the pooled row of the stored matrix
        assert np.array_equal(ro, rm[np.arange(B), rows])
        np.testing.assert_allclose(pa.sum(-1), 1.0, rtol=0, atol=1e-5)
        np.testing.assert_allclose(rm.astype(np.float64).sum(-1), 1.0, rtol=0, atol=1e-5)
        assert (rm >= 0).all() and (rm <= 1).all()


def test_tiny_fixture_rollout_row_is_recomputable(golden):
    """where every block's attentions are stored (the tiny arch) the summaries follow from them: pooled rows by slicing, the rollout by
    rollout_ref -- what the GPU parity test compares the engine with"""
    from oracle.make_golden import case_inputs
    g = golden("tower_outputs_tiny")
    cfg, sd, px, ids, mask = case_inputs("tiny_b6")
    att = g["eos_masked/text_attentions"]
    rows = pooled_rows("text", att.shape[1], ids, cfg.eos_token_id)
    R = rollout_ref(att)
    row = R[np.arange(len(rows)), rows]
    assert row.shape == (6, cfg.context_length)
    np.testing.assert_allclose(row.sum(-1), 1.0, rtol=0, atol=1e-5)
    for b, r in enumerate(rows):
        assert (row[b, r + 1:] == 0).all()


def test_buffer_size_arithmetic_and_bound():
    from plip_amd.config import get_config
    from plip_amd.outputs import AttentionSummary, attention_summary_bytes
    l14 = get_config("ViT-L/14@336px")
    S = (l14.image_size // l14.patch_size) ** 2 + 1
    nb = attention_summary_bytes(1, S, l14.v_heads, l14.v_layers, True, True, False)
    # ViT-L/14@336: two [577, 577] fp32 buffers, 2.7 MB per image, against 511 MB of attentions
    assert nb["scratch"] == 4 + 2 * 577 * 577 * 4 and 2.6e6 < nb["scratch"] < 2.7e6
    assert nb["pooled_attention"] == 24 * 16 * 577 * 4 and nb["rollout"] == 577 * 4 and nb["rollout_matrix"] == 0
    nb = attention_summary_bytes(4, 50, 12, 12, False, False, True)
    assert nb == {"pooled_attention": 0, "rollout": 0, "rollout_matrix": 4 * 50 * 50 * 4, "scratch": 16 + 4 * 50 * 50 * 4}
    assert attention_summary_bytes(4, 50, 12, 12, True, False, False)["scratch"] == 16
    assert [f for f in AttentionSummary.__dataclass_fields__] == ["pooled_attention", "rollout", "rollout_matrix"]
    assert AttentionSummary().rollout_matrix is None
    assert rollout_bound(3, 50, 12) == 3 * 66 * 2.0 ** -24


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_summary_kernel_resources(tmp_path):
    """attention_summary.hip: no scratch, no vector-register spills, no inline assembly, dynamic LDS only; the recorded table
    (profiles/attention_summary_resource_usage.txt) names every kernel the file builds"""
    from plip_amd.build import CSRC, FLAGS, _hipcc
    src = os.path.join(CSRC, "attention_summary.hip")
    assert "asm" not in open(src).read() and "asm" not in open(os.path.join(CSRC, "attention_probs_dev.h")).read()
    r = subprocess.run([_hipcc(), *FLAGS, "-I", CSRC, "-c", src, "-o", str(tmp_path / "s.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    assert sum("attention_pooled_rows_kernel" in k for k in kernels) == 3          # fp32, bf16, f16
    assert sum("attention_rollout_step_kernel" in k for k in kernels) == 9         # x 3 row splits
    assert sum("attention_rollout_row_kernel" in k for k in kernels) == 1
    # (the 16-rows-per-lane form of the rollout step parks a few scalar registers in vector-register lanes: no memory is involved)
    for key in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill", "LDS Size \\[bytes/block\\]"):
        vals = re.findall(r"%s: (\d+)" % key, r.stderr)
        assert len(vals) == len(kernels) and all(v == "0" for v in vals), (key, vals)
    vgprs = [int(v) for v in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    assert max(vgprs) <= 128, vgprs
    table = open(os.path.join(ROOT, "profiles", "attention_summary_resource_usage.txt")).read()
    for k in set(kernels):
        assert k in table, k
