"""CPU-side checks of the dense image-text similarity (include/plipmi.h plipmi_encode_token_similarity): the C-ABI declarations and
bindings, the argument checks that need no device, the float64 reference the GPU tests compare with against the HF fixtures of
tools/make_token_similarity_golden.py, the fixtures themselves, the buffer arithmetic, the Python surface and the scores kernel's
resource usage."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from token_similarity_refs import FIXTURES, head_ref, head_weights, scores_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_entries():
    from plip_amd import _lib
    header = open(os.path.join(ROOT, "include", "plipmi.h")).read()
    m = re.search(r"\bint\s+plipmi_encode_token_similarity\s*\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 10 == len(_lib.SYMBOLS["plipmi_encode_token_similarity"][1])
    assert "plipmi_encode_token_similarity" not in _lib.TEST_SYMBOLS
    assert re.search(r"#define PLIPMI_TOKEN_SIM_MAX_C 64\b", header) and _lib.TOKEN_SIM_MAX_C == 64
    test_header = open(os.path.join(ROOT, "include", "plipmi_test.h")).read()
    m = re.search(r"\bint\s+plipmi_token_scores\s*\(([^;]*)\);", test_header)
    assert m and len(m.group(1).split(",")) == 9 == len(_lib.TEST_SYMBOLS["plipmi_token_scores"][1])
    assert "plipmi_token_scores" not in _lib.SYMBOLS and "plipmi_token_scores" not in header
    # the tables are the headers, name for name
    for hdr, table in ((header, _lib.SYMBOLS), (test_header, _lib.TEST_SYMBOLS)):
        assert set(re.findall(r"\b(plipmi_[a-z0-9_]+)\s*\(", hdr)) == set(table)
    assert "plipmi_encode_token_similarity" in open(os.path.join(ROOT, "plip_amd", "token_similarity.py")).read()
    # additive: the version number and the entry whose walk it uses are as they were
    assert re.search(r"#define PLIPMI_VERSION 412\b", header)
    assert len(_lib.SYMBOLS["plipmi_encode_tower_outputs"][1]) == 11


def test_null_handle_and_bad_kernel_arguments_are_invalid():
    """what is refused before a device is touched: a null handle (checked first, whatever else is NULL or out of range), and the
    kernel-level entry's shapes and pointers"""
    from plip_amd import _lib
    lib = _lib.load()
    assert lib.plipmi_encode_token_similarity(None, None, 1, None, 4, 1.0, 0, None, None, None) == 1     # PLIPMI_ERR_INVALID
    assert "null handle" in _lib.last_error()
    assert lib.plipmi_encode_token_similarity(None, None, 0, None, 0, 1.0, 0, None, None, None) == 1
    assert "null handle" in _lib.last_error()
    assert lib.plipmi_encode_token_similarity(None, None, 1, None, 65, 1.0, 1, None, None, None) == 1
    assert "null handle" in _lib.last_error()
    buf = np.zeros(64, np.float32)
    one = buf.ctypes.data + (-buf.ctypes.data) % 16       # a 16-byte aligned address (never read: every call below is refused)
    good = dict(E=one, M=1, P=32, T=one, C=1, scale=1.0, softmax=0, out=one)
    for change, word in ((dict(E=None), "null"), (dict(T=None), "null"), (dict(out=None), "null"), (dict(M=-1), "M ="),
                         (dict(P=0), "P ="), (dict(P=48), "P ="), (dict(P=1056), "P ="), (dict(C=0), "C ="), (dict(C=65), "C ="),
                         (dict(E=one + 4), "aligned"), (dict(T=one + 8), "aligned")):
        a = {**good, **change}
        assert lib.plipmi_token_scores(a["E"], a["M"], a["P"], a["T"], a["C"], a["scale"], a["softmax"], a["out"], None) == 1, change
        assert word in _lib.last_error(), (change, _lib.last_error())


def _hf_last_hidden(name, golden):
    """HF's last_hidden_state [B, S, Dv] of the fixture's pixels, from the fixtures that hold it"""
    if name == "token_similarity_tiny":
        return golden("tower_outputs_tiny")["eos_masked/vision_last_hidden_state"]
    if name == "token_similarity_tinyp4":
        return golden(name)["last_hidden_state"]
    if name == "token_similarity_vitb32_b2":
        return golden("tower_outputs_vitb32_b2_last")["b2/vision_last_hidden_state"]
    return golden("tower_outputs_vitb32_160")["160/vision_last_hidden_state"]


@pytest.mark.parametrize("name", list(FIXTURES))
def test_head_ref_reproduces_the_hf_fixture(name, golden):
    """head_ref in float64 on HF's own last_hidden_state gives the fixture (HF's fp32 head) to 1e-6"""
    from oracle.make_golden import case_inputs
    case, n_img, (B, S, P, C) = FIXTURES[name]
    cfg, sd, px, ids, mask = case_inputs(case)
    g, X = golden(name), _hf_last_hidden(name, golden)
    assert X.shape == (B, S, cfg.v_width)
    ln_w, ln_b, proj = head_weights(sd)
    E, sim = head_ref(X, ln_w, ln_b, cfg.layer_norm_eps, proj, golden(case)["text_embeds"])
    err_e = float(np.abs(E.numpy() - g["token_embeds"]).max())
    err_s = float(np.abs(sim.numpy() - g["similarity"]).max())
    print(f"{name}: |E - fixture| {err_e:.2e} (max |E| {np.abs(g['token_embeds']).max():.2f}), |sim - fixture| {err_s:.2e}")
    assert err_e <= 1e-6 * max(1.0, float(np.abs(g["token_embeds"]).max())) and err_s <= 1e-6
    # the score part on the fixture's own E, softmax included, and text rows of other norms
    T = golden(case)["text_embeds"].astype(np.float64)
    np.testing.assert_allclose(scores_ref(g["token_embeds"], T).numpy(), g["similarity"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(scores_ref(g["token_embeds"], T * np.linspace(0.01, 100, C)[:, None]).numpy(), g["similarity"], rtol=0, atol=1e-6)
    sm = scores_ref(g["token_embeds"], T, scale=100.0, softmax=True).numpy()
    np.testing.assert_allclose(sm.sum(-1), 1.0, rtol=0, atol=1e-12)
    import torch
    np.testing.assert_allclose(sm, torch.softmax(torch.from_numpy(100.0 * g["similarity"].astype(np.float64)), -1).numpy(), rtol=0, atol=1e-4)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixture_shapes_and_consistency(name, golden):
    from oracle.make_golden import case_inputs
    case, n_img, (B, S, P, C) = FIXTURES[name]
    g = golden(name)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1 << 20
    assert set(g) == {"token_embeds", "similarity"} | ({"last_hidden_state"} if name == "token_similarity_tinyp4" else set())
    assert g["token_embeds"].shape == (B, S, P) and g["similarity"].shape == (B, S, C)
    assert g["token_embeds"].dtype == np.float32 and g["similarity"].dtype == np.float32
    cfg, sd, px, ids, mask = case_inputs(case)
    assert P == cfg.projection_dim and C == len(ids)
    assert np.isfinite(g["token_embeds"]).all() and (np.abs(g["similarity"]) <= 1 + 1e-6).all()
    assert np.linalg.norm(g["token_embeds"], axis=-1).min() > 1.0          # no row near the zero-norm case
    if n_img is not None:
        # row 0 is the CLS token: times exp(logit_scale) it is the case's own logits_per_image
        scale = float(np.exp(float(sd["logit_scale"])))
        assert S == cfg.v_tokens and n_img == B
        err = np.abs(g["similarity"][:, 0, :].astype(np.float64) * scale - golden(case)["logits_per_image"][:B]).max()
        assert err <= 2e-6 * scale, (name, err)
    else:
        assert S == 1 + (160 // cfg.patch_size) ** 2


def test_buffer_size_arithmetic():
    from plip_amd.config import get_config
    from plip_amd.outputs import token_similarity_bytes
    nb = token_similarity_bytes(256, 50, 768, 512, 10)
    assert nb == {"similarity": 256 * 50 * 10 * 4, "token_embeds": 0, "scratch": 256 * 50 * 768 * 4 + 256 * 50 * 512 * 4}
    nb = token_similarity_bytes(256, 50, 768, 512, 10, token_embeds=True)
    assert nb == {"similarity": 512000, "token_embeds": 256 * 50 * 512 * 4, "scratch": 256 * 50 * 768 * 4}
    l14 = get_config("ViT-L/14@336px")
    S = (l14.image_size // l14.patch_size) ** 2 + 1
    nb = token_similarity_bytes(1, S, l14.v_width, l14.projection_dim, 64)
    # ViT-L/14@336: 577 tokens of width 1024 projected to 768 -- 2.4 MB of LayerNorm'd rows (rounded up to 256 bytes) + 1.8 MB of E per image
    assert S == 577 and nb["similarity"] == 577 * 64 * 4 and nb["token_embeds"] == 0
    assert nb["scratch"] == (577 * 1024 * 4 + 255) // 256 * 256 + 577 * 768 * 4 == 2363392 + 1772544
    assert token_similarity_bytes(0, 50, 768, 512, 10) == {"similarity": 0, "token_embeds": 0, "scratch": 0}
    assert token_similarity_bytes(1, 17, 128, 64, 3)["scratch"] == 8704 + 17 * 64 * 4        # 17 * 128 * 4 = 8704 is a multiple of 256


def test_python_surface():
    import inspect

    from plip_amd import engine as E
    from plip_amd import model, outputs, plip, token_similarity
    assert [f for f in outputs.TokenSimilarity.__dataclass_fields__] == ["similarity", "token_embeds"]
    assert outputs.TokenSimilarity().token_embeds is None
    # the call is a function on an engine: Engine's public attributes are as they were
    assert not any("token_similarity" in k for k in dir(E.Engine) if not k.startswith("_"))
    sig = inspect.signature(token_similarity.token_similarity)
    assert list(sig.parameters) == ["engine", "pixels", "text_embeds", "scale", "softmax", "return_embeds"]
    assert [sig.parameters[k].default for k in ("scale", "softmax", "return_embeds")] == [1.0, False, False]
    assert hasattr(model._Tower, "token_similarity")
    sig = inspect.signature(plip.PLIP.similarity_maps)
    assert list(sig.parameters) == ["self", "images", "text", "batch_size", "image_size", "softmax", "scale"]
    assert sig.parameters["scale"].default is None and sig.parameters["softmax"].default is False
    # the text tower has no such call: refused before any engine is touched
    with pytest.raises(ValueError, match="vision_model"):
        model._Tower(None, vision=False).token_similarity()


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_token_scores_kernel_resources(tmp_path):
    """token_scores.hip: no scratch, no register spills, no inline assembly, dynamic LDS only; the recorded table
    (profiles/token_similarity_resource_usage.txt) names every kernel the file builds"""
    from plip_amd.build import CSRC, FLAGS, SOURCES, _hipcc
    assert "token_scores.hip" in SOURCES
    src = os.path.join(CSRC, "token_scores.hip")
    assert not re.search(r"\basm\b|__asm", open(src).read())
    r = subprocess.run([_hipcc(), *FLAGS, "-I", CSRC, "-c", src, "-o", str(tmp_path / "s.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    assert sum("token_scores_kernel" in k for k in kernels) == 5 == len(kernels)        # 1, 2, 4, 8, 16 pieces of a row per lane
    for key in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill", "SGPRs Spill", "LDS Size \\[bytes/block\\]"):
        vals = re.findall(r"%s: (\d+)" % key, r.stderr)
        assert len(vals) == len(kernels) and all(v == "0" for v in vals), (key, vals)
    vgprs = [int(v) for v in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    assert max(vgprs) <= 160, vgprs
    table = open(os.path.join(ROOT, "profiles", "token_similarity_resource_usage.txt")).read()
    for k in set(kernels):
        assert k in table, k
