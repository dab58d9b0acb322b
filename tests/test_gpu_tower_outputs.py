"""Per-token tower outputs (include/plipmi.h plipmi_encode_tower_outputs, Engine.tower_outputs, PlipModel.vision_model /
.text_model / forward(output_attentions=, output_hidden_states=)) against HF CLIPModel with eager attention
(tests/golden/tower_outputs_*.npz, tools/make_tower_outputs_golden.py), and what the entry must leave alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.make_golden import case_inputs
from plip_amd import _lib

pytestmark = pytest.mark.gpu

# Max-abs errors against HF.  attn: on the probabilities.  hid / last / pool: relative to the field's largest magnitude
# (hidden states grow through the tower; pooled rows are LayerNorm'd).  About 1.5x the errors measured on the MI355X
# (profiles/tower_outputs_parity.txt), never looser than 1e-5 (fp32) / 5e-3 (16-bit) on the probabilities.
TOL = {
    "f32": dict(attn=2e-7, hid=3.5e-6, last=3.5e-6, pool=2.5e-6),
    "bf16": dict(attn=6e-4, hid=4.5e-3, last=4.5e-3, pool=4e-3),
    "f16": dict(attn=2.7e-4, hid=1.3e-3, last=1.5e-3, pool=1.2e-3),
}
DTYPES = ["f32", "bf16", "f16"]


def _fixture(golden, *names):
    d = {}
    for n in names:
        d.update(golden(n))
    return d


def _err(got, ref, relative):
    e = float(np.abs(np.asarray(got, np.float64) - ref).max())
    return e / float(np.abs(ref).max()) if relative else e


def _compare(tag, dtype, out, g, prefix, tower):
    """every field of ``out`` (a TowerOutput) against the fixture's ``<prefix>/<tower>_*`` keys"""
    t = TOL[dtype]
    errs = {}
    errs["last"] = _err(out.last_hidden_state.cpu().numpy(), g[f"{prefix}/{tower}_last_hidden_state"], True) \
        if f"{prefix}/{tower}_last_hidden_state" in g else 0.0
    errs["pool"] = _err(out.pooler_output.cpu().numpy(), g[f"{prefix}/{tower}_pooler_output"], True) \
        if f"{prefix}/{tower}_pooler_output" in g else 0.0
    hi, ai = g[f"{prefix}/{tower}_hidden_idx"], g[f"{prefix}/{tower}_attn_idx"]
    errs["hid"] = max(_err(out.hidden_states[int(i)].cpu().numpy(), g[f"{prefix}/{tower}_hidden_states"][k], True) for k, i in enumerate(hi))
    errs["attn"] = max(_err(out.attentions[int(i)].cpu().numpy(), g[f"{prefix}/{tower}_attentions"][k], False) for k, i in enumerate(ai))
    print(f"PARITY {dtype} {tag} {tower}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= t[k], (dtype, tag, tower, k, v, t[k])


def _probs_structure(att, mask, causal):
    """rows sum to 1, exact zeros at causal and padded positions"""
    for a in att:
        a = a.cpu().numpy()
        B, H, S, _ = a.shape
        sums = a.sum(-1)
        np.testing.assert_allclose(sums, 1.0, atol=1e-5, rtol=0)
        dead = np.zeros((B, S, S), bool)
        if causal:
            dead |= np.triu(np.ones((S, S), bool), 1)[None]
        if mask is not None:
            dead |= (np.asarray(mask) == 0)[:, None, :]
        assert (a[np.broadcast_to(dead[:, None], a.shape)] == 0.0).all()
        assert (a[np.broadcast_to(~dead[:, None], a.shape)] > 0.0).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_every_layer_against_hf(dtype, engines, golden):
    """tiny arch, every hidden state and attention map of both towers: captions with their mask (padded keys), the same captions
    without one, and zero-padded captions (argmax pooling)"""
    g = golden("tower_outputs_tiny")
    model, cfg, sd, px, ids, mask = engines("tiny_b6", dtype)
    v = model.vision_model(torch.from_numpy(px), output_attentions=True, output_hidden_states=True)
    assert len(v.hidden_states) == cfg.v_layers + 1 and len(v.attentions) == cfg.v_layers
    _compare("tiny", dtype, v, g, "eos_masked", "vision")
    _probs_structure(v.attentions, None, False)
    t = model.text_model(torch.from_numpy(ids), torch.from_numpy(mask), output_attentions=True, output_hidden_states=True)
    _compare("tiny masked", dtype, t, g, "eos_masked", "text")
    _probs_structure(t.attentions, mask, True)
    t = model.text_model(torch.from_numpy(ids), output_attentions=True, output_hidden_states=True)
    _compare("tiny unmasked", dtype, t, g, "eos_nomask", "text")
    _probs_structure(t.attentions, None, True)
    model, cfg, sd, px, ids, mask = engines("tiny_b5_zero_pad_ln100", dtype)
    t = model.text_model(torch.from_numpy(ids), output_attentions=True, output_hidden_states=True)
    _compare("tiny zero-pad", dtype, t, g, "zero", "text")


@pytest.mark.parametrize("dtype", DTYPES)
def test_vitb32_against_hf(dtype, engines, golden):
    """ViT-B/32, B = 2: layers 0, 5, 11 of both towers (the text tower under its padding mask), last_hidden_state, pooler_output"""
    g = _fixture(golden, "tower_outputs_vitb32_b2_vision_attn", "tower_outputs_vitb32_b2_vision_hidden", "tower_outputs_vitb32_b2_text_attn",
                 "tower_outputs_vitb32_b2_text_hidden", "tower_outputs_vitb32_b2_last")
    model, cfg, sd, px, ids, mask = engines("vitb32_b4", dtype)
    v = model.vision_model(pixel_values=torch.from_numpy(px[:2]), output_attentions=True, output_hidden_states=True)
    assert v.last_hidden_state.shape == (2, 50, 768) and v.attentions[0].shape == (2, 12, 50, 50) and len(v.hidden_states) == 13
    _compare("vitb32", dtype, v, g, "b2", "vision")
    t = model.text_model(input_ids=torch.from_numpy(ids[:2]), attention_mask=torch.from_numpy(mask[:2]), output_attentions=True,
                         output_hidden_states=True)
    assert t.attentions[0].shape == (2, 8, 77, 77) and len(t.attentions) == 12
    _compare("vitb32", dtype, t, g, "b2", "text")
    _probs_structure(t.attentions, mask[:2], True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_resolution_handle_against_hf(dtype, engines, golden):
    """a plipmi_clone_resolution handle (160 x 160: 26 tokens) -- HF interpolate_pos_encoding=True"""
    g = golden("tower_outputs_vitb32_160")
    model, *_ = engines("vitb32_b4", dtype)
    px = np.random.RandomState(160).standard_normal((2, 3, 160, 160)).astype(np.float32)    # tools/make_tower_outputs_golden.py pixels_160
    v = model.vision_model(torch.from_numpy(px), output_attentions=True, output_hidden_states=True, interpolate_pos_encoding=True)
    assert v.attentions[0].shape == (2, 12, 26, 26)
    _compare("vitb32 160x160", dtype, v, g, "160", "vision")
    _probs_structure(v.attentions, None, False)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batch_larger_than_max_batch(dtype, golden):
    """B = 6 on an engine of max_batch 4: two chunks, every field still HF's"""
    from plip_amd.model import PlipModel
    g = golden("tower_outputs_tiny")
    cfg, sd, px, ids, mask = case_inputs("tiny_b6")
    model = PlipModel(cfg, sd, dtype=dtype, max_batch=4)
    try:
        v = model.vision_model(torch.from_numpy(px), output_attentions=True, output_hidden_states=True)
        _compare("tiny chunked", dtype, v, g, "eos_masked", "vision")
        t = model.text_model(torch.from_numpy(ids), torch.from_numpy(mask), output_attentions=True, output_hidden_states=True)
        _compare("tiny chunked", dtype, t, g, "eos_masked", "text")
    finally:
        model.engine.close()


def test_forward_fills_tower_outputs(engines):
    """forward(output_attentions=True) fills vision_model_output / text_model_output like CLIPModel; without the flags the fields
    stay None and the logits are the same bits"""
    model, cfg, sd, px, ids, mask = engines("tiny_b6", "bf16")
    kw = dict(input_ids=torch.from_numpy(ids), pixel_values=torch.from_numpy(px), attention_mask=torch.from_numpy(mask))
    plain = model(**kw)
    assert plain.vision_model_output is None and plain.text_model_output is None and len(plain.to_tuple()) == 4
    out = model(**kw, output_attentions=True)
    assert torch.equal(out.logits_per_image, plain.logits_per_image)
    assert len(out.vision_model_output.attentions) == cfg.v_layers and len(out.text_model_output.attentions) == cfg.t_layers
    assert out.vision_model_output.hidden_states is None
    ref = model.vision_model(torch.from_numpy(px), output_attentions=True)
    for a, b in zip(out.vision_model_output.attentions, ref.attentions):
        assert torch.equal(a, b)
    assert len(out.to_tuple()) == 6
    out = model(**kw, output_hidden_states=True)
    assert len(out.text_model_output.hidden_states) == cfg.t_layers + 1 and out.text_model_output.attentions is None


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_encode_bits_unchanged_after_tower_outputs(dtype):
    """the entry changes nothing the encode paths read: encode_pair returns the same bits before and after it, through the
    small-batch graph replay (eager, captured, replayed) and with caption packing on"""
    from plip_amd.model import PlipModel
    cfg, sd, px, ids, mask = case_inputs("vitb32_b4")
    model = PlipModel(cfg, sd, dtype=dtype, max_batch=8)
    eng = model.engine
    try:
        P, I, Mk = torch.from_numpy(px), torch.from_numpy(ids), torch.from_numpy(mask)
        before = [eng.encode_pair(P, I, Mk) for _ in range(3)]
        eng.tower_outputs("text", I, Mk, output_hidden_states=True, output_attentions=True)
        eng.tower_outputs("vision", P, output_hidden_states=True, output_attentions=True)
        after = [eng.encode_pair(P, I, Mk) for _ in range(2)]
        for a in before[1:] + after:
            assert torch.equal(a[0], before[0][0]) and torch.equal(a[1], before[0][1])
        eng.set_text_packing(True)
        packed = eng.encode_text(I, Mk, normalize=True)
        eng.tower_outputs("text", I, Mk, output_attentions=True)
        assert torch.equal(eng.encode_text(I, Mk, normalize=True), packed)
    finally:
        model.engine.close()


def test_errors(engines, monkeypatch):
    model, cfg, sd, px, ids, mask = engines("tiny_b6", "f32")
    eng = model.engine
    lib = eng.lib
    x = torch.from_numpy(px).cuda()
    out = torch.empty((6, 17, cfg.v_width), device="cuda")
    s = eng._stream()
    # no output buffer at all / null input / a tower that does not exist
    assert lib.plipmi_encode_tower_outputs(eng._h, _lib.VISION, C.c_void_p(x.data_ptr()), None, 6, -1, None, None, None, None, s) != 0
    assert "no output" in _lib.last_error()
    assert lib.plipmi_encode_tower_outputs(eng._h, _lib.VISION, None, None, 6, -1, C.c_void_p(out.data_ptr()), None, None, None, s) != 0
    assert lib.plipmi_encode_tower_outputs(eng._h, 2, C.c_void_p(x.data_ptr()), None, 6, -1, C.c_void_p(out.data_ptr()), None, None, None, s) != 0
    assert "tower" in _lib.last_error()
    shape = (C.c_int32 * 4)()
    assert lib.plipmi_tower_shape(eng._h, 7, shape) != 0
    assert eng.tower_shape("vision") == (17, cfg.v_width, cfg.v_heads, cfg.v_layers)
    assert eng.tower_shape("text") == (cfg.context_length, cfg.t_width, cfg.t_heads, cfg.t_layers)
    with pytest.raises(ValueError, match="tower"):
        eng.tower_outputs("audio", x)
    with pytest.raises(ValueError, match="attention_mask"):
        eng.tower_outputs("vision", x, torch.from_numpy(mask))
    # a request larger than the free device memory is refused before anything is allocated
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (4096, 1 << 30))
    with pytest.raises(ValueError, match="MiB"):
        eng.tower_outputs("vision", x, output_attentions=True, output_hidden_states=True)
