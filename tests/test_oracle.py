"""The CPU oracle (oracle/clip_oracle.py) pinned against the golden vectors produced by the
reference's arithmetic (HF CLIPModel, oracle/make_golden.py).  CPU only."""
import numpy as np
import pytest

from oracle import clip_oracle as O
from oracle import hf_reference as H
from oracle.make_golden import CASES, SLIM, case_inputs, fingerprint

FULL_CASES = [c for c in CASES if c not in SLIM]

FP32_FEAT_TOL = 2e-5     # |features| ~ 3-5; HF sdpa vs eager already differ by ~2e-6
FP32_COS_TOL = 2e-6


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_inputs_regenerate(name, golden):
    """Seeds -> exactly the tensors the fixtures were generated from (RandomState is frozen)."""
    g = golden(name)
    cfg, sd, px, ids, mask = case_inputs(name)
    np.testing.assert_array_equal(g["ids"], ids)
    np.testing.assert_array_equal(g["mask"], mask)
    np.testing.assert_allclose(fingerprint(sd), g["weights_fingerprint"], rtol=0, atol=0)
    fp = np.array([px.astype(np.float64).sum(), (px.astype(np.float64) ** 2).sum()])
    np.testing.assert_allclose(fp, g["pixels_fingerprint"], rtol=0, atol=0)


def test_oracle_matches_golden_bs256_rows(golden):
    """BASELINE configs[2] size: the oracle on eight rows of the 256-pair batch against HF's own 256 x 256 logits
    (samples are independent, so a row subset is exact; the whole batch would cost the CPU suite a minute)."""
    g = golden("vitb32_b256")
    cfg, sd, px, ids, mask = case_inputs("vitb32_b256")
    rows = [0, 1, 37, 100, 128, 199, 254, 255]
    o = O.clip_forward(px[rows], ids[rows], sd, cfg, mask[rows])
    assert np.abs(o["image_embeds"] - g["image_embeds"][rows]).max() < FP32_COS_TOL
    assert np.abs(o["text_embeds"] - g["text_embeds"][rows]).max() < FP32_COS_TOL
    scale = np.exp(np.float64(sd["logit_scale"]))
    assert np.abs(o["logits_per_image"] - g["logits_per_image"][rows][:, rows]).max() / scale < FP32_COS_TOL
    # the fixture is self-consistent: logits = scale * img @ txt^T over all 65 536 entries
    full = (g["image_embeds"].astype(np.float64) @ g["text_embeds"].astype(np.float64).T) * scale
    assert np.abs(full - g["logits_per_image"]).max() / scale < FP32_COS_TOL


@pytest.mark.parametrize("name", FULL_CASES)
def test_oracle_matches_golden(name, golden):
    g = golden(name)
    cfg, sd, px, ids, mask = case_inputs(name)
    use_mask = None if "zero_pad" in name else mask
    o = O.clip_forward(px, ids, sd, cfg, use_mask)
    for k in ("image_features", "text_features"):
        assert np.abs(o[k] - g[k]).max() < FP32_FEAT_TOL, k
    for k in ("image_embeds", "text_embeds"):
        assert np.abs(o[k] - g[k]).max() < FP32_COS_TOL, k
    scale = np.exp(np.float64(sd["logit_scale"]))
    assert np.abs(o["logits_per_image"] - g["logits_per_image"]).max() / scale < FP32_COS_TOL
    np.testing.assert_array_equal(o["logits_per_image"], o["logits_per_text"].T)
    np.testing.assert_array_equal(o["logits_per_image"].argmax(1), g["logits_per_image"].argmax(1))


def test_oracle_hidden_states_tiny(golden):
    g = golden("tiny_b6")
    cfg, sd, px, ids, mask = case_inputs("tiny_b6")
    _, vh = O.vision_tower(px, sd, cfg, return_hidden=True)
    _, th = O.text_tower(ids, sd, cfg, mask, return_hidden=True)
    assert len(vh) == cfg.v_layers + 1 and len(th) == cfg.t_layers + 1
    assert np.abs(np.stack(vh) - g["vision_hidden"]).max() < 2e-5
    # rows after the EOS see padding keys only through the mask; compare the attended rows
    m = mask[None, :, :, None].astype(np.float32)
    assert np.abs((np.stack(th) - g["text_hidden"]) * m).max() < 2e-5


def test_oracle_hidden_states_vitb32(golden):
    g = golden("vitb32_b4")
    cfg, sd, px, ids, mask = case_inputs("vitb32_b4")
    _, vh = O.vision_tower(px, sd, cfg, return_hidden=True)
    _, th = O.text_tower(ids, sd, cfg, mask, return_hidden=True)
    assert np.abs(np.stack([h[:, 0] for h in vh]) - g["vision_hidden_cls"]).max() < 1e-4
    assert np.abs(np.stack([h[:, -1] for h in vh]) - g["vision_hidden_last_token"]).max() < 1e-4
    assert np.abs(np.stack([h[:, 0] for h in th]) - g["text_hidden_bos"]).max() < 1e-4
    assert np.abs(np.stack([h[:, 1] for h in th]) - g["text_hidden_tok1"]).max() < 1e-4


def test_oracle_fp64_error_budget():
    """fp32 vs fp64 restatement: the reference-precision noise floor the GPU tolerances sit above."""
    cfg, sd, px, ids, mask = case_inputs("tiny_b6")
    o32 = O.clip_forward(px, ids, sd, cfg, mask, dtype=np.float32)
    o64 = O.clip_forward(px, ids, sd, cfg, mask, dtype=np.float64)
    assert np.abs(o32["image_embeds"] - o64["image_embeds"]).max() < 1e-6
    assert np.abs(o32["text_embeds"] - o64["text_embeds"]).max() < 1e-6


def test_padding_mask_is_irrelevant_to_pooled_output():
    """Causal attention + EOS pooling: the tokenizer's padding mask cannot change the pooled
    embedding -- which is why the OpenAI path can run without one."""
    cfg, sd, px, ids, mask = case_inputs("tiny_b6")
    a = O.text_tower(ids, sd, cfg, mask)
    b = O.text_tower(ids, sd, cfg, None)
    np.testing.assert_array_equal(a, b)


def test_eos_rules():
    ids = np.array([[5, 9, 7, 9, 0], [0, 1, 2, 3, 4], [9, 9, 9, 9, 9]])
    np.testing.assert_array_equal(O.eos_positions(ids, 9), [1, 0, 0])      # first eos, 0 if absent
    np.testing.assert_array_equal(O.eos_positions(ids, 2), [1, 4, 0])      # legacy: first arg-max
    np.testing.assert_array_equal(O.eos_positions(ids, -1), [1, 4, 0])


def test_plip_cosine_similarity_quirk():
    """plip.py:73-76 normalises only the key vectors."""
    rs = np.random.RandomState(0)
    k, s = rs.randn(4, 8).astype(np.float32), rs.randn(3, 8).astype(np.float32)
    got = O.plip_cosine_similarity(k, s)
    want = (k / np.linalg.norm(k, axis=-1, keepdims=True)) @ s.T
    np.testing.assert_allclose(got, want, rtol=1e-6)


@pytest.mark.skipif(not H.available(), reason="transformers not importable")
def test_oracle_matches_live_hf_tiny():
    """Live run of the reference's third-party forward (both attention implementations)."""
    cfg, sd, px, ids, mask = case_inputs("tiny_b5_zero_pad_ln100")
    o = O.clip_forward(px, ids, sd, cfg, None)
    for impl in ("sdpa", "eager"):
        h = H.run(H.build_model(cfg, sd, impl), px, ids, None)
        assert np.abs(o["image_features"] - h["image_features"]).max() < FP32_FEAT_TOL
        assert np.abs(o["text_features"] - h["text_features"]).max() < FP32_FEAT_TOL
        assert np.abs(o["logits_per_image"] - h["logits_per_image"]).max() / 100.0 < FP32_COS_TOL


# ---- the bf16 engine's precision plan, costed on the CPU (oracle/precision_model.py) ----------------------------
@pytest.mark.parametrize("name", ["vitb32_b4", "vitb32_b8_heavy"])
@pytest.mark.parametrize("plan", ["round_ln", "folded"])
def test_bf16_precision_plans_hold_the_cosine_bar(name, plan, golden):
    """bf16 MFMA operands + fp32 everything else, emulated in numpy against the HF golden vectors: both ways of
    pairing LayerNorm with the following Linear (normalise-then-round, and LayerNorm folded into the weights with
    the statistics applied in the GEMM epilogue) stay inside the north-star 1e-3 cosine bar -- also on the
    heavy-tailed checkpoint (outlier channels, LayerNorm gains over two decades, logit_scale ln 100)."""
    from oracle import precision_model as P
    g = golden(name)
    cfg, sd, px, ids, mask = case_inputs(name)
    n = 4
    o = P.clip_forward(px[:n], ids[:n], sd, cfg, mask[:n], plan)
    scale = np.exp(np.float64(sd["logit_scale"]))
    err = np.abs(o["logits_per_image"] - g["logits_per_image"][:n, :n]).max() / scale
    assert err < 1e-3, (name, plan, err)
    assert np.abs(o["image_embeds"] - g["image_embeds"][:n]).max() < 2e-3
    assert np.abs(o["text_embeds"] - g["text_embeds"][:n]).max() < 2e-3


def test_operand_rounding_floor_of_the_text_tower(golden):
    """WHY the bf16 engine's text_embeds sit 3x further from HF than its image_embeds at the benchmark size,
    costed on the CPU: 48 captions of the bs=256 fixture through the numpy emulation with ONE class of operand rounding
    at a time, everything else exact.  bf16 weight rounding alone already exceeds 6e-4 (the perturbation is the same for
    every token of a caption, so attention does not average it out); all six bf16 roundings give the 1.2e-3 the engine
    measures -- it is the operand type, not a kernel -- and the same plan in IEEE half (PLIPMI_F16, same MFMA rate) is
    8x closer."""
    from oracle import precision_model as P
    g = golden("vitb32_b256")
    cfg, sd, px, ids, mask = case_inputs("vitb32_b256")
    n = 48
    want = g["text_embeds"][:n]

    def err(dtype, sites):
        e = O.l2_normalize(P.text_tower(ids[:n], sd, cfg, mask[:n], "folded", dtype=dtype, sites=sites))
        d = np.abs(e - want)
        return float(d.max()), float(np.sqrt((d.astype(np.float64) ** 2).mean()))
    exact = err("bf16", ())
    w_only = err("bf16", ("w",))
    acts = err("bf16", ("xa", "qkv", "p", "att", "mlp"))
    full = err("bf16", P.ALL_SITES)
    half = err("f16", P.ALL_SITES)
    print(f"text_embeds max / rms vs HF: exact {exact}, bf16 weights only {w_only}, bf16 activations only {acts}, "
          f"bf16 all {full}, f16 all {half}")
    assert exact[0] < 2e-6
    assert w_only[0] > 6e-4 and w_only[1] > acts[1]          # the weights are the larger half, and alone past 6e-4
    assert 8e-4 < full[0] < 2e-3
    assert abs(full[1] ** 2 - (w_only[1] ** 2 + acts[1] ** 2)) < 0.25 * full[1] ** 2     # the two halves add in quadrature
    assert half[0] < 2.5e-4 and half[1] < full[1] / 6


def test_the_first_text_blocks_carry_the_bf16_error(golden):
    """WHERE in the text tower bf16's operand rounding costs text_embeds, costed on the CPU: the same
    emulation with the operand type chosen per block.  f16 in the FIRST two blocks removes a third of the error, in the
    LAST two nothing -- the residual stream is small at the bottom of the tower, so a block's rounding error is large
    against it and every later LayerNorm carries it along.  Hence plipmi_config.text_f16_layers (leading blocks), default 4."""
    from oracle import precision_model as P
    g = golden("vitb32_b256")
    cfg, sd, px, ids, mask = case_inputs("vitb32_b256")
    n = 24
    want = g["text_embeds"][:n]

    def err(lead=0, dtype="bf16"):
        e = O.l2_normalize(P.text_tower(ids[:n], sd, cfg, mask[:n], "folded", dtype=dtype, lead_f16=lead))
        return float(np.sqrt((np.abs(e - want).astype(np.float64) ** 2).mean()))
    pure, lead2, lead4, allf16 = err(0), err(2), err(4), err(cfg.t_layers)
    # "f16 in the last two blocks": an f16 tower whose first ten blocks are... not expressible as a lead; emulate by hand
    rnd_b, rnd_h = P.Rounding("bf16"), P.Rounding("f16")
    x = P._f(sd, "text_model.embeddings.token_embedding.weight")[ids[:n]] + P._f(sd, "text_model.embeddings.position_embedding.weight")[None, :ids.shape[1]]
    for i in range(cfg.t_layers):
        sub = {k.replace(f".layers.{i}.", ".layers.0."): v for k, v in sd.items() if k.startswith(f"text_model.encoder.layers.{i}.")}
        x = P._layers(x, sub, "text_model", 1, cfg.t_heads, True, mask[:n], cfg.layer_norm_eps, "folded", [],
                      rnd_h if i >= cfg.t_layers - 2 else rnd_b)
    x = O.layer_norm(x, P._f(sd, "text_model.final_layer_norm.weight"), P._f(sd, "text_model.final_layer_norm.bias"), cfg.layer_norm_eps)
    e = O.l2_normalize(x[np.arange(n), O.eos_positions(ids[:n], cfg.eos_token_id)] @ P._f(sd, "text_projection.weight").T)
    last2 = float(np.sqrt((np.abs(e - want).astype(np.float64) ** 2).mean()))
    print(f"text_embeds rms vs HF: pure bf16 {pure:.2e}, f16 in the first 2 / 4 blocks {lead2:.2e} / {lead4:.2e}, in the last 2 {last2:.2e}, "
          f"in all {allf16:.2e}")
    assert allf16 < lead4 < lead2 < pure
    assert lead2 < 0.8 * pure and last2 > 0.93 * pure


@pytest.mark.parametrize("name", ["vitb32_b4", "vitb32_b8_heavy"])
def test_f16_precision_plan(name, golden):
    """The PLIPMI_F16 engine's plan (IEEE-half MFMA operands, LayerNorm folded) against the HF golden vectors, emulated:
    a quarter of the cosine bar, also on the heavy-tailed checkpoint whose residual stream reaches |x| ~ 90."""
    from oracle import precision_model as P
    g = golden(name)
    cfg, sd, px, ids, mask = case_inputs(name)
    n = 4
    o = P.clip_forward(px[:n], ids[:n], sd, cfg, mask[:n], "folded", dtype="f16")
    scale = np.exp(np.float64(sd["logit_scale"]))
    err = np.abs(o["logits_per_image"] - g["logits_per_image"][:n, :n]).max() / scale
    assert err < 2.5e-4, (name, err)
    assert np.abs(o["image_embeds"] - g["image_embeds"][:n]).max() < 4e-4
    assert np.abs(o["text_embeds"] - g["text_embeds"][:n]).max() < 4e-4


def test_bf16_rounding_helper_is_rne():
    import torch
    from oracle.precision_model import bf16
    x = np.random.RandomState(0).standard_normal(4096).astype(np.float32) * np.float32(37.0)
    x[:4] = [1.00390625, 1.01171875, -1.00390625, 3.3895314e38]       # ties (to even) and a value near the top
    np.testing.assert_array_equal(bf16(x), torch.from_numpy(x).bfloat16().float().numpy())


# ---- the OpenAI-clip checkpoint layout, pinned independently of the converter's own inverse ------------------------
def test_openai_layout_converter_against_independent_openai_style_model():
    """reproducibility/embedders/factory.py:21-25 loads OpenAI-clip state dicts (packed ``attn.in_proj_weight``,
    ``visual.proj [width, proj]`` applied as ``x @ proj``, ``text_projection [width, proj]``).  oracle/openai_clip_ref.py
    is an OpenAI-STYLE model built from torch.nn.MultiheadAttention whose ``state_dict()`` carries that layout by
    construction; its own forward is the expected output.  Its state dict goes through
    ``convert_openai_state_dict`` into (a) HF ``CLIPModel`` and (b) the numpy oracle: both must reproduce it."""
    import torch

    from oracle import openai_clip_ref as R
    from plip_amd import weights as W
    from plip_amd.config import get_config
    cfg0 = get_config("tiny")
    ref = R.build_random(cfg0, seed=3)
    oa = R.numpy_state_dict(ref)
    assert oa["visual.transformer.resblocks.0.attn.in_proj_weight"].shape == (3 * cfg0.v_width, cfg0.v_width)
    assert oa["visual.proj"].shape == (cfg0.v_width, cfg0.projection_dim)
    assert W.is_openai_state_dict(oa)
    sd, cfg = W.normalize_state_dict(oa)
    assert cfg.eos_token_id == 2 and cfg.v_layers == cfg0.v_layers and cfg.t_heads == cfg0.t_heads
    rs = np.random.RandomState(4)
    px = rs.standard_normal((5, 3, cfg.image_size, cfg.image_size)).astype(np.float32)
    ids, _ = W.synthetic_ids(cfg0, 5, seed=6, pad="zero")           # clip.tokenize pads with 0, EOT = highest id
    with torch.no_grad():
        want_i = ref.encode_image(torch.from_numpy(px)).numpy()
        want_t = ref.encode_text(torch.from_numpy(ids)).numpy()
        want_lpi, want_lpt = (t.numpy() for t in ref(torch.from_numpy(px), torch.from_numpy(ids)))
    o = O.clip_forward(px, ids, sd, cfg, None)
    assert np.abs(o["image_features"] - want_i).max() < 2e-5
    assert np.abs(o["text_features"] - want_t).max() < 2e-5
    scale = float(np.exp(np.float64(sd["logit_scale"])))
    assert np.abs(o["logits_per_image"] - want_lpi).max() / scale < FP32_COS_TOL
    np.testing.assert_array_equal(want_lpi, want_lpt.T)
    if H.available():
        h = H.run(H.build_model(cfg, sd, "sdpa"), px, ids, None)
        assert np.abs(h["image_features"] - want_i).max() < 2e-5
        assert np.abs(h["text_features"] - want_t).max() < 2e-5
        assert np.abs(h["logits_per_image"] - want_lpi).max() / scale < FP32_COS_TOL
    # a converter that mis-ordered q|k|v or forgot a transpose must NOT pass: scramble and expect a visible miss
    bad = dict(oa)
    w = bad["visual.transformer.resblocks.0.attn.in_proj_weight"]
    D = w.shape[1]
    bad["visual.transformer.resblocks.0.attn.in_proj_weight"] = np.concatenate([w[D:2 * D], w[:D], w[2 * D:]], 0)
    sd_bad, _ = W.normalize_state_dict(bad)
    assert np.abs(O.vision_tower(px, sd_bad, cfg) - want_i).max() > 1e-3


def test_config3_zero_shot_fixture_is_the_reference_head(golden):
    """tests/golden/config3_zero_shot.npz (HF CLIPModel, oracle/make_config3_fixture.py): inputs regenerate from seeds, the
    oracle reproduces HF's scores on a few tiles, and the reference's head (zero_shot.py:12-13: dot product, per-row
    arg-max) populates at least five of the ten classes -- the property VERDICT r2 found missing."""
    from oracle.make_config3_fixture import tiles_to_pixels
    from plip_amd import weights as W
    from plip_amd.config import get_config
    g = golden("config3_zero_shot")
    tile_seed, prompt_seed, weight_seed, n, pool = (int(v) for v in g["seeds"])
    cfg = get_config("ViT-B/32")
    sd = W.synthetic_state_dict(cfg, weight_seed)
    u8 = W.synthetic_tiles(cfg, n, tile_seed)
    np.testing.assert_allclose([u8.astype(np.float64).sum(), (u8.astype(np.float64) ** 2).sum()], g["tiles_fingerprint"],
                               rtol=0, atol=0)
    cand, _ = W.synthetic_ids(cfg, pool, seed=prompt_seed)
    np.testing.assert_array_equal(cand[g["candidate_index"]], g["prompts"])
    rows = [0, 100, 511]
    img = O.l2_normalize(O.vision_tower(tiles_to_pixels(u8[rows]), sd, cfg))
    txt = O.l2_normalize(O.text_tower(g["prompts"], sd, cfg, None))
    assert np.abs(img @ txt.T - g["scores"][rows]).max() < FP32_COS_TOL
    np.testing.assert_array_equal(g["scores"].argmax(1), g["argmax"])
    hist = np.bincount(g["argmax"], minlength=10)
    assert (hist >= n // 25).sum() >= 5, hist


# ---- the oracle at the product's surface: activations, head sizes, resolutions, per-token outputs, token similarity ----------------
# Every committed HF fixture of those features against the extended oracle, under the f32 rows the fixtures' own GPU tests apply
# (tests/test_gpu_parity.py TOL, tests/test_gpu_tower_outputs.py TOL, tests/test_gpu_token_similarity.py HF_TOL and its caps,
# tests/test_gpu_attention_summary.py ROLLOUT_TOL and its cap).  The oracle runs in float32 unless a test says otherwise.
import hashlib  # noqa: E402
import os  # noqa: E402
import sys  # noqa: E402

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)

from attention_summary_refs import rollout_ref  # noqa: E402
from test_gpu_attention_summary import ROLLOUT_TOL  # noqa: E402
from test_gpu_parity import TOL as PARITY_TOL  # noqa: E402
from test_gpu_token_similarity import HF_TOL as SIM_TOL  # noqa: E402
from test_gpu_tower_outputs import TOL as TOWER_TOL  # noqa: E402

F32 = PARITY_TOL["f32"]


def _pair_fields(tag, o, g, sd, keys=("image_features", "text_features", "image_embeds", "text_embeds", "logits_per_image")):
    kind = {"image_features": "feat", "text_features": "feat", "image_embeds": "emb", "text_embeds": "emb", "logits_per_image": "cos"}
    for k in keys:
        div = np.exp(np.float64(sd["logit_scale"])) if k == "logits_per_image" else 1.0
        err = float(np.abs(o[k].astype(np.float64) - g[k]).max() / div)
        print(f"oracle vs HF {tag} {k}: {err:.2e} (bound {F32[kind[k]]:.1e})")
        assert err <= F32[kind[k]], (tag, k, err)


def test_defaults_give_the_bits_of_the_parent_oracle():
    """every call the oracle had before it learnt activations, resolutions and per-token outputs returns the same bits: sha256 over
    clip_forward, both towers with hidden states and the unmasked text tower of tiny_b6, float32 and float64, and over the
    precision model's three plans -- the digests are of the arrays the previous version of these modules returned"""
    from oracle import precision_model as P
    cfg, sd, px, ids, mask = case_inputs("tiny_b6")
    h = hashlib.sha256()
    for dt in (np.float32, np.float64):
        o = O.clip_forward(px, ids, sd, cfg, mask, dtype=dt)
        for k in sorted(o):
            h.update(np.ascontiguousarray(o[k]).tobytes())
        e, vh = O.vision_tower(px, sd, cfg, dt, return_hidden=True)
        h.update(e.tobytes())
        h.update(np.stack(vh).tobytes())
        e, th = O.text_tower(ids, sd, cfg, mask, dt, return_hidden=True)
        h.update(e.tobytes())
        h.update(np.stack(th).tobytes())
        h.update(O.text_tower(ids, sd, cfg, None, dt).tobytes())
    assert h.hexdigest() == "d0f5b3bbd69fc45c7d1334aad3a6a3268fd77855ceb6fbef0227a266ad7e5053"
    h = hashlib.sha256()
    for dt, plan in (("bf16", "folded"), ("f16", "folded"), ("bf16", "round_ln")):
        o = P.clip_forward(px, ids, sd, cfg, mask, plan, dtype=dt)
        for k in sorted(o):
            h.update(np.ascontiguousarray(o[k]).tobytes())
    e, th = P.text_tower(ids, sd, cfg, mask, return_hidden=True, lead_f16=1)
    h.update(e.tobytes())
    h.update(np.stack(th).tobytes())
    assert h.hexdigest() == "949613712008f2be0c97f23d0fd2b8ed704cc6c06a9e99644ab5be01d204f49e"


def test_gelu_is_the_erf_form():
    import math
    x = np.linspace(-6, 6, 241).astype(np.float32)
    want = np.array([0.5 * float(v) * (1.0 + math.erf(float(v) / math.sqrt(2.0))) for v in x])
    assert np.abs(O.gelu(x).astype(np.float64) - want).max() <= 2.0 ** -24 * 6
    assert O.gelu(x).dtype == np.float32 and O.gelu(x.astype(np.float64)).dtype == np.float64
    with pytest.raises(ValueError, match="hidden_act"):
        O.activation("gelu_new")


@pytest.mark.parametrize("name,v_act,t_act", [("gelu_tiny_b6", "gelu", "gelu"), ("gelu_tiny_b6_vision", "gelu", "quick_gelu"),
                                              ("gelu_tiny_b6_text", "quick_gelu", "gelu")])
def test_oracle_matches_hf_gelu_towers(name, v_act, t_act, golden):
    g = golden(name)
    cfg, sd, px, ids, mask = case_inputs("tiny_b6")
    cfg = cfg.replace(v_hidden_act=v_act, t_hidden_act=t_act)
    _pair_fields(name, O.clip_forward(px, ids, sd, cfg, mask), g, sd)
    if "vision_hidden" in g:
        _, vh = O.vision_tower(px, sd, cfg, return_hidden=True)
        _, th = O.text_tower(ids, sd, cfg, mask, return_hidden=True)
        assert np.abs(np.stack(vh) - g["vision_hidden"]).max() <= F32["hidden"]
        assert np.abs((np.stack(th) - g["text_hidden"]) * mask[None, :, :, None]).max() <= F32["hidden"]
    # the fixture separates the activations: the quick_gelu oracle misses the same bound on a field of each gelu tower
    q = O.clip_forward(px, ids, sd, cfg.replace(v_hidden_act="quick_gelu", t_hidden_act="quick_gelu"), mask)
    for tower, act in (("image", v_act), ("text", t_act)):
        assert (np.abs(q[f"{tower}_features"] - g[f"{tower}_features"]).max() > 30 * F32["feat"]) == (act == "gelu")


def test_oracle_matches_hf_gelu_at_144x128(golden):
    g = golden("gelu_tiny_144x128")
    cfg, sd, *_ = case_inputs("tiny_b6")
    cfg = cfg.replace(v_hidden_act="gelu", t_hidden_act="gelu")
    px = np.random.RandomState(int(g["seed"])).standard_normal(tuple(int(v) for v in g["shape"])).astype(np.float32)
    got = O.vision_tower(px, sd, cfg, image_hw=px.shape[2:])
    err = float(np.abs(got - g["image_features"]).max())
    print(f"oracle vs HF gelu 144x128 image_features: {err:.2e}")
    assert err <= F32["feat"]


@pytest.mark.parametrize("name", ["hd80", "hd88_p4", "text80", "hd128"])
def test_oracle_matches_hf_head_sizes(name, golden):
    import make_head_dim_golden as M
    g = golden(f"head_dim_{name}")
    cfg, sd, px, ids, mask = M.case_inputs(name)
    _pair_fields(name, O.clip_forward(px, ids, sd, cfg, mask), g, sd)
    _, vh = O.vision_tower(px, sd, cfg, return_hidden=True)
    vh = np.stack(vh)
    for key, rows in (("vision_hidden", vh), ("vision_hidden_cls", vh[:, :, 0]), ("vision_hidden_last_token", vh[:, :, -1])):
        if key in g:
            assert np.abs(rows - g[key]).max() <= F32["hidden"], (name, key)
    if "text_hidden" in g:
        _, th = O.text_tower(ids, sd, cfg, mask, return_hidden=True)
        assert np.abs((np.stack(th) - g["text_hidden"]) * mask[None, :, :, None]).max() <= F32["hidden"]
    if "res96/image_features" in g:
        got = O.vision_tower(M.res_pixels(), sd, cfg, image_hw=M.RES_HW)
        err = float(np.abs(got - g["res96/image_features"]).max())
        print(f"oracle vs HF {name} res96/image_features: {err:.2e}")
        assert err <= F32["feat"]


@pytest.mark.parametrize("size", ["448x448", "288x256", "250x250", "230x224", "160x160"])
def test_oracle_matches_hf_at_other_resolutions(size, golden):
    """ViT-B/32 with interpolate_pos_encoding=True: up- and down-scaled grids, a non-square one, a size that is no multiple of the
    patch (the grid floors; HF keeps its own table on the square 7 x 7) and 7 x 7 on a non-square image (resampled 7 -> 7)"""
    g = golden("vitb32_b4_resolutions")
    cfg, sd, _, ids, mask = case_inputs("vitb32_b4")
    shape = tuple(int(v) for v in g[f"{size}/shape"])
    px = np.random.RandomState(int(g[f"{size}/seed"])).standard_normal(shape).astype(np.float32)
    o = O.clip_forward(px, ids, sd, cfg, mask, image_hw=shape[2:])
    _pair_fields(size, o, {k: g[f"{size}/{k}"] for k in ("image_features", "image_embeds", "logits_per_image")}, sd,
                 ("image_features", "image_embeds", "logits_per_image"))


def _tower_fields(tag, out, g, prefix, tower):
    """tests/test_gpu_tower_outputs.py _compare on the oracle's fields: hid / last / pool relative to the field's largest magnitude,
    attn absolute"""
    t = TOWER_TOL["f32"]
    rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())
    errs = {"last": rel(out["last_hidden_state"], g[f"{prefix}/{tower}_last_hidden_state"]),
            "pool": rel(out["pooler_output"], g[f"{prefix}/{tower}_pooler_output"]),
            "hid": max(rel(out["hidden_states"][int(i)], g[f"{prefix}/{tower}_hidden_states"][k])
                       for k, i in enumerate(g[f"{prefix}/{tower}_hidden_idx"])),
            "attn": max(float(np.abs(np.asarray(out["attentions"][int(i)], np.float64) - g[f"{prefix}/{tower}_attentions"][k]).max())
                        for k, i in enumerate(g[f"{prefix}/{tower}_attn_idx"]))}
    print(f"oracle vs HF tower outputs {tag} {tower}: " + " ".join(f"{k} {v:.2e} (bound {t[k]:.1e})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= t[k], (tag, tower, k, v, t[k])


def _masked_entries_are_zero(att, mask, causal):
    for a in att:
        B, H, S, _ = a.shape
        dead = np.zeros((B, S, S), bool)
        if causal:
            dead |= np.triu(np.ones((S, S), bool), 1)[None]
        if mask is not None:
            dead |= (np.asarray(mask) == 0)[:, None, :]
        assert (a[np.broadcast_to(dead[:, None], a.shape)] == 0.0).all()
        np.testing.assert_allclose(a.sum(-1), 1.0, atol=1e-5, rtol=0)


def test_oracle_matches_hf_tower_outputs_tiny(golden):
    """every hidden state and attention map of both towers, last_hidden_state and pooler_output: captions under their mask, without
    one, and zero-padded captions (argmax pooling)"""
    g = golden("tower_outputs_tiny")
    cfg, sd, px, ids, mask = case_inputs("tiny_b6")
    _tower_fields("tiny", O.vision_outputs(px, sd, cfg, attentions=True), g, "eos_masked", "vision")
    t = O.text_outputs(ids, sd, cfg, mask, attentions=True)
    _tower_fields("tiny masked", t, g, "eos_masked", "text")
    _masked_entries_are_zero(t["attentions"], mask, True)
    t = O.text_outputs(ids, sd, cfg, None, attentions=True)
    _tower_fields("tiny unmasked", t, g, "eos_nomask", "text")
    _masked_entries_are_zero(t["attentions"], None, True)
    cfg, sd, px, ids, mask = case_inputs("tiny_b5_zero_pad_ln100")
    _tower_fields("tiny zero-pad", O.text_outputs(ids, sd, cfg, None, attentions=True), g, "zero", "text")
    # the tuple forms of the towers carry the same arrays
    emb, hid, att = O.text_tower(ids, sd, cfg, None, return_hidden=True, return_attentions=True)
    assert len(hid) == cfg.t_layers + 1 and len(att) == cfg.t_layers and att[0].shape == (5, cfg.t_heads, 16, 16)
    emb2, att2 = O.vision_tower(px, sd, cfg, return_attentions=True)
    assert emb2.shape == (5, cfg.projection_dim) and len(att2) == cfg.v_layers


def test_oracle_matches_hf_token_similarity_tiny(golden):
    g = golden("token_similarity_tiny")
    cfg, sd, px, ids, mask = case_inputs("tiny_b6")
    T = golden("tiny_b6")["text_embeds"]
    last = O.vision_outputs(px, sd, cfg)["last_hidden_state"]
    E, s = O.token_similarity(last, sd, cfg, T)
    emax = float(np.abs(g["token_embeds"]).max())
    err_e = float(np.abs(E.astype(np.float64) - g["token_embeds"]).max()) / emax
    err_s = float(np.abs(s.astype(np.float64) - g["similarity"]).max())
    cap_e = 0.1 * float(g["token_embeds"].astype(np.float64).std()) / emax
    cap_s = 0.1 * float(g["similarity"][:, 1:].astype(np.float64).std())
    print(f"oracle vs HF token similarity: token_embeds {err_e:.2e}, similarity {err_s:.2e}")
    assert err_e <= min(SIM_TOL["embeds"]["f32"], cap_e) and err_s <= min(SIM_TOL["similarity"]["f32"], cap_s)
    # text rows of any norm give the same scores; the scale multiplies them; softmax runs over the prompts
    scaled = T * np.logspace(-2, 2, T.shape[0], dtype=np.float32)[:, None]
    assert np.abs(O.token_similarity(last, sd, cfg, scaled)[1] - s).max() <= 4 * 2.0 ** -24
    s100 = O.token_similarity(last, sd, cfg, T, scale=100.0, dtype=np.float64)[1]
    sm = O.token_similarity(last, sd, cfg, T, scale=100.0, softmax=True, dtype=np.float64)[1]
    e = np.exp(s100 - s100.max(-1, keepdims=True))
    np.testing.assert_allclose(sm, e / e.sum(-1, keepdims=True), rtol=0, atol=1e-15)
    # row 0 is the pooled row: its scores are the pair's cosines
    assert np.abs(s[:, 0] - golden("tiny_b6")["image_embeds"] @ T.T).max() <= F32["cos"]


def test_oracle_matches_hf_attention_summary_tinyp4(golden):
    """257 vision tokens: the pooled rows of every block and the rollout (tests/attention_summary_refs.rollout_ref on the oracle's
    probabilities) against HF's"""
    g = golden("attention_summary_tinyp4")
    cfg, sd, px, ids, mask = case_inputs("tinyp4_b3")
    att = O.vision_outputs(px, sd, cfg, attentions=True)["attentions"]
    L = len(att)
    e_pool = max(float(np.abs(att[l][:, :, 0, :].astype(np.float64) - g["vision_pooled_attention"][l]).max()) for l in range(L))
    R = rollout_ref(att)
    e_mat = float(np.abs(R - g["vision_rollout_matrix"]).max())
    e_row = float(np.abs(R[:, 0] - g["vision_rollout"]).max())
    print(f"oracle vs HF attention summary tinyp4: pooled {e_pool:.2e} rollout_matrix {e_mat:.2e} rollout {e_row:.2e}")
    assert e_pool <= TOWER_TOL["f32"]["attn"]
    assert max(e_mat, e_row) <= min(ROLLOUT_TOL["f32"], L * TOWER_TOL["f32"]["attn"])
