"""The draw of the feature-combination sweep (tests/feature_sweep_common.py), checked without a GPU: every case is legal, every
value of every drawn dimension occurs, the feature PAIRS the sweep exists for occur, and the extended oracle is fast enough on
every case.  These are conditions on the draw: ``feature_sweep_common.BASE`` was picked so that they hold."""
import time

import numpy as np
import pytest

import feature_sweep_common as F

CASES = [F.draw_case(s) for s in range(F.N_CASES)]


def _count(pred):
    return sum(1 for c in CASES if pred(*c))


def _in_between(cfg, kw):
    return 0 < kw.get("text_f16_layers", 0) < cfg.t_layers


def test_the_draw_is_deterministic_and_legal():
    for s, (cfg, B, kw, probes, ws) in enumerate(CASES):
        cfg.validate()
        assert F.draw_case(s) == (cfg, B, kw, probes, ws)
        assert 1 <= B <= 9 and 1 <= cfg.v_layers <= 3 and 1 <= cfg.t_layers <= 3
        assert cfg.head_dim in (64, 80, 88, 96, 112, 128) and cfg.t_head_dim in (64, 80, 96, 112)
        assert cfg.v_tokens <= 145 and 5 <= cfg.context_length <= 160 and 32 <= cfg.projection_dim <= 256
        assert not (kw.get("text_f16") and "text_f16_layers" in kw)
        assert 0 <= kw.get("text_f16_layers", 0) <= cfg.t_layers
        if kw.get("pack_captions"):      # where csrc/handle_host.h and csrc/towers.hip Forward let the packed rows run
            assert cfg.t_head_dim == 64 and cfg.context_length <= 128
            assert not {"ln_fold", "pooled_last_block", "mfma_attention"} & set(kw)
        if probes["image_hw"]:
            h, w = probes["image_hw"]
            assert h != w and h >= cfg.patch_size and w >= cfg.patch_size
            assert (h // cfg.patch_size) * (w // cfg.patch_size) + 1 <= 145
            assert (h, w) != (cfg.image_size, cfg.image_size)
        for dtype in ("f32", "bf16", "f16"):
            k = F.engine_kwargs_for(dtype, kw)
            assert dtype == "bf16" or not ({"text_f16", "text_f16_layers"} & set(k))
            assert dtype != "f32" or set(k) <= {"graph_batch"}


def test_every_value_occurs():
    need = {}
    for hd in (64, 80, 96, 112, 128):
        need[f"vision head {hd}"] = lambda cfg, *_, hd=hd: cfg.head_dim == hd
    for hd in (64, 80, 96, 112):
        need[f"text head {hd}"] = lambda cfg, *_, hd=hd: cfg.t_head_dim == hd
    for kc in ("all", "none", "mixed"):
        need[f"K {kc}"] = lambda cfg, *_, kc=kc: F.k_class_of(cfg) == kc
    for act in ("gelu", "quick_gelu"):
        need[f"vision {act}"] = lambda cfg, *_, act=act: cfg.v_hidden_act == act
        need[f"text {act}"] = lambda cfg, *_, act=act: cfg.t_hidden_act == act
    for p in F.PATCHES:
        need[f"patch {p}"] = lambda cfg, *_, p=p: cfg.patch_size == p
    for g in range(2, 10):
        need[f"grid {g}"] = lambda cfg, *_, g=g: cfg.grid == g
    need["ctx 5..100"] = lambda cfg, *_: cfg.context_length <= 100
    need["ctx 65..80 on text head 64"] = lambda cfg, *_: 65 <= cfg.context_length <= 80 and cfg.t_head_dim == 64
    need["ctx 129..160"] = lambda cfg, *_: cfg.context_length >= 129
    for p in F.PROJECTIONS:
        need[f"projection {p}"] = lambda cfg, *_, p=p: cfg.projection_dim == p
    for n in (1, 2, 3):
        need[f"v_layers {n}"] = lambda cfg, *_, n=n: cfg.v_layers == n
        need[f"t_layers {n}"] = lambda cfg, *_, n=n: cfg.t_layers == n
    for b in range(1, 10):
        need[f"batch {b}"] = lambda cfg, B, *_, b=b: B == b
    for sw in ("ln_fold", "pooled_last_block", "mfma_attention"):
        need[f"{sw}=False"] = lambda cfg, B, kw, *_, sw=sw: kw.get(sw) is False
        need[f"{sw} default"] = lambda cfg, B, kw, *_, sw=sw: sw not in kw
    need["graph_batch=0"] = lambda cfg, B, kw, *_: kw.get("graph_batch") == 0
    need["text_f16"] = lambda cfg, B, kw, *_: kw.get("text_f16") is True
    need["text_f16_layers 0"] = lambda cfg, B, kw, *_: kw.get("text_f16_layers") == 0
    need["text_f16_layers in between"] = lambda cfg, B, kw, *_: _in_between(cfg, kw)
    need["text_f16_layers all"] = lambda cfg, B, kw, *_: kw.get("text_f16_layers") == cfg.t_layers
    need["pack_captions"] = lambda cfg, B, kw, *_: kw.get("pack_captions") is True
    need["latency_batch 8"] = lambda cfg, B, kw, *_: kw.get("latency_batch") == 8
    need["latency_batch 0"] = lambda cfg, B, kw, *_: "latency_batch" not in kw
    for pad in ("eos", "zero"):
        for use in (True, False):
            need[f"pad {pad} mask {use}"] = lambda cfg, B, kw, pr, *_, pad=pad, use=use: pr["pad"] == pad and pr["use_mask"] == use
    need["softmax"] = lambda cfg, B, kw, pr, *_: pr["softmax"]
    short = {name: _count(pred) for name, pred in need.items() if _count(pred) < 3}
    assert not short, short
    assert _count(lambda cfg, *_: cfg.head_dim == 88 and cfg.v_layers == 1) >= 2
    assert _count(lambda cfg, *_: cfg.v_tokens >= 145) >= F.N_CASES // 5
    assert all(CASES[s][0].v_tokens >= 145 for s in range(0, F.N_CASES, 5))
    assert _count(lambda cfg, *_: cfg.projection_dim % 32 == 0) >= 3 and _count(lambda cfg, *_: cfg.projection_dim % 32) >= 3
    # non-native sizes: about a third, all non-square; one whose width is no multiple of 4, one that the im2col-on-load patch GEMM
    # takes on a 16-bit engine (csrc/gemm.hip gemm_gather_supports: patch 16 / 32, width % 4 == 0, v_width % 256 == 0)
    res = [(cfg, pr["image_hw"]) for cfg, B, kw, pr, ws in CASES if pr["image_hw"]]
    assert F.N_CASES // 4 <= len(res) <= F.N_CASES // 2
    assert any(hw[1] % 4 for cfg, hw in res)
    assert any(hw[1] % 4 == 0 and cfg.v_width % 256 == 0 and cfg.patch_size in (16, 32) for cfg, hw in res)
    assert any(not (hw[1] % 4 == 0 and cfg.v_width % 256 == 0 and cfg.patch_size in (16, 32)) for cfg, hw in res)


def test_the_pairs_the_sweep_exists_for_occur():
    gelu = lambda cfg: "gelu" in (cfg.v_hidden_act, cfg.t_hidden_act)
    odd_head = lambda cfg: cfg.head_dim != 64 or cfg.t_head_dim != 64
    lat = lambda kw: kw.get("latency_batch") == 8
    pairs = {
        "gelu x latency": lambda cfg, B, kw, pr, ws: gelu(cfg) and lat(kw),
        "gelu x text_f16_layers in between": lambda cfg, B, kw, pr, ws: cfg.t_hidden_act == "gelu" and _in_between(cfg, kw),
        "head != 64 x non-native size": lambda cfg, B, kw, pr, ws: cfg.head_dim != 64 and pr["image_hw"] is not None,
        "head != 64 x latency": lambda cfg, B, kw, pr, ws: odd_head(cfg) and lat(kw),
        "latency x mixed K": lambda cfg, B, kw, pr, ws: lat(kw) and F.k_class_of(cfg) == "mixed",
        "latency x text_f16_layers in between": lambda cfg, B, kw, pr, ws: lat(kw) and _in_between(cfg, kw),
        "packing x gelu": lambda cfg, B, kw, pr, ws: kw.get("pack_captions") and cfg.t_hidden_act == "gelu",
        "packing x fused-range context": lambda cfg, B, kw, pr, ws: kw.get("pack_captions") and 65 <= cfg.context_length <= 80,
        "more than 128 tokens x head != 64": lambda cfg, B, kw, pr, ws: (cfg.v_tokens > 128 and cfg.head_dim != 64) or
                                                                        (cfg.context_length > 128 and cfg.t_head_dim != 64),
        "mfma_attention=False x head != 64": lambda cfg, B, kw, pr, ws: kw.get("mfma_attention") is False and odd_head(cfg),
    }
    short = {name: _count(pred) for name, pred in pairs.items() if _count(pred) < 2}
    assert not short, short


@pytest.mark.parametrize("seed", range(F.N_CASES))
def test_the_oracle_is_fast_on_every_case(seed):
    t0 = time.perf_counter()
    o = F.oracle_fields(seed, np.float32)
    dt = time.perf_counter() - t0
    cfg, B, kw, probes, ws = CASES[seed]
    assert np.isfinite(o["logits_per_image"]).all() and o["logits_per_image"].shape == (B, B)
    assert len(o["vision"]["attentions"]) == cfg.v_layers and o["text"]["attentions"][0].shape == (B, cfg.t_heads, cfg.context_length,
                                                                                                 cfg.context_length)
    assert (o["res_image_features"].shape == (B, cfg.projection_dim)) if probes["image_hw"] else "res_image_features" not in o
    assert dt < 3.0, (seed, dt, cfg, B)
