"""Shared by tests/test_feature_sweep_host.py and tests/test_gpu_feature_sweep.py: the draw of the feature-combination sweep and the
CPU references of a case.

``draw_case(seed)`` -> ``(cfg, batch, engine_kwargs, probes, weight_seed)`` for ``seed`` in ``range(N_CASES)``: a random dual encoder
small enough for the numpy oracle, with every product switch drawn together -- head sizes other than 64, the erf GELU per tower, a
non-native image size, the split-K latency path, mixed f16 / bf16 text blocks, caption packing, the A/B forms.  Deterministic, and legal
by construction: it knows what csrc/handle_host.h validate_config and PlipConfig.validate refuse (head sizes 64 .. 128 / 120 in steps of
8, widths and MLP sizes multiples of 128, packing only on 64-wide text heads with the folded LayerNorm and the pooled last block,
``text_f16`` excluding ``text_f16_layers``), so no case is ever skipped.

Balanced dimensions come from fixed permutations of the case numbers (every value of a dimension occurs about equally often whatever
the base); the rest from ``RandomState(BASE + seed)``.  ``BASE`` was picked so that the pair conditions of
tests/test_feature_sweep_host.py hold; they are conditions on this draw, not measurements.
"""
import functools

import numpy as np

from plip_amd import weights as W
from plip_amd.config import PlipConfig

N_CASES = 40
BASE = 9107

# (width, heads) per head size.  Vision also has 88 = 1408 / 16 (ViT-g/14's), in HD88_SEEDS only and one block deep: a 1408-wide
# block is most of a case's oracle time.  The text tower goes up to 112 (120 would need a 1920-wide tower: the kernel tests have it).
V_PAIRS = [(128, 2), (256, 4), (384, 6), (640, 8), (384, 4), (896, 8), (256, 2), (512, 4)]
T_PAIRS = [(128, 2), (256, 4), (384, 6), (512, 8), (640, 8), (384, 4), (896, 8)]
HD88 = (1408, 16)
HD88_SEEDS = (9, 29)
PATCHES = [4, 8, 14, 16, 32]
PROJECTIONS = [32, 64, 80, 96, 200, 256]
K_CLASSES = ["all", "none", "mixed", "free"]       # which GEMM K of the towers are multiples of 256 (the split-K kernel's condition)
CTX_CLASSES = ["short", "short", "short", "fused", "fused", "long", "short"]     # 5 .. 100; 65 .. 80 on 64-wide text heads; 129 .. 160


@functools.lru_cache(maxsize=None)
def _table(j):
    return np.random.RandomState(BASE + 1000 + j).permutation(N_CASES)


def _balanced(seed, j, values):
    """value of balanced dimension ``j`` for this case: every value occurs N_CASES // len(values) times or once more"""
    return values[int(_table(j)[seed]) % len(values)]


def k_class_of(cfg):
    """"all" / "none" / "mixed": which of the towers' GEMM reduction sizes (the widths: q/k/v, out-proj, fc1; the MLP sizes: fc2) are
    multiples of 256 -- on the latency path those GEMMs take the split-K kernel, the others the tiled one"""
    ks = [cfg.v_width % 256 == 0, cfg.v_mlp % 256 == 0, cfg.t_width % 256 == 0, cfg.t_mlp % 256 == 0]
    return "all" if all(ks) else "none" if not any(ks) else "mixed"


def _mlp(rs, width, kc):
    if kc == "all":
        return 256 * int(rs.randint(1, 4))
    if kc == "none":
        return 128 * int(rs.choice([1, 3, 5]))
    if kc == "mixed":           # the other parity than the width's
        return 128 * int(rs.choice([1, 3, 5])) if width % 256 == 0 else 256 * int(rs.randint(1, 4))
    return 128 * int(rs.randint(1, 6))


def _pairs(pairs, kc, head64):
    ok = [p for p in pairs if (kc != "all" or p[0] % 256 == 0) and (kc != "none" or p[0] % 256) and (not head64 or p[0] // p[1] == 64)]
    return ok or [p for p in pairs if not head64 or p[0] // p[1] == 64]


def draw_case(seed):
    assert 0 <= seed < N_CASES
    rs = np.random.RandomState(BASE + seed)
    kc = _balanced(seed, 0, K_CLASSES)
    ctx_class = _balanced(seed, 1, CTX_CLASSES)
    v_pairs = _pairs(V_PAIRS, kc, False)
    vw, vh = HD88 if seed in HD88_SEEDS else v_pairs[int(_table(2)[seed]) % len(v_pairs)]
    t_pairs = _pairs(T_PAIRS, kc, ctx_class == "fused")
    tw, th = t_pairs[int(_table(3)[seed]) % len(t_pairs)]
    patch = _balanced(seed, 4, PATCHES)
    grid = 12 if seed % 5 == 0 else _balanced(seed, 5, list(range(2, 10)))       # every fifth case: 145 vision tokens
    ctx = int({"short": rs.randint(5, 101), "fused": rs.randint(65, 81), "long": rs.randint(129, 161)}[ctx_class])
    v_layers = 1 if seed in HD88_SEEDS else _balanced(seed, 6, [1, 2, 3])
    t_layers = _balanced(seed, 7, [1, 2, 3])
    batch = _balanced(seed, 8, list(range(1, 10)))
    # the oracle's time: the widest towers on the most tokens run fewer blocks on fewer samples (the checks stay the same)
    if vw >= 896 and grid >= 8:
        v_layers, batch = min(v_layers, 2), min(batch, 5)
    if tw >= 896 and ctx > 100:
        t_layers, batch = min(t_layers, 2), min(batch, 5)
    vocab = int(rs.randint(300, 2000))
    cfg = PlipConfig(image_size=patch * grid, patch_size=patch, v_width=vw, v_layers=v_layers, v_heads=vh, v_mlp=_mlp(rs, vw, kc),
                     vocab_size=vocab, context_length=ctx, t_width=tw, t_layers=t_layers, t_heads=th, t_mlp=_mlp(rs, tw, kc),
                     projection_dim=_balanced(seed, 9, PROJECTIONS), eos_token_id=vocab - 1, bos_token_id=vocab - 2,
                     v_hidden_act=_balanced(seed, 10, ["gelu", "quick_gelu"]), t_hidden_act=_balanced(seed, 11, ["quick_gelu", "gelu"]))
    kw = {}
    if _balanced(seed, 12, [True, False, False]):
        kw["ln_fold"] = False
    if _balanced(seed, 13, [True, False, False]):
        kw["pooled_last_block"] = False
    if _balanced(seed, 14, [True, False, False]):
        kw["mfma_attention"] = False
    if _balanced(seed, 15, [True, False, False]):
        kw["graph_batch"] = 0
    if _balanced(seed, 16, [True, False, False, False]):
        kw["text_f16"] = True                                       # bf16 engine only; excludes text_f16_layers
    else:
        kw["text_f16_layers"] = int(_table(17)[seed]) % (t_layers + 1)           # bf16 engine only; 0 .. t_layers
    if _balanced(seed, 18, [True, False]):
        kw["latency_batch"] = 8
    # packing: 16-bit engines with the folded LayerNorm, the pooled last block and the MFMA attention, 64-wide text heads, captions of
    # at most 128 tokens (validate_config refuses other head sizes by name; the other conditions turn it off silently)
    pack_legal = not ({"ln_fold", "pooled_last_block", "mfma_attention"} & set(kw)) and tw // th == 64 and ctx <= 128
    if pack_legal and _balanced(seed, 19, [True, True, False]):
        kw["pack_captions"] = True
    probes = {"pad": "eos" if seed % 2 else "zero", "use_mask": bool(seed % 3), "softmax": bool(_balanced(seed, 20, [True, False])),
              "image_hw": None}
    if _balanced(seed, 21, [True, False, False]):
        # a non-native, non-square size: the grid floors; about every other one has sides that are no multiple of the patch
        # (a width that is no multiple of 4 keeps the patch GEMM off the im2col-on-load route)
        gh, gw = (int(v) for v in rs.choice(np.arange(2, 10), size=2, replace=False))
        extra = rs.rand() < 0.5
        h = patch * gh + (int(rs.randint(0, patch)) if extra else 0)
        w = patch * gw + (int(rs.randint(1, patch)) if extra else 0)
        probes["image_hw"] = (h, w)
    return cfg, batch, kw, probes, int(rs.randint(0, 1 << 30))


def engine_kwargs_for(dtype, kw):
    """the switches a dtype has (as tests/test_gpu_random_archs.py drops them): the fp32 engine has no A/B forms, no packing and no
    latency path; ``text_f16`` / ``text_f16_layers`` are modes of the bf16 engine"""
    if dtype == "f32":
        return {k: v for k, v in kw.items() if k == "graph_batch"}
    return {k: v for k, v in kw.items() if dtype == "bf16" or k not in ("text_f16", "text_f16_layers")}


def case_inputs(seed):
    cfg, B, kw, probes, s = draw_case(seed)
    sd = W.synthetic_state_dict(cfg, s)
    px = W.synthetic_pixels(cfg, B, s + 1)
    ids, mask = W.synthetic_ids(cfg, B, s + 2, pad=probes["pad"])
    px_res = None
    if probes["image_hw"] is not None:
        px_res = np.random.RandomState(s + 3).standard_normal((B, 3) + probes["image_hw"]).astype(np.float32)
    return cfg, B, kw, probes, sd, px, ids, mask, px_res


def oracle_fields(seed, dtype=np.float32):
    """the extended oracle on a case, every field the sweep compares, in ``dtype``"""
    from oracle import clip_oracle as O
    cfg, B, kw, probes, sd, px, ids, mask, px_res = case_inputs(seed)
    use_mask = mask if probes["use_mask"] else None
    v = O.vision_outputs(px, sd, cfg, dtype, attentions=True)
    t = O.text_outputs(ids, sd, cfg, use_mask, dtype, attentions=True)
    img, txt = O.l2_normalize(v["image_features"]), O.l2_normalize(t["text_features"])
    scale = np.exp(dtype(sd["logit_scale"]))
    out = {"vision": v, "text": t, "image_features": v["image_features"], "text_features": t["text_features"],
           "logits_per_image": (img @ txt.T) * scale}
    # the dense head at scale 1, and its softmax over the prompts at the model's logit scale
    out["token_embeds"], out["similarity"] = O.token_similarity(v["last_hidden_state"], sd, cfg, t["text_features"], dtype=dtype)
    out["similarity_softmax"] = O.token_similarity(v["last_hidden_state"], sd, cfg, t["text_features"], float(scale), True, dtype)[1]
    if px_res is not None:
        out["res_image_features"] = O.vision_tower(px_res, sd, cfg, dtype, image_hw=probes["image_hw"])
    return out


def precision_fields(seed, dtype):
    """oracle/precision_model.py on a case: all six rounding sites, the engine's operand type ("bf16" / "f16"), the LayerNorm plan
    and the f16 lead blocks its switches select -- the per-token fields and the token similarity"""
    from oracle import clip_oracle as O
    from oracle import precision_model as P
    cfg, B, kw, probes, sd, px, ids, mask, px_res = case_inputs(seed)
    kw = engine_kwargs_for(dtype, kw)
    plan = "folded" if kw.get("ln_fold", True) else "round_ln"
    use_mask = mask if probes["use_mask"] else None
    v = P.vision_outputs(px, sd, cfg, plan, dtype, attentions=True)
    t = P.text_outputs(ids, sd, cfg, use_mask, plan, "f16" if kw.get("text_f16") else dtype, lead_f16=kw.get("text_f16_layers", 0),
                       attentions=True)
    out = {"vision": v, "text": t}
    scale = float(np.exp(np.float64(sd["logit_scale"])))
    # the head is fp32 on every engine; the text rows are the float64 oracle's (the test hands the engine those)
    T = oracle_fields_cached(seed, "f64")["text_features"].astype(np.float32)
    out["token_embeds"], out["similarity"] = O.token_similarity(v["last_hidden_state"], sd, cfg, T, dtype=np.float64)
    out["similarity_softmax"] = O.token_similarity(v["last_hidden_state"], sd, cfg, T, scale, True, np.float64)[1]
    return out


@functools.lru_cache(maxsize=4)
def oracle_fields_cached(seed, name):
    return oracle_fields(seed, {"f32": np.float32, "f64": np.float64}[name])


def tower_errors(got, ref):
    """the four figures tests/test_gpu_tower_outputs.py compares, of one tower's fields ``got`` against ``ref`` (dicts of
    last_hidden_state, pooler_output, hidden_states, attentions): attn max-abs on the probabilities, hid / last / pool relative to
    the reference field's largest magnitude"""
    f64 = lambda a: np.asarray(a, np.float64)
    rel = lambda a, b: float(np.abs(f64(a) - f64(b)).max() / np.abs(f64(b)).max())
    return {"last": rel(got["last_hidden_state"], ref["last_hidden_state"]), "pool": rel(got["pooler_output"], ref["pooler_output"]),
            "hid": max(rel(a, b) for a, b in zip(got["hidden_states"], ref["hidden_states"])),
            "attn": max(float(np.abs(f64(a) - f64(b)).max()) for a, b in zip(got["attentions"], ref["attentions"]))}


def similarity_errors(got, ref):
    """token_embeds relative to the reference's largest magnitude, similarity (and its softmax) max-abs, as
    tests/test_gpu_token_similarity.py measures them; ``got`` / ``ref``: dicts of token_embeds, similarity, similarity_softmax"""
    f64 = lambda a: np.asarray(a, np.float64)
    return {"embeds": float(np.abs(f64(got["token_embeds"]) - f64(ref["token_embeds"])).max() / np.abs(f64(ref["token_embeds"])).max()),
            "similarity": float(np.abs(f64(got["similarity"]) - f64(ref["similarity"])).max()),
            "softmax": float(np.abs(f64(got["similarity_softmax"]) - f64(ref["similarity_softmax"])).max())}
