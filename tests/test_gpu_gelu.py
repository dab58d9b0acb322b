"""Exact-GELU towers end to end: engines built from configs that say ``hidden_act="gelu"`` against HF ``CLIPModel`` with the same
activation (tests/golden/gelu_*.npz, tools/make_gelu_golden.py), with the bars of tests/test_gpu_parity.py.

Every fixture also holds HF's outputs for the same weights under quick_gelu and the gap ``d`` between the two.  The fp32 engine must
meet its bars against the gelu fixture; the same engine built as quick_gelu must miss them -- by more than 100 x on the fields listed in
``separates/f32`` (where HF's own two runs are that far apart), and on every field by at least ``d - bar`` (it matches HF's quick_gelu
run within the bar, so it is at least that far from the gelu one; d is at least 30 x the bar everywhere).  HF's own numbers do not put
every field 100 x apart: ViT-B/32 cosine logits differ by 73 x their bar, image_embeds by 96 x, hidden rows by 37 .. 92 x.
The 16-bit engines meet TOL / TINY, and are nearer to gelu than to quick_gelu (error below d / 3) on the fields the maker marked."""
import numpy as np
import pytest
import torch

from oracle.make_golden import case_inputs
from test_gpu_parity import TINY, TOL

pytestmark = pytest.mark.gpu

F32 = TOL["f32"]
KIND = {"image_features": "feat", "text_features": "feat", "image_embeds": "emb", "text_embeds": "emb", "logits_per_image": "cos",
        "vision_hidden": "hidden", "text_hidden": "hidden", "vision_hidden_cls": "hidden", "vision_hidden_last_token": "hidden",
        "text_hidden_bos": "hidden", "text_hidden_tok1": "hidden"}
ROW_LAYERS = (0, 1, 6, 12)
# fixture -> (golden case of its weights and inputs, vision activation, text activation)
FIXTURES = {"gelu_tiny_b6": ("tiny_b6", "gelu", "gelu"), "gelu_tiny_b6_vision": ("tiny_b6", "gelu", "quick_gelu"),
            "gelu_tiny_b6_text": ("tiny_b6", "quick_gelu", "gelu"), "gelu_vitb32_b4": ("vitb32_b4", "gelu", "gelu")}


def _bars(fixture, dtype):
    return F32 if dtype == "f32" else (TINY if "tiny" in fixture else TOL)[dtype]


@pytest.fixture(scope="module")
def gelu_models():
    """PlipModel per (golden case, dtype, vision act, text act), built through the public keyword and closed with the module"""
    from plip_amd.model import PlipModel
    cache = {}

    def get(case, dtype, v_act, t_act):
        key = (case, dtype, v_act, t_act)
        if key not in cache:
            cfg, sd, *_ = case_inputs(case)
            cache[key] = PlipModel.from_state_dict(sd, cfg, hidden_act=(v_act, t_act), dtype=dtype, max_batch=32)
            assert (cache[key].config.v_hidden_act, cache[key].config.t_hidden_act) == (v_act, t_act)
        return cache[key]

    yield get
    for m in cache.values():
        m.engine.close()


def _errors(model, fixture, g, hidden=True):
    """max |engine - fixture| of every field the fixture stores (logits as cosines; text hidden rows under the mask)"""
    case = FIXTURES[fixture][0]
    cfg, sd, px, ids, mask = case_inputs(case)
    np.testing.assert_array_equal(g["ids"], ids)
    tpx, tids, tmask = torch.from_numpy(px), torch.from_numpy(ids), torch.from_numpy(mask)
    err = {"image_features": np.abs(model.get_image_features(pixel_values=tpx).cpu().numpy() - g["image_features"]).max(),
           "text_features": np.abs(model.get_text_features(input_ids=tids, attention_mask=tmask).cpu().numpy() - g["text_features"]).max()}
    out = model(input_ids=tids, pixel_values=tpx, attention_mask=tmask)
    err["image_embeds"] = np.abs(out.image_embeds.cpu().numpy() - g["image_embeds"]).max()
    err["text_embeds"] = np.abs(out.text_embeds.cpu().numpy() - g["text_embeds"]).max()
    err["logits_per_image"] = np.abs(out.logits_per_image.cpu().numpy() - g["logits_per_image"]).max() / np.exp(np.float64(sd["logit_scale"]))
    assert torch.equal(out.logits_per_image, out.logits_per_text.T.contiguous())
    eng = model.engine
    if hidden and "vision_hidden" in g:
        m = mask[:, :, None].astype(np.float32)
        err["vision_hidden"] = max(np.abs(eng.hidden("vision", l, tpx).cpu().numpy() - g["vision_hidden"][l]).max() for l in range(cfg.v_layers + 1))
        err["text_hidden"] = max(np.abs((eng.hidden("text", l, tids).cpu().numpy() - g["text_hidden"][l]) * m).max() for l in range(cfg.t_layers + 1))
    elif hidden and "vision_hidden_cls" in g:
        for key, tower, inp, row in (("vision_hidden_cls", "vision", tpx, 0), ("vision_hidden_last_token", "vision", tpx, -1),
                                     ("text_hidden_bos", "text", tids, 0), ("text_hidden_tok1", "text", tids, 1)):
            err[key] = max(np.abs(eng.hidden(tower, l, inp)[:, row].cpu().numpy() - g[key][l]).max() for l in ROW_LAYERS)
    return {k: float(v) for k, v in err.items()}


def _hidden_bar(fixture, bars):
    # test_gpu_parity.py test_hidden_states_vitb32 applies 4 x the bar to the stored rows of the full model (scale 1 on these weights)
    return bars["hidden"] * (1 if "tiny" in fixture else 4)


def _assert_meets(fixture, dtype, err):
    bars = _bars(fixture, dtype)
    for k, e in err.items():
        bar = _hidden_bar(fixture, bars) if KIND[k] == "hidden" else bars[KIND[k]]
        print(f"PARITY group=gelu_e2e case={fixture}_{dtype} field={k} bound={bar:.3e} gpu={e:.3e}")
    for k, e in err.items():
        bar = _hidden_bar(fixture, bars) if KIND[k] == "hidden" else bars[KIND[k]]
        assert e < bar, (fixture, dtype, k, e, bar)


@pytest.mark.parametrize("fixture", ["gelu_tiny_b6", "gelu_vitb32_b4"])
def test_fp32_engine_meets_the_gelu_fixture_and_a_quick_gelu_engine_misses_it(fixture, gelu_models, engines, golden):
    """FAILS WITHOUT THE FEATURE: an engine that ignores ``hidden_act`` is the quick_gelu engine of the second half."""
    g = golden(fixture)
    case = FIXTURES[fixture][0]
    _assert_meets(fixture, "f32", _errors(gelu_models(case, "f32", "gelu", "gelu"), fixture, g))
    quick = _errors(engines(case, "f32")[0], fixture, g)
    separates = [str(k) for k in g["separates/f32"]]
    assert separates and {"image", "text"} <= {k.split("_")[0] for k in separates}
    for k, e in quick.items():
        bar, d = F32[KIND[k]], float(g[f"gap/{k}"])
        print(f"PARITY group=gelu_e2e_quick case={fixture}_f32 field={k} bar={bar:.1e} quick_gelu_engine={e:.3e} ({e / bar:.0f} x) hf_gap={d:.3e}")
        assert d >= 30 * bar and e >= d - bar, (k, e, d, bar)
        if k in separates:
            assert e > 100 * bar, (k, e, bar)


@pytest.mark.parametrize("fixture", ["gelu_tiny_b6_vision", "gelu_tiny_b6_text"])
def test_mixed_towers_meet_their_fixtures_fp32(fixture, gelu_models, golden):
    """one tower gelu, the other quick_gelu: a flag applied to the wrong tower (or to both) misses these by the HF gap"""
    case, v_act, t_act = FIXTURES[fixture]
    g = golden(fixture)
    _assert_meets(fixture, "f32", _errors(gelu_models(case, "f32", v_act, t_act), fixture, g))
    # ... and the swapped engine does miss: the fixture tells the towers apart
    swapped = _errors(gelu_models(case, "f32", t_act, v_act), fixture, g)
    for k in (str(k) for k in g["separates/f32"]):
        assert swapped[k] > 100 * F32[KIND[k]], (k, swapped[k])


@pytest.mark.parametrize("fixture", ["gelu_tiny_b6", "gelu_vitb32_b4"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_16bit_engines_meet_their_bars_and_are_nearer_to_gelu(dtype, fixture, gelu_models, golden):
    g = golden(fixture)
    err = _errors(gelu_models(FIXTURES[fixture][0], dtype, "gelu", "gelu"), fixture, g)
    _assert_meets(fixture, dtype, err)
    for k in (str(k) for k in g[f"marked/{dtype}"]):
        d = float(g[f"gap/{k}"])
        print(f"PARITY group=gelu_e2e_nearer case={fixture}_{dtype} field={k} bound={d / 3:.3e} gpu={err[k]:.3e}")
        assert err[k] < d / 3, (k, err[k], d)
    if fixture == "gelu_vitb32_b4":
        assert "text_embeds" in g[f"marked/{dtype}"]


# ---- routing: the same launches, the fc1 kernels of the flagged tower renamed ----------------------------------------------------
def _launches(group, cfg):
    """the call lists of tests/launch_set_cases.py for these groups, on engines of ``cfg`` (built here: the recorded file is not read)"""
    from launch_set_cases import _encodes
    from plip_amd import weights as W
    from plip_amd.engine import Engine
    sd = W.synthetic_state_dict(cfg, 0)
    out = {}

    def tiny(**kw):
        return Engine(cfg, sd, dtype=kw.pop("dtype", "bf16"), max_batch=8, **kw)

    if group == "tiny_bf16":
        plan = [("bf16 B=3", {}, 0, True)]
    elif group == "tiny_latency":
        plan = [("bf16 latency_batch=8 B=3", {}, 8, True), ("bf16 text_f16_layers=1 latency_batch=8 B=3", dict(text_f16_layers=1), 8, False)]
    elif group == "tiny_flags":
        plan = [(f"bf16 {tag} B=3", kw, 0, False) for tag, kw in (
            ("dense last block", dict(pooled_last_block=False)), ("separate LayerNorm", dict(ln_fold=False)),
            ("text tower f16", dict(text_f16=True)), ("text_f16_layers=2", dict(text_f16_layers=2)), ("text_f16_layers=1", dict(text_f16_layers=1)))]
    else:
        assert group == "tiny_f32"
        plan = [("f32 B=3", dict(dtype="f32"), 0, False)]
    for tag, kw, latency, packed in plan:
        eng = tiny(**kw)
        try:
            if latency:
                eng.set_latency_batch(latency)
            _encodes(eng, cfg, 3, out, tag, packed=packed)
        finally:
            eng.close()
    return out


@pytest.mark.parametrize("group", ["tiny_bf16", "tiny_latency", "tiny_flags", "tiny_f32"])
def test_gelu_engines_launch_the_same_kernels_with_fc1_renamed(group):
    from plip_amd.config import get_config
    base = get_config("tiny")
    quick = _launches(group, base)
    assert quick and any("qgelu" in r[0] for rows in quick.values() for r in rows)
    for v_act, t_act in (("gelu", "gelu"), ("gelu", "quick_gelu"), ("quick_gelu", "gelu")):
        got = _launches(group, base.replace(v_hidden_act=v_act, t_hidden_act=t_act))
        assert list(got) == list(quick)
        for call, rows in quick.items():
            flagged = (v_act if "encode_image" in call else t_act) == "gelu"
            want = []
            for name, calls, flops, nbytes in rows:
                role = name.split("|")[-1]
                if flagged and role in ("fc1", "fc1_pooled"):
                    assert "qgelu" in name, name
                    name = name.replace("qgelu", "gelu")
                want.append([name, calls, flops, nbytes])
            assert got[call] == want, (group, v_act, t_act, call)
            assert flagged == any("_gelu>" in r[0] for r in got[call]), (call, got[call])


# ---- same bits on every path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_gelu_engine_same_bits_packed_cloned_and_split(dtype):
    from plip_amd import weights as W
    from plip_amd.config import get_config
    from plip_amd.engine import Engine
    cfg = get_config("tiny").with_hidden_act("gelu")
    sd = W.synthetic_state_dict(cfg, 0)
    px = torch.from_numpy(W.synthetic_pixels(cfg, 7, 21))
    ids_np, mask_np = W.synthetic_ids(cfg, 7, 22)
    ids, mask = torch.from_numpy(ids_np), torch.from_numpy(mask_np)
    eng = Engine(cfg, sd, dtype=dtype, max_batch=8)
    split = Engine(cfg, sd, dtype=dtype, max_batch=8, pass_batch=2)
    quick = Engine(get_config("tiny"), sd, dtype=dtype, max_batch=8)
    try:
        img, txt = eng.encode_image(px), eng.encode_text(ids, mask)
        assert not torch.equal(img, quick.encode_image(px)) and not torch.equal(txt, quick.encode_text(ids, mask))
        eng.set_text_packing(True)
        assert torch.equal(eng.encode_text(ids, mask), txt)
        eng.set_text_packing(False)
        other = eng.clone()
        assert torch.equal(other.encode_image(px), img) and torch.equal(other.encode_text(ids, mask), txt)
        assert split.pass_batch == 2
        assert torch.equal(split.encode_image(px), img) and torch.equal(split.encode_text(ids, mask), txt)
        a, b = eng.encode_pair(px, ids, mask, normalize=False)
        assert torch.equal(a, img) and torch.equal(b, txt)
    finally:
        for e in (eng, split, quick):
            e.close()


def test_tower_outputs_and_attention_summaries_of_a_gelu_engine(gelu_models, engines, golden):
    """the every-token walks run the same blocks: hidden states against the gelu fixture; the attention maps of block 1 see block 0's MLP"""
    g = golden("gelu_tiny_b6")
    cfg, sd, px, ids, mask = case_inputs("tiny_b6")
    tpx, tids, tmask = torch.from_numpy(px), torch.from_numpy(ids), torch.from_numpy(mask)
    eng, quick = gelu_models("tiny_b6", "f32", "gelu", "gelu").engine, engines("tiny_b6", "f32")[0].engine
    vo = eng.tower_outputs("vision", tpx, output_hidden_states=True, output_attentions=True)
    to = eng.tower_outputs("text", tids, tmask, output_hidden_states=True)
    m = mask[:, :, None].astype(np.float32)
    for l in range(cfg.v_layers + 1):
        assert np.abs(vo.hidden_states[l].cpu().numpy() - g["vision_hidden"][l]).max() < F32["hidden"], l
        assert np.abs((to.hidden_states[l].cpu().numpy() - g["text_hidden"][l]) * m).max() < F32["hidden"], l
    qo = quick.tower_outputs("vision", tpx, output_attentions=True)
    assert torch.equal(vo.attentions[0], qo.attentions[0]) and not torch.equal(vo.attentions[1], qo.attentions[1])
    s, qs = eng.attention_summary("vision", tpx), quick.attention_summary("vision", tpx)
    assert torch.isfinite(s.rollout).all() and not torch.equal(s.rollout, qs.rollout)
    for dtype in ("bf16", "f16"):       # the 16-bit walk (dense last block, join_planes) against the same fixture
        e16 = gelu_models("tiny_b6", dtype, "gelu", "gelu").engine
        ho = e16.tower_outputs("vision", tpx, output_hidden_states=True).hidden_states
        for l in range(cfg.v_layers + 1):
            assert np.abs(ho[l].cpu().numpy() - g["vision_hidden"][l]).max() < TINY[dtype]["hidden"], (dtype, l)


def test_at_resolution_on_a_gelu_engine_fp32(gelu_models, engines, golden):
    g = golden("gelu_tiny_144x128")
    px = torch.from_numpy(np.random.RandomState(int(g["seed"])).standard_normal(tuple(int(x) for x in g["shape"])).astype(np.float32))
    h, w = px.shape[2:]
    err = float(np.abs(gelu_models("tiny_b6", "f32", "gelu", "gelu").engine.at_resolution(h, w).encode_image(px).cpu().numpy()
                       - g["image_features"]).max())
    quick = float(np.abs(engines("tiny_b6", "f32")[0].engine.at_resolution(h, w).encode_image(px).cpu().numpy() - g["image_features"]).max())
    print(f"PARITY group=gelu_e2e case=tiny_144x128_f32 field=image_features bound={F32['feat']:.3e} gpu={err:.3e} quick_gelu_engine={quick:.3e}")
    assert err < F32["feat"]
    assert quick >= float(g["gap/image_features"]) - F32["feat"] > 29 * F32["feat"]
