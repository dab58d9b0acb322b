"""Feature combinations nobody hand-picked, against the extended numpy oracle, through the public Python surface.

tests/test_gpu_random_archs.py sweeps widths, depths and token counts with every later feature at its default; this sweeps the features
TOGETHER (tests/feature_sweep_common.py draw_case): head sizes 64 .. 128, the erf GELU per tower, a non-native image size, the split-K
latency path, mixed f16 / bf16 text blocks, caption packing, the A/B forms -- and compares every output the product has: the pair step,
the per-token tower outputs, the attention summaries, the token similarity, the resolution handle, and the bit-for-bit invariants
between them.

Reference: oracle/clip_oracle.py in float64 (pinned against HF on every committed fixture: tests/test_oracle.py).  Bounds:
* fp32 engine: the larger of the project's fp32 bound for the kind of field and 4 x the distance between the float32 and the float64
  run of the oracle on the case (numpy's and the engine's summation orders differ by that class of error);
* 16-bit engines, logits and features: the COS table and the relative feature bounds of tests/test_gpu_random_archs.py;
* 16-bit engines, per-token fields and token similarity: the larger of the bound of tests/test_gpu_tower_outputs.py /
  tests/test_gpu_token_similarity.py and 3 x the error of oracle/precision_model.py on the case (all six rounding sites, the engine's
  operand type, its LayerNorm plan and f16 lead blocks) against the float64 oracle.  The model carries the operand roundings with wide
  accumulation; the engine adds fp32 accumulation and the 8-bit remainder plane, both far below one operand ulp; the realisation of the
  rounding noise differs between the two: hence 3 x.
Nothing is measured against the engine itself.  Every comparison prints a PARITY line (profiles/feature_sweep_parity.txt)."""
import functools

import numpy as np
import pytest
import torch

import feature_sweep_common as F
from attention_summary_refs import pooled_rows, rollout_bound, rollout_ref
from test_gpu_random_archs import COS
from test_gpu_token_similarity import HF_TOL as SIM_TOL
from test_gpu_tower_outputs import TOL as TOWER_TOL
from test_gpu_tower_outputs import _probs_structure

pytestmark = pytest.mark.gpu

FEAT_REL = {"f32": 5e-5, "bf16": 4e-2, "f16": 6e-3}         # tests/test_gpu_random_archs.py: features, relative to the largest magnitude
DTYPES = ("f32", "bf16", "f16")


def _rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-6))


def _np_fields(out):
    """a TowerOutput as the dict of numpy arrays feature_sweep_common.tower_errors takes"""
    return {"last_hidden_state": out.last_hidden_state.cpu().numpy(), "pooler_output": out.pooler_output.cpu().numpy(),
            "hidden_states": [h.cpu().numpy() for h in out.hidden_states], "attentions": [a.cpu().numpy() for a in out.attentions]}


@functools.lru_cache(maxsize=2)
def _references(seed):
    """the CPU side of a case, once for its three engines: the oracle in float64 (the reference) and float32, the precision model
    for both 16-bit operand types, and the yardsticks that follow from them"""
    o64, o32 = F.oracle_fields_cached(seed, "f64"), F.oracle_fields_cached(seed, "f32")
    scale = float(np.exp(np.float64(F.case_inputs(seed)[4]["logit_scale"])))
    yard = {"f32": {"cos": float(np.abs(o32["logits_per_image"].astype(np.float64) - o64["logits_per_image"]).max() / scale),
                    "image_features": _rel(o32["image_features"], o64["image_features"]),
                    "text_features": _rel(o32["text_features"], o64["text_features"]),
                    "vision": F.tower_errors(o32["vision"], o64["vision"]), "text": F.tower_errors(o32["text"], o64["text"]),
                    "sim": F.similarity_errors(o32, o64)}}
    if "res_image_features" in o64:
        yard["f32"]["res_image_features"] = _rel(o32["res_image_features"], o64["res_image_features"])
    for dtype in ("bf16", "f16"):
        pm = F.precision_fields(seed, dtype)
        yard[dtype] = {"vision": F.tower_errors(pm["vision"], o64["vision"]), "text": F.tower_errors(pm["text"], o64["text"]),
                       "sim": F.similarity_errors(pm, o64)}
    return o64, yard, scale


@pytest.mark.parametrize("seed", range(F.N_CASES))
def test_feature_combination_matches_the_oracle(seed):
    from plip_amd.model import PlipModel
    from plip_amd.token_similarity import token_similarity
    cfg, B, kw_all, probes, sd, px, ids, mask, px_res = F.case_inputs(seed)
    o64, yard, scale = _references(seed)
    use_mask = mask if probes["use_mask"] else None
    P, I = torch.from_numpy(px), torch.from_numpy(ids)
    Mk = None if use_mask is None else torch.from_numpy(mask)
    T = torch.from_numpy(o64["text_features"].astype(np.float32))
    rows_t = pooled_rows("text", B, ids, cfg.eos_token_id)

    for dtype in DTYPES:
        kw = F.engine_kwargs_for(dtype, kw_all)
        case = (seed, dtype, cfg, B, kw, probes)
        mult = 4.0 if dtype == "f32" else 3.0

        def check(field, err, project, yardstick=None):
            """``yardstick`` None: the project's bound alone (16-bit logits and features)"""
            bound = project if yardstick is None else max(project, mult * yardstick)
            print(f"\nPARITY group=feature_sweep case={seed} dtype={dtype} field={field} bound={bound:.3e} gpu={err:.3e}")
            assert np.isfinite(err) and err <= bound, (field, err, bound, case)

        f32y = yard["f32"] if dtype == "f32" else None
        model = PlipModel(cfg, sd, dtype=dtype, max_batch=B, **kw)
        twin = None
        try:
            eng = model.engine
            # ---- 1. the pair step: eager, captured, replayed ---------------------------------------------------------------------
            outs = [model(input_ids=I, pixel_values=P, attention_mask=Mk) for _ in range(3)]
            for rep, out in enumerate(outs):
                got = out.logits_per_image.cpu().numpy()
                assert got.shape == (B, B), case
                check(f"logits call{rep}", float(np.abs(got - o64["logits_per_image"]).max() / scale), COS[dtype], f32y and f32y["cos"])
                assert torch.equal(out.logits_per_image, out.logits_per_text.T.contiguous()), case
                for k in ("logits_per_image", "image_embeds", "text_embeds"):
                    assert torch.equal(out[k], outs[0][k]), ("call", rep, k, case)
            img = model.get_image_features(pixel_values=P).cpu().numpy()
            txt = model.get_text_features(input_ids=I, attention_mask=Mk).cpu().numpy()
            check("image_features", _rel(img, o64["image_features"]), FEAT_REL[dtype], f32y and f32y["image_features"])
            check("text_features", _rel(txt, o64["text_features"]), FEAT_REL[dtype], f32y and f32y["text_features"])

            # ---- 2. per-token outputs of both towers, 3. their summaries ---------------------------------------------------------
            for tower, inp, m, rows in (("vision", P, None, pooled_rows("vision", B)), ("text", I, Mk, rows_t)):
                S, D, H, L = eng.tower_shape(tower)
                t = eng.tower_outputs(tower, inp, m, output_hidden_states=True, output_attentions=True)
                assert len(t.hidden_states) == L + 1 and len(t.attentions) == L and t.attentions[0].shape == (B, H, S, S), case
                _probs_structure(t.attentions, None if m is None else mask, tower == "text")
                got = _np_fields(t)
                for k, err in F.tower_errors(got, o64[tower]).items():
                    check(f"{tower}_{k}", err, TOWER_TOL[dtype][k], yard[dtype][tower][k])
                s = eng.attention_summary(tower, inp, m, rollout_matrix=True)
                idx, r = torch.arange(B, device=eng.device), torch.as_tensor(rows, device=eng.device)
                for l in range(L):
                    assert torch.equal(s.pooled_attention[l], t.attentions[l][idx, :, r, :]), (tower, "pooled_attention", l, case)
                assert torch.equal(s.rollout, s.rollout_matrix[idx, r]), (tower, "rollout", case)
                err = float(np.abs(s.rollout_matrix.cpu().numpy().astype(np.float64) - rollout_ref(got["attentions"])).max())
                check(f"{tower}_rollout", err, rollout_bound(L, S, H))

            # ---- 4. token similarity ---------------------------------------------------------------------------------------------
            if cfg.projection_dim % 32:
                # no per-token head for such a projection (plip_amd/token_similarity.py, README): refused by name, nothing launched
                with pytest.raises(ValueError, match=f"projection_dim = {cfg.projection_dim}.*multiples of 32"):
                    token_similarity(eng, P, T, return_embeds=True)
            else:
                ts = token_similarity(eng, P, T, return_embeds=True)
                got = {"token_embeds": ts.token_embeds.cpu().numpy(), "similarity": ts.similarity.cpu().numpy(),
                       "similarity_softmax": o64["similarity_softmax"]}
                if probes["softmax"]:
                    got["similarity_softmax"] = token_similarity(eng, P, T, scale=scale, softmax=True).similarity.cpu().numpy()
                errs = F.similarity_errors(got, o64)
                check("token_embeds", errs["embeds"], SIM_TOL["embeds"][dtype], yard[dtype]["sim"]["embeds"])
                check("similarity", errs["similarity"], SIM_TOL["similarity"][dtype], yard[dtype]["sim"]["similarity"])
                if probes["softmax"]:
                    check("similarity_softmax", errs["softmax"], SIM_TOL["similarity"][dtype], yard[dtype]["sim"]["softmax"])
                # row 0 is the pooled token: its cosines are the pair's logits
                check("similarity_row0", float(np.abs(got["similarity"][:, 0] - o64["logits_per_image"] / scale).max()), COS[dtype],
                      f32y and f32y["cos"])

            # ---- 5. another image size on the resolution handle --------------------------------------------------------------------
            n_small = min(B, 8) if kw.get("latency_batch") else B        # rows that share a regime with a row encoded alone
            if px_res is not None:
                res = eng.at_resolution(*probes["image_hw"])
                R = torch.from_numpy(px_res)
                feats = res.encode_image(R)
                check("res_image_features", _rel(feats.cpu().numpy(), o64["res_image_features"]), FEAT_REL[dtype],
                      f32y and f32y["res_image_features"])
                assert torch.equal(res.encode_image(R[:1])[0], res.encode_image(R[:n_small])[0]), ("resolution, sample 0 alone", case)

            # ---- 6. invariants, bit for bit ----------------------------------------------------------------------------------------
            if kw.get("latency_batch"):
                # the latency path met the oracle's bounds above (B <= 8); a row alone has the bits it has in a batch of that regime
                bi = eng.encode_image(P[:n_small], normalize=True)
                bt = eng.encode_text(I[:n_small], None if Mk is None else Mk[:n_small], normalize=True)
                for b in range(n_small):
                    assert torch.equal(eng.encode_image(P[b:b + 1], normalize=True)[0], bi[b]), ("latency, image row alone", b, case)
                    assert torch.equal(eng.encode_text(I[b:b + 1], None if Mk is None else Mk[b:b + 1], normalize=True)[0], bt[b]), \
                        ("latency, text row alone", b, case)
            if kw.get("pack_captions"):
                # packed rows keep the tiled GEMMs (csrc/towers.hip run_gemm), so the two forms share bits where the unpacked one runs
                # them too: off the latency path
                eng.set_latency_batch(0)
                packed = eng.encode_text(I, Mk, normalize=True)
                eng.set_text_packing(False)
                plain = eng.encode_text(I, Mk, normalize=True)
                eng.set_text_packing(True)
                eng.set_latency_batch(kw.get("latency_batch", 0))
                assert torch.equal(packed, plain), ("packing on / off", case)
            twin = PlipModel(cfg, sd, dtype=dtype, max_batch=B, **kw)
            out2 = twin(input_ids=I, pixel_values=P, attention_mask=Mk)
            for k in ("logits_per_image", "image_embeds", "text_embeds"):
                assert torch.equal(out2[k], outs[0][k]), ("second engine", k, case)
            t2 = twin.engine.tower_outputs("text", I, Mk, output_attentions=True)
            assert torch.equal(t2.last_hidden_state, t.last_hidden_state) and torch.equal(t2.attentions[-1], t.attentions[-1]), \
                ("second engine, text tower outputs", case)
        finally:
            model.engine.close()
            if twin is not None:
                twin.engine.close()
