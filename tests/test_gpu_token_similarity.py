"""The dense image-text similarity on the MI355X (include/plipmi.h plipmi_encode_token_similarity, plip_amd.token_similarity,
PlipModel.vision_model.token_similarity, PLIP.similarity_maps): the scores kernel of csrc/token_scores.hip against the float64 restatement
of tests/token_similarity_refs.py under the project's fp32 rule, the entry's head against the same reference on the engine's own
last_hidden_state, the entry against HF (tests/golden/token_similarity_*.npz, tools/make_token_similarity_golden.py), and what the entry
must leave alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.make_golden import case_inputs
from plip_amd import _lib
from small_kernel_refs import fp32_bound
from token_similarity_refs import FIXTURES, head_ref, head_weights, scores_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = ["f32", "bf16", "f16"]
F64 = torch.float64

# Max-abs error against HF (fp32, eager attention).  Not derivable for the 16-bit engines: the towers' hidden-state error enters every
# token row.  About 1.5x the largest error measured on the MI355X over the four fixtures (profiles/token_similarity_parity.txt);
# `embeds` is relative to the fixture field's largest magnitude.  A case is further capped at a tenth of the fixture field's own standard
# deviation (similarity: over the patch rows) -- the cap only keeps a tolerance from hiding a failure.
# Largest measurements: similarity f32 2.98e-7, bf16 1.22e-3, f16 1.68e-4; embeds f32 1.69e-6, bf16 3.06e-3, f16 3.98e-4.
HF_TOL = {"similarity": {"f32": 4.5e-7, "bf16": 1.85e-3, "f16": 2.5e-4},
          "embeds": {"f32": 2.5e-6, "bf16": 4.6e-3, "f16": 6.0e-4}}


# =====================================================================================================================================
# kernel level (plipmi_test.h plipmi_token_scores)
# =====================================================================================================================================
MS = [1, 17, 150, 257 * 3]          # one row; a partial workgroup; several workgroups with a partial one; 48 full workgroups + 3 rows
CS = [1, 2, 10, 63, 64]             # both ends; one lane slot; a partial last chunk of sixteen; four full chunks


def _inputs(M, P, C, seed):
    """E: random rows of mixed norms, every third one close to a text row (cosines over the whole range, not only near 0)"""
    g = torch.Generator().manual_seed(seed)
    T = torch.randn(C, P, generator=g)
    E = torch.randn(M, P, generator=g) * (0.1 + 5.0 * torch.rand(M, 1, generator=g))
    near = torch.arange(0, M, 3)
    E[near] = T[near % C] * (0.5 + torch.rand(len(near), 1, generator=g)) * torch.where(near % 2 == 0, 1.0, -1.0)[:, None] \
        + 0.3 * torch.randn(len(near), P, generator=g)
    return E, T


@pytest.mark.parametrize("P", [32, 64, 512, 1024])
def test_scores_kernel_against_float64(P):
    """every (M, C) of the list at this P: the scores, their softmax at scale 100 and the scores from text rows of other norms against
    float64 under the fp32 rule -- ONE bound per group over all the cases (4 x the error plain CPU fp32 makes on the same inputs);
    guard rows behind the M written ones stay untouched; a row computed alone has the bits it has in the batch"""
    from plip_amd.kernel_entries import token_scores
    groups = {k: {"gpu": [], "cpu": [], "ref": []} for k in ("scores", "softmax", "unnormalised")}
    for M in MS:
        for Cn in CS:
            E, T = _inputs(M, P, Cn, 1000 * P + 10 * M + Cn)
            Ed, Td = E.to(DEV), T.to(DEV)
            tag = (M, P, Cn)
            # scores at scale 1, with guard rows
            out = torch.full((M + 3, Cn), -7.5, device=DEV)
            token_scores(Ed, Td, out=out)
            assert torch.equal(out[M:], torch.full((3, Cn), -7.5, device=DEV)), tag
            got = out[:M].cpu()
            assert torch.isfinite(got).all() and (got.abs() <= 1 + 1e-6).all(), tag
            groups["scores"]["gpu"].append(got.flatten())
            groups["scores"]["cpu"].append(scores_ref(E, T, dtype=torch.float32).flatten())
            groups["scores"]["ref"].append(scores_ref(E, T).flatten())
            # a row alone: the same bits (first, a middle one, last)
            for r in sorted({0, M // 2, M - 1}):
                assert torch.equal(token_scores(Ed[r:r + 1].contiguous(), Td)[0].cpu(), got[r]), (tag, r)
            # softmax at scale 100
            sm = torch.full((M + 3, Cn), -7.5, device=DEV)
            token_scores(Ed, Td, scale=100.0, softmax=True, out=sm)
            assert torch.equal(sm[M:], torch.full((3, Cn), -7.5, device=DEV)), tag
            sm = sm[:M].cpu()
            assert torch.isfinite(sm).all() and (sm >= 0).all() and (sm <= 1).all(), tag
            dev = float((sm.to(F64).sum(-1) - 1).abs().max())
            assert dev <= (Cn + 10) * 2.0 ** -24, (tag, dev)
            groups["softmax"]["gpu"].append(sm.flatten())
            groups["softmax"]["cpu"].append(scores_ref(E, T, 100.0, True, dtype=torch.float32).flatten())
            groups["softmax"]["ref"].append(scores_ref(E, T, 100.0, True).flatten())
            # text rows scaled by 0.01 .. 100: the same scores
            Ts = T * torch.logspace(-2, 2, Cn)[:, None] if Cn > 1 else T * 100.0
            groups["unnormalised"]["gpu"].append(token_scores(Ed, Ts.to(DEV)).cpu().flatten())
            groups["unnormalised"]["cpu"].append(scores_ref(E, Ts, dtype=torch.float32).flatten())
            groups["unnormalised"]["ref"].append(scores_ref(E, T).flatten())
    for name, g in groups.items():
        gpu, cpu, ref = (torch.cat(g[k]) for k in ("gpu", "cpu", "ref"))
        bound, cpu_err = fp32_bound(cpu, ref)
        err = float((gpu.to(F64) - ref).abs().max())
        print(f"token_scores P={P} {name}: gpu {err:.3e}  cpu fp32 {cpu_err:.3e}  bound {bound:.3e}")
        assert err <= bound, (P, name, err, bound)


# =====================================================================================================================================
# through plip_amd.token_similarity
# =====================================================================================================================================
def _case_pixels(name, px):
    case, n_img, shape = FIXTURES[name]
    if n_img is None:
        return torch.from_numpy(np.random.RandomState(160).standard_normal((2, 3, 160, 160)).astype(np.float32))   # make_tower_outputs_golden.pixels_160
    return torch.from_numpy(px[:n_img])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["token_similarity_tiny", "token_similarity_tinyp4", "token_similarity_vitb32_b2"])
def test_head_alone_against_float64(name, dtype, engines, golden):
    """token_embeds and similarity against head_ref in float64 on the ENGINE's own last_hidden_state of the same pixels: the head is
    fp32 on every engine, so the fp32 rule applies and the towers' error stays out"""
    from plip_amd.token_similarity import token_similarity
    case, n_img, (B, S, P, Cn) = FIXTURES[name]
    model, cfg, sd, px, ids, mask = engines(case, dtype)
    eng = model.engine
    pix = _case_pixels(name, px)
    T = golden(case)["text_embeds"]
    out = token_similarity(eng, pix, torch.from_numpy(T), return_embeds=True)
    assert out.similarity.shape == (B, S, Cn) and out.token_embeds.shape == (B, S, P)
    assert out.similarity.dtype == torch.float32 and out.token_embeds.dtype == torch.float32
    X = eng.tower_outputs("vision", pix).last_hidden_state.cpu()
    ln_w, ln_b, proj = head_weights(sd)
    E64, s64 = head_ref(X, ln_w, ln_b, cfg.layer_norm_eps, proj, T)
    E32, s32 = head_ref(X, ln_w, ln_b, cfg.layer_norm_eps, proj, T, dtype=torch.float32)
    for field, got, c32, r64 in (("token_embeds", out.token_embeds, E32, E64), ("similarity", out.similarity, s32, s64)):
        bound, cpu_err = fp32_bound(c32, r64)
        err = float((got.cpu().to(F64) - r64).abs().max())
        print(f"head alone {name} {dtype} {field}: gpu {err:.3e}  cpu fp32 {cpu_err:.3e}  bound {bound:.3e}")
        assert err <= bound, (name, dtype, field, err, bound)
    # without return_embeds E lives in handle scratch: the same scores
    assert torch.equal(token_similarity(eng, pix, torch.from_numpy(T)).similarity, out.similarity)
    assert token_similarity(eng, pix, torch.from_numpy(T)).token_embeds is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_against_hf(name, dtype, engines, golden):
    """all four HF fixtures (the 160 x 160 one on the plipmi_clone_resolution handle), every engine dtype"""
    from plip_amd.token_similarity import token_similarity
    case, n_img, (B, S, P, Cn) = FIXTURES[name]
    model, cfg, sd, px, ids, mask = engines(case, dtype)
    eng = model.engine if n_img is not None else model.engine.at_resolution(160, 160)
    pix = _case_pixels(name, px)
    g = golden(name)
    T = torch.from_numpy(golden(case)["text_embeds"])
    out = token_similarity(eng, pix, T, return_embeds=True)
    emax = float(np.abs(g["token_embeds"]).max())
    err_e = float((out.token_embeds.cpu().to(F64) - torch.from_numpy(g["token_embeds"]).to(F64)).abs().max()) / emax
    err_s = float((out.similarity.cpu().to(F64) - torch.from_numpy(g["similarity"]).to(F64)).abs().max())
    cap_e = 0.1 * float(g["token_embeds"].astype(np.float64).std()) / emax
    cap_s = 0.1 * float(g["similarity"][:, 1:].astype(np.float64).std())
    print(f"HF parity {name} {dtype}: token_embeds {err_e:.3e} of max |E| = {emax:.2f} (cap {cap_e:.2e}), similarity {err_s:.3e} (cap {cap_s:.2e})")
    assert err_e <= min(HF_TOL["embeds"][dtype], cap_e), (name, dtype, err_e)
    assert err_s <= min(HF_TOL["similarity"][dtype], cap_s), (name, dtype, err_s)
    if n_img is None:
        via = model.vision_model.token_similarity(pix, T, interpolate_pos_encoding=True, return_embeds=True)
        assert torch.equal(via.similarity, out.similarity) and torch.equal(via.token_embeds, out.token_embeds)
    else:
        via = model.vision_model.token_similarity(pixel_values=pix, text_embeds=T)
        assert torch.equal(via.similarity, out.similarity) and via.token_embeds is None


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", ["tiny_b6", "vitb32_b4"])
def test_batch_larger_than_max_batch_and_empty(case, dtype, golden):
    """B = 2 max_batch + 1 on an engine of max_batch 2 (three chunks) equals the per-sample calls bit for bit -- on the 32 x 32 tile of the
    tiny projection and on the 128 x 128 tile of ViT-B/32's --; B = 0 returns empty tensors of the right shapes"""
    from plip_amd.model import PlipModel
    from plip_amd.token_similarity import token_similarity
    cfg, sd, px, ids, mask = case_inputs(case)
    model = PlipModel(cfg, sd, dtype=dtype, max_batch=2)
    eng = model.engine
    try:
        pix = torch.from_numpy(np.concatenate([px, px[::-1] * 0.5])[:5].copy())
        T = torch.from_numpy(golden(case)["text_embeds"])
        S, P, Cn = eng.v_tokens, cfg.projection_dim, T.shape[0]
        out = token_similarity(eng, pix, T, return_embeds=True)
        assert out.similarity.shape == (5, S, Cn) and out.token_embeds.shape == (5, S, P)
        for b in range(5):
            one = token_similarity(eng, pix[b:b + 1], T, return_embeds=True)
            assert torch.equal(one.similarity[0], out.similarity[b]) and torch.equal(one.token_embeds[0], out.token_embeds[b]), b
        e = token_similarity(eng, pix[:0], T, return_embeds=True)
        assert e.similarity.shape == (0, S, Cn) and e.token_embeds.shape == (0, S, P)
        assert token_similarity(eng, pix[:0], T).token_embeds is None
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_encode_bits_unchanged_after_token_similarity(dtype, golden):
    """the entry changes nothing the encode paths read: encode_pair returns the same bits before and after it, through the
    small-batch graph replay (eager, captured, replayed) and, for encode_text, with caption packing on"""
    from plip_amd.model import PlipModel
    from plip_amd.token_similarity import token_similarity
    cfg, sd, px, ids, mask = case_inputs("vitb32_b4")
    model = PlipModel(cfg, sd, dtype=dtype, max_batch=8)
    eng = model.engine
    try:
        P, I, Mk = torch.from_numpy(px), torch.from_numpy(ids), torch.from_numpy(mask)
        T = torch.from_numpy(golden("vitb32_b4")["text_embeds"])
        before = [eng.encode_pair(P, I, Mk) for _ in range(3)]
        token_similarity(eng, P, T, return_embeds=True)
        token_similarity(eng, P[:1], T, scale=100.0, softmax=True)
        after = [eng.encode_pair(P, I, Mk) for _ in range(2)]
        for a in before[1:] + after:
            assert torch.equal(a[0], before[0][0]) and torch.equal(a[1], before[0][1])
        eng.set_text_packing(True)
        packed = eng.encode_text(I, Mk, normalize=True)
        token_similarity(eng, P, T)
        assert torch.equal(eng.encode_text(I, Mk, normalize=True), packed)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["tiny_b6", "vitb32_b4"])
def test_launches_of_a_call(case, engines, golden):
    """behind the every-token walk: ONE LayerNorm, ONE GEMM in the token_proj role, ONE token_scores; no probabilities, no rollout, no
    fused q/k/v + attention kernel.  (The walk itself has a `layernorm` launch of its own -- pre_layrnorm, and the blocks' on an engine
    that does not fold them -- so the head's is counted as the one launch more than Engine.tower_outputs makes on the same pixels.)"""
    from plip_amd.token_similarity import token_similarity
    model, cfg, sd, px, ids, mask = engines(case, "bf16")
    eng = model.engine
    pix, T = torch.from_numpy(px), torch.from_numpy(golden(case)["text_embeds"])

    def calls_of(fn):
        rows, calls = [], {}
        with eng.profile(rows):
            fn()
        for r in rows:
            calls[r["name"].split("|")[0]] = calls.get(r["name"].split("|")[0], 0) + r["calls"]
        return rows, calls
    rows, calls = calls_of(lambda: token_similarity(eng, pix, T))
    _, walk = calls_of(lambda: eng.tower_outputs("vision", pix))
    assert calls.get("token_scores") == 1
    assert calls.get("layernorm") == walk.get("layernorm", 0) + 1
    proj = [r for r in rows if r["name"].endswith("|token_proj")]
    assert len(proj) == 1 and proj[0]["calls"] == 1
    assert proj[0]["name"].startswith("gemm_nt<f32," if cfg.projection_dim % 128 == 0 else "head_gemm"), proj[0]["name"]
    for name in ("attention_probs", "attention_rollout_step", "attention_pooled_rows", "qkv_attention", "pool_layernorm"):
        assert name not in calls, name
    # everything else is the walk's: the same launches, the same counts
    tail = {"token_scores", "layernorm", proj[0]["name"].split("|")[0]}
    assert {k: v for k, v in calls.items() if k not in tail} == {k: v for k, v in walk.items() if k not in tail | {"pool_layernorm"}}
    # token_embeds only: no scores launch
    _, only = calls_of(lambda: _embeds_only(eng, pix, T))
    assert "token_scores" not in only and only.get("layernorm") == calls.get("layernorm")


def _embeds_only(eng, pix, T):
    """the C entry with similarity NULL (the Python call always takes the scores)"""
    x, t = pix.to(DEV).contiguous(), T.to(DEV).contiguous()
    emb = torch.empty((x.shape[0], eng.v_tokens, eng.cfg.projection_dim), device=DEV)
    _lib.check(eng.lib.plipmi_encode_token_similarity(eng._h, C.c_void_p(x.data_ptr()), x.shape[0], C.c_void_p(t.data_ptr()), t.shape[0], 1.0, 0,
                                                      C.c_void_p(emb.data_ptr()), None, eng._stream()), "plipmi_encode_token_similarity")
    torch.cuda.synchronize()
    return emb


def test_softmax_and_errors(engines, golden, monkeypatch):
    from plip_amd.token_similarity import token_similarity
    model, cfg, sd, px, ids, mask = engines("tiny_b6", "f32")
    eng = model.engine
    pix, T = torch.from_numpy(px), torch.from_numpy(golden("tiny_b6")["text_embeds"])
    scale = eng.logit_scale_exp
    plain = token_similarity(eng, pix, T, scale=scale)
    unit = token_similarity(eng, pix, T)
    sm = token_similarity(eng, pix, T, scale=scale, softmax=True)
    assert float((plain.similarity - scale * unit.similarity).abs().max()) <= 1e-6 * scale
    assert float((sm.similarity - torch.softmax(plain.similarity, -1)).abs().max()) <= 1e-6
    # the embeds alone are those of the full call
    assert torch.equal(_embeds_only(eng, pix, T), token_similarity(eng, pix, T, return_embeds=True).token_embeds)

    lib, s = eng.lib, eng._stream()
    x, t = pix.to(DEV), T.to(DEV)
    out = torch.empty((6, 17, 6), device=DEV)
    p = lambda v: C.c_void_p(v.data_ptr())
    call = lambda h, px_, B, tx, Cn, emb, sim: lib.plipmi_encode_token_similarity(h, px_, B, tx, Cn, 1.0, 0, emb, sim, s)
    for args, word in (((eng._h, None, 6, p(t), 6, None, p(out)), "pixels"), ((eng._h, p(x), 6, None, 6, None, p(out)), "text_embeds"),
                       ((eng._h, p(x), 6, p(t), 6, None, None), "no output"), ((eng._h, p(x), 6, p(t), 0, None, p(out)), "C ="),
                       ((eng._h, p(x), 6, p(t), 65, None, p(out)), "C ="), ((eng._h, p(x), eng.max_batch + 1, p(t), 6, None, p(out)), "max_batch"),
                       ((None, p(x), 6, p(t), 6, None, p(out)), "null handle")):
        assert call(*args) == 1, word
        assert word in _lib.last_error(), (word, _lib.last_error())
    assert call(eng._h, None, 0, None, 6, None, None) == 0           # B == 0: nothing to do, nothing launched
    with pytest.raises(ValueError, match="64"):
        token_similarity(eng, pix, torch.randn(65, cfg.projection_dim))
    with pytest.raises(ValueError, match="text_embeds"):
        token_similarity(eng, pix, torch.randn(3, cfg.projection_dim + 32))
    with pytest.raises(ValueError, match="Input image size"):
        token_similarity(eng, pix[:, :, :16], T)
    with pytest.raises(ValueError, match="You have to specify"):
        model.vision_model.token_similarity(pix)
    with pytest.raises(ValueError, match="vision_model"):
        model.text_model.token_similarity(pix, T)
    # a request larger than the free device memory is refused before anything is allocated
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (4096, 1 << 30))
    with pytest.raises(ValueError, match="MiB"):
        token_similarity(eng, pix, T)


@pytest.mark.parametrize("P", [80, 200])
def test_projection_widths_without_a_kernel_are_refused_by_name(P):
    """a projection_dim that is no multiple of 32 encodes (head_gemm takes any width) but has no per-token head: Python refuses before
    anything is allocated, the C entry before anything is launched, both by name; the encode paths of the same engine still run"""
    from plip_amd.config import get_config
    from plip_amd.model import PlipModel
    from plip_amd.token_similarity import token_similarity
    model = PlipModel.from_synthetic(get_config("tiny").replace(projection_dim=P), seed=3, dtype="bf16", max_batch=2)
    eng = model.engine
    try:
        pix = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(P))
        with pytest.raises(ValueError, match=f"projection_dim = {P}.*multiples of 32"):
            token_similarity(eng, pix, torch.randn(3, P))
        with pytest.raises(ValueError, match="multiples of 32"):
            model.vision_model.token_similarity(pix, torch.randn(3, P))
        x, t = pix.to(DEV), torch.randn(3, P).to(DEV)
        out = torch.full((2, 17, 3), -7.5, device=DEV)
        rc = eng.lib.plipmi_encode_token_similarity(eng._h, C.c_void_p(x.data_ptr()), 2, C.c_void_p(t.data_ptr()), 3, 1.0, 0, None,
                                                    C.c_void_p(out.data_ptr()), eng._stream())
        assert rc == 1 and f"projection_dim = {P}" in _lib.last_error() and "multiples of 32" in _lib.last_error()
        torch.cuda.synchronize()
        assert (out == -7.5).all()
        assert torch.isfinite(eng.encode_image(pix, normalize=True)).all()
    finally:
        eng.close()


def test_plip_similarity_maps(engines, golden):
    """three native-size uint8 tiles of the tiny model against six prompts: [3, 6, 4, 4] maps = the engine's scores on the pixels
    encode_images encodes, CLS dropped; token ids and a ready [C, P] array give the same maps; image_size= runs on the resolution handle"""
    from plip_amd.plip import _CROP, PLIP
    from plip_amd.preprocess import preprocess_images
    from plip_amd.token_similarity import token_similarity
    model, cfg, sd, px, ids, mask = engines("tiny_b6", "bf16")
    n = cfg.image_size
    g = n // cfg.patch_size
    tiles = [np.random.RandomState(k).randint(0, 256, (n, n, 3), dtype=np.uint8) for k in range(3)]
    plip = PLIP(model=model)
    txt = plip.encode_text(ids, batch_size=8)                      # float32 [6, P], un-normalised
    maps = plip.similarity_maps(tiles, txt, batch_size=2)
    assert maps.shape == (3, 6, g, g) and maps.dtype == np.float32
    pixels = torch.from_numpy(preprocess_images(tiles, n, crop=_CROP))
    sim = token_similarity(model.engine, pixels, torch.from_numpy(txt)).similarity
    assert np.array_equal(maps, sim[:, 1:].permute(0, 2, 1).reshape(3, 6, g, g).cpu().numpy())
    assert (np.abs(maps) <= 1 + 1e-6).all()
    assert np.array_equal(plip.similarity_maps(tiles, torch.from_numpy(ids), batch_size=3), maps)     # token ids; the caller's batching does not show
    sm = plip.similarity_maps(tiles, txt, batch_size=8, softmax=True)
    ref = token_similarity(model.engine, pixels, torch.from_numpy(txt), scale=model.engine.logit_scale_exp, softmax=True).similarity
    assert np.array_equal(sm, ref[:, 1:].permute(0, 2, 1).reshape(3, 6, g, g).cpu().numpy())
    np.testing.assert_allclose(sm.sum(1), 1.0, rtol=0, atol=16 * 2.0 ** -24)
    assert np.array_equal(plip.similarity_maps(tiles, txt, batch_size=8, scale=3.0),
                          token_similarity(model.engine, pixels, torch.from_numpy(txt), scale=3.0).similarity[:, 1:].permute(0, 2, 1)
                          .reshape(3, 6, g, g).cpu().numpy())
    assert plip.similarity_maps([], txt, batch_size=4).shape == (0, 6, g, g)
    # another resolution: tiles of 1.5 x the checkpoint's size on the plipmi_clone_resolution handle
    n2 = n + n // 2
    g2 = n2 // cfg.patch_size
    big = [np.random.RandomState(10 + k).randint(0, 256, (n2, n2, 3), dtype=np.uint8) for k in range(2)]
    maps2 = plip.similarity_maps(big, txt, batch_size=2, image_size=n2)
    assert maps2.shape == (2, 6, g2, g2)
    pix2 = torch.from_numpy(preprocess_images(big, n2, crop=_CROP))
    sim2 = token_similarity(model.engine.at_resolution(n2, n2), pix2, torch.from_numpy(txt)).similarity
    assert np.array_equal(maps2, sim2[:, 1:].permute(0, 2, 1).reshape(2, 6, g2, g2).cpu().numpy())
    with pytest.raises(ValueError, match="64"):
        plip.similarity_maps(tiles, np.ones((65, cfg.projection_dim), np.float32), batch_size=2)
