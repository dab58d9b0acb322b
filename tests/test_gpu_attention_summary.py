"""The attention summaries on the MI355X (include/plipmi.h plipmi_encode_attention_summary, Engine.attention_summary,
PlipModel.vision_model / .text_model .attention_summary, PLIP.attention_maps): the two kernels of csrc/attention_summary.hip against
plipmi_attention_probs on the same qkv (bit for bit where they share its device code, a derived fp32 bound for the rollout), the entry
against Engine.tower_outputs on the same engine and against HF (tests/golden/attention_summary_*.npz, tower_outputs_tiny.npz,
tools/make_attention_summary_golden.py), and what the entry must leave alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from attention_summary_refs import pooled_rows, rollout_bound, rollout_ref
from oracle.make_golden import case_inputs
from plip_amd import _lib
from test_gpu_tower_outputs import TOL as TOWER_TOL          # the `attn` tolerances of the probabilities against HF

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = ["f32", "bf16", "f16"]
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

# Max-abs error of the rollout (matrix and pooled row) against HF eager attention rolled out in float64.  Not derivable: the 16-bit
# engines' hidden-state error enters every block's probabilities.  About 1.5x the largest error measured on the MI355X over the HF
# fixtures below (profiles/attention_summary_parity.txt: f32 2.98e-7, bf16 8.66e-5, f16 4.76e-5); a case is further capped at L x the
# dtype's `attn` tolerance of tests/test_gpu_tower_outputs.py, L its tower's depth (_hf_errors) -- the cap only keeps these from hiding
# a failure; every measurement fits under it.
ROLLOUT_TOL = {"f32": 4.5e-7, "bf16": 1.3e-4, "f16": 7.2e-5}


# =====================================================================================================================================
# kernel level (plipmi_test.h plipmi_attention_pooled_rows / plipmi_attention_rollout_step)
# =====================================================================================================================================
def _qkv(B, S, H, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3 * H * 64, generator=g)
    qkv[:, : H * 64] *= 0.125 * 3.0                     # q pre-scaled; x3 sharpens the softmax (tests/test_gpu_small_kernels.py)
    return qkv.to(dtype).to(DEV)


def _masking(kind, B, S):
    """(causal, key_mask, dead): dense; causal; causal under a key mask whose sample 1 has key 0 masked -- its query row 0 then has no
    live key at all -- and, where there is room, a padded tail"""
    if kind == "dense":
        return False, None, False
    if kind == "causal":
        return True, None, False
    mask = torch.ones(B, S, dtype=torch.int64)
    mask[1, 0] = 0
    if S > 4:
        mask[2, S - 2:] = 0
    return True, mask.to(DEV), True


# S: one partial tile, an exact tile, a 1-row tail tile, one wave of keys (and the last S of the 4-rows-per-lane form), one key more than
# a wave (the 8-rows-per-lane form), more keys than the workgroup has lanes (16 rows per lane)
@pytest.mark.parametrize("dname", DTYPES)
@pytest.mark.parametrize("S", [5, 16, 17, 50, 64, 65, 257])
def test_kernels_against_attention_probs(S, dname):
    from plip_amd.kernel_entries import attention_pooled_rows, attention_probs, attention_rollout_step
    B = 3
    eye = torch.eye(S, device=DEV).expand(B, S, S).contiguous()
    for H in (1, 2, 12):
        for kind in ("dense", "causal", "causal_keymask"):
            causal, mask, dead = _masking(kind, B, S)
            case = f"S{S}_H{H}_{kind}_{dname}"
            qkvs = [_qkv(B, S, H, 7919 * S + 31 * H + k, TORCH_DT[dname]) for k in range(3)]
            probs = [attention_probs(q, B, S, H, causal, mask) for q in qkvs]

            # the pooled rows: the same device code on a 1-row tile, so the same bits.  Rows: first, last, and (sample 1) the dead row 0
            rows = torch.tensor([S - 1, 0, S // 2], dtype=torch.int32, device=DEV)
            got = attention_pooled_rows(qkvs[0], rows, B, S, H, causal, mask)
            want = probs[0][torch.arange(B, device=DEV), :, rows.long(), :]
            assert got.shape == (B, H, S) and torch.equal(got, want), case
            if dead:
                assert (got[1] == 0).all(), case

            # R_in = NULL is the identity: adding exact zeros changes nothing
            r1 = attention_rollout_step(qkvs[0], None, B, S, H, causal, mask)
            assert torch.equal(r1, attention_rollout_step(qkvs[0], eye, B, S, H, causal, mask)), case

            # one step and a chain of three against float64 arithmetic on the probabilities the probs kernel wrote
            r3 = attention_rollout_step(qkvs[2], attention_rollout_step(qkvs[1], r1, B, S, H, causal, mask), B, S, H, causal, mask)
            torch.cuda.synchronize()
            P = [p.cpu().numpy() for p in probs]
            for steps, r in ((1, r1), (3, r3)):
                r = r.cpu().numpy()
                bound = rollout_bound(steps, S, H)
                err = float(np.abs(r.astype(np.float64) - rollout_ref(P[:steps])).max())
                sums = r.astype(np.float64).sum(-1)
                sum_err = float(np.abs(sums - 1.0).max())
                print(f"\nPARITY group=rollout_kernel case={case} steps={steps} err={err:.3e} rowsum_err={sum_err:.3e} bound={bound:.3e}")
                assert err <= bound, (case, steps, err, bound)
                assert (r >= 0).all(), case
                if not dead:
                    assert sum_err <= bound, (case, steps, sum_err, bound)
            if dead:            # the dead row of block 1 leaves 1/2 e_0
                half = np.zeros(S, np.float32)
                half[0] = 0.5
                assert np.array_equal(r1[1, 0].cpu().numpy(), half), case


@pytest.mark.parametrize("dname", ["f32", "bf16"])
def test_rollout_step_above_64_kib_of_lds(dname):
    """S = 577 (ViT-L/14@336): the rollout tile takes 76 KiB of dynamic LDS, past the 64 KiB a kernel gets without the attribute;
    37 query tiles with a 1-row tail; a chain of two steps"""
    from plip_amd.kernel_entries import attention_pooled_rows, attention_probs, attention_rollout_step
    B, S, H = 2, 577, 2
    for kind in ("dense", "causal_keymask"):
        causal, mask, dead = _masking(kind, 3, S)
        mask = None if mask is None else mask[:B].contiguous()
        qkvs = [_qkv(B, S, H, 577 + k, TORCH_DT[dname]) for k in range(2)]
        probs = [attention_probs(q, B, S, H, causal, mask) for q in qkvs]
        rows = torch.tensor([S - 1, 0], dtype=torch.int32, device=DEV)
        got = attention_pooled_rows(qkvs[0], rows, B, S, H, causal, mask)
        assert torch.equal(got, probs[0][torch.arange(B, device=DEV), :, rows.long(), :]), kind
        r1 = attention_rollout_step(qkvs[0], None, B, S, H, causal, mask)
        r2 = attention_rollout_step(qkvs[1], r1, B, S, H, causal, mask)
        torch.cuda.synchronize()
        P = [p.cpu().numpy() for p in probs]
        for steps, r in ((1, r1), (2, r2)):
            err = float(np.abs(r.cpu().numpy().astype(np.float64) - rollout_ref(P[:steps])).max())
            print(f"\nPARITY group=rollout_kernel case=S{S}_H{H}_{kind}_{dname} steps={steps} err={err:.3e} bound={rollout_bound(steps, S, H):.3e}")
            assert err <= rollout_bound(steps, S, H), (kind, steps, err)


def test_kernel_entries_refuse_bad_arguments():
    lib = _lib.load()
    qkv = _qkv(1, 16, 1, 1, torch.float32)
    out = torch.empty(1, 16, 16, device=DEV)
    rows = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.plipmi_attention_rollout_step(_lib.F32, p(qkv), p(out), p(out), 1, 16, 1, 0, None, None) == 1
    assert "R_in" in _lib.last_error()
    assert lib.plipmi_attention_rollout_step(_lib.F32, p(qkv), None, p(out), 1, 1025, 1, 0, None, None) == 1
    assert lib.plipmi_attention_pooled_rows(_lib.F32, p(qkv), None, p(out), 1, 16, 1, 0, None, None) == 1
    assert lib.plipmi_attention_pooled_rows(5, p(qkv), p(rows), p(out), 1, 16, 1, 0, None, None) == 1
    assert lib.plipmi_attention_rollout_step(_lib.F32, p(qkv), None, p(out), 0, 16, 1, 0, None, None) == 0      # B = 0: nothing to do


# =====================================================================================================================================
# through Engine.attention_summary
# =====================================================================================================================================
def _check_against_tower_outputs(tag, eng, tower, inp, mask, rows):
    """the three summaries against tower_outputs(output_attentions=True) of the same engine; returns (summary, attentions as numpy)"""
    S, D, H, L = eng.tower_shape(tower)
    B = inp.shape[0]
    s = eng.attention_summary(tower, inp, mask, rollout_matrix=True)
    att = eng.tower_outputs(tower, inp, mask, output_attentions=True).attentions
    assert len(s.pooled_attention) == L and s.rollout.shape == (B, S) and s.rollout_matrix.shape == (B, S, S)
    idx = torch.arange(B, device=eng.device)
    r = torch.as_tensor(rows, device=eng.device)
    for l in range(L):
        assert s.pooled_attention[l].shape == (B, H, S)
        assert torch.equal(s.pooled_attention[l], att[l][idx, :, r, :]), (tag, l)
    assert torch.equal(s.rollout, s.rollout_matrix[idx, r]), tag
    att = [a.cpu().numpy() for a in att]
    err = float(np.abs(s.rollout_matrix.cpu().numpy().astype(np.float64) - rollout_ref(att)).max())
    bound = rollout_bound(L, S, H)
    print(f"\nPARITY group=rollout_engine case={tag} err={err:.3e} bound={bound:.3e}")
    assert err <= bound, (tag, err, bound)
    # each output alone is the same bits as all three together (another scratch layout, the caller's matrix as a ping-pong buffer or not)
    only = eng.attention_summary(tower, inp, mask, pooled_attention=False, rollout=True)
    assert only.pooled_attention is None and only.rollout_matrix is None and torch.equal(only.rollout, s.rollout), tag
    only = eng.attention_summary(tower, inp, mask, pooled_attention=True, rollout=False)
    assert only.rollout is None and all(torch.equal(a, b) for a, b in zip(only.pooled_attention, s.pooled_attention)), tag
    return s, att


def _hf_errors(tag, dtype, s, hf_pooled, hf_matrix, rows):
    """pooled rows / rollout against HF: hf_pooled [L, B, H, S], hf_matrix float64 or fp32 [B, S, S]"""
    L = len(s.pooled_attention)
    e_pool = max(float(np.abs(s.pooled_attention[l].cpu().numpy().astype(np.float64) - hf_pooled[l]).max()) for l in range(L))
    e_mat = float(np.abs(s.rollout_matrix.cpu().numpy().astype(np.float64) - hf_matrix).max())
    e_row = float(np.abs(s.rollout.cpu().numpy().astype(np.float64) - np.asarray(hf_matrix)[np.arange(len(rows)), rows]).max())
    cap = L * TOWER_TOL[dtype]["attn"]
    print(f"\nPARITY group=summary_vs_hf dtype={dtype} case={tag} L={L} pooled={e_pool:.3e} (tol {TOWER_TOL[dtype]['attn']:.1e}) "
          f"rollout_matrix={e_mat:.3e} rollout={e_row:.3e} (tol {ROLLOUT_TOL[dtype]:.1e}, cap {cap:.1e})")
    assert ROLLOUT_TOL[dtype] <= 12 * TOWER_TOL[dtype]["attn"]
    assert e_pool <= TOWER_TOL[dtype]["attn"], (tag, e_pool)
    assert max(e_mat, e_row) <= min(ROLLOUT_TOL[dtype], cap), (tag, e_mat, e_row)


def _hf_tiny(g, run, tower, rows):
    att = g[f"{run}/{tower}_attentions"]                 # [L, B, H, S, S], every block
    return att[:, np.arange(att.shape[1]), :, rows, :].transpose(1, 0, 2, 3), rollout_ref(att)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_against_tower_outputs_and_hf(dtype, engines, golden):
    """tiny arch, both towers: captions under their mask, the same captions without one, zero-padded captions (argmax pooling)"""
    g = golden("tower_outputs_tiny")
    model, cfg, sd, px, ids, mask = engines("tiny_b6", dtype)
    eng = model.engine
    P, I, Mk = torch.from_numpy(px), torch.from_numpy(ids), torch.from_numpy(mask)
    rows_v, rows_t = pooled_rows("vision", 6), pooled_rows("text", 6, ids, cfg.eos_token_id)
    s, _ = _check_against_tower_outputs(f"tiny vision {dtype}", eng, "vision", P, None, rows_v)
    _hf_errors("tiny vision", dtype, s, *_hf_tiny(g, "eos_masked", "vision", rows_v), rows_v)
    s, _ = _check_against_tower_outputs(f"tiny text masked {dtype}", eng, "text", I, Mk, rows_t)
    _hf_errors("tiny text masked", dtype, s, *_hf_tiny(g, "eos_masked", "text", rows_t), rows_t)
    s, _ = _check_against_tower_outputs(f"tiny text unmasked {dtype}", eng, "text", I, None, rows_t)
    _hf_errors("tiny text unmasked", dtype, s, *_hf_tiny(g, "eos_nomask", "text", rows_t), rows_t)
    # the tower objects route to the same call
    via = model.text_model.attention_summary(I, Mk, rollout_matrix=True)
    ref = eng.attention_summary("text", I, Mk, rollout_matrix=True)
    assert torch.equal(via.rollout_matrix, ref.rollout_matrix) and torch.equal(via.pooled_attention[-1], ref.pooled_attention[-1])
    assert torch.equal(model.vision_model.attention_summary(pixel_values=P).rollout, eng.attention_summary("vision", P).rollout)

    model, cfg, sd, px, ids, mask = engines("tiny_b5_zero_pad_ln100", dtype)
    rows_t = pooled_rows("text", 5, ids, cfg.eos_token_id)
    s, _ = _check_against_tower_outputs(f"tiny text zero-pad {dtype}", model.engine, "text", torch.from_numpy(ids), None, rows_t)
    _hf_errors("tiny text zero-pad", dtype, s, *_hf_tiny(g, "zero", "text", rows_t), rows_t)


@pytest.mark.parametrize("dtype", DTYPES)
def test_vitb32_against_tower_outputs_and_hf(dtype, engines, golden):
    """ViT-B/32, the first two samples of vitb32_b4: both towers (the text tower under its padding mask), and the 160 x 160
    plipmi_clone_resolution handle (26 tokens) through interpolate_pos_encoding=True"""
    g = golden("attention_summary_vitb32_b2")
    model, cfg, sd, px, ids, mask = engines("vitb32_b4", dtype)
    eng = model.engine
    rows_v = pooled_rows("vision", 2)
    s, _ = _check_against_tower_outputs(f"vitb32 vision {dtype}", eng, "vision", torch.from_numpy(px[:2]), None, rows_v)
    assert s.rollout.shape == (2, 50) and s.pooled_attention[0].shape == (2, 12, 50)
    _hf_errors("vitb32 vision", dtype, s, g["vision_pooled_attention"], g["vision_rollout_matrix"], rows_v)
    rows_t = pooled_rows("text", 2, ids[:2], cfg.eos_token_id)
    assert rows_t.tolist() == g["text_rows"].tolist()
    s, _ = _check_against_tower_outputs(f"vitb32 text {dtype}", eng, "text", torch.from_numpy(ids[:2]), torch.from_numpy(mask[:2]), rows_t)
    assert s.rollout_matrix.shape == (2, 77, 77)
    _hf_errors("vitb32 text", dtype, s, g["text_pooled_attention"], g["text_rollout_matrix"], rows_t)

    g = golden("attention_summary_vitb32_160")
    p160 = torch.from_numpy(np.random.RandomState(160).standard_normal((2, 3, 160, 160)).astype(np.float32))   # make_tower_outputs_golden.pixels_160
    e160 = eng.at_resolution(160, 160)
    s, _ = _check_against_tower_outputs(f"vitb32 160x160 {dtype}", e160, "vision", p160, None, rows_v)
    assert s.rollout.shape == (2, 26)
    _hf_errors("vitb32 160x160", dtype, s, g["vision_pooled_attention"], g["vision_rollout_matrix"], rows_v)
    via = model.vision_model.attention_summary(p160, interpolate_pos_encoding=True)
    assert torch.equal(via.rollout, s.rollout)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tinyp4_against_tower_outputs_and_hf(dtype, engines, golden):
    """257 vision tokens: 17 query tiles with a 1-row tail, the 16-rows-per-lane form"""
    g = golden("attention_summary_tinyp4")
    model, cfg, sd, px, ids, mask = engines("tinyp4_b3", dtype)
    rows_v = pooled_rows("vision", 3)
    s, _ = _check_against_tower_outputs(f"tinyp4 vision {dtype}", model.engine, "vision", torch.from_numpy(px), None, rows_v)
    assert s.rollout_matrix.shape == (3, 257, 257)
    _hf_errors("tinyp4 vision", dtype, s, g["vision_pooled_attention"], g["vision_rollout_matrix"], rows_v)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batch_larger_than_max_batch_and_empty(dtype):
    """B = 2 max_batch + 1 on an engine of max_batch 2 (three chunks) equals the per-sample calls bit for bit; B = 0 returns empty tensors"""
    from plip_amd.model import PlipModel
    cfg, sd, px, ids, mask = case_inputs("tiny_b6")
    model = PlipModel(cfg, sd, dtype=dtype, max_batch=2)
    eng = model.engine
    try:
        P, I, Mk = torch.from_numpy(px[:5]), torch.from_numpy(ids[:5]), torch.from_numpy(mask[:5])
        for tower, inp, m in (("vision", P, None), ("text", I, Mk)):
            S, D, H, L = eng.tower_shape(tower)
            s = eng.attention_summary(tower, inp, m, rollout_matrix=True)
            assert s.rollout.shape == (5, S) and s.rollout_matrix.shape == (5, S, S) and s.pooled_attention[0].shape == (5, H, S)
            for b in range(5):
                one = eng.attention_summary(tower, inp[b:b + 1], None if m is None else m[b:b + 1], rollout_matrix=True)
                assert torch.equal(one.rollout[0], s.rollout[b]) and torch.equal(one.rollout_matrix[0], s.rollout_matrix[b]), (tower, b)
                for l in range(L):
                    assert torch.equal(one.pooled_attention[l][0], s.pooled_attention[l][b]), (tower, b, l)
            e = eng.attention_summary(tower, inp[:0], None if m is None else m[:0], rollout_matrix=True)
            assert e.rollout.shape == (0, S) and e.rollout_matrix.shape == (0, S, S) and len(e.pooled_attention) == L
            assert e.pooled_attention[0].shape == (0, H, S)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_encode_bits_unchanged_after_attention_summary(dtype):
    """the entry changes nothing the encode paths read: encode_pair returns the same bits before and after it, through the
    small-batch graph replay (eager, captured, replayed) and with caption packing on"""
    from plip_amd.model import PlipModel
    cfg, sd, px, ids, mask = case_inputs("vitb32_b4")
    model = PlipModel(cfg, sd, dtype=dtype, max_batch=8)
    eng = model.engine
    try:
        P, I, Mk = torch.from_numpy(px), torch.from_numpy(ids), torch.from_numpy(mask)
        before = [eng.encode_pair(P, I, Mk) for _ in range(3)]
        eng.attention_summary("text", I, Mk, rollout_matrix=True)
        eng.attention_summary("vision", P)
        after = [eng.encode_pair(P, I, Mk) for _ in range(2)]
        for a in before[1:] + after:
            assert torch.equal(a[0], before[0][0]) and torch.equal(a[1], before[0][1])
        eng.set_text_packing(True)
        packed = eng.encode_text(I, Mk, normalize=True)
        eng.attention_summary("text", I, Mk)
        assert torch.equal(eng.encode_text(I, Mk, normalize=True), packed)
    finally:
        eng.close()


def test_launches_of_a_summary_call(engines):
    """one rollout step per block (it stores the pooled rows on its way), or one pooled-rows kernel per block when no rollout is asked
    for; no [B,H,S,S] kernel, no fused q/k/v + attention kernel"""
    model, cfg, sd, px, ids, mask = engines("tiny_b6", "bf16")
    eng = model.engine
    rows = []
    with eng.profile(rows):
        eng.attention_summary("vision", torch.from_numpy(px), rollout_matrix=True)
    calls = {}
    for r in rows:
        calls[r["name"].split("|")[0]] = calls.get(r["name"].split("|")[0], 0) + r["calls"]
    L = cfg.v_layers
    assert calls.get("attention_rollout_step") == L and "attention_pooled_rows" not in calls
    assert calls.get("attention_rollout_row") == 1 and calls.get("pooled_row_index") == 1
    assert "attention_probs" not in calls and "qkv_attention" not in calls
    rows = []
    with eng.profile(rows):
        eng.attention_summary("vision", torch.from_numpy(px), rollout=False)
    names = {r["name"].split("|")[0] for r in rows}
    assert sum(r["calls"] for r in rows if r["name"] == "attention_pooled_rows") == L
    assert "attention_pooled_rows" in names and "attention_rollout_step" not in names and "attention_rollout_row" not in names


def test_errors(engines, monkeypatch):
    model, cfg, sd, px, ids, mask = engines("tiny_b6", "f32")
    eng = model.engine
    lib = eng.lib
    x = torch.from_numpy(px).cuda()
    m = torch.from_numpy(mask).cuda()
    out = torch.empty((64, 17), device="cuda")
    s = eng._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    # all outputs off / null input / an attention mask for the vision tower / a tower that does not exist / B > max_batch
    assert lib.plipmi_encode_attention_summary(eng._h, _lib.VISION, p(x), None, 6, -1, None, None, None, s) == 1
    assert "no output" in _lib.last_error()
    assert lib.plipmi_encode_attention_summary(eng._h, _lib.VISION, None, None, 6, -1, None, p(out), None, s) == 1
    assert lib.plipmi_encode_attention_summary(eng._h, _lib.VISION, p(x), p(m), 6, -1, None, p(out), None, s) == 1
    assert "mask" in _lib.last_error()
    assert lib.plipmi_encode_attention_summary(eng._h, 2, p(x), None, 6, -1, None, p(out), None, s) == 1
    assert "tower" in _lib.last_error()
    assert lib.plipmi_encode_attention_summary(eng._h, _lib.VISION, p(x), None, eng.max_batch + 1, -1, None, p(out), None, s) == 1
    assert "max_batch" in _lib.last_error()
    with pytest.raises(ValueError, match="tower"):
        eng.attention_summary("audio", x)
    with pytest.raises(ValueError, match="attention_mask"):
        eng.attention_summary("vision", x, torch.from_numpy(mask))
    with pytest.raises(ValueError, match="nothing asked for"):
        eng.attention_summary("vision", x, pooled_attention=False, rollout=False)
    with pytest.raises(ValueError, match="Input image size"):
        eng.attention_summary("vision", x[:, :, :32])
    with pytest.raises(ValueError, match="You have to specify"):
        model.vision_model.attention_summary()
    # a request larger than the free device memory is refused before anything is allocated
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (4096, 1 << 30))
    with pytest.raises(ValueError, match="MiB"):
        eng.attention_summary("vision", x, rollout_matrix=True)


def test_plip_attention_maps(engines):
    """three native-size uint8 tiles of the tiny model: [3, 4, 4] maps = the summary on the pixels encode_images encodes, CLS dropped"""
    from plip_amd.plip import _CROP, PLIP
    from plip_amd.preprocess import preprocess_images
    model, cfg, sd, px, ids, mask = engines("tiny_b6", "bf16")
    tiles = [np.random.RandomState(k).randint(0, 256, (cfg.image_size, cfg.image_size, 3), dtype=np.uint8) for k in range(3)]
    plip = PLIP(model=model)
    maps = plip.attention_maps(tiles, batch_size=2)
    assert maps.shape == (3, 4, 4) and maps.dtype == np.float32
    pixels = torch.from_numpy(preprocess_images(tiles, cfg.image_size, crop=_CROP))
    s = model.engine.attention_summary("vision", pixels)
    assert np.array_equal(maps, s.rollout[:, 1:].reshape(3, 4, 4).cpu().numpy())
    assert np.array_equal(plip.attention_maps(tiles, batch_size=3, kind="rollout"), maps)      # the caller's batching does not show
    last = plip.attention_maps(tiles, batch_size=8, kind="last")
    assert np.array_equal(last, s.pooled_attention[-1].mean(dim=1)[:, 1:].reshape(3, 4, 4).cpu().numpy())
    assert (maps > 0).all() and (maps.reshape(3, -1).sum(-1) < 1).all()                         # not renormalised: CLS keeps its share
    assert plip.attention_maps([], batch_size=4).shape == (0, 4, 4)
    with pytest.raises(ValueError, match="kind"):
        plip.attention_maps(tiles, batch_size=2, kind="mean")
