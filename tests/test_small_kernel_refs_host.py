"""The float64 references of tests/small_kernel_refs.py against independent formulations, on the CPU: the GPU test
(tests/test_gpu_small_kernels.py) measures the kernels against these references, so they are pinned here first --
torch.nn.functional, numpy and oracle/clip_oracle.py never enter the references themselves."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_kernel_refs as R
from oracle import clip_oracle as O


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("D", [4, 252, 768, 1664])
def test_layer_norm_matches_torch(D):
    g0 = _gen(D)
    x = (torch.randn(7, D, generator=g0) + 1.5).double()
    x[:, 1] += 60.0
    g, b = torch.randn(D, generator=g0).double(), torch.randn(D, generator=g0).double()
    want = F.layer_norm(x, (D,), g, b, 1e-5)
    assert (R.layer_norm(x, g, b, 1e-5) - want).abs().max().item() < 1e-12
    const = torch.full((2, D), 3.25, dtype=torch.float64)                 # variance 0: the output is beta
    assert (R.layer_norm(const, g, b, 1e-5) - b).abs().max().item() < 1e-12


def test_slice_stats_recombine_to_the_row_statistics():
    """Chan's formula over the 64-column partials gives the row's mean and variance"""
    x = torch.randn(5, 256, generator=_gen(1)).double() * 3 + 11
    st = R.slice_stats(x).double()
    mean = st[..., 0].sum(-1) / 256
    m2 = st[..., 1].sum(-1) + (64 * (st[..., 0] / 64 - mean[:, None]) ** 2).sum(-1)
    assert (mean - x.mean(-1)).abs().max().item() < 1e-5
    assert (m2 / 256 - x.var(-1, unbiased=False)).abs().max().item() < 1e-4


@pytest.mark.parametrize("pre", [1.0, 0.125])
def test_folded_weights_are_layernorm_then_linear(pre):
    """rstd * (x . Wf^T) + c2 == pre * Linear(LayerNorm(x)): the centred rows subtract the mean"""
    g0 = _gen(3)
    D, N = 260, 9
    x = torch.randn(6, D, generator=g0).double() + 1.5
    W, bias = torch.randn(N, D, generator=g0).double(), torch.randn(N, generator=g0).double()
    g = torch.exp(torch.empty(D).uniform_(-2.3, 2.3, generator=g0)).double()
    b = torch.randn(D, generator=g0).double()
    Wf, c2 = R.fold_ln(W, bias, g, b, pre)
    assert Wf.sum(1).abs().max().item() < 1e-12
    rstd = 1.0 / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + 1e-5)
    want = pre * F.linear(F.layer_norm(x, (D,), g, b, 1e-5), W, bias)
    assert (rstd * (x @ Wf.T) + c2 - want).abs().max().item() < 1e-11


@pytest.mark.parametrize("causal,kind", [(False, None), (True, None), (True, "pad"), (True, "holes"), (False, "holes"), (True, "key0"),
                                         (True, "empty")])
def test_attention_probs_match_the_additive_mask_softmax(causal, kind):
    B, S, H = 2, 19, 3
    g0 = _gen(S)
    qkv = torch.randn(B * S, 3 * H * 64, generator=g0).double()
    mask = None
    if kind == "pad":
        mask = (torch.arange(S)[None, :] < torch.tensor([[7], [19]])).long()
    elif kind == "holes":
        mask = (torch.rand(B, S, generator=g0) < 0.6).long()
        mask[:, 3], mask[:, 4] = 0, 1
    elif kind == "key0":
        mask = torch.ones(B, S, dtype=torch.long)
        mask[0, :5] = 0
    elif kind == "empty":
        mask = torch.ones(B, S, dtype=torch.long)
        mask[1] = 0
    p = R.attention_probs(qkv, B, S, H, causal, mask)
    x = qkv.reshape(B, S, 3, H, 64)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
    add = torch.zeros(B, 1, S, S, dtype=torch.float64)
    if causal:
        add = add + torch.triu(torch.full((S, S), float("-inf"), dtype=torch.float64), 1)
    if mask is not None:
        add = add.masked_fill((mask == 0)[:, None, None, :], float("-inf"))
    want = torch.softmax(q @ k.transpose(-1, -2) + add, dim=-1)         # NaN where a row has no live key
    live = R.live_keys(B, S, causal, mask)
    has = live.any(-1)[:, None, :].expand(B, H, S)
    assert torch.isnan(want[~has]).all() and (p[~has] == 0).all()
    assert (p[has] - want[has]).abs().max().item() < 1e-14
    assert (p[~live[:, None].expand(B, H, S, S)] == 0).all()
    if kind == "key0":
        assert not has[0, :, :5].any() and has[0, :, 5:].all() and has[1].all()
    if kind == "empty":
        assert not has[1].any()


def test_embed_rows_match_embedding():
    g0 = _gen(5)
    tok, pos = torch.randn(50, 64, generator=g0), torch.randn(9, 64, generator=g0)
    ids = torch.randint(0, 50, (3, 7), generator=g0)
    want = (F.embedding(ids, tok) + pos[:7][None]).reshape(21, 64)
    assert torch.equal(R.embed_rows(ids, tok, pos, torch.float32), want)
    assert torch.equal(R.embed_rows(ids, tok, pos), (F.embedding(ids, tok.double()) + pos[:7].double()[None]).reshape(21, 64))


def _captions(vocab, S, gen):
    ids = torch.randint(3, vocab - 1, (8, S), generator=gen)
    ids[0, 0] = vocab - 1                                    # EOS first
    ids[1, S - 1] = vocab - 1                                # EOS last
    ids[3, 2] = ids[3, S - 2] = vocab - 1                    # two EOS: the first counts          (row 2: none)
    ids[4] = torch.randint(3, 20, (S,), generator=gen)
    ids[4, 1] = ids[4, 3] = 30                               # the maximum twice, no EOS
    ids[5:, S // 2] = vocab - 1
    return ids


@pytest.mark.parametrize("S", [5, 77])
def test_eos_rules_and_pack_plan(S):
    vocab = 100
    ids = _captions(vocab, S, _gen(S))
    first = R.eos_positions(ids, vocab - 1)
    assert torch.equal(first, (ids == vocab - 1).int().argmax(-1))          # HF: first position of eos, 0 when absent
    assert first.tolist()[:5] == [0, S - 1, 0, 2, 0]
    for legacy in (2, -1):
        got = R.eos_positions(ids, legacy)
        assert torch.equal(got, ids.argmax(-1)) and np.array_equal(got.numpy(), O.eos_positions(ids.numpy(), legacy))
        assert got[4] == 1
    assert np.array_equal(first.numpy(), O.eos_positions(ids.numpy(), vocab - 1))
    ln, cu, rowmap = R.pack_plan(ids, vocab - 1)
    assert torch.equal(ln.long(), first + 1) and torch.equal(cu.long(), torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(first + 1, 0)]))
    b = torch.repeat_interleave(torch.arange(8), ln.long())
    s = torch.arange(int(cu[-1])) - cu.long()[b]
    assert torch.equal(rowmap.long(), (b << 8) | s) and ln[2] == 1


@pytest.mark.parametrize("eos_id", [None, 99, 2])
@pytest.mark.parametrize("normalize", [False, True])
def test_pooled_head_matches_the_oracle(eos_id, normalize):
    """oracle/clip_oracle.py text_tower / vision_tower tail: LayerNorm of EVERY row, then the pick, then the projection"""
    g0 = _gen(7)
    B, S, D, P = 8, 9, 64, 40
    x = torch.randn(B, S, D, generator=g0).double() * 2 + 0.5
    w, b = torch.randn(D, generator=g0).double(), torch.randn(D, generator=g0).double()
    W = torch.randn(P, D, generator=g0).double()
    ids = None if eos_id is None else _captions(100, S, g0)
    got = R.pooled_head(x, ids, eos_id if eos_id is not None else -1, w, b, 1e-5, W, normalize)
    ln = O.layer_norm(x.numpy(), w.numpy(), b.numpy(), 1e-5)
    pos = np.zeros(B, np.int64) if ids is None else O.eos_positions(ids.numpy(), eos_id)
    want = ln[np.arange(B), pos] @ W.numpy().T
    if normalize:
        want = O.l2_normalize(want)
    assert np.abs(got.numpy() - want).max() < 1e-12
    assert np.abs(R.pooled_head(x, ids, eos_id if eos_id is not None else -1, w, b, 1e-5).numpy() - ln[np.arange(B), pos]).max() < 1e-12


def test_topk_and_first_argmax_match_numpy():
    rs = np.random.RandomState(11)
    sc = rs.randint(-3, 4, size=(6, 300)).astype(np.float32)                # many ties
    sc[0, 5:40] = -np.inf
    sc[1, 7] = sc[1, 250] = np.inf
    sc[2, ::7] = np.nan
    clean = np.where(np.isnan(sc), -np.inf, sc)
    for k in (1, 50, 300):
        np.testing.assert_array_equal(R.topk_stable(sc, k), np.argsort(-clean, axis=1, kind="stable")[:, :k])
    np.testing.assert_array_equal(R.first_argmax(clean), np.argmax(clean, axis=1))
    tie = np.zeros((3, 130), np.float32)
    tie[0, [63, 64]] = 2.0
    tie[1, [5, 69]] = 2.0
    tie[2, 129] = 1.0
    assert R.first_argmax(tie).tolist() == [63, 5, 129] == np.argmax(tie, axis=1).tolist()


def test_tolerance_helpers():
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(3.0) == 2.0 ** -22
    ref = torch.tensor([1.0, 3.0, 0.0], dtype=torch.float64)
    assert R.ulp16(ref, torch.bfloat16)[:2].tolist() == [2.0 ** -8, 3 * 2.0 ** -8] and R.ulp16(ref, torch.float16)[2].item() == 2.0 ** -24
    cpu = torch.tensor([1.0 + 2.0 ** -20, 3.0, 0.0])
    bound, err = R.fp32_bound(cpu, ref)
    assert abs(err - 2.0 ** -20) < 1e-12 and bound == 4 * err
    assert R.fp32_bound(ref.float(), ref)[0] == R.ulp32(3.0)                # floor: one fp32 ulp of the largest magnitude
    assert R.fp32_bound(cpu, ref, cap=1e-7)[0] == 1e-7


# ---- the vision front end (tests/test_gpu_front_end.py) ---------------------------------------------------------------------------------
FRONT_END_CASES = [(32, 64, 96), (16, 52, 72), (16, 48, 50), (14, 30, 44), (15, 31, 47)]


@pytest.mark.parametrize("P,H,W", FRONT_END_CASES)
def test_unfold_ref_is_torch_unfold_with_zero_padding(P, H, W):
    B, K = 3, 3 * P * P
    kpad = (K + 63) // 64 * 64
    px = torch.randn(B, 3, H, W, generator=_gen(P * H)).double()
    got = R.unfold_ref(px, P, kpad)
    gh, gw = H // P, W // P
    want = F.unfold(px[:, :, :gh * P, :gw * P], kernel_size=P, stride=P).transpose(1, 2).reshape(B * gh * gw, K)
    assert got.shape == (B * gh * gw, kpad) and torch.equal(got[:, :K], want)
    assert (got[:, K:] == 0).all()
    # element by element on a few rows, from the definition
    for row, k in ((0, 0), (B * gh * gw - 1, K - 1), (gw + 1 if gh > 1 and gw > 1 else 0, P * P + P + 1)):
        b, cell = divmod(row, gh * gw)
        gi, gj = divmod(cell, gw)
        c, rem = divmod(k, P * P)
        u, v = divmod(rem, P)
        assert got[row, k] == px[b, c, gi * P + u, gj * P + v]
    # the remainder pixels the grid floors away never appear: poisoning them changes nothing
    px2 = px.clone()
    px2[:, :, gh * P:, :] = float("nan")
    px2[:, :, :, gw * P:] = float("nan")
    assert torch.equal(R.unfold_ref(px2, P, kpad), got)


@pytest.mark.parametrize("P,H,W", FRONT_END_CASES)
def test_patch_embed_ref_is_the_unfolded_rows_times_the_weights(P, H, W):
    """unfold_ref @ W^T + pos == the conv2d form, CLS rows cls + pos[0]"""
    B, N, K = 3, 24, 3 * P * P
    g0 = _gen(W)
    px = torch.randn(B, 3, H, W, generator=g0).double()
    w = torch.randn(N, K, generator=g0).double() / K ** 0.5
    np_ = (H // P) * (W // P)
    pos, cls = torch.randn(np_ + 1, N, generator=g0).double(), torch.randn(N, generator=g0).double()
    ref = R.patch_embed_ref(px, w, P, pos, cls)
    assert ref.shape == (B, np_ + 1, N)
    rows = R.unfold_ref(px, P, (K + 63) // 64 * 64)[:, :K] @ w.T
    want = rows.reshape(B, np_, N) + pos[None, 1:]
    assert (ref[:, 1:] - want).abs().max().item() < 1e-12
    assert torch.equal(ref[:, 0], (cls + pos[0])[None].expand(B, N))
    assert torch.isnan(R.patch_embed_ref(px, w, P, pos)[:, 0]).all()
    # against HF's module arithmetic: conv -> flatten(2).transpose(1, 2), cat with the class row, + position embedding
    conv = F.conv2d(px, w.reshape(N, 3, P, P), stride=P).flatten(2).transpose(1, 2)
    hf = torch.cat((cls.expand(B, 1, N), conv), dim=1) + pos[None]
    assert (ref - hf).abs().max().item() < 1e-12


def test_u8_norm_ref_is_three_fp32_roundings_per_byte():
    """every byte value and channel, against scalar numpy float32 arithmetic, and within fp32 round-off of the float64 transform"""
    tiles = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()
    got = R.u8_norm_ref(tiles)
    assert got.dtype == torch.float32 and got.shape == (1, 3, 16, 16)
    for c in range(3):
        mean, istd = np.float32(R.CLIP_MEAN[c]), np.float32(1.0) / np.float32(R.CLIP_STD[c])
        for b in range(256):
            x = np.float32(np.float32(b) / np.float32(255.0))
            x = np.float32(np.float32(x - mean) * istd)
            assert got[0, c, b // 16, b % 16].item() == float(x), (c, b)
        exact = (np.arange(256, dtype=np.float64) / 255.0 - R.CLIP_MEAN[c]) / R.CLIP_STD[c]
        assert np.abs(got[0, c].reshape(-1).numpy().astype(np.float64) - exact).max() < 4 * 2.0 ** -24 * 3
    # the layout: HWC bytes -> NCHW planes
    t2 = torch.randint(0, 256, (2, 5, 7, 3), generator=_gen(5), dtype=torch.uint8)
    g2 = R.u8_norm_ref(t2)
    assert g2.shape == (2, 3, 5, 7)
    assert g2[1, 2, 4, 6].item() == got[0, 2].reshape(-1)[int(t2[1, 4, 6, 2])].item()


# ---- round_to: the 16-bit roundings the value-range GPU test compares the kernels' stores with ---------------------------------------
def _rne_rational(x, p, emin):
    """x (a finite float) rounded to nearest even on the grid of a binary format with p significand bits and smallest normal
    exponent emin, in exact rational arithmetic; no overflow handling (the caller's values stay in range)"""
    from fractions import Fraction
    if x == 0:
        return 0.0
    fx = Fraction(abs(x))
    e = emin
    while fx >= Fraction(2) ** (e + 1):
        e += 1
    unit = Fraction(2) ** (e - (p - 1))                     # spacing of the binade (of the subnormals below 2^emin)
    q, r = divmod(fx, unit)
    if r * 2 > unit or (r * 2 == unit and q % 2 == 1):
        q += 1
    return float(q * unit) * (1 if x > 0 else -1)


_FMT = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}


@pytest.mark.parametrize("dtype", list(_FMT), ids=["bf16", "f16"])
def test_round_to_is_one_nearest_even_rounding_from_float64(dtype):
    """against exact rational arithmetic: random values over the type's whole range, ties, near-ties that a detour through a
    nearest fp32 would round the wrong way, subnormals"""
    p, emin = _FMT[dtype]
    g0 = _gen(11)
    lo_e, hi_e = (emin - p - 2, 15) if dtype == torch.float16 else (emin - p - 2, 126)
    e = torch.randint(lo_e, hi_e + 1, (4000,), generator=g0).double()
    x = (torch.rand(4000, generator=g0, dtype=torch.float64) + 1.0) * torch.pow(torch.tensor(2.0, dtype=torch.float64), e)
    x = x * torch.where(torch.rand(4000, generator=g0) < 0.5, -1.0, 1.0).double()
    x = x[x.abs() <= (65504.0 if dtype == torch.float16 else 3.3e38)]
    ties = []
    for k in (-3, 0, 5, emin, emin - 3):                     # midpoints of neighbours, and the same a float64 ulp / an fp32 half-ulp off
        u = 2.0 ** (k - (p - 1)) if k >= emin else 2.0 ** (emin - (p - 1))
        base = 2.0 ** k if k >= emin else 3 * u
        for m in (base + 0.5 * u, base + 1.5 * u, base + 0.5 * u * (1 + 2.0 ** -30), base + 1.5 * u * (1 - 2.0 ** -30),
                  base + 0.5 * u + base * 2.0 ** -52, base + 1.5 * u - base * 2.0 ** -52):
            ties += [m, -m]
    x = torch.cat((x, torch.tensor(ties, dtype=torch.float64)))
    got = R.round_to(x, dtype)
    assert got.dtype == dtype
    want = torch.tensor([_rne_rational(float(v), p, emin) for v in x], dtype=torch.float64)
    assert torch.equal(got.double(), want)
    assert (got.double() != x).any()


def test_round_to_f16_saturates_keeps_nan_and_underflows_gradually():
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([65504.0, 65519.9, 65520.0, 65536.0, 1e30, inf, -65519.9, -65520.0, -inf, nan,
                      2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -40), 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, -(2.0 ** -26), 0.0, -0.0,
                      2049.0, 2051.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], dtype=torch.float64)
    want = [65504.0, 65504.0, 65504.0, 65504.0, 65504.0, 65504.0, -65504.0, -65504.0, -65504.0, nan,
            2.0 ** -24, 0.0, 2.0 ** -24, 2.0 ** -23, 2.0 ** -23, -0.0, 0.0, -0.0,
            2048.0, 2052.0, 1.0, 1.0 + 2.0 ** -9]
    got = R.round_to(x, torch.float16)
    assert got.dtype == torch.float16
    for g, w, v in zip(got.double().tolist(), want, x.tolist()):
        assert (g != g and w != w) or (g == w and np.signbit(g) == np.signbit(w)), (v, g, w)


def test_round_to_bf16_overflows_to_inf_and_is_torchs_conversion_on_fp32_values():
    inf, nan = float("inf"), float("nan")
    big = float(torch.tensor(3.3895313892515355e38))          # the largest bf16
    x = torch.tensor([big, big * (1 + 2.0 ** -10), big * (1 + 2.0 ** -8), 1e300, inf, -inf, nan, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
                      2.0 ** -133, 2.0 ** -134, 2.0 ** -134 * 1.0000001, -0.0], dtype=torch.float64)
    want = [big, big, inf, inf, inf, -inf, nan, 1.0, 1.0 + 2.0 ** -6, 2.0 ** -133, 0.0, 2.0 ** -133, -0.0]
    for g, w, v in zip(R.round_to(x, torch.bfloat16).double().tolist(), want, x.tolist()):
        assert (g != g and w != w) or (g == w and np.signbit(g) == np.signbit(w)), (v, g, w)
    g0 = _gen(12)
    f = (torch.randn(20000, generator=g0) * torch.exp(torch.empty(20000).uniform_(-80, 80, generator=g0)))
    f = torch.cat((f, torch.tensor([1.00390625, 1.01171875, inf, -inf, 3.39e38, -3.4e38, 1e-40, -9.2e-41])))   # two ties, overflow, subnormals
    assert torch.equal(R.round_to(f.double(), torch.bfloat16).view(torch.int16), f.to(torch.bfloat16).view(torch.int16))


def test_round_to_f16_agrees_with_the_hi_plane_of_split_planes():
    """kernel_entries.split_planes is the host mirror of the kernels' split store; its ``hi`` is the same saturating rounding of an
    fp32 value -- over the whole range, the saturating values and +-inf included"""
    from plip_amd.kernel_entries import split_planes
    g0 = _gen(13)
    f = torch.randn(64, 512, generator=g0) * torch.exp2(torch.randint(-30, 20, (64, 512), generator=g0).float())
    f[0, :8] = torch.tensor([65504.0, 65519.99, 65520.0, -65520.0, float("inf"), float("-inf"), 5.96e-8, 2.98e-8])
    hi, _ = split_planes(f, torch.float16)
    got = R.round_to(f.double(), torch.float16)
    assert torch.equal(got.view(torch.int16), hi.view(torch.int16))
    assert (got.abs() == 65504).sum() > 100 and ((got != 0) & (got.abs() < 2.0 ** -14)).sum() > 1000 and (got == 0).sum() > 1000


def test_ord16_counts_units_in_the_last_place():
    for dtype in (torch.float16, torch.bfloat16):
        t = torch.tensor([-2.0, -1.0, -0.0, 0.0, 1.0], dtype=dtype)
        o = R.ord16(t)
        assert o[2] == 0 and o[3] == 0 and (o[1:] >= o[:-1]).all()
        one = torch.tensor([1.0], dtype=dtype)
        nxt = (one.view(torch.int16) + 1).view(dtype)
        assert int(R.ord16(nxt) - R.ord16(one)) == 1 and int(R.ord16(-nxt) - R.ord16(-one)) == -1
    tiny = torch.tensor([2.0 ** -24, -(2.0 ** -24)], dtype=torch.float16)
    assert R.ord16(tiny).tolist() == [1, -1]
