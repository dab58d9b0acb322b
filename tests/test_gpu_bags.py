"""The bag heads on the GPU (include/plipmi.h "bags of embeddings", csrc/bags.hip) against the numpy oracle of tests/bags_common.py --
never against the code under test.

Every raw call goes through ``_pool`` / ``_mean``: X is carved out of a larger NaN-filled buffer, every output buffer and the workspace
carry sentinel-filled guard elements that must come back untouched.

Bounds.  Integer data (|x|, |t| <= 4, scale 0.5, D <= 1024): every product and every sum is an integer or a half-integer below 2^24, so
fp32 is exact in any order, float64 sums are exact, and scores, pooled values, predictions and indices must equal the oracle bit for bit.
Random data: ``small_kernel_refs.fp32_bound`` for the scores (4 x the error of plain CPU fp32 on the same inputs, never below one fp32
ulp of the largest value); the selection is exact and the device adds the selected scores rank by rank as the oracle does, so given the
device's own scores the indices are the oracle's and pooled is within one fp32 ulp (in fact equal); end to end pooled is within the score
bound plus one ulp, because a top-K mean is 1-Lipschitz in the maximum norm (tests/test_bags_host.py).  Every test prints its figures
before it asserts (profiles/bag_pool_parity.txt keeps them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bags_common as BC
from small_kernel_refs import fp32_bound

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 5                       # guard rows / elements behind every buffer
INT_SENTINEL, FLOAT_SENTINEL = -77, -12345.5
ERR_INVALID = 1


@pytest.fixture(scope="module")
def eng():
    from plip_amd.engine import heads_engine
    return heads_engine()


def _ptr(t):
    from plip_amd._lib import _ptr as p
    return p(t)


def _guarded_x(x):
    """x on the device inside a NaN-filled buffer -> (view, buffer)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    big = torch.full((x.shape[0] + 2 * GUARD, x.shape[1]), float("nan"), dtype=torch.float32, device=DEV)
    big[GUARD:GUARD + x.shape[0]] = torch.from_numpy(x).to(DEV)
    view = big[GUARD:GUARD + x.shape[0]]
    assert view.data_ptr() % 16 == 0
    return view, big


def _out(n, dtype):
    return torch.full((n + GUARD,), INT_SENTINEL if dtype == torch.int32 else FLOAT_SENTINEL, dtype=dtype, device=DEV)


def _untouched(t, n):
    return bool((t[n:] == (INT_SENTINEL if t.dtype == torch.int32 else FLOAT_SENTINEL)).all())


def _workspace(eng, n, s, c, kmax):
    nbytes = int(eng.lib.plipmi_bag_workspace(n, s, c, kmax))
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.full((nbytes + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    return ws, nbytes


def _ks(ks):
    arr = np.ascontiguousarray(ks, dtype=np.int32)
    return arr, arr.ctypes.data_as(C.POINTER(C.c_int32))


def _pool(eng, off, ks, x=None, t=None, scale=1.0, scores=None, ld=None, want_idx=True, want_pred=True, want_scores=True, expect=0, **ov):
    """plipmi_bag_topk_pool (x, t given) or plipmi_bag_pool_scores (scores [C, N] given, laid out with leading dimension ld).  ``ov``
    overrides single arguments (N, D, S, C, nks, ld, X, T, offsets, ws, pooled) for the refusals.  -> dict of numpy arrays"""
    off = np.ascontiguousarray(off, dtype=np.int32)
    S = len(off) - 1
    ksa, ksp = _ks(ks)
    kmax = int(ksa[-1]) if len(ksa) and 1 <= ksa[-1] <= 1024 else 1
    nks_alloc = max(len(ksa), 1)
    if scores is None:
        xv, xbig = _guarded_x(x)
        td = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(DEV)
        N, D, Cn = xv.shape[0], xv.shape[1], td.shape[0]
    else:
        sc = np.asarray(scores, dtype=np.float32)
        Cn, N = sc.shape
        ld = N if ld is None else ld
        sbuf = torch.full((Cn, max(ld, N)), float("nan"), dtype=torch.float32, device=DEV)      # (ld < N: a refusal, nothing is read)
        sbuf[:, :N] = torch.from_numpy(sc).to(DEV)
    od = torch.from_numpy(off).to(DEV)
    ws, nbytes = _workspace(eng, N, S, Cn, kmax)
    pooled = _out(S * nks_alloc * Cn, torch.float32)
    pred = _out(S * nks_alloc, torch.int32) if want_pred else None
    top = _out(S * Cn * kmax, torch.int32) if want_idx else None
    a = dict(N=N, S=S, C=Cn, nks=len(ksa), offsets=_ptr(od), ws=_ptr(ws), pooled=_ptr(pooled))
    if scores is None:
        sout = _out(Cn * N, torch.float32) if want_scores else None
        a.update(D=D, X=_ptr(xv), T=_ptr(td))
        a.update(ov)
        rc = eng.lib.plipmi_bag_topk_pool(eng._h, a["X"], a["N"], a["D"], a["offsets"], a["S"], a["T"], a["C"], float(scale), ksp, a["nks"],
                                          a["ws"], a["pooled"], _ptr(pred), _ptr(top), _ptr(sout), eng._stream())
    else:
        sout = None
        a.update(ld=ld, scoresT=_ptr(sbuf))
        a.update(ov)
        rc = eng.lib.plipmi_bag_pool_scores(eng._h, a["scoresT"], a["ld"], a["N"], a["C"], a["offsets"], a["S"], ksp, a["nks"], a["ws"],
                                            a["pooled"], _ptr(pred), _ptr(top), eng._stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect, eng.lib.plipmi_last_error())
    outs = [o for o in (pooled, pred, top, sout) if o is not None]
    if expect:                                         # a refusal launches nothing: every output and the workspace are as they were
        assert all(_untouched(o, 0) for o in outs) and bool((ws == 0xAB).all())
        return eng.lib.plipmi_last_error().decode()
    assert _untouched(pooled, S * len(ksa) * Cn) and bool((ws[nbytes:] == 0xAB).all())
    res = {"pooled": pooled[:S * len(ksa) * Cn].reshape(S, len(ksa), Cn).cpu().numpy()}
    if want_pred:
        assert _untouched(pred, S * len(ksa))
        res["pred"] = pred[:S * len(ksa)].reshape(S, len(ksa)).cpu().numpy()
    if want_idx:
        assert _untouched(top, S * Cn * kmax)
        res["top_idx"] = top[:S * Cn * kmax].reshape(S, Cn, kmax).cpu().numpy()
    if sout is not None:
        assert _untouched(sout, Cn * N)
        res["scores"] = sout[:Cn * N].reshape(Cn, N).cpu().numpy()
    if scores is None:
        assert torch.isnan(xbig[:GUARD]).all() and torch.isnan(xbig[GUARD + N:]).all()
    return res


def _mean(eng, x, off, normalize, expect=0, **ov):
    off = np.ascontiguousarray(off, dtype=np.int32)
    S = len(off) - 1
    xv, xbig = _guarded_x(x)
    N, D = xv.shape
    od = torch.from_numpy(off).to(DEV)
    ws, nbytes = _workspace(eng, N, S, 1, 1)
    mean = _out(S * D, torch.float32)
    a = dict(N=N, D=D, S=S, X=_ptr(xv), offsets=_ptr(od), ws=_ptr(ws), mean=_ptr(mean))
    a.update(ov)
    rc = eng.lib.plipmi_bag_mean(eng._h, a["X"], a["N"], a["D"], a["offsets"], a["S"], int(normalize), a["ws"], a["mean"], eng._stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect, eng.lib.plipmi_last_error())
    if expect:
        assert _untouched(mean, 0) and bool((ws == 0xAB).all())
        return eng.lib.plipmi_last_error().decode()
    assert _untouched(mean, S * D) and bool((ws[nbytes:] == 0xAB).all())
    return mean[:S * D].reshape(S, D).cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _in_bag(top, off, kmax):
    """every index written lies in its bag, the first min(kmax, n_b) are written and the rest is -1"""
    for b in range(len(off) - 1):
        m = min(kmax, int(off[b + 1] - off[b]))
        w = top[b, :, :m]
        if not ((w >= off[b]) & (w < off[b + 1])).all() or not (top[b, :, m:] == -1).all():
            return False
    return True


def _check_exact(what, got, want, off, kmax):
    pooled, pred, top = want
    mism = {"pooled": int((~((got["pooled"] == pooled) | (np.isnan(got["pooled"]) & np.isnan(pooled)))).sum()),
            "pred": int((got["pred"] != pred).sum()), "top_idx": int((got["top_idx"] != top).sum())}
    print(f"bag parity: {what}: mismatches {mism}")
    assert mism == {"pooled": 0, "pred": 0, "top_idx": 0} and _in_bag(got["top_idx"], off, kmax)


# ---- integer data: bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [1, 2, 9, 16, 17, 64])
@pytest.mark.parametrize("D", [4, 36, 512, 1024])
def test_integer_data_equals_the_oracle_bit_for_bit(eng, D, C_):
    sizes = BC.mixed_sizes()
    assert max(sizes) > 2 * BC.CHUNK                   # 9 000 rows at the kernel's chunk of 2 048: five pieces, four merges
    off = BC.offsets_of(sizes)
    x, t = BC.integer_case(D, C_, sizes)
    s64 = BC.scores64(x, t, 0.5)
    assert np.abs(s64).max() < 2 ** 24 and np.array_equal(s64.astype(np.float32).astype(np.float64), s64)
    got = _pool(eng, off, BC.KS, x=x, t=t, scale=0.5)
    bad = int((got["scores"].astype(np.float64) != s64).sum())
    print(f"bag parity: integer D {D} C {C_} N {len(x)}: score mismatches {bad}")
    assert bad == 0
    _check_exact(f"integer D {D} C {C_} ks {BC.KS}", got, BC.pool(s64, off, BC.KS), off, BC.KS[-1])


@pytest.mark.parametrize("D,C_", [(36, 9), (512, 17)])
def test_integer_data_with_k_1024(eng, D, C_):
    """(1, 1024): the 1 000-row bag is shorter than k, the 1 500-row bag is longer, the long bag merges lists of 1 024"""
    sizes = BC.mixed_sizes()
    off = BC.offsets_of(sizes)
    x, t = BC.integer_case(D, C_, sizes, seed=1)
    s64 = BC.scores64(x, t, 0.5)
    got = _pool(eng, off, (1, 1024), x=x, t=t, scale=0.5)
    assert np.array_equal(got["scores"].astype(np.float64), s64)
    _check_exact(f"integer D {D} C {C_} ks (1, 1024)", got, BC.pool(s64, off, (1, 1024)), off, 1024)


def test_smallest_call(eng):
    got = _pool(eng, [0, 1], (1,), x=np.full((1, 4), 2.0, np.float32), t=np.full((1, 4), 3.0, np.float32), scale=0.5)
    assert got["scores"].tolist() == [[12.0]] and got["pooled"].tolist() == [[[12.0]]] and got["pred"].tolist() == [[0]]
    assert got["top_idx"].tolist() == [[[0]]]


# ---- ties --------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_row(eng):
    rng = np.random.default_rng(5)
    long_rows = 3 * BC.CHUNK + 500
    sizes = [300, 700, long_rows, 40]
    off = BC.offsets_of(sizes)
    x = rng.integers(-1, 2, size=(int(off[-1]), 8)).astype(np.float32)
    x[:300] = x[0]                                     # a bag of identical rows
    t = rng.integers(-1, 2, size=(5, 8)).astype(np.float32)
    t[0] = (1, 1, 1, 0, 0, 0, 0, 0)                    # class 0: one row in 27 holds the best score
    s64 = BC.scores64(x, t, 0.5)
    want = BC.pool(s64, off, BC.KS)
    # the cases are there: ties straddle every rank k in the long bag (in 20 or more of the 25 class x k pairs), and its best score is held by rows of more than one chunk
    lo, hi = int(off[2]), int(off[3])
    srt = -np.sort(-s64[:, lo:hi], axis=1)
    straddle = np.array([[srt[c, k - 1] == srt[c, k] for k in BC.KS] for c in range(5)])      # rank k and rank k + 1 hold one score
    assert straddle.any(axis=0).all() and straddle.sum() >= 20
    best_rows = lo + np.flatnonzero(s64[0, lo:hi] == s64[0, lo:hi].max())
    assert len(set(best_rows // BC.CHUNK)) >= 4 and len(best_rows) > BC.KS[-1]
    assert len(np.unique(s64)) <= 17
    got = _pool(eng, off, BC.KS, x=x, t=t, scale=0.5)
    assert np.array_equal(got["scores"].astype(np.float64), s64)
    _check_exact("ties, D 8", got, want, off, BC.KS[-1])
    assert (got["top_idx"][0, :, :100] == np.arange(100)[None, :]).all()      # identical rows: ranks are the rows in order


# ---- pooling of given scores -------------------------------------------------------------------------------------------------------
def test_pooling_of_given_scores_with_special_values(eng):
    rng = np.random.default_rng(6)
    sizes = [50, 0, 2 * BC.CHUNK + 404, 300]
    off = BC.offsets_of(sizes)
    n = int(off[-1])
    s = rng.standard_normal((3, n)).astype(np.float32)
    s[0, 7] = np.inf                                   # bag 0: an infinity on top of class 0
    s[1, 11], s[1, 30], s[1, 31], s[1, 40] = np.nan, -np.inf, np.nan, -np.inf      # bag 0, class 1: NaN ranks as -inf, by row
    b3 = int(off[3])
    s[2, b3:b3 + 300] = -np.abs(s[2, b3:b3 + 300]) - 1.0          # bag 3, class 2: both zeros on top, told apart by the row only
    s[2, b3 + 5:b3 + 300:9] = -0.0
    s[2, b3 + 2:b3 + 300:9] = 0.0
    den = np.array([1, -1, 3, 2, -2, 0x7fffff], np.int64)        # bag 3, class 0: denormals around the zeros
    s[0, b3:b3 + 300] = (den[rng.integers(0, len(den), 300)] * 2.0 ** -149).astype(np.float32)
    s[0, b3 + 1:b3 + 300:7] = -0.0
    s[0, b3 + 4:b3 + 300:7] = 0.0
    s[1, int(off[2]) + BC.CHUNK - 3] = np.nan          # the long bag: a NaN that is never selected
    assert (np.abs(s[0, b3:b3 + 300]) < 2.0 ** -126).all()
    want = BC.pool(s, off, BC.KS)
    got = _pool(eng, off, BC.KS, scores=s, ld=n + 7)
    idx_bad = int((got["top_idx"] != want[2]).sum())
    finite = np.zeros(want[0].shape, bool)
    for b in range(len(sizes)):
        for c in range(3):
            for j, k in enumerate(BC.KS):
                m = min(k, sizes[b])
                finite[b, j, c] = m > 0 and np.isfinite(s[c, want[2][b, c, :m]]).all()
    pooled_bad = int((_bits(got["pooled"])[finite] != _bits(want[0])[finite]).sum())
    print(f"bag parity: given scores, ld = N + 7: index mismatches {idx_bad}, pooled mismatches {pooled_bad} of {int(finite.sum())} finite "
          f"({finite.size - int(finite.sum())} not finite or empty)")
    assert idx_bad == 0 and pooled_bad == 0 and _in_bag(got["top_idx"], off, BC.KS[-1])
    assert finite.sum() >= 30 and not finite[0, -1, 0] and not finite[0, -1, 1] and finite[3].all() and finite[2].all()
    assert np.isnan(got["pooled"][1]).all() and (got["pred"][1] == -1).all()
    assert want[2][0, 1, 46:50].tolist() == [11, 30, 31, 40] and got["pooled"][0, 0, 0] == np.inf


# ---- random data -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_run(eng):
    sizes = list(BC.SIZES) + [20000]
    off = BC.offsets_of(sizes)
    x, t = BC.random_case(512, 9, sizes)
    assert len(x) == sum(sizes) == 22912
    x64, t64 = torch.from_numpy(x).to(torch.float64), torch.from_numpy(t).to(torch.float64)
    ref64 = 100.0 * (t64 @ x64.T)
    cpu32 = np.float32(100.0) * (torch.from_numpy(t) @ torch.from_numpy(x).T)
    bound, cpu_err = fp32_bound(cpu32, ref64)
    s64 = ref64.numpy()
    p64 = BC.pooled64(s64, off, BC.KS)
    margin = BC.margins(p64)
    nonempty = np.diff(off) > 0
    print(f"bag parity: random D 512 C 9 N {len(x)}: score bound {bound:.3e} (cpu fp32 error {cpu_err:.3e}), smallest float64 margin "
          f"{np.nanmin(margin):.3e} = {np.nanmin(margin) / bound:.0f} x bound")
    assert (margin[nonempty] >= 2 * bound).all()       # on the oracle alone: every prediction is decided beyond the rounding
    got = _pool(eng, off, BC.KS, x=x, t=t, scale=100.0)
    return dict(x=x, t=t, off=off, sizes=sizes, s64=s64, p64=p64, bound=bound, got=got, nonempty=nonempty)


def test_random_scores_are_within_the_fp32_bound(random_run):
    r = random_run
    err = np.abs(r["got"]["scores"].astype(np.float64) - r["s64"]).max()
    print(f"bag parity: random: worst score error {err:.3e} = {err / r['bound']:.3f} x bound {r['bound']:.3e}")
    assert err <= r["bound"]


def test_random_selection_is_exact_on_the_devices_own_scores(random_run):
    r = random_run
    pooled, pred, top = BC.pool(r["got"]["scores"], r["off"], BC.KS)
    ne = r["nonempty"]
    idx_bad = int((r["got"]["top_idx"] != top).sum())
    ulps = np.abs(r["got"]["pooled"][ne].astype(np.float64) - pooled[ne].astype(np.float64)) / BC.ulp32(pooled[ne])
    print(f"bag parity: random, oracle pooling of the device's scores: index mismatches {idx_bad}, pooled worst {ulps.max():.0f} ulp, "
          f"pred mismatches {int((r['got']['pred'] != pred).sum())}")
    assert idx_bad == 0 and ulps.max() <= 1 and np.array_equal(r["got"]["pred"], pred)
    assert np.isnan(r["got"]["pooled"][~ne]).all() and _in_bag(r["got"]["top_idx"], r["off"], BC.KS[-1])


def test_random_pooled_is_within_the_score_bound_end_to_end(random_run):
    r = random_run
    ne = r["nonempty"]
    err = np.abs(r["got"]["pooled"][ne].astype(np.float64) - r["p64"][ne])
    allowed = r["bound"] + BC.ulp32(r["p64"][ne])
    print(f"bag parity: random: worst pooled error {err.max():.3e} against score bound + 1 ulp {allowed.min():.3e}")
    assert (err <= allowed).all()


def test_random_predictions_equal_the_float64_oracle(random_run):
    r = random_run
    want = np.where(r["nonempty"][:, None], np.argmax(np.nan_to_num(r["p64"], nan=-np.inf), axis=2), -1).astype(np.int32)
    bad = int((r["got"]["pred"] != want).sum())
    print(f"bag parity: random: prediction mismatches {bad} of {want.size}")
    assert bad == 0
    assert len(set(want[r["nonempty"]].ravel().tolist())) >= 5        # (the bags do lean towards different classes)


# ---- invariance and repeatability --------------------------------------------------------------------------------------------------
def test_a_bag_pooled_alone_gives_the_bits_it_gives_in_the_big_call(eng, random_run):
    r = random_run
    diffs = 0
    for b in np.flatnonzero(r["nonempty"]):
        lo, hi = int(r["off"][b]), int(r["off"][b + 1])
        alone = _pool(eng, [0, hi - lo], BC.KS, x=r["x"][lo:hi], t=r["t"], scale=100.0)
        diffs += int(not _same_bits(alone["scores"], r["got"]["scores"][:, lo:hi]))
        diffs += int(not _same_bits(alone["pooled"][0], r["got"]["pooled"][b])) + int(not np.array_equal(alone["pred"][0], r["got"]["pred"][b]))
        shifted = np.where(alone["top_idx"][0] >= 0, alone["top_idx"][0] + lo, -1)
        diffs += int(not np.array_equal(shifted, r["got"]["top_idx"][b]))
    print(f"bag parity: bags alone against the big call: {diffs} differing outputs over {int(r['nonempty'].sum())} bags")
    assert diffs == 0


def test_topk_pool_equals_scores_then_pool_scores_and_repeats(eng, random_run):
    r = random_run
    again = _pool(eng, r["off"], BC.KS, x=r["x"], t=r["t"], scale=100.0)
    two = _pool(eng, r["off"], BC.KS, scores=r["got"]["scores"], ld=len(r["x"]) + 3)
    quiet = _pool(eng, r["off"], BC.KS, x=r["x"], t=r["t"], scale=100.0, want_idx=False, want_pred=False, want_scores=False)
    for name in ("pooled", "pred", "top_idx", "scores"):
        assert _same_bits(again[name], r["got"][name]), name
    for name in ("pooled", "pred", "top_idx"):
        assert _same_bits(two[name], r["got"][name]), name
    assert _same_bits(quiet["pooled"], r["got"]["pooled"])


# ---- bag mean ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 36, 512, 1024])
def test_bag_mean_integer_data(eng, D):
    sizes = [0, 1, 4, 0, 0, 32, 100, 2 * BC.CHUNK + 904, 1000, 0]
    off = BC.offsets_of(sizes)
    x, _ = BC.integer_case(D, 1, sizes, seed=2)
    # sums are integers below 2^24; only power-of-two bag sizes divide exactly, the others round once, as the oracle does
    got, want = _mean(eng, x, off, False), BC.bag_mean(x, off, False)
    bad = int((_bits(got) != _bits(want)).sum())
    print(f"bag parity: mean, integer D {D}: {bad} differing values")
    assert bad == 0 and not got[[0, 3, 4, 9]].any()
    assert _same_bits(_mean(eng, x, off, False), got)


def test_bag_mean_random_data_and_normalize(eng):
    sizes = list(BC.SIZES) + [3 * BC.CHUNK + 77]
    off = BC.offsets_of(sizes)
    rng = np.random.default_rng(9)
    x = BC.unit_rows(int(off[-1]), 512, rng) + np.float32(0.05)
    x64 = torch.from_numpy(x).to(torch.float64)
    ne = np.diff(off) > 0
    ref64 = torch.stack([x64[off[b]:off[b + 1]].mean(dim=0) if ne[b] else torch.zeros(512, dtype=torch.float64) for b in range(len(sizes))])
    cpu32 = torch.stack([torch.from_numpy(x[off[b]:off[b + 1]]).mean(dim=0) if ne[b] else torch.zeros(512) for b in range(len(sizes))])
    bound, cpu_err = fp32_bound(cpu32, ref64)
    got = _mean(eng, x, off, False)
    err = np.abs(got.astype(np.float64) - ref64.numpy()).max()
    print(f"bag parity: mean, random D 512 N {len(x)}: error {err:.3e}, bound {bound:.3e} (cpu fp32 error {cpu_err:.3e}); "
          f"against the oracle {int((_bits(got) != _bits(BC.bag_mean(x, off, False))).sum())} values differ")
    assert err <= bound and not got[~ne].any()
    unit, want = _mean(eng, x, off, True), BC.bag_mean(x, off, True)
    ref_unit = ref64 / ref64.norm(dim=1, keepdim=True).clamp_min(1e-300)
    nbound, _ = fp32_bound(cpu32 / cpu32.norm(dim=1, keepdim=True).clamp_min(1e-30), ref_unit)
    nerr = np.abs(unit.astype(np.float64) - ref_unit.numpy()).max()
    oerr = np.abs(unit.astype(np.float64) - want.astype(np.float64)).max()
    print(f"bag parity: mean, normalize: error {nerr:.3e}, bound {nbound:.3e}; against the oracle {oerr:.3e}")
    assert nerr <= nbound and oerr <= 2 * float(BC.ulp32(1.0)) and not unit[~ne].any()
    assert _same_bits(_mean(eng, x, off, True), unit)
    zero = _mean(eng, np.concatenate([x[:8], -x[:8]]), [0, 16], True)
    assert not zero.any()                              # a zero mean has no direction: zeros, not NaN


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_limit_and_launch_nothing(eng):
    x = np.ones((40, 8), np.float32)
    t = np.ones((3, 8), np.float32)
    off = [0, 10, 40]
    s = np.ones((3, 40), np.float32)
    good = _pool(eng, off, (1, 5), x=x, t=t)
    assert good["pooled"].shape == (2, 2, 3)
    xv, _ = _guarded_x(x)
    cases = [
        (dict(X=None), "null X"), (dict(T=None), "null X / T"), (dict(offsets=None), "null offsets"), (dict(ws=None), "null offsets / workspace"),
        (dict(pooled=None), "pooled"), (dict(S=0), "S >= 1"), (dict(C=0), "1 <= C <= 64"), (dict(C=65), "1 <= C <= 64"),
        (dict(nks=0), "1 <= nks <= 8"), (dict(nks=9), "1 <= nks <= 8"), (dict(N=0), "N > 0"), (dict(D=6), "D % 4 == 0"),
        (dict(D=1028), "4 <= D <= 1024"), (dict(X=C.c_void_p(xv.data_ptr() + 4)), "X must be 16-byte aligned"),
    ]
    for ov, message in cases:
        msg = _pool(eng, off, (1, 5), x=x, t=t, expect=ERR_INVALID, **ov)
        assert message in msg, (ov, msg)
    td = torch.zeros((4, 8), dtype=torch.float32, device=DEV)
    assert "T must be 16-byte aligned" in _pool(eng, off, (1, 5), x=x, t=t, expect=ERR_INVALID, T=C.c_void_p(td.data_ptr() + 4))
    ws = torch.zeros((1 << 16,), dtype=torch.uint8, device=DEV)
    assert "workspace must be 16-byte aligned" in _pool(eng, off, (1, 5), x=x, t=t, expect=ERR_INVALID, ws=C.c_void_p(ws.data_ptr() + 8))
    for ks, message in (((0, 5), "outside 1 .. 1024"), ((5, 1025), "outside 1 .. 1024"), ((5, 5), "strictly ascending"), ((7, 3), "strictly ascending")):
        assert message in _pool(eng, off, ks, x=x, t=t, expect=ERR_INVALID), ks
        assert message in _pool(eng, off, ks, scores=s, expect=ERR_INVALID), ks
    for ov, message in ((dict(ld=39), "ld >= N"), (dict(scoresT=None), "null scoresT"), (dict(N=0), "N > 0"), (dict(S=0), "S >= 1"),
                        (dict(C=65), "1 <= C <= 64"), (dict(nks=9), "1 <= nks <= 8"), (dict(offsets=None), "null offsets")):
        assert message in _pool(eng, off, (1, 5), scores=s, expect=ERR_INVALID, **ov), ov
    for ov, message in ((dict(X=None), "null X"), (dict(mean=None), "mean"), (dict(S=0), "S >= 1"), (dict(D=2), "4 <= D <= 1024"),
                        (dict(N=-1), "N > 0"), (dict(offsets=None), "null offsets"), (dict(ws=None), "workspace")):
        assert message in _mean(eng, x, off, True, expect=ERR_INVALID, **ov), ov
    assert eng.lib.plipmi_bag_topk_pool(None, None, 1, 4, None, 1, None, 1, 1.0, None, 1, None, None, None, None, None, None) == ERR_INVALID


def test_offsets_the_python_layer_would_refuse_are_clamped_on_the_device(eng):
    """the C entry cannot see the contents of offsets: whatever they hold, nothing is read or written outside the buffers (guards), and the
    bags are those of the clamped, non-decreasing array"""
    x, t = BC.integer_case(8, 3, [60])
    raw = np.array([-5, 20, 10, 2 ** 30, 7], np.int32)
    clean = np.array([0, 20, 20, 60, 60], np.int32)
    got = _pool(eng, raw, (1, 5), x=x, t=t, scale=0.5)
    s64 = BC.scores64(x, t, 0.5)
    _check_exact("hostile offsets", got, BC.pool(s64, clean, (1, 5)), clean, 5)
    assert _same_bits(_mean(eng, x, raw, False), BC.bag_mean(x, clean, False))


# ---- routes ------------------------------------------------------------------------------------------------------------------------
CASE = "tiny_b6"


def _fake_tokenizer(cfg):
    """deterministic stand-in for CLIPTokenizer (no vocabulary files offline): words hashed to ids"""
    def fn(texts, context_length):
        ids = np.full((len(texts), context_length), cfg.eos_token_id, dtype=np.int64)
        mask = np.zeros_like(ids)
        for i, text in enumerate(texts):
            toks = [cfg.bos_token_id] + [1 + (sum(map(ord, w)) * 31 + len(w)) % (cfg.bos_token_id - 2) for w in text.lower().split()][:context_length - 2]
            toks.append(cfg.eos_token_id)
            ids[i, :len(toks)] = toks
            mask[i, :len(toks)] = 1
        return ids, mask
    return fn


@pytest.fixture(scope="module")
def plip(engines):
    from plip_amd.plip import PLIP
    model, cfg, *_ = engines(CASE, "f32")
    return PLIP(model=model, tokenizer=_fake_tokenizer(cfg))


CLASSES = [["tumor", "carcinoma"], ["stroma"], ["lymphocytes", "immune cells", "lymphoid aggregate"]]
TEMPLATES = ("an h&e image of {}", "a photo of {} tissue")


def test_class_prototypes_equal_numpy_on_encode_text(plip):
    protos = plip.class_prototypes(CLASSES, templates=TEMPLATES)
    prompts = [t.format(s) for syn in CLASSES for s in syn for t in TEMPLATES]
    emb = plip.encode_text(prompts, batch_size=4)
    e64 = torch.from_numpy(emb).to(torch.float64)
    e32 = torch.from_numpy(emb)
    want64, want32, at = [], [], 0
    for syn in CLASSES:
        n = len(syn) * len(TEMPLATES)
        for e, out in ((e64, want64), (e32, want32)):
            rows = e[at:at + n]
            m = (rows / rows.norm(dim=1, keepdim=True)).mean(dim=0)
            out.append(m / m.norm())
        at += n
    bound, cpu_err = fp32_bound(torch.stack(want32), torch.stack(want64))
    err = float((torch.from_numpy(protos).to(torch.float64) - torch.stack(want64)).abs().max())
    print(f"bag parity: class prototypes [{protos.shape[0]}, {protos.shape[1]}]: error {err:.3e}, bound {bound:.3e} (cpu fp32 error {cpu_err:.3e})")
    assert protos.shape == (3, emb.shape[1]) and protos.dtype == np.float32 and err <= bound
    single = plip.class_prototypes(["stroma"], templates="{}")
    one = plip.encode_text(["stroma"], batch_size=1)[0].astype(np.float64)
    assert np.abs(single[0] - one / np.linalg.norm(one)).max() <= 2 * float(BC.ulp32(1.0))


def test_slide_zero_shot_forms_give_the_same_bits(plip):
    rng = np.random.default_rng(11)
    P = plip.model.config.projection_dim
    protos = plip.class_prototypes(CLASSES, templates=TEMPLATES)
    sizes = [7, 120, 0, 33]
    ids_of_bag = [4, 9, None, 17]
    bags = [(rng.standard_normal((n, P)) * 3 + protos[b % 3] * 2).astype(np.float32) for b, n in enumerate(sizes)]
    emb = np.concatenate(bags)
    off = BC.offsets_of(sizes)
    a = plip.slide_zero_shot(bags, protos, ks=(1, 5, 50), return_top_tiles=5)
    b = plip.slide_zero_shot((emb, off), protos, ks=(1, 5, 50), return_top_tiles=5)
    ids = np.concatenate([np.full(n, i) for n, i in zip(sizes, ids_of_bag) if n])
    perm = rng.permutation(len(ids))
    c = plip.slide_zero_shot((torch.from_numpy(emb[perm]), ids[perm]), protos, ks=(1, 5, 50), return_top_tiles=5)
    keep = [0, 1, 3]                                   # the ids form has no empty slide
    assert a["ks"] == b["ks"] == c["ks"] == (1, 5, 50) and a["pooled"].shape == (4, 3, 3) and c["pooled"].shape == (3, 3, 3)
    assert _same_bits(a["pooled"], b["pooled"]) and np.array_equal(a["pred"], b["pred"])
    assert _same_bits(a["pooled"][keep], c["pooled"]) and np.array_equal(a["pred"][keep], c["pred"])
    assert np.isnan(a["pooled"][2]).all() and (a["pred"][2] == -1).all() and (a["top_tiles"][2] == -1).all()
    # the same tiles, each form in its own index space
    assert np.array_equal(np.where(a["top_tiles"] >= 0, a["top_tiles"] + off[:-1][:, None, None], -1), b["top_tiles"])
    assert np.array_equal(emb[perm][c["top_tiles"][1, 0]], emb[b["top_tiles"][1, 0]])
    # against the oracle on the rows the device normalised, at the model's scale
    scale = float(np.exp(float(plip.model.logit_scale)))
    unit = plip.model.engine.l2_normalize_(torch.from_numpy(emb).to(plip.model.engine.device)).cpu().numpy()
    s64 = BC.scores64(unit, protos, np.float32(scale))
    bound, _ = fp32_bound(np.float32(scale) * (torch.from_numpy(protos) @ torch.from_numpy(unit).T), torch.from_numpy(s64))
    p64 = BC.pooled64(s64, off, (1, 5, 50))
    err = np.nanmax(np.abs(a["pooled"].astype(np.float64) - p64))
    print(f"bag parity: slide_zero_shot at scale {scale:.2f}: pooled error {err:.3e}, score bound {bound:.3e}")
    assert err <= bound + float(BC.ulp32(np.nanmax(np.abs(p64))))
    named = plip.slide_zero_shot(bags, CLASSES, ks=(1, 5, 50), templates=TEMPLATES)
    assert _same_bits(named["pooled"], a["pooled"])


def test_region_zero_shot_equals_encode_region_then_bag_topk_pool(plip):
    from region_common import synthetic_region
    from plip_amd.bags import bag_topk_pool
    region = synthetic_region()
    protos = plip.class_prototypes(CLASSES, templates=TEMPLATES)
    out = plip.region_zero_shot(region, protos, ks=(1, 5, 10), return_top_tiles=4, stride=40)
    reg = plip.encode_region(region, stride=40)
    assert np.array_equal(out["region"].embeddings, reg.embeddings) and np.array_equal(out["region"].coords, reg.coords)
    n = reg.embeddings.shape[0]
    assert n == 15
    eng = plip.model.engine
    x = eng.l2_normalize_(torch.from_numpy(reg.embeddings.copy()).to(eng.device))
    want = bag_topk_pool(eng, x, np.array([0, n], np.int32), protos, ks=(1, 5, 10), scale=float(np.exp(float(plip.model.logit_scale))),
                         return_indices=True)
    assert _same_bits(out["pooled"], want["pooled"].cpu().numpy()) and np.array_equal(out["pred"], want["pred"].cpu().numpy())
    top = want["top_idx"].cpu().numpy()[:, :, :4]
    assert np.array_equal(out["top_tiles"], top) and out["top_coords"].shape == (3, 4, 2)
    assert np.array_equal(out["top_coords"], reg.coords[top[0]])
    glass = np.full((128, 128, 3), 240, np.uint8)
    none = plip.region_zero_shot(glass, protos, ks=(1, 5))
    assert np.isnan(none["pooled"]).all() and none["pooled"].shape == (1, 2, 3) and (none["pred"] == -1).all() and (none["top_coords"] == -1).all()


def test_slide_zero_shot_classifier_equals_the_oracle(eng):
    from plip_amd.reproducibility import SlideZeroShotClassifier
    rng = np.random.default_rng(12)
    labels = ["benign", "tumor", "necrosis"]
    txt = BC.unit_rows(3, 64, rng)
    slide_names = np.array(["s3", "s1", "s2", "s0", "s4"])
    sizes = [130, 20, 75, 300, 51]
    rows, ids = [], []
    for name, n in zip(slide_names, sizes):
        cls = int(name[1]) % 3
        rows.append(BC.unit_rows(n, 64, rng) + np.float32(0.4) * txt[cls])
        ids += [name] * n
    emb, ids = np.concatenate(rows).astype(np.float32), np.array(ids)
    perm = rng.permutation(len(ids))
    emb, ids = emb[perm], ids[perm]
    order = np.argsort(ids, kind="stable")
    off = BC.offsets_of([sizes[list(slide_names).index(s)] for s in np.unique(ids)])
    p64 = BC.pooled64(BC.scores64(emb[order], txt, 1.0), off, (50,))
    assert BC.margins(p64).min() > 1e-3
    want = [labels[i] for i in p64[:, 0].argmax(axis=1)]
    clf = SlideZeroShotClassifier(eng, k=50)
    got = clf.predict(emb, ids, txt, labels)
    print(f"bag parity: SlideZeroShotClassifier: {got}")
    assert got == want == [labels[i % 3] for i in range(5)]
    train, test = clf.zero_shot_classification(emb, ids, txt, labels, want)
    assert test["split"] == "test" and train["split"] == "train" and {k: v for k, v in test.items() if k != "split"} == \
        {k: v for k, v in train.items() if k != "split"}
