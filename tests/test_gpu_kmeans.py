"""K-means on the GPU (include/plipmi.h "k-means on cached embeddings", csrc/kmeans.hip) against the numpy float64 oracle of
tests/kmeans_common.py -- never against the code under test.

Every call here goes through ``_Run``: X is carved out of a larger NaN-filled buffer, every output buffer is sentinel-filled and carries
guard rows past N or K that must come back untouched.

Bounds.  Integer data (|x|, |c| <= 4, D <= 1024): every product, sum, bias and distance is an integer or a half-integer below 2^24, so
fp32 is exact in any order and the kernels must equal the oracle bit for bit.  Random data: ``small_kernel_refs.fp32_bound`` -- 4 x the
error the same formula makes in plain numpy float32 on the same inputs, never below one fp32 ulp of the largest value.  Every test
prints its figures before it asserts (profiles/kmeans_parity.txt keeps them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import kmeans_common as KM
from small_kernel_refs import fp32_bound

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 5                       # guard rows behind every buffer
LABEL_SENTINEL, FLOAT_SENTINEL = -77, -12345.5
METRICS = {KM.EUCLIDEAN: 0, KM.COSINE: 1}
ERR_INVALID = 1


@pytest.fixture(scope="module")
def eng():
    from plip_amd.engine import heads_engine
    return heads_engine()


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


class _Run:
    """the raw entries on guarded, sentinel-filled buffers"""

    def __init__(self, eng, x):
        from plip_amd._lib import _ptr
        self.eng, self.ptr = eng, _ptr
        x = np.ascontiguousarray(x, dtype=np.float32)
        self.n, self.d = x.shape
        self.big = torch.full((self.n + 2 * GUARD, self.d), float("nan"), dtype=torch.float32, device=DEV)
        self.big[GUARD:GUARD + self.n] = torch.from_numpy(x).to(DEV)
        self.x = self.big[GUARD:GUARD + self.n]
        assert self.x.data_ptr() % 16 == 0

    def out(self, rows, dtype, cols=None):
        shape = (rows + GUARD,) if cols is None else (rows + GUARD, cols)
        fill = LABEL_SENTINEL if dtype == torch.int32 else FLOAT_SENTINEL
        return torch.full(shape, fill, dtype=dtype, device=DEV)

    @staticmethod
    def untouched(t, rows):
        fill = LABEL_SENTINEL if t.dtype == torch.int32 else FLOAT_SENTINEL
        return bool((t[rows:] == fill).all())

    @staticmethod
    def all_untouched(*ts):
        return all(_Run.untouched(t, 0) for t in ts)

    def check_x(self):
        assert torch.isnan(self.big[:GUARD]).all() and torch.isnan(self.big[GUARD + self.n:]).all()

    def stream(self):
        return self.eng._stream()

    def assign(self, centers, metric, n=None, d=None, k=None, x_ptr="x", expect=0):
        c = torch.from_numpy(np.ascontiguousarray(centers, dtype=np.float32)).to(DEV)
        n, d, k = self.n if n is None else n, self.d if d is None else d, c.shape[0] if k is None else k
        labels, scores = self.out(self.n, torch.int32), self.out(self.n, torch.float32)
        xp = self.ptr(self.x) if x_ptr == "x" else x_ptr
        rc = self.eng.lib.plipmi_kmeans_assign(self.eng._h, xp, n, d, self.ptr(c), k, metric, self.ptr(labels), self.ptr(scores), self.stream())
        torch.cuda.synchronize()
        assert rc == expect, (rc, expect)
        if expect:
            assert self.all_untouched(labels, scores)
            return None
        assert self.untouched(labels, self.n) and self.untouched(scores, self.n)
        self.check_x()
        return labels[:self.n].cpu().numpy(), scores[:self.n].cpu().numpy()

    def update(self, labels, scores, k, metric):
        lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(DEV)
        sc = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(DEV)
        sums, counts, reps = self.out(k, torch.float32, self.d), self.out(k, torch.int32), self.out(k, torch.int32)
        inertia = torch.full((1 + GUARD,), FLOAT_SENTINEL, dtype=torch.float64, device=DEV)
        from plip_amd.kernel_entries import kmeans_update
        kmeans_update(self.eng, self.x, lab, sc, sums, counts, reps, inertia, metric, n=self.n, k=k)
        torch.cuda.synchronize()
        assert self.untouched(sums, k) and self.untouched(counts, k) and self.untouched(reps, k) and bool((inertia[1:] == FLOAT_SENTINEL).all())
        self.check_x()
        return sums[:k].cpu().numpy(), counts[:k].cpu().numpy(), reps[:k].cpu().numpy(), float(inertia[0])

    def seed(self, k, metric, u):
        u = np.ascontiguousarray(u, dtype=np.float64)
        centers, picks = self.out(k, torch.float32, self.d), self.out(k, torch.int32)
        rc = self.eng.lib.plipmi_kmeans_seed(self.eng._h, self.ptr(self.x), self.n, self.d, k, metric, u.ctypes.data_as(C.POINTER(C.c_double)),
                                             self.ptr(centers), self.ptr(picks), self.stream())
        torch.cuda.synchronize()
        assert rc == 0 and self.untouched(centers, k) and self.untouched(picks, k)
        self.check_x()
        return centers[:k].cpu().numpy(), picks[:k].cpu().numpy()

    def fit(self, c0, metric, max_iter=300, tol_abs=0.0, k=None, n=None, d=None, expect=0):
        from plip_amd import _lib
        c0 = np.ascontiguousarray(c0, dtype=np.float32)
        k_rows = c0.shape[0]
        centers = self.out(k_rows, torch.float32, self.d)
        centers[:k_rows] = torch.from_numpy(c0).to(DEV)
        labels, scores = self.out(self.n, torch.int32), self.out(self.n, torch.float32)
        counts, reps = self.out(k_rows, torch.int32), self.out(k_rows, torch.int32)
        info = _lib.KMeansInfo()
        rc = self.eng.lib.plipmi_kmeans_fit(self.eng._h, self.ptr(self.x), self.n if n is None else n, self.d if d is None else d,
                                            k_rows if k is None else k, metric, max_iter, float(tol_abs), self.ptr(centers), self.ptr(labels),
                                            self.ptr(scores), self.ptr(counts), self.ptr(reps), C.byref(info), self.stream())
        torch.cuda.synchronize()
        assert rc == expect, (rc, expect)
        if expect:
            assert self.all_untouched(labels, scores, counts, reps) and self.untouched(centers, k_rows)
            assert np.array_equal(centers[:k_rows].cpu().numpy(), c0)
            return None
        for t, rows in ((centers, k_rows), (labels, self.n), (scores, self.n), (counts, k_rows), (reps, k_rows)):
            assert self.untouched(t, rows)
        self.check_x()
        return dict(centers=centers[:k_rows].cpu().numpy(), labels=labels[:self.n].cpu().numpy(), scores=scores[:self.n].cpu().numpy(),
                    counts=counts[:k_rows].cpu().numpy(), reps=reps[:k_rows].cpu().numpy(), inertia=float(info.inertia),
                    n_iter=int(info.iterations), converged=bool(info.converged), relocations=int(info.relocations),
                    shift=float(info.center_shift))


# ---- assignment, exact ------------------------------------------------------------------------------------------------------------------
# (N, D, K): one row and one centre; below, at and above the 32-row tile; below, at and above a group of 16 centres; more than one
# workgroup's tiles; every column-tile width from the narrowest (D = 4) to the widest, no-prefetch one (D = 1024); 19 groups
EXACT_SHAPES = [(1, 4, 1), (31, 36, 2), (32, 4, 15), (33, 36, 16), (33, 512, 17), (1000, 36, 33), (1000, 1024, 300), (1000, 512, 300),
                (31, 1024, 16)]


def _exact_case(n, d, k, metric, seed):
    x = KM.integer_rows(n, d, seed)
    c = KM.integer_rows(k, d, seed + 100) if metric == KM.EUCLIDEAN else KM.signed_axes(k, d, seed + 100)
    # ties: the same centre at both ends of a group of 16, across groups and at the very end; duplicated rows
    for dst, src in ((15, 0), (16, 0), (31, 17), (k - 1, 1)):
        if 0 <= src < dst < k:
            c[dst] = c[src]
    if n > 2:
        x[n - 1] = x[0]
        x[1] = x[0]
    return x, c


@pytest.mark.parametrize("metric", [KM.EUCLIDEAN, KM.COSINE])
@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_assignment_equals_the_integer_oracle_bit_for_bit(eng, shape, metric):
    n, d, k = shape
    x, c = _exact_case(n, d, k, metric, seed=n + d + k)
    want_l, want_s = KM.assign(x, c, metric)
    assert np.array_equal(want_s, want_s.astype(np.float32).astype(np.float64)), "the case is not exactly representable in fp32"
    got_l, got_s = _Run(eng, x).assign(c, METRICS[metric])
    full = KM.all_scores(x, c, metric)
    ties = int(((full == full.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    print(f"ASSIGN exact {metric} N={n} D={d} K={k}: rows with a tied maximum {ties}, label differences {int((got_l != want_l).sum())}, "
          f"score differences {int((got_s != want_s.astype(np.float32)).sum())}")
    if k > 16 and n > 2:
        assert ties > 0, "the case was meant to hold ties"
    assert np.array_equal(got_l, want_l) and np.array_equal(got_s, want_s.astype(np.float32))
    if n > 2:
        assert got_l[1] == got_l[0] == got_l[n - 1]


# ---- assignment, random data --------------------------------------------------------------------------------------------------------------
_RANDOM = {}


def _random(i, metric):
    """the case and its float64 / float32 references, computed once"""
    if (i, metric) not in _RANDOM:
        x, c = KM.random_case(i, metric)
        lab64, s64 = KM.assign(x, c, metric)
        _, s32 = KM.assign(x, c, metric, np.float32)
        _RANDOM[(i, metric)] = (x, c, lab64, s64, s32, KM.margins(x, c, metric))
    return _RANDOM[(i, metric)]


@pytest.mark.parametrize("metric", [KM.EUCLIDEAN, KM.COSINE])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_assignment_on_random_data_is_within_the_fp32_bound(eng, i, metric):
    x, c, lab64, s64, s32, margin = _random(i, metric)
    bound, err32 = fp32_bound(torch.from_numpy(s32), _t64(s64))
    # fixture validity, on the oracle alone: no row's float64 margin is under twice the bound, so no row is excused
    assert margin.min() >= 2 * bound, (margin.min(), bound)
    got_l, got_s = _Run(eng, x).assign(c, METRICS[metric])
    err = float(np.abs(got_s.astype(np.float64) - s64).max())
    print(f"ASSIGN random {metric} {KM.RANDOM_SHAPES[i]}: score err {err:.3e} (numpy fp32 {err32:.3e}, bound {bound:.3e})  smallest margin "
          f"{margin.min():.3e} = {margin.min() / bound:.1f} x bound  label differences {int((got_l != lab64).sum())}")
    assert err <= bound
    assert np.array_equal(got_l, lab64)


# ---- update -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [KM.EUCLIDEAN, KM.COSINE])
@pytest.mark.parametrize("shape,mode", [((1000, 36, 33), "holes"), ((700, 512, 17), "one"), ((33, 4, 3), "holes"), ((2049, 1024, 300), "holes")])
def test_update_equals_the_integer_oracle(eng, shape, mode, metric):
    n, d, k = shape
    rng = np.random.default_rng(n + k)
    x = KM.integer_rows(n, d, seed=n)
    if mode == "one":
        labels = np.full(n, 5, np.int32)                  # every row in one cluster: 3 chunks of it, every other cluster empty
    else:
        labels = rng.choice(np.arange(0, k, 2), n).astype(np.int32)      # the odd clusters stay empty
    scores = rng.integers(-40, 41, n).astype(np.float32) / 2             # many equal scores: the representative is a tie-break
    want = KM.update(x, labels, scores, k, metric)
    run = _Run(eng, x)
    got = run.update(labels, scores, k, METRICS[metric])
    print(f"UPDATE exact {metric} N={n} D={d} K={k} ({mode}): sums differences {int((got[0] != want[0]).sum())}, counts {int((got[1] != want[1]).sum())}, "
          f"reps {int((got[2] != want[2]).sum())}, inertia {got[3]} vs {want[3]}")
    assert np.array_equal(got[0], want[0].astype(np.float32)) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[3] == want[3]
    assert (want[1] == 0).any() and (got[2][want[1] == 0] == -1).all()
    again = run.update(labels, scores, k, METRICS[metric])
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3])) and got[3] == again[3]


@pytest.mark.parametrize("metric", [KM.EUCLIDEAN, KM.COSINE])
@pytest.mark.parametrize("i", [0, 1])
def test_update_on_random_data_is_within_the_fp32_bound_and_repeats_bit_for_bit(eng, i, metric):
    x, c, lab64, s64, s32, _ = _random(i, metric)
    k = len(c)
    scores = s64.astype(np.float32)
    want = KM.update(x, lab64, scores, k, metric)
    cpu32 = KM.update(x, lab64, scores, k, metric, np.float32)
    b_sums, e_sums = fp32_bound(torch.from_numpy(cpu32[0]), _t64(want[0]))
    b_in, e_in = fp32_bound(torch.tensor([float(cpu32[3])], dtype=torch.float32), _t64([want[3]]))
    run = _Run(eng, x)
    got = run.update(lab64, scores, k, METRICS[metric])
    err_s, err_i = float(np.abs(got[0].astype(np.float64) - want[0]).max()), abs(got[3] - want[3])
    print(f"UPDATE random {metric} {KM.RANDOM_SHAPES[i]}: sums err {err_s:.3e} (numpy fp32 {e_sums:.3e}, bound {b_sums:.3e})  inertia err "
          f"{err_i:.3e} (numpy fp32 {e_in:.3e}, bound {b_in:.3e})")
    assert err_s <= b_sums and err_i <= b_in
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    again = run.update(lab64, scores, k, METRICS[metric])
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3])) and got[3] == again[3]


# ---- seeding ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [KM.EUCLIDEAN, KM.COSINE])
@pytest.mark.parametrize("n,d,k", [(1000, 36, 17), (3000, 512, 9), (40, 4, 40)])
def test_seeding_on_integer_rows_equals_the_oracle(eng, n, d, k, metric):
    x = KM.integer_rows(n, d, seed=n + 1)
    u = np.random.default_rng(k).random(k)
    want = KM.seed(x, k, metric, u)
    centers, picks = _Run(eng, x).seed(k, METRICS[metric], u)
    print(f"SEED exact {metric} N={n} D={d} K={k}: pick differences {int((picks != want).sum())}")
    assert np.array_equal(picks, want) and np.array_equal(centers, x[picks])


def test_seeding_when_all_rows_coincide_takes_the_lowest_rows_not_yet_picked(eng):
    x = np.tile(KM.integer_rows(1, 36, seed=9), (50, 1))
    u = np.array([0.5, 0.9, 0.1, 0.7, 0.3])
    _, picks = _Run(eng, x).seed(5, 0, u)
    assert picks.tolist() == KM.seed(x, 5, KM.EUCLIDEAN, u).tolist() == [25, 0, 1, 2, 3]


@pytest.mark.parametrize("metric", [KM.EUCLIDEAN, KM.COSINE])
def test_seeding_on_random_rows_gives_distinct_rows_and_repeats(eng, metric):
    x = np.random.default_rng(4).standard_normal((2049, 512))
    x = (KM.normalised(x) if metric == KM.COSINE else x).astype(np.float32)
    u = np.random.default_rng(5).random(64)
    run = _Run(eng, x)
    centers, picks = run.seed(64, METRICS[metric], u)
    assert len(set(picks.tolist())) == 64 and picks.min() >= 0 and picks.max() < len(x) and picks[0] == int(u[0] * len(x))
    assert np.array_equal(centers, x[picks])
    again = run.seed(64, METRICS[metric], u)
    assert np.array_equal(again[1], picks) and np.array_equal(again[0], centers)


# ---- fit --------------------------------------------------------------------------------------------------------------------------------
def _blob_case(metric):
    x, _, _ = KM.blobs(1000, 36, 5, seed=21)
    return (KM.normalised(x).astype(np.float32) if metric == KM.COSINE else x)


def _check_fit(eng, run, x, metric, out, ref, what):
    k = len(ref["centers"])
    # the returned centres are the update of ref["center_labels"]: the bound is what that update costs in plain numpy float32
    bound, e32 = fp32_bound(torch.from_numpy(KM.centres_of(x, ref["center_labels"], k, metric, np.float32)), _t64(ref["centers"]))
    err = float(np.abs(out["centers"].astype(np.float64) - ref["centers"]).max())
    print(f"FIT {what} {metric}: n_iter {out['n_iter']} (oracle {ref['n_iter']})  label differences {int((out['labels'] != ref['labels']).sum())}  "
          f"centre err {err:.3e} (bound {bound:.3e})  inertia {out['inertia']:.6f} (oracle {ref['inertia']:.6f})  relocations {out['relocations']}")
    assert np.array_equal(out["labels"], ref["labels"]) and out["n_iter"] == ref["n_iter"] and out["converged"] == ref["converged"]
    assert out["relocations"] == ref["relocations"]
    assert err <= bound
    lab, sc = run.assign(out["centers"], METRICS[metric])
    assert np.array_equal(lab, out["labels"]) and np.array_equal(sc, out["scores"])
    _, counts, reps, inertia = KM.update(x, out["labels"], out["scores"], k, metric)
    assert np.array_equal(out["counts"], counts) and np.array_equal(out["reps"], reps)
    assert abs(out["inertia"] - inertia) <= 1e-5 * max(1.0, inertia)


@pytest.mark.parametrize("metric", [KM.EUCLIDEAN, KM.COSINE])
@pytest.mark.parametrize("init", ["given", "k-means++"])
def test_fit_on_separated_blobs_equals_the_oracle(eng, metric, init):
    x = _blob_case(metric)
    run = _Run(eng, x)
    if init == "given":
        c0 = x[np.random.default_rng(8).choice(len(x), 5, replace=False)]
    else:
        c0, picks = run.seed(5, METRICS[metric], np.random.default_rng([0, 0]).random(5))
        assert np.array_equal(c0, x[picks])
    tol_abs = 1e-4 * float(x.astype(np.float64).var(axis=0).mean())
    out = run.fit(c0, METRICS[metric], tol_abs=tol_abs)
    ref = KM.lloyd(x, c0, metric, tol_abs=tol_abs)
    _check_fit(eng, run, x, metric, out, ref, f"blobs/{init}")
    again = run.fit(c0, METRICS[metric], tol_abs=tol_abs)
    for key in ("centers", "labels", "scores", "counts", "reps"):
        assert np.array_equal(out[key], again[key]), key
    assert (out["inertia"], out["n_iter"], out["shift"]) == (again["inertia"], again["n_iter"], again["shift"])


@pytest.mark.parametrize("metric", [KM.EUCLIDEAN, KM.COSINE])
def test_a_centre_far_from_every_row_is_relocated(eng, metric):
    x = _blob_case(metric)
    run = _Run(eng, x)
    c0 = x[np.random.default_rng(8).choice(len(x), 5, replace=False)].copy()
    # far from every row (euclidean) / opposite the data's mean direction (cosine): no row's best centre
    c0[2] = 1000.0 if metric == KM.EUCLIDEAN else -KM.normalised(x.astype(np.float64).mean(axis=0, keepdims=True))[0]
    out = run.fit(c0, METRICS[metric])
    ref = KM.lloyd(x, c0, metric)
    assert ref["relocations"] >= 1
    _check_fit(eng, run, x, metric, out, ref, "relocation")
    assert out["relocations"] >= 1 and (out["counts"] > 0).all()


def test_python_fit_assign_and_restarts(eng):
    from plip_amd.kmeans import kmeans_assign, kmeans_fit
    x = _blob_case(KM.COSINE)
    xd = torch.from_numpy(x).to(DEV)
    # restart r of seed 3 draws its uniforms from default_rng([3, r])
    import plip_amd.kmeans as km
    singles = []
    for r in range(3):
        c0, _ = km.kmeans_seed(eng, xd, 7, "cosine", uniforms=np.random.default_rng([3, r]).random(7))
        singles.append(kmeans_fit(eng, xd, 7, metric="cosine", init=c0))
    best = kmeans_fit(eng, xd, 7, metric="cosine", n_init=3, seed=3)
    inertias = [s.inertia for s in singles]
    print(f"FIT n_init=3: restart inertias {inertias}, kept {best.inertia}")
    assert best.inertia == min(inertias)
    keep = singles[int(np.argmin(inertias))]
    assert torch.equal(best.labels, keep.labels) and torch.equal(best.centers, keep.centers)
    assert best.labels.dtype == torch.int32 and best.counts.sum().item() == len(x) and best.converged and isinstance(best.n_iter, int)
    lab, sc = kmeans_assign(eng, x, best.centers, "cosine")          # host input
    assert torch.equal(lab, best.labels) and torch.equal(sc, best.scores)


def test_fit_on_unseparated_data_ends_at_a_fixed_point(eng):
    """A trajectory may leave float64's at a near-tie, so only invariants are tested.  Euclidean from the first K rows: the float64
    oracle needs six iterations there (spherical k-means on these rows is at its fixed point after two)."""
    M, m = KM.EUCLIDEAN, METRICS[KM.EUCLIDEAN]
    x = _random(1, M)[0]                                       # N = 2049, D = 512, K = 300
    c0 = x[:300]
    run = _Run(eng, x)
    out = run.fit(c0, m, max_iter=300, tol_abs=0.0)
    assert out["converged"] and 2 < out["n_iter"] < 300
    lab, sc = run.assign(out["centers"], m)
    assert np.array_equal(lab, out["labels"]) and np.array_equal(sc, out["scores"])
    assert (out["counts"] > 0).all()
    want = KM.centres_of(x, out["labels"], 300, M)
    bound, e32 = fp32_bound(torch.from_numpy(KM.centres_of(x, out["labels"], 300, M, np.float32)), _t64(want))
    err = float(np.abs(out["centers"].astype(np.float64) - want).max())
    start = KM.update(x, *KM.assign(x, c0, M), 300, M)[3]
    print(f"FIT unseparated: n_iter {out['n_iter']}  centre err vs update(labels) {err:.3e} (numpy fp32 {e32:.3e}, bound {bound:.3e})  "
          f"inertia {out['inertia']:.4f} (start {start:.4f})")
    assert err <= bound and out["inertia"] <= start
    two = run.fit(c0, m, max_iter=2, tol_abs=0.0)
    assert not two["converged"] and two["n_iter"] == 2
    lab2, _ = run.assign(two["centers"], m)
    assert np.array_equal(lab2, two["labels"])


# ---- PLIP on the tiny model ---------------------------------------------------------------------------------------------------------------
def test_region_mosaic_and_cluster_embeddings(engines):
    from region_common import synthetic_region
    from plip_amd.kmeans import kmeans_fit
    from plip_amd.plip import PLIP
    model = engines("tiny_b6", "f32")[0]
    plip, eng = PLIP(model=model), model.engine
    region = synthetic_region()
    kw = dict(tile_px=64, stride=40)                           # 15 tiles kept of 28
    reg = plip.encode_region(region, **kw)
    n = len(reg.kept)
    assert n == 15
    mosaic = plip.region_mosaic(region, 4, **kw)
    x = eng.l2_normalize_(torch.from_numpy(reg.embeddings.copy()).to(eng.device))
    ref = kmeans_fit(eng, x, 4, metric="cosine")
    assert np.array_equal(mosaic.labels, ref.labels.cpu().numpy()) and mosaic.labels.shape == (n,)
    reps = ref.representatives.cpu().numpy()
    assert np.array_equal(mosaic.representatives, reps) and np.array_equal(mosaic.rep_coords, reg.coords[reps])
    assert np.array_equal(mosaic.rep_kept, reg.kept[reps]) and np.array_equal(mosaic.counts, ref.counts.cpu().numpy())
    assert mosaic.counts.sum() == n and np.array_equal(mosaic.region.embeddings, reg.embeddings)
    # fewer tiles than clusters: K is lowered to the tile count, every tile its own cluster
    few = plip.region_mosaic(region, 100, **kw)
    assert few.counts.shape == (n,) and (few.counts == 1).all() and sorted(few.representatives.tolist()) == list(range(n))
    # no tissue: empty results (the engine is never asked: the embeddings are empty)
    glass = (240 + np.random.RandomState(5).randint(-3, 4, size=(150, 210, 3))).astype(np.uint8)
    none = plip.region_mosaic(glass, 4)
    assert none.labels.shape == (0,) and none.representatives.shape == (0,) and none.rep_coords.shape == (0, 2) and none.result is None
    # cluster_embeddings: numpy and device input give the same bits; cosine normalises first
    a = plip.cluster_embeddings(reg.embeddings, 4)
    b = plip.cluster_embeddings(torch.from_numpy(reg.embeddings.copy()).to(eng.device), 4)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.centers, b.centers) and torch.equal(a.labels, ref.labels)
    e = plip.cluster_embeddings(reg.embeddings, 3, metric="euclidean", init=reg.embeddings[:3])
    want = KM.lloyd(reg.embeddings, reg.embeddings[:3], KM.EUCLIDEAN, tol_abs=1e-4 * float(reg.embeddings.astype(np.float64).var(axis=0).mean()))
    assert np.array_equal(e.labels.cpu().numpy(), want["labels"])


# ---- refusals through the C ABI -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(eng):
    from plip_amd import _lib
    x = KM.integer_rows(40, 8, seed=1)
    run = _Run(eng, x)
    c = x[:4]
    for kw, word in ((dict(k=41), "min(N"), (dict(k=4097, n=5000), "4096"), (dict(d=6), "D % 4"), (dict(x_ptr=None), "null X")):
        assert run.assign(np.zeros((max(4, min(kw.get("k", 4), 4097)), 8), np.float32), 0, expect=ERR_INVALID, **kw) is None
        assert word in _lib.last_error(), (_lib.last_error(), word)
    assert run.assign(c, 7, expect=ERR_INVALID) is None and "metric" in _lib.last_error()
    for kw, word in ((dict(k=41), "min(N"), (dict(k=4097, n=5000), "4096"), (dict(d=6), "D % 4")):
        assert run.fit(c, 0, expect=ERR_INVALID, **kw) is None
        assert word in _lib.last_error(), (_lib.last_error(), word)
    assert run.fit(c, 2, expect=ERR_INVALID) is None and "metric" in _lib.last_error()
    assert run.fit(c, 0, max_iter=0, expect=ERR_INVALID) is None and "max_iter" in _lib.last_error()
    # misaligned X
    off = run.big.view(-1)[GUARD * 8 + 1:]
    assert run.assign(c, 0, x_ptr=run.ptr(off), n=30, expect=ERR_INVALID) is None and "16-byte" in _lib.last_error()
    # the seed entry: K > N and a uniform outside [0, 1)
    centers, picks = run.out(4, torch.float32, 8), run.out(4, torch.int32)
    u = np.array([0.1, 1.0, 0.2, 0.3])
    for k, uu in ((41, np.zeros(41)), (4, u)):
        rc = eng.lib.plipmi_kmeans_seed(eng._h, run.ptr(run.x), 40, 8, k, 0, uu.ctypes.data_as(C.POINTER(C.c_double)), run.ptr(centers),
                                        run.ptr(picks), run.stream())
        torch.cuda.synchronize()
        assert rc == ERR_INVALID and run.all_untouched(centers, picks)
