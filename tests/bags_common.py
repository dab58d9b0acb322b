"""Shared by tests/test_bags_host.py, tests/test_gpu_bags.py and tools/bag_pool_bench.py: the numpy statement of the bag heads as
include/plipmi.h "bags of embeddings" defines them, and the case generators.  Nothing here touches the GPU code.

    bag b = rows [offsets[b], offsets[b + 1]) of x [N, D]
    s[c, i] = scale * (x_i . t_c)                                   class-major [C, N]
    order: larger score first, equal scores: the lower row first; -0.0 == +0.0; NaN counts as -inf
    pooled[b, j, c] = float32(sum of the min(ks[j], n_b) first-ranked scores, SEQUENTIAL float64 / m); NaN for an empty bag
    pred[b, j] = first arg-max over c (a NaN never wins over a number); -1 for an empty bag
    top_idx[b, c, r] = row of rank r < min(kmax, n_b), -1 beyond
    mean[b] = float32(float64 sum of the rows in ascending order / n_b); normalize: that row / its float64 norm; zeros when empty
"""
import numpy as np

F64 = np.float64
CHUNK = 2048                      # csrc/bags.hip kBagChunk: rows per chunk of the row axis (a bag's pieces are its cuts at multiples of it)
SIZES = (0, 1, 4, 5, 6, 31, 32, 33, 99, 100, 101, 1000, 1500)
KS = (1, 5, 10, 50, 100)


def scores64(x, t, scale):
    """float64 [C, N]"""
    return F64(scale) * (np.asarray(t, dtype=F64) @ np.asarray(x, dtype=F64).T)


def order_keys(v):
    """the values the order compares: NaN -> -inf, -0.0 -> +0.0"""
    v = np.array(v, dtype=F64)
    v[np.isnan(v)] = -np.inf
    return v + 0.0


def rank_rows(v):
    """indices of ``v`` in rank order: value descending, index ascending"""
    k = order_keys(v)
    return np.lexsort((np.arange(len(k)), -k))


def seq_sum(v):
    """v[0] + v[1] + ... left to right in float64 (np.cumsum accumulates sequentially)"""
    v = np.asarray(v, dtype=F64)
    return np.cumsum(v)[-1] if len(v) else F64(0)


def pairwise_sum(v):
    v = np.asarray(v, dtype=F64)
    if len(v) <= 2:
        return seq_sum(v)
    h = len(v) // 2
    return pairwise_sum(v[:h]) + pairwise_sum(v[h:])


def pool(scores_t, offsets, ks, summer=seq_sum):
    """(pooled float32 [S, nks, C], pred int32 [S, nks], top_idx int32 [S, C, kmax]) of class-major scores [C, N] (any float dtype: the
    values are taken to float64 exactly)"""
    s = np.asarray(scores_t)
    C, S, kmax = s.shape[0], len(offsets) - 1, int(ks[-1])
    pooled = np.full((S, len(ks), C), np.nan, np.float32)
    pred = np.full((S, len(ks)), -1, np.int32)
    top = np.full((S, C, kmax), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(S):
            lo, hi = int(offsets[b]), int(offsets[b + 1])
            if hi <= lo:
                continue
            for c in range(C):
                v = s[c, lo:hi].astype(F64)
                r = rank_rows(v)[:kmax]
                top[b, c, :len(r)] = lo + r
                vals = order_keys(v)[r]
                vals = np.where(np.isnan(v[r]), np.nan, vals)       # a selected NaN makes the mean NaN (compared nowhere)
                for j, k in enumerate(ks):
                    m = min(int(k), hi - lo)
                    pooled[b, j, c] = np.float32(summer(vals[:m]) / F64(m))
            for j in range(len(ks)):
                row = pooled[b, j]
                best = 0
                for c in range(1, C):
                    if row[c] > row[best] or (np.isnan(row[best]) and not np.isnan(row[c])):
                        best = c
                pred[b, j] = best
    return pooled, pred, top


def pooled64(scores_t, offsets, ks):
    """float64 [S, nks, C] top-K means without the final rounding (NaN for an empty bag)"""
    s = np.asarray(scores_t, dtype=F64)
    C, S = s.shape[0], len(offsets) - 1
    out = np.full((S, len(ks), C), np.nan, F64)
    for b in range(S):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if hi <= lo:
            continue
        srt = -np.sort(-s[:, lo:hi], axis=1)
        for j, k in enumerate(ks):
            m = min(int(k), hi - lo)
            out[b, j] = srt[:, :m].sum(axis=1) / m
    return out


def margins(p64):
    """[S, nks]: the best pooled value minus the second best over the classes (inf for C == 1, NaN for an empty bag)"""
    if p64.shape[2] == 1:
        return np.where(np.isnan(p64[:, :, 0]), np.nan, np.inf)
    s = np.sort(p64, axis=2)
    return s[:, :, -1] - s[:, :, -2]


def bag_mean(x, offsets, normalize):
    x = np.asarray(x, dtype=F64)
    S = len(offsets) - 1
    out = np.zeros((S, x.shape[1]), np.float32)
    for b in range(S):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if hi <= lo:
            continue
        acc = np.zeros(x.shape[1], F64)
        for r in range(lo, hi):
            acc = acc + x[r]
        m = (acc / F64(hi - lo)).astype(np.float32)
        if normalize:
            nrm = np.sqrt((m.astype(F64) ** 2).sum())
            m = (m.astype(F64) / nrm).astype(np.float32) if nrm > 0 else np.zeros_like(m)
        out[b] = m
    return out


def ulp32(v):
    """one fp32 ulp at |v| (elementwise)"""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(F64)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int32)


def mixed_sizes(long_rows=None):
    """the size list with a leading, a trailing and two adjacent empty bags, and one bag longer than two chunks"""
    long_rows = 4 * CHUNK + 808 if long_rows is None else long_rows
    return [0, 1, 4, 5, 0, 0, 6, 31, 32, 33, 99, 100, long_rows, 101, 1000, 1500, 0]


def integer_case(D, C, sizes, seed=0, amp=4):
    """x [N, D], t [C, D] with integer entries in [-amp, amp]: every score (scale 0.5) and every float64 sum is exact"""
    rng = np.random.default_rng([seed, D, C])
    n = int(np.sum(sizes))
    x = rng.integers(-amp, amp + 1, size=(n, D)).astype(np.float32)
    t = rng.integers(-amp, amp + 1, size=(C, D)).astype(np.float32)
    return x, t


def unit_rows(n, D, rng):
    x = rng.standard_normal((n, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def random_case(D=512, C=9, sizes=None, seed=0):
    """unit rows and unit class vectors.  Class c is a fixed random direction; bag b's rows lean towards class b % C with a strength
    that differs from row to row, so that every bag has a clear best class at every k (the fixture checks the margin)."""
    sizes = list(SIZES) + [20000] if sizes is None else sizes
    rng = np.random.default_rng([seed, D, C])
    t = unit_rows(C, D, rng)
    rows = []
    for b, n in enumerate(sizes):
        if n == 0:
            continue
        lean = rng.uniform(0.2, 0.6, size=(n, 1))
        g = rng.standard_normal((n, D)) / np.sqrt(D) + lean * t[b % C].astype(F64)
        rows.append((g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32))
    return np.concatenate(rows), t
