"""Shared by tests/test_kmeans_host.py, tests/test_gpu_kmeans.py and tools/kmeans_bench.py: a numpy restatement of k-means as
include/plipmi.h defines it (assign, update, finalise, the empty-cluster rule, the seeding rule, Lloyd's loop), in float64 by default and
in any dtype on request (float32: what fp32 arithmetic alone costs on the same inputs), and the fixtures.  Nothing here touches the GPU
code; the Euclidean loop is pinned against scikit-learn by the host test.

    s_ik = x_i . c_k + h_k          euclidean: h_k = -|c_k|^2 / 2, d_i = max(0, |x_i|^2 - 2 s_i), centre = mean of the members
                                    cosine:    h_k = 0,            d_i = max(0, 1 - s_i),        centre = sum / |sum| (zero sum: empty)
    label_i = the FIRST arg-max over k;  rep_k = the member of largest score, ties to the lower row, -1 when empty;  inertia = sum d_i
"""
import numpy as np

EUCLIDEAN, COSINE = "euclidean", "cosine"
F64 = np.float64


def bias(c, metric, dt=F64):
    c = np.asarray(c, dtype=dt)
    return dt(-0.5) * (c * c).sum(axis=1) if metric == EUCLIDEAN else np.zeros(len(c), dt)


def all_scores(x, c, metric, dt=F64):
    """[N, K] scores"""
    return np.asarray(x, dtype=dt) @ np.asarray(c, dtype=dt).T + bias(c, metric, dt)[None, :]


def assign(x, c, metric, dt=F64):
    """(labels int32 [N], scores [N]): np.argmax returns the first maximum"""
    s = all_scores(x, c, metric, dt)
    lab = s.argmax(axis=1)
    return lab.astype(np.int32), s[np.arange(len(s)), lab]


def margins(x, c, metric):
    """float64 best score minus second best per row (inf for K == 1)"""
    s = np.sort(all_scores(x, c, metric), axis=1)
    return s[:, -1] - s[:, -2] if s.shape[1] > 1 else np.full(len(s), np.inf)


def dist(x, s, metric, dt=F64):
    x, s = np.asarray(x, dtype=dt), np.asarray(s, dtype=dt)
    if metric == EUCLIDEAN:
        return np.maximum(dt(0), (x * x).sum(axis=1) - dt(2) * s)
    return np.maximum(dt(0), dt(1) - s)


def update(x, labels, scores, K, metric, dt=F64):
    """(sums [K, D], counts int32 [K], reps int32 [K], inertia); a label outside [0, K) belongs to no cluster"""
    x = np.asarray(x, dtype=dt)
    labels = np.asarray(labels)
    ok = (labels >= 0) & (labels < K)
    sums = np.zeros((K, x.shape[1]), dt)
    counts = np.zeros(K, np.int32)
    reps = np.full(K, -1, np.int32)
    for k in range(K):
        rows = np.flatnonzero(ok & (labels == k))
        counts[k] = len(rows)
        if len(rows):
            sums[k] = x[rows].sum(axis=0, dtype=dt)
            sc = np.asarray(scores)[rows]
            reps[k] = rows[np.flatnonzero(sc == sc.max())[0]]
    d = dist(x, np.asarray(scores, dtype=dt), metric, dt)
    return sums, counts, reps, (d[ok].sum(dtype=dt) if dt == np.float32 else float(d[ok].sum()))


def finalise(sums, counts, old, metric):
    """(centres, shift, empty bool [K]): an empty cluster keeps its old centre and adds nothing to the shift"""
    sums, old = np.asarray(sums, F64), np.asarray(old, F64)
    c = old.copy()
    if metric == EUCLIDEAN:
        empty = np.asarray(counts) == 0
        c[~empty] = sums[~empty] / np.asarray(counts, F64)[~empty, None]
    else:
        nrm = np.sqrt((sums * sums).sum(axis=1))
        empty = (np.asarray(counts) == 0) | (nrm == 0)
        c[~empty] = sums[~empty] / nrm[~empty, None]
    return c, float(((c - old) ** 2).sum()), empty


def centres_of(x, labels, K, metric, dt=F64):
    """the update and finalise steps in ``dt`` throughout: the centres of the clusters ``labels`` describe (an empty one: zeros)"""
    x = np.asarray(x, dtype=dt)
    c = np.zeros((K, x.shape[1]), dt)
    for k in range(K):
        rows = np.flatnonzero(np.asarray(labels) == k)
        if len(rows):
            sm = x[rows].sum(axis=0, dtype=dt)
            c[k] = sm / dt(len(rows)) if metric == EUCLIDEAN else sm / np.sqrt((sm * sm).sum(dtype=dt))
    return c


def relocate(d, empty):
    """The empty-cluster rule: in ascending k, an empty cluster takes the row with the largest d not yet taken in this iteration, ties to
    the lower row.  Returns {k: row}."""
    d = np.asarray(d, F64).copy()
    out = {}
    for k in np.flatnonzero(empty):
        row = int(np.flatnonzero(d == d.max())[0])       # taken rows hold -inf
        out[int(k)] = row
        d[row] = -np.inf
    return out


def seed_pick(mind, u, taken):
    """One k-means++ pick: the first row whose float64 prefix sum of ``mind`` over ascending rows exceeds u * total; total == 0 (or no
    such row): the lowest row not in ``taken``."""
    cum = np.cumsum(np.asarray(mind, F64))
    total = cum[-1]
    if total > 0:
        hit = np.flatnonzero(cum > u * total)
        if len(hit):
            return int(hit[0])
    return next(i for i in range(len(mind)) if i not in taken)


def seed(x, K, metric, u):
    """plain k-means++ D^2 sampling from the K uniforms ``u``: picks int32 [K]"""
    x = np.asarray(x, F64)
    n = len(x)
    picks = [min(n - 1, int(u[0] * n))]
    mind = None
    for t in range(1, K):
        c = x[picks[-1]][None, :]
        d = dist(x, all_scores(x, c, metric)[:, 0], metric)
        mind = d if mind is None else np.minimum(mind, d)
        mind[picks] = 0.0
        picks.append(seed_pick(mind, u[t], set(picks)))
    return np.asarray(picks, np.int32)


def lloyd(x, c0, metric, max_iter=300, tol_abs=0.0):
    """Lloyd's loop as plipmi_kmeans_fit runs it (scikit-learn's order: assign, update, then the two stopping tests; an iteration that
    relocated a centre does not stop).  Returns a dict: centers, labels, scores, counts, reps, inertia, n_iter, converged, relocations,
    history (the inertia of every assignment)."""
    x = np.asarray(x, F64)
    c = np.asarray(c0, F64).copy()
    K = len(c)
    old = np.full(len(x), -1, np.int32)
    strict = converged = False
    relocations = n_iter = 0
    history = []
    for it in range(max_iter):
        labels, s = assign(x, c, metric)
        center_labels = labels                           # the labels the returned centres are the update of
        sums, counts, reps, inertia = update(x, labels, s, K, metric)
        history.append(inertia)
        c, shift, empty = finalise(sums, counts, c, metric)
        n_iter = it + 1
        changed = int((labels != old).sum())
        old = labels
        if empty.any():
            for k, row in relocate(dist(x, s, metric), empty).items():
                c[k] = x[row]
                relocations += 1
            continue
        if changed == 0:
            strict = converged = True
            break
        if shift <= tol_abs:
            converged = True
            break
    if not strict:
        labels, s = assign(x, c, metric)
        sums, counts, reps, inertia = update(x, labels, s, K, metric)
    return dict(centers=c, labels=labels, scores=s, counts=counts, reps=reps, inertia=inertia, n_iter=n_iter, converged=converged,
                relocations=relocations, history=history, center_labels=center_labels)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def normalised(x):
    x = np.asarray(x, F64)
    return x / np.sqrt((x * x).sum(axis=1, keepdims=True))


def blobs(n, d, k, seed, spread=8.0):
    """k separated Gaussian blobs: (x float32 [n, d], true labels, blob centres)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, d)) * spread
    lab = rng.integers(0, k, n)
    lab[:k] = np.arange(k)                               # every blob has a member
    x = centres[lab] + rng.standard_normal((n, d))
    return x.astype(np.float32), lab.astype(np.int32), centres


def integer_rows(n, d, seed, lo=-4, hi=4):
    return np.random.default_rng(seed).integers(lo, hi + 1, (n, d)).astype(np.float32)


def signed_axes(k, d, seed):
    """k unit-norm integer centres: +-e_j"""
    rng = np.random.default_rng(seed)
    c = np.zeros((k, d), np.float32)
    c[np.arange(k), rng.integers(0, d, k)] = rng.choice([-1.0, 1.0], k)
    return c


RANDOM_SHAPES = [(1000, 36, 17), (2049, 512, 300), (333, 768, 33)]      # (N, D, K), default_rng seeds 1, 2, 3


def random_case(i, metric):
    """X = standard_normal (normalised rows for cosine) as float32, centres = four float64 Lloyd iterations from the first K rows, as
    float32"""
    n, d, k = RANDOM_SHAPES[i]
    x = np.random.default_rng(i + 1).standard_normal((n, d))
    if metric == COSINE:
        x = normalised(x)
    x = x.astype(np.float32)
    c = lloyd(x, x[:k], metric, max_iter=4)["centers"].astype(np.float32)
    return x, c
