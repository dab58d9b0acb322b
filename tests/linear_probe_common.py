"""Shared by tests/test_linear_probe_host.py, tests/test_gpu_linear_probe.py and tools/make_linear_probe_golden.py: the synthetic
embedding draw of the linear-probe fixtures and a numpy float64 restatement of the probe's objective.

The objective (scikit-learn ``SGDClassifier(loss="log_loss", penalty="l2", alpha, class_weight="balanced")``, one-vs-rest):

    f_k(w, b) = (1/N) sum_i c_ik log(1 + exp(-t_ik (x_i . w + b))) + alpha/2 |w|^2,    t_ik = +1 if y_i == k else -1

with cw_k = N / (C count_k); more than two classes: c_ik = cw_k for positives, 1 for negatives (``fit_binary(...,
_expanded_class_weight[i], 1.0)``); two classes: ONE problem for class 1, positives cw_1, negatives cw_0.  The intercept is not
regularised.  Nothing here touches the GPU code: the fixtures' recorded optimum is checked against THIS, and so is the kernel."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name: (seed, N train, classes, D, alpha, sep); the test split has N // 4 rows (ragged: 11)
CASES = {
    "hard9": (9001, 12000, 9, 512, 0.01, 0.08),
    "loose9": (9002, 12000, 9, 512, 0.0001, 0.08),
    "bin2": (9003, 12000, 2, 512, 0.001, 0.06),
    "ragged3": (9004, 37, 3, 64, 0.01, 0.5),
}
METRIC_KEYS = ("Accuracy", "WF1", "precision", "recall", "mcc", "tp", "fp", "tn", "fn", "sensitivity", "specificity", "ppv", "npv",
               "hitrate", "instances")        # AUC (always nan here) is left out: nan != nan


def n_test_of(name):
    n = CASES[name][1]
    return 11 if name == "ragged3" else n // 4


def draw(name):
    """(train_x, train_y, test_x, test_y): float32 unit rows, int64 labels.  Legacy RandomState streams are stable across numpy
    versions; the fixtures still carry a checksum of x (float64 sum and sum of squares) to make a different draw fail loudly."""
    seed, n, C, D, _, sep = CASES[name]
    rs = np.random.RandomState(seed)
    mu = rs.standard_normal((C, D))
    mu /= np.linalg.norm(mu, axis=1, keepdims=True)
    prior = rs.dirichlet(np.full(C, 3.0))
    out = []
    for rows in (n, n_test_of(name)):
        y = rs.choice(C, size=rows, p=prior)
        y[:C] = np.arange(C)                          # every class present in every split
        x = sep * mu[y] + rs.standard_normal((rows, D)) / np.sqrt(D)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        out += [x.astype(np.float32), y.astype(np.int64)]
    return tuple(out)


def checksum(x):
    x64 = np.asarray(x, dtype=np.float64)
    return np.array([x64.sum(), (x64 * x64).sum()])


def sample_weights(y, C, balanced=True):
    """(pos_w [K], neg_w [K]) of the K one-vs-rest problems (K = C, or 1 for two classes)."""
    y = np.asarray(y)
    cw = len(y) / (C * np.bincount(y, minlength=C).astype(np.float64)) if balanced else np.ones(C)
    if C == 2:
        return cw[1:2].copy(), cw[0:1].copy()
    return cw.copy(), np.ones(C)


def problem_classes(C):
    return np.array([1]) if C == 2 else np.arange(C)


def objective(x, y, C, alpha, W, b, balanced=True):
    """float64 (f [K], gW [K, D], gb [K], G [K]) at (W [K, D], b [K]); G_k = (1/N) sum_i c_ik |x_i| is the size of the terms the
    gradient sums, the yardstick the kernel's gradient error is divided by."""
    x = np.asarray(x, dtype=np.float64)
    W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = len(x)
    pos_w, neg_w = sample_weights(y, C, balanced)
    pos = np.asarray(y)[:, None] == problem_classes(C)[None, :]            # [N, K]
    c = np.where(pos, pos_w[None, :], neg_w[None, :])
    z = x @ W.T + b[None, :]
    tz = np.where(pos, z, -z)
    loss = np.log1p(np.exp(-np.abs(tz))) + np.maximum(-tz, 0.0)
    e = np.exp(-np.abs(z))
    sig = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    r = c * (sig - pos)
    f = (c * loss).sum(0) / n + 0.5 * alpha * (W * W).sum(1)
    gW = r.T @ x / n + alpha * W
    gb = r.sum(0) / n
    G = (c * np.linalg.norm(x, axis=1)[:, None]).sum(0) / n
    return f, gW, gb, G


def decide(x, W, b):
    """float64 decision values [N, K], predictions (class INDEX) and margins (top-1 minus top-2; |z| for one problem)."""
    z = np.asarray(x, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)[None, :]
    if z.shape[1] == 1:
        return z, (z[:, 0] > 0).astype(np.int64), np.abs(z[:, 0])
    top = np.sort(z, axis=1)
    return z, z.argmax(1), top[:, -1] - top[:, -2]


def load_case(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, f"linear_probe_{name}.npz"), allow_pickle=False))
