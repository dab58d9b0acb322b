"""Shared by tests/test_softmax_probe_host.py, tests/test_gpu_softmax_probe.py and tools/make_softmax_probe_golden.py: a numpy float64
restatement of the softmax probe's objective, the same formulas in numpy float32 (the "fp32 restatement": what fp32 arithmetic alone costs
on the same inputs), and the cases -- the draws of tests/linear_probe_common.py with a class weighting each.

    f(W, b) = (1/N) sum_i cw[y_i] (logsumexp_k(x_i.w_k + b_k) - (x_i.w_{y_i} + b_{y_i})) + alpha/2 |W|_F^2

for C >= 2 classes, always C rows; cw = ones or N / (C count_k) ("balanced"); the intercepts are not regularised; a label outside [0, C)
gives its row weight 0.  f does not change when a constant is added to every intercept: intercepts are compared centred (``centre``).
Nothing here touches the GPU code: the fixtures' recorded optimum is checked against THIS, and so is the kernel."""
import os

import numpy as np

import linear_probe_common as LP

GOLDEN_DIR = LP.GOLDEN_DIR
# case -> class_weight; draw, sizes and alpha are linear_probe_common.CASES[case].  hard9 is NOT balanced: balanced, 2.4 % of its train
# rows lie within 1e-3 of a tie at the float64 optimum
CASES = {"ragged3": "balanced", "bin2": None, "hard9": None, "loose9": "balanced"}
draw = LP.draw


def shape_of(case):
    """(N train, C, D, alpha, class_weight)"""
    _, n, C, D, alpha, _ = LP.CASES[case]
    return n, C, D, alpha, CASES[case]


def class_weights(y, C, class_weight):
    y = np.asarray(y)
    if class_weight is None:
        return np.ones(C)
    assert class_weight == "balanced"
    ok = (y >= 0) & (y < C)
    return len(y) / (C * np.bincount(y[ok], minlength=C).astype(np.float64))


def centre(b):
    b = np.asarray(b, dtype=np.float64)
    return b - b.mean()


def _objective(x, y, C, alpha, W, b, cw, dt):
    x, W, b, cw = (np.asarray(a, dtype=dt) for a in (x, W, b, cw))
    y = np.asarray(y)
    n = len(x)
    ok = (y >= 0) & (y < C)
    yc = np.where(ok, y, 0)
    w = np.where(ok, cw[yc], dt(0))                                   # [N] row weights
    z = x @ W.T + b[None, :]
    m = z.max(axis=1)
    e = np.exp(z - m[:, None])
    s = e.sum(axis=1)
    zy = z[np.arange(n), yc]
    f = (w * ((m + np.log(s)) - zy)).sum() / dt(n) + dt(0.5) * dt(alpha) * (W * W).sum()
    r = e / s[:, None]
    r[np.arange(n), yc] -= dt(1)
    r *= w[:, None]
    gW = r.T @ x / dt(n) + dt(alpha) * W
    gb = r.sum(axis=0) / dt(n)
    G = (w * np.linalg.norm(x, axis=1)).sum() / dt(n)
    return f, gW, gb, G


def objective(x, y, C, alpha, W, b, cw):
    """float64 (f, gW [C, D], gb [C], G) at (W [C, D], b [C]); G = (1/N) sum_i cw[y_i] |x_i| is the size of the terms the gradient sums,
    the yardstick the kernel's gradient error is divided by."""
    return _objective(x, y, C, alpha, W, b, cw, np.float64)


def objective_f32(x, y, C, alpha, W, b, cw):
    """the same formulas with every operand, product and sum in numpy float32"""
    return _objective(x, y, C, alpha, W, b, cw, np.float32)


def minimise(x, y, C, alpha, cw):
    """float64 minimiser (W [C, D], centred b [C]) of ``objective`` from zeros: scipy's L-BFGS-B (gtol=1e-11, ftol=0), restarted while its
    own line search stops it above that"""
    from scipy.optimize import minimize
    D = x.shape[1]
    x64 = np.asarray(x, dtype=np.float64)

    def fg(theta):
        wb = theta.reshape(C, D + 1)
        f, gW, gb, _ = objective(x64, y, C, alpha, wb[:, :D], wb[:, D], cw)
        return f, np.concatenate([gW, gb[:, None]], axis=1).ravel()

    theta = np.zeros(C * (D + 1))
    for _ in range(20):
        theta = minimize(fg, theta, jac=True, method="L-BFGS-B",
                         options=dict(gtol=1e-11, ftol=0.0, maxiter=100000, maxfun=1000000, maxcor=30, maxls=50)).x
        if np.abs(fg(theta)[1]).max() <= 1e-11:
            break
    wb = theta.reshape(C, D + 1)
    return wb[:, :D].copy(), centre(wb[:, D])


def errors(f, g, f64, gW64, gb64, G64):
    """(loss relative error, gradient error / G) of an evaluation (f, g [C, D + 1]) against the float64 one"""
    g64 = np.concatenate([gW64, gb64[:, None]], axis=1)
    return float(abs(float(f) - f64) / abs(f64)), float(np.abs(np.asarray(g, dtype=np.float64) - g64).max() / G64)


def decide(x, W, b):
    """float64 decision values [N, C] on CENTRED intercepts, predictions (class index) and margins (top-1 minus top-2)"""
    z = np.asarray(x, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T + centre(b)[None, :]
    top = np.sort(z, axis=1)
    return z, z.argmax(1), top[:, -1] - top[:, -2]


def load_case(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, f"softmax_probe_{name}.npz"), allow_pickle=False))
