"""Generate tests/golden/softmax_probe_*.npz: the recorded float64 optimum of the softmax probe -- TEST INFRASTRUCTURE.

    python tools/make_softmax_probe_golden.py                 # needs scipy and scikit-learn (its metric functions); CPU, no GPU

Per case of tests/softmax_probe_common.py CASES (the data is redrawn from the seed by the tests, only its checksum is stored):

* ``Wstar, bstar, fstar``: the float64 minimiser of the objective restated in softmax_probe_common.objective -- scipy's L-BFGS-B from
  zeros (``gtol=1e-11``, ``ftol=0``), ``bstar`` centred; ``opt_grad_inf`` = |grad f|_inf there (asserted <= 1e-9); ``G`` (the gradient's
  term size);
* ``opt_macro_*``: sklearn's own metric functions on the optimum's predictions on both splits (linear_probe_common.METRIC_KEYS order);
* ``under_margin_*``: how many rows of a split lie within 1e-3 of a tie at the optimum (the tests leave those rows out, at most 2 %).

Predictions and margins of the optimum are not stored: the tests recompute them from ``Wstar`` in float64.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import linear_probe_common as LP  # noqa: E402
import softmax_probe_common as SP  # noqa: E402
from make_linear_probe_golden import sk_metrics  # noqa: E402


def optimum(x, y, C, alpha, cw):
    W, b = SP.minimise(x, y, C, alpha, cw)
    f, gW, gb, G = SP.objective(x, y, C, alpha, W, b, cw)
    gn = max(np.abs(gW).max(), np.abs(gb).max())
    assert gn <= 1e-9, gn
    return W, b, f, G, gn


def make_case(name):
    n, C, D, alpha, class_weight = SP.shape_of(name)
    xtr, ytr, xte, yte = SP.draw(name)
    cw = SP.class_weights(ytr, C, class_weight)
    W, b, f, G, gn = optimum(xtr, ytr, C, alpha, cw)
    out = {"seed": LP.CASES[name][0], "n_train": n, "n_test": len(yte), "classes": C, "dim": D, "alpha": alpha,
           "balanced": int(class_weight == "balanced"), "x_train_checksum": LP.checksum(xtr), "x_test_checksum": LP.checksum(xte),
           "Wstar": W, "bstar": b, "fstar": f, "G": G, "opt_grad_inf": gn, "metric_keys": np.array(LP.METRIC_KEYS)}
    for split, x, y in (("train", xtr, ytr), ("test", xte, yte)):
        _, pred, margin = SP.decide(x, W, b)
        out[f"opt_macro_{split}"] = sk_metrics(y, pred, "macro")
        out[f"under_margin_{split}"] = int((margin < 1e-3).sum())
    path = os.path.join(SP.GOLDEN_DIR, f"softmax_probe_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: f* {f:.12f} |grad|_inf {gn:.1e} sum(b) {b.sum():.1e} |colsum W|_inf {np.abs(W.sum(0)).max():.1e}  acc train/test "
          f"{out['opt_macro_train'][0]:.4f}/{out['opt_macro_test'][0]:.4f}  under 1e-3: {out['under_margin_train']}/{n} train, "
          f"{out['under_margin_test']}/{len(yte)} test  {os.path.getsize(path) / 1024:.0f} KiB", flush=True)


if __name__ == "__main__":
    for c in (sys.argv[1:] or list(SP.CASES)):
        make_case(c)
