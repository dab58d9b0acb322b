"""Generate tests/golden/linear_probe_*.npz: recorded results for the linear-probe head -- TEST INFRASTRUCTURE.

    python tools/make_linear_probe_golden.py                 # needs scikit-learn; CPU, no GPU
    python tools/make_linear_probe_golden.py --sgd-timing    # SGDClassifier wall time at N = 100 000 -> profiles/linear_probe_sgd_cpu.txt

Per case of tests/linear_probe_common.py CASES (the data is redrawn from the seed by the tests, only its checksum is stored):

* ``Wstar, bstar, fstar``: the float64 minimiser of the probe's objective -- ``LogisticRegression(C=1/(alpha N), lbfgs, tol=1e-10)``
  per one-vs-rest problem with the class weights as sample weights, polished with float64 Newton steps until the gradient
  (recomputed by linear_probe_common.objective) is below 1e-9 in the infinity norm -- and ``G`` (the gradient's term size);
* ``opt_pred_*, opt_margin_*`` on both splits (class index; top-1 minus top-2 decision value, float32);
* ``opt_macro_*`` / ``opt_weighted_sklearn_*``: sklearn's own metric functions on those predictions (METRIC_KEYS order);
  ``opt_weighted_pkg_*``: ``plip_amd.reproducibility.metrics.eval_metrics`` (weighted) as the package computed it when the fixture was
  made, the value a later change must not move;
* ``sgd_*``: the reference path, ``SGDClassifier`` exactly as reproducibility/evaluation/linear_probing/linear_classifier.py builds
  it (seed 7): coef, intercept, n_iter, predictions, objective at its solution, macro metrics.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import linear_probe_common as LP  # noqa: E402


def sk_metrics(y_true, y_pred, average):
    """reproducibility/metrics.py eval_metrics with sklearn's functions, METRIC_KEYS order."""
    from sklearn.metrics import accuracy_score, f1_score, matthews_corrcoef, precision_score, recall_score
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    tp = int(((y_true == y_pred) & (y_pred == 1)).sum()); fp = int(((y_pred == 1) & (y_true != y_pred)).sum())
    tn = int(((y_true == y_pred) & (y_pred == 0)).sum()); fn = int(((y_pred == 0) & (y_true != y_pred)).sum())
    nan = float("nan")
    d = {"Accuracy": accuracy_score(y_true, y_pred), "WF1": f1_score(y_true, y_pred, average=average, zero_division=0),
         "precision": precision_score(y_true, y_pred, average=average, zero_division=0),
         "recall": recall_score(y_true, y_pred, average=average, zero_division=0), "mcc": matthews_corrcoef(y_true, y_pred),
         "tp": tp, "fp": fp, "tn": tn, "fn": fn, "sensitivity": tp / (tp + fn) if tp + fn else nan,
         "specificity": tn / (tn + fp) if tn + fp else nan, "ppv": tp / (tp + fp) if tp + fp else nan,
         "npv": tn / (tn + fn) if tn + fn else nan, "hitrate": (tp + tn) / (tp + tn + fp + fn) if tp + tn + fp + fn else nan,
         "instances": len(y_true)}
    return np.array([float(d[k]) for k in LP.METRIC_KEYS])


def pkg_metrics(y_true, y_pred, **kw):
    from plip_amd.reproducibility.metrics import eval_metrics
    d = eval_metrics(list(y_true), list(y_pred), **kw)
    return np.array([float(d[k]) for k in LP.METRIC_KEYS])


def optimum(x, y, C, alpha):
    from sklearn.linear_model import LogisticRegression
    x64 = x.astype(np.float64)
    n, D = x64.shape
    pos_w, neg_w = LP.sample_weights(y, C)
    ks = LP.problem_classes(C)
    W, b = np.zeros((len(ks), D)), np.zeros(len(ks))
    for j, k in enumerate(ks):
        t = (y == k).astype(int)
        if t.all() or not t.any():
            raise ValueError("a one-vs-rest problem needs both signs")
        lr = LogisticRegression(C=1.0 / (alpha * n), tol=1e-10, max_iter=20000, solver="lbfgs")
        lr.fit(x64, t, sample_weight=np.where(t == 1, pos_w[j], neg_w[j]))
        W[j], b[j] = lr.coef_[0], lr.intercept_[0]
    xa = np.concatenate([x64, np.ones((n, 1))], axis=1)
    for it in range(30):                                # Newton polish, float64
        f, gW, gb, _ = LP.objective(x, y, C, alpha, W, b)
        gn = max(np.abs(gW).max(), np.abs(gb).max())
        if gn < 1e-12:
            break
        z = x64 @ W.T + b
        s = 1.0 / (1.0 + np.exp(-z))
        pos = y[:, None] == ks[None, :]
        c = np.where(pos, pos_w[None, :], neg_w[None, :])
        for j in range(len(ks)):
            h = c[:, j] * s[:, j] * (1 - s[:, j]) / n
            H = (xa * h[:, None]).T @ xa
            H[np.arange(D), np.arange(D)] += alpha
            step = np.linalg.solve(H, np.concatenate([gW[j], gb[j:j + 1]]))
            W[j] -= step[:D]
            b[j] -= step[D]
    f, gW, gb, G = LP.objective(x, y, C, alpha, W, b)
    gn = max(np.abs(gW).max(), np.abs(gb).max())
    assert gn < 1e-9, gn
    return W, b, f, G, gn


def sgd(x, y, alpha):
    from sklearn.linear_model import SGDClassifier
    clf = SGDClassifier(random_state=7, loss="log_loss", alpha=alpha, verbose=0, penalty="l2", max_iter=10000,
                        class_weight="balanced")
    t0 = time.perf_counter()
    clf.fit(x, y)
    return clf, time.perf_counter() - t0


def make_case(name):
    seed, n, C, D, alpha, sep = LP.CASES[name]
    xtr, ytr, xte, yte = LP.draw(name)
    W, b, f, G, gn = optimum(xtr, ytr, C, alpha)
    out = {"seed": seed, "n_train": n, "n_test": len(yte), "classes": C, "dim": D, "alpha": alpha, "sep": sep,
           "x_train_checksum": LP.checksum(xtr), "x_test_checksum": LP.checksum(xte),
           "y_train": ytr.astype(np.int16), "y_test": yte.astype(np.int16),
           "Wstar": W, "bstar": b, "fstar": f, "G": G, "opt_grad_inf": gn, "metric_keys": np.array(LP.METRIC_KEYS)}
    clf, secs = sgd(xtr, ytr, alpha)
    sW, sb = clf.coef_.astype(np.float64), clf.intercept_.astype(np.float64)
    out.update({"sgd_coef": sW, "sgd_intercept": sb, "sgd_n_iter": clf.n_iter_, "sgd_fit_seconds_cpu": secs,
                "sgd_f": LP.objective(xtr, ytr, C, alpha, sW, sb)[0]})
    for split, x, y in (("train", xtr, ytr), ("test", xte, yte)):
        _, pred, margin = LP.decide(x, W, b)
        out[f"opt_pred_{split}"] = pred.astype(np.int16)
        out[f"opt_margin_{split}"] = margin.astype(np.float32)
        out[f"opt_macro_{split}"] = sk_metrics(y, pred, "macro")
        out[f"opt_weighted_sklearn_{split}"] = sk_metrics(y, pred, "weighted")
        out[f"opt_weighted_pkg_{split}"] = pkg_metrics(y, pred)
        sp = clf.predict(x)
        out[f"sgd_pred_{split}"] = sp.astype(np.int16)
        out[f"sgd_macro_{split}"] = sk_metrics(y, sp, "macro")
    path = os.path.join(LP.GOLDEN_DIR, f"linear_probe_{name}.npz")
    np.savez_compressed(path, **out)
    gap = (out["sgd_f"] - f) / f
    print(f"{name}: |grad|_inf {gn:.1e}  acc train/test {out['opt_macro_train'][0]:.3f}/{out['opt_macro_test'][0]:.3f}  "
          f"SGD acc test {out['sgd_macro_test'][0]:.3f} n_iter {clf.n_iter_} gap {gap.min():.1e}..{gap.max():.1e} "
          f"agree {np.mean(out['sgd_pred_test'] == out['opt_pred_test']):.3f}  left out at 1e-3/1e-4: "
          f"{np.mean(out['opt_margin_train'] < 1e-3):.4f}/{np.mean(out['opt_margin_train'] < 1e-4):.4f}  "
          f"{os.path.getsize(path) / 1024:.0f} KiB", flush=True)


def sgd_timing():
    """SGDClassifier on the 100 000-row draw the GPU timing uses (tools/linear_probe_bench.py), four alphas of reproduce.sh."""
    from linear_probe_bench import draw_bench  # tools/linear_probe_bench.py
    lines = ["# SGDClassifier(loss=log_loss, penalty=l2, class_weight=balanced, max_iter=10000, random_state=7), one CPU core of the",
             "# fixture host -- NOT the GPU host; N = 100000, D = 512", "# classes alpha seconds n_iter"]
    for C in (9, 2):
        x, y = draw_bench(100000, C, 512)
        for alpha in (0.0001, 0.001, 0.01, 0.1):
            clf, secs = sgd(x, y, alpha)
            lines.append(f"{C} {alpha} {secs:.2f} {clf.n_iter_}")
            print(lines[-1], flush=True)
    with open(os.path.join(ROOT, "profiles", "linear_probe_sgd_cpu.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sgd-timing", action="store_true")
    ap.add_argument("cases", nargs="*", default=list(LP.CASES))
    a = ap.parse_args()
    if a.sgd_timing:
        sgd_timing()
    else:
        for c in a.cases:
            make_case(c)
