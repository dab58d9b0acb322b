"""Time the linear-probe head at the size of a Kather-like training split: N = 100 000 cached embeddings, D = 512.

    python tools/linear_probe_bench.py                 # probe_fit wall time for the four alphas of reproduce.sh, K = 9 and K = 2
    python tools/linear_probe_bench.py --evals 20      # only loss-and-gradient evaluations (run it under rocprofv3 --kernel-trace --stats)

X stays resident on the device.  tools/make_linear_probe_golden.py --sgd-timing measures scikit-learn's SGDClassifier on the same draw.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def draw_bench(n, C, D, seed=77, sep=0.08):
    rs = np.random.RandomState(seed + C)
    mu = rs.standard_normal((C, D))
    mu /= np.linalg.norm(mu, axis=1, keepdims=True)
    y = rs.choice(C, size=n, p=rs.dirichlet(np.full(C, 3.0)))
    x = sep * mu[y] + rs.standard_normal((n, D)) / np.sqrt(D)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), y.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--evals", type=int, default=0)
    a = ap.parse_args()
    import torch
    from plip_amd.engine import heads_engine
    eng = heads_engine()
    for C in (9, 2):
        x, y = draw_bench(a.n, C, 512)
        xd = torch.from_numpy(x).cuda()
        if a.evals:
            from plip_amd.kernel_entries import probe_loss_grad
            K = 1 if C == 2 else C
            wb = torch.zeros((K, 513), device="cuda")
            w = torch.ones((K,), device="cuda")
            yd = torch.from_numpy(y.astype(np.int32)).cuda()
            for _ in range(a.evals):
                probe_loss_grad(eng, xd, yd, wb, w, w, 0.01)
            torch.cuda.synchronize()
            continue
        eng.probe_fit(xd, y, C, 0.1)                      # warm-up: scratch, kernel attributes
        for alpha in (0.0001, 0.001, 0.01, 0.1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            coef, b, info = eng.probe_fit(xd, y, C, alpha)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"probe_fit N={a.n} D=512 classes={C} alpha={alpha}: {dt * 1e3:.1f} ms, {info['iterations']} iterations, "
                  f"{info['evaluations']} evaluations ({dt * 1e6 / info['evaluations']:.0f} us each), |grad|_inf {info['grad_norm']:.1e}, "
                  f"converged {info['converged']}", flush=True)


if __name__ == "__main__":
    main()
