"""Time the softmax probe beside the one-vs-rest pass at the size of a Kather-like training split: N = 100 000 cached embeddings, D = 512,
nine classes (and C = 17, 64 for the two-pass path), in ONE run.

    python tools/softmax_probe_bench.py            # -> stdout; profiles/softmax_probe_timing.txt keeps a run's lines
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/softmax_probe_bench.py --classes 9 --no-fits     # kernel times

One evaluation = the test entry (loss-and-gradient kernels, the finish kernel, two device copies of the results) between two HIP events on
the stream, min / median of ``--evals`` calls after a warm-up; X stays resident on the device.  A whole fit is wall time around the call.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from linear_probe_bench import draw_bench  # noqa: E402


def _time(fn, evals):
    import torch
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(evals):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return min(us), float(np.median(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--evals", type=int, default=30)
    ap.add_argument("--classes", default="9,17,64", help="class counts to time")
    ap.add_argument("--no-fits", action="store_true", help="evaluations only (for a rocprofv3 --kernel-trace --stats run)")
    a = ap.parse_args()
    import torch
    from plip_amd.engine import heads_engine
    from plip_amd.kernel_entries import probe_loss_grad, softmax_loss_grad
    from plip_amd.softmax_probe import softmax_fit
    eng = heads_engine()
    D = 512
    mb = a.n * D * 4 / 1e6
    print(f"# one MI355X, N = {a.n}, D = {D}, X resident on the device ({mb:.1f} MB); min / median of {a.evals} evaluations")
    for C in (int(c) for c in a.classes.split(",")):
        x, y = draw_bench(a.n, C, D)
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda()
        wb = torch.zeros((C, D + 1), device="cuda")
        w = torch.ones((C,), device="cuda")
        passes = 1 if C <= 16 else 1 + (C + 15) // 16
        lo, med = _time(lambda: softmax_loss_grad(eng, xd, yd, wb, None, 0.01), a.evals)
        print(f"softmax evaluation C={C}: {lo:.1f} / {med:.1f} us, X read {passes} time(s) = {passes * mb:.1f} MB -> {passes * mb / lo:.2f} TB/s")
        passes = (C + 15) // 16
        lo, med = _time(lambda: probe_loss_grad(eng, xd, yd, wb, w, w, 0.01), a.evals)
        print(f"one-vs-rest evaluation K={C}: {lo:.1f} / {med:.1f} us, X read {passes} time(s) = {passes * mb:.1f} MB -> {passes * mb / lo:.2f} TB/s")
        if C != 9 or a.no_fits:
            continue
        softmax_fit(eng, xd, y, C, alpha=0.1)                   # warm-up: scratch, kernel attributes
        eng.probe_fit(xd, y, C, 0.1)
        for alpha in (1.0 / (0.316 * a.n), 0.001, 0.01):
            for name, fit in (("softmax_fit", lambda: softmax_fit(eng, xd, y, C, alpha=alpha, class_weight="balanced")),
                              ("probe_fit (one-vs-rest)", lambda: eng.probe_fit(xd, y, C, alpha))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, _, info = fit()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print(f"{name} N={a.n} D={D} classes={C} alpha={alpha:.3g} balanced: {dt * 1e3:.1f} ms, {info['iterations']} iterations, "
                      f"{info['evaluations']} evaluations ({dt * 1e6 / info['evaluations']:.0f} us each), |grad|_inf {info['grad_norm']:.1e}, "
                      f"converged {info['converged']}", flush=True)


if __name__ == "__main__":
    main()
