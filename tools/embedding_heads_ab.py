"""Digests of what the heads on cached embeddings compute (probe.hip, probe_softmax.hip, kmeans.hip), for comparing two builds bit for bit.

    python tools/embedding_heads_ab.py              # one line per (entry, shape): a sha256 of the output bytes on seeded inputs
    python tools/embedding_heads_ab.py --time       # instead: the median of 30 event-timed calls at N = 100 000, X resident

Uses only Python entries that exist on both sides of a change to those units: kernel_entries.probe_loss_grad / softmax_loss_grad /
kmeans_update, Engine.probe_predict with decisions, plip_amd.kmeans.kmeans_assign / kmeans_seed and one short kmeans_fit.  Run it in a
checkout of each build (this file copied in) and compare the two outputs line for line: the arithmetic of these kernels is fixed by
their source, so equal inputs must give equal bytes (profiles/embedding_tile_bits.txt).

Shapes: every instantiated tile (D = 4, 64, 128, 256, 384, 512, 768, 1024), N = 33 (one row in the second tile) and 1000 (many tiles
per workgroup), 1 / 3 / 16 / 17 / 64 problems for the probes (17 and 64 take the two-pass softmax; the softmax needs two classes, so
its smallest is 2), K = 1 / 16 / 17 / 300 clusters (K <= N) in both metrics.  --time covers what --only names (default: the two-pass
softmax evaluation at C = 17, the kernels that profiles/embedding_tile_isa_diff.txt lists as not identical).
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS = (4, 64, 128, 256, 384, 512, 768, 1024)
ROWS = (33, 1000)
PROBLEMS = (1, 3, 16, 17, 64)
CLUSTERS = (1, 16, 17, 300)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()[:32]


def inputs(n, d, k, seed):
    """x fp32 [n, d], labels int32 [n] in [0, k] (k itself matches no problem), wb fp32 [k, d + 1], weights fp32 [k]: seeded, on the device"""
    import torch
    rng = np.random.default_rng([seed, n, d, k])
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = rng.integers(0, k + 1, n).astype(np.int32)
    wb = (0.3 * rng.standard_normal((k, d + 1))).astype(np.float32)
    w = (0.5 + rng.random((2, k))).astype(np.float32)
    return tuple(torch.from_numpy(a).cuda() for a in (x, y, wb, w[0], w[1]))


def bits(out):
    import torch
    from plip_amd.engine import heads_engine
    from plip_amd.kernel_entries import kmeans_update, probe_loss_grad, softmax_loss_grad
    from plip_amd.kmeans import kmeans_assign, kmeans_fit, kmeans_seed
    eng = heads_engine()
    for d in WIDTHS:
        for n in ROWS:
            for k in PROBLEMS:
                x, y, wb, pw, nw = inputs(n, d, k, 1)
                loss, grad = probe_loss_grad(eng, x, y, wb, pw, nw, 1e-3)
                out(f"probe_loss_grad   N={n} D={d} K={k}: {digest(loss, grad)}")
                pred, dec = eng.probe_predict(x, wb[:, :d], wb[:, d], return_decision=True)
                out(f"probe_predict     N={n} D={d} K={k}: {digest(pred, dec)}")
                c = max(k, 2)
                x, y, wb, cw, _ = inputs(n, d, c, 2)
                loss, grad = softmax_loss_grad(eng, x, y, wb, cw, 1e-3)
                out(f"softmax_loss_grad N={n} D={d} C={c}: {digest(loss, grad)}")
            for k in CLUSTERS:
                if k > n:
                    continue
                for mi, metric in enumerate(("euclidean", "cosine")):
                    x, _, wb, _, _ = inputs(n, d, k, 3)
                    cen = wb[:, :d].contiguous()
                    labels, scores = kmeans_assign(eng, x, cen, metric)
                    out(f"kmeans_assign     N={n} D={d} K={k} {metric}: {digest(labels, scores)}")
                    sums = torch.empty((k, d), dtype=torch.float32, device=x.device)
                    counts = torch.empty((k,), dtype=torch.int32, device=x.device)
                    reps = torch.empty((k,), dtype=torch.int32, device=x.device)
                    inertia = torch.empty((1,), dtype=torch.float64, device=x.device)
                    kmeans_update(eng, x, labels, scores, sums, counts, reps, inertia, mi)
                    out(f"kmeans_update     N={n} D={d} K={k} {metric}: {digest(sums, counts, reps, inertia)}")
                    u = np.random.default_rng([4, n, d, k]).random(k)
                    c0, picks = kmeans_seed(eng, x, k, metric, uniforms=u)
                    out(f"kmeans_seed       N={n} D={d} K={k} {metric}: {digest(c0, picks)}")
    for d, k, metric in ((64, 5, "cosine"), (512, 17, "euclidean")):
        x, _, _, _, _ = inputs(1000, d, k, 5)
        r = kmeans_fit(eng, x, k, metric, init=x[:k].clone(), max_iter=4, tol=0.0)
        out(f"kmeans_fit        N=1000 D={d} K={k} {metric} 4 iterations: {digest(r.centers, r.labels, r.scores, r.counts, r.representatives)} "
            f"inertia {r.inertia!r}")


def timing(out, only, n=100_000, calls=30):
    import torch
    from plip_amd.engine import heads_engine
    from plip_amd.kernel_entries import probe_loss_grad, softmax_loss_grad
    from plip_amd.kmeans import kmeans_assign
    eng = heads_engine()
    for d in WIDTHS:
        x, y, wb, cw, nw = inputs(n, d, 17, 6)
        runs = {"softmax_loss_grad C=17": lambda: softmax_loss_grad(eng, x, y, wb, cw, 1e-3),
                "softmax_loss_grad C=16": lambda: softmax_loss_grad(eng, x, y, wb[:16].contiguous(), cw[:16].contiguous(), 1e-3),
                "probe_loss_grad K=16": lambda: probe_loss_grad(eng, x, y, wb[:16].contiguous(), cw[:16].contiguous(), nw[:16].contiguous(), 1e-3),
                "probe_predict K=17": lambda: eng.probe_predict(x, wb[:, :d], wb[:, d], return_decision=True),
                "kmeans_assign K=17": lambda: kmeans_assign(eng, x, wb[:, :d].contiguous(), "cosine")}
        for name, fn in runs.items():
            if only not in name:
                continue
            fn()
            torch.cuda.synchronize()
            us = []
            for _ in range(calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                us.append(a.elapsed_time(b) * 1e3)
            out(f"time {name} N={n} D={d}: median {float(np.median(us)):.1f} us  min {min(us):.1f} us  ({calls} calls)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--time", action="store_true", help="time instead of digesting")
    ap.add_argument("--only", default="softmax_loss_grad C=17", help="--time: the rows whose name contains this (\"\" = all)")
    a = ap.parse_args()
    out = lambda s: print(s, flush=True)
    timing(out, a.only) if a.time else bits(out)


if __name__ == "__main__":
    main()
