"""Time k-means on the GPU at the size of a corpus of cached embeddings: N = 100 000 unit rows, D = 512, K = 16 / 256 / 1024, cosine.

    python tools/kmeans_bench.py                   # -> profiles/kmeans_timing.txt and profiles/kmeans_parity.txt (and stdout)
    python tools/kmeans_bench.py --timing-only / --parity-only
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/kmeans_bench.py --passes-only      # kernel times

* One pass = the entry (plipmi_kmeans_assign: the bias kernel and the assignment kernel; plipmi_kmeans_update: the counting sort, the chunk
  sums and the combine kernel) between two HIP events on the stream, min / median of ``--evals`` calls after a warm-up; X stays resident.
* Yardstick 1: X read once at 2.75 TB/s (what the probe passes reach on the same bytes, profiles/linear_probe_timing.txt).
* Yardstick 2: ``plipmi_similarity_topk(k = 1)`` on the same X and centres -- what a caller could do before this entry existed (it finds
  the arg-max of x.c only: no bias, no sums).
* A whole fit is wall time around ``kmeans_fit`` from given centres, beside scikit-learn's ``KMeans`` from the same centres on the host
  (Euclidean, where the two are the same algorithm).
* The parity file keeps the figure lines tests/test_gpu_kmeans.py prints before it asserts.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

X_RATE = 2.75e12      # bytes / s: the probe passes' rate on X (profiles/linear_probe_timing.txt: 2.7 - 2.8 TB/s)


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


def draw(n, d, k, seed=0):
    """n unit rows around k directions (float32), and k starting centres = rows of it"""
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((k, d))
    x = dirs[rng.integers(0, k, n)] + 2.0 * rng.standard_normal((n, d))
    x /= np.sqrt((x * x).sum(axis=1, keepdims=True))
    return x.astype(np.float32), x[rng.choice(n, k, replace=False)].astype(np.float32)


def timing(a, out):
    import torch
    from plip_amd.engine import heads_engine
    from plip_amd.kernel_entries import kmeans_update
    from plip_amd.kmeans import kmeans_assign, kmeans_fit
    eng = heads_engine()
    D = 512
    mb = a.n * D * 4 / 1e6
    floor_us = a.n * D * 4 / X_RATE * 1e6
    out(f"# one MI355X, N = {a.n}, D = {D}, cosine, X resident on the device ({mb:.1f} MB); min / median of {a.evals} calls, device events")
    out(f"# yardstick 1: X read once at {X_RATE / 1e12:.2f} TB/s = {floor_us:.1f} us")
    for K in (int(k) for k in a.clusters.split(",")):
        x, c0 = draw(a.n, D, K)
        xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(c0).cuda()
        labels, scores = kmeans_assign(eng, xd, cd, "cosine")
        t_as = _time(lambda: kmeans_assign(eng, xd, cd, "cosine"), a.evals)
        sums = torch.empty((K, D), device="cuda")
        counts, reps = torch.empty((K,), dtype=torch.int32, device="cuda"), torch.empty((K,), dtype=torch.int32, device="cuda")
        inertia = torch.empty((1,), dtype=torch.float64, device="cuda")
        t_up = _time(lambda: kmeans_update(eng, xd, labels, scores, sums, counts, reps, inertia, 1), a.evals)
        t_tk = _time(lambda: eng.similarity_topk(xd, cd, 1), a.evals)
        idx = eng.similarity_topk(xd, cd, 1).reshape(-1).to(torch.int32)
        agree = float((idx == labels).float().mean())
        flops = 2.0 * a.n * D * K
        out(f"K = {K:5d}  assignment pass {t_as[0]:9.1f} / {t_as[1]:9.1f} us  = {t_as[0] / floor_us:6.2f} x the X-read floor, "
            f"{flops / t_as[0] / 1e6:6.1f} TFLOP/s fp32   update pass {t_up[0]:9.1f} / {t_up[1]:9.1f} us")
        out(f"           similarity_topk(k = 1) on the same inputs {t_tk[0]:9.1f} / {t_tk[1]:9.1f} us  -> the fused pass takes "
            f"{t_as[0] / t_tk[0]:5.2f} x its time (labels agree on {100 * agree:.3f} % of the rows)")
        if a.passes_only:
            continue
        t0 = time.perf_counter()
        res = kmeans_fit(eng, xd, K, metric="euclidean", init=cd, max_iter=a.max_iter, tol=0.0)
        torch.cuda.synchronize()
        t_fit = time.perf_counter() - t0
        out(f"           whole fit (euclidean, from the same centres, tol = 0, max_iter = {a.max_iter}): {t_fit * 1e3:9.1f} ms wall, "
            f"{res.n_iter} iterations, converged {res.converged}, inertia {res.inertia:.3f}")
        if a.sklearn and K <= a.sklearn_max_k:
            from sklearn.cluster import KMeans
            t0 = time.perf_counter()
            sk = KMeans(n_clusters=K, init=c0, n_init=1, algorithm="lloyd", tol=0, max_iter=a.max_iter).fit(x)
            t_sk = time.perf_counter() - t0
            same = float((sk.labels_ == res.labels.cpu().numpy()).mean())
            out(f"           scikit-learn KMeans on the host ({os.cpu_count()} logical CPUs visible), same centres: {t_sk * 1e3:9.1f} ms wall, "
                f"{sk.n_iter_} iterations, inertia {sk.inertia_:.3f}  -> {t_sk / t_fit:6.1f} x the GPU fit; labels agree on {100 * same:.3f} % of the rows")


def parity(out):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_kmeans.py"), "-m", "gpu", "-q", "-s",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, cwd=ROOT)
    out("# the figures tests/test_gpu_kmeans.py prints before it asserts (one MI355X); bounds: tests/small_kernel_refs.py fp32_bound")
    for line in r.stdout.splitlines():
        line = line.lstrip(".")
        if line.startswith(("ASSIGN", "UPDATE", "SEED", "FIT")):
            out(line)
    out("# " + (r.stdout.strip().splitlines() or ["no output"])[-1])
    return r.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--clusters", default="16,256,1024")
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--passes-only", action="store_true", help="the passes only (for a rocprofv3 --kernel-trace --stats run)")
    ap.add_argument("--no-sklearn", dest="sklearn", action="store_false")
    ap.add_argument("--sklearn-max-k", type=int, default=256, help="scikit-learn is timed up to this K (it is slow beyond)")
    ap.add_argument("--timing-only", action="store_true")
    ap.add_argument("--parity-only", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    rc = 0
    for name, on, fn in (("kmeans_timing.txt", not a.parity_only, lambda o: timing(a, o)), ("kmeans_parity.txt", not a.timing_only and not a.passes_only, parity)):
        if not on:
            continue
        lines = []

        def out(s):
            print(s, flush=True)
            lines.append(s)
        rc = fn(out) or rc
        if not a.passes_only:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, name), "w") as f:
                f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
