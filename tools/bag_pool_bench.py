"""Time slide-level top-K pooling on the GPU at the size of a cohort of cached embeddings: N = 100 000 unit rows, D = 512,
ks = (1, 5, 10, 50, 100), four workloads.

    python tools/bag_pool_bench.py                 # -> profiles/bag_pool_timing.txt and profiles/bag_pool_parity.txt (and stdout)
    python tools/bag_pool_bench.py --timing-only / --parity-only
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bag_pool_bench.py --passes-only      # kernel times

* Workloads: (i) S = 64 bags of 500 .. 5 000 rows from a seeded generator, C = 9; (ii) the same, C = 64; (iii) S = 1, C = 2;
  (iv) S = 1 000 bags of 100 rows, C = 9.
* New: ``bag_topk_pool`` (plipmi_bag_topk_pool: offsets, score pass, pieces, merges, predictions) between two HIP events on the stream,
  min / median of ``--evals`` calls after a warm-up; X, T and the offsets stay resident, the workspace is allocated once.
* Baseline: the route the library offered before, timed the same way in the same process: ``Engine.logits`` with the transposed output,
  then PER BAG ``Engine.topk(k = 100)`` on the [C, n_b] slice, a gather, a torch mean per k and an arg-max.
* Reported beside them: the score pass alone (``return_scores`` costs nothing extra: the scores are written either way) against
  ``kmeans_assign`` at K = 16 on the same X -- the same walk over the same bytes plus N C 4 bytes written -- and the pooling kernels alone
  (``bag_pool_scores`` on resident scores) against the bytes they move.
* The parity file keeps the figure lines tests/test_gpu_bags.py prints before it asserts.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KS = (1, 5, 10, 50, 100)
HBM_RATE = 2.75e12    # bytes / s: what the probe passes reach on X (profiles/linear_probe_timing.txt)


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


def workloads(n):
    rng = np.random.default_rng(0)
    lo, hi = n // 200, n // 20                           # 500 .. 5 000 rows at N = 100 000: a few large slides, many small ones
    extra = rng.random(64) ** 3.2
    for _ in range(16):                                  # scaled to the row count, capped at the largest bag
        extra = np.minimum(extra * ((n - 64 * lo) / extra.sum()), hi - lo)
    sizes = lo + np.floor(extra).astype(np.int64)
    sizes[np.argsort(sizes)[:n - sizes.sum()]] += 1      # the rounding's remainder goes to the smallest bags
    assert sizes.sum() == n and sizes.min() >= lo and sizes.max() <= hi
    return [("(i)   S = 64 bags of 500 .. 5 000 rows, C = 9", sizes, 9), ("(ii)  S = 64 bags of 500 .. 5 000 rows, C = 64", sizes, 64),
            ("(iii) S = 1, C = 2", np.array([n]), 2), ("(iv)  S = 1 000 bags of 100 rows, C = 9", np.full(n // 100, 100), 9)]


def timing(a, out):
    import torch
    from plip_amd import _lib
    from plip_amd._lib import _ptr
    from plip_amd.bags import bag_pool_scores, bag_topk_pool
    from plip_amd.engine import heads_engine
    from plip_amd.kmeans import kmeans_assign
    eng = heads_engine()
    D, n = 512, a.n
    rng = np.random.default_rng(1)
    x = rng.standard_normal((n, D)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    xd = torch.from_numpy(x).cuda()
    out(f"# one MI355X, N = {n}, D = {D}, unit rows, ks = {KS}, X resident on the device ({n * D * 4 / 1e6:.1f} MB); min / median of "
        f"{a.evals} calls, device events")
    c16 = torch.from_numpy(x[:16].copy()).cuda()
    t_km = _time(lambda: kmeans_assign(eng, xd, c16, "cosine"), a.evals)
    out(f"# kmeans_assign at K = 16 on the same X: {t_km[0]:9.1f} / {t_km[1]:9.1f} us   (X read once at {HBM_RATE / 1e12:.2f} TB/s: "
        f"{n * D * 4 / HBM_RATE * 1e6:.1f} us)")
    ks = np.asarray(KS, dtype=np.int32)
    ksp = ks.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    for name, sizes, C in workloads(n):
        S = len(sizes)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        t = rng.standard_normal((C, D)).astype(np.float32)
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        td, od = torch.from_numpy(t).cuda(), torch.from_numpy(off).cuda()
        ws = torch.empty((int(eng.lib.plipmi_bag_workspace(n, S, C, int(ks[-1]))),), dtype=torch.uint8, device="cuda")
        pooled = torch.empty((S, len(ks), C), device="cuda")
        pred = torch.empty((S, len(ks)), dtype=torch.int32, device="cuda")
        scores = torch.empty((C, n), device="cuda")

        def new():
            _lib.check(eng.lib.plipmi_bag_topk_pool(eng._h, _ptr(xd), n, D, _ptr(od), S, _ptr(td), C, 100.0, ksp, len(ks), _ptr(ws), _ptr(pooled),
                                                    _ptr(pred), None, _ptr(scores), eng._stream()), "plipmi_bag_topk_pool")

        def pool_only():
            _lib.check(eng.lib.plipmi_bag_pool_scores(eng._h, _ptr(scores), n, n, C, _ptr(od), S, ksp, len(ks), _ptr(ws), _ptr(pooled), _ptr(pred),
                                                      None, eng._stream()), "plipmi_bag_pool_scores")

        def baseline():
            _, lpt, _ = eng.logits(xd, td, scale=100.0, want_text=True)
            res = []
            for b in range(S):
                seg = lpt[:, int(off[b]):int(off[b + 1])]
                idx = eng.topk(seg, min(100, seg.shape[1]))
                vals = torch.gather(seg, 1, idx)
                p = torch.stack([vals[:, :k].mean(dim=1) for k in KS])
                res.append((p, p.argmax(dim=1)))
            return res

        t_new, t_pool = _time(new, a.evals), _time(pool_only, a.evals)
        out(f"{name}")
        out(f"    plipmi_bag_topk_pool            {t_new[0]:10.1f} / {t_new[1]:10.1f} us")
        moved = n * C * 4 + S * C * len(ks) * 4
        out(f"    plipmi_bag_pool_scores alone    {t_pool[0]:10.1f} / {t_pool[1]:10.1f} us   ({moved / 1e6:.1f} MB of scores read and results written: "
            f"{moved / HBM_RATE * 1e6:.1f} us at {HBM_RATE / 1e12:.2f} TB/s)")
        t_sc = t_new[0] - t_pool[0]
        out(f"    score pass (the difference)     {t_sc:10.1f} us   = {t_sc / t_km[0]:5.2f} x kmeans_assign at K = 16 ({n * C * 4 / 1e6:.1f} MB of scores written)")
        if a.passes_only:
            continue
        # the two routes agree on the predictions (the baseline's own rounding aside: only bags decided by more than 1e-3 are compared)
        ref = baseline()
        torch.cuda.synchronize()
        new()
        torch.cuda.synchronize()
        bp = torch.stack([r[0] for r in ref]).cpu().numpy()                    # [S, nks, C]
        gap = np.sort(bp, axis=2)
        clear = (gap[:, :, -1] - gap[:, :, -2]) > 1e-3 if C > 1 else np.ones(bp.shape[:2], bool)
        same = (np.stack([r[1].cpu().numpy() for r in ref]) == pred.cpu().numpy())[clear].mean()
        worst = np.abs(bp - pooled.cpu().numpy()).max()
        t_base = _time(baseline, max(3, a.evals // 4))
        out(f"    baseline (logits, per-bag topk) {t_base[0]:10.1f} / {t_base[1]:10.1f} us   -> the new entry is {t_base[0] / t_new[0]:7.1f} x faster "
            f"(pooled values differ by at most {worst:.2e}, predictions agree on {100 * same:.1f} % of the clear cases)")


def parity(out):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_bags.py"), "-m", "gpu", "-q", "-s",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, cwd=ROOT)
    out("# the figures tests/test_gpu_bags.py prints before it asserts (one MI355X); bounds: tests/small_kernel_refs.py fp32_bound")
    for line in r.stdout.splitlines():
        line = line.lstrip(".")
        if line.startswith("bag parity:"):
            out(line)
    out("# " + (r.stdout.strip().splitlines() or ["no output"])[-1])
    return r.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--passes-only", action="store_true", help="the new entries only (for a rocprofv3 --kernel-trace --stats run)")
    ap.add_argument("--timing-only", action="store_true")
    ap.add_argument("--parity-only", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    rc = 0
    for name, on, fn in (("bag_pool_timing.txt", not a.parity_only, lambda o: timing(a, o)),
                         ("bag_pool_parity.txt", not a.timing_only and not a.passes_only, parity)):
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
