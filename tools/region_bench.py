"""Measure slide regions (plipmi_region_select / plipmi_region_gather, PLIP.encode_region) on ViT-B/32 bf16.

    python tools/region_bench.py [--out profiles/region_timing.txt]

An 8192 x 8192 synthetic region (glass = 240 +- 3 per channel; about 40 % of the 36 x 36 tiles of 224 px filled with random bytes),
tile = stride = 224.  Two steps, each in a fresh child process under a time limit of its own; the first failure ends the run:

  entry  the two entries alone on the region on the device: GPU time of their launches from the engine's per-launch events
         (Engine.profile) -- region_select with GB/s over the region's bytes, region_gather per 256 tiles with GB/s over source +
         destination bytes -- against the image tower's step on those 256 tiles (encode_image_u8, host clock around a synchronise).
  e2e    tiles/s of PLIP.encode_region on the region in host memory and on the device, alternating with the route such a region took
         before: crop every tile in numpy, keep it by the same rule (preprocess.tissue_mask), PLIP.encode_images on the list.  Host clock
         around calls that end in the copy of the embeddings to the host; the embeddings of the routes are compared.

Weights are synthetic (timing does not depend on their values).
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

SIDE, TILE = 8192, 224


def _region(seed=0, share=0.4):
    rs = np.random.RandomState(seed)
    region = (240 + rs.randint(-3, 4, size=(SIDE, SIDE, 3), dtype=np.int16)).astype(np.uint8)
    g = SIDE // TILE
    for idx in np.flatnonzero(rs.rand(g * g) < share):
        y, x = (idx // g) * TILE, (idx % g) * TILE
        region[y:y + TILE, x:x + TILE] = rs.randint(0, 256, size=(TILE, TILE, 3), dtype=np.uint8)
    return region


def _model(max_batch=256):
    from plip_amd import weights as W
    from plip_amd.config import get_config
    from plip_amd.model import PlipModel
    cfg = get_config("ViT-B/32")
    return PlipModel(cfg, W.synthetic_state_dict(cfg, 0), dtype="bf16", max_batch=max_batch), cfg


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _stats(v):
    v = np.asarray(v, dtype=np.float64)
    return f"median {np.median(v):9.1f} (min {v.min():.1f}, max {v.max():.1f})"


def step_entry(a):
    import torch
    from plip_amd.engine_region import region_gather, region_select
    model, cfg = _model()
    eng = model.engine
    host = _region()
    dev = torch.from_numpy(host).to(eng.device)
    counts, kept, n_kept = region_select(eng, dev, TILE)
    K = int(n_kept.item())
    assert K >= 256, K
    tiles = region_gather(eng, dev, kept, 0, 256, TILE)
    for _ in range(3):                              # warm-up: code objects, the tower's first calls
        region_select(eng, dev, TILE)
        region_gather(eng, dev, kept, 0, 256, TILE)
        eng.encode_image_u8(tiles)
    torch.cuda.synchronize()
    sel, gat, step = [], [], []
    for _ in range(a.windows):                      # the three alternate inside every window
        rows = []
        with eng.profile(rows):
            for _ in range(a.iters):
                region_select(eng, dev, TILE)
            for i in range(a.iters):
                region_gather(eng, dev, kept, (i * 64) % (K - 255), 256, TILE)
            torch.cuda.synchronize()
        by = {r["name"]: r for r in rows}
        assert by["region_count"]["calls"] == by["region_compact"]["calls"] == by["region_gather"]["calls"] == a.iters, rows
        sel.append((by["region_count"]["total_ms"] + by["region_compact"]["total_ms"]) * 1e3 / a.iters)
        gat.append(by["region_gather"]["total_ms"] * 1e3 / a.iters)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            eng.encode_image_u8(tiles)
        torch.cuda.synchronize()
        step.append((time.perf_counter() - t0) * 1e6 / a.iters)
    g = SIDE // TILE
    read = g * g * TILE * TILE * 3
    moved = 2 * 256 * TILE * TILE * 3
    print(f"device {eng.device_name}; region {SIDE} x {SIDE} x 3 uint8 on the device ({host.nbytes / 1e6:.0f} MB), {g} x {g} tiles of {TILE} px, "
          f"{K} kept; {a.windows} windows of {a.iters} calls")
    print(f"region_select (count + compact launches, HIP events): {_stats(sel)} us per call; {read / 1e6:.0f} MB of tile pixels read "
          f"-> {read / np.median(sel) / 1e3:.0f} GB/s ({host.nbytes / np.median(sel) / 1e3:.0f} GB/s over the region's {host.nbytes / 1e6:.0f} MB)")
    print(f"region_gather, 256 tiles (HIP events): {_stats(gat)} us per call; {moved / 1e6:.0f} MB source + destination "
          f"-> {moved / np.median(gat) / 1e3:.0f} GB/s")
    print(f"image tower step, encode_image_u8 on those 256 tiles (host clock, synchronised): {_stats(step)} us per call")
    print(f"gather / step: {100 * np.median(gat) / np.median(step):.2f} %")


def _host_route(plip, region, min_count):
    """what a caller did before: the grid, the filter and the list in numpy, then encode_images"""
    from plip_amd.preprocess import tissue_mask
    g = SIDE // TILE
    tiles = []
    for i in range(g):
        for j in range(g):
            tile = region[i * TILE:(i + 1) * TILE, j * TILE:(j + 1) * TILE]
            if int(tissue_mask(tile).sum()) >= min_count:
                tiles.append(tile)
    return plip.encode_images(tiles, batch_size=256)


def step_e2e(a):
    import torch
    from plip_amd.plip import PLIP
    from plip_amd.preprocess import region_min_count
    model, cfg = _model()
    plip = PLIP(model=model)
    region = _region()
    dev = torch.from_numpy(region).to(model.engine.device)
    min_count = region_min_count(0.5, TILE)
    routes = {"encode_region, host region": lambda: plip.encode_region(region).embeddings,
              "encode_region, device region": lambda: plip.encode_region(dev).embeddings,
              "numpy crop + mask, encode_images": lambda: _host_route(plip, region, min_count)}
    outs = {k: fn() for k, fn in routes.items()}            # warm-up of every route
    K = outs["encode_region, host region"].shape[0]
    g = SIDE // TILE
    print(f"device {model.engine.device_name}; host CPU {_cpu_model()} (this process may use {len(os.sched_getaffinity(0))} CPUs); "
          f"region {SIDE} x {SIDE} x 3 uint8 ({region.nbytes / 1e6:.0f} MB), {g * g} tiles of {TILE} px, {K} kept")
    ref = outs["numpy crop + mask, encode_images"]
    for k in list(routes)[:2]:
        same = outs[k].shape == ref.shape and bool((outs[k].view(np.uint32) == ref.view(np.uint32)).all())
        print(f"{k} vs the numpy route: {'bit-identical embeddings' if same else 'EMBEDDINGS DIFFER'}")
    secs = {k: [] for k in routes}
    for _ in range(a.windows):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                            # ends in the D2H copy of the embeddings
            secs[k].append(time.perf_counter() - t0)
    for k in routes:
        s = np.asarray(secs[k])
        print(f"{k:34s}: median {np.median(s) * 1e3:8.1f} ms per region (min {s.min() * 1e3:.1f}, max {s.max() * 1e3:.1f}) over {a.windows} windows "
              f"-> {K / np.median(s):8.0f} kept tiles/s, {g * g / np.median(s):8.0f} grid tiles/s")
    base = np.median(secs["numpy crop + mask, encode_images"])
    for k in list(routes)[:2]:
        print(f"numpy route / {k}: {base / np.median(secs[k]):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["entry", "e2e"])
    ap.add_argument("--out", default=None, help="also write the steps' output to this file")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if a.step:
        return {"entry": step_entry, "e2e": step_e2e}[a.step](a)
    log = []
    for step, limit in (("entry", 240), ("e2e", 300)):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--windows", str(a.windows),
               "--iters", str(a.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        text = f"== {step} ==\n{r.stdout}"
        print(text, end="", flush=True)
        log.append(text)
        if r.returncode != 0:
            print(r.stderr[-4000:], file=sys.stderr)
            log.append(f"step {step} failed with exit status {r.returncode}\n")
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(log))
    return 1 if r.returncode != 0 else 0


if __name__ == "__main__":
    sys.exit(main() or 0)
