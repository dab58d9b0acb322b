"""Measure the ragged resize (plipmi_resize_crop_u8_ragged) on ViT-B/32 bf16 at batch 256.

    python tools/ragged_resize_bench.py [--out profiles/ragged_resize_bench.txt]

Runs two steps, each in a fresh child process under a time limit of its own, and stops at the first one that fails:

  entry  the ragged entry alone on 256 images with sizes drawn uniformly from 150..400 per side, against plipmi_resize_crop_u8 on 256
         images of the draw's mean side length in the same process: GPU time per call from the engine's per-launch events
         (Engine.profile), GB/s of source + destination bytes, and the ragged / uniform ratio per byte.
  e2e    PLIP.encode_images on 4096 such images held in host memory, num_workers=16, batch_size=256, ragged_resize on and off
         alternately (off = the host Pillow route such lists took before): img/s of each window, host clock around a call that ends
         in the copy of the embeddings back to the host.

Weights are synthetic (timing does not depend on their values); pixels are random bytes.
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


def _draw(count, lo=150, hi=400, seed=0):
    rs = np.random.RandomState(seed)
    hw = rs.randint(lo, hi + 1, size=(count, 2))
    return [rs.randint(0, 256, (int(h), int(w), 3), dtype=np.uint8) for h, w in hw]


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


def step_entry(a):
    import torch
    from plip_amd.engine import ragged_blob
    model, cfg = _model()
    eng, n = model.engine, cfg.image_size
    imgs = _draw(256)
    blob, offsets, hw = ragged_blob(imgs)
    dev = blob.to(eng.device)
    mean = int(round(float(np.mean(hw))))
    uni = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (256, mean, mean, 3), dtype=np.uint8)).to(eng.device)
    src_r, src_u, dst = int(blob.numel()) - 16 * 256, int(uni.numel()), 256 * n * n * 3
    calls = {"ragged": lambda: eng.resize_crop_ragged((dev, offsets, hw), crop="hf"),
             "uniform": lambda: eng.resize_crop_u8(uni, crop="hf")}
    scope = {"ragged": "resize_crop_u8_ragged", "uniform": "resize_crop_u8"}
    for fn in calls.values():                       # warm-up: code objects, the workspace, the uniform plan
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    per_call = {k: [] for k in calls}
    for _ in range(a.windows):                      # alternate the two inside every window
        for k, fn in calls.items():
            rows = []
            with eng.profile(rows):
                for _ in range(a.iters):
                    fn()
                torch.cuda.synchronize()
            r = [x for x in rows if x["name"] == scope[k]]
            assert len(r) == 1 and r[0]["calls"] == a.iters, rows
            per_call[k].append(r[0]["total_ms"] * 1e3 / a.iters)
    print(f"device {eng.device_name}; n_px {n}; 256 images; {a.windows} windows of {a.iters} calls; GPU time of the entry's launches (HIP events)")
    out = {}
    for k, nbytes in (("ragged", src_r + dst), ("uniform", src_u + dst)):
        us = np.asarray(per_call[k])
        med = float(np.median(us))
        out[k] = med / nbytes
        what = "sizes 150..400 per side" if k == "ragged" else f"all {mean} x {mean}"
        print(f"{k:8s} ({what}): median {med:8.1f} us per call (min {us.min():.1f}, max {us.max():.1f}); "
              f"{nbytes / 1e6:.1f} MB source + destination -> {nbytes / med / 1e3:.1f} GB/s")
    print(f"ragged / uniform time per byte: {out['ragged'] / out['uniform']:.2f}")


def step_e2e(a):
    import torch
    from plip_amd.plip import PLIP
    model, cfg = _model()
    imgs = _draw(a.images, seed=2)
    mb = sum(im.size for im in imgs) / 1e6
    plips = {"on": PLIP(model=model, ragged_resize=True), "off": PLIP(model=model)}
    outs = {}
    for k, p in plips.items():                      # warm-up of both routes on a slice
        outs[k] = p.encode_images(imgs[:512], batch_size=256, num_workers=16)
    print(f"device {model.engine.device_name}; host CPU {_cpu_model()} (this process may use {len(os.sched_getaffinity(0))} CPUs); "
          f"{a.images} images of 150..400 px per side in host memory ({mb:.0f} MB); batch_size 256, num_workers 16")
    print(f"on vs off embeddings on the first 512 images: max |diff| {np.abs(outs['on'] - outs['off']).max():.3e} (bf16 engine)")
    rate = {k: [] for k in plips}
    for _ in range(a.windows):
        for k, p in plips.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p.encode_images(imgs, batch_size=256, num_workers=16)           # ends in the D2H copy of the embeddings
            rate[k].append(a.images / (time.perf_counter() - t0))
    for k in plips:
        r = np.asarray(rate[k])
        print(f"ragged_resize {k:3s}: median {np.median(r):9.0f} img/s (min {r.min():.0f}, max {r.max():.0f}) over {a.windows} windows")
    print(f"on / off: {np.median(rate['on']) / np.median(rate['off']):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["entry", "e2e"])
    ap.add_argument("--out", default=None, help="also write the steps' output to this file")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--images", type=int, default=4096)
    a = ap.parse_args()
    if a.step:
        return {"entry": step_entry, "e2e": step_e2e}[a.step](a)
    log = []
    for step, limit in (("entry", 240), ("e2e", 420)):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--windows", str(a.windows),
               "--iters", str(a.iters), "--images", str(a.images)]
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
