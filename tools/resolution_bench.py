"""Throughput of the vision tower at other image sizes (Engine.at_resolution, the interpolated position table).

    python tools/resolution_bench.py [--sizes 224,336,448] [--iters 30] [--warmup 5] [--dtype bf16]

ViT-B/32 with synthetic weights, inputs resident on the GPU; for each size a derived engine (plipmi_clone_resolution) and
one full workspace batch (its ``max_batch``: about the 256-image workspace of the 224 px engine), fp32 pixels and uint8 tiles.
Warm-up calls, then ``--iters`` timed calls between two device events.  One JSON line per size: img/s of each input kind,
GFLOP per image (``PlipConfig.image_flops_at``), TFLOP/s and the share of the 2.5 PFLOP/s dense bf16 peak.  The 224 px row
runs on the derived engine at the native size (the checkpoint's own table), which is bit-identical to the native engine.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from plip_amd import weights as W  # noqa: E402
from plip_amd.config import get_config  # noqa: E402
from plip_amd.model import PlipModel  # noqa: E402

PEAK_BF16 = 2.5e15      # MI355X dense bf16 MFMA peak (FLOP/s)


def timed(fn, iters: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3 / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="224,336,448")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--max-batch", type=int, default=256, help="workspace of the 224 px engine the derived ones are sized from")
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    cfg = get_config("ViT-B/32")
    model = PlipModel(cfg, W.synthetic_state_dict(cfg, 0), dtype=a.dtype, max_batch=a.max_batch)
    try:
        for n in (int(s) for s in a.sizes.split(",")):
            eng = model.engine.at_resolution(n, n)
            B = eng.max_batch
            rs = np.random.RandomState(n)
            px = torch.from_numpy(rs.standard_normal((B, 3, n, n)).astype(np.float32)).cuda()
            tiles = torch.from_numpy(rs.randint(0, 256, size=(B, n, n, 3), dtype=np.uint8)).cuda()
            torch.cuda.synchronize()
            with torch.no_grad():
                s_px = timed(lambda: eng.encode_image(px), a.iters, a.warmup)
                s_u8 = timed(lambda: eng.encode_image_u8(tiles), a.iters, a.warmup)
            flop = cfg.image_flops_at(n, n)
            line = {"arch": "ViT-B/32", "dtype": a.dtype, "image": [n, n], "tokens": eng.v_tokens, "batch": B,
                    "pass_batch": eng.pass_batch, "iters": a.iters, "gflop_per_img": round(flop / 1e9, 4)}
            for kind, s in (("f32_pixels", s_px), ("u8_tiles", s_u8)):
                tf = flop * B / s / 1e12
                line[kind] = {"ms_per_call": round(s * 1e3, 4), "img_per_s": round(B / s, 1), "tflops": round(tf, 1),
                              "share_of_bf16_peak": round(tf * 1e12 / PEAK_BF16, 4)}
            line["device"] = model.engine.device_name
            print(json.dumps(line), flush=True)
    finally:
        model.engine.close()


if __name__ == "__main__":
    main()
