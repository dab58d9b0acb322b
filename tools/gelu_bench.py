"""What the exact (erf) GELU costs against QuickGELU: the same weights run as a quick_gelu engine and as a gelu engine.

    python tools/gelu_bench.py [--dtypes bf16,f16] [--batch 256] [--iters 30] [--warmup 5] [--rounds 3]

ViT-B/32 with synthetic weights, inputs resident on the GPU.  For each dtype the two engines take turns (``--rounds`` alternations:
other work shares the host, so the spread between rounds is printed next to the difference), each turn ``--iters`` pair steps
(``Engine.encode_pair``: both towers, normalised embeddings) between two device events after ``--warmup`` untimed ones.  Then one
profiled step per engine (``Engine.profile``: HIP-event time per kernel and role) gives the ``fc1`` kernels' own time -- the only
launches that differ.  One JSON line per dtype: ms per pair step of both engines (median and range over the rounds), their ratio, and
the fc1 kernels' ms per step with their ratio."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from plip_amd import weights as W  # noqa: E402
from plip_amd.config import get_config  # noqa: E402
from plip_amd.engine import Engine  # noqa: E402


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
    return t0.elapsed_time(t1) / iters


def fc1_ms(eng: Engine, px, ids, mask, steps: int) -> dict:
    """ms per step of the fc1 launches (role ``fc1`` / ``fc1_pooled``), by kernel name, one tower after the other"""
    rows = []
    with eng.profile(rows):
        for _ in range(steps):
            eng.encode_image(px)
            eng.encode_text(ids, mask)
    torch.cuda.synchronize()
    return {r["name"]: round(r["total_ms"] / steps, 5) for r in rows if r["name"].split("|")[-1] in ("fc1", "fc1_pooled")}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="bf16,f16")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    base = get_config("ViT-B/32")
    sd = W.synthetic_state_dict(base, 0)
    B = a.batch
    px = torch.from_numpy(W.synthetic_pixels(base, B, 1000)).cuda()
    ids_np, mask_np = W.synthetic_ids(base, B, 2000)
    ids, mask = torch.from_numpy(ids_np).cuda(), torch.from_numpy(mask_np).cuda()
    for dtype in a.dtypes.split(","):
        engines = {act: Engine(base.with_hidden_act(act), sd, dtype=dtype, max_batch=B) for act in ("quick_gelu", "gelu")}
        try:
            ms = {act: [] for act in engines}
            with torch.no_grad():
                for _ in range(a.rounds):
                    for act, eng in engines.items():
                        ms[act].append(timed(lambda: eng.encode_pair(px, ids, mask), a.iters, a.warmup))
                fc1 = {act: fc1_ms(eng, px, ids, mask, 10) for act, eng in engines.items()}
            med = {act: statistics.median(v) for act, v in ms.items()}
            tot = {act: sum(v.values()) for act, v in fc1.items()}
            line = {"arch": "ViT-B/32", "dtype": dtype, "batch": B, "iters": a.iters, "rounds": a.rounds,
                    "pair_step_ms": {act: {"median": round(med[act], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                                     for act, v in ms.items()},
                    "pair_step_ratio_gelu_over_quick_gelu": round(med["gelu"] / med["quick_gelu"], 4),
                    "fc1_ms_per_step": fc1, "fc1_total_ms": {act: round(v, 4) for act, v in tot.items()},
                    "fc1_ratio_gelu_over_quick_gelu": round(tot["gelu"] / tot["quick_gelu"], 4),
                    "device": engines["gelu"].device_name}
            print(json.dumps(line), flush=True)
        finally:
            for eng in engines.values():
                eng.close()


if __name__ == "__main__":
    main()
