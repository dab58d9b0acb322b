"""Time the attention summaries against the attention tensor they replace, with the engine's own event profile, on one box in one run.

    python tools/attention_summary_bench.py [--arch ViT-B/32] [--dtype bf16] [--batch 256] [--reps 5] [--size 448] [--out FILE]

For the vision tower at the checkpoint's own size and at ``--size`` x ``--size`` (``Engine.at_resolution``; batch = that engine's
max_batch), after one warm-up call of each kind, ``--reps`` alternating pairs of

* ``attention_summary(rollout=True, pooled_attention=True)``           -- attention_rollout_step per block (it stores the pooled rows
                                                                           on its way: no attention_pooled_rows launch)
* ``attention_summary(rollout=False, pooled_attention=True)``          -- attention_pooled_rows per block
* ``tower_outputs(output_attentions=True)``                             -- attention_probs per block (the [L,B,H,S,S] tensor)

run inside ``Engine.profile``; printed per call kind: the per-block time of those kernels (total over calls / number of launches) and
the whole walk's time (sum of every kernel's event time per call, and the host clock around one synchronised call).  Synthetic
weights and pixels: the time does not depend on the values."""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _measure(eng, px, reps, lines):
    import torch
    S, D, H, L = eng.tower_shape("vision")
    B = px.shape[0]
    calls = {"summary": lambda: eng.attention_summary("vision", px),
             "summary_pooled_only": lambda: eng.attention_summary("vision", px, rollout=False),
             "tower_outputs": lambda: eng.tower_outputs("vision", px, output_attentions=True)}
    rows = {k: [] for k in calls}
    wall = {k: [] for k in calls}
    for fn in calls.values():          # warm-up: code objects loaded, kernel attributes set, scratch and outputs allocated once
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for kind, fn in calls.items():
            with eng.profile(rows[kind]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                wall[kind].append((time.perf_counter() - t0) * 1e3)
            del out
    lines.append(f"vision tower, {S} tokens, B = {B}, {L} blocks of {H} heads, {reps} alternating calls of each kind")
    per_block = {}
    in_summary = {}
    for kind in calls:
        agg = {}
        for r in rows[kind]:
            a = agg.setdefault(r["name"], [0, 0.0])
            a[0] += r["calls"]
            a[1] += r["total_ms"]
        total = sum(v[1] for v in agg.values()) / reps
        lines.append(f"  {kind}: every kernel of the walk {total:.3f} ms per call (events), host clock around a synchronised call "
                     f"{sorted(wall[kind])[len(wall[kind]) // 2]:.3f} ms (median of {reps})")
        for name in ("attention_rollout_step", "attention_pooled_rows", "attention_probs"):
            if name in agg:
                per_block[name] = agg[name][1] / agg[name][0] * 1e3
                if kind == "summary":
                    in_summary[name] = per_block[name]
                lines.append(f"    {name:<24s} {per_block[name]:9.1f} us per block ({agg[name][0]} launches)")
    pair = in_summary["attention_rollout_step"] + in_summary.get("attention_pooled_rows", 0.0)
    lines.append(f"  per block, rollout + pooled rows in one call: rollout step {in_summary['attention_rollout_step']:.1f} us + pooled rows "
                 f"{in_summary.get('attention_pooled_rows', 0.0):.1f} us (stored by the step) = {pair:.1f} us against attention_probs "
                 f"{per_block['attention_probs']:.1f} us (ratio {pair / per_block['attention_probs']:.2f}); the two kernels launched "
                 f"separately: {per_block['attention_rollout_step'] + per_block['attention_pooled_rows']:.1f} us")
    return pair, per_block["attention_probs"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="ViT-B/32")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=448, help="second image size (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from plip_amd import weights as W
    from plip_amd.config import get_config
    from plip_amd.model import PlipModel
    cfg = get_config(a.arch)
    model = PlipModel(cfg, W.synthetic_state_dict(cfg, 0), dtype=a.dtype, max_batch=a.batch)
    eng = model.engine
    lines = [f"{a.arch} {a.dtype} on {eng.device_name}"]
    px = torch.from_numpy(W.synthetic_pixels(cfg, a.batch, 1)).to(eng.device)
    _measure(eng, px, a.reps, lines)
    if a.size:
        e2 = eng.at_resolution(a.size, a.size)
        g = torch.Generator().manual_seed(2)
        px2 = torch.randn((e2.max_batch, 3, a.size, a.size), generator=g).to(eng.device)
        _measure(e2, px2, a.reps, lines)
    eng.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
