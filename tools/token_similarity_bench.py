"""Time the dense image-text similarity against what a caller had to compose before it, on one box in one run.

    python tools/token_similarity_bench.py [--arch ViT-B/32] [--dtype bf16] [--batch 256] [--prompts 10] [--reps 5] [--size 448] [--out FILE]

For the vision tower at the checkpoint's own size and at ``--size`` x ``--size`` (``Engine.at_resolution``; batch = that engine's
max_batch), after one warm-up call of each kind, ``--reps`` alternating pairs of

* ``token_similarity(engine, pixels, text_embeds)``                     -- the entry (plipmi_encode_token_similarity): the every-token walk,
                                                                           then layernorm, the token_proj GEMM and token_scores
* ``Engine.tower_outputs("vision", pixels).last_hidden_state`` followed by LayerNorm, the projection, both normalisations and the dot
  products in PyTorch on the GPU                                       -- the composition the entry replaces (it needs the caller's
                                                                           [B,S,Dv] copy)

timed by the host clock around one synchronised call (median), profile off; then ``--reps`` calls of the entry inside ``Engine.profile``
for the event times of its three tail launches and of the whole walk.  Synthetic weights, pixels and text rows: the time does not depend
on the values.  The two results are compared once (max-abs difference) so that the composition is known to compute the same thing."""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _measure(eng, px, txt, head, reps, lines):
    import torch

    from plip_amd.token_similarity import token_similarity
    ln_w, ln_b, proj, eps = head
    S, D, H, L = eng.tower_shape("vision")
    B, Cn = px.shape[0], txt.shape[0]

    def composed():
        x = eng.tower_outputs("vision", px).last_hidden_state
        e = torch.nn.functional.layer_norm(x, (D,), ln_w, ln_b, eps) @ proj.t()
        e = e / e.norm(dim=-1, keepdim=True)
        return e @ (txt / txt.norm(dim=-1, keepdim=True)).t()
    calls = {"entry": lambda: token_similarity(eng, px, txt).similarity, "composed": composed}
    outs = {k: fn() for k, fn in calls.items()}          # warm-up: code objects loaded, kernel attributes set, scratch allocated once
    torch.cuda.synchronize()
    diff = float((outs["entry"] - outs["composed"]).abs().max())
    outs = None
    wall = {k: [] for k in calls}
    for _ in range(reps):
        for kind, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            wall[kind].append((time.perf_counter() - t0) * 1e3)
            del out
    rows = []
    for _ in range(reps):
        with eng.profile(rows):
            out = calls["entry"]()
        del out
    agg = {}
    for r in rows:
        a = agg.setdefault(r["name"], [0, 0.0])
        a[0] += r["calls"]
        a[1] += r["total_ms"]
    med = {k: sorted(v)[len(v) // 2] for k, v in wall.items()}
    lines.append(f"vision tower, {S} tokens, B = {B}, C = {Cn} prompts, {reps} alternating calls of each kind; the two results differ by {diff:.2e}")
    lines.append(f"  entry:    host clock around a synchronised call {med['entry']:.3f} ms (median of {reps}; min {min(wall['entry']):.3f})")
    lines.append(f"  composed: host clock around a synchronised call {med['composed']:.3f} ms (median of {reps}; min {min(wall['composed']):.3f})"
                 f" -- tower_outputs + PyTorch; ratio entry / composed {med['entry'] / med['composed']:.3f}")
    lines.append(f"  entry, event profile: every kernel of the call {sum(v[1] for v in agg.values()) / reps:.3f} ms per call")
    tail = 0.0
    for name, (n, ms) in sorted(agg.items()):
        if name == "token_scores" or name.endswith("|token_proj"):
            lines.append(f"    {name:<56s} {ms / n * 1e3:9.1f} us per launch ({n} launches)")
            tail += ms / n
    ln = agg.get("layernorm")
    if ln:   # the walk's own LayerNorm launches share the name: per launch, over all of them
        lines.append(f"    {'layernorm (the walk own launches included)':<56s} {ln[1] / ln[0] * 1e3:9.1f} us per launch ({ln[0]} launches)")
    lines.append(f"    token_proj + token_scores together {tail * 1e3:.1f} us per call")
    return med


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="ViT-B/32")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--prompts", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=448, help="second image size (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from plip_amd import weights as W
    from plip_amd.config import get_config
    from plip_amd.model import PlipModel
    cfg = get_config(a.arch)
    sd = W.synthetic_state_dict(cfg, 0)
    model = PlipModel(cfg, sd, dtype=a.dtype, max_batch=a.batch)
    eng = model.engine
    dev = dict(device=eng.device, dtype=torch.float32)
    head = tuple(torch.as_tensor(sd[k]).to(**dev) for k in ("vision_model.post_layernorm.weight", "vision_model.post_layernorm.bias",
                                                             "visual_projection.weight")) + (cfg.layer_norm_eps,)
    txt = torch.randn((a.prompts, cfg.projection_dim), generator=torch.Generator().manual_seed(3)).to(eng.device)
    lines = [f"{a.arch} {a.dtype} on {eng.device_name}"]
    px = torch.from_numpy(W.synthetic_pixels(cfg, a.batch, 1)).to(eng.device)
    _measure(eng, px, txt, head, a.reps, lines)
    if a.size:
        e2 = eng.at_resolution(a.size, a.size)
        px2 = torch.randn((e2.max_batch, 3, a.size, a.size), generator=torch.Generator().manual_seed(2)).to(eng.device)
        _measure(e2, px2, txt, head, a.reps, lines)
    eng.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
