"""Measure the padded-head attention on an MI355X, once: the figures of profiles/head_dim_parity.txt and head_dim_timing.txt.

    python tools/head_dim_report.py [parity] [tower] [kernel]       # default: all three; needs the GPU

* ``parity``  ``PRESETS["ViT-H/14"]`` with GELU towers at full size, B = 2, on the f32, bf16 and f16 engines against the HF CPU fixture
              tests/golden/head_dim_vith14_b2.npz (tools/make_head_dim_golden.py vith14_b2); bars: tests/test_gpu_parity.py TOL.
* ``tower``   the ViT-H/14 image tower on the bf16 engine: img/s at B = 64 and the fraction of the dense bf16 MFMA peak via
              ``image_flops()`` (bench.py PEAK_TFLOPS).
* ``kernel``  the new MFMA kernel at head 80 / 88 / 128 against the head-64 chunked kernel at S = 257 and equal B * H: microseconds per
              launch and per workgroup (B * H * ceil(S / 128) of them).  About DP / 64 x the head-64 figure is the arithmetic.

Timings are medians of event-timed repeats after a warm-up, one process, nothing else on the card."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK_TFLOPS = 2500.0     # bench.py PEAK_TFLOPS["bf16"]
TOL = {"f32": dict(feat=2e-4, cos=1e-5, emb=1e-5), "bf16": dict(feat=6e-2, cos=1e-3, emb=6e-4), "f16": dict(feat=1.5e-2, cos=2.5e-4, emb=4e-4)}
KIND = {"image_features": "feat", "text_features": "feat", "image_embeds": "emb", "text_embeds": "emb", "logits_per_image": "cos"}


def _median_ms(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def parity():
    import make_head_dim_golden as M
    from plip_amd.model import PlipModel
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "head_dim_vith14_b2.npz")))
    cfg, sd, px, ids, mask = M.case_inputs("vith14_b2")
    np.testing.assert_array_equal(g["ids"], ids)
    tpx, tids, tmask = torch.from_numpy(px), torch.from_numpy(ids), torch.from_numpy(mask)
    scale = np.exp(np.float64(sd["logit_scale"]))
    for dtype in ("f32", "bf16", "f16"):
        model = PlipModel(cfg, sd, dtype=dtype, max_batch=8)
        out = model(input_ids=tids, pixel_values=tpx, attention_mask=tmask)
        err = {"image_features": np.abs(model.get_image_features(pixel_values=tpx).cpu().numpy() - g["image_features"]).max(),
               "text_features": np.abs(model.get_text_features(input_ids=tids, attention_mask=tmask).cpu().numpy() - g["text_features"]).max(),
               "image_embeds": np.abs(out.image_embeds.cpu().numpy() - g["image_embeds"]).max(),
               "text_embeds": np.abs(out.text_embeds.cpu().numpy() - g["text_embeds"]).max(),
               "logits_per_image": np.abs(out.logits_per_image.cpu().numpy() - g["logits_per_image"]).max() / scale}
        for k, e in err.items():
            bar = TOL[dtype][KIND[k]]
            print(f"PARITY group=head_dim_full case=vith14_b2_{dtype} field={k} bound={bar:.3e} gpu={float(e):.3e} {'ok' if e < bar else 'MISS'}", flush=True)
        model.engine.close()


def tower(B=64):
    import make_head_dim_golden as M
    from plip_amd import weights as W
    from plip_amd.engine import Engine
    cfg = M.case_config("vith14_b2")
    eng = Engine(cfg, W.synthetic_state_dict(cfg, 0), dtype="bf16", max_batch=B)
    px = torch.from_numpy(W.synthetic_pixels(cfg, B, 1)).to(eng.device)
    ms = _median_ms(lambda: eng.encode_image(px), reps=10, warmup=2)
    tf = B * cfg.image_flops() / (ms * 1e-3) / 1e12
    print(f"TIMING vith14 image tower bf16 B={B}: {ms:.2f} ms, {B / (ms * 1e-3):.0f} img/s, {tf:.0f} TFLOP/s = {tf / PEAK_TFLOPS:.3f} of the "
          f"{PEAK_TFLOPS:.0f} TFLOP/s dense peak ({cfg.image_flops() / 1e9:.1f} GFLOP per image)", flush=True)
    rows = []
    with eng.profile(rows):
        eng.encode_image(px)
    total = sum(r["total_ms"] for r in rows)
    for r in sorted(rows, key=lambda r: -r["total_ms"])[:6]:
        print(f"TIMING   {r['name']:60s} {r['calls']:4d} calls {r['total_ms']:8.3f} ms {100 * r['total_ms'] / total:5.1f} %", flush=True)
    eng.close()


def kernel(S=257, B=8, H=16):
    from plip_amd.kernel_entries import attention
    chunks = (S + 127) // 128
    base = None
    for dtype, name in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
        for head in (64, 80, 88, 96, 128):
            qkv = torch.randn(B * S, 3 * H * head, generator=torch.Generator().manual_seed(head)).to("cuda:0").to(dtype)
            out = torch.empty((B * S, H * head), dtype=dtype, device="cuda:0")
            ms = _median_ms(lambda: attention(qkv, B, S, H, impl=1, head_dim=None if head == 64 else head, out=out), reps=50, warmup=5)
            us = ms * 1e3
            if head == 64:
                base = us
            pad = 64 if head == 64 else (96 if head <= 96 else 128)
            print(f"TIMING attention mfma {name} head {head:3d} (padded {pad:3d}) S={S} B*H={B * H}: {us:7.1f} us per launch, "
                  f"{us / (B * H * chunks) * 1e3:6.1f} ns per workgroup (grid-averaged), {us / base:4.2f} x head 64 (arithmetic: {pad / 64:4.2f} x)", flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["parity", "tower", "kernel"]
    for w in what:
        {"parity": parity, "tower": tower, "kernel": kernel}[w]()
