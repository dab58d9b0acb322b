"""Measure augmented views (plipmi_warp_u8, plip_amd/augment.py) on ViT-B/32 bf16, and count their mismatches against Pillow.

    python tools/augment_bench.py [--timing profiles/augment_timing.txt] [--parity profiles/augment_parity.txt]

timing  256 tiles of 512 x 512 px on the device; per window, alternating: the train chain's two warps for 256 views of 224 px
        (crop + flip + affine, then perspective; GPU time of each launch from the engine's per-launch events, Engine.profile), the D4
        set of 256 tiles of 224 px (8 launches, 2048 views), and the image tower's step on 256 of those views (encode_image_u8, host clock
        around a synchronise).  Then host Pillow's rate for the same chain (crop -> flip -> affine -> perspective on PIL images), one
        thread, on this machine's cores.
parity  mismatching bytes of the kernel against the numpy oracle and against Pillow, per shape; every count is to be 0.

Weights are synthetic (timing does not depend on their values)."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, SRC, NPX = 256, 512, 224


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


def _pil_warp(Image, im, row, perspective, n, fill=(127, 127, 127)):
    return im.transform((n, n), Image.PERSPECTIVE if perspective else Image.AFFINE, [float(v) for v in (row if perspective else row[:6])],
                        Image.BILINEAR, fillcolor=fill)


def _pil_chain(Image, im, window, affine, persp):
    wy, wx, n, _, flip = (int(v) for v in window)
    im = im.crop((wx, wy, wx + n, wy + n))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return _pil_warp(Image, _pil_warp(Image, im, affine, False, n), persp, True, n)


def timing(a, model):
    import torch
    from PIL import Image
    from plip_amd.augment import dihedral_views, train_views
    from plip_amd.preprocess import train_params
    eng = model.engine
    rs = np.random.RandomState(0)
    host = rs.randint(0, 256, size=(N, SRC, SRC, 3), dtype=np.uint8)
    dev = torch.from_numpy(host).to(eng.device)
    params = train_params(0, N, 1, (SRC, SRC), NPX)
    persp_drawn = int((params[2][:, 0] != np.asarray([1.0, 0, 0, 0, 1, 0, 0, 0])).any(axis=-1).sum())
    views = train_views(eng, dev, params)[0]
    tiles = views.clone()
    for _ in range(3):                              # warm-up: code objects, the tower's first calls
        train_views(eng, dev, params)
        dihedral_views(eng, tiles)
        eng.encode_image_u8(tiles)
    torch.cuda.synchronize()
    aff, per, d4, step = [], [], [], []
    for _ in range(a.windows):
        rows = []
        with eng.profile(rows):
            for _ in range(a.iters):
                train_views(eng, dev, params)
            torch.cuda.synchronize()
        by = {r["name"]: r for r in rows}
        assert by["warp_affine"]["calls"] == by["warp_perspective"]["calls"] == a.iters, rows
        aff.append(by["warp_affine"]["total_ms"] * 1e3 / a.iters)
        per.append(by["warp_perspective"]["total_ms"] * 1e3 / a.iters)
        rows = []
        with eng.profile(rows):                     # (the D4 launches are affine ones too; 224 % 4 == 0: the four-pixel kernel)
            for _ in range(a.iters):
                dihedral_views(eng, tiles)
            torch.cuda.synchronize()
        by = {r["name"]: r for r in rows}
        assert by["warp_affine"]["calls"] == 8 * a.iters, rows
        d4.append(by["warp_affine"]["total_ms"] * 1e3 / a.iters)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            eng.encode_image_u8(views)
        torch.cuda.synchronize()
        step.append((time.perf_counter() - t0) * 1e6 / a.iters)
    out_bytes = N * NPX * NPX * 3
    lines = [f"device {eng.device_name}; ViT-B/32 bf16, max_batch {eng.max_batch}; {N} source tiles of {SRC} x {SRC} px on the device, views of {NPX} px; "
             f"{a.windows} windows of {a.iters} calls; {persp_drawn} of the {N} views drew a perspective (the others: the identity row)",
             f"train stage 1, crop + flip + affine, {N} views (one launch, HIP events): {_stats(aff)} us  -> {out_bytes / np.median(aff) / 1e3:.0f} GB/s of output",
             f"train stage 2, perspective, {N} views (one launch, HIP events):          {_stats(per)} us  -> {out_bytes / np.median(per) / 1e3:.0f} GB/s of output",
             f"D4 set of {N} tiles, 8 launches, {8 * N} views (HIP events):            {_stats(d4)} us  -> {np.median(d4) / 8:.1f} us per {N} views",
             f"image tower step, encode_image_u8 on {N} views (host clock, synchronised): {_stats(step)} us",
             f"(stage 1 + stage 2) / step: {100 * (np.median(aff) + np.median(per)) / np.median(step):.2f} %   D4 per {N} views / step: "
             f"{100 * np.median(d4) / 8 / np.median(step):.2f} %   (DESIGN 4.11's threshold for considering a fused form: 3 %)"]
    # host Pillow, the same chain, one thread
    ims = [Image.fromarray(host[i]) for i in range(64)]
    for i in range(8):
        _pil_chain(Image, ims[i], params[0][i, 0], params[1][i, 0], params[2][i, 0])
    t0 = time.perf_counter()
    for i in range(64):
        _pil_chain(Image, ims[i], params[0][i, 0], params[1][i, 0], params[2][i, 0])
    dt = time.perf_counter() - t0
    cpus = len(os.sched_getaffinity(0))
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():         # a job's share of the machine, where its launcher states one
        cpus = min(cpus, int(os.environ["OMP_NUM_THREADS"]))
    lines.append(f"host Pillow, the same chain on PIL images, one thread: {64 / dt:.0f} views/s ({dt / 64 * 1e6:.0f} us per view) on {_cpu_model()}; "
                 f"this process may use {cpus} CPUs -> at most {cpus * 64 / dt:.0f} views/s with one worker per CPU; "
                 f"the two warps make {N / (np.median(aff) + np.median(per)) * 1e6:.0f} views/s")
    return lines


def _parity_rows(rs, h, w, oh, ow, B, perspective):
    """B rows well past the train ranges for an h x w source and an oh x ow output (host arithmetic only)"""
    from plip_amd.preprocess import affine_coeffs, check_perspective, perspective_coeffs
    rows = np.zeros((B, 8))
    for b in range(B):
        rows[b, :6] = affine_coeffs((w * 0.5, h * 0.5), rs.uniform(-40, 40), rs.uniform(-0.2, 0.2, 2) * [w, h], rs.uniform(0.5, 2.0), rs.uniform(-30, 30, 2))
        if not perspective:
            continue
        rows[b, 6:] = rs.uniform(-0.4, 0.4, 2) / [ow, oh]        # the fallback: the affine row under a denominator of 0.2 .. 1.8 at the corners
        if min(h, w) >= 3:                                       # (the corners of a thinner source coincide: no quadrilateral to distort)
            start = np.asarray([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
            for _ in range(20):                                  # a strongly distorted quadrilateral may fold over: a few more draws
                end = start + rs.uniform(0, 0.45, (4, 2)) * [w, h] * np.asarray([[1, 1], [-1, 1], [-1, -1], [1, -1]])
                try:
                    rows[b] = check_perspective(perspective_coeffs(start, end), oh, ow)
                    break
                except ValueError:
                    continue
    return check_perspective(rows, oh, ow) if perspective else rows


def parity(a, model):
    import torch
    from PIL import Image
    from plip_amd.augment import dihedral_views, train_views, warp_u8
    from plip_amd.preprocess import train_params, train_view_reference, warp_reference
    eng = model.engine
    rs = np.random.RandomState(1)
    lines = [f"device {eng.device_name}; mismatching bytes of plipmi_warp_u8 against preprocess.warp_reference (numpy float64) and against "
             f"Pillow {Image.__version__} Image.transform(..., BILINEAR, fillcolor=(127, 5, 250)); every count is to be 0"]
    total = 0
    fill = (127, 5, 250)
    for (h, w), (oh, ow), B in (((37, 53), (24, 24), 5), ((37, 53), (20, 33), 5), ((37, 53), (1, 1), 5), ((1, 1), (5, 6), 3), ((70, 5), (48, 4), 4),
                                ((224, 224), (224, 224), 8), ((512, 512), (224, 224), 8), ((300, 411), (97, 131), 6)):
        big = rs.randint(0, 256, size=(B, h + 4, w + 4, 3), dtype=np.uint8)
        src_np = big[:, 2:2 + h, 3:3 + w]
        src = torch.from_numpy(big).to(eng.device)[:, 2:2 + h, 3:3 + w]
        for perspective in (False, True):
            rows = _parity_rows(rs, h, w, oh, ow, B, perspective)
            for windowed in (False, True):
                wins = None
                if windowed:
                    wh, ww = rs.randint(1, h + 1, B), rs.randint(1, w + 1, B)
                    wins = np.stack([rs.randint(0, h - wh + 1), rs.randint(0, w - ww + 1), wh, ww, rs.randint(0, 2, B)], axis=1).astype(np.int32)
                got = warp_u8(eng, src, rows, wins, perspective, (oh, ow), fill).cpu().numpy()
                ref = np.stack([warp_reference(src_np[b], rows[b], perspective, (oh, ow), fill, None if wins is None else wins[b]) for b in range(B)])
                pw = []
                for b in range(B):
                    wy, wx, wh_, ww_, flip = (0, 0, h, w, 0) if wins is None else (int(v) for v in wins[b])
                    im = Image.fromarray(np.ascontiguousarray(src_np[b])).crop((wx, wy, wx + ww_, wy + wh_))
                    im = im.transpose(Image.FLIP_LEFT_RIGHT) if flip else im
                    pw.append(np.asarray(im.transform((ow, oh), Image.PERSPECTIVE if perspective else Image.AFFINE,
                                                      [float(v) for v in (rows[b] if perspective else rows[b, :6])], Image.BILINEAR, fillcolor=fill)))
                bad_ref, bad_pil = int((got != ref).sum()), int((got != np.stack(pw)).sum())
                total += bad_ref + bad_pil
                lines.append(f"source {h:3d} x {w:3d} (a view: pitch {3 * (w + 4)}, images {(h + 4) * (w + 4) * 3} bytes apart) -> {B} x {oh:3d} x {ow:3d}, "
                             f"{'perspective' if perspective else 'affine     '}, {'windows + flips' if windowed else 'whole source   '}: {got.size:8d} bytes, "
                             f"{bad_ref} differ from the oracle, {bad_pil} from Pillow")
    for n in (7, 224):
        tiles = rs.randint(0, 256, size=(4, n, n, 3), dtype=np.uint8)
        got = dihedral_views(eng, torch.from_numpy(tiles).to(eng.device)).cpu().numpy()
        want = np.stack([np.stack([np.rot90(t if k < 4 else t[:, ::-1], k % 4) for t in tiles]) for k in range(8)])
        total += int((got != want).sum())
        lines.append(f"dihedral views of 4 tiles of {n} px against np.rot90 / flips: {got.size} bytes, {int((got != want).sum())} differ")
    tiles = rs.randint(0, 256, size=(8, SRC, SRC, 3), dtype=np.uint8)
    params = train_params(0, 8, 3, (SRC, SRC), NPX)
    got = train_views(eng, torch.from_numpy(tiles).to(eng.device), params).cpu().numpy().transpose(1, 0, 2, 3, 4)
    ref = np.stack([np.stack([train_view_reference(tiles[i], params[0][i, v], params[1][i, v], params[2][i, v]) for v in range(3)]) for i in range(8)])
    pw = np.stack([np.stack([np.asarray(_pil_chain(Image, Image.fromarray(tiles[i]), params[0][i, v], params[1][i, v], params[2][i, v]))
                             for v in range(3)]) for i in range(8)])
    total += int((got != ref).sum()) + int((got != pw).sum())
    lines.append(f"train chain, 8 tiles of {SRC} px x 3 views of {NPX} px (two stages, each through bytes): {got.size} bytes, {int((got != ref).sum())} differ from "
                 f"the oracle, {int((got != pw).sum())} from the PIL chain crop -> transpose -> transform(AFFINE) -> transform(PERSPECTIVE)")
    lines.append(f"total mismatches: {total}")
    return lines, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timing", default=None, help="write the timing lines to this file")
    ap.add_argument("--parity", default=None, help="write the parity lines to this file")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from plip_amd import weights as W
    from plip_amd.config import get_config
    from plip_amd.model import PlipModel
    cfg = get_config("ViT-B/32")
    model = PlipModel(cfg, W.synthetic_state_dict(cfg, 0), dtype="bf16", max_batch=256)
    plines, total = parity(a, model)
    print("\n".join(plines), flush=True)
    if a.parity:
        with open(a.parity, "w") as f:
            f.write("\n".join(plines) + "\n")
    tlines = timing(a, model)
    print("\n".join(tlines), flush=True)
    if a.timing:
        with open(a.timing, "w") as f:
            f.write("\n".join(tlines) + "\n")
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
