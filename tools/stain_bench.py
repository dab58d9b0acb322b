"""Time Macenko stain normalisation on the GPU beside the tower step it feeds, on ViT-B/32 bf16 (synthetic weights: the timing does not
depend on them) and synthetic H&E tiles.

    python tools/stain_bench.py                    # -> profiles/stain_timing.txt (and stdout)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/stain_bench.py --passes-only      # kernel times

* A pass = the entry between two HIP events on the stream, min / median of ``--evals`` calls after a warm-up; the tiles stay resident.
* The tower step is ``encode_image_u8`` on the same 256 tiles; 3 % of it is where DESIGN 4.11 stops fusing a pre-processing pass into the gather.
* The host figure is the numpy oracle (``preprocess.stain_fit_reference`` / ``stain_apply_reference``) on the same tiles, wall time.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def _wall(fn, evals):
    import torch
    fn()
    ts = []
    for _ in range(evals):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--evals", type=int, default=10)
    ap.add_argument("--region", type=int, default=8192, help="side of the device region of the region fit")
    ap.add_argument("--encode-region", type=int, default=4096, help="side of the host region of the encode_region pair")
    ap.add_argument("--host-tiles", type=int, default=32, help="tiles the numpy oracle is timed on (scaled to --tiles)")
    ap.add_argument("--passes-only", action="store_true", help="the device passes only (for a rocprofv3 --kernel-trace --stats run)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    import stain_common as SC
    from plip_amd import preprocess as PP
    from plip_amd import weights as W
    from plip_amd.config import get_config
    from plip_amd.model import PlipModel
    from plip_amd.plip import PLIP
    from plip_amd.stain import stain_apply, stain_fit
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    cfg = get_config("ViT-B/32")
    model = PlipModel(cfg, W.synthetic_state_dict(cfg, 0), device="cuda:0", dtype="bf16", max_batch=a.tiles)
    plip, eng = PLIP(model=model), model.engine
    n, B = cfg.image_size, a.tiles
    side = int(np.ceil(np.sqrt(B)))
    sheet = SC.he_tile(1, side * n, side * n)
    tiles = np.ascontiguousarray(sheet.reshape(side, n, side, n, 3).transpose(0, 2, 1, 3, 4).reshape(-1, n, n, 3)[:B])
    dev = torch.from_numpy(tiles).to(eng.device)
    px = B * n * n
    out(f"# one MI355X ({eng.device_name}), ViT-B/32 bf16, {B} synthetic H&E tiles of {n} px resident on the device ({px * 3 / 1e6:.1f} MB); "
        f"min / median of {a.evals} calls, device events")
    t_tower = _time(lambda: eng.encode_image_u8(dev), a.evals)
    out(f"tower step (encode_image_u8, {B} tiles)            {t_tower[0]:10.1f} / {t_tower[1]:10.1f} us   3 % of it = {0.03 * t_tower[0]:8.1f} us")
    share = lambda t: f"{100 * t / t_tower[0]:6.2f} % of the tower step ({'under' if t < 0.03 * t_tower[0] else 'over'} the 3 % line)"
    passes = (("per-tile fit, step 1", lambda: stain_fit(eng, dev, pooled=False, step=1), 4 * 3.0),
              ("pooled fit, step 1", lambda: stain_fit(eng, dev, pooled=True, step=1), 4 * 3.0),
              ("pooled fit, default step 2", lambda: stain_fit(eng, dev, pooled=True, step=2), 4 * 3.0 / 4))
    res = {}
    for name, fn, bytes_px in passes:
        t = _time(fn, a.evals)
        res[name] = t
        # bytes: the pixels are read four times (moments and three key passes); the keys (4 B a sample) are written three times and read nine
        out(f"{name:<50s} {t[0]:10.1f} / {t[1]:10.1f} us   {share(t[0])}   {px * bytes_px / t[0] / 1e6:7.3f} TB/s of pixel reads")
    fit = stain_fit(eng, dev, pooled=False, step=1)
    t_apply = _time(lambda: stain_apply(eng, dev, fit), a.evals)
    out(f"{'apply, one fit per tile':<50s} {t_apply[0]:10.1f} / {t_apply[1]:10.1f} us   {share(t_apply[0])}   {px * 6 / t_apply[0] / 1e6:7.3f} TB/s read + written, "
        f"{px * 3 / t_apply[0] / 1e3:7.2f} G fp64 exp / s")
    del dev
    R = a.region
    reg = torch.from_numpy(np.tile(SC.he_tile(2, 2048, 2048), (R // 2048, R // 2048, 1))).to(eng.device)
    step = PP.stain_default_step(1, R, R)
    t_reg = _time(lambda: stain_fit(eng, reg, pooled=True, step=step), a.evals)
    out(f"{f'fit of a {R} x {R} device region, default step {step}':<50s} {t_reg[0]:10.1f} / {t_reg[1]:10.1f} us   {share(t_reg[0])}   "
        f"({(R // step) ** 2} samples)")
    del reg
    if a.passes_only:
        return 0
    E = a.encode_region
    host_region = np.tile(SC.he_tile(3, 1024, 1024), (E // 1024, E // 1024, 1))
    rfit = plip.fit_stain(host_region)
    w_plain = _wall(lambda: plip.encode_region(host_region), 3)
    w_stain = _wall(lambda: plip.encode_region(host_region, stain=rfit), 3)
    k = len(plip.encode_region(host_region).kept)
    out(f"encode_region, {E} x {E} host region, {k} tiles kept: {w_plain[0]:8.1f} / {w_plain[1]:8.1f} ms wall without stain=, {w_stain[0]:8.1f} / {w_stain[1]:8.1f} ms with "
        f"(+ {100 * (w_stain[0] / w_plain[0] - 1):.1f} %)")
    w_fit = _wall(lambda: plip.fit_stain(host_region), 3)
    out(f"fit_stain of that host region (subsampled on the host, step {rfit.step}, then uploaded): {w_fit[0]:8.1f} / {w_fit[1]:8.1f} ms wall")
    hb = min(a.host_tiles, B)
    t0 = time.perf_counter()
    rows = PP.stain_fit_reference(tiles[:hb])
    t_hfit = (time.perf_counter() - t0) * B / hb
    t0 = time.perf_counter()
    PP.stain_apply_reference(tiles[:hb], rows)
    t_happly = (time.perf_counter() - t0) * B / hb
    out(f"numpy oracle on this host ({os.cpu_count()} logical CPUs visible, one thread), timed on {hb} tiles and scaled to {B}: per-tile fit {t_hfit * 1e3:8.1f} ms, "
        f"apply {t_happly * 1e3:8.1f} ms")
    out(f"  -> the device per-tile fit takes 1 / {t_hfit * 1e6 / res['per-tile fit, step 1'][0]:.0f} and the device apply 1 / {t_happly * 1e6 / t_apply[0]:.0f} of the host's time")
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "stain_timing.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
