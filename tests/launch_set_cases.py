"""The launch set of the engine's entries: what ``plipmi_profile_read`` reports (kernel name | role, calls, flops, bytes) for a
fixed list of calls.  tests/golden/launch_set.json is this recorded on the commit before csrc/engine.hip was split
(tests/golden/make_launch_set.py); tests/test_gpu_launch_set.py asserts the library still issues exactly those launches.
The numbers are the host's own arithmetic (no timing), so the comparison is exact.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np
import torch

GROUPS = ("tiny_bf16", "tiny_latency", "tiny_passes", "tiny_flags", "tiny_f32", "tiny_debug_and_outputs", "tiny_resolution",
          "vitb32_resolution")


def _rows(eng, fn):
    rows = []
    with eng.profile(rows):
        fn()
    torch.cuda.synchronize()
    return [[r["name"], r["calls"], r["flops"], r["bytes"]] for r in rows]


def _inputs(cfg, B, hw=None, seed=0):
    rs = np.random.RandomState(seed)
    h, w = hw or (cfg.image_size, cfg.image_size)
    px = torch.from_numpy(rs.standard_normal((B, 3, h, w)).astype(np.float32))
    tiles = torch.from_numpy(rs.randint(0, 256, size=(B, h, w, 3), dtype=np.uint8))
    ids = rs.randint(1, cfg.bos_token_id, size=(B, cfg.context_length)).astype(np.int64)
    for b in range(B):              # captions of different lengths, EOS-padded: the packed form has rows to drop
        ids[b, min(cfg.context_length - 1, 4 + 5 * b):] = cfg.eos_token_id
    return px, tiles, torch.from_numpy(ids)


def _encodes(eng, cfg, B, out, tag, packed=True):
    px, tiles, ids = _inputs(cfg, B)
    out[f"{tag}/encode_image"] = _rows(eng, lambda: eng.encode_image(px))
    out[f"{tag}/encode_image_u8"] = _rows(eng, lambda: eng.encode_image_u8(tiles))
    out[f"{tag}/encode_text"] = _rows(eng, lambda: eng.encode_text(ids))
    if packed:
        eng.set_text_packing(True)
        out[f"{tag}/encode_text_packed"] = _rows(eng, lambda: eng.encode_text(ids))
        eng.set_text_packing(False)


def record(group: str) -> dict:
    """{case: [[name, calls, flops, bytes], ...]} for one group of calls (each builds and closes its own engines)."""
    from plip_amd import _lib, weights as W
    from plip_amd import kernel_entries  # noqa: F401  (binds the test header: the fused-kernel hook)
    from plip_amd.config import get_config
    from plip_amd.engine import Engine
    cfg = get_config("tiny")
    sd = W.synthetic_state_dict(cfg, 0)
    out = {}

    def tiny(**kw):
        return Engine(cfg, sd, dtype=kw.pop("dtype", "bf16"), max_batch=8, **kw)

    if group == "tiny_bf16":
        eng = tiny()
        _encodes(eng, cfg, 3, out, "bf16 B=3")
        eng.close()
    elif group == "tiny_latency":
        eng = tiny()
        eng.set_latency_batch(8)
        _encodes(eng, cfg, 3, out, "bf16 latency_batch=8 B=3")
        eng.close()
        eng = tiny(text_f16_layers=1)           # a text tower that changes operand type after block 0: the re-coding pass
        eng.set_latency_batch(8)
        _encodes(eng, cfg, 3, out, "bf16 text_f16_layers=1 latency_batch=8 B=3", packed=False)
        eng.close()
    elif group == "tiny_passes":
        eng = tiny(pass_batch=2)
        _encodes(eng, cfg, 5, out, "bf16 pass_batch=2 B=5")
        eng.close()
    elif group == "tiny_flags":
        for tag, kw in (("dense last block", dict(pooled_last_block=False)), ("separate LayerNorm", dict(ln_fold=False)),
                        ("text tower f16", dict(text_f16=True)), ("text_f16_layers=2", dict(text_f16_layers=2)),
                        ("text_f16_layers=1", dict(text_f16_layers=1))):
            eng = tiny(**kw)
            _encodes(eng, cfg, 3, out, f"bf16 {tag} B=3", packed=False)
            eng.close()
    elif group == "tiny_f32":
        eng = tiny(dtype="f32")
        _encodes(eng, cfg, 3, out, "f32 B=3", packed=False)
        eng.close()
    elif group == "tiny_debug_and_outputs":
        for dtype in ("bf16", "f32"):
            eng = tiny(dtype=dtype)
            px, _, ids = _inputs(cfg, 3)
            out[f"{dtype}/debug_hidden vision layer 1"] = _rows(eng, lambda: eng.hidden("vision", 1, px))
            out[f"{dtype}/debug_hidden text layer 1"] = _rows(eng, lambda: eng.hidden("text", 1, ids))
            out[f"{dtype}/tower_outputs vision"] = _rows(eng, lambda: eng.tower_outputs(
                "vision", px, output_hidden_states=True, output_attentions=True))
            out[f"{dtype}/tower_outputs text"] = _rows(eng, lambda: eng.tower_outputs(
                "text", ids, output_hidden_states=True, output_attentions=True))
            eng.close()
    elif group == "tiny_resolution":
        # 144 x 128 on 16-pixel patches: 9 x 8 + 1 = 73 tokens, inside the fused q/k/v + attention kernel's range
        eng = tiny()
        d = eng.at_resolution(144, 128)
        px, tiles, _ = _inputs(cfg, d.max_batch, (144, 128))
        lib = _lib.load()
        try:
            _lib.check(lib.plipmi_test_fused_qkv_attention(2), "plipmi_test_fused_qkv_attention")
            out["bf16 144x128 fused/encode_image"] = _rows(d, lambda: d.encode_image(px))
        finally:
            lib.plipmi_test_reset_hooks()
        out["bf16 144x128/encode_image"] = _rows(d, lambda: d.encode_image(px))
        out["bf16 144x128/encode_image_u8"] = _rows(d, lambda: d.encode_image_u8(tiles))
        eng.close()
    elif group == "vitb32_resolution":
        # the im2col-on-load patch GEMM needs widths of 256 columns and a batch that fills the ring tile: never the tiny model.
        # ViT-B/32 at 288 x 256 (73 tokens), 175 images: the gather path, and the fused kernel by the product rule
        big = get_config("ViT-B/32")
        eng = Engine(big, W.synthetic_state_dict(big, 0), dtype="bf16", max_batch=256)
        d = eng.at_resolution(288, 256)
        px, tiles, _ = _inputs(big, d.max_batch, (288, 256))
        out["ViT-B/32 bf16 288x256 B=175/encode_image"] = _rows(d, lambda: d.encode_image(px))
        out["ViT-B/32 bf16 288x256 B=175/encode_image_u8"] = _rows(d, lambda: d.encode_image_u8(tiles))
        eng.close()
    else:
        raise KeyError(group)
    return out
