"""Kernel-level entries of libplipmi.so (include/plipmi_test.h) for ``tests/`` and ``tools/`` -- NOT part of the product path.

``plip_amd.PLIP`` / ``PlipModel`` / ``Engine`` never call anything in here: these wrappers drive single kernels (the NT GEMM with every
epilogue, the attention kernels, the fused text q/k/v + attention kernel, the residual-plane re-coding) through the same C ABI so that the
GPU tests can compare them with fp64 references, plus the host mirrors of the split residual planes the tests check the kernels against.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _lib
from ._lib import _TORCH_DTYPE, _code, _ptr, _stream_ptr


def gemm_nt(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = 0,
            variant: int = -1, alpha: float = 1.0, out: Optional[torch.Tensor] = None,
            trace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Kernel-level entry (tests / micro-bench): epilogue(A[M,K] @ W[N,K]^T); a, w fp32 or bf16 CUDA tensors."""
    lib = _lib.load()
    assert a.is_cuda and w.is_cuda and a.dtype == w.dtype and a.is_contiguous() and w.is_contiguous()
    code = _code(a.dtype)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.zeros((M, N), dtype=a.dtype if epilogue in (0, 1) else torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.plipmi_gemm_nt_traced(code, epilogue, variant, M, N, K, _ptr(a), _ptr(w), _ptr(bias), float(alpha),
                                             _ptr(out), _ptr(trace),
                                             _stream_ptr(a.device)),
                   "plipmi_gemm_nt")
    return out


def gemm_nt_ld(a: torch.Tensor, w: torch.Tensor, K: int, bias: Optional[torch.Tensor] = None, epilogue: int = 0,
               variant: int = -1, alpha: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """epilogue(A[:, :K] @ W[:, :K]^T) on row-padded operands: a [M, lda >= K], w [N, ldw >= K] (tests)."""
    lib = _lib.load()
    assert a.is_cuda and w.is_cuda and a.dtype == w.dtype and a.is_contiguous() and w.is_contiguous()
    code = _code(a.dtype)
    M, N = a.shape[0], w.shape[0]
    if out is None:
        out = torch.zeros((M, N), dtype=a.dtype if epilogue in (0, 1) else torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.plipmi_gemm_nt_ld(code, epilogue, variant, M, N, K, _ptr(a), a.shape[1], _ptr(w), w.shape[1],
                                         _ptr(bias), float(alpha), _ptr(out),
                                         _stream_ptr(a.device)), "plipmi_gemm_nt_ld")
    return out


def attention(qkv: torch.Tensor, B: int, S: int, H: int, causal: bool = False, key_mask: Optional[torch.Tensor] = None,
              impl: int = 0, head_dim: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Kernel-level entry (tests): qkv [B*S, 3*H*64] (scale folded into q) -> [B*S, H*64].  With ``head_dim`` the entry that carries
    the head size (``plipmi_attention_hd``): qkv [B*S, 3*H*head_dim] -> [B*S, H*head_dim], into ``out`` if the caller brings one."""
    lib = _lib.load()
    hd = 64 if head_dim is None else int(head_dim)
    assert qkv.is_cuda and qkv.is_contiguous() and qkv.shape == (B * S, 3 * H * hd)
    code = _code(qkv.dtype)
    if out is None:
        out = torch.empty((B * S, H * hd), dtype=qkv.dtype, device=qkv.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == qkv.dtype and out.shape == (B * S, H * hd)
    with torch.cuda.device(qkv.device):
        if head_dim is None:
            _lib.check(lib.plipmi_attention(code, impl, _ptr(qkv), _ptr(out), B, S, H, int(causal), _ptr(key_mask),
                                            _stream_ptr(qkv.device)), "plipmi_attention")
        else:
            _lib.check(lib.plipmi_attention_hd(code, impl, _ptr(qkv), _ptr(out), B, S, H, hd, int(causal), _ptr(key_mask),
                                               _stream_ptr(qkv.device)), "plipmi_attention_hd")
    return out


def qkv_attention(a: torch.Tensor, w: torch.Tensor, c2: torch.Tensor, stats: torch.Tensor, B: int, S: int, H: int,
                  causal: bool = True, key_mask: Optional[torch.Tensor] = None, eps: float = 1e-5,
                  trace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Kernel-level entry (tests) of the fused LayerNorm-folded q/k/v projection + attention (plipmi_qkv_attention):
    a [B*S, 64H], w [3*64H, 64H] (16-bit), c2 [3*64H], stats [B*S, H, 2] -> attention output [B*S, 64H]."""
    lib = _lib.load()
    D = H * 64
    assert a.is_cuda and a.is_contiguous() and w.is_contiguous() and a.shape == (B * S, D) and w.shape == (3 * D, D) and w.dtype == a.dtype
    assert stats.shape == (B * S, H, 2) and stats.is_contiguous()
    out = torch.empty((B * S, D), dtype=a.dtype, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.plipmi_qkv_attention(_code(a.dtype), _ptr(a), _ptr(w), _ptr(c2), _ptr(stats), H, float(eps), _ptr(out),
                                            B, S, H, int(causal), _ptr(key_mask), _ptr(trace),
                                            _stream_ptr(a.device)), "plipmi_qkv_attention")
    return out


def gemm_nt_ln(mode: int, a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, stats: Optional[torch.Tensor] = None,
               eps: float = 1e-5, variant: int = -1, out: Optional[torch.Tensor] = None):
    """Kernel-level entry (tests) for the LayerNorm-folded epilogues, see include/plipmi.h plipmi_gemm_nt_ln.
    mode 0/1 -> bf16 [M,N]; mode 2 -> (C fp32 updated in place, xb bf16 [M,N], st fp32 [M,N/64,2]); mode 3 -> the same
    update on the split residual stream: ``out`` = (hi 16-bit [M,N], lo uint8 [lo_plane_bytes(M, N)], the blocked 8-bit remainder
    plane), both updated in place; returns (hi, lo, st).  variant -3 (the small-M split-K kernel, K % 256 == 0) runs modes 0 .. 3 and
    refuses mode 4; its mode 3 adds (x + bias) + product like the tiles, its mode 2 x + (product + bias)."""
    lib = _lib.load()
    assert a.dtype in (torch.bfloat16, torch.float16) and w.dtype == a.dtype and a.is_contiguous() and w.is_contiguous()
    code, hdt = _code(a.dtype), a.dtype
    M, K = a.shape
    N = w.shape[0]
    stream = _stream_ptr(a.device)
    with torch.cuda.device(a.device):
        if mode in (0, 1):
            if out is None:
                out = torch.empty((M, N), dtype=hdt, device=a.device)
            _lib.check(lib.plipmi_gemm_nt_ln(code, mode, variant, M, N, K, _ptr(a), _ptr(w), _ptr(bias), _ptr(stats),
                                             stats.shape[1], float(eps), _ptr(out), None, None, stream), "plipmi_gemm_nt_ln")
            return out
        st = torch.empty((M, N // 64, 2), dtype=torch.float32, device=a.device)
        if mode in (3, 4):           # 4: planes read in a's format, written in the other 16-bit type's (hi is then to be VIEWED as that type)
            hi, lo = out
            assert hi.dtype == hdt and lo.dtype == torch.uint8 and lo.numel() == lo_plane_bytes(M, N) and hi.is_contiguous() and lo.is_contiguous()
            _lib.check(lib.plipmi_gemm_nt_ln(code, mode, variant, M, N, K, _ptr(a), _ptr(w), _ptr(bias), None, 0, float(eps),
                                             _ptr(lo), _ptr(hi), _ptr(st), stream), "plipmi_gemm_nt_ln")
            return hi, lo, st
        xb = torch.empty((M, N), dtype=hdt, device=a.device)
        _lib.check(lib.plipmi_gemm_nt_ln(code, 2, variant, M, N, K, _ptr(a), _ptr(w), _ptr(bias), None, 0, float(eps),
                                         _ptr(out), _ptr(xb), _ptr(st), stream), "plipmi_gemm_nt_ln")
        return out, xb, st


def gemm_nt_gelu(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stats: Optional[torch.Tensor] = None, eps: float = 1e-5,
                 variant: int = -1, out: Optional[torch.Tensor] = None, ln: Optional[bool] = None) -> torch.Tensor:
    """Kernel-level entry (tests) for the exact-GELU epilogues (plipmi_gemm_nt_gelu): gelu(A @ W^T + bias) in a's dtype, or with
    ``stats`` [M, ns, 2] the LayerNorm-folded form gelu(rstd * A @ W^T + bias) (16-bit).  ``ln`` overrides what ``stats`` implies."""
    lib = _lib.load()
    assert a.is_cuda and w.is_cuda and a.dtype == w.dtype and a.is_contiguous() and w.is_contiguous()
    M, K = a.shape
    N = w.shape[0]
    if ln is None:
        ln = stats is not None
    if out is None:
        out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.plipmi_gemm_nt_gelu(_code(a.dtype), int(ln), variant, M, N, K, _ptr(a), _ptr(w), _ptr(bias), _ptr(stats),
                                           0 if stats is None else stats.shape[1], float(eps), _ptr(out), _stream_ptr(a.device)),
                   "plipmi_gemm_nt_gelu")
    return out


def _pow2(k: torch.Tensor) -> torch.Tensor:
    """2^k as float64, built from the bit pattern (torch.pow / torch.ldexp are not exact on the GPU)"""
    return ((k.to(torch.int64) + 1023) << 52).view(torch.float64)


def lo_plane_index(M: int, N: int, device=None) -> torch.Tensor:
    """Byte offset of element (m, n) in the blocked lo plane (csrc/common.h lo_plane_off): blocks of 16 rows x 8 columns = 128 B,
    [row & 7][row >> 3 & 1][column & 7] inside a block, blocks column-major inside a 16-row band.  int64 [M, N]."""
    m = torch.arange(M, dtype=torch.int64, device=device)[:, None]
    n = torch.arange(N, dtype=torch.int64, device=device)[None, :]
    return (m >> 4) * 16 * N + (n >> 3) * 128 + (m & 7) * 16 + ((m >> 3) & 1) * 8 + (n & 7)


def lo_plane_bytes(M: int, N: int) -> int:
    return (M + 15) // 16 * 16 * N


def lo_plane_values(lo: torch.Tensor, M: int, N: int) -> torch.Tensor:
    """The remainders of rows 0 .. M-1 as int8 [M, N] (a band's rows past M are padding: kernels may leave anything there)."""
    return lo[lo_plane_index(M, N, lo.device).reshape(-1)].reshape(M, N).view(torch.int8)


def split_planes(x: torch.Tensor, dtype=torch.bfloat16):
    """fp32 [M, N] -> the engine's two-plane residual form (csrc/common.h split_f32<H>), on the host in torch integer / float64
    arithmetic, bit for bit what the kernels write: ``hi`` [M, N] in the operand type, ``lo`` = uint8 [lo_plane_bytes(M, N)] in the
    blocked layout (padding bytes zero).
    bf16: hi = nearest bf16 (ties away from zero); r = bits(x) - (hi << 16) in [-32768, 32767]; lo = min((r + 128) >> 8, 127).
    f16:  hi = nearest f16 (ties to even, saturating); lo = clamp(rint((x - hi) * 2^(18 - E(hi))), -127, 127), E >= -14 (symmetric: split(join(hi, lo)) gives hi back)."""
    assert x.dim() == 2
    M, N = x.shape
    if dtype == torch.bfloat16:
        u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        t = (u + 0x8000) & 0xFFFFFFFF
        hi = (t >> 16).to(torch.int32)
        r = (u - (t & 0xFFFF0000))                                   # in [-32768, 32767]
        lo = ((r + 128) >> 8).clamp(max=127)
        hi16 = torch.where(hi >= 32768, hi - 65536, hi).to(torch.int16).view(torch.bfloat16)
    else:
        assert dtype == torch.float16
        xc = x.contiguous().float()
        hi16 = xc.clamp(-65504.0, 65504.0).to(torch.float16)
        hf = hi16.float()
        eb = ((hf.view(torch.int32) >> 23) & 0xFF).clamp(min=113)
        lo = torch.round((xc.double() - hf.double()) * _pow2(145 - eb)).clamp(-127, 127).to(torch.int64)   # exact power-of-two scaling, ties to even
    plane = torch.zeros(lo_plane_bytes(M, N), dtype=torch.uint8, device=x.device)
    plane[lo_plane_index(M, N, x.device).reshape(-1)] = (lo & 0xFF).to(torch.uint8).reshape(-1)
    return hi16, plane


def join_planes(hi: torch.Tensor, lo: torch.Tensor) -> torch.Tensor:
    """The fp32 value the two planes stand for (csrc/common.h join_f32<H>), bit for bit what the kernels read."""
    M, N = hi.shape
    l8 = lo[lo_plane_index(M, N, hi.device).reshape(-1)].reshape(M, N).to(torch.int64)
    l8 = torch.where(l8 >= 128, l8 - 256, l8)
    if hi.dtype == torch.float16:
        hf = hi.float()
        eb = ((hf.view(torch.int32) >> 23) & 0xFF).clamp(min=113)
        return (hf.double() + l8.double() * _pow2(eb - 145)).float()
    h = hi.view(torch.int16).to(torch.int64) & 0xFFFF
    u = ((h << 16) + (l8 << 8)) & 0xFFFFFFFF
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u)
    return u.to(torch.int32).view(torch.float32)


def recode_planes(hi: torch.Tensor, lo: torch.Tensor, to_dtype) -> tuple:
    """The residual planes re-coded in place for the other 16-bit operand type (plipmi_recode_planes): returns (hi, lo) views."""
    lib = _lib.load()
    frm = _code(hi.dtype)
    to = _code(to_dtype)
    M, N = hi.shape
    assert hi.is_cuda and lo.is_cuda and hi.is_contiguous() and lo.is_contiguous() and lo.dtype == torch.uint8 and lo.numel() == lo_plane_bytes(M, N)
    with torch.cuda.device(hi.device):
        _lib.check(lib.plipmi_recode_planes(_ptr(hi), _ptr(lo), M, N, frm, to,
                                            _stream_ptr(hi.device)), "plipmi_recode_planes")
    return hi.view(_TORCH_DTYPE[to]), lo


def gemm_variant_built(dtype, variant: int) -> bool:
    return bool(_lib.load().plipmi_gemm_variant_built(_code(dtype), int(variant)))


def gemm_variants():
    lib = _lib.load()
    names, i = [], 0
    while True:
        n = lib.plipmi_gemm_variant_name(i)
        if not n:
            return names
        names.append(n.decode())
        i += 1


def resample_pos(table: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    """The position-table resampler of ``plipmi_clone_resolution`` on its own (include/plipmi_test.h ``plipmi_resample_pos``):
    fp32 [1 + n0*n0, D] (CLS row first) -> fp32 [1 + gh*gw, D], bicubic like ``torch.nn.functional.interpolate``."""
    lib = _lib.load()
    assert table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2
    n0 = int(round((table.shape[0] - 1) ** 0.5))
    assert n0 * n0 + 1 == table.shape[0], "table rows must be 1 + n0 * n0"
    out = torch.empty((1 + gh * gw, table.shape[1]), dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        _lib.check(lib.plipmi_resample_pos(_ptr(table), _ptr(out), n0, int(gh), int(gw), table.shape[1],
                                           _stream_ptr(table.device)), "plipmi_resample_pos")
    return out


def probe_loss_grad(engine, x: torch.Tensor, y: torch.Tensor, wb: torch.Tensor, pos_w: torch.Tensor, neg_w: torch.Tensor, alpha: float):
    """One evaluation of the linear-probe objective (include/plipmi_test.h ``plipmi_probe_loss_grad``): x fp32 [N, D], y int32 [N],
    wb fp32 [K, D + 1], pos_w / neg_w fp32 [K], all on the engine's device -> (loss double [K], grad fp32 [K, D + 1])."""
    lib = _lib.load()
    for t, dt in ((x, torch.float32), (y, torch.int32), (wb, torch.float32), (pos_w, torch.float32), (neg_w, torch.float32)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous()
    N, D = x.shape
    K = wb.shape[0]
    assert wb.shape[1] == D + 1 and y.shape == (N,) and pos_w.shape == (K,) and neg_w.shape == (K,)
    loss = torch.empty((K,), dtype=torch.float64, device=x.device)
    grad = torch.empty((K, D + 1), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.plipmi_probe_loss_grad(engine._h, _ptr(x), N, D, _ptr(y), K, _ptr(pos_w), _ptr(neg_w), float(alpha), _ptr(wb),
                                              _ptr(loss), _ptr(grad), _stream_ptr(x.device)),
                   "plipmi_probe_loss_grad")
    return loss, grad


def softmax_loss_grad(engine, x: torch.Tensor, y: torch.Tensor, wb: torch.Tensor, class_w: Optional[torch.Tensor], alpha: float):
    """One evaluation of the softmax probe's objective (include/plipmi_test.h ``plipmi_softmax_loss_grad``): x fp32 [N, D], y int32 [N],
    wb fp32 [C, D + 1], class_w fp32 [C] or None (ones), all on the engine's device -> (loss double [1], grad fp32 [C, D + 1]).  The
    outputs are filled with NaN first, so an element the kernels do not write shows."""
    lib = _lib.load()
    for t, dt in ((x, torch.float32), (y, torch.int32), (wb, torch.float32)) + (() if class_w is None else ((class_w, torch.float32),)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous()
    N, D = x.shape
    C = wb.shape[0]
    assert wb.shape[1] == D + 1 and y.shape == (N,) and (class_w is None or class_w.shape == (C,))
    loss = torch.full((1,), float("nan"), dtype=torch.float64, device=x.device)
    grad = torch.full((C, D + 1), float("nan"), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.plipmi_softmax_loss_grad(engine._h, _ptr(x), N, D, _ptr(y), C, _ptr(class_w), float(alpha), _ptr(wb),
                                                _ptr(loss), _ptr(grad), _stream_ptr(x.device)),
                   "plipmi_softmax_loss_grad")
    return loss, grad


def kmeans_update(engine, x: torch.Tensor, labels: torch.Tensor, scores: torch.Tensor, sums: torch.Tensor, counts: torch.Tensor,
                  reps: torch.Tensor, inertia: torch.Tensor, metric: int, n: Optional[int] = None, k: Optional[int] = None) -> None:
    """The update step of k-means (include/plipmi_test.h ``plipmi_kmeans_update``) INTO the caller's buffers, so a test can fill them with
    sentinels and hang guard rows behind them: x fp32 [>= N, D], labels int32 [>= N], scores fp32 [>= N] -> sums fp32 [>= K, D], counts /
    reps int32 [>= K], inertia double [>= 1].  ``n`` / ``k`` default to the leading sizes of x / sums.  metric: 0 euclidean, 1 cosine."""
    lib = _lib.load()
    for t, dt in ((x, torch.float32), (labels, torch.int32), (scores, torch.float32), (sums, torch.float32), (counts, torch.int32),
                  (reps, torch.int32), (inertia, torch.float64)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous()
    N = x.shape[0] if n is None else int(n)
    K = sums.shape[0] if k is None else int(k)
    D = x.shape[1]
    assert sums.shape[1] == D
    with torch.cuda.device(x.device):
        _lib.check(lib.plipmi_kmeans_update(engine._h, _ptr(x), N, D, _ptr(labels), _ptr(scores), K, int(metric), _ptr(sums), _ptr(counts),
                                            _ptr(reps), _ptr(inertia), _stream_ptr(x.device)), "plipmi_kmeans_update")


def stain_percentile(engine, keys: torch.Tensor, q, out: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None):
    """The exact percentile of the stain fit alone (include/plipmi_test.h ``plipmi_stain_percentile``): keys fp32 [S, n] on the
    engine's device (NaN = absent), ``q`` percentiles in [0, 100] -> (out double [S, Q], counts int32 [S]), written INTO the caller's
    buffers where given (a test hangs sentinels around them)."""
    import ctypes as C_
    lib = _lib.load()
    assert keys.is_cuda and keys.dtype == torch.float32 and keys.is_contiguous() and keys.dim() == 2
    S, n = keys.shape
    qs = (C_.c_double * len(q))(*[float(v) for v in q])
    if out is None:
        out = torch.empty((S, len(q)), dtype=torch.float64, device=keys.device)
    if counts is None:
        counts = torch.empty((S,), dtype=torch.int32, device=keys.device)
    assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= S * len(q)
    assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= S
    with torch.cuda.device(keys.device):
        ws = torch.empty((max(int(lib.plipmi_stain_workspace(max(S, 1), 1, max(n, 1), 1)), 16),), dtype=torch.uint8, device=keys.device)
        _lib.check(lib.plipmi_stain_percentile(engine._h, _ptr(keys), S, n, qs, len(q), _ptr(out), _ptr(counts), _ptr(ws),
                                               _stream_ptr(keys.device)), "plipmi_stain_percentile")
    return out, counts


def stain_apply_into(engine, src: torch.Tensor, fits: torch.Tensor, target: torch.Tensor, lut: torch.Tensor, dst: torch.Tensor, Io: float = 240.0,
                     pitch: Optional[int] = None, image_stride: Optional[int] = None) -> torch.Tensor:
    """``plipmi_stain_apply`` INTO the caller's ``dst`` (uint8, at least B * H * W * 3 bytes from its first element, guard bytes around
    it if the test wants them): src uint8 [B,H,W,3] view with last strides (3, 1), fits double [1 or B, 16], target double [8], lut
    double [256], all on the engine's device.  ``pitch`` / ``image_stride`` override what the view's strides say (to be refused)."""
    lib = _lib.load()
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 4 and dst.is_cuda and dst.dtype == torch.uint8
    B, H, W = (int(v) for v in src.shape[:3])
    p = (int(src.stride(1)) if H > 1 else 3 * W) if pitch is None else int(pitch)
    st = (int(src.stride(0)) if B > 1 else H * p) if image_stride is None else int(image_stride)
    with torch.cuda.device(src.device):
        _lib.check(lib.plipmi_stain_apply(engine._h, _ptr(src), B, H, W, p, st, _ptr(fits), int(fits.shape[0]), _ptr(target), float(Io), _ptr(lut),
                                          _ptr(dst), _stream_ptr(src.device)), "plipmi_stain_apply")
    return dst


# ---- the kernels around the GEMMs (include/plipmi_test.h, tests/test_gpu_small_kernels.py) ---------------------------------------------
def _f32(*ts):
    for t in ts:
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


def attention_probs(qkv: torch.Tensor, B: int, S: int, H: int, causal: bool = False, key_mask: Optional[torch.Tensor] = None,
                    head_dim: Optional[int] = None) -> torch.Tensor:
    """``plipmi_attention_probs``: qkv [B*S, 3*H*64] (fp32 / bf16 / f16, scale folded into q) -> fp32 probabilities [B, H, S, S].
    With ``head_dim`` (here and in the two summaries below): the ``_hd`` entry, qkv [B*S, 3*H*head_dim]."""
    lib = _lib.load()
    assert qkv.is_cuda and qkv.is_contiguous() and qkv.shape == (B * S, 3 * H * (64 if head_dim is None else head_dim))
    assert key_mask is None or (key_mask.is_cuda and key_mask.dtype == torch.int64 and key_mask.is_contiguous() and key_mask.shape == (B, S))
    probs = torch.empty((B, H, S, S) if S <= 1024 else (1,), dtype=torch.float32, device=qkv.device)   # S > 1024 is refused before any launch
    with torch.cuda.device(qkv.device):
        if head_dim is None:
            _lib.check(lib.plipmi_attention_probs(_code(qkv.dtype), _ptr(qkv), _ptr(probs), B, S, H, int(causal), _ptr(key_mask), _stream_ptr(qkv.device)),
                       "plipmi_attention_probs")
        else:
            _lib.check(lib.plipmi_attention_probs_hd(_code(qkv.dtype), _ptr(qkv), _ptr(probs), B, S, H, int(head_dim), int(causal), _ptr(key_mask),
                                                     _stream_ptr(qkv.device)), "plipmi_attention_probs_hd")
    return probs


def attention_pooled_rows(qkv: torch.Tensor, rows: torch.Tensor, B: int, S: int, H: int, causal: bool = False,
                          key_mask: Optional[torch.Tensor] = None, head_dim: Optional[int] = None) -> torch.Tensor:
    """``plipmi_attention_pooled_rows``: row ``rows[b]`` (int32 [B]) of every head's probabilities -> fp32 [B, H, S]."""
    lib = _lib.load()
    assert qkv.is_cuda and qkv.is_contiguous() and qkv.shape == (B * S, 3 * H * (64 if head_dim is None else head_dim))
    assert rows.is_cuda and rows.dtype == torch.int32 and rows.is_contiguous() and rows.shape == (B,)
    assert key_mask is None or (key_mask.is_cuda and key_mask.dtype == torch.int64 and key_mask.is_contiguous() and key_mask.shape == (B, S))
    out = torch.empty((B, H, S) if S <= 1024 else (1,), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        if head_dim is None:
            _lib.check(lib.plipmi_attention_pooled_rows(_code(qkv.dtype), _ptr(qkv), _ptr(rows), _ptr(out), B, S, H, int(causal), _ptr(key_mask),
                                                        _stream_ptr(qkv.device)), "plipmi_attention_pooled_rows")
        else:
            _lib.check(lib.plipmi_attention_pooled_rows_hd(_code(qkv.dtype), _ptr(qkv), _ptr(rows), _ptr(out), B, S, H, int(head_dim), int(causal),
                                                           _ptr(key_mask), _stream_ptr(qkv.device)), "plipmi_attention_pooled_rows_hd")
    return out


def attention_rollout_step(qkv: torch.Tensor, R_in: Optional[torch.Tensor], B: int, S: int, H: int, causal: bool = False,
                           key_mask: Optional[torch.Tensor] = None, head_dim: Optional[int] = None) -> torch.Tensor:
    """``plipmi_attention_rollout_step``: (1/2 mean_h P + 1/2 I) . R_in -> a new fp32 [B, S, S]; ``R_in`` None = the identity."""
    lib = _lib.load()
    assert qkv.is_cuda and qkv.is_contiguous() and qkv.shape == (B * S, 3 * H * (64 if head_dim is None else head_dim))
    assert R_in is None or (R_in.is_cuda and R_in.dtype == torch.float32 and R_in.is_contiguous() and R_in.shape == (B, S, S))
    assert key_mask is None or (key_mask.is_cuda and key_mask.dtype == torch.int64 and key_mask.is_contiguous() and key_mask.shape == (B, S))
    out = torch.empty((B, S, S) if S <= 1024 else (1,), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        if head_dim is None:
            _lib.check(lib.plipmi_attention_rollout_step(_code(qkv.dtype), _ptr(qkv), _ptr(R_in), _ptr(out), B, S, H, int(causal),
                                                         _ptr(key_mask), _stream_ptr(qkv.device)), "plipmi_attention_rollout_step")
        else:
            _lib.check(lib.plipmi_attention_rollout_step_hd(_code(qkv.dtype), _ptr(qkv), _ptr(R_in), _ptr(out), B, S, H, int(head_dim), int(causal),
                                                            _ptr(key_mask), _stream_ptr(qkv.device)), "plipmi_attention_rollout_step_hd")
    return out


def layernorm(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float = 1e-5, out_dtype=torch.float32, inplace: bool = False) -> torch.Tensor:
    """``plipmi_layernorm``: x fp32 [rows, D], possibly a strided view of a wider buffer (row stride and storage offset multiples of 4
    elements, unit column stride) -> contiguous [rows, D] of ``out_dtype``; ``inplace``: y is x itself (contiguous fp32 rows)."""
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and (x.shape[1] == 1 or x.stride(1) == 1)
    _f32(g, b)
    rows, D = x.shape
    assert g.numel() == D and b.numel() == D
    xs = x.stride(0) if rows > 1 else D
    if inplace:
        assert x.is_contiguous() and out_dtype == torch.float32
        y = x
    else:
        y = torch.empty((rows, D), dtype=out_dtype, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.plipmi_layernorm(_ptr(x), xs, _ptr(g), _ptr(b), _ptr(y), _code(out_dtype), rows, D, float(eps), _stream_ptr(x.device)),
                   "plipmi_layernorm")
    return y


def layernorm_emit(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, dtype, eps: float = 1e-5):
    """``plipmi_layernorm_emit``: x fp32 [rows, D] -> (hi [rows, D] of ``dtype``, lo uint8 [lo_plane_bytes], st fp32 [rows, D // 64, 2])."""
    lib = _lib.load()
    _f32(x, g, b)
    rows, D = x.shape
    assert g.numel() == D and b.numel() == D
    hi = torch.empty((rows, D), dtype=dtype, device=x.device)
    lo = torch.zeros(lo_plane_bytes(rows, D), dtype=torch.uint8, device=x.device)
    st = torch.empty((rows, max(D // 64, 1), 2), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.plipmi_layernorm_emit(_code(dtype), _ptr(x), _ptr(g), _ptr(b), _ptr(hi), _ptr(lo), _ptr(st), rows, D, float(eps),
                                             _stream_ptr(x.device)), "plipmi_layernorm_emit")
    return hi, lo, st


def fold_ln(w: torch.Tensor, bias: torch.Tensor, g: torch.Tensor, b: torch.Tensor, dtype, pre: float = 1.0):
    """``plipmi_fold_ln``: W fp32 [rows, K], bias [rows], LayerNorm gain / bias [K] -> (Wf [rows, K] of ``dtype``, c2 fp32 [rows])."""
    lib = _lib.load()
    _f32(w, bias, g, b)
    rows, K = w.shape
    assert bias.numel() == rows and g.numel() == K and b.numel() == K
    wf = torch.empty((rows, K), dtype=dtype, device=w.device)
    c2 = torch.empty((rows,), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(lib.plipmi_fold_ln(_code(dtype), _ptr(w), _ptr(bias), _ptr(g), _ptr(b), _ptr(wf), _ptr(c2), rows, K, float(pre), _stream_ptr(w.device)),
                   "plipmi_fold_ln")
    return wf, c2


def text_embed_emit(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, dtype, packed: bool = False, eos_id: int = -1):
    """``plipmi_text_embed_emit``: ids int64 [B, S], tok fp32 [vocab, D], pos fp32 [>= S, D] -> (hi, lo, st) of the [B*S, D] rows; with
    ``packed`` the pack plan runs first and the result is (hi, lo, st, cu int32 [B + 1], rowmap int32 [B*S], m int32 [1]): only rows
    0 .. m-1 of the planes / statistics and entries 0 .. m-1 of rowmap are written (rowmap starts zeroed)."""
    lib = _lib.load()
    assert ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.dim() == 2
    _f32(tok, pos)
    B, S = ids.shape
    vocab, D = tok.shape
    assert pos.shape[1] == D and pos.shape[0] >= S
    dev = ids.device
    hi = torch.zeros((B * S, D), dtype=dtype, device=dev)
    lo = torch.zeros(lo_plane_bytes(B * S, D), dtype=torch.uint8, device=dev)
    st = torch.zeros((B * S, max(D // 64, 1), 2), dtype=torch.float32, device=dev)
    cu = rowmap = m = None
    if packed:
        cu = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
        rowmap = torch.zeros((B * S,), dtype=torch.int32, device=dev)
        m = torch.zeros((1,), dtype=torch.int32, device=dev)
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.plipmi_text_embed_emit(_code(dtype), int(packed), _ptr(ids), _ptr(tok), _ptr(pos), _ptr(hi), _ptr(lo), _ptr(st), B, S, D,
                                              vocab, int(eos_id), _ptr(cu), _ptr(rowmap), _ptr(m), _ptr(bad), _stream_ptr(ids.device)),
                   "plipmi_text_embed_emit")
    assert int(bad.item()) == 0, "token id outside the vocabulary"
    return (hi, lo, st, cu, rowmap, m) if packed else (hi, lo, st)


def pool_rows(x: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, ids: Optional[torch.Tensor] = None, eos_id: int = -1,
              wt: Optional[torch.Tensor] = None, normalize: bool = False, eps: float = 1e-5) -> torch.Tensor:
    """``plipmi_pool_rows``: x fp32 [B, S, D] -> LayerNorm of the pooled row (row 0, or the EOS row of ``ids`` int64 [B, S]); with
    ``wt`` fp32 [D, P] (the projection transposed) the pooled head [B, P] (mode 0), without it the LayerNorm'd row [B, D] (mode 1)."""
    lib = _lib.load()
    _f32(x, ln_w, ln_b)
    B, S, D = x.shape
    assert ln_w.numel() == D and ln_b.numel() == D
    assert ids is None or (ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.shape == (B, S))
    P = 0
    if wt is not None:
        _f32(wt)
        assert wt.shape[0] == D
        P = wt.shape[1]
    out = torch.empty((B, P if wt is not None else D), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.plipmi_pool_rows(0 if wt is not None else 1, _ptr(x), B, S, D, _ptr(ids), int(eos_id), _ptr(ln_w), _ptr(ln_b), float(eps),
                                        _ptr(wt), P, int(normalize), _ptr(out), _stream_ptr(x.device)), "plipmi_pool_rows")
    return out


def pool_gather(att: torch.Tensor, hi: torch.Tensor, lo: torch.Tensor, B: int, S: int, ids: Optional[torch.Tensor] = None, eos_id: int = -1,
                cu: Optional[torch.Tensor] = None):
    """``plipmi_pool_gather``: att [rows, D] (16-bit) and the planes (hi [rows, D], lo) -> (attp [B, D], xp fp32 [B, D]) of each sample's
    pooled row; rows = B * S, or cu[B] packed rows with ``cu`` int32 [B + 1] (every cu[b + 1] - 1 must be a row of the buffers)."""
    lib = _lib.load()
    rows, D = att.shape
    assert att.is_cuda and att.is_contiguous() and hi.is_contiguous() and lo.is_contiguous() and hi.dtype == att.dtype
    assert hi.shape == (rows, D) and lo.dtype == torch.uint8 and lo.numel() == lo_plane_bytes(rows, D)
    assert ids is None or (ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.shape == (B, S))
    if cu is not None:
        assert cu.is_cuda and cu.dtype == torch.int32 and cu.shape == (B + 1,)
        c = cu.cpu()
        assert int(c[1:].min()) >= 1 and int(c.max()) <= rows
    else:
        assert rows == B * S
    attp = torch.empty((B, D), dtype=att.dtype, device=att.device)
    xp = torch.empty((B, D), dtype=torch.float32, device=att.device)
    with torch.cuda.device(att.device):
        _lib.check(lib.plipmi_pool_gather(_code(att.dtype), _ptr(att), _ptr(hi), _ptr(lo), B, S, D, _ptr(ids), int(eos_id), _ptr(cu), _ptr(attp),
                                          _ptr(xp), _stream_ptr(att.device)), "plipmi_pool_gather")
    return attp, xp


def head_gemm(a: torch.Tensor, w: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """``plipmi_head_gemm``: scale * a [M, K] @ w [N, K]^T in fp32 (split-K MFMA kernel of the heads and the logits)."""
    lib = _lib.load()
    _f32(a, w)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.plipmi_head_gemm(_ptr(a), _ptr(w), _ptr(out), M, N, K, float(scale), _stream_ptr(a.device)), "plipmi_head_gemm")
    return out


def resize_ragged_tables(in_size: int, out_size: int, first: int = 0, count: Optional[int] = None, ksize: Optional[int] = None,
                         device="cuda"):
    """``plipmi_resize_ragged_tables``: the table kernel of the ragged resize alone, one axis resampled from ``in_size`` to
    ``out_size`` pixels, outputs ``first .. first + count`` (default: all) -> (bounds int32 [count, 2], coef int32 [count, ksize]) on
    the device, to compare with ``preprocess.resample_coeffs(in_size, out_size)`` rows ``first .. first + count``."""
    lib = _lib.load()
    count = out_size - first if count is None else int(count)
    if ksize is None:
        scale = float(torch.tensor(in_size, dtype=torch.float32)) / out_size
        ksize = int(math.ceil(2.0 * max(scale, 1.0))) * 2 + 1
    dev = torch.device(device)
    bounds = torch.zeros((count, 2), dtype=torch.int32, device=dev)
    coef = torch.zeros((count, int(ksize)), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.plipmi_resize_ragged_tables(int(in_size), int(out_size), int(first), count, int(ksize), _ptr(bounds), _ptr(coef),
                                                   _stream_ptr(bounds.device)), "plipmi_resize_ragged_tables")
    return bounds, coef


# ---- the vision front end and the packed-row mechanisms (include/plipmi_test.h, tests/test_gpu_front_end.py) ---------------------------
# Every wrapper here writes into buffers the CALLER allocates (and may have pre-filled with a sentinel, with guard rows behind them):
# what a kernel leaves alone is part of what the tests check.
def patch_kpad(patch: int) -> int:
    """the patch rows' padded width: 3 * patch^2 rounded up to 64 (csrc/handle_host.h init_model)"""
    return (3 * patch * patch + 63) // 64 * 64


def unfold_patches(src: torch.Tensor, out: torch.Tensor, patch: int, kpad: int) -> torch.Tensor:
    """``plipmi_unfold_patches``: src fp32 [B, 3, H, W] or uint8 tiles [B, H, W, 3] -> rows 0 .. B * (H // patch) * (W // patch) - 1 of
    ``out`` [>= that many rows, kpad] (fp32 / bf16 / f16)."""
    lib = _lib.load()
    assert src.is_cuda and out.is_cuda and src.is_contiguous() and out.is_contiguous() and src.dim() == 4 and out.dim() == 2
    u8 = src.dtype == torch.uint8
    assert u8 or src.dtype == torch.float32
    B, H, W = (src.shape[0], src.shape[1], src.shape[2]) if u8 else (src.shape[0], src.shape[2], src.shape[3])
    assert src.shape[3 if u8 else 1] == 3 and out.shape[1] == kpad and out.shape[0] >= B * (H // patch) * (W // patch)
    with torch.cuda.device(src.device):
        _lib.check(lib.plipmi_unfold_patches(_code(out.dtype), int(u8), _ptr(src), _ptr(out), B, H, W, int(patch), int(kpad), _stream_ptr(src.device)),
                   "plipmi_unfold_patches")
    return out


def cls_rows(cls: torch.Tensor, pos: torch.Tensor, x: torch.Tensor, B: int, tokens: int) -> torch.Tensor:
    """``plipmi_cls_rows``: row 0 of each of the B images of x fp32 [>= B * tokens, D] = cls [D] + pos[0] (pos fp32 [>= 1, D])."""
    lib = _lib.load()
    _f32(cls, pos, x)
    D = cls.numel()
    assert pos.shape[-1] == D and x.dim() == 2 and x.shape[1] == D and x.shape[0] >= B * tokens
    with torch.cuda.device(x.device):
        _lib.check(lib.plipmi_cls_rows(_ptr(cls), _ptr(pos), _ptr(x), int(B), int(tokens), D, _stream_ptr(x.device)), "plipmi_cls_rows")
    return x


def gemm_patch(a: torch.Tensor, w: torch.Tensor, pos: torch.Tensor, out: torch.Tensor, K: Optional[int] = None, variant: int = -1) -> torch.Tensor:
    """``plipmi_gemm_patch`` (the EPI_PATCH epilogue): a [B * np, lda], w [N, ldw] (K <= lda, ldw columns used; default all of a's),
    pos fp32 [np + 1, N] -> token rows img * (np + 1) + 1 + p of ``out`` fp32 [>= B * (np + 1), N].  variant -3 = the small-M split-K
    kernel (bf16 / f16, N % 64 == 0, K % 256 == 0; anything else is refused before a launch)."""
    lib = _lib.load()
    assert a.is_cuda and w.is_cuda and a.dtype == w.dtype and a.is_contiguous() and w.is_contiguous()
    _f32(pos, out)
    M, N, np_ = a.shape[0], w.shape[0], pos.shape[0] - 1
    K = a.shape[1] if K is None else int(K)
    assert np_ >= 1 and M % np_ == 0 and pos.shape[1] == N and out.shape[1] == N and out.shape[0] >= M // np_ * (np_ + 1)
    with torch.cuda.device(a.device):
        _lib.check(lib.plipmi_gemm_patch(_code(a.dtype), int(variant), M, N, K, _ptr(a), a.shape[1], _ptr(w), w.shape[1], _ptr(pos), np_,
                                         _ptr(out), _stream_ptr(a.device)), "plipmi_gemm_patch")
    return out


def gemm_patch_gather(src: torch.Tensor, w: torch.Tensor, pos: torch.Tensor, out: torch.Tensor, patch: int) -> torch.Tensor:
    """``plipmi_gemm_patch_gather`` (im2col on load, the ring tile at any batch): src fp32 [B, 3, H, W] or uint8 [B, H, W, 3], w [N, 3 * patch^2]
    (bf16 / f16; fp32 is passed on to be refused), pos fp32 [np + 1, N] -> the token rows of ``out`` fp32 [>= B * (np + 1), N]."""
    lib = _lib.load()
    assert src.is_cuda and w.is_cuda and src.is_contiguous() and w.is_contiguous() and src.dim() == 4
    _f32(pos, out)
    u8 = src.dtype == torch.uint8
    assert u8 or src.dtype == torch.float32
    B, H, W = (src.shape[0], src.shape[1], src.shape[2]) if u8 else (src.shape[0], src.shape[2], src.shape[3])
    N = w.shape[0]
    assert out.shape[1] == N and pos.shape[1] == N and out.shape[0] >= B * pos.shape[0]
    with torch.cuda.device(src.device):
        _lib.check(lib.plipmi_gemm_patch_gather(_code(w.dtype), None if u8 else _ptr(src), _ptr(src) if u8 else None, _ptr(w), _ptr(pos),
                                                _ptr(out), B, H, W, int(patch), N, _stream_ptr(src.device)), "plipmi_gemm_patch_gather")
    return out


def gemm_nt_ln_rows(mode: int, a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, m_dev: torch.Tensor, out, st: Optional[torch.Tensor] = None,
                    stats: Optional[torch.Tensor] = None, M: Optional[int] = None, eps: float = 1e-5, variant: int = -1) -> None:
    """``plipmi_gemm_nt_ln_rows``: ``gemm_nt_ln`` on the first min(m_dev[0], M) rows of a grid sized for M rows (default a.shape[0]), into
    the caller's buffers: mode 0 / 1 ``out`` = C [>= M, N] (16-bit), modes 3 / 4 ``out`` = (hi [>= M, N], lo uint8) and ``st``
    fp32 [>= M, N // 64, 2].  m_dev int32 [1] on the device; None runs ``plipmi_gemm_nt_ln`` itself (the same call without it)."""
    lib = _lib.load()
    assert a.dtype in (torch.bfloat16, torch.float16) and w.dtype == a.dtype and a.is_contiguous() and w.is_contiguous() and mode in (0, 1, 3, 4)
    assert m_dev is None or (m_dev.is_cuda and m_dev.dtype == torch.int32 and m_dev.numel() == 1)
    M = a.shape[0] if M is None else int(M)
    K, N = a.shape[1], w.shape[0]
    assert a.shape[0] >= M
    if mode in (0, 1):
        assert out.dtype == a.dtype and out.is_contiguous() and out.shape[1] == N and out.shape[0] >= M and stats.is_contiguous() and stats.shape[0] >= M
        args = (_ptr(stats), stats.shape[1], float(eps), _ptr(out), None, None)
    else:
        hi, lo = out
        assert hi.dtype == a.dtype and hi.is_contiguous() and hi.shape[1] == N and hi.shape[0] >= M and lo.dtype == torch.uint8 and lo.is_contiguous()
        assert lo.numel() >= lo_plane_bytes(M, N) and st.is_contiguous() and st.shape[0] >= M and st.shape[1:] == (N // 64, 2)
        args = (None, 0, float(eps), _ptr(lo), _ptr(hi), _ptr(st))
    with torch.cuda.device(a.device):
        if m_dev is None:
            _lib.check(lib.plipmi_gemm_nt_ln(_code(a.dtype), mode, int(variant), M, N, K, _ptr(a), _ptr(w), _ptr(bias), *args, _stream_ptr(a.device)),
                       "plipmi_gemm_nt_ln")
        else:
            _lib.check(lib.plipmi_gemm_nt_ln_rows(_code(a.dtype), mode, int(variant), M, N, K, _ptr(a), _ptr(w), _ptr(bias), *args, _ptr(m_dev),
                                                  _stream_ptr(a.device)), "plipmi_gemm_nt_ln_rows")


def attention_packed(qkv: torch.Tensor, out: torch.Tensor, cu: torch.Tensor, S: int, H: int, causal: bool = False,
                     key_mask: Optional[torch.Tensor] = None, impl: int = 1) -> torch.Tensor:
    """``plipmi_attention_packed``: qkv [rows, 3 * H * 64] packed rows, cu int32 [B + 1] (caption b = rows cu[b] .. cu[b + 1] - 1, each
    1 .. S long), key_mask int64 [B, S] or None -> rows 0 .. cu[B] - 1 of ``out`` [>= cu[B], H * 64]."""
    lib = _lib.load()
    assert qkv.is_cuda and qkv.is_contiguous() and out.is_contiguous() and qkv.shape[1] == 3 * H * 64 and out.shape[1] == H * 64 and out.dtype == qkv.dtype
    assert cu.is_cuda and cu.dtype == torch.int32 and cu.dim() == 1
    B = cu.numel() - 1
    c = cu.cpu()
    ln = c[1:] - c[:-1]
    assert int(c[0]) == 0 and (B == 0 or (int(ln.min()) >= 1 and int(ln.max()) <= max(S, 1))) and int(c[-1]) <= min(qkv.shape[0], out.shape[0])
    assert key_mask is None or (key_mask.is_cuda and key_mask.dtype == torch.int64 and key_mask.is_contiguous() and key_mask.shape == (B, S))
    with torch.cuda.device(qkv.device):
        _lib.check(lib.plipmi_attention_packed(_code(qkv.dtype), int(impl), _ptr(qkv), _ptr(out), B, int(S), H, int(causal), _ptr(key_mask),
                                               _ptr(cu), _stream_ptr(qkv.device)), "plipmi_attention_packed")
    return out


def token_scores(E: torch.Tensor, T: torch.Tensor, scale: float = 1.0, softmax: bool = False, out: Optional[torch.Tensor] = None,
                 M: Optional[int] = None) -> torch.Tensor:
    """``plipmi_token_scores``: E fp32 [M, P], T fp32 [C, P] -> fp32 [M, C] = scale * cosine, or its softmax over C.  ``out``: a
    contiguous fp32 buffer of at least [M, C] whose first M rows are written (the tests put guard rows behind them); ``M``: fewer rows
    than E holds."""
    lib = _lib.load()
    assert E.is_cuda and T.is_cuda and E.dtype == T.dtype == torch.float32 and E.is_contiguous() and T.is_contiguous()
    assert E.dim() == 2 and T.dim() == 2 and E.shape[1] == T.shape[1]
    M = E.shape[0] if M is None else int(M)
    C, P = T.shape
    assert 0 <= M <= E.shape[0]
    if out is None:
        out = torch.empty((M, C), dtype=torch.float32, device=E.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= M * C
    with torch.cuda.device(E.device):
        _lib.check(lib.plipmi_token_scores(_ptr(E), M, int(P), _ptr(T), int(C), float(scale), int(bool(softmax)), _ptr(out),
                                           _stream_ptr(E.device)), "plipmi_token_scores")
    return out
