"""Shared by tests/test_small_kernel_refs_host.py, tests/test_gpu_small_kernels.py and tests/test_gpu_front_end.py (and tests/test_gpu_gemm.py
for ``slice_stats``): plain float64 torch restatements of the kernels around the GEMMs (plip_amd/csrc/tower_kernels.hip, head_kernels.hip, setup_kernels.hip, attention_probs.hip), written from
the operations' definitions and not from the kernels.  Each is checked on the CPU against an independent formulation
(torch.nn.functional, numpy, oracle/clip_oracle.py) by the host test; the GPU test compares the kernels with them.

Also here: the rule the GPU test takes its fp32 tolerances from (``fp32_bound``) and the sizes of one unit in the last place."""
import numpy as np
import torch

F64 = torch.float64


# ---- LayerNorm and its by-products --------------------------------------------------------------------------------------------------
def layer_norm(x, g, b, eps, dtype=F64):
    """nn.LayerNorm over the last axis (biased variance), two passes, in ``dtype`` (float64: the reference; float32: the plain
    unfused CPU form the tolerances are measured on)."""
    x, g, b = x.to(dtype), g.to(dtype), b.to(dtype)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def slice_stats(x, dtype=F64):
    """per-row partials over 64-column slices, fp32 [M, D // 64, 2]: {sum, centred M2} -- what the producers emit"""
    M, D = x.shape
    xs = x.to(dtype).reshape(M, D // 64, 64)
    s = xs.sum(-1)
    m2 = ((xs - s[..., None] / 64) ** 2).sum(-1)
    return torch.stack((s, m2), dim=-1).float().contiguous()


def fold_ln(W, bias, g, b, pre, dtype=F64):
    """LayerNorm folded into the Linear behind it: Wf = pre * (W * g, rows centred), c2 = pre * (W . b + bias)."""
    W, bias, g, b = W.to(dtype), bias.to(dtype), g.to(dtype), b.to(dtype)
    Wg = W * g[None, :]
    return pre * (Wg - Wg.mean(1, keepdim=True)), pre * (W @ b + bias)


# ---- attention probabilities ---------------------------------------------------------------------------------------------------------
def live_keys(B, S, causal, mask):
    """bool [B, S, S]: key j is visible to query i of sample b"""
    live = torch.ones(B, S, S, dtype=torch.bool)
    if causal:
        live &= torch.tril(torch.ones(S, S, dtype=torch.bool))[None]
    if mask is not None:
        live &= (mask != 0)[:, None, :]
    return live


def attention_probs(qkv, B, S, H, causal, mask, dtype=F64):
    """eager softmax(q k^T) over the live keys of qkv [B*S, 3*H*64] (q | k | v, scale folded into q) -> [B, H, S, S]; masked
    entries are exactly 0 and a row with no live key is all zeros.  Written with a multiplicative mask on exp(s - max over the
    live keys), not with an additive -inf."""
    x = qkv.to(dtype).reshape(B, S, 3, H, 64)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
    live = live_keys(B, S, causal, mask)[:, None].expand(B, H, S, S)
    s = torch.where(live, q @ k.transpose(-1, -2), torch.zeros((), dtype=dtype))   # dead keys may hold anything: never looked at
    big = torch.finfo(dtype).max
    m = torch.where(live, s, torch.full((), -big, dtype=dtype)).amax(-1, keepdim=True)
    e = torch.where(live, torch.exp(torch.where(live, s - m, torch.zeros((), dtype=dtype))), torch.zeros((), dtype=dtype))
    den = e.sum(-1, keepdim=True)
    return torch.where(den > 0, e / torch.where(den > 0, den, torch.ones((), dtype=dtype)), torch.zeros((), dtype=dtype))


# ---- embedding rows, EOS rules, pack plan, pooled head ---------------------------------------------------------------------------------
def embed_rows(ids, tok, pos, dtype=F64):
    """tok[ids[b, s]] + pos[s] -> [B * S, D]"""
    B, S = ids.shape
    rows = torch.stack([tok[int(i)].to(dtype) for i in ids.reshape(-1)]).reshape(B, S, -1)
    return (rows + pos[:S].to(dtype)[None]).reshape(B * S, -1)


def eos_positions(ids, eos_id):
    """the pooled row of each caption: eos_id == 2 or < 0 -> the first position holding the largest id; otherwise the first
    position holding eos_id, 0 when there is none.  Plain loops."""
    out = []
    for row in ids.tolist():
        if eos_id == 2 or eos_id < 0:
            want = max(row)
            out.append(next(s for s, v in enumerate(row) if v == want))
        else:
            out.append(next((s for s, v in enumerate(row) if v == eos_id), 0))
    return torch.tensor(out, dtype=torch.int64)


def pack_plan(ids, eos_id):
    """(len [B], cu [B + 1], rowmap [cu[B]]) int32: caption b keeps its rows 0 .. EOS; rowmap[r] = (b << 8) | s of packed row r"""
    ln = (eos_positions(ids, eos_id) + 1).tolist()
    cu, rowmap = [0], []
    for b, n in enumerate(ln):
        cu.append(cu[-1] + n)
        rowmap += [(b << 8) | s for s in range(n)]
    return torch.tensor(ln, dtype=torch.int32), torch.tensor(cu, dtype=torch.int32), torch.tensor(rowmap, dtype=torch.int32)


def pooled_head(x, ids, eos_id, ln_w, ln_b, eps, W=None, normalize=False, dtype=F64):
    """x [B, S, D]: the pooled row (row 0 without ids) -> LayerNorm [-> @ W [P, D]^T [-> / its L2 norm]]"""
    B = x.shape[0]
    pos = torch.zeros(B, dtype=torch.int64) if ids is None else eos_positions(ids, eos_id)
    y = layer_norm(x[torch.arange(B), pos], ln_w, ln_b, eps, dtype)
    if W is None:
        return y
    y = y @ W.to(dtype).T
    return y / torch.sqrt((y * y).sum(-1, keepdim=True)) if normalize else y


# ---- the vision front end: patch unfold, patch embedding, uint8 normalisation -----------------------------------------------------------
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def unfold_ref(px, P, kpad=None):
    """Conv2d(kernel = stride = P) as a re-index of px [B, 3, H, W]: row (b, gi, gj) of the floored (H // P) x (W // P) grid, column
    (c, u, v) = px[b, c, gi * P + u, gj * P + v] -- the order of conv.weight.reshape(out, -1) --, zeros in columns 3 P^2 .. kpad.
    Same dtype as px: nothing is computed."""
    B, C, H, W = px.shape
    gh, gw, K = H // P, W // P, C * P * P
    out = torch.zeros(B * gh * gw, K if kpad is None else kpad, dtype=px.dtype)
    for gi in range(gh):
        for gj in range(gw):
            cell = px[:, :, gi * P:(gi + 1) * P, gj * P:(gj + 1) * P].reshape(B, K)
            out[gi * gw + gj::gh * gw, :K] = cell                        # rows b * gh * gw + gi * gw + gj, b = 0 .. B - 1
    return out


def patch_embed_ref(px, w, P, pos, cls=None):
    """CLIPVisionEmbeddings in float64: conv2d(px [B, 3, H, W], w [N, 3 P^2] viewed [N, 3, P, P], stride P), flattened to token rows
    [B, np + 1, N] with pos [np + 1, N] added; row 0 of each image is cls + pos[0] (NaN without cls: rows the patch GEMM does not own).
    px and w are taken as given -- the caller passes the operands already rounded to the kernel's type."""
    N = w.shape[0]
    y = torch.nn.functional.conv2d(px.to(F64), w.to(F64).reshape(N, 3, P, P), stride=P)      # [B, N, gh, gw]
    y = y.flatten(2).transpose(1, 2) + pos.to(F64)[None, 1:]
    first = torch.full((N,), float("nan"), dtype=F64) if cls is None else cls.to(F64) + pos.to(F64)[0]
    return torch.cat((first[None, None].expand(y.shape[0], 1, N), y), dim=1)


def u8_norm_ref(tiles):
    """uint8 HWC tiles [B, H, W, 3] -> fp32 NCHW pixels, the reference transform's three fp32 roundings: (b / 255 - mean_c) * (1 / std_c)
    with 1 / std_c itself rounded to fp32 -- the mirror tests/test_host.py proves the one-fma form against."""
    b = tiles.numpy().astype(np.float32)
    mean = np.array(CLIP_MEAN, dtype=np.float32)
    istd = (np.float32(1.0) / np.array(CLIP_STD, dtype=np.float32)).astype(np.float32)
    x = (b / np.float32(255.0)).astype(np.float32)
    x = ((x - mean).astype(np.float32) * istd).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))


# ---- top-k, arg-max ------------------------------------------------------------------------------------------------------------------
def topk_stable(scores, k):
    """indices int64 [N, k] of each row's k largest scores, descending, equal scores in index order; NaN counts as -inf.
    A lexicographic sort on (-score, index): a total order, so nothing rests on a sort's stability."""
    sc = np.asarray(scores, dtype=np.float64).copy()
    sc[np.isnan(sc)] = -np.inf
    col = np.arange(sc.shape[1])
    out = np.empty((sc.shape[0], k), dtype=np.int64)
    for i, row in enumerate(sc):
        out[i] = np.lexsort((col, -row))[:k]
    return out


def first_argmax(x):
    """int64 [N]: the lowest index holding each row's maximum"""
    x = np.asarray(x, dtype=np.float64)
    return np.array([min(j for j in range(x.shape[1]) if row[j] == row.max()) for row in x], dtype=np.int64)


# ---- the engines' 16-bit roundings (tests/test_gpu_value_range.py) ------------------------------------------------------------------
def round_to(x64, dtype):
    """float64 -> what a kernel's store of that value holds, ONE rounding from float64:
    bf16: round to nearest even, overflow to inf, NaN stays NaN (torch's ``.to(bfloat16)`` of an fp32 value);
    f16:  clamp to +-65504 (so +-inf too), then round to nearest even with gradual underflow, NaN stays NaN -- the engine's saturating
          store (csrc/common.h from_f32<f16_t>).
    Neither goes through fp32 with a second nearest rounding: f16 is numpy's float64 -> float16 conversion (correctly rounded), bf16
    rounds float64 -> fp32 TO ODD first (truncate, set the last bit when inexact), after which the nearest-even step to 8 bits
    rounds the original value."""
    x = np.asarray(x64.detach().cpu().to(F64).numpy())
    if dtype == torch.float32:
        return torch.from_numpy(x.astype(np.float32))
    if dtype == torch.float16:
        with np.errstate(invalid="ignore"):
            return torch.from_numpy(np.clip(x, -65504.0, 65504.0).astype(np.float16))        # np.clip keeps NaN
    assert dtype == torch.bfloat16
    nan = np.isnan(x)
    xs = np.where(nan, 0.0, x)
    with np.errstate(over="ignore"):
        f = xs.astype(np.float32)                                                             # nearest; may be one step past xs
    away = np.abs(f.astype(np.float64)) > np.abs(xs)
    t = np.where(away, np.nextafter(f, np.float32(0)), f).astype(np.float32)                  # truncated towards zero (inf -> max)
    inexact = t.astype(np.float64) != xs
    bits = t.view(np.uint32) | inexact.astype(np.uint32)                                      # round to odd
    out = torch.from_numpy(bits.view(np.float32).copy()).to(torch.bfloat16)                   # nearest even, overflow -> inf
    out[torch.from_numpy(nan)] = float("nan")
    return out


def ord16(t):
    """the bit patterns of a 16-bit float tensor as int32 ordinals that grow with the value (-0 and +0 both 0): the difference of two
    is their distance in units in the last place"""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def quick_gelu(x):
    """x * sigmoid(1.702 x) (transformers/activations.py QuickGELUActivation)"""
    return x * torch.sigmoid(1.702 * x)


# ---- tolerances ----------------------------------------------------------------------------------------------------------------------
def ulp32(v):
    """one fp32 unit in the last place at magnitude v (a float)"""
    return float(np.spacing(np.float32(abs(v)))) if v != 0 else float(np.spacing(np.float32(0)))


def ulp16(ref, dtype):
    """one unit in the last place of the 16-bit type at each element of ``ref`` (float64 tensor), as the relative figure 2^-8 (bf16) /
    2^-11 (f16) of the value -- the spacing of its binade is between that and twice that --, never below the type's smallest spacing"""
    if dtype == torch.bfloat16:
        return (ref.abs() * 2.0 ** -8).clamp(min=2.0 ** -133)
    return (ref.abs() * 2.0 ** -11).clamp(min=2.0 ** -24)


def fp32_bound(cpu32, ref64, cap=None):
    """The tolerance of an fp32 result on random data: 4 x the error of the plain fp32 CPU computation of the same inputs against the
    float64 reference (the kernels sum in another order and use expf / 1/sqrtf where torch rounds correctly), never below one fp32
    ulp of the largest reference magnitude, never above ``cap``.  Returns (bound, measured cpu error)."""
    err = float((cpu32.to(F64) - ref64).abs().max()) if ref64.numel() else 0.0
    bound = max(4.0 * err, ulp32(float(ref64.abs().max()) if ref64.numel() else 0.0))
    return (min(bound, cap) if cap is not None else bound), err
