"""Kernel-level parity of the attention kernels at head sizes other than 64 (include/plipmi_test.h ``plipmi_attention_hd`` and the three
``_hd`` entries of the probabilities and their summaries; the padded-head kernels of csrc/attention.hip, attention_mfma.hip,
attention_probs.hip and attention_summary.hip).

The reference is the fp64 softmax(Q K^T) V of tests/test_gpu_attention.py with the head size as a parameter, q pre-scaled by
head^-0.5 * 3, and that file's tolerances unchanged: they come from the rounding of the outputs (and of P as an MFMA operand), not from
the head size.  Outputs are pre-filled with a sentinel: a head slot has exactly ``head`` columns, so a store that is too wide lands in
the neighbouring head and shows as a wrong value there, one that is too narrow leaves the sentinel.  One exact-integer case per padded
size proves the MFMA operand maps bit for bit.  The probabilities, pooled rows and rollout step use the bounds of
tests/test_gpu_small_kernels.py / tests/test_gpu_attention_summary.py for the head-64 kernels."""
import numpy as np
import pytest
import torch

import small_kernel_refs as R
from attention_summary_refs import rollout_bound, rollout_ref
from test_gpu_small_kernels import PROB_CAP, Checks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
HEADS = [72, 80, 88, 96, 104, 128]
H = 2
# (B, S, causal, mask): one token; an odd length below a key tile, causal + padding; the vision tower's 50; exactly one chunk; one key
# more than a chunk; 257 tokens (three chunks) under a mask; 300 causal + padding
SHAPES = [(2, 1, False, False), (2, 33, True, True), (3, 50, False, False), (1, 128, False, False), (2, 129, False, False),
          (2, 257, False, True), (2, 300, True, True)]
TOL = {"valu_f32": 2e-5, "valu_bf16": 2e-2, "mfma_bf16": 3e-2, "valu_f16": 2.5e-3, "mfma_f16": 4e-3}     # tests/test_gpu_attention.py
SENTINEL = 777.0


def _ref(qkv, B, S, heads, head, causal, mask):
    """tests/test_gpu_attention.py ``_ref`` with the head size as a parameter: float64 on the operands the kernel reads"""
    x = qkv.double().reshape(B, S, 3, heads, head)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2)
    neg = float("-inf")
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(S, S, dtype=torch.bool, device=qkv.device)), neg)
    if mask is not None:
        s = s.masked_fill(~mask.bool()[:, None, None, :], neg)
    return (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B * S, heads * head)


_INPUTS = {}


def _inputs(head, B, S, causal, use_mask):
    """fp32 qkv on the CPU, the key mask on the device, per (head, shape): drawn once, shared by the five modes, never changed"""
    key = (head, B, S, causal, use_mask)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * S + head)
        qkv = torch.randn(B * S, 3 * H * head, generator=g)
        qkv[:, : H * head] *= head ** -0.5 * 3.0          # q pre-scaled; x3 sharpens the softmax
        mask = None
        if use_mask:
            lens = torch.randint(1, S + 1, (B,), generator=g)
            mask = (torch.arange(S)[None, :] < lens[:, None]).long().to(DEV)
        _INPUTS[key] = (qkv, mask)
    return _INPUTS[key]


@pytest.mark.parametrize("B,S,causal,use_mask", SHAPES)
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("mode", list(TOL))
def test_attention_kernels_at_other_head_sizes(mode, head, B, S, causal, use_mask):
    from plip_amd.kernel_entries import attention
    qkv32, mask = _inputs(head, B, S, causal, use_mask)
    qkv = qkv32.to(DEV).to(DT[mode.split("_")[1]])
    out = torch.full((B * S, H * head), SENTINEL, dtype=qkv.dtype, device=DEV)
    attention(qkv, B, S, H, causal, mask, impl=1 if mode.startswith("mfma") else 0, head_dim=head, out=out)
    torch.cuda.synchronize()
    ref = _ref(qkv, B, S, H, head, causal, mask)
    assert torch.isfinite(out).all()
    err = (out.double() - ref).abs().max().item()        # |o| <~ 4: a sentinel left behind, or a neighbour overwritten, is far outside
    print(f"\nPARITY group=attention_head_dim case={mode}_hd{head}_B{B}_S{S}_causal{int(causal)}_mask{int(use_mask)} bound={TOL[mode]:.1e} gpu={err:.3e}")
    assert err < TOL[mode], f"{mode} head {head} B{B} S{S} causal={causal} mask={use_mask}: max err {err:.3e}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("head", [88, 96, 104, 128])          # both padded sizes, each with and without padding columns
def test_mfma_operand_maps_are_exact_on_integers(head, dtype):
    """Q = 4 K[t(i)] with K in {-1, +1}: the score of key t(i) is 4 head, every other one at least 100 below it (checked on the host
    below), so the softmax is one-hot in fp32 -- exp of -100 and less adds nothing to 1 and rounds to 0 as an operand -- and the
    output row of query i must be V[t(i)], an asymmetric table of small integers, BIT FOR BIT: any slip in the column maps of Q against
    K, in the key permutation of P against V^T, in the zero fill or in the output columns lands on another integer.  Causal with a
    padding mask; 300 tokens: three key chunks, targets in every chunk and in earlier chunks than the query's own."""
    from plip_amd.kernel_entries import attention
    B, S = 2, 300
    g = torch.Generator().manual_seed(head)
    k = (torch.randint(0, 2, (B, S, H, head), generator=g) * 2 - 1).double()
    lens = torch.tensor([S, 141])
    i = torch.arange(S)
    target = torch.stack([(i * 7 + 3 * b) % (i + 1) for b in range(B)])                  # t(i) <= i: visible under the causal mask
    target = torch.minimum(target, (lens - 1)[:, None])                                   # ... and inside the sample's valid keys
    q = 4.0 * torch.gather(k, 1, target[:, :, None, None].expand(B, S, H, head))
    j, d, h = torch.arange(S)[:, None, None], torch.arange(head)[None, None, :], torch.arange(H)[None, :, None]
    v = ((j * 7 + d * 3 + h * 5) % 13 - 6).double()[None].expand(B, S, H, head)         # [-6, 6]; V[j, d] != V[d, j], no period in j or d
    qkv = torch.stack((q, k, v), dim=2).reshape(B * S, 3 * H * head)
    mask = (i[None, :] < lens[:, None]).long()
    # the host's own check of the construction: the winner leads every other visible key by at least 100
    s = torch.einsum("bihd,bjhd->bhij", q, k)
    visible = (torch.tril(torch.ones(S, S, dtype=torch.bool))[None] & mask.bool()[:, None, :])[:, None]
    win = torch.gather(s, 3, target[:, None, :, None].expand(B, H, S, 1))
    assert (win == 4.0 * head).all()
    others = s.masked_fill(~visible, -1e9).scatter(3, target[:, None, :, None].expand(B, H, S, 1), -1e9)
    assert float((win - others.amax(-1, keepdim=True)).min()) >= 100.0
    want = torch.gather(v, 1, target[:, :, None, None].expand(B, S, H, head)).reshape(B * S, H * head).to(dtype)
    out = torch.full((B * S, H * head), SENTINEL, dtype=dtype, device=DEV)
    attention(qkv.to(dtype).to(DEV), B, S, H, True, mask.to(DEV), impl=1, head_dim=head, out=out)
    torch.cuda.synchronize()
    live = (i[None, :] < lens[:, None]).reshape(B * S)           # rows of masked QUERIES are don't-cares downstream
    assert torch.equal(out.cpu()[live], want[live])


def test_head_64_through_the_new_entry_is_the_old_kernel():
    from plip_amd.kernel_entries import attention
    g = torch.Generator().manual_seed(5)
    for S in (50, 257):
        qkv = torch.randn(2 * S, 3 * H * 64, generator=g).to(DEV).to(torch.bfloat16)
        for impl in (0, 1):
            assert torch.equal(attention(qkv, 2, S, H, impl=impl, head_dim=64), attention(qkv, 2, S, H, impl=impl))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("S,causal,lens", [(129, False, None), (300, True, (300, 141))], ids=["S129_plain", "S300_causal_mask"])
def test_padded_flash_kernel_is_the_head_64_chunked_kernel_on_a_zero_padded_head(S, causal, lens, dtype):
    """The two chunked MFMA kernels take one online-softmax step (csrc/attention_flash_step.inc) and perform the same operations in the
    same order per query.  A head-72 problem whose q and k columns 64 .. 71 are zeros is the head-64 problem: the extra k-step adds exact
    zeros to every score, and output tiles 0 and 1 read the same V columns (v columns 64 .. 71 are arbitrary: they only reach output
    columns 64 ..).  So columns 0 .. 63 of every head must be the head-64 kernel's output BIT FOR BIT.  S > 128: at or below it head 64
    takes the single-pass kernel, which is other arithmetic."""
    from plip_amd.kernel_entries import attention
    B = 2
    g = torch.Generator().manual_seed(64 * S)
    x64 = torch.randn(B * S, 3, H, 64, generator=g)
    x64[:, 0] *= 64 ** -0.5 * 3.0                       # q pre-scaled; x3 sharpens the softmax
    x72 = torch.zeros(B * S, 3, H, 72)
    x72[..., :64] = x64
    x72[:, 2, :, 64:] = torch.randn(B * S, H, 8, generator=g)
    mask = None if lens is None else (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long().to(DEV)
    o64 = attention(x64.reshape(B * S, 3 * H * 64).to(dtype).to(DEV), B, S, H, causal, mask, impl=1, head_dim=64)
    o72 = attention(x72.reshape(B * S, 3 * H * 72).to(dtype).to(DEV), B, S, H, causal, mask, impl=1, head_dim=72)
    torch.cuda.synchronize()
    assert torch.isfinite(o64).all()
    assert torch.equal(o72.reshape(B * S, H, 72)[..., :64], o64.reshape(B * S, H, 64))


@pytest.mark.parametrize("head", [32, 56, 100, 136, 192])
def test_entries_refuse_other_head_sizes_by_name(head):
    from plip_amd._lib import PlipmiError
    from plip_amd.kernel_entries import attention, attention_pooled_rows, attention_probs, attention_rollout_step
    qkv = torch.zeros(4, 3 * head, device=DEV, dtype=torch.bfloat16)
    rows = torch.zeros(1, dtype=torch.int32, device=DEV)
    for call in (lambda: attention(qkv, 1, 4, 1, impl=1, head_dim=head), lambda: attention(qkv, 1, 4, 1, impl=0, head_dim=head),
                 lambda: attention_probs(qkv, 1, 4, 1, head_dim=head), lambda: attention_pooled_rows(qkv, rows, 1, 4, 1, head_dim=head),
                 lambda: attention_rollout_step(qkv, None, 1, 4, 1, head_dim=head)):
        with pytest.raises(PlipmiError, match="head_dim"):
            call()


# ---- probabilities, pooled rows, rollout step ------------------------------------------------------------------------------------
def _probs_ref(qkv, B, S, heads, head, causal, mask, dtype=torch.float64):
    """tests/small_kernel_refs.py ``attention_probs`` with the head size as a parameter"""
    x = qkv.to(dtype).reshape(B, S, 3, heads, head)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
    live = R.live_keys(B, S, causal, mask)[:, None].expand(B, heads, S, S)
    zero = torch.zeros((), dtype=dtype)
    s = torch.where(live, q @ k.transpose(-1, -2), zero)
    m = torch.where(live, s, torch.full((), -torch.finfo(dtype).max, dtype=dtype)).amax(-1, keepdim=True)
    e = torch.where(live, torch.exp(torch.where(live, s - m, zero)), zero)
    den = e.sum(-1, keepdim=True)
    return torch.where(den > 0, e / torch.where(den > 0, den, torch.ones((), dtype=dtype)), zero)


@pytest.mark.parametrize("dname", list(DT))
@pytest.mark.parametrize("S", [17, 257])
@pytest.mark.parametrize("head", [80, 88])
def test_probabilities_pooled_rows_and_rollout_at_other_head_sizes(head, S, dname):
    from plip_amd.kernel_entries import attention_pooled_rows, attention_probs, attention_rollout_step
    B, heads = 3, 3
    ck = Checks()
    for kind in ("dense", "causal", "causal_mask"):
        causal = kind != "dense"
        mask = None
        if kind == "causal_mask":                   # sample 1: key 0 masked (its query row 0 has no live key); sample 2: a padded tail
            mask = torch.ones(B, S, dtype=torch.int64)
            mask[1, 0] = 0
            mask[2, S - 2:] = 0
        dmask = None if mask is None else mask.to(DEV)
        case = f"hd{head}_S{S}_{kind}"
        qkvs = []
        for n in range(2):
            q = torch.randn(B * S, 3 * heads * head, generator=torch.Generator().manual_seed(7919 * S + 31 * head + n))
            q[:, : heads * head] *= head ** -0.5 * 3.0
            qkvs.append(q.to(DT[dname]))
        probs = [attention_probs(q.to(DEV), B, S, heads, causal, dmask, head_dim=head) for q in qkvs]
        torch.cuda.synchronize()
        got = probs[0].cpu()
        live = R.live_keys(B, S, causal, mask)[:, None].expand(B, heads, S, S)
        assert (got[~live] == 0.0).all(), case
        has = live.any(-1)
        sums = got.double().sum(-1)[has]
        assert float((sums - 1.0).abs().max()) <= ((S + 63) // 64 + 10) * 2.0 ** -24, case        # tests/test_gpu_small_kernels.py
        ck.add("probs_head_dim_" + dname, case, got, _probs_ref(qkvs[0], B, S, heads, head, causal, mask),
               _probs_ref(qkvs[0], B, S, heads, head, causal, mask, torch.float32), cap=PROB_CAP[dname])
        # pooled rows: the same device code on a 1-row tile, the same bits
        rows = torch.tensor([S - 1, 0, S // 2], dtype=torch.int32, device=DEV)
        pooled = attention_pooled_rows(qkvs[0].to(DEV), rows, B, S, heads, causal, dmask, head_dim=head)
        assert torch.equal(pooled, probs[0][torch.arange(B, device=DEV), :, rows.long(), :]), case
        # rollout: one step from the identity and a second one, against float64 on the probabilities the probs kernel wrote
        r1 = attention_rollout_step(qkvs[0].to(DEV), None, B, S, heads, causal, dmask, head_dim=head)
        r2 = attention_rollout_step(qkvs[1].to(DEV), r1, B, S, heads, causal, dmask, head_dim=head)
        torch.cuda.synchronize()
        P = [p.cpu().numpy() for p in probs]
        for steps, r in ((1, r1), (2, r2)):
            err = float(np.abs(r.cpu().numpy().astype(np.float64) - rollout_ref(P[:steps])).max())
            print(f"\nPARITY group=rollout_head_dim case={case}_{dname} steps={steps} err={err:.3e} bound={rollout_bound(steps, S, heads):.3e}")
            assert err <= rollout_bound(steps, S, heads), (case, steps, err)
    ck.done()
