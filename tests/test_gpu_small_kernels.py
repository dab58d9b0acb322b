"""Kernel-level fp64 parity of the kernels AROUND the GEMMs on the MI355X, one kernel at a time through include/plipmi_test.h
(plip_amd/kernel_entries.py) and the evaluation heads of include/plipmi.h: attention probabilities, the LayerNorm family, the
LayerNorm weight fold, token + position embedding with its planes and statistics, caption packing, the pooled rows and heads, the
fp32 head GEMM, logits, arg-max, top-k and L2 normalisation.

References: tests/small_kernel_refs.py (float64, pinned on the CPU by tests/test_small_kernel_refs_host.py).  Inputs are seeded
on the CPU; where a kernel reads 16-bit operands the reference starts from the same rounded operands.

Tolerances are not tuned to the kernels.  An fp32 result on random data must stay within 4 x the error the plain, unfused fp32
CPU computation of the SAME inputs makes against float64 -- the largest such error over all inputs of the test (``Checks``) --,
floored at one fp32 ulp of the largest reference magnitude and capped where an existing test already sets a figure (1e-5 / 5e-3 on
probabilities, 1e-3 / 1e-4 on the statistics partials).  A 16-bit output adds one unit in the last place of its type (2^-8 bf16 /
2^-11 f16 relative).  Integer-valued inputs make the GEMM / logits / top-k checks exact.  Every test prints ``PARITY`` lines
{cpu32 error, bound, MI355X error}; profiles/small_kernels_parity.txt keeps one line per group."""
import ctypes as C

import numpy as np
import pytest
import torch

import small_kernel_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
PLANE_REL = {torch.bfloat16: 2.0 ** -15, torch.float16: 2.0 ** -18}      # test_split_plane_residual_epilogue's format bound


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _parity(group, case, cpu_err, bound, gpu_err):
    print(f"\nPARITY group={group} case={case} cpu32={cpu_err:.3e} bound={bound:.3e} gpu={gpu_err:.3e}")


class Checks:
    """The fp32 checks of ONE test: ``add`` records {kernel result, float64 reference, fp32 CPU result} per case, ``done`` asserts them
    all against one bound per group -- small_kernel_refs.fp32_bound over ALL of the test's inputs (4 x the largest CPU-fp32 error on
    any of them, floored at one fp32 ulp of the largest reference magnitude).  Pooling matters for the cases with a single row: there
    the CPU's error on the one large element is a draw from 0 .. 1 ulp, and 4 x a lucky draw is no bound for anything."""

    def __init__(self):
        self.items = {}

    def add(self, group, case, got, ref64, cpu32, cap=None, extra=None):
        diff = (got.detach().cpu().to(torch.float64) - ref64).abs()
        assert torch.isfinite(diff).all(), (group, case)
        if extra is not None:
            diff = (diff - extra).clamp(min=0.0)                          # what is left after the 16-bit output's own rounding
        cpu_err = float((cpu32.to(torch.float64) - ref64).abs().max()) if ref64.numel() else 0.0
        self.items.setdefault(group, []).append((case, float(diff.max()) if diff.numel() else 0.0, cpu_err,
                                                 float(ref64.abs().max()) if ref64.numel() else 0.0, cap))

    def done(self):
        for group, rows in self.items.items():
            cpu_err = max(r[2] for r in rows)
            bound = max(4.0 * cpu_err, R.ulp32(max(r[3] for r in rows)))
            if rows[0][4] is not None:
                bound = min(bound, rows[0][4])
            case, gpu_err = max(((r[0], r[1]) for r in rows), key=lambda t: t[1])
            _parity(group, f"{len(rows)}_cases_worst_{case}", cpu_err, bound, gpu_err)
            assert gpu_err <= bound, (group, case, gpu_err, bound)


@pytest.fixture(scope="module")
def heads():
    from plip_amd.engine import heads_engine
    return heads_engine(DEV)


# =====================================================================================================================================
# attention probabilities (csrc/attention_probs.hip)
# =====================================================================================================================================
PROB_S = [1, 15, 16, 17, 64, 65, 77, 255, 256, 257, 577, 1000, 1024]
PROB_CAP = {"f32": 1e-5, "bf16": 5e-3, "f16": 5e-3}                       # tests/test_gpu_tower_outputs.py


def _qkv(B, S, H, seed, dtype):
    qkv = torch.randn(B * S, 3 * H * 64, generator=_gen(seed))
    qkv[:, : H * 64] *= 0.125 * 3.0                                      # q pre-scaled; x3 sharpens the softmax (test_gpu_attention.py)
    return qkv.to(dtype)                                                  # the rounded operands the kernel AND the reference read


def _check_probs(ck, case, qkv, B, S, H, causal, mask, dname):
    from plip_amd.kernel_entries import attention_probs
    got = attention_probs(qkv.to(DEV), B, S, H, causal, None if mask is None else mask.to(DEV))
    torch.cuda.synchronize()
    got = got.cpu()
    ref = R.attention_probs(qkv, B, S, H, causal, mask)
    cpu = R.attention_probs(qkv, B, S, H, causal, mask, torch.float32)
    live = R.live_keys(B, S, causal, mask)[:, None].expand(B, H, S, S)
    assert (got[~live] == 0.0).all(), case                                # masked entries are exact zeros (never -0.0 / NaN / denormal)
    has = live.any(-1)
    assert (got[~has] == 0.0).all(), case                                 # a row with no live key: zeros everywhere
    # live rows sum to 1.  Roundings between the exponentials and the stored row: ceil(S / 64) adds per lane + 6 for the wave
    # reduction (all in the common factor 1 / sum), the reciprocal, the product and expf (<= 2 ulp): (ceil(S/64) + 10) * 2^-24
    sums = got.double().sum(-1)[has]
    sum_tol = ((S + 63) // 64 + 10) * 2.0 ** -24
    sum_err = float((sums - 1.0).abs().max()) if sums.numel() else 0.0
    print(f"\nPARITY group=probs_rowsum case={case} cpu32={float((cpu.double().sum(-1)[has] - 1).abs().max()) if sums.numel() else 0.0:.3e} "
          f"bound={sum_tol:.3e} gpu={sum_err:.3e}")
    assert sum_err <= sum_tol, (case, sum_err, sum_tol)
    ck.add("probs_" + dname, case, got, ref, cpu, cap=PROB_CAP[dname])
    return got


@pytest.mark.parametrize("masking", ["dense", "causal", "causal_mask"])
@pytest.mark.parametrize("dname", list(DT))
@pytest.mark.parametrize("S", PROB_S)
def test_attention_probs(S, dname, masking):
    """every S around the kernel's borders (16-row blocks, 64 lanes, 256 threads, the 64 KiB LDS attribute at S > 960), H in {1, 3},
    B in {1, 2}; dense (vision), causal (text), causal + a right-padded key mask"""
    ck = Checks()
    for H, B in [(1, 1), (3, 2), (1, 2), (3, 1)]:
        qkv = _qkv(B, S, H, 1000 * S + 10 * H + B, DT[dname])
        mask = None
        if masking == "causal_mask":
            lens = torch.randint(1, S + 1, (B,), generator=_gen(S + B))
            mask = (torch.arange(S)[None, :] < lens[:, None]).long()
        _check_probs(ck, f"S{S}_H{H}_B{B}_{masking}", qkv, B, S, H, masking != "dense", mask, dname)
    ck.done()


@pytest.mark.parametrize("dname", list(DT))
@pytest.mark.parametrize("S", [17, 77, 257, 1000])
@pytest.mark.parametrize("kind", ["holes_causal", "holes_dense", "key0_dead", "sample_empty"])
def test_attention_probs_masks_with_dead_keys_and_dead_rows(kind, S, dname):
    """a live key after a dead one; key 0 dead under the causal rule (row 0 and every row up to the first live key have NO live key
    and must be 0.0 everywhere); a sample whose mask is all zero"""
    B, H = 2, 3
    g0 = _gen(7 * S)
    qkv = _qkv(B, S, H, 31 * S, DT[dname])
    causal = kind != "holes_dense"
    if kind.startswith("holes"):
        mask = (torch.rand(B, S, generator=g0) < 0.6).long()
        if S > 8:
            mask[:, 3], mask[:, 4] = 0, 1
            mask[0, S - 1], mask[1, S - 2], mask[1, S - 1] = 1, 0, 1
    elif kind == "key0_dead":
        mask = torch.ones(B, S, dtype=torch.long)
        first = min(S - 1, 20)                                            # past the first 16-row block where S allows
        mask[0, :first] = 0
        mask[1, 0] = 0
    else:
        mask = torch.ones(B, S, dtype=torch.long)
        mask[1] = 0
    ck = Checks()
    got = _check_probs(ck, f"S{S}_{kind}", qkv, B, S, H, causal, mask, dname)
    ck.done()
    if kind == "key0_dead":
        assert (got[0, :, :first] == 0.0).all() and (got[1, :, 0] == 0.0).all()
        assert (got[0, :, first:].sum(-1) > 0.99).all()
    if kind == "sample_empty":
        assert (got[1] == 0.0).all() and (got[0].sum(-1) > 0.99).all()


@pytest.mark.parametrize("dname", list(DT))
@pytest.mark.parametrize("S,causal", [(77, True), (300, False), (1000, True)])
def test_attention_probs_never_read_dead_key_rows(S, causal, dname):
    """large finite values (3e4) in the dead key rows: the live entries are the same BITS as with ordinary values there"""
    from plip_amd.kernel_entries import attention_probs
    B, H = 2, 2
    qkv = _qkv(B, S, H, 5 * S, DT[dname])
    mask = torch.ones(B, S, dtype=torch.long)
    mask[:, S // 2:] = 0
    mask[1, 2] = 0                                                        # and a hole
    loud = qkv.clone().view(B, S, 3, H * 64)
    loud[:, :, 1][mask == 0] = 3.0e4
    want = attention_probs(qkv.to(DEV), B, S, H, causal, mask.to(DEV))
    got = attention_probs(loud.view(B * S, -1).to(DEV), B, S, H, causal, mask.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    live = R.live_keys(B, S, causal, mask)[:, None].expand(B, H, S, S)
    assert (got.cpu()[~live] == 0.0).all() and torch.isfinite(got).all()


# =====================================================================================================================================
# LayerNorm family (csrc/tower_kernels.hip)
# =====================================================================================================================================
LN_D = [4, 64, 128, 252, 384, 512, 640, 768, 1024, 1280, 1664, 2048]
LN_ROWS = [1, 2, 3, 7, 8, 9, 1001]
EPS = 1e-5


def _ln_inputs(rows, D, seed):
    """rows as in test_layernorm_folded_consumer_epilogue: a common offset and one outlier channel, so that a one-pass variance would
    lose digits"""
    g0 = _gen(seed)
    x = torch.randn(rows, D, generator=g0) + 1.5
    x[:, min(5, D - 1)] += 60.0
    return x, torch.randn(D, generator=g0) * 0.5 + 1.0, torch.randn(D, generator=g0)


@pytest.mark.parametrize("oname", list(DT))
@pytest.mark.parametrize("D", LN_D)
def test_layernorm(D, oname):
    """layernorm_kernel (any D % 4 == 0 up to 2048) and layernorm_fixed_kernel (16-bit outputs at 512 / 768 / 1024: two rows per
    wave, odd row counts run the clamped second row), contiguous rows and rows picked out of a three times wider buffer"""
    from plip_amd.kernel_entries import layernorm
    odt = DT[oname]
    ck = Checks()
    for rows in LN_ROWS:
        x, g, b = _ln_inputs(rows, D, 100 * D + rows)
        ref = R.layer_norm(x, g, b, EPS)
        cpu = R.layer_norm(x, g, b, EPS, torch.float32)
        extra = None if odt == torch.float32 else R.ulp16(ref, odt)
        wide = torch.full((rows, 3 * D), 777.0)
        wide[:, D:2 * D] = x
        wide_d = wide.to(DEV)
        for tag, xin in (("dense", x.to(DEV)), ("strided", wide_d[:, D:2 * D])):
            y = layernorm(xin, g.to(DEV), b.to(DEV), EPS, odt)
            torch.cuda.synchronize()
            assert y.shape == (rows, D) and y.dtype == odt
            ck.add(f"layernorm_{oname}", f"D{D}_rows{rows}_{tag}", y, ref, cpu, extra=extra)
        assert torch.equal(wide_d.cpu(), wide)                            # the input is only read
    ck.done()


@pytest.mark.parametrize("D", LN_D)
def test_layernorm_in_place_fp32(D):
    """y == x (the vision tower's pre-LayerNorm on the fp32 engine), the fixed-kernel widths included"""
    from plip_amd.kernel_entries import layernorm
    ck = Checks()
    for rows in (1, 9, 1001):
        x, g, b = _ln_inputs(rows, D, 200 * D + rows)
        xd = x.to(DEV)
        y = layernorm(xd, g.to(DEV), b.to(DEV), EPS, inplace=True)
        torch.cuda.synchronize()
        assert y.data_ptr() == xd.data_ptr()
        ck.add("layernorm_inplace", f"D{D}_rows{rows}", y, R.layer_norm(x, g, b, EPS), R.layer_norm(x, g, b, EPS, torch.float32))
    ck.done()


@pytest.mark.parametrize("oname", list(DT))
@pytest.mark.parametrize("D", [4, 252, 512, 768, 1024, 2048])
def test_layernorm_of_a_constant_row_is_beta(D, oname):
    """variance 0: rstd = eps^-1/2 (finite only because of eps) times an exactly zero numerator -- the output is beta.  3.25 * D is
    exact in fp32, so the mean is exactly 3.25 whatever the summation order."""
    from plip_amd.kernel_entries import layernorm, layernorm_emit
    odt = DT[oname]
    g0 = _gen(D)
    g, b = torch.randn(D, generator=g0), torch.randn(D, generator=g0)
    for rows in (1, 3, 8):
        x = torch.randn(rows, D, generator=g0)
        x[rows - 1] = 3.25                                               # the LAST row: the one the fixed kernel's clamp re-reads
        y = layernorm(x.to(DEV), g.to(DEV), b.to(DEV), EPS, odt)
        torch.cuda.synchronize()
        assert torch.isfinite(y).all()
        assert torch.equal(y[rows - 1].cpu(), b.to(odt)), (D, rows)
        if D % 64 == 0 and odt != torch.float32:
            from plip_amd.kernel_entries import join_planes
            hi, lo, st = layernorm_emit(x.to(DEV), g.to(DEV), b.to(DEV), odt, EPS)
            torch.cuda.synchronize()
            assert torch.isfinite(st).all()
            bq = b[None, :].to(DEV)
            assert ((join_planes(hi, lo)[rows - 1:] - bq).abs() <= bq.abs() * PLANE_REL[odt] + 2.0 ** -32).all()


def _check_stats(ck, group, case, st, y_ref64, y_cpu32):
    """the statistics partials {sum, centred M2} per 64 columns describe the fp32 rows BEFORE they are split: against slice_stats of
    the float64 result.  Bounds from the fp32 CPU partials of the fp32 CPU rows, never looser than the producer-epilogue test's
    (1e-3 absolute on the sums, 1e-4 relative on M2, M2 clamped at 1e-3)."""
    want = R.slice_stats(y_ref64).double()
    cpu = R.slice_stats(y_cpu32, torch.float32).double()
    st = st.detach().cpu().double()
    assert st.shape == want.shape and torch.isfinite(st).all(), (group, case)
    ck.add(group + "_sum", case, st[..., 0], want[..., 0], cpu[..., 0], cap=1e-3)
    # M2 relative to the reference (clamped at 1e-3): the same rule on the scaled quantity, its floor one fp32 ulp of 1
    den = want[..., 1].clamp(min=1e-3)
    ck.add(group + "_m2rel", case, st[..., 1] / den, want[..., 1] / den, cpu[..., 1] / den, cap=1e-4)


def _check_planes(ck, group, case, hi, lo, y_ref64, y_cpu32, hdt):
    """joined planes within the format's bound of the float64 rows (+ the fp32 allowance)"""
    from plip_amd.kernel_entries import join_planes
    ck.add(group, case, join_planes(hi, lo), y_ref64, y_cpu32, extra=y_ref64.abs() * PLANE_REL[hdt] + 2.0 ** -32)


@pytest.mark.parametrize("hname", list(HALF))
@pytest.mark.parametrize("D", [d for d in LN_D if d % 64 == 0])
def test_layernorm_emit(D, hname):
    from plip_amd.kernel_entries import layernorm_emit
    hdt = HALF[hname]
    ck = Checks()
    for rows in LN_ROWS:
        x, g, b = _ln_inputs(rows, D, 300 * D + rows)
        ref = R.layer_norm(x, g, b, EPS)
        cpu = R.layer_norm(x, g, b, EPS, torch.float32)
        hi, lo, st = layernorm_emit(x.to(DEV), g.to(DEV), b.to(DEV), hdt, EPS)
        torch.cuda.synchronize()
        case = f"D{D}_rows{rows}"
        _check_planes(ck, f"ln_emit_{hname}", case, hi, lo, ref, cpu, hdt)
        _check_stats(ck, f"ln_emit_{hname}", case, st, ref, cpu)
    ck.done()


@pytest.mark.parametrize("hname", list(HALF))
@pytest.mark.parametrize("D", [d for d in LN_D if d % 64 == 0])
def test_layernorm_emit_hi_plane_is_self_consistent(D, hname):
    """hi equals the hi that split_planes(join_planes(hi, lo)) gives: the format is self-consistent.  (This test found the f16 split
    non-idempotent while its remainder was clamped to [-128, 127]: hi - 128 units is exactly the midpoint of two f16 neighbours, and
    the re-split rounded that tie to the other one -- 9.0e-4 of N(0, 2) values on the host mirror alone, 1 .. 3 elements per case
    here.  csrc/common.h split_f32<f16> and kernel_entries.split_planes now clamp to [-127, 127].)"""
    from plip_amd.kernel_entries import join_planes, layernorm_emit, split_planes
    hdt = HALF[hname]
    for rows in LN_ROWS:
        x, g, b = _ln_inputs(rows, D, 300 * D + rows)
        hi, lo, st = layernorm_emit(x.to(DEV), g.to(DEV), b.to(DEV), hdt, EPS)
        hi2, lo2 = split_planes(join_planes(hi, lo), hdt)
        torch.cuda.synchronize()
        moved = int((hi2.view(torch.int16) != hi.view(torch.int16)).sum())
        print(f"\nPARITY group=ln_emit_{hname}_hi_moved case=D{D}_rows{rows} cpu32=nan bound=0 gpu={moved}")
        assert moved == 0, (D, rows, moved, hi.numel())


# =====================================================================================================================================
# fold_ln: the device fold every 16-bit engine's weights come from
# =====================================================================================================================================
@pytest.mark.parametrize("pre", [1.0, 0.125])
@pytest.mark.parametrize("hname", list(HALF))
@pytest.mark.parametrize("K", [64, 260, 768, 1024, 3072])
def test_fold_ln(K, hname, pre):
    from plip_amd.kernel_entries import fold_ln, gemm_nt_ln
    hdt = HALF[hname]
    ck = Checks()
    for rows in (1, 5, 770):
        g0 = _gen(1000 * K + rows)
        W = torch.randn(rows, K, generator=g0) / K ** 0.5
        bias = torch.randn(rows, generator=g0) * 0.1
        gain = torch.exp(torch.empty(K).uniform_(-2.3, 2.3, generator=g0))
        beta = torch.randn(K, generator=g0)
        Wf, c2 = fold_ln(W.to(DEV), bias.to(DEV), gain.to(DEV), beta.to(DEV), hdt, pre)
        torch.cuda.synchronize()
        ref_w, ref_c = R.fold_ln(W, bias, gain, beta, pre)
        cpu_w, _ = R.fold_ln(W, bias, gain, beta, pre, torch.float32)
        case = f"K{K}_rows{rows}_pre{pre}"
        # one unit in the last place of the output type at the reference's magnitude, plus the fp32 allowance
        ck.add(f"fold_ln_{hname}", case, Wf, ref_w, cpu_w, extra=R.ulp16(ref_w, hdt))
        # centred rows: each entry is off by at most half an ulp of the largest entry's binade
        wf64 = Wf.cpu().double()
        big = wf64.abs().amax(1)
        half_ulp = 0.5 * 2.0 ** (torch.floor(torch.log2(big.clamp(min=2.0 ** -126))) - (7 if hdt == torch.bfloat16 else 10))
        assert (wf64.sum(1).abs() <= K * half_ulp).all(), case
        rel = float(((c2.cpu().double() - ref_c).abs() / ref_c.abs().clamp(min=1e-300)).max())
        print(f"\nPARITY group=fold_ln_c2 case={case}_{hname} cpu32=nan bound=1.000e-06 gpu={rel:.3e}")
        assert rel <= 1e-6, (case, rel)
        if rows == 770 and K % 128 == 0:                                  # the folded epilogue reads the partials in pairs: widths of 128 k
            # ... and the folded weights DO what they are for: gemm_nt_ln(mode 0) reproduces textbook LayerNorm -> Linear within
            # test_layernorm_folded_consumer_epilogue's second bound
            M, N = 77, 768
            x = torch.randn(M, K, generator=g0) + 1.5
            x[:, 5] += 60.0
            y = gemm_nt_ln(0, x.to(DEV).to(hdt), Wf[:N].contiguous(), c2[:N].contiguous(), R.slice_stats(x).to(DEV), eps=EPS)
            torch.cuda.synchronize()
            book = pre * (R.layer_norm(x, gain, beta, EPS) @ W[:N].double().T + bias[:N].double())
            err = float((y.cpu().double() - book).abs().max())
            tol = (4e-2 if hdt == torch.bfloat16 else 6e-3) * max(1.0, float(book.abs().max()))
            print(f"\nPARITY group=fold_ln_gemm case={case}_{hname} cpu32=nan bound={tol:.3e} gpu={err:.3e}")
            assert err < tol, (case, err, tol)
    ck.done()


# =====================================================================================================================================
# token + position embedding, caption packing, pooled rows
# =====================================================================================================================================
VOCAB = 300
EMB_S = [5, 77, 129, 256]
EMB_B = [1, 3, 64, 65, 200]
EMB_D = [128, 512, 768]


def _captions(B, S, seed):
    """EOS (VOCAB - 1) at position 0 / at the last position / absent (pools row 0: packed length 1) / twice (the first counts) /
    absent with the largest id twice; every other caption has it somewhere.  B == 1 takes the kind from S."""
    g0 = _gen(seed)
    ids = torch.randint(3, 250, (B, S), generator=g0)
    for b in range(B):
        kind = (b + (S if B == 1 else 0)) % 8
        if kind == 0:
            ids[b, 0] = VOCAB - 1
        elif kind == 1:
            ids[b, S - 1] = VOCAB - 1
        elif kind == 2:
            pass
        elif kind == 3:
            ids[b, 2] = ids[b, S - 2] = VOCAB - 1
        elif kind == 4:
            ids[b, 1] = ids[b, 3] = 260
        else:
            ids[b, int(torch.randint(0, S, (1,), generator=g0))] = VOCAB - 1
    return ids


def _emb_cases():
    out = []
    for i, S in enumerate(EMB_S):
        for j, B in enumerate(EMB_B):
            D = EMB_D[(i + j) % 3]
            if B * S * D > (1 << 22):                                     # the big batches at the narrow width: every S, B and D still occurs
                D = 128
            out.append((S, B, D))
    return out


def _eq_planes(hi, lo, want_hi, want_lo, rows, D):
    from plip_amd.kernel_entries import lo_plane_values
    return torch.equal(hi[:rows].view(torch.int16), want_hi[:rows].view(torch.int16)) and \
        torch.equal(lo_plane_values(lo, rows, D), lo_plane_values(want_lo, rows, D))


@pytest.mark.parametrize("hname", list(HALF))
@pytest.mark.parametrize("S,B,D", _emb_cases())
def test_text_embed_pack_and_pool_gather(S, B, D, hname):
    """rows = tok[id] + pos[s]: ONE fp32 add, so the planes equal the host split of the CPU fp32 sum bit for bit; the packed rows are
    those rows picked by the reference row map; cu / rowmap / m equal the reference plan (the scan carries across 64-caption
    chunks); pool_gather returns the pooled rows bit for bit, with and without cu"""
    from plip_amd.kernel_entries import join_planes, pool_gather, split_planes, text_embed_emit
    hdt = HALF[hname]
    g0 = _gen(S * 1000 + B)
    ids = _captions(B, S, S * 1000 + B)
    tok = torch.randn(VOCAB, D, generator=g0) * 0.7
    pos = torch.randn(S, D, generator=g0) * 0.3 + 0.1
    x32 = R.embed_rows(ids, tok, pos, torch.float32)                      # the same single fp32 add
    x64 = R.embed_rows(ids, tok, pos)
    want_hi, want_lo = split_planes(x32, hdt)
    ids_d, tok_d, pos_d = ids.to(DEV), tok.to(DEV), pos.to(DEV)
    hi, lo, st = text_embed_emit(ids_d, tok_d, pos_d, hdt)
    torch.cuda.synchronize()
    case = f"S{S}_B{B}_D{D}"
    assert _eq_planes(hi.cpu(), lo.cpu(), want_hi, want_lo, B * S, D), case
    ck = Checks()
    _check_stats(ck, f"embed_{hname}", case, st, x64, x32)
    ck.done()
    att = torch.randn(B * S, D, generator=g0).to(hdt)
    xq = join_planes(want_hi, want_lo)                                    # the fp32 value the planes stand for
    for eos_id in (VOCAB - 1, 2, -1):
        ln, cu, rowmap = R.pack_plan(ids, eos_id)
        m = int(cu[-1])
        if eos_id == VOCAB - 1 and B >= 5:
            assert ln[2] == 1 and ln[0] == 1 and ln[1] == S and ln[3] == 3           # no EOS -> 1; first; last; the first of two
        hp, lp, sp, cu_g, rowmap_g, m_g = text_embed_emit(ids_d, tok_d, pos_d, hdt, packed=True, eos_id=eos_id)
        torch.cuda.synchronize()
        assert int(m_g.item()) == m and torch.equal(cu_g.cpu(), cu) and torch.equal(rowmap_g.cpu()[:m], rowmap), (case, eos_id)
        sel = (rowmap.long() >> 8) * S + (rowmap.long() & 255)
        ph, pl = split_planes(x32[sel], hdt)
        assert _eq_planes(hp.cpu(), lp.cpu(), ph, pl, m, D), (case, eos_id)
        assert torch.equal(sp.cpu()[:m].view(torch.int32), st.cpu()[sel].view(torch.int32)), (case, eos_id)   # same rows, same partials
        # pooled rows: the [B, S] form picks by the EOS rule, the packed form takes each caption's last packed row
        rows_ref = torch.arange(B) * S + R.eos_positions(ids, eos_id)
        attp, xp = pool_gather(att.to(DEV), hi, lo, B, S, ids_d, eos_id)
        att_p = torch.zeros_like(att)
        att_p[:m] = att[sel]
        attp2, xp2 = pool_gather(att_p.to(DEV), hp, lp, B, S, ids_d, eos_id, cu=cu.to(DEV))      # the REFERENCE plan, not the kernel's
        torch.cuda.synchronize()
        for a, x in ((attp, xp), (attp2, xp2)):
            assert torch.equal(a.cpu().view(torch.int16), att[rows_ref].view(torch.int16)), (case, eos_id)
            assert torch.equal(x.cpu().view(torch.int32), xq[rows_ref].view(torch.int32)), (case, eos_id)
    attp, xp = pool_gather(att.to(DEV), hi, lo, B, S)                     # vision: the CLS row
    torch.cuda.synchronize()
    assert torch.equal(attp.cpu().view(torch.int16), att[::S].view(torch.int16)) and torch.equal(xp.cpu().view(torch.int32), xq[::S].view(torch.int32))


@pytest.mark.parametrize("D", EMB_D)
@pytest.mark.parametrize("pick", ["cls", "eos", "argmax2", "argmax_neg"])
def test_pool_head_and_pool_layernorm(pick, D):
    """pool_head_kernel (the generic head, P % 128 != 0 included) and pool_layernorm_kernel against float64: LayerNorm of the row the
    EOS rule picks [-> projection -> L2 normalise]"""
    from plip_amd.kernel_entries import pool_rows
    ck = Checks()
    for S, B in ((5, 9), (77, 13), (256, 3)):
        g0 = _gen(D + S)
        x = torch.randn(B, S, D, generator=g0) + 1.5
        x[:, :, 5] += 60.0
        w, b = torch.randn(D, generator=g0) * 0.5 + 1.0, torch.randn(D, generator=g0)
        ids = None if pick == "cls" else _captions(B, S, D + S)
        eos_id = {"cls": -1, "eos": VOCAB - 1, "argmax2": 2, "argmax_neg": -1}[pick]
        xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
        ids_d = None if ids is None else ids.to(DEV)
        case = f"D{D}_S{S}_B{B}_{pick}"
        y = pool_rows(xd, wd, bd, ids_d, eos_id, eps=EPS)
        torch.cuda.synchronize()
        ck.add("pool_layernorm", case, y, R.pooled_head(x, ids, eos_id, w, b, EPS), R.pooled_head(x, ids, eos_id, w, b, EPS, dtype=torch.float32))
        for P in (32, 80, 200, 512, 1000):
            W = torch.randn(P, D, generator=g0) / D ** 0.5
            wt = W.T.contiguous().to(DEV)
            for normalize in (False, True):
                y = pool_rows(xd, wd, bd, ids_d, eos_id, wt=wt, normalize=normalize, eps=EPS)
                torch.cuda.synchronize()
                ck.add(f"pool_head_n{int(normalize)}", f"{case}_P{P}", y, R.pooled_head(x, ids, eos_id, w, b, EPS, W, normalize),
                       R.pooled_head(x, ids, eos_id, w, b, EPS, W, normalize, torch.float32))
    ck.done()


# =====================================================================================================================================
# head GEMM, logits, arg-max, top-k, L2 normalise.  Integer entries in -8 .. 8 with D <= 1024 keep every partial sum below 2^24, so
# ANY correct fp32 summation order gives the float64 result exactly: no tolerance.
# =====================================================================================================================================
def _ints(rows, cols, gen):
    return torch.randint(-8, 9, (rows, cols), generator=gen).float()


def test_head_gemm_exact_on_integers():
    from plip_amd.kernel_entries import head_gemm
    g0 = _gen(41)
    for M in (1, 31, 32, 33, 256):
        for N in (32, 512, 992):
            for K in (32, 512, 768, 1024):
                a, w = _ints(M, K, g0), _ints(N, K, g0)
                for scale in (1.0, 0.5):
                    y = head_gemm(a.to(DEV), w.to(DEV), scale)
                    torch.cuda.synchronize()
                    assert torch.equal(y.cpu().double(), scale * (a.double() @ w.double().T)), (M, N, K, scale)


def test_head_gemm_random_data_and_row_independence():
    from plip_amd.kernel_entries import head_gemm
    g0 = _gen(42)
    ck = Checks()
    for M, N, K in ((1, 32, 32), (33, 512, 768), (256, 992, 1024)):
        a, w = torch.randn(M, K, generator=g0), torch.randn(N, K, generator=g0) / K ** 0.5
        y = head_gemm(a.to(DEV), w.to(DEV), 0.37)
        torch.cuda.synchronize()
        ck.add(f"head_gemm_K{K}", f"{M}x{N}x{K}", y, 0.37 * (a.double() @ w.double().T), np.float32(0.37) * (a @ w.T))
        if M >= 8:                                                        # rows 3..7 alone: the same bits (batch invariance of the heads)
            y2 = head_gemm(a[3:8].contiguous().to(DEV), w.to(DEV), 0.37)
            assert torch.equal(y2.view(torch.int32), y[3:8].view(torch.int32))
    ck.done()


def test_logits_exact_on_integers(heads):
    """both logits kernels (the scalar-FMA tile with its zero-filled k tail, and the MFMA head GEMM where the shape tiles): lpi exact,
    lpt its transpose bit for bit, arg-max = np.argmax"""
    g0 = _gen(43)
    for Ni in (1, 63, 64, 65, 300):
        for Nt in (1, 10, 64, 130):
            for D in (20, 64, 500, 512):
                img, txt = _ints(Ni, D, g0), _ints(Nt, D, g0)
                lpi, lpt, am = heads.logits(img, txt, scale=0.5, want_text=True, want_argmax=True)
                torch.cuda.synchronize()
                ref = 0.5 * (img.double() @ txt.double().T)
                assert torch.equal(lpi.cpu().double(), ref), (Ni, Nt, D)
                assert torch.equal(lpt.cpu(), lpi.cpu().T.contiguous()), (Ni, Nt, D)
                np.testing.assert_array_equal(am.cpu().numpy(), np.argmax(ref.numpy(), axis=1))
                np.testing.assert_array_equal(am.cpu().numpy(), R.first_argmax(ref.numpy()))


@pytest.mark.parametrize("Nt,want_text", [(130, True), (160, False), (128, True), (1, True)])
def test_row_argmax_takes_the_first_of_exact_ties(heads, Nt, want_text):
    """image i is 8 e_i, so row i of the logits is 8 * txt[:, i]: the columns of txt ARE the score rows.  2-way and 70-way ties, a tie
    across lanes 63 | 64, a tie inside one lane's columns (5 and 69), the maximum in the last column, a whole row of equal scores"""
    D = 64
    txt = torch.randint(-8, 0, (Nt, D), generator=_gen(Nt)).float()       # background: negative
    want = []
    if Nt > 100:
        txt[[63, 64], 0] = 3.0; want.append(63)
        txt[[5, 69], 1] = 3.0; want.append(5)
        txt[30:100, 2] = 2.0; want.append(30)
        txt[Nt - 1, 3] = 1.0; want.append(Nt - 1)
        txt[:, 4] = 7.0; want.append(0)
        txt[[64, 127], 5] = 4.0; want.append(64)
        txt[[Nt - 2, Nt - 1], 6] = 4.0; want.append(Nt - 2)
    else:
        want = [0] * 7
    Ni = 32 if Nt % 32 == 0 else len(want)                                # 32 rows: the shape the MFMA logits path takes
    img = torch.zeros(Ni, D)
    img[torch.arange(Ni), torch.arange(Ni)] = 8.0
    lpi, lpt, am = heads.logits(img, txt, scale=1.0, want_text=want_text, want_argmax=True)
    torch.cuda.synchronize()
    ref = img.double() @ txt.double().T
    assert torch.equal(lpi.cpu().double(), ref)
    assert am.cpu().tolist()[:len(want)] == want
    np.testing.assert_array_equal(am.cpu().numpy(), np.argmax(ref.numpy(), axis=1))


@pytest.mark.parametrize("M", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("N", [1, 9])
def test_topk_is_the_stable_descending_argsort(heads, N, M):
    """integer scores with many ties, -inf entries, NaNs (sorted as -inf) and +inf; k == M is the full sort"""
    rs = np.random.RandomState(1000 * N + M)
    sc = rs.randint(-3, 4, size=(N, M)).astype(np.float32)
    if M > 10:
        sc[0, 5:M // 3] = -np.inf
        sc[N - 1, ::7] = np.nan
        sc[N // 2, [3, M - 1]] = np.inf
        sc[N - 1, M - 2] = -np.inf
    for k in sorted({1, min(50, M), M}):
        idx = heads.topk(torch.from_numpy(sc), k)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(idx.cpu().numpy(), R.topk_stable(sc, k))


def test_similarity_topk_exact_across_panel_borders(heads):
    """integer embeddings: the index matrix equals the stable reference across the 8192-column panel border (a tie between the last
    column of one panel and the first of the next), the ragged tail panel, the 4096-query block border, at the list capacity k = 1024"""
    g0 = _gen(44)
    Nq, Ns, D, k = 4096 + 5, 8192 + 3, 32, 1024
    q = torch.randint(-2, 3, (Nq, D), generator=g0).float()
    sp = torch.randint(-2, 3, (Ns, D), generator=g0).float()
    sp[8191] = sp[8192] = sp[17] = 2.0 * torch.sign(q[0]) + (q[0] == 0).float()      # the same vector: top of the list for query 0
    idx, vals = heads.similarity_topk(q, sp, k, return_values=True)
    torch.cuda.synchronize()
    ref = q.double() @ sp.double().T
    want = R.topk_stable(ref.numpy(), k)
    assert idx[0, :3].tolist() == [17, 8191, 8192]
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    assert torch.equal(vals.cpu().double(), torch.gather(ref, 1, torch.from_numpy(want)))


@pytest.mark.parametrize("D", [1, 3, 64, 65, 512, 1000])
def test_l2_normalize(heads, D):
    ck = Checks()
    for N in (1, 4, 5, 1027):
        g0 = _gen(100 * D + N)
        x = torch.randn(N + 2, D, generator=g0) * 3.0
        zero = N // 2 if N >= 4 else None
        if zero is not None:
            x[1 + zero] = 0.0
        buf = x.to(DEV)
        heads.l2_normalize_(buf[1:N + 1])                                 # rows 1 .. N of the buffer: rows 0 and N + 1 are not the call's
        torch.cuda.synchronize()
        got = buf.cpu()
        assert torch.equal(got[0], x[0]) and torch.equal(got[N + 1], x[N + 1])
        keep = torch.ones(N, dtype=torch.bool)
        if zero is not None:
            keep[zero] = False
            assert not torch.isfinite(got[1 + zero]).any()                # 0 / 0, as the reference's division
        xs = x[1:N + 1][keep]
        ref = xs.double() / torch.sqrt((xs.double() ** 2).sum(-1, keepdim=True))
        cpu = xs / torch.sqrt((xs * xs).sum(-1, keepdim=True))
        ck.add("l2_normalize", f"D{D}_N{N}", got[1:N + 1][keep], ref, cpu)        # the zero row's neighbours included
    ck.done()


# =====================================================================================================================================
# argument checks: return codes only, every one refused on the host before any launch
# =====================================================================================================================================
def test_argument_checks():
    from plip_amd import _lib
    from plip_amd._lib import PlipmiError
    from plip_amd import kernel_entries as KE
    lib = _lib.load()
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)
    with pytest.raises(PlipmiError):
        KE.attention_probs(z(1025, 192), 1, 1025, 1)                      # S = 1025
    qkv = z(16, 192)
    assert lib.plipmi_attention_probs(_lib.F32, C.c_void_p(qkv.data_ptr()), None, 1, 16, 1, 0, None, None) != 0      # null probs
    with pytest.raises(PlipmiError):
        KE.layernorm(z(2, 2052), z(2052), z(2052))                        # D > 2048
    with pytest.raises(PlipmiError):
        KE.layernorm(z(2, 6), z(6), z(6))                                 # D % 4 != 0
    with pytest.raises(PlipmiError):
        KE.layernorm_emit(z(2, 96), z(96), z(96), torch.bfloat16)         # D % 64 != 0
    with pytest.raises(PlipmiError):
        KE.head_gemm(z(4, 48), z(32, 48))                                 # K % 32 != 0
    with pytest.raises(PlipmiError):
        KE.pool_rows(z(1, 2, 64), z(64), z(64), wt=z(64, 1025))           # P > 1024
    with pytest.raises(PlipmiError):
        KE.text_embed_emit(z(1, 257, dtype=torch.int64), z(8, 64), z(257, 64), torch.bfloat16, packed=True, eos_id=7)   # S > 256
    with pytest.raises(PlipmiError):
        KE.fold_ln(z(2, 6), z(2), z(6), z(6), torch.bfloat16)             # K % 4 != 0
    with pytest.raises(PlipmiError):                                      # one 64-column slice: the folded epilogue reads the partials in pairs
        KE.gemm_nt_ln(0, z(4, 64, dtype=torch.bfloat16), z(256, 64, dtype=torch.bfloat16), z(256), z(4, 1, 2))
    torch.cuda.synchronize()
