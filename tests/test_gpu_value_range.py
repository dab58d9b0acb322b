"""Range-edge and non-finite VALUES through every 16-bit rounding site, on the MI355X, one kernel at a time through
plip_amd/kernel_entries.py.  The other kernel-level modules vary shapes, tiles, types and masks on unit-scale ``randn``; this one
varies the values:

  1. operands spread over 2^-20 .. 2^12 (rows of A) x 2^-14 .. 2^10 (rows of W), so that the outputs of ONE product cover the f16
     saturation (+-65504), its subnormal range, underflow to zero, and f16-subnormal operands into the matrix cores -- on every GEMM
     tile, the naive kernel and the small-M split-K kernel, through every epilogue that rounds to 16 bits;
  2. NaN / +inf / -inf in one operand element: propagated inside the row / column it belongs to exactly where float64 arithmetic
     propagates it (inf saturating in the f16 engine's 16-bit stores: INTEGRATION.md), and NOT ONE BIT moved anywhere else, the
     guard rows behind every output included; the same for the attention kernels, the small kernels with an f16 output, and the
     engine (one NaN pixel -> that image's embedding NaN, the other images' embeddings unchanged);
  3. a saturated softmax (one score leads its row by more than 200: exp(-200) is 0 in fp32, P is exactly one-hot): every attention
     kernel must return the selected V row bit for bit.

References: float64 on the SAME rounded operands; ``small_kernel_refs.round_to`` is the engines' store rounding (pinned on the CPU
by tests/test_small_kernel_refs_host.py).  Bounds:
  * fp32 result of a product: |y32 - ref| <= 2e-6 * (|A| |W|^T + |bias|) per element -- the CPU's own fp32 product of these operands
    sits at 2.5e-7 of that bound, the 8x is for another summation order;
  * a 16-bit store of an fp32 value the test also holds: BIT FOR BIT ``round_to`` of it (same K loop, same fp32 add: only the
    conversion differs);
  * QuickGELU (v_exp_f32 / v_rcp_f32, 1 fp32 ulp each): at most ONE unit in the last place of the 16-bit type from ``round_to`` of
    the float64 function of the kernel's own fp32 pre-activation, exact +-65504 where the reference saturates, finite everywhere.
    One allowance, from the range of fp32 and not from the kernels: where 1 + exp(-1.702 y) leaves fp32's normal range (y < -51.3:
    the reciprocal is an fp32 subnormal or the sum overflows) the fp32 formula itself gives -0 while the float64 one gives
    |q| < 52 * 2^-126 < 2^-120; there a difference of at most 2^-120 passes (bf16 only: all of it is 0 in f16), on no more
    elements than have their pre-activation in (-58, -51.3) -- 0.6 % of the 169 472;
  * LayerNorm-folded epilogues: test_gpu_gemm.py's figures (6e-3 bf16 / 8e-4 f16) times the PER-ELEMENT bound
    rstd * (|A| |W|^T) + |c2| instead of the largest reference magnitude, plus half the type's smallest spacing -- measured, like
    there, from the float64 value itself (clamped to +-65504 for f16: the continuous part of ``round_to``), not from its rounding:
    next to a midpoint the kernel's rounding of its fp32 value and ``round_to`` of the float64 one are a WHOLE spacing apart,
    2^-10 of a value just above a power of two, which no half-ulp figure covers (measured: 1.11 x the bound at one element).
    Where the reference saturates the result must be exactly +-65504.
Every test prints ``PARITY`` lines; profiles/value_range_parity.txt keeps them."""
import functools

import pytest
import torch

import small_kernel_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
TILES = list(range(7))                                                    # csrc/gemm_inst.h
M, N, K = 331, 512, 256       # ragged last row tile on the 128- / 160- / 192- / 256- / 320-row tiles; two 256-column tiles; four 16-bit K tiles
GUARD = 21                    # 352 rows allocated: rows 336 .. 351 are a whole lo band of guard
EPS = 1e-5
SENT = 0xA5
F16_MAX = 65504.0
F16_SAT = 65520.0             # the first value that rounds beyond the largest f16
LN_RND = {torch.bfloat16: 6e-3, torch.float16: 8e-4}                      # test_gpu_gemm.py test_layernorm_folded_consumer_epilogue
HALF_SPACING = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}    # half the types' smallest spacing (their subnormals')
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
POISON = {"nan": float("nan"), "pinf": float("inf"), "ninf": float("-inf")}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    t = t.contiguous()
    return t.view(_INT[t.element_size()])


def _sent(rows, cols, dtype):
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full((rows, cols * size), SENT, dtype=torch.uint8, device=DEV).view(dtype)


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == SENT).all())


def _parity(group, case, bound, value):
    print(f"\nPARITY group={group} case={case} bound={bound:.3e} gpu={value:.3e}")


# every tile, the naive checker (-2) and the small-M split-K kernel (-3: the 16-bit types only)
GEMM_CASES = [(d, v) for d in DT for v in TILES + [-2, -3] if not (d == "f32" and v == -3)]
GEMM_IDS = [f"{d}-v{v}" for d, v in GEMM_CASES]


def _same_or_both_nan(got, want):
    """bit-identical, a NaN counting as equal to any NaN"""
    return bool(((_bits(got) == _bits(want)) | (torch.isnan(got) & torch.isnan(want))).all())


# =====================================================================================================================================
# 1. wide-range operands
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _operands(dname):
    """A = randn * 2^ea[m], W = randn / 16 * 2^ew[n], bias = randn * 2^ew[n] (zero on odd columns), rounded to the operand type;
    the float64 reference product, its per-element bound, the LayerNorm statistics of section 1's folded epilogues.  On the CPU,
    computed once, never written to."""
    dt = DT[dname]
    g = _gen(4242)
    ea = -20 + (7 * torch.arange(M)) % 33
    ew = -10 + (5 * torch.arange(N)) % 25
    a = (torch.randn(M, K, generator=g) * torch.exp2(ea.float())[:, None]).to(dt)
    w = (torch.randn(N, K, generator=g) / 16 * torch.exp2(ew.float())[:, None]).to(dt)
    bias = torch.randn(N, generator=g) * torch.exp2(ew.float())
    bias[1::2] = 0.0
    bias = bias.to(dt).float()
    assert torch.isfinite(a).all() and torch.isfinite(w).all() and torch.isfinite(bias).all()
    acc = a.double() @ w.double().T
    mag = a.double().abs() @ w.double().abs().T
    # statistics [M, K // 64, 2] = {sum, M2} per 64 columns: a third of the rows CONSTANT (M2 = 0 everywhere, equal slice sums:
    # rstd = eps^-1/2), a third very WIDE (M2 = 1e12), a third ordinary
    st = torch.zeros(M, K // 64, 2)
    rows = torch.arange(M)
    st[:, :, 0] = (torch.randn(M, K // 64, generator=g) * 8.0)
    st[:, :, 1] = 64.0 * (0.5 + torch.rand(M, K // 64, generator=g))
    const, wide = rows % 3 == 0, rows % 3 == 1
    st[const, :, 0] = (64.0 * ((rows[const] % 7) - 3).float())[:, None]
    st[const, :, 1] = 0.0
    st[wide, :, 0] = 0.0
    st[wide, :, 1] = 2.5e11
    s64 = st.double()
    mean = s64[..., 0].sum(-1) / K
    m2 = s64[..., 1].sum(-1) + (64.0 * (s64[..., 0] / 64.0 - mean[:, None]) ** 2).sum(-1)          # Chan, in float64
    rstd = 1.0 / torch.sqrt(m2 / K + EPS)
    assert (rstd[const] == EPS ** -0.5).all() and (rstd[wide] < 2e-5).all()
    return dict(a=a, w=w, bias=bias, acc=acc, mag=mag, ref=acc + bias.double(), bound=mag + bias.double().abs(), st=st, rstd=rstd[:, None])


@functools.lru_cache(maxsize=None)
def _dev(dname):
    d = _operands(dname)
    return {k: d[k].to(DEV) for k in ("a", "w", "bias", "st")}


def test_the_reference_covers_every_class():
    """the classes the module is about, counted on the float64 reference of the f16 operands (each at least half the figure the
    inputs were designed to: 6648 saturating, 16049 subnormal, 4147 underflowing outputs, 23 % subnormal entries of A, 28771 outputs
    that flushing those operands would change) -- a change of inputs cannot empty a class unnoticed"""
    d = _operands("f16")
    ref, a, w = d["ref"], d["a"], d["w"]
    r = R.round_to(ref, torch.float16)
    sat = int((ref.abs() >= F16_SAT).sum())
    sub = int(((r != 0) & (r.abs() < 2.0 ** -14)).sum())
    zero = int(((r == 0) & (ref != 0)).sum())
    a_sub = float(((a != 0) & (a.abs() < 2.0 ** -14)).float().mean())
    a_flushed = torch.where(a.abs() < 2.0 ** -14, torch.zeros_like(a), a)
    flushed = int((_bits(R.round_to(a_flushed.double() @ w.double().T + d["bias"].double(), torch.float16)) != _bits(r)).sum())
    for name, got, least in (("saturating", sat, 6648 / 2), ("subnormal", sub, 16049 / 2), ("underflow", zero, 4147 / 2),
                             ("subnormal_A_fraction", a_sub, 0.23 / 2), ("changed_by_flushing_A", flushed, 28771 / 2)):
        _parity("class_counts", name, least, got)
        assert got >= least, (name, got, least)
    assert torch.isfinite(_operands("bf16")["ref"]).all()


def _ulp_histogram(got, want):
    d = (R.ord16(got) - R.ord16(want)).reshape(-1)
    return d, {int(k): int((d == k).sum()) for k in torch.unique(d)}


@pytest.mark.parametrize("dname,variant", GEMM_CASES, ids=GEMM_IDS)
def test_wide_range_gemm_stores_round_saturate_and_underflow(dname, variant):
    from plip_amd.kernel_entries import gemm_nt
    dt, d, g = DT[dname], _operands(dname), _dev(dname)
    case = f"{dname}_v{variant}"
    # the fp32 twin: epilogue 2 on C = 0
    y32 = gemm_nt(g["a"], g["w"], g["bias"], epilogue=2, variant=variant, out=torch.zeros(M, N, device=DEV))
    y0 = gemm_nt(g["a"], g["w"], g["bias"], epilogue=0, variant=variant)
    y1 = gemm_nt(g["a"], g["w"], g["bias"], epilogue=1, variant=variant)
    torch.cuda.synchronize()
    y32, y0, y1 = y32.cpu(), y0.cpu(), y1.cpu()
    ratio = float(((y32.double() - d["ref"]).abs() / d["bound"].clamp(min=1e-300)).max())
    _parity("wide_gemm_fp32_twin", case, 2e-6, ratio)
    assert torch.isfinite(y32).all() and ratio <= 2e-6, (case, ratio)
    # epilogue 0: the same fp32 value through the type's store
    want0 = R.round_to(y32.double(), dt)
    moved = int((_bits(y0) != _bits(want0)).sum())
    _parity("wide_gemm_store_bits_moved", case, 0, moved)
    assert moved == 0, (case, moved)
    if dt == torch.float16:
        assert int((y0.abs() == F16_MAX).sum()) >= 6648 // 2 and int(((y0 != 0) & (y0.abs() < 2.0 ** -14)).sum()) >= 16049 // 2
    # epilogue 1: QuickGELU of that value
    q = R.quick_gelu(y32.double())
    assert torch.isfinite(y1).all(), case
    if dt == torch.float32:
        # expf and the divide are correctly rounded to an ulp or two; the argument -1.702f * y carries |arg| ulps into exp
        tol = (8.0 + 2.0 * 1.702 * y32.double().abs().clamp(max=90.0)) * 2.0 ** -24 * q.abs() + 2.0 ** -120
        ratio = float(((y1.double() - q).abs() / tol).max())
        _parity("wide_gemm_quickgelu_fp32", case, 1.0, ratio)
        assert ratio <= 1.0, (case, ratio)
        return
    want1 = R.round_to(q, dt)
    dist, hist = _ulp_histogram(y1, want1)
    edge = (dist.abs() > 1) & ((y1.double() - want1.double()).abs().reshape(-1) <= 2.0 ** -120) & (y32.reshape(-1) < -51.3)
    near = {k: v for k, v in hist.items() if abs(k) <= 1}
    print(f"\nPARITY group=wide_gemm_quickgelu_ulps case={case} bound=1 histogram={near} beyond={int((dist.abs() > 1).sum())} "
          f"of_them_at_the_fp32_range_edge={int(edge.sum())}")
    assert int(((dist.abs() > 1) & ~edge).sum()) == 0, (case, hist)
    # the allowance cannot grow unnoticed: it exists only where the float64 result still rounds to a non-zero bf16 (y > -58), i.e. on
    # the pre-activations in (-58, -51.3) -- 1020 of the 169 472 here (0.6 %), 765 of them measured beyond one ulp -- and never in f16
    window = int(((y32 < -51.3) & (y32 > -58.0)).sum())
    assert int(edge.sum()) <= (window if dt == torch.bfloat16 else 0) and window <= M * N * 7 // 1000, (case, int(edge.sum()), window)
    if dt == torch.float16:
        sat = q.abs() >= F16_SAT
        assert int(sat.sum()) > 1000 and torch.equal(y1[sat].double(), torch.sign(q[sat]) * F16_MAX), case


def _ln_ref(d, mode):
    v = d["rstd"] * d["acc"] + d["bias"].double()
    bound = d["rstd"] * d["mag"] + d["bias"].double().abs()
    return (R.quick_gelu(v) if mode == 1 else v), bound


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("variant", TILES + [-1, -3])
@pytest.mark.parametrize("hname", list(HALF))
def test_wide_range_layernorm_folded_epilogues(hname, variant, mode):
    """rstd * (A @ W^T) + c2 [QuickGELU] with statistics that describe constant rows (M2 = 0: rstd = eps^-1/2 = 316), very wide
    rows (M2 = 1e12: rstd = 1.6e-5) and ordinary rows, against float64 of the same operands and statistics"""
    from plip_amd.kernel_entries import gemm_nt_ln
    hdt, d, g = HALF[hname], _operands(hname), _dev(hname)
    y = gemm_nt_ln(mode, g["a"], g["w"], g["bias"], g["st"], eps=EPS, variant=variant)
    torch.cuda.synchronize()
    y = y.cpu()
    ref, bound = _ln_ref(d, mode)
    want = ref.clamp(-F16_MAX, F16_MAX) if hdt == torch.float16 else ref
    assert torch.isfinite(y).all()
    tol = LN_RND[hdt] * bound + HALF_SPACING[hdt]                         # (bf16 does not overflow on these operands, f16 saturates: all finite)
    r = (y.double() - want).abs() / tol
    ratio, at = float(r.max()), int(r.argmax())
    case = f"{hname}_v{variant}_mode{mode}"
    _parity("wide_ln_folded", case, 1.0, ratio)
    m, n = at // N, at % N
    assert ratio <= 1.0, (case, ratio, (m, n), float(y[m, n]), float(want[m, n]), float(ref[m, n]), float(bound[m, n]))
    if hdt == torch.float16:
        sat = ref.abs() >= F16_SAT * (1 + 1e-5)                           # fp32 round-off of the kernel's value stays beyond 65520
        assert int(sat.sum()) > 1000 and torch.equal(y[sat].double(), torch.sign(ref[sat]) * F16_MAX), case
    rows = torch.arange(M) % 3 == 0                                       # constant rows: rstd = 316, not 0 -- c2 is 0 on the odd columns
    assert float((y[rows][:, 1::2] != 0).float().mean()) > 0.4, case


def _small_m_split_ref(a, w, bias, x0q):
    """What the small-M kernel's split-plane epilogue computes, composed from calls whose arithmetic is known (test_gpu_gemm.py
    test_small_m_split_plane_residual_epilogue): its raw fp32 accumulators v from the fp32 twin on C = 0, bias = 0 (0 + (v + 0) = v,
    NaN and inf included), then (x0q + bias) + v as two IEEE fp32 adds.  Mode 2 is no reference at -3: it adds x + (v + bias).
    (The twin turns an accumulator of -0 into +0, which matters only next to an x0q + bias of -0: asserted absent.)"""
    from plip_amd.kernel_entries import gemm_nt
    v = gemm_nt(a, w, torch.zeros(N, device=DEV), epilogue=2, variant=-3, out=torch.zeros(M, N, device=DEV))
    xb = x0q + bias[None, :]
    assert not bool(((xb == 0) & torch.signbit(xb)).any())
    return xb + v


# every tile and the cost model's for the three (type, mode) pairs; the small-M kernel has mode 3 only, in both types
SPLIT_CASES = [(h, m, v) for h, m in (("f16", 3), ("f16", 4), ("bf16", 4)) for v in TILES + [-1]] + [("f16", 3, -3), ("bf16", 3, -3)]


@pytest.mark.parametrize("hname,mode,variant", SPLIT_CASES, ids=[f"{h}-{m}-{v}" for h, m, v in SPLIT_CASES])
def test_wide_range_split_plane_epilogues(hname, mode, variant):
    """the residual update on planes whose values sit at the edges of f16: 65500 carried past 65504 by the update, subnormal entries
    that stay subnormal, and the wide-range update everywhere else -- planes = the host split (of the type the mode writes) of the
    plain-array epilogue's fp32 result, bit for bit, as test_gpu_gemm.py requires at ordinary magnitudes (variant -3: of the composed
    reference _small_m_split_ref, the small-M kernel's plain-array epilogue adding in another order)"""
    from plip_amd.kernel_entries import gemm_nt_ln, join_planes, lo_plane_values, split_planes
    hdt, d, g = HALF[hname], _operands(hname), _dev(hname)
    odt = hdt if mode == 3 else (torch.bfloat16 if hdt == torch.float16 else torch.float16)
    g0 = _gen(4300)
    x0 = torch.randn(M, N, generator=g0) * 3.0 + 1.0
    ref = d["ref"]
    up, down, tiny = (ref > 10.0) & (ref < 1e4), (ref < -10.0) & (ref > -1e4), ref.abs() < 2.0 ** -17
    if hdt == torch.float16:
        x0[up], x0[down] = 65500.0, -65500.0
        x0[tiny] = torch.randn(int(tiny.sum()), generator=g0) * 2.0 ** -16
    hi0, lo0 = split_planes(x0.to(DEV), hdt)
    x0q = join_planes(hi0, lo0)
    if variant == -3:
        x_ref = _small_m_split_ref(g["a"], g["w"], g["bias"], x0q)
    else:
        x_ref, _, _ = gemm_nt_ln(2, g["a"], g["w"], g["bias"], variant=variant, out=x0q.clone())
    hi, lo, st = gemm_nt_ln(mode, g["a"], g["w"], g["bias"], variant=variant, out=(hi0.clone(), lo0.clone()))
    torch.cuda.synchronize()
    hi = hi.view(odt)
    want_hi, want_lo = split_planes(x_ref, odt)
    assert torch.isfinite(x_ref).all()
    bad_hi = int((_bits(hi) != _bits(want_hi)).sum())
    bad_lo = int((lo_plane_values(lo, M, N) != lo_plane_values(want_lo, M, N)).sum())
    _parity("wide_split_planes_moved", f"{hname}_mode{mode}_v{variant}", 0, bad_hi + bad_lo)
    assert bad_hi == 0 and bad_lo == 0, (bad_hi, bad_lo)
    if odt == torch.float16:
        h = hi.cpu()
        assert int((h.abs() == F16_MAX).sum()) > 1000
        if hdt == torch.float16:
            assert (h[up] == F16_MAX).all() and (h[down] == -F16_MAX).all() and int(up.sum()) > 100 and int(down.sum()) > 100
            sub = (h[tiny] != 0) & (h[tiny].abs() < 2.0 ** -14)
            assert int(sub.sum()) > 100


# =====================================================================================================================================
# 2. non-finite operands: propagated inside their row / column, contained everywhere else
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _nf_operands(dname):
    """section 1's operands with no zero in the A column / W column an inf will meet (an inf meets no zero), C / x0 of the residual
    epilogues; K0 = the poisoned column of A's row M - 1, (N0, K1) = the poisoned element of W"""
    d = _operands(dname)
    a, w = d["a"].clone(), d["w"].clone()
    tiny = 2.0 ** -24 if dname == "f16" else 2.0 ** -100
    K0, N0, K1 = 77, 300, 130
    w[:, K0] = torch.where(w[:, K0] == 0, torch.full_like(w[:, K0], tiny), w[:, K0])
    a[:, K1] = torch.where(a[:, K1] == 0, torch.full_like(a[:, K1], tiny), a[:, K1])
    c0 = torch.randn(M, N, generator=_gen(4343)) * 3.0 + 1.0
    return dict(a=a, w=w, bias=d["bias"], st=d["st"], rstd=d["rstd"], c0=c0, K0=K0, N0=N0, K1=K1)


EPIS = ["e0", "e1", "e2", "ln0", "ln1", "ln2", "ln3"]


def _epis(dname, variant):
    out = ["e0", "e1", "e2"]
    if dname != "f32" and variant != -2:                                  # the naive checker has no LayerNorm-folded epilogue
        out += ["ln0", "ln1", "ln2", "ln3"]                                # (-3 too: the latency path's out_proj and fc2 run its ln3)
    return out


def _run(epi, dname, variant, a, w, dv):
    """one launch into sentinel-filled buffers with guard rows -> {name: tensor} of everything the launch writes"""
    import ctypes as C

    from plip_amd import _lib
    from plip_amd.engine import _code, _ptr
    from plip_amd.kernel_entries import gemm_nt, gemm_nt_ln_rows, lo_plane_bytes
    dt = DT[dname]
    rows = M + GUARD
    if epi in ("e0", "e1"):
        out = _sent(rows, N, dt)
        gemm_nt(a, w, dv["bias"], epilogue=int(epi[1]), variant=variant, out=out)
        return {"y": out}
    if epi == "e2":
        out = _sent(rows, N, torch.float32)
        out[:M] = dv["c0"]
        gemm_nt(a, w, dv["bias"], epilogue=2, variant=variant, out=out)
        return {"c": out}
    if epi in ("ln0", "ln1"):
        out = _sent(rows, N, dt)
        gemm_nt_ln_rows(int(epi[2]), a, w, dv["bias"], None, out, stats=dv["st"], eps=EPS, variant=variant)
        return {"y": out}
    if epi == "ln2":
        out = _sent(rows, N, torch.float32)
        out[:M] = dv["c0"]
        xb = _sent(rows, N, dt)                                            # the C entry itself: the wrapper would allocate xb and st, M rows each
        st = _sent(rows, (N // 64) * 2, torch.float32).view(rows, N // 64, 2)
        with torch.cuda.device(a.device):
            _lib.check(_lib.load().plipmi_gemm_nt_ln(_code(dt), 2, variant, M, N, K, _ptr(a), _ptr(w), _ptr(dv["bias"]), None, 0, float(EPS),
                                                     _ptr(out), _ptr(xb), _ptr(st), C.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)),
                       "plipmi_gemm_nt_ln")
        return {"c": out, "xb": xb, "st": st}
    hi = _sent(rows, N, dt)
    lo = torch.full((lo_plane_bytes(rows, N),), SENT, dtype=torch.uint8, device=DEV)
    st = _sent(rows, (N // 64) * 2, torch.float32).view(rows, N // 64, 2)
    hi[:M], lo[dv["idx"][:M].reshape(-1)] = dv["hi0"], dv["lo0v"].reshape(-1)
    gemm_nt_ln_rows(3, a, w, dv["bias"], None, (hi, lo), st=st, eps=EPS, variant=variant)
    return {"hi": hi, "lo": lo[dv["idx"].reshape(-1)].reshape(rows, N), "st": st}


def _expected(epi, a_part, w_part, bias, rstd, c0):
    """float64 arithmetic on the poisoned row (a_part [1, K], w_part [N, K]) or column (a_part [M, K], w_part [1, K])"""
    acc = (a_part.double()[:, None, :] * w_part.double()[None, :, :]).sum(-1)          # plain products and sums: no BLAS
    if epi in ("e0", "e1"):
        v = acc + bias
        return R.quick_gelu(v) if epi == "e1" else v
    if epi in ("ln0", "ln1"):
        v = rstd * acc + bias
        return R.quick_gelu(v) if epi == "ln1" else v
    return c0 + (acc + bias)


@pytest.mark.parametrize("dname,variant", GEMM_CASES, ids=GEMM_IDS)
def test_a_non_finite_operand_stays_in_its_row_or_column(dname, variant):
    """NaN, +inf, -inf in one element of A's last live row, then of one row of W; every epilogue the kernel has.
    Containment: outside the poisoned output row / column every output -- the 16-bit copy, both planes, the statistics (outside the
    poisoned column's 64-column slice) -- is bit-identical to the clean run, and the guard rows still hold the sentinel.
    Propagation: inside, NaN exactly where float64 arithmetic gives NaN, in all three types; inf stays inf in fp32 / bf16 and in the
    fp32 outputs of the f16 engine, and is +-65504 with the reference's sign in the f16 engine's 16-bit outputs."""
    from plip_amd.kernel_entries import join_planes, lo_plane_index, lo_plane_values, split_planes
    dt, d = DT[dname], _nf_operands(dname)
    dv = {k: d[k].to(DEV) for k in ("a", "w", "bias", "st", "c0")}
    if dname != "f32":
        dv["idx"] = lo_plane_index(M + GUARD, N, DEV)
        hi0, lo0 = split_planes(dv["c0"], dt)
        dv["hi0"], dv["lo0v"] = hi0, lo_plane_values(lo0, M, N).view(torch.uint8)
        dv["c0"] = join_planes(hi0, lo0)                                   # the stream value the planes stand for: every residual epilogue starts from it
    bias64, rstd64, c064 = d["bias"].double(), d["rstd"], dv["c0"].cpu().double()
    worst = 0
    for epi in _epis(dname, variant):
        clean = _run(epi, dname, variant, dv["a"], dv["w"], dv)
        for site in ("A", "W"):
            for pname, pval in POISON.items():
                a, w = dv["a"].clone(), dv["w"].clone()
                if site == "A":
                    a[M - 1, d["K0"]] = pval
                    part = (slice(M - 1, M), slice(None))
                    want = _expected(epi, a[M - 1:].cpu(), d["w"], bias64[None, :], rstd64[M - 1:], c064[M - 1:])
                else:
                    w[d["N0"], d["K1"]] = pval
                    part = (slice(0, M), slice(d["N0"], d["N0"] + 1))
                    want = _expected(epi, d["a"], w[d["N0"]:d["N0"] + 1].cpu(), bias64[None, d["N0"]:d["N0"] + 1], rstd64, c064[:, d["N0"]:d["N0"] + 1])
                got = _run(epi, dname, variant, a, w, dv)
                torch.cuda.synchronize()
                tag = f"{dname} v{variant} {epi} {site} {pname}"
                assert bool(torch.isnan(want).all()) if pname == "nan" else bool((torch.isinf(want) | torch.isnan(want)).all()), tag
                for name, t in got.items():
                    ref = clean[name]
                    if name == "st":                                       # [rows, N // 64, 2]: the poisoned column's slice belongs to the column
                        inside = torch.zeros(t.shape, dtype=torch.bool, device=DEV)
                        if site == "A":
                            inside[M - 1] = True
                        else:
                            inside[:M, d["N0"] // 64] = True
                    else:
                        inside = torch.zeros(t.shape, dtype=torch.bool, device=DEV)
                        inside[part] = True
                    leaked = int(((_bits(t) != _bits(ref)) & ~inside).sum())
                    worst = max(worst, leaked)
                    assert leaked == 0, (tag, name, leaked)
                    first_guard = 336 if name == "lo" else M                # rows 331 .. 335 share a lo band with live rows: padding
                    if t.shape[0] == M + GUARD:
                        assert _untouched(t[first_guard:]), (tag, name)
                    if name in ("st", "lo"):
                        continue
                    inner = t[part].cpu()
                    nan = torch.isnan(want)
                    assert torch.equal(torch.isnan(inner), nan), (tag, name, int(torch.isnan(inner).sum()), int(nan.sum()))
                    if inner.dtype == torch.float16:                       # the documented contract: +-inf saturate
                        assert torch.equal(inner[~nan].double(), torch.sign(want[~nan]) * F16_MAX), (tag, name)
                    else:
                        assert torch.equal(inner[~nan].double(), want[~nan]), (tag, name)
                if "hi" in got:                                            # ... and the planes are still the host split of the plain-array result
                    # (the small-M kernel: of the composed reference -- its plain-array form adds in another order)
                    x_ref = _small_m_split_ref(a, w, dv["bias"], dv["c0"]) if variant == -3 else _run("ln2", dname, variant, a, w, dv)["c"][:M]
                    want_hi, want_lo = split_planes(x_ref, dt)
                    assert _same_or_both_nan(got["hi"][:M], want_hi), tag
                    ok = ~torch.isnan(x_ref)
                    assert torch.equal(got["lo"][:M][ok], lo_plane_values(want_lo, M, N).view(torch.uint8)[ok]), tag
    _parity("non_finite_gemm_leaked_elements", f"{dname}_v{variant}", 0, worst)


# ---- attention -----------------------------------------------------------------------------------------------------------------------
def _att_kernels():
    return ["valu", "mfma", "mfma_streamed", "packed"]


def _att_run(kernel, qkv, B, S, H, causal, mask, lens=None):
    """-> [B, S, H, 64]; ``packed``: the rows of each caption's first lens[b] tokens packed, the result scattered back (other rows 0)"""
    from plip_amd.kernel_entries import attention, attention_packed
    if kernel != "packed":
        return attention(qkv, B, S, H, causal, mask, impl=0 if kernel == "valu" else 1).view(B, S, H, 64)
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    sel = torch.cat([b * S + torch.arange(int(lens[b])) for b in range(B)]).to(DEV)
    packed = qkv[sel].contiguous()
    out = torch.zeros(packed.shape[0], H * 64, dtype=qkv.dtype, device=DEV)
    attention_packed(packed, out, cu.to(DEV), S, H, causal, mask)
    full = torch.zeros(B * S, H * 64, dtype=qkv.dtype, device=DEV)
    full[sel] = out
    return full.view(B, S, H, 64)


@pytest.mark.parametrize("where", ["live_key", "masked_key"])
@pytest.mark.parametrize("kernel", _att_kernels())
@pytest.mark.parametrize("hname", list(HALF))
def test_a_nan_key_row_reaches_the_queries_that_multiply_it_and_nothing_else(hname, kernel, where):
    """test_gpu_attention.py's NaN-in-a-key-row case in both 16-bit types, on every attention kernel, for a live key and for a key
    the mask hides.  One key row of sample 0, head 0 is NaN at position p (not a multiple of 32).
    The queries that MULTIPLY the key are NaN: under the causal mask the queries j >= p; the MFMA kernels mask additively (score +
    -inf, as HF adds its mask: NaN + -inf = NaN), so there a key the tokenizer mask hides poisons like a live one, and so does the
    part of the key's own 32-key tile above the diagonal: a wave's 32 queries multiply every 32-key tile that reaches their diagonal,
    so queries 32 * (p // 32) .. p - 1 are NaN there too (a change of the tile-skipping rule would show here); the exact-fp32 VALU
    kernel selects, so a hidden key reaches nobody and a live one only the queries j >= p.  Every other sample, head and query:
    bit-identical to the clean run."""
    hdt = HALF[hname]
    S = 300 if kernel == "mfma_streamed" else 77
    B, H = 2, 2
    for causal in (True, False):
        g = _gen(S + int(causal))
        qkv = torch.randn(B * S, 3 * H * 64, generator=g)
        qkv[:, : H * 64] *= 0.125
        n_valid = S // 2 + 3
        lens = torch.full((B,), S if kernel != "packed" else n_valid + 20, dtype=torch.int64)
        mask = (torch.arange(S)[None, :] < n_valid).long().repeat(B, 1).to(DEV)
        p = 40 if where == "live_key" else n_valid + 7
        base = qkv.to(DEV).to(hdt)
        bad = base.clone().view(B, S, 3, H * 64)
        bad[0, p, 1, :64] = float("nan")
        clean = _att_run(kernel, base, B, S, H, causal, mask, lens)
        out = _att_run(kernel, bad.view(B * S, -1), B, S, H, causal, mask, lens)
        torch.cuda.synchronize()
        tag = (hname, kernel, where, causal)
        assert torch.isfinite(clean).all(), tag
        same = (_bits(out) == _bits(clean)).all(-1)                          # [B, S, H]
        assert same[1].all() and same[0, :, 1].all(), tag                   # the other sample, the other head
        nan = torch.isnan(out[0, :, 0]).all(-1)                             # per query of the poisoned (sample, head)
        anynan = torch.isnan(out[0, :, 0]).any(-1)
        assert torch.equal(nan, anynan), tag                                # a row is NaN as a whole or not at all
        ok = nan | same[0, :, 0]
        assert ok.all(), tag
        rows = int(lens[0])                                                 # rows past a packed caption's end do not exist
        additive = kernel != "valu"
        if where == "masked_key" and not additive:
            assert same[0, :, 0].all(), tag                                 # a select: the hidden key reaches nobody
            continue
        if causal:
            first = 32 * (p // 32) if additive else p                       # the first query that multiplies the key
            assert nan[first:rows].all() and same[0, :first, 0].all(), (tag, nan.nonzero().flatten().tolist()[:3], first)
        else:
            assert nan[:rows].all(), tag


def _one_hot_case(S, B, H, causal, hdt, seed, lens):
    """keys in {+-1}^64, q = 16 * the target key: the target's score 1024 leads every other key's by 16 * (64 - k_t . k_j); targets are
    random live keys (j <= i under the causal mask, j < lens[b] always: a packed caption's keys end at its length).  Returns the
    operands and the target rows."""
    g = _gen(seed)
    k = torch.where(torch.rand(B, S, H, 64, generator=g) < 0.5, -1.0, 1.0)
    v = torch.randn(B, S, H, 64, generator=g) * 3.0
    tgt = torch.stack([torch.stack([torch.randint(0, min(i + 1, int(lens[b])) if causal else int(lens[b]), (H,), generator=g) for b in range(B)])
                       for i in range(S)], dim=1)                                                                      # [B, S, H]
    q = 16.0 * torch.gather(k, 1, tgt[..., None].expand(B, S, H, 64))
    qkv = torch.stack((q, k, v), dim=2).reshape(B * S, 3 * H * 64).to(hdt)
    sc = torch.einsum("bihd,bjhd->bhij", q.double(), k.double())
    live = R.live_keys(B, S, causal, None)[:, None].expand(B, H, S, S)
    top = torch.gather(sc, 3, tgt.permute(0, 2, 1)[..., None])
    others = sc.masked_fill(~live, -1e9).scatter(3, tgt.permute(0, 2, 1)[..., None], -1e9).amax(-1, keepdim=True)
    lead = float((top - others).min())
    want = torch.gather(v.to(hdt), 1, tgt[..., None].expand(B, S, H, 64))
    return qkv, want, lead


@pytest.mark.parametrize("kernel", _att_kernels())
@pytest.mark.parametrize("hname", list(HALF))
def test_a_saturated_softmax_returns_the_selected_value_row_bit_for_bit(hname, kernel):
    hdt = HALF[hname]
    S = 300 if kernel == "mfma_streamed" else 77
    B, H = 2, 2
    for causal in (True, False):
        lens = torch.tensor([S, S - 9]) if kernel == "packed" else torch.full((B,), S)
        qkv, want, lead = _one_hot_case(S, B, H, causal, hdt, 500 + S + int(causal), lens)
        assert lead > 200.0, lead                                           # exp(-200) = 0 in fp32: P is exactly one-hot
        out = _att_run(kernel, qkv.to(DEV), B, S, H, causal, None, lens).cpu()
        for b in range(B):
            rows = int(lens[b])
            moved = int((_bits(out[b, :rows]) != _bits(want[b, :rows])).sum())
            _parity("one_hot_attention_bits_moved", f"{hname}_{kernel}_causal{int(causal)}_b{b}", 0, moved)
            assert moved == 0, (hname, kernel, causal, b, moved)


def _fused_inputs(B, S, H, hdt, seed):
    """qkv_attention's operands for a one-hot softmax on the DIAGONAL: a's rows are +-1 patterns, the q block of W is 16 * I, the
    k block I, the v block random; statistics that describe unit variance -- q_i . k_j = 16 rstd^2 a_i . a_j leads at j = i"""
    D = H * 64
    g = _gen(seed)
    x = torch.where(torch.rand(B * S, D, generator=g) < 0.5, -1.0, 1.0)
    eye = torch.eye(D)
    w = torch.cat((16.0 * eye, eye, torch.randn(D, D, generator=g) / D ** 0.5), dim=0)
    c2 = torch.zeros(3 * D)
    c2[2 * D:] = torch.randn(D, generator=g) * 0.2
    st = torch.zeros(B * S, H, 2)
    st[..., 1] = 64.0
    return x.to(DEV).to(hdt), w.to(DEV).to(hdt), c2.to(DEV), st.to(DEV)


@pytest.mark.parametrize("hname", list(HALF))
def test_fused_qkv_attention_one_hot_and_nan_row(hname):
    """csrc/qkv_attention.hip at S = 77: (a) a softmax saturated on the diagonal returns each row's own V row -- the V the two-kernel
    path's GEMM computes -- bit for bit; (b) a NaN in one input row makes that caption's queries from the row on NaN in every head
    (the row's q, k and v are NaN) and leaves the other captions bit-identical to the clean run, NaN for NaN like the two kernels"""
    from plip_amd.kernel_entries import attention, gemm_nt_ln, qkv_attention
    hdt = HALF[hname]
    B, S, H = 5, 77, 2
    D = H * 64
    a, w, c2, st = _fused_inputs(B, S, H, hdt, 77)
    qkv = gemm_nt_ln(0, a, w, c2, st, eps=EPS, variant=-1)
    got = qkv_attention(a, w, c2, st, B, S, H, True, None, eps=EPS)
    torch.cuda.synchronize()
    x = qkv.double().cpu().reshape(B, S, 3, H, 64)
    sc = torch.einsum("bihd,bjhd->bhij", x[:, :, 0], x[:, :, 1])
    off = sc.masked_fill(~torch.tril(torch.ones(S, S, dtype=torch.bool), -1), -1e9).amax(-1)
    lead = float((torch.diagonal(sc, dim1=-2, dim2=-1) - off)[..., 1:].min())
    assert lead > 200.0, lead
    moved = int((_bits(got) != _bits(qkv[:, 2 * D:])).sum())
    _parity("one_hot_attention_bits_moved", f"{hname}_qkv_attention", 0, moved)
    assert moved == 0, moved
    p = 40
    bad = a.clone()
    bad[1 * S + p, 5] = float("nan")
    out = qkv_attention(bad, w, c2, st, B, S, H, True, None, eps=EPS)
    two = attention(gemm_nt_ln(0, bad, w, c2, st, eps=EPS, variant=-1), B, S, H, True, None, impl=1)
    torch.cuda.synchronize()
    assert _same_or_both_nan(out, two)
    o, c = out.view(B, S, H, 64), got.view(B, S, H, 64)
    keep = [b for b in range(B) if b != 1]
    assert torch.equal(_bits(o[keep]), _bits(c[keep]))
    # queries 32 .. p - 1 share the key's 32-key tile: the additive mask makes them NaN too, as in the short MFMA kernel
    assert torch.isnan(o[1, 32:]).all() and torch.equal(_bits(o[1, :32]), _bits(c[1, :32]))


# ---- the small kernels with an f16 output --------------------------------------------------------------------------------------------
def _rows_same_except(got, clean, row):
    keep = torch.ones(got.shape[0], dtype=torch.bool, device=got.device)
    keep[row] = False
    return torch.equal(_bits(got[keep]), _bits(clean[keep]))


@pytest.mark.parametrize("D", [260, 768])                                  # layernorm_kernel / layernorm_fixed_kernel (two rows per wave)
@pytest.mark.parametrize("hname", list(HALF))
def test_layernorm_kernels_nan_row_and_saturation(hname, D):
    from plip_amd.kernel_entries import layernorm, layernorm_emit, lo_plane_values, split_planes
    hdt = HALF[hname]
    g0 = _gen(D)
    rows, bad_row = 9, 4
    x = torch.randn(rows, D, generator=g0) + 1.5
    gain = torch.randn(D, generator=g0) * 0.5 + 1.0
    gain[::3] = 1.0e5                                                      # |xhat| > 0.655 goes past 65504
    beta = torch.randn(D, generator=g0)
    xn = x.clone()
    xn[bad_row, 17] = float("nan")
    xd, xnd, gd, bd = x.to(DEV), xn.to(DEV), gain.to(DEV), beta.to(DEV)
    ref = R.layer_norm(x, gain, beta, EPS)
    sat = ref.abs() >= F16_SAT * (1 + 1e-5)
    assert int(sat.sum()) > 100
    clean = layernorm(xd, gd, bd, EPS, hdt)
    y = layernorm(xnd, gd, bd, EPS, hdt)
    torch.cuda.synchronize()
    assert torch.isnan(y[bad_row]).all() and _rows_same_except(y, clean, bad_row)
    if hdt == torch.float16:
        c = clean.cpu()
        assert torch.isfinite(c).all() and torch.equal(c[sat].double(), torch.sign(ref[sat]) * F16_MAX)
    if D % 64:
        return
    hi0, lo0, st0 = layernorm_emit(xd, gd, bd, hdt, EPS)
    hi, lo, st = layernorm_emit(xnd, gd, bd, hdt, EPS)
    torch.cuda.synchronize()
    assert torch.isnan(hi[bad_row]).all() and _rows_same_except(hi, hi0, bad_row) and _rows_same_except(st, st0, bad_row)
    assert _rows_same_except(lo_plane_values(lo, rows, D), lo_plane_values(lo0, rows, D), bad_row)
    if hdt == torch.float16:
        want_hi, want_lo = split_planes(ref.float(), hdt)                  # beyond 65520: hi = +-65504, the remainder clamped at +-127
        assert torch.isfinite(hi0).all()
        assert torch.equal(_bits(hi0.cpu()[sat]), _bits(want_hi[sat]))
        assert torch.equal(lo_plane_values(lo0.cpu(), rows, D)[sat], lo_plane_values(want_lo, rows, D)[sat])


@pytest.mark.parametrize("hname", list(HALF))
def test_fold_ln_nan_row_and_saturation(hname):
    from plip_amd.kernel_entries import fold_ln
    hdt = HALF[hname]
    g0 = _gen(21)
    rows, K, bad_row = 11, 260, 6
    W = torch.randn(rows, K, generator=g0)
    bias = torch.randn(rows, generator=g0) * 0.1
    gain = torch.exp(torch.empty(K).uniform_(-2.3, 2.3, generator=g0))
    gain[::5] = 2.0e5
    beta = torch.randn(K, generator=g0)
    Wn = W.clone()
    Wn[bad_row, 3] = float("nan")
    wf0, c0 = fold_ln(W.to(DEV), bias.to(DEV), gain.to(DEV), beta.to(DEV), hdt)
    wf, c2 = fold_ln(Wn.to(DEV), bias.to(DEV), gain.to(DEV), beta.to(DEV), hdt)
    torch.cuda.synchronize()
    assert torch.isnan(wf[bad_row]).all() and bool(torch.isnan(c2[bad_row])) and _rows_same_except(wf, wf0, bad_row) and _rows_same_except(c2[:, None], c0[:, None], bad_row)
    if hdt == torch.float16:
        ref_w, _ = R.fold_ln(W, bias, gain, beta, 1.0)
        sat = ref_w.abs() >= F16_SAT * (1 + 1e-5)
        w0 = wf0.cpu()
        assert int(sat.sum()) > 100 and torch.isfinite(w0).all() and torch.equal(w0[sat].double(), torch.sign(ref_w[sat]) * F16_MAX)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("hname", list(HALF))
def test_text_embed_emit_nan_table_row_and_saturation(hname, packed):
    """rows = tok[id] + pos[s] is ONE fp32 add: the planes are the host split of the CPU's fp32 sum bit for bit -- with table values
    that carry the sum past 65504 (f16: hi saturates, the remainder clamps) and with a NaN table row (those rows' hi is NaN)"""
    from plip_amd.kernel_entries import lo_plane_values, split_planes, text_embed_emit
    hdt = HALF[hname]
    g0 = _gen(31)
    B, S, D, vocab, eos = 5, 20, 128, 60, 59
    ids = torch.randint(3, 50, (B, S), generator=g0)
    ids[:, -1] = eos
    ids[1, 9] = eos                                                        # a caption that packs to 10 rows
    ids[2, 7] = ids[4, 0] = 55                                             # the NaN table row: no random id reaches it
    tok = torch.randn(vocab, D, generator=g0) * 0.7
    tok[10:20] *= 9.0e4                                                    # sums far past 65504
    tok[20] = 65400.0                                                      # ... and just around it: + pos ~ N(100, 60)
    pos = torch.randn(S, D, generator=g0) * 60.0 + 100.0
    ids[0, 3], ids[3, 11] = 20, 20
    tok[55, 9] = float("nan")
    x32 = R.embed_rows(ids, tok, pos, torch.float32)
    if packed:
        _, cu, rowmap = R.pack_plan(ids, eos)
        sel = (rowmap.long() >> 8) * S + (rowmap.long() & 255)
        x32 = x32[sel]
    rows = x32.shape[0]
    want_hi, want_lo = split_planes(x32, hdt)
    out = text_embed_emit(ids.to(DEV), tok.to(DEV), pos.to(DEV), hdt, packed=packed, eos_id=eos)
    torch.cuda.synchronize()
    hi, lo = out[0].cpu()[:rows], out[1].cpu()
    assert int(torch.isnan(want_hi).sum()) == 2 and _same_or_both_nan(hi, want_hi)
    ok = ~torch.isnan(x32)
    assert torch.equal(lo_plane_values(lo, rows, D)[ok], lo_plane_values(want_lo, rows, D)[ok])
    if hdt == torch.float16:
        assert int((hi.abs() == F16_MAX).sum()) > 100 and int(((x32 > 65504) & (x32 < 65520)).sum()) > 0


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_one_nan_pixel_poisons_its_image_and_no_other(dtype, engines):
    """tiny model, batch of 6: a NaN pixel in image 2 makes image 2's embedding NaN and leaves the other five bit-identical to the clean
    batch -- eager and on graph replay (the third call of a shape replays)"""
    model, cfg, sd, px, ids, mask = engines("tiny_b6", dtype)
    eng = model.engine
    clean_px = torch.from_numpy(px).clone()
    bad_px = clean_px.clone()
    bad_px[2, 1, 5, 7] = float("nan")
    keep = [0, 1, 3, 4, 5]
    try:
        for graph in (0, 32):
            eng.set_graph_batch(graph)
            for rep in range(4 if graph else 1):
                clean = eng.encode_image(clean_px.clone()).clone()
                bad = eng.encode_image(bad_px.clone()).clone()
                torch.cuda.synchronize()
                assert torch.isfinite(clean).all()
                assert torch.isnan(bad[2]).all(), (dtype, graph, rep, bad[2])
                assert torch.equal(_bits(bad[keep]), _bits(clean[keep])), (dtype, graph, rep)
    finally:
        eng.set_graph_batch(32)
