"""The exact-GELU epilogues (gemm.h EPI_BIAS_GELU / EPI_GELU_LN) one kernel at a time through ``kernel_entries.gemm_nt_gelu``, by the
method of tests/test_gpu_value_range.py: M = 331 x N = 512 x K = 256 (a ragged last row tile on every tile height, two 256-column
tiles, four 16-bit K tiles), the output allocated with sentinel-filled guard rows, every tile 0 .. 6, the cost model's (-1), the naive
checker (-2) and the small-M split-K kernel (-3).

The kernel's own fp32 pre-activation ``y32`` comes from the existing entry ``gemm_nt(..., epilogue=2, out=zeros)`` on the same operands
and variant (same K loop, same fp32 add); the reference is float64 ``0.5 * y * (1 + erf(y / sqrt 2))`` of ``y32``.  Operands: rows of A
scaled 0.25 / 1 / 2.5, exactly zero, 2^-30 (f16: 2^-13) and LARGE (2^50; f16: 2^11), columns of W scaled 1 / 2 / 2^-13 / LARGE (2^50;
f16: 2^9) -- most of the outputs lie densely in [-8, 8], the rest are +0 (fp32 accumulation from +0 cannot produce a -0
pre-activation; the negative zeros are on the OUTPUT side: tiny negative pre-activations whose result rounds to -0 in f16), 1e-8 and
smaller, and magnitudes out to 1e30 (f16: far past 65504).

Bounds:
  * 16-bit outputs: finite; within ONE unit in the last place of ``round_to(float64 value)``; exactly +-65504 where the reference reaches
    +-65520.  One allowance, only where y32 < -3: a difference of at most |y32| * 2^-21 -- the noise of the formula HF itself runs in
    fp32 (torch.nn.functional.gelu in fp32 against float64 on 200 001 points of [-8, 8]: 3.32e-7 |y| = 2^-21.5 |y|, from ``1 + erf``
    cancelling; past y = -5.5 that reference returns -0).  The test prints the ulp histogram and how many elements used the allowance.
  * fp32 outputs: |got - ref| <= |y32| * 2^-21 + 8 * 2^-24 * |ref| + 2^-120, finite.
  * ln = 1: the statistics cases of the existing folded-epilogue test (constant, very wide and ordinary rows) and its per-element bound
    LN_RND x (rstd |A| |W|^T + |c2|) + half the smallest spacing, on the pre-activation, carried through the activation's slope (at most
    1.13); exactly +-65504 where the reference saturates.
Every test prints ``PARITY`` lines; profiles/gelu_parity.txt keeps them."""
import functools
import math

import pytest
import torch

import small_kernel_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
TILES = list(range(7))
M, N, K = 331, 512, 256
GUARD = 21
EPS = 1e-5
SENT = 0xA5
F16_MAX, F16_SAT = 65504.0, 65520.0
LN_RND = {torch.bfloat16: 6e-3, torch.float16: 8e-4}                      # test_gpu_gemm.py test_layernorm_folded_consumer_epilogue
HALF_SPACING = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
GELU_SLOPE = 1.13                                                         # max |d gelu / dy| = 1.1290 at y = 1.41
ALLOW = 2.0 ** -21

PLAIN_CASES = [(d, v) for d in DT for v in TILES + [-1, -2, -3] if not (d == "f32" and v == -3)]
LN_CASES = [(h, v) for h in HALF for v in TILES + [-1, -3]]


def gelu64(y):
    y = y.double()
    return 0.5 * y * (1.0 + torch.special.erf(y / math.sqrt(2.0)))


@functools.lru_cache(maxsize=None)
def _operands(dname):
    """On the CPU, computed once, never written to."""
    dt = DT[dname]
    g = torch.Generator().manual_seed(777)
    big_a, big_w = (2.0 ** 11, 2.0 ** 9) if dt == torch.float16 else (2.0 ** 50, 2.0 ** 50)
    tiny_a = 2.0 ** -13 if dt == torch.float16 else 2.0 ** -30          # (2^-30 is below f16's subnormals)
    sa = torch.tensor([0.25, 1.0, 2.5, 1.0, 0.0, tiny_a, big_a, 1.0])[torch.arange(M) % 8]
    sw = torch.tensor([1.0, 1.0, 2.0, 2.0 ** -13, 1.0, 1.0, 1.0, big_w])[torch.arange(N) % 8]
    a = (torch.randn(M, K, generator=g) * sa[:, None]).to(dt)
    w = (torch.randn(N, K, generator=g) / 16 * sw[:, None]).to(dt)
    bias = torch.randn(N, generator=g) * 0.5
    bias[1::2] = -0.0
    bias = bias.to(dt).float()
    assert torch.isfinite(a).all() and torch.isfinite(w).all()
    acc = a.double() @ w.double().T
    mag = a.double().abs() @ w.double().abs().T
    # the statistics of tests/test_gpu_value_range.py: a third of the rows constant (rstd = eps^-1/2), a third very wide, a third ordinary
    st = torch.zeros(M, K // 64, 2)
    rows = torch.arange(M)
    st[:, :, 0] = torch.randn(M, K // 64, generator=g) * 8.0
    st[:, :, 1] = 64.0 * (0.5 + torch.rand(M, K // 64, generator=g))
    const, wide = rows % 3 == 0, rows % 3 == 1
    st[const, :, 0] = (64.0 * ((rows[const] % 7) - 3).float())[:, None]
    st[const, :, 1] = 0.0
    st[wide, :, 0] = 0.0
    st[wide, :, 1] = 2.5e11
    s64 = st.double()
    mean = s64[..., 0].sum(-1) / K
    m2 = s64[..., 1].sum(-1) + (64.0 * (s64[..., 0] / 64.0 - mean[:, None]) ** 2).sum(-1)
    rstd = 1.0 / torch.sqrt(m2 / K + EPS)
    assert (rstd[const] == EPS ** -0.5).all() and (rstd[wide] < 2e-5).all()
    return dict(a=a, w=w, bias=bias, acc=acc, mag=mag, st=st, rstd=rstd[:, None])


@functools.lru_cache(maxsize=None)
def _dev(dname):
    d = _operands(dname)
    return {k: d[k].to(DEV) for k in ("a", "w", "bias", "st")}


def _guarded(dt):
    size = torch.empty((), dtype=dt).element_size()
    full = torch.full((M + GUARD, N * size), SENT, dtype=torch.uint8, device=DEV).view(dt)
    return full, full[:M]


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == SENT).all())


def test_the_pre_activations_cover_every_class():
    """counted on the float64 pre-activation of each type's operands: a change of inputs cannot empty a class unnoticed"""
    for dname in DT:
        d = _operands(dname)
        y = d["acc"] + d["bias"].double()
        dense = (y.abs() <= 8) & (y != 0)
        hist = torch.histc(y[dense].float(), bins=32, min=-8, max=8)
        neg_tail = int(((y < -3) & (y > -8)).sum())
        zeros, tiny_neg = int((y == 0).sum()), int(((y < 0) & (y > -1e-6)).sum())
        largest = float(y.abs().max())
        print(f"\nPARITY group=gelu_classes case={dname} dense={int(dense.sum())} emptiest_bin={int(hist.min())} in(-8,-3)={neg_tail} "
              f"zeros={zeros} tiny_negative={tiny_neg} largest={largest:.2e}")
        assert int(dense.sum()) > M * N // 2 and int(hist.min()) >= 20 and neg_tail > 1000 and zeros > 5000 and tiny_neg > 1000
        assert largest > (1e6 if dname == "f16" else 1e30)
        if dname == "f16":
            assert int((gelu64(y).abs() >= F16_SAT).sum()) > 1000


def _check_16bit(case, dt, got, y32):
    ref = gelu64(y32)
    want = R.round_to(ref, dt)
    assert torch.isfinite(got).all(), case
    dist = (R.ord16(got) - R.ord16(want)).reshape(-1)
    hist = {int(k): int((dist == k).sum()) for k in torch.unique(dist)}
    beyond = dist.abs() > 1
    allowed = beyond & (y32.reshape(-1) < -3.0) & ((got.double() - want.double()).abs().reshape(-1) <= y32.double().abs().reshape(-1) * ALLOW)
    near = {k: v for k, v in hist.items() if abs(k) <= 1}
    print(f"\nPARITY group=gelu_ulps case={case} bound=1 histogram={near} beyond={int(beyond.sum())} used_the_allowance={int(allowed.sum())}")
    bad = beyond & ~allowed
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError((case, hist, float(y32.reshape(-1)[i]), float(got.reshape(-1)[i]), float(ref.reshape(-1)[i])))
    if dt == torch.float16:
        sat = ref.abs() >= F16_SAT
        assert int(sat.sum()) > 1000 and torch.equal(got[sat].double(), torch.sign(ref[sat]) * F16_MAX), case
        assert int(((got == 0) & torch.signbit(got)).sum()) > 500, case         # negative zeros on the output side


@pytest.mark.parametrize("dname,variant", PLAIN_CASES, ids=[f"{d}-v{v}" for d, v in PLAIN_CASES])
def test_gelu_epilogue_against_float64_of_the_kernels_own_pre_activation(dname, variant):
    from plip_amd.kernel_entries import gemm_nt, gemm_nt_gelu
    dt, g = DT[dname], _dev(dname)
    case = f"{dname}_v{variant}"
    y32 = gemm_nt(g["a"], g["w"], g["bias"], epilogue=2, variant=variant, out=torch.zeros(M, N, device=DEV))
    full, out = _guarded(dt)
    gemm_nt_gelu(g["a"], g["w"], g["bias"], variant=variant, out=out)
    torch.cuda.synchronize()
    assert _untouched(full[M:]), case
    y32, got = y32.cpu(), out.cpu()
    assert torch.isfinite(y32).all()
    if dt != torch.float32:
        _check_16bit(case, dt, got, y32)
        return
    ref = gelu64(y32)
    tol = y32.double().abs() * ALLOW + 8.0 * 2.0 ** -24 * ref.abs() + 2.0 ** -120
    assert torch.isfinite(got).all(), case
    ratio = float(((got.double() - ref).abs() / tol).max())
    print(f"\nPARITY group=gelu_fp32 case={case} bound=1.000e+00 gpu={ratio:.3e}")
    assert ratio <= 1.0, (case, ratio)


@pytest.mark.parametrize("hname,variant", LN_CASES, ids=[f"{h}-v{v}" for h, v in LN_CASES])
def test_layernorm_folded_gelu_epilogue(hname, variant):
    from plip_amd.kernel_entries import gemm_nt_gelu
    hdt, d, g = HALF[hname], _operands(hname), _dev(hname)
    case = f"{hname}_v{variant}_ln"
    full, out = _guarded(hdt)
    gemm_nt_gelu(g["a"], g["w"], g["bias"], g["st"], eps=EPS, variant=variant, out=out)
    torch.cuda.synchronize()
    assert _untouched(full[M:]), case
    y = out.cpu()
    v = d["rstd"] * d["acc"] + d["bias"].double()
    bound = d["rstd"] * d["mag"] + d["bias"].double().abs()
    ref = gelu64(v)
    want = ref.clamp(-F16_MAX, F16_MAX) if hdt == torch.float16 else ref
    assert torch.isfinite(y).all(), case
    tol = GELU_SLOPE * LN_RND[hdt] * bound + HALF_SPACING[hdt]
    r = (y.double() - want).abs() / tol
    ratio, at = float(r.max()), int(r.argmax())
    print(f"\nPARITY group=gelu_ln_folded case={case} bound=1.000e+00 gpu={ratio:.3e}")
    m, n = at // N, at % N
    assert ratio <= 1.0, (case, ratio, (m, n), float(y[m, n]), float(want[m, n]), float(v[m, n]), float(bound[m, n]))
    if hdt == torch.float16:
        sat = ref.abs() >= F16_SAT * (1 + 1e-5)
        assert int(sat.sum()) > 1000 and torch.equal(y[sat].double(), torch.sign(ref[sat]) * F16_MAX), case


def test_bad_arguments_are_refused_with_a_message():
    from plip_amd import _lib
    from plip_amd.kernel_entries import gemm_nt_gelu
    a32, w32 = torch.zeros(8, 256, device=DEV), torch.zeros(128, 256, device=DEV)
    ah, wh = a32.to(torch.bfloat16), w32.to(torch.bfloat16)
    bias, st = torch.zeros(128, device=DEV), torch.zeros(8, 4, 2, device=DEV)
    with pytest.raises(_lib.PlipmiError, match="16-bit"):
        gemm_nt_gelu(a32, w32, bias, st)                          # fp32 with ln = 1
    with pytest.raises(_lib.PlipmiError, match="null pointer"):
        gemm_nt_gelu(ah, wh, None)
    with pytest.raises(_lib.PlipmiError, match="variant -2"):
        gemm_nt_gelu(ah, wh, bias, st, variant=-2)
    with pytest.raises(_lib.PlipmiError, match="statistics"):
        gemm_nt_gelu(ah, wh, bias, None, ln=True)
    with pytest.raises(_lib.PlipmiError, match="variant -3"):
        gemm_nt_gelu(a32, w32, bias, variant=-3)
    # the neighbour keeps its range: the new kinds are not reachable through it
    from plip_amd.kernel_entries import gemm_nt
    with pytest.raises(_lib.PlipmiError, match="epilogue must be 0..3"):
        gemm_nt(ah, wh, bias, epilogue=9)
