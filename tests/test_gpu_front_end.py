"""Kernel-level tests of the code that FEEDS the towers and the code that SHORTENS them, on the MI355X, one kernel at a time through
include/plipmi_test.h (plip_amd/kernel_entries.py):

  the vision front end (csrc/towers.hip vision_embed) -- the unfold kernels (vector, scalar, uint8), cls_rows, the patch GEMM's
  EPI_PATCH scatter on every tile, the two im2col-on-load kernels (gemm.h ADDR 2 / 3) at batches the cost model would never give them,
  the GEMM on padded leading dimensions (what the patch GEMM runs with when K < Kpad);
  the packed-caption mechanisms -- GemmParams.m_dev (the live row count read on the device) and the `cu` argument of the
  short-sequence MFMA attention kernel.

References: tests/small_kernel_refs.py unfold_ref / patch_embed_ref (conv2d in float64 on the rounded operands) / u8_norm_ref, pinned on
the CPU by tests/test_small_kernel_refs_host.py; float64 softmax of each caption alone (small_kernel_refs.attention_probs).  Index maps
are checked EXACTLY (bit for bit) wherever the operation is a re-index or two routes promise the same bits; sums are checked with the
project's own bounds for the same quantities: 2e-4 on the fp32 output of an MFMA GEMM with operands A ~ N(0, 1), W ~ N(0, 1) / sqrt(K)
(test_gpu_gemm.py _half_tol), 3e-2 (bf16) / 4e-3 (f16) on the MFMA attention output (test_gpu_attention.py).

Every output buffer starts as the sentinel byte 0xA5 with guard rows behind it; whatever a call does not own must still hold it.
Every test prints ``PARITY`` lines; profiles/front_end_parity.txt keeps the worst figure per group."""
import functools

import pytest
import torch

import small_kernel_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
TILES = list(range(7))                                                    # csrc/gemm_inst.h; -2 = the naive checker kernel
GEMM_TOL = 2e-4                                                           # test_gpu_gemm.py _half_tol, fp32 outputs
ATT_TOL = {"bf16": 3e-2, "f16": 4e-3}                                     # test_gpu_attention.py, MFMA kernels
SENT = 0xA5
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sent(rows, cols, dtype, device=DEV):
    """[rows, cols] of ``dtype``, every byte the sentinel (a finite value in every type used here)"""
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full((rows, cols * size), SENT, dtype=torch.uint8, device=device).view(dtype)


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == SENT).all())


def _bits(t):
    t = t.contiguous()
    return t.view(_INT[t.element_size()])


def _parity(group, case, bound, err):
    print(f"\nPARITY group={group} case={case} bound={bound:.3e} gpu={err:.3e}")


def _tiles(B, H, W, P, seed):
    """uint8 HWC tiles whose bytes inside the patch grid take all 256 values in each channel"""
    g = _gen(seed)
    t = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    gh, gw = H // P, W // P
    for c in range(3):
        where = torch.randperm(gh * P * gw * P, generator=g)[:256]
        t[0, where // (gw * P), where % (gw * P), c] = torch.randperm(256, generator=g).to(torch.uint8)
        assert t[:, :gh * P, :gw * P, c].unique().numel() == 256
    return t


def _pixels(B, H, W, P, seed):
    """fp32 NCHW pixels; the remainder rows / columns the floored grid leaves out are NaN: one read of them poisons a result"""
    px = torch.randn(B, 3, H, W, generator=_gen(seed))
    px[:, :, H // P * P:, :] = float("nan")
    px[:, :, :, W // P * P:] = float("nan")
    return px


def _in_grid(px, P):
    return px[:, :, :px.shape[2] // P * P, :px.shape[3] // P * P]


# =====================================================================================================================================
# unfold_kernel<vector / scalar>, unfold_u8_kernel (csrc/tower_kernels.hip): a re-index, so exact
# =====================================================================================================================================
UNFOLD_CASES = [(32, 64, 96),      # vector path
                (16, 52, 72),      # vector path; the grid floors (3 x 4): the remainder pixels must not appear
                (16, 48, 50),      # W % 4 != 0: scalar path with a 16-pixel patch
                (14, 30, 44),      # scalar path, K = 588 < Kpad = 640
                (15, 31, 47)]      # K = 675, K % 4 == 3: the four-wide store straddles K; Kpad = 704


@pytest.mark.parametrize("source", ["f32", "u8"])
@pytest.mark.parametrize("P,H,W", UNFOLD_CASES)
def test_unfold_is_the_exact_reindex(P, H, W, source):
    """Row (b, gi, gj), column (c, u, v), zeros in columns K .. Kpad, for fp32 / bf16 / f16 outputs: the bits of unfold_ref rounded with
    torch's RNE conversion.  uint8 tiles: of the fp32 three-rounding mirror u8_norm_ref ((b / 255 - mean) * (1 / std), each step fp32),
    on tiles holding all 256 byte values in each channel -- the GPU half of test_host.py's one-fma proof."""
    from plip_amd.kernel_entries import patch_kpad, unfold_patches
    B, K, kpad = 3, 3 * P * P, patch_kpad(P)
    assert kpad == {32: 3072, 16: 768, 14: 640, 15: 704}[P]
    rows = B * (H // P) * (W // P)
    if source == "u8":
        src = _tiles(B, H, W, P, 11 * P + W)
        want32 = R.unfold_ref(R.u8_norm_ref(src), P, kpad)
    else:
        src = _pixels(B, H, W, P, 7 * P + W)
        want32 = R.unfold_ref(src, P, kpad)
    assert torch.isfinite(want32).all() and (want32[:, K:] == 0).all()
    src = src.to(DEV)
    for dname, dt in DT.items():
        out = _sent(rows + 2, kpad, dt)
        unfold_patches(src, out, P, kpad)
        torch.cuda.synchronize()
        got, want = out.cpu(), want32.to(dt)
        bad = int((_bits(got[:rows]) != _bits(want)).sum())
        _parity(f"unfold_{source}", f"P{P}_{H}x{W}_{dname}", 0.0, float(bad))
        assert bad == 0, f"{source} -> {dname}, P={P} {H}x{W}: {bad} elements differ from the re-index (max |diff| " \
                         f"{(got[:rows].double() - want.double()).abs().max().item():.3e})"
        assert _untouched(got[rows:]), "the unfold pass wrote past its last patch row"


# =====================================================================================================================================
# cls_rows_kernel
# =====================================================================================================================================
@pytest.mark.parametrize("tokens", [1, 13])
@pytest.mark.parametrize("D", [128, 768])
def test_cls_rows_writes_row_zero_of_each_image_only(D, tokens):
    from plip_amd.kernel_entries import cls_rows
    B, g = 3, _gen(D + tokens)
    cls, pos = torch.randn(D, generator=g), torch.randn(tokens, D, generator=g)
    x = _sent(B * tokens + 1, D, torch.float32)
    cls_rows(cls.to(DEV), pos.to(DEV), x, B, tokens)
    torch.cuda.synchronize()
    got = x.cpu()
    want = cls + pos[0]                                                    # one fp32 add per element: exact
    for b in range(B):
        assert torch.equal(_bits(got[b * tokens]), _bits(want)), b
    other = torch.ones(B * tokens + 1, dtype=torch.bool)
    other[torch.arange(B) * tokens] = False
    assert _untouched(got[other])


# =====================================================================================================================================
# the patch GEMM's EPI_PATCH epilogue on every tile
# =====================================================================================================================================
# (P, H, W, B, N): np = 12 on a floored 3 x 4 grid, B = 30 -> M = 360: every tile height (128 / 160 / 192 / 256 / 320) ends inside an
# image and leaves a partial last tile; np = 1: CLS and patch rows alternate; P = 14: K = 588 inside lda = ldw = Kpad = 640, the padding
# columns zero in A and in W as the engine has them; P = 32: K = 3072, M = 42 in one partial tile.
# The small-M split-K kernel (variant -3, the latency path's patch GEMM; 16-bit types, K % 256 == 0) has 32-row tiles: M = 360 puts
# their borders inside images and leaves a partial last one, M = 42 one whole and one partial; K = 768 is one pass of its (4, 3) form,
# K = 3072 two of (8, 3)
PATCH_SHAPES = {"np12": (16, 52, 72, 30, 256), "np1": (16, 16, 16, 5, 256), "np12_n512": (16, 52, 72, 30, 512),
                "np12_k588": (14, 44, 58, 30, 256), "p32_b7": (32, 64, 96, 7, 256)}


def _patch_operands(P, H, W, B, N, dt, seed):
    """(rounded pixels, A [B * np, Kpad] = their unfolded rows, w [N, Kpad], pos fp32 [np + 1, N], float64 reference [B, np + 1, N])"""
    from plip_amd.kernel_entries import patch_kpad
    g = _gen(seed)
    K, kpad = 3 * P * P, patch_kpad(P)
    px = _in_grid(torch.randn(B, 3, H, W, generator=g), P).to(dt)
    w = torch.zeros(N, kpad, dtype=dt)
    w[:, :K] = (torch.randn(N, K, generator=g) / K ** 0.5).to(dt)
    pos = torch.randn((H // P) * (W // P) + 1, N, generator=g)
    return px, R.unfold_ref(px, P, kpad), w, pos, R.patch_embed_ref(px, w[:, :K], P, pos)


def _check_token_rows(got, ref, np_, group, case):
    """got fp32 [B * (np + 1) + guard, N] on the host: patch rows within the GEMM bound of ref, CLS rows and guard rows untouched"""
    B = ref.shape[0]
    rows = got[:B * (np_ + 1)].reshape(B, np_ + 1, -1)
    assert _untouched(rows[:, 0]), f"{case}: a CLS row was written"
    assert _untouched(got[B * (np_ + 1):]), f"{case}: a row past the last image was written"
    diff = (rows[:, 1:].double() - ref[:, 1:]).abs()
    assert torch.isfinite(diff).all(), case
    err = diff.max().item()
    _parity(group, case, GEMM_TOL, err)
    assert err < GEMM_TOL, f"{case}: max err {err:.3e}"
    return err


@pytest.mark.parametrize("shape", list(PATCH_SHAPES))
@pytest.mark.parametrize("dname", list(DT))
def test_patch_epilogue_scatters_patch_rows_to_token_rows(dname, shape):
    """Patch row img * np + p lands in token row img * (np + 1) + 1 + p with position row 1 + p added, on every tile and the naive kernel,
    against conv2d in float64; for the 16-bit types every tile gives tile 0's bits (test_every_tile_sums_k_in_the_same_order).
    The small-M split-K kernel (-3) is held to the same convolution where it applies (its K order differs: no bit claim) and must
    refuse, before it launches anything, fp32 operands and a K that is no multiple of 256."""
    from plip_amd._lib import PlipmiError
    from plip_amd.kernel_entries import gemm_patch
    P, H, W, B, N = PATCH_SHAPES[shape]
    dt = DT[dname]
    px, a, w, pos, ref = _patch_operands(P, H, W, B, N, dt, 500 + P + N + B)
    np_ = pos.shape[0] - 1
    assert a.shape == (B * np_, w.shape[1]) and (P != 14 or ((a[:, 588:] == 0).all() and a.shape[1] == 640))
    a, w, pos = a.to(DEV), w.to(DEV), pos.to(DEV)
    first, worst = None, 0.0
    for v in TILES + [-2]:
        out = _sent(B * (np_ + 1) + 2, N, torch.float32)
        gemm_patch(a, w, pos, out, variant=v)
        torch.cuda.synchronize()
        got = out.cpu()
        worst = max(worst, _check_token_rows(got, ref, np_, f"epi_patch_{dname}", f"{shape}_tile{v}"))
        if dt != torch.float32 and v >= 0:
            if first is None:
                first = got
            assert torch.equal(_bits(got), _bits(first)), f"tile {v} differs from tile 0: {shape} {dname}"
    out = _sent(B * (np_ + 1) + 2, N, torch.float32)
    if dt != torch.float32 and a.shape[1] % 256 == 0:
        gemm_patch(a, w, pos, out, variant=-3)
        torch.cuda.synchronize()
        worst = max(worst, _check_token_rows(out.cpu(), ref, np_, f"epi_patch_{dname}", f"{shape}_tile-3"))
    else:
        with pytest.raises(PlipmiError, match="16-bit operands" if dt == torch.float32 else "K % 256 == 0"):
            gemm_patch(a, w, pos, out, variant=-3)
        torch.cuda.synchronize()
        assert _untouched(out), f"{shape} {dname}: the refused small-M call wrote"
    assert worst < GEMM_TOL


# =====================================================================================================================================
# im2col on load (gemm.h ADDR 2 / 3), at batches the cost model never picks the ring tile for
# =====================================================================================================================================
# (P, H, W, B, N): floored 3 x 4 grid, M = 360, a partial last ring tile; M = 42 in one partial tile with K = 3072; np = 1
GATHER_SHAPES = {"p16_b30": (16, 52, 72, 30, 256), "p32_b7": (32, 64, 96, 7, 256), "p16_np1": (16, 16, 16, 5, 256),
                 "p16_b30_n512": (16, 52, 72, 30, 512)}


@pytest.mark.parametrize("shape", list(GATHER_SHAPES))
@pytest.mark.parametrize("source", ["f32", "u8"])
@pytest.mark.parametrize("dname", list(HALF))
def test_gathering_patch_gemm_gives_the_unfold_pass_and_plain_gemm_bits(dname, source, shape):
    """vision_embed's claim: the patch GEMM that gathers its A operand from the pixels (fp32 NCHW / uint8 HWC tiles with the one-fma
    normalisation) writes the embedding rows the unfold pass + the plain patch GEMM on the ring tile write, bit for bit -- and both are
    the convolution."""
    from plip_amd.kernel_entries import gemm_patch, gemm_patch_gather, unfold_patches
    P, H, W, B, N = GATHER_SHAPES[shape]
    dt, K = HALF[dname], 3 * P * P
    np_, seed = (H // P) * (W // P), 900 + P + B + N
    g = _gen(seed)
    if source == "u8":
        src = _tiles(B, H, W, P, seed)
        px = R.u8_norm_ref(src)
    else:
        src = _pixels(B, H, W, P, seed)
        px = src
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dt)
    pos = torch.randn(np_ + 1, N, generator=g)
    ref = R.patch_embed_ref(_in_grid(px, P).to(dt), w, P, pos)
    src, w, pos = src.to(DEV), w.to(DEV), pos.to(DEV)
    out = _sent(B * (np_ + 1) + 2, N, torch.float32)
    gemm_patch_gather(src, w, pos, out, P)
    a = _sent(B * np_ + 1, K, dt)
    unfold_patches(src, a, P, K)
    two = _sent(B * (np_ + 1) + 2, N, torch.float32)
    gemm_patch(a[:B * np_], w, pos, two, variant=6)
    torch.cuda.synchronize()
    got, two = out.cpu(), two.cpu()
    case = f"{shape}_{source}"
    _check_token_rows(two, ref, np_, f"gather_two_pass_{dname}", case)
    _check_token_rows(got, ref, np_, f"gather_{dname}", case)
    bad = int((_bits(got) != _bits(two)).sum())
    assert bad == 0, f"{case} {dname}: {bad} elements differ between the gathering GEMM and unfold + patch GEMM on the ring tile"


def test_gathering_patch_gemm_refuses_what_it_cannot_address():
    from plip_amd._lib import PlipmiError
    from plip_amd.kernel_entries import gemm_patch_gather
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    for P, H, W, N, dt, text in ((16, 48, 50, 256, torch.bfloat16, "width % 4"),          # a row of pixels is not whole 16-byte loads
                                 (16, 48, 48, 128, torch.bfloat16, "256-column"),         # N % 256 != 0
                                 (14, 28, 28, 256, torch.float16, "patch 14"),
                                 (16, 48, 48, 256, torch.float32, "16-bit-engine")):
        np_ = (H // P) * (W // P)
        out = _sent(2 * (np_ + 1), N, torch.float32)
        for src in (z(2, 3, H, W), z(2, H, W, 3, dt=torch.uint8)):
            with pytest.raises(PlipmiError, match=text):
                gemm_patch_gather(src, z(N, 3 * P * P, dt=dt), z(np_ + 1, N), out, P)
        assert _untouched(out)


# =====================================================================================================================================
# padded leading dimensions (plipmi_gemm_nt_ld): lda = Kpad != K is what the patch GEMM runs with
# =====================================================================================================================================
@pytest.mark.parametrize("M,N,K", [(37, 256, 64), (300, 256, 192), (515, 512, 768)])
@pytest.mark.parametrize("dname", list(DT))
def test_padded_leading_dimensions_read_k_columns_and_no_more(dname, M, N, K):
    """A [M, K + 8], W [N, K + 24] with NaN in the padding columns, every tile and the naive kernel, epilogues 0 .. 3: the bits of the
    same kernel on contiguous copies of the first K columns (same summation order: no tolerance) -- one read past column K poisons
    the output."""
    from plip_amd.kernel_entries import gemm_nt, gemm_nt_ld
    dt, g = DT[dname], _gen(M + K)
    a = torch.full((M, K + 8), float("nan"))
    w = torch.full((N, K + 24), float("nan"))
    a[:, :K] = torch.randn(M, K, generator=g)
    w[:, :K] = torch.randn(N, K, generator=g) / K ** 0.5
    a, w = a.to(DEV).to(dt), w.to(DEV).to(dt)
    ac, wc = a[:, :K].contiguous(), w[:, :K].contiguous()
    bias, c0 = torch.randn(N, generator=g).to(DEV), torch.randn(M, N, generator=g).to(DEV)
    for epi in range(4):
        odt = dt if epi < 2 else torch.float32
        for v in TILES + [-2]:
            buf = _sent(M + 1, N, odt)
            if epi == 2:
                buf[:M] = c0
            y = gemm_nt_ld(a, w, K, bias, epilogue=epi, variant=v, alpha=0.37, out=buf[:M])
            want = gemm_nt(ac, wc, bias, epilogue=epi, variant=v, alpha=0.37, out=c0.clone() if epi == 2 else None)
            assert torch.isfinite(y).all(), f"tile {v} epi {epi}: a padding column was read"
            assert torch.equal(_bits(y), _bits(want)), f"tile {v} epi {epi} {M}x{N}x{K} {dname}"
            assert _untouched(buf[M:])
    _parity(f"leading_dims_{dname}", f"{M}x{N}x{K}", 0.0, 0.0)


# =====================================================================================================================================
# GemmParams.m_dev: the live row count read on the device (the packed text tower's q/k/v, out-proj, fc1, fc2)
# =====================================================================================================================================
ROWS_M, ROWS_N, ROWS_K, ROWS_GUARD = 700, 512, 256, 36                    # 736 rows allocated: two whole 16-row lo bands of guard
TILE_ROWS = {0: 128, 1: 128, 2: 256, 3: 320, 4: 192, 5: 160, 6: 160, -1: 128}   # -1: the cost model's tile at M <= 1024 is tile 0


def _live_rows(bm):
    return [0, 1, bm - 1, bm, bm + 1, 699, 700, 900]


@functools.lru_cache(maxsize=None)
def _rows_inputs(dname):
    from plip_amd.kernel_entries import lo_plane_index, split_planes
    hdt, g = HALF[dname], _gen(4242)
    Mt = ROWS_M + ROWS_GUARD
    x = torch.randn(Mt, ROWS_K, generator=g) + 1.5
    w = (torch.randn(ROWS_N, ROWS_K, generator=g) / ROWS_K ** 0.5).to(hdt)
    bias = torch.randn(ROWS_N, generator=g) * 0.1
    x0 = (torch.randn(Mt, ROWS_N, generator=g) * 3.0 + 1.0).to(DEV)
    hi0, lo0 = split_planes(x0, hdt)
    return dict(a=x.to(hdt).to(DEV), w=w.to(DEV), bias=bias.to(DEV), stats=R.slice_stats(x).to(DEV), hi0=hi0, lo0=lo0,
                idx=lo_plane_index(Mt, ROWS_N, DEV))


def _run_rows(mode, dname, v, m):
    """One launch with m live rows on a grid sized for ROWS_M, outputs pre-filled with the sentinel past the live rows, and the same call
    with M = min(m, ROWS_M) and no m_dev.  Returns (live rows, the outputs, the plain call's outputs); lo planes come with idx."""
    from plip_amd.kernel_entries import gemm_nt_ln_rows
    d = _rows_inputs(dname)
    hdt, Mt, mm = HALF[dname], ROWS_M + ROWS_GUARD, min(m, ROWS_M)
    md = torch.tensor([m], dtype=torch.int32, device=DEV)
    if mode in (0, 1):
        c, cr = _sent(Mt, ROWS_N, hdt), torch.zeros(Mt, ROWS_N, dtype=hdt, device=DEV)
        gemm_nt_ln_rows(mode, d["a"], d["w"], d["bias"], md, c, stats=d["stats"], M=ROWS_M, variant=v)
        gemm_nt_ln_rows(mode, d["a"], d["w"], d["bias"], None, cr, stats=d["stats"], M=mm, variant=v)
        return mm, dict(C=c), dict(C=cr)
    hi, lo = d["hi0"].clone(), d["lo0"].clone()
    hi.view(torch.int16)[mm:] = SENT * 257 - 65536                         # bytes A5 A5
    lo[d["idx"][mm:].reshape(-1)] = SENT
    st = _sent(Mt, ROWS_N // 64 * 2, torch.float32).view(Mt, ROWS_N // 64, 2)
    hir, lor, str_ = d["hi0"].clone(), d["lo0"].clone(), torch.zeros(Mt, ROWS_N // 64, 2, device=DEV)
    gemm_nt_ln_rows(mode, d["a"], d["w"], d["bias"], md, (hi, lo), st=st, M=ROWS_M, variant=v)
    gemm_nt_ln_rows(mode, d["a"], d["w"], d["bias"], None, (hir, lor), st=str_, M=mm, variant=v)
    return mm, dict(hi=hi, st=st, lo=lo), dict(hi=hir, st=str_, lo=lor)


@pytest.mark.parametrize("mode", [0, 1, 3, 4])
@pytest.mark.parametrize("dname", list(HALF))
def test_device_row_count_computes_the_live_rows_and_writes_nothing_else(dname, mode):
    """For m in {0, 1, bm - 1, bm, bm + 1, 699, 700, 900} live rows on a 700-row grid, every tile and the cost model's: rows
    [0, min(m, 700)) of every output (C; hi plane, lo plane, statistics) are the bits of the same call made with M = min(m, 700) and no
    m_dev; every row past them keeps the sentinel -- for the lo plane here: every 16-row band past the last live one (the dead rows INSIDE
    a partly live band have their own test below).  m = 0 is safe by the code: every workgroup leaves at `if (m0 >= Mrt) return;`
    before it forms an address."""
    d = _rows_inputs(dname)
    problems = []
    for v in TILES + [-1]:
        for m in _live_rows(TILE_ROWS[v]):
            mm, got, ref = _run_rows(mode, dname, v, m)
            for name in got:
                if name == "lo":
                    live, dead = d["idx"][:mm].reshape(-1), d["idx"][(mm + 15) // 16 * 16:].reshape(-1)
                    same, clean = torch.equal(got[name][live], ref[name][live]), bool((got[name][dead] == SENT).all())
                else:
                    same, clean = torch.equal(_bits(got[name][:mm]), _bits(ref[name][:mm])), _untouched(got[name][mm:])
                if not same:
                    problems.append(f"tile {v} m={m}: live rows of {name} differ from the call with M={mm}")
                if not clean:
                    problems.append(f"tile {v} m={m}: {name} written past row {mm}")
    _parity(f"m_dev_mode{mode}_{dname}", "8_tiles_x_8_row_counts", 0.0, float(len(problems)))
    assert not problems, problems[:12]


@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("dname", list(HALF))
def test_device_row_count_leaves_the_dead_rows_of_a_partly_live_lo_band_alone(dname, mode):
    """The same launches, the bytes of rows min(m, 700) .. the end of their 16-row band in the blocked lo plane (lo_plane_index): dead
    rows, so they must keep the sentinel.

    The EPI_RESID_SPLIT epilogue (csrc/gemm.h) holds rows r and r + 8 of a band as ONE 16-byte piece of the lo plane.  It used to store the
    whole piece whenever row r was live, so with m live rows, m % 16 = j != 0, the dead rows 16 * (m / 16) + 8 + r for
    max(0, j - 8) <= r < min(j, 8) were written (m = 1: row 8; m = 127: row 127; m = 700: rows 700 .. 703 -- 48 of the 64 (tile, m)
    pairs here).  Nothing read those bytes before their rows were written again, so no embedding changed, but with a device-side row
    count they are real rows of the plane; the epilogue now stores only the live row's 8-byte half there."""
    d = _rows_inputs(dname)
    problems = []
    for v in TILES + [-1]:
        for m in _live_rows(TILE_ROWS[v]):
            mm, got, _ = _run_rows(mode, dname, v, m)
            band = d["idx"][mm:(mm + 15) // 16 * 16]
            hit = (got["lo"][band.reshape(-1)].reshape(band.shape) != SENT).any(dim=1)
            if bool(hit.any()):
                problems.append(f"tile {v} m={m}: dead rows {[mm + int(r) for r in hit.nonzero().reshape(-1)]} of the last live band written")
    _parity(f"m_dev_lo_band_mode{mode}_{dname}", "8_tiles_x_8_row_counts", 0.0, float(len(problems)))
    assert not problems, problems[:12]


def test_kernels_that_do_not_read_a_device_row_count_refuse_one():
    from plip_amd._lib import PlipmiError
    from plip_amd.kernel_entries import gemm_nt_ln_rows
    d = _rows_inputs("bf16")
    md = torch.tensor([5], dtype=torch.int32, device=DEV)
    c = _sent(ROWS_M + ROWS_GUARD, ROWS_N, torch.bfloat16)
    for v in (-2, -3):
        with pytest.raises(PlipmiError, match="does not read a device-side row count"):
            gemm_nt_ln_rows(0, d["a"], d["w"], d["bias"], md, c, stats=d["stats"], M=ROWS_M, variant=v)
    torch.cuda.synchronize()
    assert _untouched(c)


# =====================================================================================================================================
# packed rows in the short-sequence MFMA attention kernel (the `cu` argument)
# =====================================================================================================================================
PACKED = {"s77": (77, [1, 2, 31, 32, 33, 64, 65, 77]), "s128": (128, [96, 97, 128, 1])}


@pytest.mark.parametrize("use_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("causal", [False, True], ids=["dense", "causal"])
@pytest.mark.parametrize("shape", list(PACKED))
@pytest.mark.parametrize("dname", list(HALF))
def test_packed_attention_gives_the_padded_layouts_bits(dname, shape, causal, use_mask):
    """The kernel's promise: a caption's rows, packed back to back, get the result the padded [B, S] layout gives them with the keys past
    the caption's length masked -- bit for bit --, the tokenizer mask keeping its [B, S] layout; each caption within the MFMA bound of its
    own float64 softmax; nothing written past cu[B]."""
    from plip_amd.kernel_entries import attention, attention_packed
    S, lens = PACKED[shape]
    B, H, dt = len(lens), 2, HALF[dname]
    g = _gen(S + 2 * causal + use_mask)
    padded = torch.randn(B * S, 3 * H * 64, generator=g)                   # rows past a caption's length: other finite random values
    padded[:, :H * 64] *= 0.125 * 3.0                                      # q pre-scaled; x3 sharpens the softmax (test_gpu_attention.py)
    padded = padded.to(dt)
    tok = None
    if use_mask:
        tok = (torch.rand(B, S, generator=g) < 0.7).long()
        tok[:, 0] = 1                                                      # every query keeps a live key
    packed = torch.cat([padded[b * S:b * S + n] for b, n in enumerate(lens)])
    cu = torch.tensor([sum(lens[:b]) for b in range(B + 1)], dtype=torch.int32)
    total = int(cu[-1])
    out = _sent(total + 2, H * 64, dt)
    attention_packed(packed.to(DEV), out, cu.to(DEV), S, H, causal, None if tok is None else tok.to(DEV))
    in_len = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    want = attention(padded.to(DEV), B, S, H, causal, (in_len if tok is None else in_len * tok).to(DEV), impl=1)
    torch.cuda.synchronize()
    got, want = out.cpu(), want.cpu()
    assert _untouched(got[total:]), "rows past cu[B] were written"
    worst = 0.0
    for b, n in enumerate(lens):
        mine = got[int(cu[b]):int(cu[b]) + n]
        assert torch.equal(_bits(mine), _bits(want[b * S:b * S + n])), f"caption {b} (length {n}) differs from the padded layout"
        rows = padded[b * S:b * S + n]
        probs = R.attention_probs(rows, 1, n, H, causal, None if tok is None else tok[b:b + 1, :n])[0]            # [H, n, n]
        ref = (probs @ rows.double().reshape(n, 3, H, 64)[:, 2].permute(1, 0, 2)).permute(1, 0, 2).reshape(n, H * 64)
        diff = (mine.double() - ref).abs()
        assert torch.isfinite(diff).all()
        worst = max(worst, diff.max().item())
    _parity(f"packed_attention_{dname}", f"{shape}_{'causal' if causal else 'dense'}_{'mask' if use_mask else 'nomask'}", ATT_TOL[dname], worst)
    assert worst < ATT_TOL[dname], worst


def test_packed_attention_is_a_form_of_the_short_mfma_kernel_only():
    from plip_amd._lib import PlipmiError
    from plip_amd.kernel_entries import attention_packed
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    qkv = torch.zeros(4, 3 * 64, dtype=torch.bfloat16, device=DEV)
    out = _sent(5, 64, torch.bfloat16)
    with pytest.raises(PlipmiError, match="impl 1"):
        attention_packed(qkv, out, cu, 16, 1, impl=0)
    with pytest.raises(PlipmiError, match="S <= 128"):
        attention_packed(qkv, out, cu, 129, 1, impl=1)
    torch.cuda.synchronize()
    assert _untouched(out)
