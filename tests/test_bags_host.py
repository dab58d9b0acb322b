"""Host checks of the bag heads (plip_amd/bags.py, include/plipmi.h "bags of embeddings"): the oracle of tests/bags_common.py against an
independent statement of it, the two properties the GPU tests lean on, ``bag_offsets``, every validation error of bags.py, and the header /
binding / library / build agreement.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import bags_common as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle against an independent statement -----------------------------------------------------------------------------------
def _independent(scores_t, offsets, ks):
    """torch.topk values averaged in float64; a stable argsort of the negated keys for the indices"""
    s = np.asarray(scores_t, dtype=np.float64)
    S, Cn, kmax = len(offsets) - 1, s.shape[0], ks[-1]
    pooled = np.full((S, len(ks), Cn), np.nan, np.float32)
    top = np.full((S, Cn, kmax), -1, np.int32)
    for b in range(S):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if hi <= lo:
            continue
        seg = torch.from_numpy(s[:, lo:hi])
        for j, k in enumerate(ks):
            m = min(k, hi - lo)
            pooled[b, j] = (torch.topk(seg, m, dim=1).values.sum(dim=1, dtype=torch.float64) / m).numpy().astype(np.float32)
        for c in range(Cn):
            idx = np.argsort(-(s[c, lo:hi] + 0.0), kind="stable")[:kmax]
            top[b, c, :len(idx)] = lo + idx
    return pooled, top


def test_oracle_agrees_with_topk_means_and_a_stable_argsort():
    rng = np.random.default_rng(0)
    sizes = [0, 1, 3, 7, 0, 0, 40, 130, 0]
    off = BC.offsets_of(sizes)
    n = int(off[-1])
    # few distinct values: ties everywhere; both zeros in every bag
    s = rng.integers(-3, 4, size=(5, n)).astype(np.float32) * 0.25
    s[:, ::7] = -0.0
    s[:, 3::7] = 0.0
    for ks in ((1, 5, 10, 50, 100), (2,), (1, 200)):
        pooled, pred, top = BC.pool(s, off, ks)
        ip, it = _independent(s, off, ks)
        assert np.array_equal(top, it), ks
        ne = np.flatnonzero(np.diff(off) > 0)
        diff = np.abs(pooled[ne].astype(np.float64) - ip[ne]).max()
        print(f"ks {ks}: pooled vs topk means max diff {diff:.3e}")
        assert (np.abs(pooled[ne].astype(np.float64) - ip[ne]) <= BC.ulp32(ip[ne])).all()
        empty = np.flatnonzero(np.diff(off) == 0)
        assert np.isnan(pooled[empty]).all() and (pred[empty] == -1).all() and (top[empty] == -1).all()
        assert np.array_equal(pred[ne], np.argmax(pooled[ne], axis=2).astype(np.int32))      # first maximum
        for b in ne:                                   # k > n_b: the mean of the whole bag, -1 behind the bag's rows
            nb = sizes[b]
            assert (top[b, :, :min(nb, ks[-1])] >= off[b]).all() and (top[b, :, :min(nb, ks[-1])] < off[b + 1]).all()
            assert (top[b, :, nb:] == -1).all()
            if ks[-1] >= nb:
                want = s[:, off[b]:off[b + 1]].astype(np.float64).mean(axis=1)
                assert np.allclose(pooled[b, -1], want, rtol=0, atol=1e-6)


def test_oracle_order_ties_zeros_nan_and_inf():
    s = np.array([[1.0, np.nan, -np.inf, 0.0, -0.0, 1.0, np.inf, -0.0, 5e-45, -5e-45]], np.float32)
    off = np.array([0, 10], np.int32)
    pooled, pred, top = BC.pool(s, off, (1, 2, 10))
    assert top[0, 0].tolist() == [6, 0, 5, 8, 3, 4, 7, 9, 1, 2]        # NaN ranks as -inf: row 1 before row 2
    assert pooled[0, 0, 0] == np.inf and pred[0].tolist() == [0, 0, 0]
    finite = np.array([[1.0, 0.0, -0.0, 1.0, 5e-45]], np.float32)
    pooled, _, top = BC.pool(finite, np.array([0, 5], np.int32), (1, 3, 4))
    assert top[0, 0].tolist()[:4] == [0, 3, 4, 1] and pooled[0, :, 0].tolist() == [1.0, np.float32((2.0 + 5e-45) / 3), np.float32(0.5)]


# ---- the two properties the GPU tests lean on --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_scores():
    sizes = [n for n in BC.SIZES if n] + [3000]
    x, t = BC.random_case(512, 9, sizes, seed=3)
    off = BC.offsets_of(sizes)
    s64 = BC.scores64(x, t, 100.0)
    s32 = (np.float32(100.0) * (t @ x.T)).astype(np.float32)             # what fp32 arithmetic gives on the same inputs
    return off, s64, s32


def test_topk_mean_is_1_lipschitz(random_scores):
    off, s64, s32 = random_scores
    score_err = np.abs(s32.astype(np.float64) - s64).max()
    a, b = BC.pooled64(s64, off, BC.KS), BC.pooled64(s32, off, BC.KS)
    pool_err = np.abs(a - b).max()
    print(f"score error {score_err:.3e}  pooled error {pool_err:.3e}")
    assert pool_err <= score_err
    p32, _, _ = BC.pool(s32, off, BC.KS)
    assert (np.abs(p32.astype(np.float64) - a) <= score_err + BC.ulp32(a)).all()


def test_another_association_of_the_float64_sum_moves_the_result_by_at_most_one_ulp(random_scores):
    off, _, s32 = random_scores
    seq, _, _ = BC.pool(s32, off, BC.KS, summer=BC.seq_sum)
    pair, _, _ = BC.pool(s32, off, BC.KS, summer=BC.pairwise_sum)

    back, _, _ = BC.pool(s32, off, BC.KS, summer=lambda v: BC.seq_sum(v[::-1]))
    for name, other in (("pairwise", pair), ("last rank first", back)):
        ulps = np.abs(other.astype(np.float64) - seq.astype(np.float64)) / BC.ulp32(seq)
        print(f"{name} vs sequential: max {ulps.max():.0f} ulp, {int((ulps > 0).sum())} of {ulps.size} differ")
        assert ulps.max() <= 1


def test_bag_mean_oracle():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((50, 8)).astype(np.float32)
    off = np.array([0, 0, 20, 20, 50], np.int32)
    m = BC.bag_mean(x, off, False)
    assert np.allclose(m[1], x[:20].astype(np.float64).mean(0), atol=1e-7) and not m[0].any() and not m[2].any()
    u = BC.bag_mean(x, off, True)
    assert np.allclose(np.linalg.norm(u[[1, 3]].astype(np.float64), axis=1), 1.0, atol=1e-6) and not u[0].any()
    assert not BC.bag_mean(np.concatenate([x[:4], -x[:4]]), np.array([0, 8], np.int32), True).any()      # a zero mean has no direction


# ---- bag_offsets -------------------------------------------------------------------------------------------------------------------
def test_bag_offsets_from_sizes_and_from_shuffled_ids():
    from plip_amd.bags import as_bags, bag_offsets
    off, order = bag_offsets(sizes=[3, 0, 2])
    assert off.dtype == np.int32 and off.tolist() == [0, 3, 3, 5] and order is None
    rng = np.random.default_rng(2)
    ids = np.repeat(np.array([7, 3, 11, 5]), [4, 1, 6, 2])
    perm = rng.permutation(len(ids))
    shuffled = ids[perm]
    off, order = bag_offsets(ids=shuffled)
    assert off.tolist() == [0, 1, 3, 7, 13] and order.dtype == np.int64
    assert shuffled[order].tolist() == sorted(ids.tolist())
    for b in range(4):                                 # stable: a bag's rows keep their original order
        rows = order[off[b]:off[b + 1]]
        assert (np.diff(rows) > 0).all()
    off2, _ = bag_offsets(ids=np.array(["b", "a", "b"]))
    assert off2.tolist() == [0, 1, 3]
    x = rng.standard_normal((13, 8)).astype(np.float32)
    rows, o, p = as_bags((x, shuffled))
    assert rows is x and o.tolist() == off.tolist() and np.array_equal(p, order)
    rows, o, p = as_bags((x, np.array([0, 5, 13])))
    assert o.tolist() == [0, 5, 13] and p is None
    rows, o, p = as_bags([x[:5], x[5:5], x[5:]])
    assert np.array_equal(rows, x) and o.tolist() == [0, 5, 5, 13] and p is None


# ---- what Python refuses before the library is touched -----------------------------------------------------------------------------
def _engine():
    class NoDevice:
        @property
        def device(self):
            raise AssertionError("a refused call asked for the device")

        @property
        def lib(self):
            raise AssertionError("a refused call asked for the library")
    return NoDevice()


_X = np.zeros((10, 8), np.float32)
_T = np.zeros((3, 8), np.float32)
_OFF = np.array([0, 4, 10], np.int32)
_ST = np.zeros((3, 10), np.float32)


@pytest.mark.parametrize("call,message", [
    (lambda B, e: B.bag_topk_pool(e, _X, _OFF, _T, ks=()), "ks must be 1 .. 8 integers"),
    (lambda B, e: B.bag_topk_pool(e, _X, _OFF, _T, ks=tuple(range(1, 10))), "ks must be 1 .. 8 integers"),
    (lambda B, e: B.bag_topk_pool(e, _X, _OFF, _T, ks=(1.5,)), "ks must be 1 .. 8 integers"),
    (lambda B, e: B.bag_topk_pool(e, _X, _OFF, _T, ks=(0, 5)), "every k must lie in 1 .. 1024"),
    (lambda B, e: B.bag_topk_pool(e, _X, _OFF, _T, ks=(5, 1025)), "every k must lie in 1 .. 1024"),
    (lambda B, e: B.bag_topk_pool(e, _X, _OFF, _T, ks=(5, 5)), "strictly ascending"),
    (lambda B, e: B.bag_topk_pool(e, _X, _OFF, _T, ks=(10, 5)), "strictly ascending"),
    (lambda B, e: B.bag_topk_pool(e, _X, np.array([0, 4, 9]), _T), "end at N = 10"),
    (lambda B, e: B.bag_topk_pool(e, _X, np.array([1, 4, 10]), _T), "start at 0"),
    (lambda B, e: B.bag_topk_pool(e, _X, np.array([0, 6, 4, 10]), _T), "non-decreasing"),
    (lambda B, e: B.bag_topk_pool(e, _X, np.array([10]), _T), "S + 1 >= 2 values"),
    (lambda B, e: B.bag_topk_pool(e, _X, np.array([0.0, 10.0]), _T), "integer array"),
    (lambda B, e: B.bag_topk_pool(e, _X, np.array([[0, 10]]), _T), "1-d integer array"),
    (lambda B, e: B.bag_topk_pool(e, np.zeros((10, 6), np.float32), _OFF, np.zeros((3, 6), np.float32)), "embedding width 6 unsupported"),
    (lambda B, e: B.bag_topk_pool(e, np.zeros((10, 1028), np.float32), _OFF, np.zeros((3, 1028), np.float32)), "embedding width 1028 unsupported"),
    (lambda B, e: B.bag_topk_pool(e, np.zeros((0, 8), np.float32), np.array([0, 0]), _T), "x must be [N >= 1, D]"),
    (lambda B, e: B.bag_topk_pool(e, np.zeros((10,), np.float32), _OFF, _T), "x must be [N >= 1, D]"),
    (lambda B, e: B.bag_topk_pool(e, _X.astype(np.int32), _OFF, _T), "x must be floating point"),
    (lambda B, e: B.bag_topk_pool(e, _X, _OFF, np.zeros((3, 12), np.float32)), "class_embeds must be [C, 8]"),
    (lambda B, e: B.bag_topk_pool(e, _X, _OFF, np.zeros((65, 8), np.float32)), "1 <= C <= 64"),
    (lambda B, e: B.bag_topk_pool(e, _X, _OFF, np.zeros((0, 8), np.float32)), "1 <= C <= 64"),
    (lambda B, e: B.bag_topk_pool(e, _X, _OFF, _T.astype(np.int64)), "class_embeds must be floating point"),
    (lambda B, e: B.bag_pool_scores(e, np.zeros((65, 10), np.float32), _OFF), "class-major"),
    (lambda B, e: B.bag_pool_scores(e, np.zeros((10,), np.float32), _OFF), "class-major"),
    (lambda B, e: B.bag_pool_scores(e, _ST.astype(np.int32), _OFF), "scores_t must be floating point"),
    (lambda B, e: B.bag_pool_scores(e, _ST, np.array([0, 4, 11])), "end at N = 10"),
    (lambda B, e: B.bag_pool_scores(e, _ST, _OFF, ks=(3, 2)), "strictly ascending"),
    (lambda B, e: B.bag_mean(e, _X, np.array([0, 11])), "end at N = 10"),
    (lambda B, e: B.bag_mean(e, np.zeros((10, 2), np.float32), _OFF), "embedding width 2 unsupported"),
    (lambda B, e: B.bag_offsets(), "exactly one of sizes and ids"),
    (lambda B, e: B.bag_offsets(sizes=[1], ids=[0]), "exactly one of sizes and ids"),
    (lambda B, e: B.bag_offsets(sizes=[3, -1]), "non-negative integers"),
    (lambda B, e: B.bag_offsets(sizes=[1.5]), "non-negative integers"),
    (lambda B, e: B.bag_offsets(ids=[]), "one id per row"),
    (lambda B, e: B.slide_zero_shot(e, (_X, np.arange(7)), _T), "one slide id per row"),
    (lambda B, e: B.slide_zero_shot(e, [], _T), "non-empty list"),
    (lambda B, e: B.slide_zero_shot(e, [_X, np.zeros((2, 12), np.float32)], _T), "every bag must be [n_b, D]"),
    (lambda B, e: B.slide_zero_shot(e, [_X], _T, ks=(1, 5), return_top_tiles=6), "return_top_tiles must lie in 0 .. ks[-1] = 5"),
    (lambda B, e: B.slide_zero_shot(e, [_X], np.zeros((65, 8), np.float32)), "1 <= C <= 64"),
])
def test_bad_arguments_are_refused_with_a_message_that_names_them(call, message):
    import plip_amd.bags as B
    with pytest.raises(ValueError) as err:
        call(B, _engine())
    assert message in str(err.value), str(err.value)


# ---- headers, symbols and the build ------------------------------------------------------------------------------------------------
_CTYPES = {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64, "size_t": C.c_size_t}
_ENTRIES = (("plipmi_bag_workspace", "size_t", 4), ("plipmi_bag_topk_pool", "int", 17), ("plipmi_bag_pool_scores", "int", 14),
            ("plipmi_bag_mean", "int", 10))


def _header_args(header, ret, name):
    m = re.search(r"\b%s %s\(([^;]*?)\);" % (ret, name), header, re.S)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    return [" ".join(a.split()).rsplit(" ", 1) for a in args]            # [type, name]


def test_header_binding_and_library_agree_on_the_entries():
    from plip_amd import _lib
    from plip_amd import build as BLD
    BLD.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "plipmi.h")).read()
    test_header = open(os.path.join(ROOT, "include", "plipmi_test.h")).read()
    for name, ret, nargs in _ENTRIES:
        args = _header_args(header, ret, name)
        restype, argtypes = _lib.SYMBOLS[name]
        assert len(args) == nargs == len(argtypes), name
        assert restype is _CTYPES[ret], name
        for (ctype, arg), bound in zip(args, argtypes):
            if ctype == "const int32_t*" and arg == "ks_host":
                want = C.POINTER(C.c_int32)             # a HOST array: passed as a ctypes pointer
            elif ctype.endswith("*") or ctype == "plipmi_handle":
                want = C.c_void_p
            else:
                want = _CTYPES[ctype]
            assert bound is want or bound == want, (name, arg, ctype, bound)
        assert name not in _lib.TEST_SYMBOLS and name not in test_header and hasattr(lib, name)
    for macro, value, bound in (("PLIPMI_BAG_MAX_K", 1024, _lib.BAG_MAX_K), ("PLIPMI_BAG_MAX_KS", 8, _lib.BAG_MAX_KS),
                                ("PLIPMI_BAG_MAX_CLASSES", 64, _lib.BAG_MAX_CLASSES)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), header) and bound == value
    assert lib.plipmi_version() == 412 and re.search(r"#define PLIPMI_VERSION\s+412\b", header)
    # the new unit: compiled and linked last, behind stain.hip; the three older lists are what they were
    assert BLD.BAG_SOURCES == ["bags.hip"] and BLD.STAIN_SOURCES == ["stain.hip"] and BLD.LATER_SOURCES == ["kmeans.hip"]
    assert BLD.SOURCES[-1] == "region.hip" and len(BLD.SOURCES) == 27
    order = BLD.SOURCES + BLD.LATER_SOURCES + BLD.STAIN_SOURCES + BLD.BAG_SOURCES
    assert order[-3:] == ["kmeans.hip", "stain.hip", "bags.hip"] and len(set(order)) == len(order)
    assert os.path.getmtime(os.path.join(BLD.BUILD, "bags.o")) > 0
    src = open(os.path.join(BLD.CSRC, "bags.hip")).read()
    assert re.search(r"constexpr int kBagChunk = %d;" % BC.CHUNK, src)      # the tests' long bags are taken from the kernel's constant
    # the workspace: zero for sizes the entries refuse, and it grows with the rows, the classes and kmax
    ws = lib.plipmi_bag_workspace
    assert ws(0, 1, 1, 1) == 0 and ws(10, 0, 1, 1) == 0 and ws(10, 1, 0, 1) == 0 and ws(10, 1, 65, 1) == 0
    assert ws(10, 1, 1, 0) == 0 and ws(10, 1, 1, 1025) == 0
    assert ws(100000, 64, 9, 100) > ws(10000, 64, 9, 100) > 0 and ws(10000, 64, 64, 100) > ws(10000, 64, 9, 100)
    assert ws(10000, 64, 9, 1024) > ws(10000, 64, 9, 100) >= ws(10000, 64, 1, 1)
