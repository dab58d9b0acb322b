"""K-means without a GPU: the numpy oracle of tests/kmeans_common.py pinned against scikit-learn and against its own rules, the header /
binding / build agreement, and every argument limit refused from Python before anything touches a device."""
import os
import re

import numpy as np
import pytest

import kmeans_common as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle against scikit-learn -------------------------------------------------------------------------------------------------
def test_euclidean_lloyd_is_scikit_learns():
    from sklearn.cluster import KMeans
    x, _, _ = KM.blobs(600, 36, 5, seed=11)
    x = x.astype(np.float64)
    c0 = x[np.random.default_rng(5).choice(len(x), 5, replace=False)]
    ours = KM.lloyd(x, c0, KM.EUCLIDEAN, max_iter=300, tol_abs=0.0)
    sk = KMeans(n_clusters=5, init=c0, n_init=1, algorithm="lloyd", tol=0, max_iter=300).fit(x)
    assert ours["converged"] and ours["relocations"] == 0
    assert np.array_equal(ours["labels"], sk.labels_) and ours["n_iter"] == sk.n_iter_
    assert np.abs(ours["centers"] - sk.cluster_centers_).max() <= 1e-10
    assert abs(ours["inertia"] - sk.inertia_) <= 1e-9 * sk.inertia_
    assert np.array_equal(ours["counts"], np.bincount(sk.labels_, minlength=5))


# ---- the oracle's own rules ----------------------------------------------------------------------------------------------------------
def test_spherical_centres_are_unit_and_the_objective_never_increases():
    x = KM.normalised(np.random.default_rng(3).standard_normal((500, 24)))
    out = KM.lloyd(x, x[:7], KM.COSINE, max_iter=50)
    assert np.abs(np.sqrt((out["centers"] ** 2).sum(axis=1)) - 1).max() <= 1e-12
    h = np.asarray(out["history"])
    assert len(h) >= 2 and (np.diff(h) <= 1e-12 * h[0]).all()
    assert out["inertia"] <= h[-1] + 1e-12 * h[0]
    # the reported outputs belong to the returned centres
    lab, s = KM.assign(x, out["centers"], KM.COSINE)
    assert np.array_equal(lab, out["labels"]) and np.array_equal(np.bincount(lab, minlength=7), out["counts"])
    for k in range(7):
        rows = np.flatnonzero(lab == k)
        assert out["reps"][k] == rows[np.argmax(s[rows])]


def test_ties_go_to_the_lower_cluster_and_row():
    x = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [1.0, 0, 0, 0]])
    c = np.array([[0, 1.0, 0, 0], [1.0, 0, 0, 0], [1.0, 0, 0, 0]])
    lab, s = KM.assign(x, c, KM.COSINE)
    assert lab.tolist() == [1, 0, 1] and s.tolist() == [1.0, 1.0, 1.0]
    _, counts, reps, inertia = KM.update(x, lab, s, 3, KM.COSINE)
    assert counts.tolist() == [1, 2, 0] and reps.tolist() == [1, 0, -1] and inertia == 0.0


def test_seeding_rule_on_a_hand_made_vector():
    mind = np.array([0.0, 2.0, 0.0, 1.0, 1.0])           # prefix sums 0 2 2 3 4
    assert KM.seed_pick(mind, 0.0, set()) == 1              # the first prefix that EXCEEDS 0
    assert KM.seed_pick(mind, 0.49, set()) == 1
    assert KM.seed_pick(mind, 0.5, set()) == 3              # 2 does not exceed 0.5 * 4
    assert KM.seed_pick(mind, 0.75, set()) == 4
    assert KM.seed_pick(mind, 0.999, set()) == 4
    zero = np.zeros(4)
    assert KM.seed_pick(zero, 0.3, set()) == 0 and KM.seed_pick(zero, 0.3, {0, 1, 3}) == 2
    # all rows coincide: total == 0 at every step, the picks are the lowest rows not yet picked, after floor(u_0 N)
    x = np.ones((6, 4))
    assert KM.seed(x, 4, KM.EUCLIDEAN, np.array([0.5, 0.9, 0.1, 0.7])).tolist() == [3, 0, 1, 2]
    # integer rows: exact distances, checked by hand for two steps
    x = np.array([[0.0, 0, 0, 0], [3.0, 0, 0, 0], [0, 4.0, 0, 0], [3.0, 4.0, 0, 0]])
    picks = KM.seed(x, 3, KM.EUCLIDEAN, np.array([0.0, 0.5, 0.99]))     # d to row 0: 0 9 16 25, prefix 0 9 25 50: > 25 first at row 3
    assert picks.tolist()[:2] == [0, 3] and picks[2] in (1, 2) and len(set(picks.tolist())) == 3


def test_empty_cluster_rule_on_a_hand_made_case():
    d = np.array([1.0, 5.0, 5.0, 0.5, 3.0])
    empty = np.array([False, True, False, True, True])
    assert KM.relocate(d, empty) == {1: 1, 3: 2, 4: 4}
    # in the loop: a centre far from every row is empty, takes the farthest row, and no final cluster is empty
    x, _, _ = KM.blobs(300, 8, 3, seed=2)
    c0 = np.vstack([x[:2].astype(np.float64), np.full((1, 8), 1e3)])
    out = KM.lloyd(x, c0, KM.EUCLIDEAN)
    assert out["relocations"] >= 1 and (out["counts"] > 0).all() and out["converged"]


# ---- headers, symbols and the build ----------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_entries():
    from plip_amd import _lib
    from plip_amd.build import LATER_SOURCES, SOURCES, build
    build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "plipmi.h")).read()
    test_header = open(os.path.join(ROOT, "include", "plipmi_test.h")).read()
    for name, nargs in (("plipmi_kmeans_seed", 10), ("plipmi_kmeans_assign", 10), ("plipmi_kmeans_fit", 15)):
        m = re.search(r"\bint %s\(([^;]*?)\);" % name, header, re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert name not in _lib.TEST_SYMBOLS and not re.search(r"\b%s\s*\(" % name, test_header) and hasattr(lib, name)
    m = re.search(r"\bint plipmi_kmeans_update\(([^;]*?)\);", test_header, re.S)
    assert m and len(m.group(1).split(",")) == 13 == len(_lib.TEST_SYMBOLS["plipmi_kmeans_update"][1])
    assert "plipmi_kmeans_update" not in _lib.SYMBOLS and "plipmi_kmeans_update" not in header and hasattr(lib, "plipmi_kmeans_update")
    assert re.search(r"#define PLIPMI_KMEANS_MAX_K\s+%d\b" % _lib.KMEANS_MAX_K, header) and _lib.KMEANS_MAX_K == 4096
    assert re.search(r"PLIPMI_KMEANS_EUCLIDEAN = 0, PLIPMI_KMEANS_COSINE = 1", header) and _lib.KMEANS_METRICS == {"euclidean": 0, "cosine": 1}
    import ctypes
    assert ctypes.sizeof(_lib.KMeansInfo) == 32 and _lib.KMeansInfo.inertia.offset == 16 and _lib.KMeansInfo.center_shift.offset == 24
    # the last unit compiled and linked, behind every unit that existed; the list the earlier tests pin keeps its tail
    assert (SOURCES + LATER_SOURCES)[-1] == "kmeans.hip" and "kmeans.hip" not in SOURCES and SOURCES[-1] == "region.hip"
    assert lib.plipmi_version() == 412
    assert re.search(r"#define PLIPMI_VERSION\s+412\b", header)


# ---- what Python refuses before any device work ------------------------------------------------------------------------------------------
def _engine():
    import plip_amd.engine as E

    class NoDevice:
        _probe_shape = staticmethod(E.Engine._probe_shape)

        @property
        def device(self):
            raise AssertionError("a refused call asked for the device")
    return NoDevice()


@pytest.mark.parametrize("call,message", [
    (lambda km, e: km.kmeans_fit(e, np.zeros((10, 6), np.float32), 2), "D % 4 == 0"),
    (lambda km, e: km.kmeans_fit(e, np.zeros((10, 1028), np.float32), 2), "4 <= D <= 1024"),
    (lambda km, e: km.kmeans_fit(e, np.zeros((10, 8), np.float32), 11), "min(N, 4096)"),
    (lambda km, e: km.kmeans_fit(e, np.zeros((5000, 8), np.float32), 4097), "min(N, 4096)"),
    (lambda km, e: km.kmeans_fit(e, np.zeros((10, 8), np.float32), 0), "1 <= n_clusters"),
    (lambda km, e: km.kmeans_fit(e, np.zeros((10, 8), np.float32), 2, metric="manhattan"), "'euclidean' or 'cosine'"),
    (lambda km, e: km.kmeans_fit(e, np.zeros((10, 8), np.float32), 2, init="random"), "'k-means++' or an array"),
    (lambda km, e: km.kmeans_fit(e, np.zeros((10, 8), np.float32), 2, init=np.zeros((3, 8), np.float32)), "init must be [2, 8]"),
    (lambda km, e: km.kmeans_fit(e, np.zeros((10, 8), np.float32), 2, init=np.zeros((2, 8), np.float32), n_init=2), "n_init == 1"),
    (lambda km, e: km.kmeans_fit(e, np.zeros((10, 8), np.float32), 2, max_iter=0), "max_iter >= 1"),
    (lambda km, e: km.kmeans_fit(e, np.zeros((10, 8), np.float32), 2, tol=-1.0), "tol >= 0"),
    (lambda km, e: km.kmeans_fit(e, np.zeros((8,), np.float32), 2), "[N >= 1, D]"),
    (lambda km, e: km.kmeans_assign(e, np.zeros((10, 8), np.float32), np.zeros((2, 12), np.float32)), "centers must be [K, 8]"),
    (lambda km, e: km.kmeans_assign(e, np.zeros((10, 8), np.float32), np.zeros((11, 8), np.float32)), "min(N, 4096)"),
    (lambda km, e: km.kmeans_assign(e, np.zeros((10, 6), np.float32), np.zeros((2, 6), np.float32)), "D % 4 == 0"),
    (lambda km, e: km.kmeans_seed(e, np.zeros((10, 8), np.float32), 3, uniforms=np.array([0.1, 1.0, 0.2])), "[0, 1)"),
    (lambda km, e: km.kmeans_seed(e, np.zeros((10, 8), np.float32), 11), "min(N, 4096)"),
])
def test_argument_limits_are_refused_with_a_message_that_names_them(call, message):
    import plip_amd.kmeans as km
    with pytest.raises(ValueError) as err:
        call(km, _engine())
    assert message in str(err.value), str(err.value)
