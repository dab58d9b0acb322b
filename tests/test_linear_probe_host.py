"""Linear-probe head, host side (no GPU): macro-averaged metrics against scikit-learn's recorded values, label encoding, argument
validation of the C entries, and the fixtures themselves -- the recorded float64 optimum is checked against the numpy restatement of
the objective in tests/linear_probe_common.py, independently of the GPU code (tools/make_linear_probe_golden.py made the files)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import linear_probe_common as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(LP.CASES)


def _metrics(y, p, **kw):
    from plip_amd.reproducibility.metrics import eval_metrics
    d = eval_metrics(list(y), list(p), **kw)
    return np.array([float(d[k]) for k in LP.METRIC_KEYS])


@pytest.mark.parametrize("case", CASES)
def test_macro_metrics_equal_recorded_sklearn(case):
    g = LP.load_case(case)
    assert tuple(g["metric_keys"]) == LP.METRIC_KEYS
    for split in ("train", "test"):
        y = g[f"y_{split}"].astype(np.int64)
        for pred, want in ((g[f"opt_pred_{split}"], g[f"opt_macro_{split}"]), (g[f"sgd_pred_{split}"], g[f"sgd_macro_{split}"])):
            got = _metrics(y, pred.astype(np.int64), average_method="macro")
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, equal_nan=True)


@pytest.mark.parametrize("case", CASES)
def test_weighted_metrics_are_unchanged(case):
    """the default averaging returns what it returned before "macro" existed (recorded then), and what sklearn returns"""
    g = LP.load_case(case)
    for split in ("train", "test"):
        y, pred = g[f"y_{split}"].astype(np.int64), g[f"opt_pred_{split}"].astype(np.int64)
        got = _metrics(y, pred)
        assert np.array_equal(got, g[f"opt_weighted_pkg_{split}"], equal_nan=True)
        np.testing.assert_allclose(got, g[f"opt_weighted_sklearn_{split}"], rtol=0, atol=1e-12, equal_nan=True)


def test_macro_metrics_equal_live_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    rs = np.random.RandomState(3)
    for C_ in (2, 5):
        y = rs.randint(0, C_, 400)
        p = rs.randint(0, C_ - 1 if C_ > 2 else C_, 400)          # five classes: the last one is never predicted (zero division)
        from plip_amd.reproducibility.metrics import eval_metrics
        d = eval_metrics(list(y), list(p), average_method="macro")
        assert abs(d["WF1"] - skm.f1_score(y, p, average="macro", zero_division=0)) < 1e-12
        assert abs(d["precision"] - skm.precision_score(y, p, average="macro", zero_division=0)) < 1e-12
        assert abs(d["recall"] - skm.recall_score(y, p, average="macro", zero_division=0)) < 1e-12
        assert abs(d["Accuracy"] - skm.accuracy_score(y, p)) < 1e-12


def test_other_averaging_still_raises():
    from plip_amd.reproducibility.metrics import eval_metrics
    with pytest.raises(NotImplementedError):
        eval_metrics([0, 1], [0, 1], average_method="micro")


def test_linear_prober_is_exported_with_the_reference_signature():
    import inspect
    from plip_amd import reproducibility as R
    sig = inspect.signature(R.LinearProber.__init__)
    assert list(sig.parameters)[:4] == ["self", "alpha", "seed", "engine"] and sig.parameters["seed"].default == 7
    assert list(inspect.signature(R.LinearProber.train_and_test).parameters) == ["self", "train_x", "train_y", "test_x", "test_y"]
    assert "LinearProber" in R.__doc__


def test_label_encoding_follows_label_encoder():
    from plip_amd.reproducibility.linear_probe import _encode
    classes = np.unique(np.array(["tumor", "stroma", "adipose", "stroma"]))
    assert list(classes) == ["adipose", "stroma", "tumor"]
    assert list(_encode(classes, ["tumor", "adipose", "stroma"], "y")) == [2, 0, 1]
    assert list(_encode(np.unique([7, 3, 5]), [5, 5, 3, 7], "y")) == [1, 1, 0, 2]
    with pytest.raises(ValueError, match="unseen"):
        _encode(classes, ["tumor", "lymph"], "test_y")
    with pytest.raises(ValueError, match="unseen"):
        _encode(np.unique([0, 1, 2]), [3], "test_y")


def test_two_class_classifier_has_sklearn_shapes():
    import torch
    from plip_amd.reproducibility.linear_probe import ProbeClassifier
    clf = ProbeClassifier(None, torch.zeros((1, 8)), torch.zeros((1,)), np.array(["a", "b"]), {"iterations": 3})
    assert clf.coef_.shape == (1, 8) and clf.intercept_.shape == (1,) and clf.n_iter_ == 3 and list(clf.classes_) == ["a", "b"]
    clf = ProbeClassifier(None, torch.zeros((3, 8)), torch.zeros((3,)), np.arange(3), {"iterations": 1})
    assert clf.coef_.shape == (3, 8) and clf.intercept_.shape == (3,)


def test_probe_entries_are_declared_and_bound_together():
    from plip_amd import _lib
    product = open(os.path.join(ROOT, "include", "plipmi.h")).read()
    test_h = open(os.path.join(ROOT, "include", "plipmi_test.h")).read()
    for name in ("plipmi_probe_fit", "plipmi_probe_predict"):
        assert re.search(r"\b%s\s*\(" % name, product) and name in _lib.SYMBOLS and name not in _lib.TEST_SYMBOLS
    assert re.search(r"\bplipmi_probe_loss_grad\s*\(", test_h) and "plipmi_probe_loss_grad" in _lib.TEST_SYMBOLS
    assert not re.search(r"\bplipmi_probe_loss_grad\s*\(", product)
    m = re.search(r"#define PLIPMI_PROBE_MAX_K (\d+)", product)
    assert int(m.group(1)) == _lib.PROBE_MAX_K
    # the info struct: four int32, a double, then the losses
    assert C.sizeof(_lib.ProbeInfo) == 16 + 8 + 8 * _lib.PROBE_MAX_K
    assert "probe.hip" in __import__("plip_amd.build", fromlist=["SOURCES"]).SOURCES


def test_probe_entries_reject_bad_arguments_before_touching_the_device():
    """N <= 0, K out of range, an unsupported D and a bad alpha are PLIPMI_ERR_INVALID before the handle or the GPU is used (the
    handle here is a block of host memory nobody may read: a launch or an allocation on it would not come back with code 1)."""
    from plip_amd import _lib
    from plip_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    buf = C.create_string_buffer(4096)
    p = C.cast(C.c_void_p((C.addressof(buf) + 15) // 16 * 16), C.c_void_p)
    info = _lib.ProbeInfo()

    def fit(N=64, D=64, K=3, alpha=0.01, max_iter=10, gtol=1e-6, X=p):
        return lib.plipmi_probe_fit(h, X, N, D, p, K, p, p, alpha, max_iter, gtol, p, C.byref(info), None)

    for kw, word in ((dict(N=0), "N > 0"), (dict(N=-5), "N > 0"), (dict(K=0), "problems"), (dict(K=65), "problems"),
                     (dict(D=62), "width"), (dict(D=1028), "width"), (dict(D=0), "width"), (dict(alpha=0.0), "alpha"),
                     (dict(alpha=-1.0), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(alpha=float("inf")), "alpha"),
                     (dict(max_iter=0), "max_iter"), (dict(gtol=0.0), "gtol"), (dict(X=None), "null")):
        assert fit(**kw) == 1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert lib.plipmi_probe_predict(h, p, 0, 64, p, 3, None, p, None) == 1
    assert lib.plipmi_probe_predict(h, p, 8, 64, p, 3, None, None, None) == 1
    assert lib.plipmi_probe_predict(h, C.c_void_p(p.value + 4), 8, 64, p, 3, None, p, None) == 1 and "aligned" in _lib.last_error()
    assert lib.plipmi_probe_loss_grad(h, p, 8, 64, p, 3, p, p, -1.0, p, p, p, None) == 1
    assert lib.plipmi_probe_fit(None, p, 8, 64, p, 3, p, p, 0.01, 5, 1e-6, p, None, None) == 1


@pytest.mark.parametrize("case", CASES)
def test_recorded_optimum_minimises_the_restated_objective(case):
    """pins the objective -- class weights, two-class rule, unregularised intercept -- without any GPU code: the float64 restatement
    reproduces the recorded f_k(W*) and has no gradient left there; the redrawn data is the data the fixture was made from."""
    g = LP.load_case(case)
    seed, n, C_, D, alpha, sep = LP.CASES[case]
    xtr, ytr, xte, yte = LP.draw(case)
    assert (int(g["seed"]), int(g["n_train"]), int(g["classes"]), int(g["dim"])) == (seed, n, C_, D) and float(g["alpha"]) == alpha
    assert xtr.dtype == np.float32 and xtr.shape == (n, D) and xte.shape == (LP.n_test_of(case), D)
    np.testing.assert_allclose(LP.checksum(xtr), g["x_train_checksum"], rtol=1e-12)
    np.testing.assert_allclose(LP.checksum(xte), g["x_test_checksum"], rtol=1e-12)
    assert np.array_equal(ytr, g["y_train"]) and np.array_equal(yte, g["y_test"])
    K = 1 if C_ == 2 else C_
    assert g["Wstar"].shape == (K, D) and g["Wstar"].dtype == np.float64 and g["bstar"].shape == (K,)
    f, gW, gb, G = LP.objective(xtr, ytr, C_, alpha, g["Wstar"], g["bstar"])
    np.testing.assert_allclose(f, g["fstar"], rtol=1e-13)
    np.testing.assert_allclose(G, g["G"], rtol=1e-13)
    assert max(np.abs(gW).max(), np.abs(gb).max()) < 1e-9
    # a minimiser, not just a stationary point of something else: every perturbation raises f_k
    rs = np.random.RandomState(1)
    f2 = LP.objective(xtr, ytr, C_, alpha, g["Wstar"] + 1e-3 * rs.standard_normal((K, D)), g["bstar"] + 1e-3)[0]
    assert (f2 > f).all()
    # the reference's own solution is a worse (or equal) point of the same objective, and its recorded value is reproduced
    fs = LP.objective(xtr, ytr, C_, alpha, g["sgd_coef"], g["sgd_intercept"])[0]
    np.testing.assert_allclose(fs, g["sgd_f"], rtol=1e-13)
    assert (fs >= f).all()
    for split, x in (("train", xtr), ("test", xte)):
        _, pred, margin = LP.decide(x, g["Wstar"], g["bstar"])
        assert np.array_equal(pred, g[f"opt_pred_{split}"])
        np.testing.assert_allclose(margin, g[f"opt_margin_{split}"], rtol=1e-6, atol=1e-9)


def test_class_weights_follow_sklearn_balanced():
    y = np.array([0] * 6 + [1] * 3 + [2] * 1)
    pos, neg = LP.sample_weights(y, 3)
    np.testing.assert_allclose(pos, 10 / (3 * np.array([6.0, 3.0, 1.0])))
    assert list(neg) == [1.0, 1.0, 1.0]
    pos, neg = LP.sample_weights(np.array([0, 0, 0, 1]), 2)
    np.testing.assert_allclose([pos[0], neg[0]], [4 / (2 * 1.0), 4 / (2 * 3.0)])
