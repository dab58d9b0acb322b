"""Softmax linear probe, host side (no GPU): the fixtures themselves -- the recorded float64 optimum is checked against the numpy
restatement of the objective in tests/softmax_probe_common.py, independently of the GPU code (tools/make_softmax_probe_golden.py made the
files) --, the restatement against a live scikit-learn, the two-class relation, the C entries' declaration, binding and argument checks,
and the Python surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import linear_probe_common as LP
import softmax_probe_common as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(SP.CASES)


@pytest.mark.parametrize("case", CASES)
def test_recorded_optimum_minimises_the_restated_objective(case):
    g = SP.load_case(case)
    n, C_, D, alpha, class_weight = SP.shape_of(case)
    xtr, ytr, xte, yte = SP.draw(case)
    assert (int(g["n_train"]), int(g["classes"]), int(g["dim"])) == (n, C_, D) and float(g["alpha"]) == alpha
    assert bool(g["balanced"]) == (class_weight == "balanced")
    np.testing.assert_allclose(LP.checksum(xtr), g["x_train_checksum"], rtol=1e-12)
    np.testing.assert_allclose(LP.checksum(xte), g["x_test_checksum"], rtol=1e-12)
    W, b = g["Wstar"], g["bstar"]
    assert W.shape == (C_, D) and W.dtype == np.float64 and b.shape == (C_,)          # always C rows, two classes included
    cw = SP.class_weights(ytr, C_, class_weight)
    f, gW, gb, G = SP.objective(xtr, ytr, C_, alpha, W, b, cw)
    gn = max(np.abs(gW).max(), np.abs(gb).max())
    print(f"OPTIMUM {case}: f* {f:.12f} |grad|_inf {gn:.2e} sum(b) {b.sum():.2e} |column sums of W|_inf {np.abs(W.sum(0)).max():.2e}")
    np.testing.assert_allclose(f, g["fstar"], rtol=1e-13)
    np.testing.assert_allclose(G, g["G"], rtol=1e-13)
    assert gn <= 1e-9
    assert abs(b.sum()) <= 1e-12                                  # recorded centred
    assert abs(gb.sum()) <= 1e-14                                 # the intercepts' gradient sums to zero: sum(b) never moves
    # sum_k grad_{w_k} f = alpha sum_k w_k (the residuals of a row sum to zero), so the column sums are bounded by the gradient left
    assert np.abs(W.sum(0)).max() <= C_ * gn / alpha + 1e-12
    # a constant added to every intercept changes nothing
    f2 = SP.objective(xtr, ytr, C_, alpha, W, b + 0.37, cw)[0]
    assert abs(f2 - f) <= 1e-13
    # a minimiser: every perturbation raises f
    rs = np.random.RandomState(1)
    assert SP.objective(xtr, ytr, C_, alpha, W + 1e-3 * rs.standard_normal((C_, D)), b + 1e-3 * rs.standard_normal(C_), cw)[0] > f
    for split, x, y in (("train", xtr, ytr), ("test", xte, yte)):
        _, pred, margin = SP.decide(x, W, b)
        under = int((margin < 1e-3).sum())
        assert under == int(g[f"under_margin_{split}"]) and under <= 0.02 * len(y)
        from plip_amd.reproducibility.metrics import eval_metrics
        d = eval_metrics(list(y), list(pred), average_method="macro")
        got = np.array([float(d[k]) for k in LP.METRIC_KEYS])
        np.testing.assert_allclose(got, g[f"opt_macro_{split}"], rtol=0, atol=1e-12, equal_nan=True)


@pytest.mark.parametrize("class_weight", ["balanced", None])
def test_restatement_matches_live_sklearn_on_three_classes(class_weight):
    """three or more classes: the minimiser of f is LogisticRegression(C = 1 / (alpha N), class_weight)'s"""
    lm = pytest.importorskip("sklearn.linear_model")
    pytest.importorskip("scipy.optimize")
    n, C_, D, alpha, _ = SP.shape_of("ragged3")
    x, y, _, _ = SP.draw("ragged3")
    W, b = SP.minimise(x, y, C_, alpha, SP.class_weights(y, C_, class_weight))
    lr = lm.LogisticRegression(C=1.0 / (alpha * n), class_weight=class_weight, tol=1e-12, max_iter=100000).fit(x.astype(np.float64), y)
    e_w, e_b = np.abs(lr.coef_ - W).max(), np.abs(SP.centre(lr.intercept_) - b).max()
    print(f"SKLEARN ragged3 {class_weight}: max|coef_ - W*| {e_w:.2e}  max|centred intercept_ - b*| {e_b:.2e}")
    assert lr.coef_.shape == (C_, D) and e_w <= 1e-6 and e_b <= 1e-6
    if class_weight == "balanced":              # the recorded fixture is this very point
        g = SP.load_case("ragged3")
        assert np.abs(g["Wstar"] - W).max() <= 1e-8 and np.abs(g["bstar"] - b).max() <= 1e-8


def test_two_classes_are_the_binary_problem_at_half_the_penalty():
    """W1 - W0 and b1 - b0 of the two-row softmax equal LogisticRegression(C = 2 / (alpha N))'s binary solution; coef stays [2, D]"""
    lm = pytest.importorskip("sklearn.linear_model")
    pytest.importorskip("scipy.optimize")
    rs = np.random.RandomState(77)
    n, D, alpha = 200, 32, 0.01
    y = rs.randint(0, 2, n)
    mu = rs.standard_normal((2, D))
    x = 0.5 * mu[y] / np.linalg.norm(mu, axis=1)[y, None] + rs.standard_normal((n, D)) / np.sqrt(D)      # unit rows, as the fixtures' draw
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    W, b = SP.minimise(x, y, 2, alpha, np.ones(2))
    assert W.shape == (2, D)
    lr = lm.LogisticRegression(C=2.0 / (alpha * n), tol=1e-12, max_iter=100000).fit(x.astype(np.float64), y)
    e_w, e_b = np.abs(lr.coef_[0] - (W[1] - W[0])).max(), abs(lr.intercept_[0] - (b[1] - b[0]))
    print(f"TWO-CLASS 200 x 32: max|coef_ - (W1 - W0)| {e_w:.2e}  |intercept_ - (b1 - b0)| {e_b:.2e}")
    assert e_w <= 1e-6 and e_b <= 1e-6
    np.testing.assert_allclose(W[0], -W[1], atol=1e-8)          # the columns of the optimal W sum to zero
    other = lm.LogisticRegression(C=1.0 / (alpha * n), tol=1e-12, max_iter=100000).fit(x.astype(np.float64), y)
    assert np.abs(other.coef_[0] - (W[1] - W[0])).max() > 100 * e_w     # and NOT the problem at the same penalty


def test_fp32_restatement_is_the_same_formula():
    x, y, _, _ = SP.draw("ragged3")
    rs = np.random.RandomState(4)
    W, b = rs.standard_normal((3, 64)).astype(np.float32), rs.standard_normal(3).astype(np.float32)
    cw = SP.class_weights(y, 3, "balanced").astype(np.float32)
    f32 = SP.objective_f32(x, y, 3, 0.01, W, b, cw)
    f64 = SP.objective(x, y, 3, 0.01, W, b, cw)
    assert f32[0].dtype == np.float32 and f32[1].dtype == np.float32
    e_loss, e_grad = SP.errors(f32[0], np.concatenate([f32[1], f32[2][:, None]], axis=1), *f64)
    assert 0 < e_loss < 1e-5 and 0 < e_grad < 1e-5
    # a label outside [0, C) carries weight 0: the same value as with the row dropped, up to the 1/N
    bad = y.copy()
    bad[5], bad[6] = 1 << 30, -7
    keep = np.ones(len(y), bool)
    keep[[5, 6]] = False
    fa = SP.objective(x, bad, 3, 0.0, W, b, cw)[0] * len(y)
    fb = SP.objective(x[keep], y[keep], 3, 0.0, W, b, cw)[0] * keep.sum()
    assert abs(fa - fb) <= 1e-12 * abs(fb)


def test_softmax_entries_are_declared_and_bound_together():
    from plip_amd import _lib
    product = open(os.path.join(ROOT, "include", "plipmi.h")).read()
    test_h = open(os.path.join(ROOT, "include", "plipmi_test.h")).read()
    assert re.search(r"\bplipmi_softmax_fit\s*\(", product) and "plipmi_softmax_fit" in _lib.SYMBOLS
    assert "plipmi_softmax_fit" not in _lib.TEST_SYMBOLS
    assert re.search(r"\bplipmi_softmax_loss_grad\s*\(", test_h) and "plipmi_softmax_loss_grad" in _lib.TEST_SYMBOLS
    assert not re.search(r"\bplipmi_softmax_loss_grad\s*\(", product)
    assert not re.search(r"\bplipmi_softmax_predict", product + test_h)          # predictions are plipmi_probe_predict
    assert _lib.SYMBOLS["plipmi_softmax_fit"][1][-2] == C.POINTER(_lib.ProbeInfo)
    assert C.sizeof(_lib.ProbeInfo) == 16 + 8 + 8 * _lib.PROBE_MAX_K              # the info struct kept its layout
    sources = __import__("plip_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "probe_softmax.hip" in sources and "probe.hip" in sources
    # a product module: it binds nothing from the test header
    src = open(os.path.join(ROOT, "plip_amd", "softmax_probe.py")).read()
    assert "plipmi_softmax_fit" in src and "plipmi_softmax_loss_grad" not in src


def test_softmax_entries_reject_bad_arguments_before_touching_the_device():
    """a null handle, N <= 0, C out of range, an unsupported D and a bad alpha are PLIPMI_ERR_INVALID before the handle or the GPU is
    used (the handle here is a block of host memory nobody may read: a launch or an allocation on it would not come back with code 1)."""
    from plip_amd import _lib
    from plip_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    buf = C.create_string_buffer(4096)
    p = C.cast(C.c_void_p((C.addressof(buf) + 15) // 16 * 16), C.c_void_p)
    info = _lib.ProbeInfo()

    def fit(N=64, D=64, K=3, alpha=0.01, max_iter=10, gtol=1e-6, X=p, y=p, WB=p, handle=h):
        return lib.plipmi_softmax_fit(handle, X, N, D, y, K, None, alpha, max_iter, gtol, WB, C.byref(info), None)

    for kw, word in ((dict(N=0), "N > 0"), (dict(N=-5), "N > 0"), (dict(K=1), "classes"), (dict(K=0), "classes"), (dict(K=65), "classes"),
                     (dict(D=62), "width"), (dict(D=1028), "width"), (dict(D=0), "width"), (dict(alpha=0.0), "alpha"),
                     (dict(alpha=-1.0), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(alpha=float("inf")), "alpha"),
                     (dict(max_iter=0), "max_iter"), (dict(gtol=0.0), "gtol"), (dict(gtol=float("nan")), "gtol"), (dict(X=None), "null"),
                     (dict(y=None), "null"), (dict(WB=None), "null"), (dict(handle=None), "null"),
                     (dict(X=C.c_void_p(p.value + 4)), "aligned")):
        assert fit(**kw) == 1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert lib.plipmi_softmax_loss_grad(None, p, 8, 64, p, 3, None, 0.01, p, p, p, None) == 1
    assert lib.plipmi_softmax_loss_grad(h, p, 8, 64, p, 3, None, -1.0, p, p, p, None) == 1
    assert lib.plipmi_softmax_loss_grad(h, p, 8, 64, p, 3, None, 0.01, p, None, p, None) == 1
    assert lib.plipmi_softmax_loss_grad(h, p, 8, 64, p, 3, None, 0.01, p, p, None, None) == 1
    assert lib.plipmi_softmax_loss_grad(h, p, 8, 64, p, 1, None, 0.01, p, p, p, None) == 1


def test_softmax_prober_takes_c_xor_alpha_and_is_exported():
    import inspect
    from plip_amd import reproducibility as R
    from plip_amd.softmax_probe import softmax_fit
    sig = inspect.signature(R.SoftmaxProber.__init__)
    assert list(sig.parameters)[:6] == ["self", "alpha", "C", "class_weight", "seed", "engine"]
    assert sig.parameters["C"].default == 0.316 and sig.parameters["alpha"].default is None and sig.parameters["seed"].default == 7
    assert sig.parameters["class_weight"].default is None
    assert list(inspect.signature(R.SoftmaxProber.train_and_test).parameters) == list(inspect.signature(R.LinearProber.train_and_test).parameters)
    assert "SoftmaxProber" in R.__doc__ and "LinearProber" in R.__doc__
    p = R.SoftmaxProber()
    assert (p.alpha, p.C) == (None, 0.316)                      # the CLIP protocol
    p = R.SoftmaxProber(alpha=0.01)
    assert (p.alpha, p.C) == (0.01, None)
    p = R.SoftmaxProber(C=1.0, class_weight="balanced")
    assert (p.alpha, p.C, p.class_weight) == (None, 1.0, "balanced")
    for kw in (dict(alpha=0.01, C=1.0), dict(C=None), dict(class_weight="auto")):
        with pytest.raises(ValueError):
            R.SoftmaxProber(**kw)
    names = list(inspect.signature(softmax_fit).parameters)
    assert names == ["engine", "x", "y", "n_classes", "alpha", "C", "class_weight", "max_iter", "gtol", "coef_init", "intercept_init"]

    class NoDevice:             # the argument checks that need no device come first
        pass
    x, y = np.zeros((8, 16), np.float32), np.arange(8) % 3
    for kw, word in ((dict(), "exactly one"), (dict(alpha=0.1, C=1.0), "exactly one"), (dict(C=1.0, n_classes=1), "two classes"),
                     (dict(C=1.0, n_classes=65), "at most"), (dict(C=1.0, class_weight="auto"), "class_weight"),
                     (dict(C=1.0, max_iter=0), "max_iter")):
        args = dict(x=x, y=y, n_classes=3)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            softmax_fit(NoDevice(), **args)


def test_predict_proba_rows_sum_to_one():
    import torch
    from plip_amd.reproducibility.softmax_probe import SoftmaxClassifier

    class HostEngine:           # probe_predict on the host: predict_proba only post-processes the decision values
        def probe_predict(self, x, coef, intercept, return_decision=False):
            dec = torch.as_tensor(x, dtype=torch.float32) @ coef.T + intercept
            return (dec.argmax(1).to(torch.int32), dec) if return_decision else dec.argmax(1).to(torch.int32)

    rs = np.random.RandomState(6)
    coef, intercept = torch.from_numpy(30 * rs.standard_normal((5, 16)).astype(np.float32)), torch.zeros(5)
    clf = SoftmaxClassifier(HostEngine(), coef, intercept, np.arange(5), {"iterations": 4})
    x = rs.standard_normal((40, 16)).astype(np.float32)
    p = clf.predict_proba(x)
    assert p.shape == (40, 5) and p.dtype == np.float64 and np.isfinite(p).all() and (p >= 0).all()
    np.testing.assert_allclose(p.sum(1), 1.0, rtol=0, atol=1e-12)
    assert np.array_equal(p.argmax(1), clf.predict(x)) and clf.coef_.shape == (5, 16)
    two = SoftmaxClassifier(HostEngine(), coef[:2], intercept[:2], np.array(["a", "b"]), {"iterations": 1})
    assert two.coef_.shape == (2, 16) and two.predict_proba(x).shape == (40, 2) and two.decision_function(x).shape == (40, 2)
