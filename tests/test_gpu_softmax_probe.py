"""Softmax linear probe on the GPU against the recorded float64 optimum (tests/golden/softmax_probe_*.npz, made on a CPU by
tools/make_softmax_probe_golden.py) and the numpy float64 restatement of the objective (tests/softmax_probe_common.py) -- never against
the code under test.

Bounds.  A kernel evaluation's loss error is relative, its gradient error is divided by G = (1/N) sum_i cw[y_i] |x_i|, the size of the
terms the gradient sums.  Each is held to the LARGER of the project's existing kernel bound (4 x 3.397e-8, 4 x 4.149e-8: 4 x the one-vs-rest
pass's measured errors, profiles/linear_probe_parity.txt) and 4 x the error the same formulas make in numpy float32 on the same inputs
(softmax_probe_common.objective_f32), computed here; the margin of 4 covers another summation order.  The fit's bounds follow from
convexity and from the gradient bound; none is a measurement of the code under test.  Every test prints its figures before it asserts
(profiles/softmax_probe_parity.txt keeps them)."""
import warnings

import numpy as np
import pytest
import torch

import linear_probe_common as LP
import softmax_probe_common as SP

pytestmark = pytest.mark.gpu

CASES = list(SP.CASES)
KERNEL_LOSS_REL = 4 * 3.397e-08
KERNEL_GRAD_REL = 4 * 4.149e-08
GTOL = 2e-8                     # plip_amd.softmax_probe.DEFAULT_GTOL
DECISION_TOL = 5e-4
MARGIN = 1e-3
# (N, D, C): ragged tile with 13 masked columns; narrowest D with one row in the second tile; the group boundary; the no-prefetch
# tile with a last group one class wide; the maximum C
SHAPES = [(37, 64, 3), (33, 4, 2), (1000, 128, 16), (1000, 128, 17), (70, 1024, 33), (333, 768, 64)]


@pytest.fixture(scope="module")
def eng():
    from plip_amd.engine import heads_engine
    return heads_engine()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dtype=dtype)


_DRAWS = {}


def _draw(case):
    if case not in _DRAWS:
        _DRAWS[case] = SP.draw(case)
    return _DRAWS[case]


def _eval(eng, x, y, cw, alpha, wb):
    from plip_amd.kernel_entries import softmax_loss_grad
    loss, grad = softmax_loss_grad(eng, _dev(x, torch.float32), _dev(y, torch.int32), _dev(wb, torch.float32),
                                   None if cw is None else _dev(cw, torch.float32), alpha)
    torch.cuda.synchronize()
    return loss, grad


def kernel_errors(eng, x, y, C_, alpha, W, b, cw):
    """(loss rel err, grad err / G) of the kernel and of the fp32 restatement, both against float64 at the SAME fp32 point and fp32
    class weights; also checks that nothing of the sentinel-filled outputs is left and that a second evaluation has the same bits"""
    wb = np.concatenate([W, b[:, None]], axis=1).astype(np.float32)
    cw32 = np.ones(C_, np.float32) if cw is None else cw.astype(np.float32)
    loss, grad = _eval(eng, x, y, None if cw is None else cw32, alpha, wb)          # outputs NaN-filled by the wrapper
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all(), "an output element was not written"
    ref = SP.objective(x, y, C_, alpha, wb[:, :-1], wb[:, -1], cw32)
    f32 = SP.objective_f32(x, y, C_, alpha, wb[:, :-1], wb[:, -1], cw32)
    e_k = SP.errors(loss.cpu().numpy()[0], grad.cpu().numpy(), *ref)
    e_32 = SP.errors(f32[0], np.concatenate([f32[1], f32[2][:, None]], axis=1), *ref)
    again = _eval(eng, x, y, None if cw is None else cw32, alpha, wb)
    assert torch.equal(loss, again[0]) and torch.equal(grad, again[1]), "two evaluations of the same inputs differ in bits"
    return e_k, e_32, float(ref[3])


def _check(tag, e_k, e_32):
    b_loss, b_grad = max(KERNEL_LOSS_REL, 4 * e_32[0]), max(KERNEL_GRAD_REL, 4 * e_32[1])
    print(f"KERNEL {tag}: loss rel err {e_k[0]:.3e} (fp32 restatement {e_32[0]:.3e}, bound {b_loss:.3e})  "
          f"grad err / G {e_k[1]:.3e} (fp32 restatement {e_32[1]:.3e}, bound {b_grad:.3e})")
    assert e_k[0] <= b_loss and e_k[1] <= b_grad, (tag, e_k, e_32)


@pytest.mark.parametrize("N,D,C_", SHAPES)
def test_kernel_loss_and_gradient_shapes(eng, N, D, C_):
    rs = np.random.RandomState(1000 + C_ + D)
    x = rs.standard_normal((N, D)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = rs.randint(0, C_, N)
    y[:C_] = np.arange(C_)
    for weighting in ("balanced", None):
        cw = None if weighting is None else SP.class_weights(y, C_, weighting)
        for name, W, b in (("zero", np.zeros((C_, D)), np.zeros(C_)), ("random", rs.standard_normal((C_, D)), rs.standard_normal(C_))):
            e_k, e_32, _ = kernel_errors(eng, x, y, C_, 0.003, W, b, cw)
            _check(f"N={N} D={D} C={C_} {weighting} {name}", e_k, e_32)


@pytest.mark.parametrize("case", CASES)
def test_kernel_loss_and_gradient_cases(eng, case):
    g = SP.load_case(case)
    n, C_, D, alpha, class_weight = SP.shape_of(case)
    x, y, _, _ = _draw(case)
    cw = None if class_weight is None else SP.class_weights(y, C_, class_weight)
    rs = np.random.RandomState(5)
    for name, W, b in (("zero", np.zeros((C_, D)), np.zeros(C_)), ("random", rs.standard_normal((C_, D)), rs.standard_normal(C_)),
                       ("optimum", g["Wstar"], g["bstar"])):
        e_k, e_32, G = kernel_errors(eng, x, y, C_, alpha, W, b, cw)
        if name == "optimum":
            print(f"NOISE {case}: gradient error of the kernel at the optimum {e_k[1] * G:.3e} (G {G:.4f}); gtol {GTOL:.1e}")
        _check(f"{case} {name}", e_k, e_32)


@pytest.mark.parametrize("N,D,C_", [(37, 64, 3), (1000, 128, 17)])
def test_labels_outside_the_classes_carry_weight_zero(eng, N, D, C_):
    """y is only compared, never an index: such a row adds nothing to the loss or the gradient -- the restatement with the rows dropped"""
    rs = np.random.RandomState(2 + C_)
    x = rs.standard_normal((N, D)).astype(np.float32)
    y = rs.randint(0, C_, N)
    y[:C_] = np.arange(C_)
    cw = SP.class_weights(y, C_, "balanced").astype(np.float32)
    bad = y.copy()
    bad[[5, 6, N - 1]] = 1 << 30, -7, C_
    keep = (bad >= 0) & (bad < C_)
    wb = np.concatenate([rs.standard_normal((C_, D)), rs.standard_normal((C_, 1))], axis=1).astype(np.float32)
    alpha = 0.01
    loss, grad = _eval(eng, x, bad, cw, alpha, wb)
    pen = 0.5 * alpha * (wb[:, :-1].astype(np.float64) ** 2).sum()
    f_kept, gW, gb, G = SP.objective(x[keep], bad[keep], C_, alpha, wb[:, :-1], wb[:, -1], cw)
    want = (f_kept - pen) * keep.sum() / N + pen
    f32 = SP.objective_f32(x, bad, C_, alpha, wb[:, :-1], wb[:, -1], cw)
    ref = SP.objective(x, bad, C_, alpha, wb[:, :-1], wb[:, -1], cw)
    e_32 = SP.errors(f32[0], np.concatenate([f32[1], f32[2][:, None]], axis=1), *ref)
    e_k = SP.errors(loss.cpu().numpy()[0], grad.cpu().numpy(), *ref)
    print(f"OUTSIDE N={N} C={C_}: loss {float(loss[0]):.9f} with the rows dropped {want:.9f}")
    assert torch.isfinite(grad).all() and torch.isfinite(loss).all()
    assert abs(float(loss[0]) - want) <= max(KERNEL_LOSS_REL, 4 * e_32[0]) * abs(want) + 1e-12 * abs(want)
    _check(f"outside N={N} C={C_}", e_k, e_32)


_FITS = {}


def _fit(eng, case):
    if case not in _FITS:
        from plip_amd.softmax_probe import softmax_fit
        n, C_, D, alpha, class_weight = SP.shape_of(case)
        xtr, ytr, xte, yte = _draw(case)
        with warnings.catch_warnings():
            warnings.simplefilter("error")              # non-convergence is a RuntimeWarning: a failure here
            coef, intercept, info = softmax_fit(eng, xtr, ytr, C_, alpha=alpha, class_weight=class_weight)
        _FITS[case] = (coef, intercept, info)
    return _FITS[case]


def _centred_decisions(eng, coef, intercept, x):
    _, dec = eng.probe_predict(x, coef, intercept, return_decision=True)
    return dec.cpu().numpy().astype(np.float64) - float(intercept.cpu().numpy().astype(np.float64).mean())


@pytest.mark.parametrize("case", CASES)
def test_fit_reaches_the_recorded_optimum(eng, case):
    from plip_amd.reproducibility.metrics import eval_metrics
    g = SP.load_case(case)
    n, C_, D, alpha, class_weight = SP.shape_of(case)
    xtr, ytr, xte, yte = _draw(case)
    cw = SP.class_weights(ytr, C_, class_weight)
    coef, intercept, info = _fit(eng, case)
    W, b = coef.cpu().numpy().astype(np.float64), intercept.cpu().numpy().astype(np.float64)
    f, gW, gb, G = SP.objective(xtr, ytr, C_, alpha, W, b, cw)
    gn = max(np.abs(gW).max(), np.abs(gb).max())
    dist = np.abs(W - g["Wstar"]).sum() + np.abs(SP.centre(b) - g["bstar"]).sum()
    gap = f - float(g["fstar"])
    e_dec = {}
    for split, x in (("train", xtr), ("test", xte)):
        e_dec[split] = float(np.abs(_centred_decisions(eng, coef, intercept, x) - SP.decide(x, g["Wstar"], g["bstar"])[0]).max())
    print(f"FIT {case}: iterations {info['iterations']} evaluations {info['evaluations']} solver |grad|_inf {info['grad_norm']:.2e} "
          f"float64 |grad|_inf {gn:.3e} (bound {GTOL + KERNEL_GRAD_REL * G:.3e})  gap {gap:.3e} (bound {gn * dist:.3e}, |theta - theta*|_1 "
          f"{dist:.3e})  max|W-W*| {np.abs(W - g['Wstar']).max():.3e} max|b-b*| {np.abs(SP.centre(b) - g['bstar']).max():.3e} sum(b) {b.sum():.2e}  "
          f"decision err train {e_dec['train']:.3e} test {e_dec['test']:.3e}")
    assert info["converged"] and info["grad_norm"] <= GTOL and info["evaluations"] > info["iterations"] >= 1
    assert abs(info["loss"] - f) <= 1e-6 * f                      # the solver's own f is the objective's value there
    assert coef.shape == (C_, D) and intercept.shape == (C_,)     # always C rows
    assert gn <= GTOL + KERNEL_GRAD_REL * G
    assert gap <= gn * dist                                       # convexity: f(t) - f* <= grad f(t) . (t - t*) <= |grad|_inf |t - t*|_1
    assert max(e_dec.values()) <= DECISION_TOL
    for split, x, y in (("train", xtr, ytr), ("test", xte, yte)):
        _, opt_pred, margin = SP.decide(x, g["Wstar"], g["bstar"])
        pred = eng.probe_predict(x, coef, intercept).cpu().numpy()
        keep = margin >= MARGIN
        left = int((~keep).sum())
        print(f"PREDICT {case} {split}: {left} of {len(keep)} rows under margin {MARGIN:.0e}, {int((pred != opt_pred).sum())} rows differ")
        assert left <= 0.02 * len(keep)
        assert np.array_equal(pred[keep], opt_pred[keep].astype(pred.dtype))
        if left == 0:
            m = eval_metrics(list(y), list(pred.astype(np.int64)), average_method="macro")
            want = dict(zip(LP.METRIC_KEYS, g[f"opt_macro_{split}"]))
            for k in LP.METRIC_KEYS:
                assert abs(m[k] - want[k]) <= 1e-12 or (np.isnan(m[k]) and np.isnan(want[k])), (case, split, k)


@pytest.mark.parametrize("case", CASES)
def test_fit_is_deterministic_and_stops_at_the_optimum(eng, case):
    from plip_amd.softmax_probe import softmax_fit
    g = SP.load_case(case)
    n, C_, D, alpha, class_weight = SP.shape_of(case)
    xtr, ytr, xte, _ = _draw(case)
    coef, intercept, info = _fit(eng, case)
    again = softmax_fit(eng, torch.from_numpy(xtr).cuda(), torch.from_numpy(ytr).cuda(), C_, alpha=alpha, class_weight=class_weight)
    assert torch.equal(coef, again[0]) and torch.equal(intercept, again[1]) and again[2] == info, "a second fit differs"
    # from its own optimum: the same bits give the same gradient, which met gtol -- one evaluation, no step
    c2, i2, info2 = softmax_fit(eng, xtr, ytr, C_, alpha=alpha, class_weight=class_weight, coef_init=coef, intercept_init=intercept)
    assert info2["converged"] and info2["iterations"] == 0 and info2["evaluations"] == 1
    assert torch.equal(c2, coef) and torch.equal(i2, intercept)
    # from the recorded float64 optimum (rounded to fp32 on the way in): still there
    c3, i3, info3 = softmax_fit(eng, xtr, ytr, C_, alpha=alpha, class_weight=class_weight, coef_init=g["Wstar"], intercept_init=g["bstar"])
    e = float(np.abs(_centred_decisions(eng, c3, i3, xte) - SP.decide(xte, g["Wstar"], g["bstar"])[0]).max())
    print(f"RESTART {case}: from the recorded optimum {info3['iterations']} iterations, {info3['evaluations']} evaluations "
          f"(from zeros {info['iterations']} / {info['evaluations']}), decision err {e:.3e}")
    assert info3["converged"] and info3["iterations"] <= info["iterations"] and e <= DECISION_TOL


def test_c_maps_onto_alpha_and_arguments_are_checked(eng):
    from plip_amd.softmax_probe import softmax_fit
    x, y, _, _ = _draw("ragged3")
    a = softmax_fit(eng, x, y, 3, alpha=0.01)
    b = softmax_fit(eng, x, y, 3, C=1.0 / (0.01 * len(x)))
    assert abs(b[2]["alpha"] - 0.01) <= 1e-15 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for kw, exc in ((dict(y=np.where(y == 2, 3, y)), "out of range"), (dict(y=np.where(y == 0, -1, y)), "out of range"),
                    (dict(x=x[:, :62]), "width"), (dict(alpha=0.0), "alpha"), (dict(alpha=float("nan")), "alpha"),
                    (dict(alpha=None, C=0.0), "C must"), (dict(alpha=None), "exactly one"), (dict(C=1.0), "exactly one"),
                    (dict(class_weight="auto"), "class_weight"), (dict(y=y[:-1]), "y must be"), (dict(n_classes=1), "two classes"),
                    (dict(n_classes=65), "at most"), (dict(max_iter=0), "max_iter"), (dict(y=y.astype(np.float32)), "integer")):
        args = dict(x=x, y=y, n_classes=3, alpha=0.01)
        args.update(kw)
        with pytest.raises(ValueError, match=exc):
            softmax_fit(eng, **args)
    with pytest.raises(ValueError, match="every class"):
        softmax_fit(eng, x, np.where(y == 2, 1, y), 3, alpha=0.01, class_weight="balanced")


def test_non_convergence_is_reported(eng):
    from plip_amd.softmax_probe import softmax_fit
    x, y, _, _ = _draw("ragged3")
    with pytest.warns(RuntimeWarning, match="did not reach"):
        coef, intercept, info = softmax_fit(eng, x, y, 3, alpha=0.01, max_iter=2)
    assert info["converged"] is False and info["iterations"] == 2 and info["grad_norm"] > 1e-7 and torch.isfinite(coef).all()


def test_softmax_prober_head(eng):
    from plip_amd.reproducibility import SoftmaxProber
    g = SP.load_case("ragged3")
    n, C_, D, alpha, class_weight = SP.shape_of("ragged3")
    xtr, ytr, xte, yte = _draw("ragged3")
    names = np.array([f"class_{i:02d}" for i in range(C_)])          # string labels, sorted like their indices
    clf, (test_m, train_m) = SoftmaxProber(alpha=alpha, class_weight=class_weight).train_and_test(xtr, list(names[ytr]), xte, list(names[yte]))
    assert test_m["split"] == "test" and train_m["split"] == "train"
    assert clf.coef_.shape == (C_, D) and clf.intercept_.shape == (C_,) and list(clf.classes_) == list(names) and clf.n_iter_ >= 1
    assert clf.predict(xte[:5]).dtype == names.dtype and clf.decision_function(xte[:5]).shape == (5, C_)
    for split, m in (("train", train_m), ("test", test_m)):
        want = dict(zip(LP.METRIC_KEYS, g[f"opt_macro_{split}"]))
        print(f"HEAD ragged3 {split}: accuracy {m['Accuracy']:.4f} macro-F1 {m['WF1']:.4f} (recorded {want['Accuracy']:.4f} / {want['WF1']:.4f})")
        assert int(g[f"under_margin_{split}"]) == 0
        for k in LP.METRIC_KEYS:
            assert abs(m[k] - want[k]) <= 1e-12 or (np.isnan(m[k]) and np.isnan(want[k])), (split, k)
    p = clf.predict_proba(xte)
    z = xte.astype(np.float64) @ clf.coef_.T + clf.intercept_
    e = np.exp(z - z.max(1, keepdims=True))
    err = float(np.abs(p - e / e.sum(1, keepdims=True)).max())
    print(f"PROBA ragged3: max |predict_proba - float64 softmax| {err:.3e}")
    assert p.shape == (len(xte), C_) and err <= 1e-5
    np.testing.assert_allclose(p.sum(1), 1.0, rtol=0, atol=1e-12)
    # the CLIP protocol's default: C = 0.316
    clf2, _ = SoftmaxProber().train_and_test(xtr, ytr, xte, yte)
    assert abs(clf2.info_["alpha"] - 1.0 / (0.316 * len(xtr))) <= 1e-15 and clf2.info_["converged"]
    with pytest.raises(ValueError, match="unseen"):
        SoftmaxProber(alpha=0.01).train_and_test(xtr, list(names[ytr]), xte[:2], ["class_00", "nope"])
