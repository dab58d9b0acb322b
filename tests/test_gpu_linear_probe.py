"""Linear-probe head on the GPU against the recorded float64 optimum (tests/golden/linear_probe_*.npz, made on a CPU by
tools/make_linear_probe_golden.py) and the numpy float64 restatement of the objective (tests/linear_probe_common.py) -- never
against the code under test.

Bounds.  The kernel and fit bounds are 4 x the figures measured on one MI355X and recorded in profiles/linear_probe_parity.txt
(fp32 sums over up to 12 000 rows in a fixed but arbitrary order: 4 x covers another tile order on a later change); every test
prints its figures before it asserts.  DELTA, the margin below which a row's prediction is not compared, is 10 x the largest
decision-value error measured after the fit; the rows it leaves out may be at most 2 % of a split, and a DELTA above 1e-3 would mean
the solver is not converged."""
import numpy as np
import pytest
import torch

import linear_probe_common as LP

pytestmark = pytest.mark.gpu

CASES = list(LP.CASES)
# 4 x the measured values of profiles/linear_probe_parity.txt
KERNEL_LOSS_REL = 4 * 3.397e-08
KERNEL_GRAD_REL = 4 * 4.149e-08
FIT_W = {"hard9": 4 * 5.434e-08, "loose9": 4 * 4.026e-05, "bin2": 4 * 8.346e-07, "ragged3": 4 * 9.495e-07}
FIT_B = {"hard9": 4 * 1.354e-07, "loose9": 4 * 2.659e-06, "bin2": 4 * 3.102e-08, "ragged3": 4 * 5.522e-07}
# the gap is a difference of two float64 evaluations of f_k (sums of 12 000 terms: about 1e-13 of rounding each), so it has that floor
FIT_GAP = {"hard9": max(4 * 4.94e-15, 1e-12), "loose9": max(4 * 4.66e-11, 1e-12), "bin2": max(4 * 4.40e-14, 1e-12), "ragged3": max(4 * 3.36e-13, 1e-12)}
DELTA = 10 * 5.093e-05
assert DELTA <= 1e-3


@pytest.fixture(scope="module")
def eng():
    from plip_amd.engine import heads_engine
    return heads_engine()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dtype=dtype)


def _eval(eng, x, y, C_, alpha, W, b):
    """(loss float64 [K], grad float64 [K, D + 1]) of one kernel evaluation, and the raw tensors"""
    from plip_amd.kernel_entries import probe_loss_grad
    pos_w, neg_w = LP.sample_weights(y, C_)
    wb = np.concatenate([W, b[:, None]], axis=1).astype(np.float32)
    loss, grad = probe_loss_grad(eng, _dev(x, torch.float32), _dev(y, torch.int32), _dev(wb, torch.float32),
                                 _dev(pos_w, torch.float32), _dev(neg_w, torch.float32), alpha)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), grad.cpu().numpy().astype(np.float64), (loss, grad), wb


def kernel_errors(eng, x, y, C_, alpha, W, b):
    loss, grad, raw, wb = _eval(eng, x, y, C_, alpha, W, b)
    pos_w, neg_w = LP.sample_weights(y, C_)
    # the reference sees the SAME fp32 point and fp32 sample weights the kernel saw
    f, gW, gb, G = LP.objective(x, y, C_, alpha, wb[:, :-1], wb[:, -1])
    e_loss = float((np.abs(loss - f) / f).max())
    e_grad = float((np.abs(grad - np.concatenate([gW, gb[:, None]], axis=1)) / G[:, None]).max())
    again = _eval(eng, x, y, C_, alpha, W, b)[2]
    assert torch.equal(raw[0], again[0]) and torch.equal(raw[1], again[1]), "two evaluations of the same inputs differ in bits"
    return e_loss, e_grad


def _points(g, K, D):
    rs = np.random.RandomState(5)
    return (("zero", np.zeros((K, D)), np.zeros(K)), ("optimum", g["Wstar"], g["bstar"]),
            ("random", rs.standard_normal((K, D)), rs.standard_normal(K)))


@pytest.mark.parametrize("case", CASES)
def test_kernel_loss_and_gradient(eng, case):
    g = LP.load_case(case)
    _, _, C_, D, alpha, _ = LP.CASES[case]
    x, y, _, _ = LP.draw(case)
    K = 1 if C_ == 2 else C_
    for name, W, b in _points(g, K, D):
        e_loss, e_grad = kernel_errors(eng, x, y, C_, alpha, W, b)
        print(f"KERNEL {case} {name}: loss rel err {e_loss:.3e}  grad err / G {e_grad:.3e}")
        assert e_loss <= KERNEL_LOSS_REL and e_grad <= KERNEL_GRAD_REL, (case, name, e_loss, e_grad)


@pytest.mark.parametrize("C_,D,n", [(20, 128, 1000), (64, 768, 333), (33, 1024, 70)])
def test_kernel_more_than_sixteen_problems(eng, C_, D, n):
    rs = np.random.RandomState(100 + C_)
    x = rs.standard_normal((n, D)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = rs.randint(0, C_, n)
    y[:C_] = np.arange(C_)
    for name, W, b in (("zero", np.zeros((C_, D)), np.zeros(C_)), ("random", rs.standard_normal((C_, D)), rs.standard_normal(C_))):
        e_loss, e_grad = kernel_errors(eng, x, y, C_, 0.003, W, b)
        print(f"KERNEL K={C_} D={D} N={n} {name}: loss rel err {e_loss:.3e}  grad err / G {e_grad:.3e}")
        assert e_loss <= KERNEL_LOSS_REL and e_grad <= KERNEL_GRAD_REL, (C_, name, e_loss, e_grad)


def test_kernel_ignores_labels_outside_the_classes(eng):
    """a label that is no problem's positive one is a negative everywhere: nothing is indexed by it"""
    x, y, _, _ = LP.draw("ragged3")
    bad = y.copy()
    bad[5], bad[6] = 1 << 30, -7
    rs = np.random.RandomState(2)
    W, b = rs.standard_normal((3, 64)), rs.standard_normal(3)
    pos_w, neg_w = LP.sample_weights(y, 3)
    from plip_amd.kernel_entries import probe_loss_grad
    wb = np.concatenate([W, b[:, None]], axis=1).astype(np.float32)
    loss, grad = probe_loss_grad(eng, _dev(x, torch.float32), _dev(bad, torch.int32), _dev(wb, torch.float32),
                                 _dev(pos_w, torch.float32), _dev(neg_w, torch.float32), 0.01)
    z = x.astype(np.float64) @ wb[:, :-1].astype(np.float64).T + wb[:, -1]
    pos = bad[:, None] == np.arange(3)[None, :]
    c = np.where(pos, pos_w, neg_w)
    tz = np.where(pos, z, -z)
    f = (c * (np.log1p(np.exp(-np.abs(tz))) + np.maximum(-tz, 0))).sum(0) / len(x) + 0.005 * (wb[:, :-1].astype(np.float64) ** 2).sum(1)
    np.testing.assert_allclose(loss.cpu().numpy(), f, rtol=1e-5)
    assert torch.isfinite(grad).all()


_FITS = {}


def _fit(eng, case):
    if case not in _FITS:
        _, _, C_, D, alpha, _ = LP.CASES[case]
        xtr, ytr, xte, yte = LP.draw(case)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("error")              # non-convergence is a RuntimeWarning: a failure here
            coef, intercept, info = eng.probe_fit(xtr, ytr, C_, alpha)
        _FITS[case] = (coef, intercept, info, xtr, ytr, xte, yte)
    return _FITS[case]


def _decision_err(eng, g, coef, intercept, x):
    _, dec = eng.probe_predict(x, coef, intercept, return_decision=True)
    z, _, _ = LP.decide(x, g["Wstar"], g["bstar"])
    return float(np.abs(dec.cpu().numpy().astype(np.float64) - z).max())


@pytest.mark.parametrize("case", CASES)
def test_fit_reaches_the_recorded_optimum(eng, case):
    g = LP.load_case(case)
    _, _, C_, D, alpha, _ = LP.CASES[case]
    coef, intercept, info, xtr, ytr, xte, yte = _fit(eng, case)
    assert info["converged"] and info["grad_norm"] <= 2e-8 and info["evaluations"] > info["iterations"] >= 1
    W, b = coef.cpu().numpy().astype(np.float64), intercept.cpu().numpy().astype(np.float64)
    f = LP.objective(xtr, ytr, C_, alpha, W, b)[0]
    e_w, e_b = float(np.abs(W - g["Wstar"]).max()), float(np.abs(b - g["bstar"]).max())
    gap = (f - g["fstar"]) / g["fstar"]
    sgd_gap = (g["sgd_f"] - g["fstar"]) / g["fstar"]
    e_dec = max(_decision_err(eng, g, coef, intercept, xtr), _decision_err(eng, g, coef, intercept, xte))
    print(f"FIT {case}: iterations {info['iterations']} evaluations {info['evaluations']} |grad|_inf {info['grad_norm']:.2e}  "
          f"max|W-W*| {e_w:.3e} max|b-b*| {e_b:.3e} gap {gap.min():.2e}..{gap.max():.2e} (SGD {sgd_gap.min():.2e}..{sgd_gap.max():.2e})  "
          f"decision err {e_dec:.3e}")
    np.testing.assert_allclose(info["loss"], f, rtol=1e-6)           # the solver's own f_k is the objective's value there
    assert e_w <= FIT_W[case] and e_b <= FIT_B[case] and gap.max() <= FIT_GAP[case], (case, e_w, e_b, gap.max())
    assert 10 * e_dec <= DELTA * 1.0000001, (case, e_dec)
    if sgd_gap.max() > 1e-4:     # a condition, not a measurement: a better minimiser of the reference's objective than its own solver
        assert (gap < sgd_gap).all(), (case, gap, sgd_gap)


@pytest.mark.parametrize("case", CASES)
def test_predictions_equal_the_optimum_outside_the_margin(eng, case):
    g = LP.load_case(case)
    coef, intercept, info, xtr, ytr, xte, yte = _fit(eng, case)
    for split, x in (("train", xtr), ("test", xte)):
        pred = eng.probe_predict(x, coef, intercept).cpu().numpy()
        keep = g[f"opt_margin_{split}"] >= DELTA
        left = int((~keep).sum())
        print(f"PREDICT {case} {split}: {left} of {len(keep)} rows under margin {DELTA:.1e}, {int((pred != g[f'opt_pred_{split}']).sum())} rows differ")
        assert left <= 0.02 * len(keep)
        assert np.array_equal(pred[keep], g[f"opt_pred_{split}"][keep].astype(pred.dtype))


def test_predict_first_argmax_binary_rule_and_chunks(eng):
    rs = np.random.RandomState(8)
    x = rs.standard_normal((203, 64)).astype(np.float32)
    W = rs.standard_normal((20, 64)).astype(np.float32)
    W[7] = W[3]                                          # a tie: the first maximum wins
    b = np.zeros(20, np.float32)
    pred, dec = eng.probe_predict(x, W, b, return_decision=True)
    z = x.astype(np.float64) @ W.astype(np.float64).T
    np.testing.assert_allclose(dec.cpu().numpy(), z, atol=2e-5)
    assert np.array_equal(pred.cpu().numpy(), dec.cpu().numpy().argmax(1))
    assert not (pred.cpu().numpy() == 7).any()
    assert torch.equal(eng.probe_predict(x, W, b, chunk_rows=50), pred)
    p1, d1 = eng.probe_predict(x, W[:1], b[:1], return_decision=True)
    assert d1.shape == (203, 1) and np.array_equal(p1.cpu().numpy(), (d1.cpu().numpy()[:, 0] > 0).astype(np.int32))


@pytest.mark.parametrize("case", CASES)
def test_linear_prober_head(eng, case):
    from plip_amd.reproducibility import LinearProber
    from plip_amd.reproducibility.metrics import eval_metrics
    g = LP.load_case(case)
    xtr, ytr, xte, yte = LP.draw(case)
    names = np.array([f"class_{i:02d}" for i in range(LP.CASES[case][2])])          # string labels, sorted like their indices
    clf, (test_m, train_m) = LinearProber(alpha=LP.CASES[case][4]).train_and_test(xtr, list(names[ytr]), xte, list(names[yte]))
    assert test_m["split"] == "test" and train_m["split"] == "train"
    K = 1 if len(names) == 2 else len(names)
    assert clf.coef_.shape == (K, xtr.shape[1]) and clf.intercept_.shape == (K,) and list(clf.classes_) == list(names)
    assert clf.n_iter_ >= 1 and clf.predict(xte[:5]).dtype == names.dtype
    dec = clf.decision_function(xte[:5])
    assert dec.shape == ((5,) if K == 1 else (5, K))
    for split, m, y in (("train", train_m, ytr), ("test", test_m, yte)):
        want = eval_metrics(list(y), list(g[f"opt_pred_{split}"].astype(np.int64)), average_method="macro")
        left = int((g[f"opt_margin_{split}"] < DELTA).sum())
        sgd = dict(zip(LP.METRIC_KEYS, g[f"sgd_macro_{split}"]))
        print(f"HEAD {case} {split}: accuracy {m['Accuracy']:.4f} macro-F1 {m['WF1']:.4f} (optimum {want['Accuracy']:.4f} / {want['WF1']:.4f}; "
              f"recorded SGD {sgd['Accuracy']:.4f} / {sgd['WF1']:.4f}); {left} rows under the margin")
        if left == 0:
            for k in LP.METRIC_KEYS:
                assert m[k] == want[k] or (np.isnan(m[k]) and np.isnan(want[k])), (case, split, k)
        else:
            assert abs(m["Accuracy"] - want["Accuracy"]) <= left / len(y)
    with pytest.raises(ValueError, match="unseen"):
        LinearProber(alpha=0.01).train_and_test(xtr, list(names[ytr]), xte[:2], ["class_00", "nope"])


def test_same_bits_from_numpy_and_device_inputs_and_either_engine(eng, engines):
    model, cfg, sd, px, ids, mask = engines("tiny_b6", "f32")
    x, y, xte, _ = LP.draw("ragged3")
    before = model.engine.encode_image(torch.from_numpy(px)).clone()
    a = eng.probe_fit(x, y, 3, 0.01)
    b = eng.probe_fit(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 3, 0.01)
    c = model.engine.probe_fit(x, torch.from_numpy(y), 3, 0.01)
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1]) and a[2]["evaluations"] == other[2]["evaluations"]
    pa = eng.probe_predict(xte, a[0], a[1])
    assert torch.equal(pa, model.engine.probe_predict(torch.from_numpy(xte).cuda(), a[0].cpu().numpy(), a[1].cpu().numpy()))
    after = model.engine.encode_image(torch.from_numpy(px))
    assert torch.equal(before, after), "a fit on the handle disturbed the following encode_image"


def test_engine_validates_before_the_device_sees_anything(eng):
    x, y, _, _ = LP.draw("ragged3")
    for kw, exc in ((dict(y=np.where(y == 2, 3, y)), "out of range"), (dict(y=np.where(y == 0, -1, y)), "out of range"),
                    (dict(x=x[:, :62]), "width"), (dict(alpha=0.0), "alpha"), (dict(alpha=float("nan")), "alpha"),
                    (dict(class_weight="auto"), "class_weight"), (dict(y=y[:-1]), "y must be"), (dict(n_classes=1), "two classes"),
                    (dict(n_classes=65, class_weight=None), "at most"), (dict(max_iter=0), "max_iter")):
        args = dict(x=x, y=y, n_classes=3, alpha=0.01)
        args.update(kw)
        with pytest.raises(ValueError, match=exc):
            eng.probe_fit(**args)
    class Huge:                     # an x that cannot fit: refused from its shape alone, nothing is allocated
        shape = (1 << 40, 512)
    with pytest.raises(ValueError, match="free"):
        eng.probe_fit(Huge(), np.zeros(4, np.int64), 2, 0.01, class_weight=None)
    with pytest.raises(ValueError, match="every class"):
        eng.probe_fit(x, np.where(y == 2, 1, y), 3, 0.01)


def test_non_convergence_is_reported(eng):
    x, y, _, _ = LP.draw("ragged3")
    with pytest.warns(RuntimeWarning, match="did not reach"):
        coef, intercept, info = eng.probe_fit(x, y, 3, 0.01, max_iter=2)
    assert not info["converged"] and info["iterations"] == 2 and info["grad_norm"] > 1e-7 and torch.isfinite(coef).all()
