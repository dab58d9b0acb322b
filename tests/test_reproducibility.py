"""Host-side pieces of plip_amd.reproducibility: cache naming/bytes and metric arithmetic.

The compatibility pin for SURVEY.md section 8f row 4: the same calls made through the reference's own cacher.py / metrics.py,
recorded by oracle/make_reference_fixtures.py into tests/golden/ (reference_reproducibility.json: names, save paths and metric
values; reference_cache_*.npy: the files its cacher writes, byte for byte) and compared here."""
import hashlib
import json
import os

import numpy as np
import pytest

from plip_amd.reproducibility import cacher, metrics

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the inputs the recorded reference calls were made on (oracle/make_reference_fixtures.py imports them from here)
CACHE_KEYS = (("pliptxtlabels", "/a/b/c.pt"), ("cliptxt", "ViT-B/32"))
SAVEPATH_KEYS = (("clipimgWSSS4LUAD_binary", "RN50"), ("plipimgDigestPath.csv", "/a/b/c.pt"))


def interchange_array():
    return np.random.RandomState(1).randn(5, 512).astype(np.float32)


def metric_cases():
    """([(y_true, y_pred, scores or None) per label set], (targets, predictions) of retrieval_metrics), seeded."""
    rng = np.random.RandomState(7)
    ev = []
    for labels in ([0, 1], [0, 1, 2, 3, 4], ["a", "b", "c"]):
        yt = [labels[i] for i in rng.randint(0, len(labels), 257)]
        yp = [labels[i] for i in rng.randint(0, len(labels), 257)]
        sc = rng.rand(257) if len(labels) == 2 else None
        ev.append((yt, yp, sc))
    pred = rng.randint(0, 60, size=(40, 50))
    return ev, (list(range(40)), pred)


def _recorded():
    with open(os.path.join(GOLDEN_DIR, "reference_reproducibility.json")) as f:
        return json.load(f)


def test_cache_names_and_roundtrip(tmp_path, monkeypatch):
    monkeypatch.setenv("PC_CACHE_FOLDER", str(tmp_path))
    x = np.random.RandomState(0).randn(7, 512).astype(np.float32)
    # hashed scheme (text side)
    assert cacher.cache_hit_or_miss("pliptxtKather", "/ckpt/epoch_3.pt") is None
    cacher.cache_numpy_object(x, "pliptxtKather", "/ckpt/epoch_3.pt")
    want = os.path.join(str(tmp_path), hashlib.sha256(b"pliptxtKather/ckpt/epoch_3.pt").hexdigest())
    assert os.path.exists(want) and cacher.get_cache_name("pliptxtKather", "/ckpt/epoch_3.pt") == want
    np.testing.assert_array_equal(cacher.cache_hit_or_miss("pliptxtKather", "/ckpt/epoch_3.pt"), x)
    # raw-file-name scheme (image side): <folder>/<dataset>/<model>/<basename of backbone for plip>
    assert cacher.cache_hit_or_miss_raw_filename("plipimgKather_test.csv", "/ckpt/epoch_3.pt") is None
    cacher.cache_numpy_object_raw_filename(x, "plipimgKather_test.csv", "/ckpt/epoch_3.pt")
    assert os.path.exists(os.path.join(str(tmp_path), "Kather_test", "plip", "epoch_3.pt"))
    np.testing.assert_array_equal(cacher.cache_hit_or_miss_raw_filename("plipimgKather_test.csv", "/ckpt/epoch_3.pt"), x)
    assert cacher.get_savepath("clipimgPanNuke", "ViT-B-32") == os.path.join(str(tmp_path), "PanNuke", "clip", "ViT-B-32")
    # the payload is a plain .npy stream
    with open(want, "rb") as f:
        assert f.read(6) == b"\x93NUMPY"
    monkeypatch.delenv("PC_CACHE_FOLDER")
    with pytest.raises(KeyError):
        cacher.get_cache_name("a", "b")


def test_cache_is_interchangeable_with_the_reference(tmp_path, monkeypatch):
    rec = _recorded()
    monkeypatch.setenv("PC_CACHE_FOLDER", str(tmp_path))
    x = interchange_array()
    ref_bytes = open(os.path.join(GOLDEN_DIR, "reference_cache_n_p.npy"), "rb").read()       # the reference's np.save of x
    for name, path, want in rec["cache_names"]:
        assert cacher.get_cache_name(name, path) == os.path.join(str(tmp_path), want)
    with open(cacher.get_cache_name("pliptxtlabels", "/a/b/c.pt"), "wb") as f:              # written by the reference ...
        f.write(ref_bytes)
    np.testing.assert_array_equal(cacher.cache_hit_or_miss("pliptxtlabels", "/a/b/c.pt"), x)   # ... is our hit
    cacher.cache_numpy_object_raw_filename(x * 2, "plipimgDigestPath.csv", "/a/b/c.pt")       # and the reverse: where the
    saved = dict(((n, p), w) for n, p, w in rec["savepaths"])                                 # reference looks, its own bytes
    ours = os.path.join(str(tmp_path), saved[("plipimgDigestPath.csv", "/a/b/c.pt")])
    assert (open(ours, "rb").read() == open(os.path.join(GOLDEN_DIR, "reference_cache_raw_digestpath.npy"), "rb").read())
    np.testing.assert_array_equal(np.load(ours), x * 2)
    assert cacher.get_savepath("clipimgWSSS4LUAD_binary", "RN50") == os.path.join(str(tmp_path), saved[("clipimgWSSS4LUAD_binary", "RN50")])
    a = tmp_path / "ours"
    a.mkdir()
    monkeypatch.setenv("PC_CACHE_FOLDER", str(a)); cacher.cache_numpy_object(x, "n", "p")
    fn = hashlib.sha256(b"np").hexdigest()
    assert (a / fn).read_bytes() == ref_bytes                                                 # byte-identical files


def test_retrieval_metrics():
    pred = np.array([[0] + list(range(100, 149)), [5] * 9 + [1] + [7] * 40, [9] * 10 + [2] + [8] * 39, [4] * 50])
    m = metrics.retrieval_metrics([0, 1, 2, 3], pred)
    assert m == {"p@10": 0.5, "p@50": 0.75}
    assert metrics.retrieval_metrics([0], np.array([[3, 0]])) == {"p@10": 1.0, "p@50": 1.0}   # fewer than 10 columns


@pytest.mark.parametrize("labels", [[0, 1], [0, 1, 2, 3], ["Tumor", "Normal", "Stroma"]])
def test_eval_metrics_against_closed_forms(labels):
    rng = np.random.RandomState(len(labels))
    yt = [labels[i] for i in rng.randint(0, len(labels), 300)]
    yp = [labels[i] for i in rng.randint(0, len(labels), 300)]
    m = metrics.eval_metrics(yt, yp)
    assert m["instances"] == 300 and abs(m["Accuracy"] - np.mean([a == b for a, b in zip(yt, yp)])) < 1e-12
    # support-weighted recall equals accuracy; F1 lies between 0 and 1; MCC of identical vectors is 1
    assert abs(m["recall"] - m["Accuracy"]) < 1e-12 and 0 <= m["WF1"] <= 1
    assert abs(metrics.eval_metrics(yt, yt)["mcc"] - 1.0) < 1e-12
    if labels == [0, 1]:
        tp = sum(a == 1 and b == 1 for a, b in zip(yt, yp)); fn = sum(a == 1 and b == 0 for a, b in zip(yt, yp))
        assert (m["tp"], m["fn"]) == (tp, fn) and abs(m["sensitivity"] - tp / (tp + fn)) < 1e-12
        sc = rng.rand(300)
        auc = metrics.eval_metrics(yt, yp, sc)["AUC"]
        pos, neg = sc[np.array(yt) == 1], sc[np.array(yt) == 0]
        assert abs(auc - np.mean(pos[:, None] > neg[None, :])) < 1e-12
    else:
        assert np.isnan(m["AUC"]) and (m["tp"] == 0 or labels[1] == 1)


def test_eval_metrics_match_the_reference():
    rec = _recorded()
    ev, ret = metric_cases()
    for (yt, yp, sc), theirs in zip(ev, rec["eval_metrics"]):
        ours = metrics.eval_metrics(yt, yp, sc)
        assert ours.keys() == theirs.keys()
        for k in ours:
            a, b = ours[k], theirs[k]
            assert (np.isnan(a) and np.isnan(b)) or abs(a - b) < 1e-12, k
    assert len(rec["eval_metrics"]) == len(ev) == 3
    assert metrics.retrieval_metrics(*ret) == rec["retrieval_metrics"]
