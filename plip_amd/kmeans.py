"""K-means on cached embeddings (include/plipmi.h "k-means on cached embeddings"; csrc/kmeans.hip): Lloyd's algorithm with the
assignment, the update, the finalise step and the k-means++ seeding on the GPU.  Functions on an engine, not methods of it:
``kmeans_fit(engine, x, n_clusters)`` and ``kmeans_assign(engine, x, centers)``; ``PLIP.cluster_embeddings`` and ``PLIP.region_mosaic``
route here.  Runs on the given engine alone and keeps no state.

* ``metric="euclidean"``: scikit-learn's ``KMeans(algorithm="lloyd")`` -- the label is the nearest centre, the new centre the mean of its
  members, ``inertia`` the sum of squared distances.
* ``metric="cosine"``: spherical k-means on rows used AS GIVEN (pass unit rows; ``PLIP.cluster_embeddings`` normalises them) -- the label
  is the centre of largest dot product, the new centre the members' sum divided by its norm, ``inertia`` the sum of ``1 - x.c``.
* Ties go to the lower cluster.  The same inputs give the same bits on every run.
* Seeding is plain k-means++ D^2 sampling from host uniforms -- NOT scikit-learn's greedy variant, so its draws differ from sklearn's.
* An empty cluster takes the row farthest from its centre (in ascending cluster order, ties to the lower row); ``relocations`` counts them.
"""
from __future__ import annotations

import ctypes as C_
import math

import numpy as np
import torch

from . import _lib
from ._lib import _ptr
from .outputs import KMeansResult


def _metric(metric: str) -> int:
    if metric not in _lib.KMEANS_METRICS:
        raise ValueError(f"metric must be 'euclidean' or 'cosine', got {metric!r}")
    return _lib.KMEANS_METRICS[metric]


def _check_k(k: int, n_rows: int, what: str) -> int:
    k = int(k)
    if k < 1 or k > _lib.KMEANS_MAX_K or k > n_rows:
        raise ValueError(f"{what}: need 1 <= n_clusters <= min(N, {_lib.KMEANS_MAX_K}), got n_clusters = {k} with N = {n_rows}")
    return k


def _x_on_device(engine, x, what: str) -> torch.Tensor:
    n_rows, width = engine._probe_shape(x, what)
    if not (torch.is_tensor(x) and x.device == engine.device):
        engine._probe_fits(n_rows, width, what, " (X larger than device memory is not provided)")
    return engine._probe_x(x, what)


def kmeans_seed(engine, x, n_clusters: int, metric: str = "cosine", uniforms=None, seed=0):
    """k-means++ D^2 sampling on the device: ``(centers [K, D], picks int32 [K])`` with ``centers[t] = x[picks[t]]``.  ``uniforms``: K
    float64 values in [0, 1) (default: ``np.random.default_rng(seed).random(K)``)."""
    m = _metric(metric)
    n_rows, _ = engine._probe_shape(x, "kmeans_seed")
    K = _check_k(n_clusters, n_rows, "kmeans_seed")
    u = np.random.default_rng(seed).random(K) if uniforms is None else np.ascontiguousarray(uniforms, dtype=np.float64)
    if u.shape != (K,) or not np.all((u >= 0) & (u < 1)):
        raise ValueError(f"kmeans_seed: uniforms must be {K} values in [0, 1)")
    with torch.cuda.device(engine.device):
        xd = _x_on_device(engine, x, "kmeans_seed")
        centers = torch.empty((K, xd.shape[1]), dtype=torch.float32, device=engine.device)
        picks = torch.empty((K,), dtype=torch.int32, device=engine.device)
        _lib.check(engine.lib.plipmi_kmeans_seed(engine._h, _ptr(xd), xd.shape[0], xd.shape[1], K, m, u.ctypes.data_as(C_.POINTER(C_.c_double)),
                                                 _ptr(centers), _ptr(picks), engine._stream()), "plipmi_kmeans_seed")
    return centers, picks


def kmeans_assign(engine, x, centers, metric: str = "cosine"):
    """``(labels int32 [N], scores fp32 [N])`` of rows ``x`` [N, D] for ``centers`` [K, D]: the first arg-max over k of
    ``x_i . c_k + h_k`` (``h_k = -|c_k|^2 / 2`` for "euclidean", 0 for "cosine") and that maximum.  Device tensors; enqueues only."""
    m = _metric(metric)
    n_rows, width = engine._probe_shape(x, "kmeans_assign")
    cshape = tuple(centers.shape)
    if len(cshape) != 2 or cshape[1] != width:
        raise ValueError(f"kmeans_assign: centers must be [K, {width}], got {cshape}")
    K = _check_k(cshape[0], n_rows, "kmeans_assign")
    with torch.cuda.device(engine.device):
        xd = _x_on_device(engine, x, "kmeans_assign")
        cd = torch.as_tensor(centers, dtype=torch.float32).to(engine.device).contiguous()
        labels = torch.empty((n_rows,), dtype=torch.int32, device=engine.device)
        scores = torch.empty((n_rows,), dtype=torch.float32, device=engine.device)
        _lib.check(engine.lib.plipmi_kmeans_assign(engine._h, _ptr(xd), n_rows, width, _ptr(cd), K, m, _ptr(labels), _ptr(scores),
                                                   engine._stream()), "plipmi_kmeans_assign")
    return labels, scores


def kmeans_fit(engine, x, n_clusters: int, metric: str = "cosine", init="k-means++", n_init: int = 1, max_iter: int = 300,
               tol: float = 1e-4, seed: int = 0) -> KMeansResult:
    """Cluster rows ``x`` [N, D] (host numpy or torch, either side) into ``n_clusters``.  ``init``: "k-means++" (restart r draws its K
    uniforms from ``np.random.default_rng([seed, r])``) or an array [K, D] of starting centres (then ``n_init`` must be 1).  ``tol`` is
    scikit-learn's relative figure: the loop stops when the summed squared centre shift is at most ``tol`` times the mean per-feature
    variance of ``x``; ``tol=0`` runs until no label changes.  ``n_init`` > 1 keeps the restart of lowest inertia.  Reaching
    ``max_iter`` is reported through ``converged``, not raised.  Returns an ``outputs.KMeansResult`` (device tensors, Python scalars)
    whose labels, scores, counts, representatives and inertia all belong to the returned centers."""
    m = _metric(metric)
    n_rows, width = engine._probe_shape(x, "kmeans_fit")
    K = _check_k(n_clusters, n_rows, "kmeans_fit")
    given = not isinstance(init, str)
    if not given and init != "k-means++":
        raise ValueError(f"init must be 'k-means++' or an array [K, D], got {init!r}")
    if given and tuple(init.shape) != (K, width):
        raise ValueError(f"kmeans_fit: init must be [{K}, {width}], got {tuple(init.shape)}")
    if int(n_init) < 1 or (given and int(n_init) != 1):
        raise ValueError("kmeans_fit: need n_init >= 1, and n_init == 1 with given centres")
    if int(max_iter) < 1 or not (math.isfinite(tol) and tol >= 0):
        raise ValueError("kmeans_fit: need max_iter >= 1 and a finite tol >= 0")
    best = None
    with torch.cuda.device(engine.device):
        xd = _x_on_device(engine, x, "kmeans_fit")
        tol_abs = float(tol) * float(xd.var(dim=0, unbiased=False).mean()) if tol > 0 else 0.0
        for restart in range(int(n_init)):
            if given:
                centers = torch.as_tensor(init, dtype=torch.float32).to(engine.device).contiguous().clone()
            else:
                centers, _ = kmeans_seed(engine, xd, K, metric, uniforms=np.random.default_rng([int(seed), restart]).random(K))
            labels = torch.empty((n_rows,), dtype=torch.int32, device=engine.device)
            scores = torch.empty((n_rows,), dtype=torch.float32, device=engine.device)
            counts = torch.empty((K,), dtype=torch.int32, device=engine.device)
            reps = torch.empty((K,), dtype=torch.int32, device=engine.device)
            info = _lib.KMeansInfo()
            _lib.check(engine.lib.plipmi_kmeans_fit(engine._h, _ptr(xd), n_rows, width, K, m, int(max_iter), tol_abs, _ptr(centers),
                                                    _ptr(labels), _ptr(scores), _ptr(counts), _ptr(reps), C_.byref(info), engine._stream()),
                       "plipmi_kmeans_fit")
            res = KMeansResult(centers, labels, scores, counts, reps, float(info.inertia), int(info.iterations), bool(info.converged),
                               int(info.relocations))
            if best is None or res.inertia < best.inertia:
                best = res
    return best
