"""Bags of cached embeddings (include/plipmi.h "bags of embeddings"; csrc/bags.hip): slide-level zero-shot by top-K pooling of tile
scores, as MI-Zero and CONCH do it for pathology CLIP models, and the mean tile embedding of a slide.  Functions on an engine, not methods
of it: ``bag_topk_pool(engine, x, offsets, class_embeds)``, ``bag_pool_scores(engine, scores_t, offsets)``, ``bag_mean(engine, x,
offsets)``; ``PLIP.slide_zero_shot`` / ``PLIP.region_zero_shot`` and ``reproducibility.SlideZeroShotClassifier`` route here.  They run on
the given engine alone, keep no state and only enqueue.

* A bag is a contiguous row range: bag ``b`` is rows ``[offsets[b], offsets[b + 1])`` of ``x`` [N, D]; empty bags are allowed.
  ``bag_offsets`` builds the offsets from bag sizes, or from per-row slide ids (a stable sort; it returns the permutation).
* ``s[c, i] = scale * (x_i . t_c)`` with rows used AS GIVEN (pass unit rows for cosine; ``PLIP.slide_zero_shot`` normalises them).
* Order: the larger score first, equal scores: the lower row first; -0.0 == +0.0; a NaN counts as -inf.
* ``pooled[b, j, c]`` = the mean of the ``min(ks[j], n_b)`` first-ranked scores of bag b and class c (float64 sum in a fixed association,
  rounded once), NaN for an empty bag; ``pred[b, j]`` = the first arg-max over c, -1 for an empty bag; ``top_idx[b, c, r]`` = the row of x
  of rank r, -1 beyond ``min(kmax, n_b)``.  The same inputs give the same bits on every run.
"""
from __future__ import annotations

import ctypes as C_

import numpy as np
import torch

from . import _lib
from ._lib import _ptr

DEFAULT_KS = (1, 5, 10, 50, 100)


# ---- checks: pure functions, no GPU ------------------------------------------------------------------------------------------------
def bag_offsets(sizes=None, ids=None):
    """``(offsets int32 [S + 1], order)``.  From ``sizes`` (non-negative bag lengths): their exclusive prefix sums, ``order`` None.  From
    ``ids`` (one slide id per row, any order, any sortable dtype): the rows sorted STABLY by id -- ``x[order]`` is bag-contiguous, bag s
    holds the rows of the s-th smallest id in their original order -- with ``order`` int64 [N]; the ids of the bags are
    ``np.unique(ids)``."""
    if (sizes is None) == (ids is None):
        raise ValueError("bag_offsets: give exactly one of sizes and ids")
    if sizes is not None:
        sz = np.asarray(sizes)
        if sz.ndim != 1 or sz.size < 1 or sz.dtype.kind not in "iu" or (sz < 0).any():
            raise ValueError("bag_offsets: sizes must be a non-empty 1-d array of non-negative integers")
        total = int(sz.astype(np.int64).sum())
        if total >= 2 ** 31:
            raise ValueError(f"bag_offsets: {total} rows do not fit an int32 offset")
        return np.concatenate([[0], np.cumsum(sz.astype(np.int64))]).astype(np.int32), None
    idv = np.asarray(ids)
    if idv.ndim != 1 or idv.size < 1:
        raise ValueError("bag_offsets: ids must be a non-empty 1-d array, one id per row")
    if idv.size >= 2 ** 31:
        raise ValueError(f"bag_offsets: {idv.size} rows do not fit an int32 offset")
    order = np.argsort(idv, kind="stable").astype(np.int64)
    _, counts = np.unique(idv, return_counts=True)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), order


def check_offsets(offsets, n_rows: int, what: str = "bags") -> np.ndarray:
    """``offsets`` as int32 [S + 1] on the host, or ValueError: integers, S >= 1, offsets[0] == 0, non-decreasing, offsets[S] == N"""
    off = offsets.detach().cpu().numpy() if torch.is_tensor(offsets) else np.asarray(offsets)
    if off.ndim != 1 or off.size < 2 or off.dtype.kind not in "iu":
        raise ValueError(f"{what}: offsets must be a 1-d integer array of S + 1 >= 2 values, got {off.dtype} {tuple(off.shape)}")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != int(n_rows):
        raise ValueError(f"{what}: offsets must start at 0 and end at N = {int(n_rows)}, got {int(off[0])} .. {int(off[-1])}")
    if (np.diff(off) < 0).any():
        raise ValueError(f"{what}: offsets must be non-decreasing")
    if int(n_rows) >= 2 ** 31:
        raise ValueError(f"{what}: N = {int(n_rows)} does not fit an int32 offset")
    return off.astype(np.int32)


def check_ks(ks, what: str = "bags") -> np.ndarray:
    """``ks`` as int32 [nks], or ValueError: 1 .. 8 strictly ascending integers in 1 .. 1024"""
    arr = np.asarray([ks] if np.isscalar(ks) else list(ks))
    if arr.ndim != 1 or not 1 <= arr.size <= _lib.BAG_MAX_KS or arr.dtype.kind not in "iu":
        raise ValueError(f"{what}: ks must be 1 .. {_lib.BAG_MAX_KS} integers, got {ks!r}")
    if (arr < 1).any() or (arr > _lib.BAG_MAX_K).any():
        raise ValueError(f"{what}: every k must lie in 1 .. {_lib.BAG_MAX_K}, got {ks!r}")
    if (np.diff(arr) <= 0).any():
        raise ValueError(f"{what}: ks must be strictly ascending, got {ks!r}")
    return arr.astype(np.int32)


def _float_dtype(a) -> bool:
    return a.dtype.is_floating_point if torch.is_tensor(a) else np.asarray(a).dtype.kind == "f"


def check_embeddings(x, what: str = "bags"):
    """``(N, D)`` of float rows ``x`` [N >= 1, D], D % 4 == 0, 4 <= D <= 1024, or ValueError"""
    shape = tuple(x.shape)
    if len(shape) != 2 or shape[0] < 1:
        raise ValueError(f"{what}: x must be [N >= 1, D], got {shape}")
    if shape[1] % 4 or not 4 <= shape[1] <= 1024:
        raise ValueError(f"{what}: embedding width {shape[1]} unsupported (D % 4 == 0, 4 <= D <= 1024)")
    if not _float_dtype(x):
        raise ValueError(f"{what}: x must be floating point, got {x.dtype}")
    return int(shape[0]), int(shape[1])


def check_classes(class_embeds, width: int, what: str = "bags") -> int:
    """C of float class rows [1 <= C <= 64, width], or ValueError"""
    shape = tuple(class_embeds.shape)
    if len(shape) != 2 or shape[1] != width:
        raise ValueError(f"{what}: class_embeds must be [C, {width}], got {shape}")
    if not 1 <= shape[0] <= _lib.BAG_MAX_CLASSES:
        raise ValueError(f"{what}: need 1 <= C <= {_lib.BAG_MAX_CLASSES} classes per call, got {shape[0]} (split the classes)")
    if not _float_dtype(class_embeds):
        raise ValueError(f"{what}: class_embeds must be floating point, got {class_embeds.dtype}")
    return int(shape[0])


def check_scores(scores_t, what: str = "bags"):
    """``(C, N)`` of float class-major scores [1 <= C <= 64, N >= 1], or ValueError"""
    shape = tuple(scores_t.shape)
    if len(shape) != 2 or shape[1] < 1 or not 1 <= shape[0] <= _lib.BAG_MAX_CLASSES:
        raise ValueError(f"{what}: scores_t must be class-major [1 <= C <= {_lib.BAG_MAX_CLASSES}, N >= 1], got {shape}")
    if not _float_dtype(scores_t):
        raise ValueError(f"{what}: scores_t must be floating point, got {scores_t.dtype}")
    return int(shape[0]), int(shape[1])


# ---- the entries -------------------------------------------------------------------------------------------------------------------
def _f32_on_device(engine, a) -> torch.Tensor:
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float32))
    t = t.to(device=engine.device, dtype=torch.float32).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _workspace(engine, n_rows, n_bags, n_classes, kmax) -> torch.Tensor:
    nbytes = int(engine.lib.plipmi_bag_workspace(n_rows, n_bags, n_classes, kmax))
    if nbytes == 0:
        raise ValueError(f"bags: sizes N = {n_rows}, S = {n_bags}, C = {n_classes}, kmax = {kmax} are refused")
    return torch.empty((nbytes,), dtype=torch.uint8, device=engine.device)


def _ks_ptr(ks: np.ndarray):
    return ks.ctypes.data_as(C_.POINTER(C_.c_int32))


def _outputs(engine, S, nks, C, kmax, return_indices):
    pooled = torch.empty((S, nks, C), dtype=torch.float32, device=engine.device)
    pred = torch.empty((S, nks), dtype=torch.int32, device=engine.device)
    top = torch.empty((S, C, kmax), dtype=torch.int32, device=engine.device) if return_indices else None
    return pooled, pred, top


def bag_topk_pool(engine, x, offsets, class_embeds, ks=DEFAULT_KS, scale: float = 1.0, return_indices: bool = False,
                  return_scores: bool = False) -> dict:
    """Score every row of ``x`` [N, D] against ``class_embeds`` [C <= 64, D] and pool per bag.  Returns a dict of device tensors:
    ``pooled`` fp32 [S, nks, C], ``pred`` int32 [S, nks], ``ks`` (the tuple), with ``return_indices`` ``top_idx`` int32 [S, C, kmax], with
    ``return_scores`` ``scores`` fp32 [C, N]."""
    n_rows, width = check_embeddings(x, "bag_topk_pool")
    n_classes = check_classes(class_embeds, width, "bag_topk_pool")
    off = check_offsets(offsets, n_rows, "bag_topk_pool")
    kv = check_ks(ks, "bag_topk_pool")
    S, kmax = off.size - 1, int(kv[-1])
    with torch.cuda.device(engine.device):
        xd, td = engine._probe_x(x, "bag_topk_pool"), _f32_on_device(engine, class_embeds)
        od = torch.from_numpy(off).to(engine.device)
        ws = _workspace(engine, n_rows, S, n_classes, kmax)
        pooled, pred, top = _outputs(engine, S, kv.size, n_classes, kmax, return_indices)
        scores = torch.empty((n_classes, n_rows), dtype=torch.float32, device=engine.device) if return_scores else None
        _lib.check(engine.lib.plipmi_bag_topk_pool(engine._h, _ptr(xd), n_rows, width, _ptr(od), S, _ptr(td), n_classes, float(scale),
                                                   _ks_ptr(kv), kv.size, _ptr(ws), _ptr(pooled), _ptr(pred), _ptr(top), _ptr(scores),
                                                   engine._stream()), "plipmi_bag_topk_pool")
    out = {"pooled": pooled, "pred": pred, "ks": tuple(int(k) for k in kv)}
    if return_indices:
        out["top_idx"] = top
    if return_scores:
        out["scores"] = scores
    return out


def bag_pool_scores(engine, scores_t, offsets, ks=DEFAULT_KS, return_indices: bool = False) -> dict:
    """Pool class-major per-tile scores ``scores_t`` [C <= 64, N] (``Engine.logits``' transposed output, a probe's decision values; a
    device view with a row stride >= N is read where it lies).  Returns what ``bag_topk_pool`` returns, without ``scores``."""
    n_classes, n_rows = check_scores(scores_t, "bag_pool_scores")
    off = check_offsets(offsets, n_rows, "bag_pool_scores")
    kv = check_ks(ks, "bag_pool_scores")
    S, kmax = off.size - 1, int(kv[-1])
    with torch.cuda.device(engine.device):
        sd = scores_t
        in_place = (torch.is_tensor(sd) and sd.device == engine.device and sd.dtype == torch.float32 and sd.stride(1) == 1
                    and (n_classes == 1 or sd.stride(0) >= n_rows))
        if not in_place:
            sd = _f32_on_device(engine, sd)
        ld = int(sd.stride(0)) if n_classes > 1 else n_rows
        od = torch.from_numpy(off).to(engine.device)
        ws = _workspace(engine, n_rows, S, n_classes, kmax)
        pooled, pred, top = _outputs(engine, S, kv.size, n_classes, kmax, return_indices)
        _lib.check(engine.lib.plipmi_bag_pool_scores(engine._h, _ptr(sd), ld, n_rows, n_classes, _ptr(od), S, _ks_ptr(kv), kv.size, _ptr(ws),
                                                     _ptr(pooled), _ptr(pred), _ptr(top), engine._stream()), "plipmi_bag_pool_scores")
    out = {"pooled": pooled, "pred": pred, "ks": tuple(int(k) for k in kv)}
    if return_indices:
        out["top_idx"] = top
    return out


def bag_mean(engine, x, offsets, normalize: bool = True) -> torch.Tensor:
    """The mean row of every bag, fp32 [S, D] on the device (float64 sums, rounded once); ``normalize``: divided by its norm.  Zeros for
    an empty bag or a zero norm."""
    n_rows, width = check_embeddings(x, "bag_mean")
    off = check_offsets(offsets, n_rows, "bag_mean")
    S = off.size - 1
    with torch.cuda.device(engine.device):
        xd = engine._probe_x(x, "bag_mean")
        od = torch.from_numpy(off).to(engine.device)
        ws = _workspace(engine, n_rows, S, 1, 1)
        mean = torch.empty((S, width), dtype=torch.float32, device=engine.device)
        _lib.check(engine.lib.plipmi_bag_mean(engine._h, _ptr(xd), n_rows, width, _ptr(od), S, int(bool(normalize)), _ptr(ws), _ptr(mean),
                                              engine._stream()), "plipmi_bag_mean")
    return mean


# ---- the caller's forms of a cohort ------------------------------------------------------------------------------------------------
def as_bags(bags, what: str = "bags"):
    """``(rows, offsets int32 [S + 1], order)`` of a cohort given as a list of [n_b, D] arrays / tensors (concatenated on the host unless
    all are tensors of one device), as ``(embeddings [N, D], offsets [S + 1])`` or as ``(embeddings [N, D], slide_ids [N])``.  ``order``
    (int64 [N] or None): ``rows[order]`` is bag-contiguous -- slide ids are sorted stably, bag s is the s-th smallest id.  A second
    member that is a valid offsets array for N rows is read as offsets; build offsets with ``bag_offsets(ids=...)`` to be explicit."""
    if isinstance(bags, (tuple, list)) and len(bags) == 2 and len(getattr(bags[0], "shape", ())) == 2 and np.ndim(bags[1]) == 1:
        x, second = bags
        sec = second.detach().cpu().numpy() if torch.is_tensor(second) else np.asarray(second)
        n_rows = int(x.shape[0])
        if sec.dtype.kind in "iu" and sec.size >= 2 and sec[0] == 0 and sec[-1] == n_rows and not (np.diff(sec.astype(np.int64)) < 0).any():
            return x, sec.astype(np.int32), None
        if sec.size != n_rows:
            raise ValueError(f"{what}: the second member must be offsets [S + 1] (0 .. N = {n_rows}, non-decreasing) or one slide id per row, "
                             f"got {sec.size} values")
        off, order = bag_offsets(ids=sec)
        return x, off, order
    if not isinstance(bags, (tuple, list)) or not len(bags):
        raise ValueError(f"{what}: give a non-empty list of [n_b, D] arrays, (embeddings, offsets) or (embeddings, slide_ids)")
    widths = {tuple(b.shape)[1:] for b in bags}
    if any(len(tuple(b.shape)) != 2 for b in bags) or len(widths) != 1:
        raise ValueError(f"{what}: every bag must be [n_b, D] with one D, got {[tuple(b.shape) for b in bags][:8]}")
    off, _ = bag_offsets(sizes=[int(b.shape[0]) for b in bags])
    if all(torch.is_tensor(b) for b in bags) and len({b.device for b in bags}) == 1:
        return torch.cat([b.to(torch.float32) for b in bags]), off, None
    rows = [b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b) for b in bags]
    return np.concatenate([np.asarray(r, dtype=np.float32) for r in rows]), off, None


def normalized_rows(engine, x, order=None) -> torch.Tensor:
    """a private fp32 copy of ``x`` on the engine's device, permuted by ``order`` and L2-normalised there"""
    with torch.cuda.device(engine.device):
        t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
        t = t.to(device=engine.device, dtype=torch.float32)
        t = t[torch.from_numpy(order).to(engine.device)] if order is not None else t.clone()
        return engine.l2_normalize_(t.contiguous())


def class_prototypes(embeddings, groups) -> np.ndarray:
    """CLIP's ``zeroshot_classifier`` on ready text embeddings: prototype c = the L2-normalised mean of the L2-normalised rows
    ``groups[c]`` (index lists) of ``embeddings`` [M, D]; float64 arithmetic, float32 [C, D] result"""
    e = np.asarray(embeddings, dtype=np.float64)
    e = e / np.linalg.norm(e, axis=1, keepdims=True)
    protos = np.stack([e[np.asarray(g, dtype=np.int64)].mean(axis=0) for g in groups])
    return (protos / np.linalg.norm(protos, axis=1, keepdims=True)).astype(np.float32)


def slide_zero_shot(engine, bags, prototypes, ks=DEFAULT_KS, scale: float = 1.0, return_top_tiles: int = 0) -> dict:
    """``PLIP.slide_zero_shot`` below the prompts: the cohort in any form of ``as_bags``, rows L2-normalised on the device, scored
    against ``prototypes`` [C, D] (as given) and pooled.  numpy results: ``pooled`` [S, nks, C], ``pred`` [S, nks], ``ks``; with
    ``return_top_tiles`` = R <= ks[-1] also ``top_tiles`` int64 [S, C, R]: rows of the caller's ``embeddings`` (a list of bags: rows
    of the bag itself), -1 where the bag is shorter."""
    kv = check_ks(ks, "slide_zero_shot")
    R = int(return_top_tiles)
    if R < 0 or R > int(kv[-1]):
        raise ValueError(f"slide_zero_shot: return_top_tiles must lie in 0 .. ks[-1] = {int(kv[-1])}, got {return_top_tiles}")
    x, off, order = as_bags(bags, "slide_zero_shot")
    check_embeddings(x, "slide_zero_shot")
    check_classes(prototypes, int(x.shape[1]), "slide_zero_shot")
    out = bag_topk_pool(engine, normalized_rows(engine, x, order), off, prototypes, ks=kv, scale=scale, return_indices=R > 0)
    res = {"pooled": out["pooled"].cpu().numpy(), "pred": out["pred"].cpu().numpy(), "ks": out["ks"]}
    if R:
        top = out["top_idx"][:, :, :R].cpu().numpy().astype(np.int64)
        if order is not None:
            top = np.where(top >= 0, order[np.maximum(top, 0)], -1)
        elif not (len(bags) == 2 and np.ndim(bags[1]) == 1):
            top = np.where(top >= 0, top - off[:-1].astype(np.int64)[:, None, None], -1)
        res["top_tiles"] = top
    return res
