"""Zero-shot and retrieval evaluation heads on the GPU.

* ``ZeroShotClassifier`` (reproducibility/evaluation/zero_shot/zero_shot.py:5-28): ``score = img @ txt.T`` and the
  per-row arg-max run in one ``plipmi_logits`` launch; only the [N] int32 predictions come back.  The reference
  pickles its predictions and calls ``exit()`` before returning (zero_shot.py:21-25, a debugging leftover); this
  class returns ``(train_metrics, test_metrics)`` as the signature promises and writes the pickle only on request.
* ``ImageRetrieval`` (reproducibility/evaluation/retrieval/retrieval.py:5-30): the reference loops over N captions
  doing an [N]-vector product and a full argsort each; here ``plipmi_similarity_topk`` produces the 50 best image
  indices per caption without ever holding the [N, N] score matrix.
* ``SlideZeroShotClassifier`` (an extension; the reference stops at tiles): ``ZeroShotClassifier`` over slides by top-K pooling of
  the tile scores, one ``plipmi_bag_topk_pool`` call for the cohort.
"""
from __future__ import annotations

import logging
from typing import Optional, Sequence

import numpy as np
import torch

from ..engine import Engine, heads_engine
from .metrics import eval_metrics, retrieval_metrics


def _dev(x, eng: Engine) -> torch.Tensor:
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
    return t.to(device=eng.device, dtype=torch.float32)


class ZeroShotClassifier:
    def __init__(self, engine: Optional[Engine] = None):
        self._engine = engine

    def predict(self, image_embeddings, text_embeddings, unique_labels: Sequence):
        eng = self._engine or heads_engine()
        _, _, am = eng.logits(_dev(image_embeddings, eng), _dev(text_embeddings, eng), scale=1.0, want_text=False,
                              want_argmax=True)
        return [unique_labels[i] for i in am.cpu().tolist()]

    def zero_shot_classification(self, image_embeddings, text_embeddings, unique_labels, target_labels,
                                 pickle_path: Optional[str] = None):
        predictions = self.predict(image_embeddings, text_embeddings, unique_labels)
        test_metrics = eval_metrics(target_labels, predictions)
        train_metrics = dict(test_metrics)
        test_metrics["split"] = "test"
        train_metrics["split"] = "train"
        if pickle_path:
            import pickle
            with open(pickle_path, "wb") as f:
                pickle.dump({"target": target_labels, "predictions": predictions}, f)
        logging.info("ZeroShot Done")
        return train_metrics, test_metrics


class SlideZeroShotClassifier:
    """``ZeroShotClassifier`` over slides (an extension: the reference has no slide-level head): the tile scores ``img @ txt.T`` of a
    slide are top-K pooled -- the mean of the ``k`` largest per class, MI-Zero's rule -- and the slide takes the class of the largest
    pooled score (bags.py, one call for the whole cohort).  Embeddings are used as given, like ``ZeroShotClassifier``; slides are
    reported in ``np.unique(slide_ids)`` order; at most 64 classes."""

    def __init__(self, engine: Optional[Engine] = None, k: int = 50):
        self._engine = engine
        self.k = int(k)

    def predict(self, image_embeddings, slide_ids, text_embeddings, unique_labels: Sequence):
        from ..bags import bag_offsets, bag_topk_pool
        eng = self._engine or heads_engine()
        offsets, order = bag_offsets(ids=np.asarray(slide_ids))
        img = _dev(image_embeddings, eng)
        if img.shape[0] != len(order):
            raise ValueError(f"need one slide id per embedding, got {len(order)} ids for {img.shape[0]} rows")
        rows = img[torch.from_numpy(order).to(eng.device)].contiguous()
        pred = bag_topk_pool(eng, rows, offsets, _dev(text_embeddings, eng), ks=(self.k,), scale=1.0)["pred"]
        return [unique_labels[i] for i in pred[:, 0].cpu().tolist()]

    def zero_shot_classification(self, image_embeddings, slide_ids, text_embeddings, unique_labels, target_labels,
                                 pickle_path: Optional[str] = None):
        """``target_labels``: one per slide, in ``np.unique(slide_ids)`` order.  The metric dicts of ``ZeroShotClassifier``."""
        predictions = self.predict(image_embeddings, slide_ids, text_embeddings, unique_labels)
        test_metrics = eval_metrics(target_labels, predictions)
        train_metrics = dict(test_metrics)
        test_metrics["split"] = "test"
        train_metrics["split"] = "train"
        if pickle_path:
            import pickle
            with open(pickle_path, "wb") as f:
                pickle.dump({"target": target_labels, "predictions": predictions}, f)
        logging.info("SlideZeroShot Done")
        return train_metrics, test_metrics


class ImageRetrieval:
    def __init__(self, engine: Optional[Engine] = None, top_k: int = 50):
        self._engine = engine
        self.top_k = top_k

    def best_scores(self, image_embeddings, text_embeddings) -> np.ndarray:
        """int64 [N_text, min(50, N_images)]: image indices by descending dot product (retrieval.py:13-16)."""
        eng = self._engine or heads_engine()
        img, txt = _dev(image_embeddings, eng), _dev(text_embeddings, eng)
        k = min(self.top_k, img.shape[0])
        if img.shape[1] % 32 == 0:
            return eng.similarity_topk(txt, img, k).cpu().numpy()
        lpi, _, _ = eng.logits(txt, img, scale=1.0, want_text=False)      # odd widths: materialised fallback on the GPU
        return eng.topk(lpi, k).cpu().numpy()

    def retrieval(self, image_embeddings, text_embeddings):
        best = self.best_scores(image_embeddings, text_embeddings)
        targets = list(range(0, len(image_embeddings)))                 # caption i belongs to image i (retrieval.py:20)
        test_metrics = retrieval_metrics(targets, best)
        train_metrics = dict(test_metrics)
        test_metrics["split"] = "test"
        train_metrics["split"] = "train"
        logging.info("Retrieval Done")
        return train_metrics, test_metrics
