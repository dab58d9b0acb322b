"""MI355X stand-ins for the pieces of the reference's ``reproducibility/`` tree that sit on the
embedding hot path:

=====================================================  ==========================================
reference                                              here
=====================================================  ==========================================
reproducibility/embedders/plip.py   ``CLIPEmbedder``   :class:`embedders.CLIPEmbedder`
reproducibility/embedders/factory.py                   :class:`embedders.EmbedderFactory`
reproducibility/utils/cacher.py                        :mod:`cacher` (same file names and .npy bytes)
reproducibility/evaluation/zero_shot/zero_shot.py      :class:`evaluation.ZeroShotClassifier`
(no counterpart: the same head over slides)            :class:`evaluation.SlideZeroShotClassifier`
reproducibility/evaluation/retrieval/retrieval.py      :class:`evaluation.ImageRetrieval`
reproducibility/evaluation/linear_probing/             :class:`linear_probe.LinearProber`
reproducibility/metrics.py                             :mod:`metrics`
reproducibility/fine_tuning/finetune.py (frozen tower:
``LinearClassifier`` + ``nn.CrossEntropyLoss()``)      :class:`softmax_probe.SoftmaxProber`
=====================================================  ==========================================

The towers, the normalisation, the similarity product, the arg-max, the top-50 and the linear probe's
loss-and-gradient passes and predictions all run in libplipmi.so on the GPU; only file I/O, label bookkeeping and the metric arithmetic stay on the host.
"""
from .cacher import (cache_hit_or_miss, cache_hit_or_miss_raw_filename, cache_numpy_object,  # noqa: F401
                     cache_numpy_object_raw_filename, get_cache_name, get_savepath)
from .embedders import CLIPEmbedder, EmbedderFactory  # noqa: F401
from .evaluation import ImageRetrieval, SlideZeroShotClassifier, ZeroShotClassifier  # noqa: F401
from .linear_probe import LinearProber  # noqa: F401
from .metrics import eval_metrics, retrieval_metrics  # noqa: F401
from .softmax_probe import SoftmaxProber  # noqa: F401
