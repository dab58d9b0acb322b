"""Drop-in for the reference's top-level ``PLIP`` class (/root/reference/plip.py).

Same constructor and methods -- ``encode_images``, ``encode_text``,
``_cosine_similarity``, ``_nearest_neighbours``, ``zero_shot_classification``,
``retrieval`` -- with the model forward running in the MI355X engine.  Reference
quirks that are part of its observable behaviour are kept:
``encode_*`` return UN-normalised float32 [N,512] numpy arrays (plip.py:53,71) and
``_cosine_similarity`` normalises only the key side (plip.py:73-76).  Two latent bugs
are not reproduced: ``retrieval`` read a never-assigned ``self.image_vectors``
(plip.py:114) -- here ``index_images`` sets it -- and the batch loop no longer syncs
and copies to the host once per batch (plip.py:50): batches are enqueued back to back
and copied once.

``batch_size`` keeps its place in every signature, but it no longer sizes the ENGINE calls: the reference hard-codes
``batch_size=8`` in ``zero_shot_classification`` / ``retrieval`` (plip.py:90-91,112), a tenth of the engine's bs=256
rate.  A row's embedding is bit-identical whatever batch it travels in (tests/test_gpu_parity.py), so the host loops
prepare the caller's batches one by one (same routing, same preprocessing per batch) and hand them to the towers
``engine.max_batch`` rows at a time.  ``PLIP.coalesce = False`` restores one engine call per caller batch.

This file holds the class only.  Where a batch of images goes (native tiles / one size / differing sizes / float pixels / host Pillow),
the opening of paths and the host loops that run that decision live in ``image_routes.py``: ONE direct loop (``encode_direct``) serves
the checkpoint's resolution and ``image_size=``, and the pipelined loop uses the same ``prepare_routed_batch`` / ``consume_routed_batch``
as ``CLIPEmbedder``.  Batches are joined on the host only; every device-side step of a batch -- upload, resize + crop, encode -- is
enqueued inside the call of the lane it runs on, on that lane's engine and stream.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Union

import numpy as np
import torch

from .image_routes import PinnedPair, consume_routed_batch, encode_direct, lane_loop, open_paths, prepare_routed_batch
from .model import PlipModel
from .preprocess import load_tokenizer, preprocess_images
from .token_similarity import token_similarity

# The top-level reference class preprocesses with HF ``CLIPProcessor`` (plip.py:27,35), whose centre crop starts at
# ``(extent - n) // 2``; the reproducibility/ embedders use torchvision's rounding instead (preprocess.crop_offset).
_CROP = "hf"


def _attention_pixels(chunk, n_px) -> torch.Tensor:
    """The fp32 pixels ``attention_maps`` runs on: a float array or tensor as it is, anything else through ``preprocess_images``."""
    if torch.is_tensor(chunk) and chunk.dtype != torch.uint8:
        return chunk
    if isinstance(chunk, np.ndarray) and chunk.dtype != np.uint8:
        return torch.from_numpy(chunk)
    return torch.from_numpy(preprocess_images(list(chunk.cpu().numpy() if torch.is_tensor(chunk) else chunk), n_px, crop=_CROP))


class PLIP:
    coalesce = True          # engine calls carry up to engine.max_batch rows whatever ``batch_size`` says (module docstring)
    ragged_resize = False    # lists of differing image sizes: host Pillow (False) or the GPU's ragged resize (constructor keyword)

    def __init__(self, model_name: str = None, auth_token=None, *, model: Optional[PlipModel] = None,
                 tokenizer: Optional[Callable] = None, tokenizer_dir: Optional[str] = None, dtype: str = "bf16",
                 max_batch: int = 256, device: str = "cuda:0", pack_captions: bool = False, text_f16: bool = False,
                 text_f16_layers: Optional[int] = None, ragged_resize: bool = False, hidden_act=None):
        """``model_name``: local HF directory (what ``CLIPModel/CLIPProcessor.from_pretrained`` take, plip.py:26-27)
        or an OpenAI-clip ``.pt`` state dict.  The tokenizer comes from ``tokenizer`` (a callable), else from
        ``tokenizer_dir`` / the model directory when it holds ``vocab.json`` + ``merges.txt``; with neither,
        ``encode_text`` still takes token ids.  ``pack_captions`` (extension, 16-bit engines): the text tower computes only
        the positions up to each caption's EOS token -- bit-identical embeddings, cost proportional to the caption lengths
        instead of the padded 77 (include/plipmi.h ``plipmi_set_text_packing``).  ``dtype``: "bf16" | "f16" | "f32";
        ``text_f16`` (bf16 engine): the text tower on IEEE-half operands (PLIPMI_FLAG_TEXT_TOWER_F16); ``text_f16_layers``
        (bf16 engine): only that many leading text blocks (plipmi_config.text_f16_layers; None = the default).  The engine's other
        per-handle options (ln_fold, pooled_last_block, mfma_attention, graph_batch) are reached by building the model
        explicitly -- ``PLIP(model=PlipModel.from_pretrained(path, **engine_options))``.  ``ragged_resize`` (extension): a batch of
        uint8 / PIL images whose sizes DIFFER is resized and cropped on the GPU too (``Engine.resize_crop_ragged``, Pillow-exact)
        instead of image by image in host Pillow; batches of one size and native tiles keep their routes, float inputs and images
        shrunk more than 64 x keep the host path.  Off: every route is as before.  ``hidden_act``: the towers' MLP activation where
        the checkpoint cannot say it -- an open_clip / LAION ``.pt`` state dict needs ``hidden_act="gelu"`` -- or to override an HF
        directory's ``config.json``: "gelu", "quick_gelu" or a ``(vision, text)`` pair (``weights.load_checkpoint``)."""
        if not torch.cuda.is_available():
            raise RuntimeError("plip_amd.PLIP needs an MI355X (ROCm) GPU; there is no CPU path")
        self.device = device
        self.model_name = model_name
        if model is None and model_name is None:
            raise ValueError("give a local checkpoint path (HF dir or OpenAI .pt) or a PlipModel")
        if tokenizer is None:       # resolved BEFORE the engine is built: a bad tokenizer dir must not leak a handle
            import os
            cand = tokenizer_dir or (model_name if model_name and os.path.isdir(model_name) else None)
            if tokenizer_dir is not None and not os.path.exists(os.path.join(tokenizer_dir, "vocab.json")):
                raise FileNotFoundError(f"tokenizer_dir {tokenizer_dir!r} has no vocab.json / merges.txt")
            if cand and os.path.exists(os.path.join(cand, "vocab.json")) and os.path.exists(os.path.join(cand, "merges.txt")):
                tokenizer = load_tokenizer(cand)
        if model is None:
            model = PlipModel.from_pretrained(model_name, device=device, dtype=dtype, max_batch=max_batch, text_f16=text_f16,
                                              text_f16_layers=text_f16_layers, hidden_act=hidden_act)
        self.model = model.to(self.device)
        if pack_captions:
            self.model.engine.set_text_packing(True)
        self.tokenizer = tokenizer
        self.ragged_resize = bool(ragged_resize)
        self.model_hash = hash            # the reference returns the builtin too (plip.py:29)
        self.image_vectors = None

    # -- plip.py:31-53 -------------------------------------------------------
    def encode_images(self, images: Union[List[str], list, np.ndarray, torch.Tensor], batch_size: int,
                      num_workers: int = 0, image_size: Optional[int] = None):
        """``num_workers > 0`` (extension): decode / resize with a thread pool and stream batches through pinned
        double buffers so host work and H2D overlap the towers (plip_amd/pipeline.py); results are identical.
        ``image_size`` (extension): resize the shortest edge to it and centre-crop to image_size x image_size instead of the
        checkpoint's size, and encode with the position table interpolated to that grid (``Engine.at_resolution``, HF's
        ``interpolate_pos_encoding=True``) -- e.g. 448 for pathology tiles cut at 448 / 512 px.  None: the checkpoint's size."""
        n_px = self.model.config.image_size if image_size is None else int(image_size)
        eng = self.model.engine if image_size is None else self.model.engine.at_resolution(n_px, n_px)
        if num_workers > 0 and not torch.is_tensor(images) and not isinstance(images, np.ndarray) and len(images):
            outs = self._encode_images_pipelined(list(images), batch_size, num_workers, eng, n_px)
        else:
            cap = max(int(batch_size), int(getattr(eng, "max_batch", batch_size))) if self.coalesce else int(batch_size)
            outs = encode_direct(images, batch_size, eng, n_px, cap, _CROP, ragged=self.ragged_resize,
                                 fill_stage=self._fill_stage if self.coalesce else None)
        if not outs:
            return np.zeros((0, self.model.config.projection_dim), np.float32)
        return torch.cat(outs).detach().cpu().numpy()

    def _encode_images_pipelined(self, images: list, batch_size: int, num_workers: int, eng, n_px: int):
        """The routing of the direct loop per caller batch, one batch ahead: decoded, converted and packed on the worker threads
        (``prepare_routed_batch``), then uploaded and run inside its lane (``consume_routed_batch``)."""
        from .pipeline import run_batches
        pinned = PinnedPair()
        lanes = eng.lanes() if getattr(eng, "use_lanes", False) and hasattr(eng, "lanes") else None
        with torch.no_grad():
            return run_batches(images, min(int(batch_size), eng.max_batch), None, lambda tag, t, e=eng: consume_routed_batch(e, tag, t, _CROP),
                               device=eng.device, num_workers=num_workers, lanes=lanes,
                               prepare_batch=lambda chunk, pool: prepare_routed_batch(chunk, n_px, _CROP, pool, pinned,
                                                                                      ragged=self.ragged_resize))

    def attention_maps(self, images: Union[List[str], list, np.ndarray, torch.Tensor], batch_size: int, kind: str = "rollout",
                       image_size: Optional[int] = None) -> np.ndarray:
        """(extension) One heat-map per image over the patch grid, float32 [N, gh, gw]: ``kind="rollout"`` -- the CLS row of the
        attention rollout (residual weight 1/2, head mean: include/plipmi.h ``plipmi_encode_attention_summary``) -- or ``"last"`` --
        the CLS row of the last block's probabilities, averaged over the heads --, the CLS column dropped, reshaped to the grid and
        NOT renormalised (a map sums to 1 minus the weight CLS keeps on itself).  Runs on the pixels ``encode_images`` encodes for the
        same ``images`` / ``image_size``, prepared on the host (fp32 pixels; paths are opened, anything that is not a float array goes
        through ``preprocess_images``); the attention tensor [L,B,H,S,S] is never formed."""
        if kind not in ("rollout", "last"):
            raise ValueError(f"kind must be 'rollout' or 'last', got {kind!r}")
        n_px = self.model.config.image_size if image_size is None else int(image_size)
        eng = self.model.engine if image_size is None else self.model.engine.at_resolution(n_px, n_px)
        gh = gw = n_px // self.model.config.patch_size
        outs = []
        with torch.no_grad():
            for s in range(0, len(images), batch_size):
                px = _attention_pixels(open_paths(images[s:s + batch_size]), n_px)
                out = eng.attention_summary("vision", px, pooled_attention=kind == "last", rollout=kind == "rollout")
                row = out.rollout if kind == "rollout" else out.pooled_attention[-1].mean(dim=1)
                outs.append(row[:, 1:].reshape(-1, gh, gw))
        if not outs:
            return np.zeros((0, gh, gw), np.float32)
        return torch.cat(outs).detach().cpu().numpy()

    def similarity_maps(self, images: Union[List[str], list, np.ndarray, torch.Tensor], text, batch_size: int,
                        image_size: Optional[int] = None, softmax: bool = False, scale: Optional[float] = None) -> np.ndarray:
        """(extension) One map per image and prompt over the patch grid, float32 [N, C, gh, gw]: the cosine of every patch token's
        projected embedding with the prompt's text embedding, times ``scale`` (include/plipmi.h ``plipmi_encode_token_similarity``) --
        or, with ``softmax``, the softmax of those values over the C prompts of each patch.  ``text``: a list of prompts (needs the
        tokenizer), token ids [C, context_length], or a ready float [C, P] array of text embeddings (any norm); at most 64 prompts.
        ``scale`` None: 1.0, or ``exp(logit_scale)`` with ``softmax``.  The CLS row is dropped.  Images are handled exactly as in
        ``attention_maps``."""
        n_px = self.model.config.image_size if image_size is None else int(image_size)
        eng = self.model.engine if image_size is None else self.model.engine.at_resolution(n_px, n_px)
        gh = gw = n_px // self.model.config.patch_size
        ready = (torch.is_tensor(text) and text.is_floating_point()) or (isinstance(text, np.ndarray) and text.dtype.kind == "f")
        txt = torch.as_tensor(text if ready else self.encode_text(text, batch_size=max(int(batch_size), 1)))
        if scale is None:
            scale = float(np.exp(float(self.model.logit_scale))) if softmax else 1.0
        outs = []
        with torch.no_grad():
            for s in range(0, len(images), batch_size):
                px = _attention_pixels(open_paths(images[s:s + batch_size]), n_px)
                sim = token_similarity(eng, px, txt, scale=scale, softmax=softmax).similarity
                outs.append(sim[:, 1:].transpose(1, 2).reshape(sim.shape[0], sim.shape[2], gh, gw))
        if not outs:
            return np.zeros((0, int(txt.shape[0]), gh, gw), np.float32)
        return torch.cat(outs).detach().cpu().numpy()

    def encode_region(self, region, tile_px: Optional[int] = None, stride: Optional[int] = None, origin=(0, 0),
                      min_tissue: float = 0.5, sat_min: int = 18, luma_min: int = 25, luma_max: int = 235,
                      image_size: Optional[int] = None, band_rows: Optional[int] = None, stain=None):
        """(extension) A slide region -> the embeddings of its tissue tiles; the grid, the background filter and the stacking run on the
        GPU (region_routes.py).  ``region``: uint8 [H,W,3] -- a device tensor (any row stride: a view of a larger array is read where it
        is), or a numpy array / ``np.memmap`` / PIL image on the host, uploaded in bands of ``band_rows`` whole tile-rows (default: what a
        quarter of the free device memory holds; the result does not depend on it).  Tiles of ``tile_px`` pixels (default: the encode
        resolution) every ``stride`` pixels (default ``tile_px``; smaller overlaps, larger leaves gaps) from ``origin`` = (y0, x0); tiles
        that do not fit are dropped.  A tile is kept when at least ``ceil(min_tissue * tile_px ** 2)`` of its pixels are tissue
        (``preprocess.tissue_mask``: ``sat_min``, ``luma_min``, ``luma_max``, each 0 .. 255).  Kept tiles of another size than the encode
        resolution are resized on the GPU exactly as ``encode_images`` resizes a host list of such crops; ``image_size`` selects the
        resolution as it does there.  Returns a ``RegionEmbeddings``: ``embeddings`` float32 [K,P] (un-normalised, bit for bit what
        ``encode_images`` gives for the same crops), ``coords`` int64 [K,2], ``kept`` int64 [K], ``grid`` (rows, cols), ``tissue``
        float32 [rows, cols].  An empty grid or a region without tissue gives K = 0.  ``stain``: a one-row ``StainFit``
        (``fit_stain(region)``) -- every gathered batch is stain-normalised with it (``stain.stain_apply``, default target) between the
        gather and the resize, in the lane that encodes it; the embeddings are bit for bit ``encode_images`` of the normalised crops.
        Tissue selection still sees the raw pixels.  None: exactly the path without the keyword."""
        from .region_routes import encode_region
        n_px = self.model.config.image_size if image_size is None else int(image_size)
        eng = self.model.engine if image_size is None else self.model.engine.at_resolution(n_px, n_px)
        return encode_region(eng, region, n_px, self.model.config.projection_dim, _CROP, tile_px=tile_px, stride=stride, origin=origin,
                             min_tissue=min_tissue, sat_min=sat_min, luma_min=luma_min, luma_max=luma_max, band_rows=band_rows, stain=stain)

    def fit_stain(self, images_or_region, pooled: bool = True, step: Optional[int] = None, **params):
        """(extension) Macenko stain fit on the GPU (stain.py ``stain_fit``; ``params``: ``Io``, ``alpha``, ``beta``).
        ``images_or_region``: uint8 [H,W,3] (a region or one tile) or [B,H,W,3] (tiles of one size) -- a device tensor (read where it
        lies, any row stride), a host tensor / numpy array / ``np.memmap``, or a list of equal-size arrays.  ``pooled`` (default): ONE fit
        over all of it -- what ``encode_region(stain=...)`` and a whole slide's tiles want; False: one per image.  The fit looks at
        the pixels with ``y % step == 0 and x % step == 0``; ``step`` None is the smallest that keeps them at or under 2^22.  A host
        array is subsampled on the host (``[::step, ::step]``) BEFORE the upload and fitted with step 1: the same pixels in the same
        order, so the same bits as the device-subsampled fit, for 1 / step^2 of the upload.  Returns a ``stain.StainFit`` (rows on the
        device; nothing synchronises)."""
        from .preprocess import stain_default_step
        from .stain import _check_params, stain_fit
        x = images_or_region
        if isinstance(x, (list, tuple)):
            x = np.stack([np.asarray(i, dtype=np.uint8) for i in x]) if len(x) else np.zeros((0, 1, 1, 3), np.uint8)
        on_device = torch.is_tensor(x) and x.is_cuda
        if not on_device and not torch.is_tensor(x):
            x = np.asarray(x)                     # (a memmap stays one: only the sampled pixels are read below)
        shape = tuple(x.shape)
        if x.dtype != (torch.uint8 if torch.is_tensor(x) else np.uint8) or len(shape) not in (3, 4) or shape[-1] != 3:
            raise ValueError(f"stain images are uint8 [B,H,W,3] or [H,W,3], got {x.dtype} {shape}")
        B, H, W = (1,) + shape[:2] if len(shape) == 3 else shape[:3]
        if step is None:
            step = stain_default_step(max(B, 1), max(H, 1), max(W, 1))
        _check_params(step, params.get("Io", 240.0), params.get("alpha", 1.0), params.get("beta", 0.15))
        step = int(step)
        eng = self.model.engine
        if on_device:
            return stain_fit(eng, x, pooled=pooled, step=step, **params)
        sub = x[::step, ::step] if len(shape) == 3 else x[:, ::step, ::step]
        sub = np.ascontiguousarray(sub.numpy() if torch.is_tensor(sub) else sub)
        fit = stain_fit(eng, sub, pooled=pooled, step=1, **params)
        fit.step = step
        return fit

    def normalize_stain(self, images, fit="tile", target=None) -> torch.Tensor:
        """(extension) Stain-normalised tiles, uint8 [B,H,W,3] on the device -- what ``encode_images`` takes.  ``images``: uint8
        [B,H,W,3] tiles of one size (array, tensor on either side, or a list).  ``fit``: "tile" (each tile by its own fit), "pooled"
        (one fit over all of them) or a ``StainFit`` of 1 or B rows (``fit_stain``).  ``target``: None = Macenko's reference, or a
        one-row ``StainFit`` to normalise to another slide.  A tile whose fit is invalid (hardly any tissue) comes back unchanged."""
        from .stain import StainFit, _check_images, stain_apply, stain_fit
        if not isinstance(fit, StainFit) and fit not in ("tile", "pooled"):
            raise ValueError(f"fit must be 'tile', 'pooled' or a StainFit, got {fit!r}")
        if isinstance(images, (list, tuple)):
            images = np.stack([np.asarray(i, dtype=np.uint8) for i in images]) if len(images) else np.zeros((0, 1, 1, 3), np.uint8)
        x, single = _check_images(images)
        if single:
            raise ValueError("normalize_stain takes a batch [B,H,W,3]")
        eng = self.model.engine
        x = x if x.device == eng.device else x.contiguous().to(eng.device)
        if not isinstance(fit, StainFit):
            fit = stain_fit(eng, x, pooled=fit == "pooled", step=1)
        return stain_apply(eng, x, fit, target=target)

    def cluster_embeddings(self, embeddings, n_clusters: int, metric: str = "cosine", **kw):
        """(extension) K-means on cached embeddings [N,P] (numpy or torch, host or device) on the GPU (kmeans.py ``kmeans_fit``, whose
        keyword arguments ``init``, ``n_init``, ``max_iter``, ``tol``, ``seed`` pass through).  ``metric="cosine"`` (spherical k-means)
        L2-normalises a copy of the rows first; "euclidean" uses them as given.  Returns an ``outputs.KMeansResult``."""
        from .kmeans import _metric, _x_on_device, kmeans_fit
        _metric(metric)
        eng = self.model.engine
        x = embeddings
        if metric == "cosine":
            with torch.cuda.device(eng.device):
                x = _x_on_device(eng, embeddings, "cluster_embeddings")
                x = eng.l2_normalize_(x.clone())
        return kmeans_fit(eng, x, n_clusters, metric=metric, **kw)

    def region_mosaic(self, region, n_clusters: int, seed: int = 0, **encode_region_kwargs):
        """(extension) The "mosaic" of a slide region: ``encode_region`` (its keyword arguments pass through), spherical k-means on the
        L2-normalised tile embeddings, one representative tile per cluster.  Fewer kept tiles than ``n_clusters`` lower K to the tile
        count; a region without tissue returns empty arrays and launches nothing.  Returns a ``region_routes.RegionMosaic``."""
        from .kmeans import kmeans_fit
        from .region_routes import RegionMosaic
        if int(n_clusters) < 1:
            raise ValueError(f"region_mosaic: need n_clusters >= 1, got {n_clusters}")
        reg = self.encode_region(region, **encode_region_kwargs)
        n_tiles = reg.embeddings.shape[0]
        if n_tiles == 0:
            return RegionMosaic(reg, np.zeros((0,), np.int64), np.zeros((0, 2), np.int64), np.zeros((0,), np.int64), np.zeros((0,), np.int32),
                                np.zeros((0,), np.int32), None)
        eng = self.model.engine
        with torch.cuda.device(eng.device):
            x = eng.l2_normalize_(torch.from_numpy(np.ascontiguousarray(reg.embeddings, dtype=np.float32)).to(eng.device))
        res = kmeans_fit(eng, x, min(int(n_clusters), n_tiles), metric="cosine", seed=seed)
        reps = res.representatives.cpu().numpy().astype(np.int64)
        return RegionMosaic(reg, reps, reg.coords[reps], reg.kept[reps], res.labels.cpu().numpy(), res.counts.cpu().numpy(), res)

    def class_prototypes(self, classes, templates=("{}",), batch_size: int = 256) -> np.ndarray:
        """(extension) One text prototype per class, float32 [C, P] unit rows: the L2-normalised mean of the L2-normalised
        ``encode_text`` embeddings of every template x synonym -- CLIP's ``zeroshot_classifier`` (prompt ensembling).  ``classes``: a
        list of names, or a list of lists of synonyms; ``templates``: format strings with one ``{}``."""
        from .bags import class_prototypes
        names = [[c] if isinstance(c, str) else list(c) for c in classes]
        templates = [templates] if isinstance(templates, str) else list(templates)
        if not names or not templates or any(not n for n in names):
            raise ValueError("class_prototypes: need at least one class, one name per class and one template")
        prompts, groups = [], []
        for syn in names:
            groups.append(list(range(len(prompts), len(prompts) + len(syn) * len(templates))))
            prompts.extend(t.format(s) for s in syn for t in templates)
        return class_prototypes(self.encode_text(prompts, batch_size=batch_size), groups)

    def _prototypes(self, classes_or_prototypes, templates):
        c = classes_or_prototypes
        if torch.is_tensor(c) or isinstance(c, np.ndarray):
            return c
        return self.class_prototypes(c, templates=templates)

    def slide_zero_shot(self, bags, classes_or_prototypes, ks=(1, 5, 10, 50, 100), templates=("{}",), scale: Optional[float] = None,
                        return_top_tiles: int = 0) -> dict:
        """(extension) Slide-level zero-shot by top-K pooling (MI-Zero, CONCH) on the GPU (bags.py; include/plipmi.h "bags of
        embeddings"): every tile of every slide is scored against every class prototype, the ``k`` largest scores of a slide and class
        are averaged for every ``k`` of ``ks``, and the slide's prediction is the first arg-max over the classes -- one call for the
        whole cohort.  ``bags``: a list of [n_b, P] tile embeddings (one per slide), ``(embeddings [N, P], offsets [S + 1])`` or
        ``(embeddings [N, P], slide_ids [N])`` (slides in ``np.unique`` order); numpy or torch, un-normalised as ``encode_images``
        returns them: a copy is L2-normalised on the device.  ``classes_or_prototypes``: class names / lists of synonyms
        (``class_prototypes`` with ``templates``), or a ready float [C, P] array used as given; at most 64 classes.  ``scale`` None:
        the model's ``exp(logit_scale)``.  Returns a dict of numpy arrays: ``pooled`` float32 [S, nks, C] (NaN for a slide without
        tiles), ``pred`` int32 [S, nks] (-1 for such a slide), ``ks``, and with ``return_top_tiles`` = R <= ks[-1] ``top_tiles`` int64
        [S, C, R], the best tiles per slide and class (``bags.slide_zero_shot`` says what they index)."""
        from .bags import slide_zero_shot
        if scale is None:
            scale = float(np.exp(float(self.model.logit_scale)))
        return slide_zero_shot(self.model.engine, bags, self._prototypes(classes_or_prototypes, templates), ks=ks, scale=float(scale),
                               return_top_tiles=return_top_tiles)

    def region_zero_shot(self, region, classes_or_prototypes, ks=(1, 5, 10, 50, 100), templates=("{}",), scale: Optional[float] = None,
                         return_top_tiles: int = 10, **encode_region_kwargs) -> dict:
        """(extension) ``encode_region`` (its keyword arguments pass through), then ``slide_zero_shot`` with the region's kept tiles as
        ONE bag.  Returns what ``slide_zero_shot`` returns (S = 1; ``return_top_tiles`` is lowered to ks[-1]), plus ``top_coords`` int64
        [C, R, 2] -- the (y, x) of the top tiles' top-left pixels, -1 where there are fewer tiles -- and ``region``, the
        ``RegionEmbeddings``.  A region without tissue launches nothing: NaN ``pooled``, ``pred`` -1."""
        from .bags import check_ks
        kv = check_ks(ks, "region_zero_shot")
        R = min(int(return_top_tiles), int(kv[-1]))
        protos = self._prototypes(classes_or_prototypes, templates)
        reg = self.encode_region(region, **encode_region_kwargs)
        n_classes = int(protos.shape[0])
        if reg.embeddings.shape[0] == 0:
            res = {"pooled": np.full((1, kv.size, n_classes), np.nan, np.float32), "pred": np.full((1, kv.size), -1, np.int32),
                   "ks": tuple(int(k) for k in kv)}
            if R:
                res["top_tiles"] = np.full((1, n_classes, R), -1, np.int64)
        else:
            res = self.slide_zero_shot((reg.embeddings, np.array([0, reg.embeddings.shape[0]], np.int32)), protos, ks=kv, scale=scale,
                                       return_top_tiles=R)
        if R:
            top = res["top_tiles"][0]
            res["top_coords"] = np.where((top >= 0)[..., None], reg.coords[np.maximum(top, 0)], -1) if len(reg.coords) else \
                np.full((n_classes, R, 2), -1, np.int64)
        res["region"] = reg
        return res

    def encode_views(self, images, batch_size: int, views: int = 8, transform: str = "d4", seed: int = 0, reduce: Optional[str] = None,
                     return_params: bool = False):
        """(extension) Embeddings of ``views`` augmented views of every tile, the views built on the GPU (augment.py; Pillow-exact
        warps, include/plipmi.h ``plipmi_warp_u8``) inside the lane that encodes them.  ``images``: uint8 RGB tiles of ONE size -- an
        array or tensor [N,H,W,3] (a device tensor is read where it is) or a list of arrays / PIL images.  ``transform``:

        ``"d4"``     the symmetries of the square in the order of ``preprocess.dihedral_coeffs`` (view 0 is the tile itself), ``views``
                     <= 8; tiles at the encode resolution.  Exact re-indexing: test-time augmentation over orientations.
        ``"train"``  the reference's ``_train_transform`` (reproducibility/embedders/transform.py): a random n_px crop, a horizontal
                     flip, ``RandomAffine(10, translate .1, scale (.8, 1.2), shear +-15, BILINEAR, fill 127)`` and
                     ``RandomPerspective(0.3, p=0.3)``, each stage through bytes as the PIL chain; tiles with H, W >= n_px.  Its
                     first step, ``Resize([512])``, is NOT done here: it is the resize route ``encode_images`` and
                     ``Engine.resize_crop_u8`` already have -- resize first where the tiles are not at the size to crop from.  The
                     draws of view v of tile i come from ``np.random.default_rng([seed, i, v])`` (``preprocess.sample_train_params``):
                     they do not depend on ``batch_size``, the order of the calls or the lane, and nothing claims torch's stream.

        Returns float32 [N, views, P], un-normalised rows, each bit for bit what ``encode_images`` gives for that view's bytes;
        ``reduce="mean"``: float32 [N, P], the L2-normalised mean over the views of the L2-normalised rows.  ``return_params``: also the
        ``(windows [N,V,5], affine [N,V,8], perspective [N,V,8])`` rows the views were made with (``preprocess.train_view_reference`` /
        ``warp_reference`` regenerate their bytes).  ``batch_size`` tiles (times ``views`` rows) go to a lane at a time.  ValueError
        before anything is uploaded or launched: mixed sizes, tiles smaller than n_px, ``views`` > 8 for "d4", an unknown transform."""
        from .augment import encode_views
        return encode_views(self.model.engine, images, batch_size, self.model.config.image_size, self.model.config.projection_dim, views=views,
                            transform=transform, seed=seed, reduce=reduce, return_params=return_params)

    _stages = None           # tile size -> pinned uint8 [max_batch, n, n, 3] staging rows of the direct loop (allocated on first use)

    def _fill_stage(self, tiles, n_px, cap) -> torch.Tensor:
        """The native tiles of one engine call (arrays or PIL) -> the first len(tiles) rows of the pinned staging buffer of that tile
        size (one per size: a caller alternating between resolutions does not reallocate pinned memory).
        (Plain row copies: a thread pool was measured 3x slower -- numpy keeps the GIL for 150 KB copies.)"""
        if self._stages is None:
            self._stages = {}
        stage = self._stages.get(n_px)
        if stage is None or stage.shape[0] < cap:
            stage = self._stages[n_px] = torch.empty((cap, n_px, n_px, 3), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        dst = stage.numpy()
        for i, im in enumerate(tiles):
            dst[i] = im if isinstance(im, np.ndarray) else np.asarray(im.convert("RGB"), dtype=np.uint8)
        return stage[:len(tiles)]

    # -- plip.py:55-71 ---------------------------------------------------------
    def encode_text(self, text: Union[List[str], np.ndarray, torch.Tensor], batch_size: int):
        ctx = self.model.config.context_length
        if torch.is_tensor(text) or isinstance(text, np.ndarray):
            ids, mask = torch.as_tensor(text), None      # already tokenised
        else:
            if self.tokenizer is None:
                raise RuntimeError("no tokenizer: pass tokenizer=... or token ids")
            ids, mask = self.tokenizer(list(text), ctx)
            ids, mask = torch.as_tensor(ids), (None if mask is None else torch.as_tensor(mask))
        outs = []
        step = int(batch_size)
        if self.coalesce:      # the captions are tokenised already: only the size of the engine calls changes
            step = max(step, int(getattr(self.model.engine, "max_batch", step)))
        with torch.no_grad(), lane_loop(self.model.engine) as run:
            for s in range(0, len(ids), step):
                m = None if mask is None else mask[s:s + step]
                outs.append(run(lambda e, s=s, m=m: e.encode_text(ids[s:s + step], m, normalize=False)))
        if not outs:
            return np.zeros((0, self.model.config.projection_dim), np.float32)
        return torch.cat(outs).detach().cpu().numpy()

    # -- plip.py:73-76 -----------------------------------------------------------
    def _cosine_similarity(self, key_vectors: np.ndarray, space_vectors: np.ndarray, normalize=True):
        eng = self.model.engine
        k = torch.as_tensor(np.ascontiguousarray(key_vectors, dtype=np.float32)).to(eng.device)
        s = torch.as_tensor(np.ascontiguousarray(space_vectors, dtype=np.float32)).to(eng.device)
        if normalize:
            k = eng.l2_normalize_(k.clone())            # only the key side, as the reference does
        lpi, _, _ = eng.logits(k, s, scale=1.0, want_text=False)
        return lpi.cpu().numpy()

    # -- plip.py:78-87 -----------------------------------------------------------
    def _nearest_neighbours(self, k, key_vectors, space_vectors, normalize=True, debug=False):
        eng = self.model.engine
        key_vectors, space_vectors = np.asarray(key_vectors), np.asarray(space_vectors)
        # argsort()[:, -k:] (plip.py:84) is a SLICE: it hands back every column when k exceeds the corpus, every column for
        # k = 0 ([-0:] is [0:]), and for k < 0 it drops the |k| weakest columns ([|k|:] of the ascending order), i.e. keeps
        # the n - |k| best.  Same counts here instead of failing.
        n_space = space_vectors.shape[0]
        k = int(k)
        k = n_space if k == 0 else (max(n_space + k, 0) if k < 0 else min(k, n_space))
        if k == 0 or key_vectors.shape[0] == 0:
            return np.zeros((key_vectors.shape[0], k), np.int64)
        kv = torch.as_tensor(np.ascontiguousarray(key_vectors, dtype=np.float32)).to(eng.device)
        sv = torch.as_tensor(np.ascontiguousarray(space_vectors, dtype=np.float32)).to(eng.device)
        if normalize:
            kv = eng.l2_normalize_(kv.clone())          # only the key side, as the reference does (plip.py:74-76)
        if debug:
            print(self._cosine_similarity(key_vectors, space_vectors, normalize=normalize))
        if kv.shape[1] % 32 == 0 and k <= 1024:
            return eng.similarity_topk(kv, sv, k).cpu().numpy()     # fused: no [Nq, Ns] matrix
        lpi, _, _ = eng.logits(kv, sv, scale=1.0, want_text=False)
        return eng.topk(lpi, k).cpu().numpy()

    # -- plip.py:89-103 ----------------------------------------------------------
    def zero_shot_classification(self, images, text_labels: List[str], debug=False):
        text_vectors = self.encode_text(text_labels, batch_size=8)
        image_vectors = self.encode_images(images, batch_size=8)
        cosine_sim = self._cosine_similarity(image_vectors, text_vectors)
        if debug:
            print(cosine_sim)
        preds = np.argmax(cosine_sim, axis=-1)
        return [text_labels[idx] for idx in preds]

    def index_images(self, images, batch_size: int = 256):
        """Embed the retrieval corpus (the reference forgot to: plip.py:114 reads self.image_vectors)."""
        self.image_vectors = self.encode_images(images, batch_size=batch_size)
        return self.image_vectors

    # -- plip.py:105-114 -----------------------------------------------------------
    def retrieval(self, queries: List[str], top_k: int = 10):
        if self.image_vectors is None:
            raise RuntimeError("call index_images(images) before retrieval()")
        text_vectors = self.encode_text(queries, batch_size=8)
        return self._nearest_neighbours(k=top_k, key_vectors=text_vectors, space_vectors=self.image_vectors)
