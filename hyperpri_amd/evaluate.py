"""Evaluate a split on the device: the threshold search, the test metrics and the colour-coded segmentation maps.

The reference's other two entry scripts around ``src/PLTrainer.py``: ``kfold_validate.py`` -> ``validate_net`` (:533-609, the
PR curve and the best-Dice threshold) and ``kfold_segmaps.py`` -> ``test_net`` (:631-661) + ``eval_color_segmaps`` (:219-267).
There every batch of logits goes ``.cpu()`` (``predict_step``, :142-162), the curve, AP and the confusion matrix are torchmetrics
objects on the host, and one overlay copies a whole cube to the host to read three of its bands.  Here the logits, the masks and
the cubes stay on the card; what crosses PCIe is a few scalars, the 501-point curve and 3 bytes per pixel of finished picture.

    cache = CubeCache(...); cache.fill(validation_split)
    pred  = predict_split(net, cache.epoch(batch_size=2, shuffle=False))
    val   = validate_net(pred)                                   # {'best_threshold', 'precision', 'recall', 'dice', ...}
    write_segmaps(fig_dir, pred, cache.epoch(batch_size=2, shuffle=False), val["best_threshold"])
    test  = test_net(predict_split(net, test_batches), val["best_threshold"])

Test-time augmentation (``hyperpri_amd.tta``, ``csrc/tta.hip``) is opt-in and changes nothing when it is off: with ``tta=TTA()`` the
network sees every view of a batch, ``CubeCache.epoch_views`` makes the views with the gathers that read the cube anyway, and one
``hpri_tta_merge`` per batch brings the logits back to the frame and merges them:

    tta  = TTA(views=("id", "flip_w", "flip_h", "rot180"), merge="prob", spread=True)
    pred = predict_split(net, cache.epoch_views(2, tta.views), tta=tta)      # pred.logits: the logit of the mean probability
    val  = validate_net(pred); write_spreadmaps(fig_dir, pred)

Objects instead of pixels (``hyperpri_amd.components``, ``csrc/components.hip``) are opt-in as well: ``clean_prediction`` drops the
specks and closes the pinholes of a stored split at the chosen threshold and hands back a prediction that ``test_net`` and
``write_segmaps`` take unchanged; ``object_metrics`` counts and measures predicted and true components:

    cleaned, stats = clean_prediction(pred, val["best_threshold"], min_area=8, max_hole=4)
    test = test_net(cleaned, val["best_threshold"]); objs = object_metrics(pred, val["best_threshold"], min_area=8)

Distances (``hyperpri_amd.distance``, ``csrc/distance.hip``), opt-in too: ``surface_metrics`` reports Hausdorff, HD95, the average
symmetric surface distance and surface Dice of a stored split from an exact integer distance transform, ``root_traits`` the length
and diameter of the predicted and the true roots:

    surf = surface_metrics(pred, val["best_threshold"], tolerances=(1.0, 2.0)); traits = root_traits(pred, val["best_threshold"])

Lightning-free and torchmetrics-free like ``trainer.py``; the device pieces this module composes are those of ``metrics.py``
(``SegCounts``, ``PRCurve``, ``best_dice_threshold``, ``average_precision``) and ``hpri_bce_logits_fwd``; the maps are one kernel of their own
(``csrc/segmap.hip``).  There is no CPU fallback: tensors must be fp32 on a ROCm device.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib
from ._args import (MAX_CLASSES, _TARGET_KIND, _as_f32, _class_logits, _class_target, _ignore_args, _image4d, _p, _require_cuda,
                    _require_placed, _stream)
from .metrics import (PRCurve, SegCounts, _confusion_pass, _split_counts, average_precision, best_dice_threshold,
                      multiclass_metrics_from_confusion)
from .tta import TTA, VIEW_CODES, apply_view, view_shape

# eval_color_segmaps, restated as data: the colour-blind palette (PLTrainer.py:255-258: prediction only, truth only, both), the
# overlay's alpha (:264), the bands shown as R (700 nm), G (546 nm), B (436 nm) of the band-sliced cube and its gamma (:238-239)
PALETTE = ((202 / 255, 0 / 255, 32 / 255), (5 / 255, 133 / 255, 176 / 255), (155 / 255, 191 / 255, 133 / 255))
ALPHA = 0.6
HSI_BANDS, HSI_GAMMA = (125, 49, 0), 2.2
RGB_BANDS, RGB_GAMMA = (0, 1, 2), 1.0


@dataclass
class SplitPrediction:
    """What ``predict_split`` keeps of a split, all of it on the device: image i owns elements ``offsets[i]:offsets[i + 1]`` of
    ``logits`` and ``masks`` (row-major ``sizes[i] = (h, w)``) and is called ``names[i]``."""
    logits: torch.Tensor            # fp32, flat
    masks: torch.Tensor             # fp32, flat
    offsets: List[int]              # len(names) + 1
    sizes: List[Tuple[int, int]]
    names: List[object]
    spread: Optional[torch.Tensor] = None   # fp32, flat, the offsets of ``logits``: the views' disagreement (``TTA(spread=True)`` only)

    def __len__(self) -> int:
        return len(self.names)

    def image(self, i: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(logits, mask) of image i as (h, w) views of the store."""
        a, b, (h, w) = self.offsets[i], self.offsets[i + 1], self.sizes[i]
        return self.logits[a:b].view(h, w), self.masks[a:b].view(h, w)


def _require_device(t: torch.Tensor, what: str) -> None:
    """``_require_cuda`` for masks, which may be integer tensors: only the placement is checked."""
    _require_placed(t, what, "evaluation exists", "Move the batches to a ROCm device.")


def _names(index, n: int) -> List[object]:
    if index is None:
        return [None] * n
    if isinstance(index, torch.Tensor):
        index = index.tolist()
    names = list(index) if isinstance(index, (list, tuple)) else [index]
    if len(names) != n:
        raise ValueError(f"evaluate: a batch of {n} images carries {len(names)} names")
    return names


class _SplitStore:
    """What the ``*_split`` loops keep per batch and hand over as a ``SplitPrediction``.  ``add_mask`` copies the batch's mask and records
    the names, offsets and sizes of its ``n`` images; the flat logits go into ``logits`` beside it -- apart, because ``predict_split``
    under TTA must store the mask before the views run.  ``add_scores`` does both for a baseline's score map."""

    def __init__(self) -> None:
        self.logits: List[torch.Tensor] = []
        self.masks: List[torch.Tensor] = []
        self.spreads: List[torch.Tensor] = []
        self.offsets, self.sizes, self.names = [0], [], []

    def add_mask(self, mask: torch.Tensor, index, n: int, h: int, w: int) -> None:
        self.masks.append(mask.to(torch.float32).reshape(-1).clone())
        self.names.extend(_names(index, n))
        for _ in range(n):
            self.offsets.append(self.offsets[-1] + h * w)
            self.sizes.append((h, w))

    def add_scores(self, pred: torch.Tensor, batch: dict, clone: bool = True) -> None:
        """One (N, h, w) score map of a baseline against ``batch['mask']``."""
        mask = batch["mask"]
        n, h, w = int(pred.shape[0]), int(pred.shape[-2]), int(pred.shape[-1])
        if mask.numel() != n * h * w:
            raise ValueError(f"evaluate: need one score and one mask value per pixel, got scores {tuple(pred.shape)} "
                             f"and a mask {tuple(mask.shape)}")
        self.logits.append(pred.reshape(-1).clone() if clone else pred.reshape(-1))
        self.add_mask(mask, batch.get("index"), n, h, w)

    def result(self, who: str) -> SplitPrediction:
        if not self.logits:
            raise ValueError(f"{who}: no batches")
        return SplitPrediction(torch.cat(self.logits), torch.cat(self.masks), self.offsets, self.sizes, self.names,
                               torch.cat(self.spreads) if self.spreads else None)


def _checked_batch(batch: dict) -> Tuple[torch.Tensor, torch.Tensor]:
    image, mask = batch["image"], batch["mask"]
    _require_cuda(image, "evaluation image")
    _require_device(mask, "evaluation mask")
    return image, mask


def tta_merge(view_logits: Sequence[torch.Tensor], views: Sequence[str], merge: str = "prob", spread: bool = False,
              frame: Optional[Tuple[int, int]] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """One ``hpri_tta_merge`` launch (csrc/tta.hip; the contract is restated by ``tta.tta_merge_reference``): ``view_logits[v]`` is
    the contiguous fp32 (N, K, hv, wv) device tensor a network gave for view ``views[v]``; returns ``(out, spread)``, ``out``
    (N, K, h, w) in the original frame and ``spread`` (N, h, w) or None.  ``frame`` = (h, w) is checked against the views' shapes
    when given.  Pointers and view codes travel as kernel arguments: nothing is uploaded, nothing synchronises."""
    import ctypes
    V = len(view_logits)
    if not 1 <= V <= len(VIEW_CODES) or len(views) != V:
        raise ValueError(f"tta_merge: need 1 to {len(VIEW_CODES)} views and one tensor per view, got {V} tensors for {len(views)} views")
    if merge not in ("prob", "logit"):
        raise ValueError(f"tta_merge: merge must be 'prob' or 'logit', got {merge!r}")
    codes = [VIEW_CODES[v] if v in VIEW_CODES else None for v in views]
    if None in codes:
        raise ValueError(f"tta_merge: unknown view in {tuple(views)!r}")
    first = view_logits[0]
    for x in view_logits:
        _require_cuda(x, "test-time augmentation logits")
        if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous() or x.device != first.device:
            raise ValueError("tta_merge: every view must be a contiguous fp32 (N, K, hv, wv) tensor on one device")
    N, K, hv, wv = (int(v) for v in first.shape)
    h, w = (wv, hv) if codes[0] >= 4 else (hv, wv)
    if frame is not None and (h, w) != tuple(frame):
        raise ValueError(f"tta_merge: view {views[0]!r} of a {frame[0]}x{frame[1]} frame cannot be {hv}x{wv}")
    for x, v in zip(view_logits, views):
        if tuple(x.shape) != (N, K, *view_shape(v, h, w)):
            raise ValueError(f"tta_merge: view {v!r} of a {h}x{w} frame must be {(N, K, *view_shape(v, h, w))}, got {tuple(x.shape)}")
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"tta_merge: the number of planes must lie in [1, {MAX_CLASSES}], got {K}")
    with torch.cuda.device(first.device):
        out = torch.empty((N, K, h, w), dtype=torch.float32, device=first.device)
        sp = torch.empty((N, h, w), dtype=torch.float32, device=first.device) if spread else None
        ptrs = (ctypes.c_void_p * V)(*[x.data_ptr() for x in view_logits])
        cds = (ctypes.c_int * V)(*codes)
        _lib.call("hpri_tta_merge", ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(cds, ctypes.c_void_p), V, N, K, h, w,
                  1 if merge == "prob" else 0, _p(out), _p(sp), _stream())
    return out, sp


def _view_logits(network: nn.Module, batch: dict, tta: TTA, planes: int, frame: Tuple[int, int], who: str) -> List[torch.Tensor]:
    """The network's fp32 logits for every view of ``tta``, each a contiguous (N, planes, hv, wv) tensor of its own.  A view's image
    is ``batch['image_of'](view)`` when the batch has that key (``CubeCache.epoch_views``: the gather that reads the cube anyway
    makes the view, and a view is finished with before the next one is asked for); otherwise ``apply_view(batch['image'],
    view).contiguous()`` -- the torch fallback, which costs an ATen copy of the cube per view."""
    h, w = frame
    outs: List[torch.Tensor] = []
    for v in tta.views:
        image = batch["image_of"](v) if "image_of" in batch else apply_view(batch["image"], v).contiguous()
        _require_cuda(image, "evaluation image")
        pred = network(image)
        if isinstance(pred, tuple):                      # analyze=True networks return (pred, features)
            pred = pred[0]
        n = int(pred.shape[0])
        hv, wv = view_shape(v, h, w)
        if pred.numel() != n * planes * hv * wv or (int(pred.shape[-2]), int(pred.shape[-1])) != (hv, wv):
            raise ValueError(f"{who}: view {v!r} of a {h}x{w} frame needs ({n}, {planes}, {hv}, {wv}) logits, got {tuple(pred.shape)}")
        x = pred.detach().to(torch.float32).reshape(n, planes, hv, wv).contiguous()
        if x.data_ptr() == pred.data_ptr():              # a copy: the network may hand out a buffer that its next forward rewrites
            x = x.clone()
        outs.append(x)
    return outs


def predict_split(network: nn.Module, batches: Iterable[dict], tta: Optional[TTA] = None) -> SplitPrediction:
    """``pl_trainer.predict(pl_model, loader)`` (PLTrainer.py:530-532, 626-629) without the host: the network runs in ``eval()``
    under ``torch.inference_mode()`` over ``batches`` -- any iterable of ``{'image', 'mask', 'index'}`` dicts with device tensors,
    ``CubeCache.epoch(batch_size, shuffle=False)`` or a DataLoader whose batches were moved to the card -- and every batch's
    logits and mask are kept on the device, where ``predict_step`` does ``.cpu()``.  ``(pred, features)`` of ``analyze=True``
    networks is unwrapped; a ragged last batch and images of different sizes are fine.  The previous train / eval mode of the
    network is restored afterwards.

    ``tta`` (``hyperpri_amd.TTA``; None: nothing below happens): test-time augmentation.  Per batch the mask is copied and the names
    are recorded first; the network then runs once per view (``_view_logits``: the views come from ``batch['image_of']`` --
    ``CubeCache.epoch_views(batch_size, tta.views)`` -- or, for batches with a plain ``'image'``, from ``apply_view``, an ATen copy
    of the cube per view); one ``hpri_tta_merge`` brings the views' logits back to the frame and merges them, and the result is
    stored as above.  With ``merge="prob"`` what is stored is the logit of the mean probability: ``logits`` stays a store of
    logits, and ``validate_net``, ``test_net`` and ``write_segmaps`` work on it unchanged.  ``tta.spread`` fills
    ``SplitPrediction.spread``."""
    if tta is not None and not isinstance(tta, TTA):
        raise TypeError(f"predict_split: tta must be a hyperpri_amd.TTA or None, got {type(tta).__name__}")
    was_training = network.training
    store = _SplitStore()
    network.eval()
    try:
        with torch.inference_mode():
            for batch in batches:
                if tta is not None:
                    mask = batch["mask"]
                    _require_device(mask, "evaluation mask")
                    if mask.dim() < 2:
                        raise ValueError(f"evaluate: need a (N, 1, h, w) or (N, h, w) mask, got {tuple(mask.shape)}")
                    h, w = int(mask.shape[-2]), int(mask.shape[-1])
                    n = mask.numel() // (h * w)
                    # first of all: the views below rotate through the output slots the mask lives in
                    store.add_mask(mask, batch.get("index"), n, h, w)
                    views = _view_logits(network, batch, tta, 1, (h, w), "predict_split")
                    if int(views[0].shape[0]) != n:
                        raise ValueError(f"evaluate: {int(views[0].shape[0])} images of logits for {n} masks")
                    merged, sp = tta_merge(views, tta.views, tta.merge, tta.spread, (h, w))
                    store.logits.append(merged.reshape(-1))
                    if sp is not None:
                        store.spreads.append(sp.reshape(-1))
                else:
                    image, mask = _checked_batch(batch)
                    pred = network(image)
                    if isinstance(pred, tuple):                  # analyze=True networks return (pred, features)
                        pred = pred[0]
                    n = int(pred.shape[0])
                    h, w = int(pred.shape[-2]), int(pred.shape[-1])
                    if pred.numel() != n * h * w or mask.numel() != n * h * w:
                        raise ValueError(f"evaluate: need one logit and one mask value per pixel, got logits {tuple(pred.shape)} "
                                         f"and a mask {tuple(mask.shape)}")
                    # copies: a cache hands out views of buffers it rewrites two batches later
                    store.logits.append(pred.detach().to(torch.float32).reshape(-1).clone())
                    store.add_mask(mask, batch.get("index"), n, h, w)
            return store.result("predict_split")
    finally:
        network.train(was_training)


def detect_split(detector: nn.Module, batches: Iterable[dict], score: str = "ace", target: int = 0) -> SplitPrediction:
    """``predict_split`` for a classical baseline (``hyperpri_amd.SpectralDetector``): the same loop without a network.  Per batch
    the detector's ``logit=True`` map of ``score`` for target ``target`` (``rx`` has one map) is stored as ``logits`` -- copied, as
    the cache rewrites its output slots -- with masks, offsets, sizes and names exactly as ``predict_split`` stores them, so
    ``validate_net``, ``test_net``, ``write_segmaps``, ``clean_prediction``, ``surface_metrics`` and the rest read it unchanged."""
    store = _SplitStore()
    with torch.inference_mode():
        for batch in batches:
            image, _ = _checked_batch(batch)
            maps = detector(image, score=score, logit=True)
            if not 0 <= int(target) < int(maps.shape[1]):
                raise ValueError(f"detect_split: target {target} of a detector with {int(maps.shape[1])} map(s)")
            store.add_scores(maps[:, int(target)], batch)
        return store.result("detect_split")


def cluster_split(model: nn.Module, batches: Iterable[dict]) -> SplitPrediction:
    """``detect_split`` for a clustering (``hyperpri_amd.SpectralKMeans`` after ``calibrate``): per batch the model's ``"logit"`` map --
    the logit of the foreground share of every pixel's cluster -- is stored as ``logits``, with masks, offsets, sizes and names
    exactly as ``predict_split`` stores them, so the evaluation functions read an unsupervised baseline unchanged."""
    store = _SplitStore()
    with torch.inference_mode():
        for batch in batches:
            image, _ = _checked_batch(batch)
            store.add_scores(model(image, output="logit")[:, 0], batch)
        return store.result("cluster_split")


def gmm_split(model: nn.Module, batches: Iterable[dict]) -> SplitPrediction:
    """``cluster_split`` for a Gaussian mixture classifier (``hyperpri_amd.SpectralGMM`` with two classes): per batch the model's
    ``"logit"`` map -- the log posterior odds of the foreground -- is stored as ``logits``, with masks, offsets, sizes and names exactly as
    ``predict_split`` stores them, so the evaluation functions read a statistical baseline unchanged."""
    store = _SplitStore()
    with torch.inference_mode():
        for batch in batches:
            image, _ = _checked_batch(batch)
            store.add_scores(model(image, output="logit")[:, 0], batch)
        return store.result("gmm_split")


def unmix_split(model: nn.Module, batches: Iterable[dict], mode: str = "fcls") -> SplitPrediction:
    """``cluster_split`` for an unmixer (``hyperpri_amd.SpectralUnmixer`` with a foreground endmember): per batch the model's ``"logit"``
    map under ``mode`` -- the logit of every pixel's foreground abundance -- is stored as ``logits``, with masks, offsets, sizes and
    names exactly as ``predict_split`` stores them, so the evaluation functions read a soft baseline unchanged."""
    store = _SplitStore()
    with torch.inference_mode():
        for batch in batches:
            image, _ = _checked_batch(batch)
            store.add_scores(model(image, mode=mode, output="logit")[:, 0], batch)
        return store.result("unmix_split")


def refine_split(pred: SplitPrediction, batches: Iterable[dict], guide, radius: int, eps: float, domain: str = "prob") -> SplitPrediction:
    """Edge-preserving refinement of a stored split (``hyperpri_amd.guided_filter``, ``csrc/guided.hip``): ``batches`` serves the split
    once more in the order it was predicted in, as for ``write_segmaps``; per batch ``guide(batch["image"])`` -- a
    ``SpectralProjection`` with at most three outputs, or any callable that returns ``(N, K, h, w)`` (or ``(N, 1, K, h, w)``) with
    K <= 3 -- guides the filter over the stored logits (``domain="prob"``: filtered as probabilities, stored as logits again).
    Returns a new ``SplitPrediction`` with the filtered logits and the same masks, offsets, sizes and names; ``spread`` is carried
    over.  ``validate_net``, ``test_net``, ``clean_prediction``, ``surface_metrics`` and ``write_segmaps`` read it unchanged."""
    from .guided import MAX_GUIDES, guided_filter
    if getattr(guide, "out_channels", 0) > MAX_GUIDES:
        raise ValueError(f"refine_split: the guide has {guide.out_channels} outputs, the filter takes at most {MAX_GUIDES}")
    logits: List[torch.Tensor] = []
    i = 0
    with torch.inference_mode():
        for batch in batches:
            image = batch["image"]
            _require_cuda(image, "evaluation image")
            n, (h, w) = int(image.shape[0]), (int(image.shape[-2]), int(image.shape[-1]))
            if i + n > len(pred):
                raise ValueError("refine_split: the batches hold more images than the stored prediction")
            if _names(batch.get("index"), n) != pred.names[i:i + n] or any(s != (h, w) for s in pred.sizes[i:i + n]):
                raise ValueError(f"refine_split: images {i}..{i + n - 1} are not the ones the prediction stored (serve the split in "
                                 "the same order, unshuffled)")
            a, b = pred.offsets[i], pred.offsets[i + n]
            logits.append(guided_filter(guide(image), pred.logits[a:b].view(n, h, w), radius, eps, domain).reshape(-1))
            i += n
    if i != len(pred):
        raise ValueError(f"refine_split: the batches held {i} of the {len(pred)} stored images")
    return SplitPrediction(torch.cat(logits), pred.masks, list(pred.offsets), list(pred.sizes), list(pred.names), pred.spread)


def crf_split(pred: SplitPrediction, batches: Iterable[dict], guide, **crf) -> SplitPrediction:
    """``refine_split`` for the dense CRF (``hyperpri_amd.dense_crf``, ``csrc/crf.hip``): ``batches`` serves the split once more in the
    order it was predicted in; per batch ``guide(batch["image"])`` -- a ``SpectralProjection`` with at most three outputs, or any
    callable that returns ``(N, K, h, w)`` (or ``(N, 1, K, h, w)``) with K <= 3, ``None`` for no guide -- is the appearance feature of a
    mean-field refinement of the stored binary logits (``**crf``: ``radius``, ``iterations``, ``theta_alpha``, ``theta_beta``,
    ``theta_gamma``, ``w_appearance``, ``w_smooth``, ``compat``).  Returns a new ``SplitPrediction`` with the refined logits
    ``L_1 - L_0`` and the same masks, offsets, sizes and names; ``spread`` is carried over."""
    from .crf import MAX_GUIDES, dense_crf
    if "output" in crf:
        raise ValueError("crf_split: it stores output='logit'; output is not its to take")
    if getattr(guide, "out_channels", 0) > MAX_GUIDES:
        raise ValueError(f"crf_split: the guide has {guide.out_channels} outputs, the CRF takes at most {MAX_GUIDES}")
    logits: List[torch.Tensor] = []
    i = 0
    with torch.inference_mode():
        for batch in batches:
            image = batch["image"]
            _require_cuda(image, "evaluation image")
            n, (h, w) = int(image.shape[0]), (int(image.shape[-2]), int(image.shape[-1]))
            if i + n > len(pred):
                raise ValueError("crf_split: the batches hold more images than the stored prediction")
            if _names(batch.get("index"), n) != pred.names[i:i + n] or any(s != (h, w) for s in pred.sizes[i:i + n]):
                raise ValueError(f"crf_split: images {i}..{i + n - 1} are not the ones the prediction stored (serve the split in "
                                 "the same order, unshuffled)")
            a, b = pred.offsets[i], pred.offsets[i + n]
            g = None if guide is None else guide(image)
            logits.append(dense_crf(pred.logits[a:b].view(n, h, w), g, output="logit", **crf).reshape(-1))
            i += n
    if i != len(pred):
        raise ValueError(f"crf_split: the batches held {i} of the {len(pred)} stored images")
    return SplitPrediction(torch.cat(logits), pred.masks, list(pred.offsets), list(pred.sizes), list(pred.names), pred.spread)


def fit_crf(pred: SplitPrediction, batches: Iterable[dict], guide, layer, steps: int, lr: float, loss=None):
    """Fit a ``hyperpri_amd.CRFLayer`` (``output="logit"``) to a stored split, in place: ``steps`` steps of the package's fused Adam at
    ``lr`` on ``loss`` (default: its ``BCEWithLogitsLoss``) between ``layer(stored logits, guide)`` and the stored masks, the mean over
    the split's pixels.  ``batches`` serves the split ONCE, as for ``crf_split``, for ``guide(batch["image"])`` alone (``None``: a layer
    without a guide); the guide maps stay in HBM and every step runs on them.  ``crf_split`` with the extra state of
    ``layer.frozen()`` (without ``output``) evaluates the result."""
    from .crf import MAX_GUIDES, CRFLayer
    from .losses import BCEWithLogitsLoss
    from .optim import FusedAdam
    if not isinstance(layer, CRFLayer):
        raise ValueError(f"fit_crf: the layer must be a CRFLayer (CRFLayer.from_crf makes one of a DenseCRF), got {type(layer).__name__}")
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
        raise ValueError(f"fit_crf: steps must be a positive integer, got {steps!r}")
    if layer.output != "logit":
        raise ValueError("fit_crf: the layer must have output='logit' (the stored masks are compared with logits)")
    if getattr(guide, "out_channels", 0) > MAX_GUIDES:
        raise ValueError(f"fit_crf: the guide has {guide.out_channels} outputs, the CRF takes at most {MAX_GUIDES}")
    parts = []
    i = 0
    with torch.no_grad():                              # (not inference_mode: the guide maps are saved for the backward)
        for batch in batches:
            image = batch["image"]
            _require_cuda(image, "evaluation image")
            n, (h, w) = int(image.shape[0]), (int(image.shape[-2]), int(image.shape[-1]))
            if i + n > len(pred):
                raise ValueError("fit_crf: the batches hold more images than the stored prediction")
            if _names(batch.get("index"), n) != pred.names[i:i + n] or any(s != (h, w) for s in pred.sizes[i:i + n]):
                raise ValueError(f"fit_crf: images {i}..{i + n - 1} are not the ones the prediction stored (serve the split in the same "
                                 "order, unshuffled)")
            parts.append((pred.offsets[i], pred.offsets[i + n], (n, h, w), None if guide is None else guide(image).clone()))
            i += n
    if i != len(pred):
        raise ValueError(f"fit_crf: the batches held {i} of the {len(pred)} stored images")
    loss = BCEWithLogitsLoss() if loss is None else loss
    opt = FusedAdam([p for p in layer.parameters() if p.requires_grad], lr=float(lr))
    total = float(pred.offsets[-1])
    # (a stored split was made under inference_mode; autograd saves only ordinary tensors)
    logits, masks = (t.clone() if t.is_inference() else t.detach() for t in (pred.logits, _as_f32(pred.masks)))
    with torch.enable_grad():
        for _ in range(int(steps)):
            opt.zero_grad(set_to_none=True)
            for a, b, shape, g in parts:
                part = loss(layer(logits[a:b].view(shape), g), masks[a:b].view(shape))
                (part * ((b - a) / total)).backward()
            opt.step()
    return layer


def ridge_split(batches: Iterable[dict], plane, sigmas, **ridge) -> SplitPrediction:
    """``detect_split`` for the classical spatial baseline (``hyperpri_amd.ridge_filter``, ``csrc/ridge.hip``): per batch
    ``plane(batch["image"])`` -- a ``SpectralProjection``, or any callable that returns ``(N, 1 or T, h, w)`` (or ``(N, 1, T, h, w)``),
    ``lambda im: proj(im)[:, :1]`` for instance -- is ridge-filtered at ``sigmas`` (``**ridge``: ``measure``, ``polarity``, ``beta``, ``c``,
    ``domain``) and ``output="logit"`` of map 0 is stored as ``logits``, with masks, offsets, sizes and names exactly as
    ``predict_split`` stores them, so the evaluation functions read it unchanged."""
    from .ridge import ridge_filter
    if "output" in ridge or "return_scale" in ridge or "return_hessian" in ridge:
        raise ValueError("ridge_split: it stores output='logit' of the response; output, return_scale and return_hessian are not its to take")
    store = _SplitStore()
    with torch.inference_mode():
        for batch in batches:
            image, _ = _checked_batch(batch)
            maps = plane(image)
            if maps.dim() == 5 and maps.shape[1] == 1:
                maps = maps[:, 0]
            if maps.dim() != 4:
                raise ValueError(f"ridge_split: the plane must be (N, T, h, w) or (N, 1, T, h, w), got {tuple(maps.shape)}")
            # (a fresh tensor of the filter's own: stored without a copy)
            store.add_scores(ridge_filter(maps[:, :1], sigmas, output="logit", **ridge)[:, 0], batch, clone=False)
        return store.result("ridge_split")


def enhance_split(pred: SplitPrediction, sigmas, **ridge) -> SplitPrediction:
    """The ridge measure of a stored split's probabilities (``hyperpri_amd.ridge_filter`` with ``domain="prob"`` and
    ``output="logit"``; ``**ridge``: ``measure``, ``polarity``, ``beta``, ``c``): lines are kept, blobs and flat background suppressed.  It
    reads no cube, so it needs no batches.  Returns a new ``SplitPrediction`` with the same masks, offsets, sizes and names; ``spread``
    is carried over, as in ``refine_split``."""
    from .ridge import ridge_filter
    if "output" in ridge or "domain" in ridge or "return_scale" in ridge or "return_hessian" in ridge:
        raise ValueError("enhance_split: it reads probabilities and stores logits; domain, output, return_scale and return_hessian are "
                         "not its to take")
    if len(pred) == 0:
        raise ValueError("enhance_split: an empty split")
    _require_cuda(pred.logits, "stored logits")
    logits: List[torch.Tensor] = []
    with torch.inference_mode():
        i = 0
        while i < len(pred):                                      # runs of images of one size go through one launch
            j = i + 1
            while j < len(pred) and pred.sizes[j] == pred.sizes[i]:
                j += 1
            h, w = pred.sizes[i]
            a, b = pred.offsets[i], pred.offsets[j]
            if b - a != (j - i) * h * w:
                raise ValueError(f"enhance_split: images {i}..{j - 1} hold {b - a} values, their sizes say {(j - i) * h * w}")
            logits.append(ridge_filter(pred.logits[a:b].view(j - i, h, w), sigmas, domain="prob", output="logit", **ridge).reshape(-1))
            i = j
    return SplitPrediction(torch.cat(logits), pred.masks, list(pred.offsets), list(pred.sizes), list(pred.names), pred.spread)


def _bce(logits: torch.Tensor, masks: torch.Tensor) -> float:
    n = logits.numel()
    nws = _lib.load().hpri_bce_workspace_doubles(n)
    ws = torch.empty(nws, dtype=torch.float64, device=logits.device)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    _lib.call("hpri_bce_logits_fwd", _p(logits), _p(masks), n, _p(loss), _p(ws), nws, _stream())
    return float(loss)


def _at_threshold(probs: torch.Tensor, masks: torch.Tensor, threshold: float) -> Dict[str, object]:
    """One ``hpri_seg_counts`` pass: Accuracy / JaccardIndex / Dice and the row-normalised BinaryConfusionMatrix
    (PLTrainer.py:559-565, 580-581) of ``probs > threshold``."""
    c = SegCounts(threshold)
    c.update(probs, masks, is_logits=False)
    m = c.compute()
    tp, fp, fn, tn = m["tp"], m["fp"], m["fn"], m["tn"]
    nan = float("nan")
    confusion = [[tn / (tn + fp), fp / (tn + fp)] if tn + fp > 0 else [nan, nan],
                 [fn / (fn + tp), tp / (fn + tp)] if fn + tp > 0 else [nan, nan]]
    return {"acc": m["acc"], "pos_iou": m["pos_iou"], "dice": m["dice"], "confusion": confusion,
            "counts": {"tp": int(tp), "fp": int(fp), "fn": int(fn), "tn": int(tn)}}


def patch_last_point(precision: torch.Tensor) -> torch.Tensor:
    """The reference's patch of the curve's last computed point (PLTrainer.py:594-600): at threshold 1 there is often no
    positive prediction at all and torchmetrics reports precision 0; ``precision[-2] < 1e-6`` becomes
    ``(1 + precision[-3]) / 2``.  Returns a patched copy (the argument itself when nothing applies)."""
    if len(precision) >= 3 and bool(precision[-2] < 1e-6):
        precision = precision.clone()
        precision[-2] = (1 + precision[-3]) / 2
    return precision


def validate_net(pred: SplitPrediction, thresholds: int = 500) -> Dict[str, object]:
    """``validate_net`` (PLTrainer.py:533-609) over a stored split, computed in the reference's order:

    * ``bce_loss``: nn.BCEWithLogitsLoss over every pixel of the split (:534-535), one ``hpri_bce_logits_fwd``;
    * ``probs = sigmoid(logits)`` once (:538); every decision below is taken on these fp32 numbers, as in the reference;
    * ``precision``, ``recall``, ``thresholds``: PrecisionRecallCurve('binary', thresholds=500) (:542-543), with ``curve_counts``
      (the integer tp / fp / fn per threshold) beside it;
    * ``best_threshold``, ``best_precision``, ``best_recall``: the best-Dice pick (:546-555); ``dice`` = 2PR/(P+R) of that curve
      point, the figure the reference prints (:571-572);
    * one ``hpri_seg_counts`` at ``best_threshold``: ``acc`` (:565), ``pos_iou`` (:574), ``dice_at_threshold`` (the positive-class
      Dice of the same counts), ``confusion`` = [[TN, FP], [FN, TP]] with each row divided by its sum (:580-581), raw ``counts``;
    * ``avg_prec``: AveragePrecision('binary') (:577);
    * the returned ``precision`` carries the last-point patch (``patch_last_point``, :598-600), applied after the threshold was
      picked -- as the reference does."""
    with torch.cuda.device(pred.logits.device):
        out: Dict[str, object] = {"bce_loss": _bce(pred.logits, pred.masks)}
        probs = torch.sigmoid(pred.logits)
        curve = PRCurve(thresholds)
        curve.update(probs, pred.masks, is_logits=False)
        tp, fp, fn, _ = curve.confusion()
        precision, recall, thr = curve.compute()
        best, p, r = best_dice_threshold(precision, recall, thr)
        out.update(recall=recall, thresholds=thr, curve_counts={"tp": tp, "fp": fp, "fn": fn},
                   best_threshold=best, best_precision=p, best_recall=r, dice=2 * p * r / (p + r) if p + r > 0 else float("nan"))
        at = _at_threshold(probs, pred.masks, best)
        out.update(acc=at["acc"], pos_iou=at["pos_iou"], dice_at_threshold=at["dice"], confusion=at["confusion"], counts=at["counts"])
        out["avg_prec"] = average_precision(probs, pred.masks)
        out["precision"] = patch_last_point(precision)
    return out


def test_net(pred: SplitPrediction, best_threshold: float) -> Dict[str, object]:
    """``test_net`` (PLTrainer.py:631-661) over a stored split at the validation threshold: ``acc``, ``dice``, ``pos_iou``,
    ``avg_prec``, ``confusion`` ([[TN, FP], [FN, TP]], rows divided by their sums) and the raw ``counts``, from one
    ``hpri_seg_counts`` over ``sigmoid(logits) > best_threshold`` and one ``average_precision``.

    ``dice`` is the positive-class Dice 2TP/(2TP+FP+FN) of ``metrics_from_counts``.  The reference builds
    ``Dice(num_classes=params.num_classes = 1, threshold, zero_division=1e-12)`` on an already binarised prediction there
    (:637-639, 649); torchmetrics is a pinned dependency of the reference that is NOT installed here, so this reading of that
    call is restated from its published behaviour, parity unpinned."""
    with torch.cuda.device(pred.logits.device):
        probs = torch.sigmoid(pred.logits)
        at = _at_threshold(probs, pred.masks, float(best_threshold))
        at["avg_prec"] = average_precision(probs, pred.masks)
    return at


test_net.__test__ = False       # (a public name of the reference, not a pytest case)


def _shown(C: int, bands: Optional[Sequence[int]], gamma: Optional[float]) -> Tuple[List[int], float]:
    """The bands shown as R, G, B and their gamma; by default those of the band-sliced HSI cube for C > 3, of an RGB image otherwise."""
    bands = (HSI_BANDS if C > 3 else RGB_BANDS) if bands is None else bands
    gamma = (HSI_GAMMA if C > 3 else RGB_GAMMA) if gamma is None else gamma
    return [int(b) for b in bands], float(gamma)


def color_segmaps(image: torch.Tensor, logits: torch.Tensor, mask: torch.Tensor, threshold: float,
                  bands: Optional[Sequence[int]] = None, gamma: Optional[float] = None, alpha: float = ALPHA,
                  palette: Optional[Sequence[Sequence[float]]] = None, return_classes: bool = False):
    """``eval_color_segmaps`` (PLTrainer.py:219-267) minus matplotlib, as one kernel (``hpri_segmap_overlay``): the device uint8
    picture (N, h, w, 3) of ``image``'s three ``bands`` (R, G, B), gamma-corrected, under the class colours of
    ``sigmoid(logits) > threshold`` against ``mask`` at ``alpha``; with ``return_classes`` also the uint8 class map (N, h, w):
    0 neither, 1 prediction only, 2 truth only, 3 both.

    ``image`` is (N, C, h, w) or a (N, 1, C, h, w) cube with any strides -- the zero-padded channels-last views of
    ``CubeCache`` / ``CubeStager`` are read in place, like a plain contiguous tensor; no band is copied anywhere.  ``bands`` /
    ``gamma`` default to (125, 49, 0) / 2.2 for C > 3 (the band-sliced HSI cube) and (0, 1, 2) / 1 otherwise.  Band values are
    clamped to [0, 1] and NaN shows as 0, where the reference would hand matplotlib the raw value."""
    _require_cuda(image, "segmentation-map image")
    _require_cuda(logits, "segmentation-map prediction")
    _require_device(mask, "segmentation-map mask")
    image = _image4d(image, "color_segmaps")
    N, C, h, w = (int(s) for s in image.shape)
    if logits.numel() != N * h * w or mask.numel() != N * h * w:
        raise ValueError(f"color_segmaps: need {N}x{h}x{w} predictions and mask values, got {tuple(logits.shape)} and "
                         f"{tuple(mask.shape)}")
    bands, gamma = _shown(C, bands, gamma)
    pal = [float(v) for colour in (PALETTE if palette is None else palette) for v in colour]
    if len(bands) != 3 or len(pal) != 9:
        raise ValueError("color_segmaps: need three band indices and a palette of three R, G, B colours")
    with torch.cuda.device(image.device):
        x = logits.detach().reshape(N, h, w).contiguous()
        y = _as_f32(mask).reshape(N, h, w).contiguous()
        rgb = torch.empty((N, h, w, 3), dtype=torch.uint8, device=image.device)
        classes = torch.empty((N, h, w), dtype=torch.uint8, device=image.device) if return_classes else None
        sn, sc, sy, sx = image.stride()
        _lib.call("hpri_segmap_overlay", _p(image), sn, sc, sy, sx, C, bands[0], bands[1], bands[2], _p(x), _p(y), N, h, w,
                  float(threshold), 1, gamma, 1.0 / gamma if gamma > 0 else 0.0, float(alpha), *pal,
                  _p(rgb), _p(classes), _stream())
    return (rgb, classes) if return_classes else rgb


def _write_picture(stem: str, rgb: np.ndarray) -> str:
    """One uint8 (h, w, 3) picture -> ``<stem>.png`` with PIL when PIL is importable, ``<stem>.npy`` otherwise; returns the path."""
    try:
        from PIL import Image
    except ImportError:
        np.save(stem + ".npy", rgb)
        return stem + ".npy"
    Image.fromarray(rgb).save(stem + ".png")
    return stem + ".png"


def write_segmaps(directory: str, split_pred: SplitPrediction, batches: Iterable[dict], threshold: float, **overlay) -> List[str]:
    """The second pass of ``validate_net(save_segmaps=True)`` / ``test_net(save_segmaps=True)`` (PLTrainer.py:602-606, 622) without
    running the network again: ``batches`` serves the split once more in the order ``predict_split`` saw it, each batch's
    images are paired with the stored logits and masks and rendered by ``color_segmaps`` (``overlay``: its ``bands``, ``gamma``,
    ``alpha``, ``palette``), and 3 bytes per pixel go to the host.  Writes ``<name>_seg.png`` with PIL when PIL is importable,
    ``<name>_seg.npy`` (uint8 (h, w, 3)) otherwise; returns the paths."""
    os.makedirs(directory, exist_ok=True)
    paths: List[str] = []
    i = 0
    for batch in batches:
        image = batch["image"]
        n, (h, w) = int(image.shape[0]), (int(image.shape[-2]), int(image.shape[-1]))
        if i + n > len(split_pred):
            raise ValueError("write_segmaps: the batches hold more images than the stored prediction")
        names = _names(batch.get("index"), n)
        if names != split_pred.names[i:i + n] or any(s != (h, w) for s in split_pred.sizes[i:i + n]):
            raise ValueError(f"write_segmaps: images {i}..{i + n - 1} are not the ones predict_split stored (serve the split in "
                             "the same order, unshuffled)")
        a, b = split_pred.offsets[i], split_pred.offsets[i + n]
        rgb = color_segmaps(image, split_pred.logits[a:b], split_pred.masks[a:b], threshold, **overlay).cpu().numpy()
        for j in range(n):
            paths.append(_write_picture(os.path.join(directory, f"{split_pred.names[i + j]}_seg"), rgb[j]))
        i += n
    if i != len(split_pred):
        raise ValueError(f"write_segmaps: the batches held {i} of the {len(split_pred)} stored images")
    return paths


def write_spreadmaps(directory: str, split_pred: SplitPrediction) -> List[str]:
    """The disagreement maps of a ``predict_split(tta=TTA(spread=True))``: per image the standard deviation over the views of the
    foreground probability as 8-bit grey, ``(uint8)(255 * min(1, 2 * std) + 0.5)`` (a standard deviation cannot exceed 1/2).
    Writes ``<name>_spread.png`` with PIL when PIL is importable, ``<name>_spread.npy`` (uint8 (h, w)) otherwise; returns the
    paths.  One byte per pixel goes to the host."""
    if split_pred.spread is None:
        raise ValueError("write_spreadmaps: the prediction holds no spread (predict_split(..., tta=TTA(spread=True)))")
    os.makedirs(directory, exist_ok=True)
    grey = (torch.clamp(split_pred.spread * 2.0, 0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).cpu().numpy()
    paths: List[str] = []
    for i, name in enumerate(split_pred.names):
        a, b, (h, w) = split_pred.offsets[i], split_pred.offsets[i + 1], split_pred.sizes[i]
        paths.append(_write_picture(os.path.join(directory, f"{name}_spread"), grey[a:b].reshape(h, w)))
    return paths


# ---------------------------------------------------------------------------------------------------
# The multi-class counterparts (csrc/multiclass.hip, hpri_segmap_classes): one pass over a split, nothing stored
# ---------------------------------------------------------------------------------------------------
# Colour-blind-safe colours (the three of PALETTE, then the rest of the Okabe-Ito set) for the first classes above the background
_CLASS_COLOURS = (*PALETTE, (230 / 255, 159 / 255, 0.0), (86 / 255, 180 / 255, 233 / 255), (0.0, 158 / 255, 115 / 255),
                  (240 / 255, 228 / 255, 66 / 255), (0.0, 114 / 255, 178 / 255), (213 / 255, 94 / 255, 0.0), (204 / 255, 121 / 255, 167 / 255))


def default_class_palette(num_classes: int) -> Tuple[Tuple[float, float, float], ...]:
    """``num_classes`` rows of R, G, B in [0, 1]: row 0 belongs to the background, which shows the bare picture, so it is never
    used (black); rows 1.. are distinct colours -- the colour-blind palette of ``color_segmaps`` first, golden-ratio hues at three
    brightness levels beyond the tenth."""
    import colorsys
    rows = [(0.0, 0.0, 0.0), *_CLASS_COLOURS[:max(0, num_classes - 1)]]
    i = 0
    while len(rows) < num_classes:
        rows.append(colorsys.hsv_to_rgb((0.11 + i * 0.6180339887) % 1.0, 0.85 if i % 2 else 0.55, (1.0, 0.8, 0.6)[(i // 2) % 3]))
        i += 1
    return tuple(rows)


def color_classmaps(image: torch.Tensor, classes: torch.Tensor, palette: Optional[Sequence[Sequence[float]]] = None,
                    alpha: float = ALPHA, bands: Optional[Sequence[int]] = None, gamma: Optional[float] = None) -> torch.Tensor:
    """The multi-class picture (``hpri_segmap_classes``): the device uint8 (N, h, w, 3) picture of ``image``'s three ``bands``,
    gamma-corrected exactly as ``color_segmaps`` shows them, with every pixel of a class above 0 blended with that class's colour
    at ``alpha``; class 0 -- and any value not below the palette's length -- shows the bare picture.

    ``classes``: a uint8 class map (N, h, w) or (N, 1, h, w), predicted (``argmax_classes``) or true; other dtypes are converted.
    ``palette``: K rows of R, G, B in [0, 1], 2 <= K <= 64, row 0 unused (default: ``default_class_palette(64)``, a colour for
    every class the kernels support).  ``image``, ``bands`` and ``gamma``: as ``color_segmaps``."""
    _require_cuda(image, "class-map image")
    _require_device(classes, "class map")
    image = _image4d(image, "color_classmaps")
    N, C, h, w = (int(s) for s in image.shape)
    if classes.numel() != N * h * w:
        raise ValueError(f"color_classmaps: need a {N}x{h}x{w} class map, got {tuple(classes.shape)}")
    bands, gamma = _shown(C, bands, gamma)
    rows = default_class_palette(MAX_CLASSES) if palette is None else [tuple(float(v) for v in colour) for colour in palette]
    if len(bands) != 3 or any(len(r) != 3 for r in rows) or not 2 <= len(rows) <= MAX_CLASSES:
        raise ValueError(f"color_classmaps: need three band indices and a palette of 2..{MAX_CLASSES} R, G, B colours")
    import ctypes
    pal = (ctypes.c_float * (3 * len(rows)))(*[v for r in rows for v in r])
    with torch.cuda.device(image.device):
        cls = (classes if classes.dtype == torch.uint8 else classes.to(torch.uint8)).reshape(N, h, w).contiguous()
        rgb = torch.empty((N, h, w, 3), dtype=torch.uint8, device=image.device)
        sn, sc, sy, sx = image.stride()
        _lib.call("hpri_segmap_classes", _p(image), sn, sc, sy, sx, C, bands[0], bands[1], bands[2], _p(cls), N, h, w, gamma,
                  1.0 / gamma if gamma > 0 else 0.0, float(alpha), ctypes.cast(pal, ctypes.c_void_p), len(rows), _p(rgb), _stream())
    return rgb


def evaluate_multiclass(network: nn.Module, batches: Iterable[dict], num_classes: int, ignore_index: Optional[int] = None,
                        class_weight: Optional[torch.Tensor] = None, segmap_dir: Optional[str] = None,
                        palette: Optional[Sequence[Sequence[float]]] = None, alpha: float = ALPHA,
                        bands: Optional[Sequence[int]] = None, gamma: Optional[float] = None,
                        tta: Optional[TTA] = None) -> Dict[str, object]:
    """A split under a multi-class network in ONE pass, with ``predict_split``'s contract (``eval()`` under
    ``torch.inference_mode()``, the previous mode restored, ``{'image', 'mask', 'index'}`` batches with device tensors, ragged
    batches and images of different sizes fine) -- but the (N, K, h, w) logits are never stored.  Per batch, on the device:

    * the confusion matrix of ``argmax(logits, 1)`` against the mask's class indices accumulates (``hpri_seg_confusion``);
    * the sum-reduced cross-entropy and its divisor -- the ``class_weight`` sum over the pixels that count -- accumulate in fp64
      (``hpri_softmax_ce_fwd``);
    * with ``segmap_dir``, the predicted class map of the same pass is rendered by ``color_classmaps`` (``palette``, default
      ``default_class_palette(num_classes)``; ``alpha``, ``bands``, ``gamma``) and written as ``<name>_seg.png`` (``.npy`` without
      PIL) -- 3 bytes per pixel go to the host.

    One host synchronisation at the end.  Returns ``ce_loss`` (what ``nn.CrossEntropyLoss(class_weight, ignore_index)`` gives over
    all pixels of the split), the entries of ``multiclass_metrics_from_confusion``, ``names`` and, with ``segmap_dir``, ``paths``.
    Raises ``ValueError`` if a mask held a value outside [0, num_classes) that was not ``ignore_index``.

    ``tta`` (``hyperpri_amd.TTA``; None: nothing below happens): the network runs once per view (``_view_logits``, as in
    ``predict_split``) and one ``hpri_tta_merge`` per batch replaces the logits by the merged ones before the confusion and the
    cross-entropy pass -- with ``merge="prob"`` the log of the mean softmax, whose softmax is that mean: argmax and cross-entropy
    need no change.  With ``tta.spread`` and ``segmap_dir`` the fraction of views that disagree with the merged class is also
    written per image, as ``<name>_spread.npy`` (fp32 (h, w)); ``spread_paths`` lists the files."""
    if tta is not None and not isinstance(tta, TTA):
        raise TypeError(f"evaluate_multiclass: tta must be a hyperpri_amd.TTA or None, got {type(tta).__name__}")
    K = int(num_classes)
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"evaluate_multiclass: the number of classes must lie in [2, {MAX_CLASSES}], got {num_classes}")
    if segmap_dir is not None:
        os.makedirs(segmap_dir, exist_ok=True)
        if palette is None:
            palette = default_class_palette(K)
    was_training = network.training
    names: List[object] = []
    paths: List[str] = []
    spread_paths: List[str] = []
    counts = totals = weight = None
    use_ignore, ignore = _ignore_args(ignore_index)
    network.eval()
    try:
        with torch.inference_mode():
            for batch in batches:
                spread = None
                if tta is not None:
                    mask = batch["mask"]
                    _require_device(mask, "evaluation mask")
                    if mask.dim() < 2:
                        raise ValueError(f"evaluate_multiclass: need a (N, 1, h, w) or (N, h, w) mask, got {tuple(mask.shape)}")
                    mask = mask.clone()                      # first of all: the views rotate through the output slots it lives in
                    views = _view_logits(network, batch, tta, K, (int(mask.shape[-2]), int(mask.shape[-1])), "evaluate_multiclass")
                    pred, spread = tta_merge(views, tta.views, tta.merge, tta.spread and segmap_dir is not None)
                    if segmap_dir is not None:               # the picture shows the identity orientation
                        image = batch["image_of"]("id") if "image_of" in batch else batch["image"]
                else:
                    image, mask = batch["image"], batch["mask"]
                    _require_cuda(image, "evaluation image")
                    _require_device(mask, "evaluation mask")
                    pred = network(image)
                    if isinstance(pred, tuple):                  # analyze=True networks return (pred, features)
                        pred = pred[0]
                if pred.dim() != 4 or int(pred.shape[1]) != K:
                    raise ValueError(f"evaluate_multiclass: need (N, {K}, h, w) logits, got {tuple(pred.shape)}")
                x = _class_logits(pred.detach().to(torch.float32), "evaluation logits")
                n, _, h, w = (int(v) for v in x.shape)
                batch_names = _names(batch.get("index"), n)
                with torch.cuda.device(x.device):
                    t = _class_target(mask, x, "evaluation mask")
                    if counts is None:
                        counts = torch.zeros(K * K + 1, dtype=torch.int64, device=x.device)
                        totals = torch.zeros(3, dtype=torch.float64, device=x.device)
                        if class_weight is not None:
                            if tuple(class_weight.shape) != (K,):
                                raise ValueError(f"evaluate_multiclass: class_weight must have shape ({K},), got {tuple(class_weight.shape)}")
                            weight = class_weight.detach().to(device=x.device, dtype=torch.float32).contiguous()
                    classes = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if segmap_dir is not None else None
                    _confusion_pass(x, t, ignore_index, counts, classes)
                    nws = _lib.load().hpri_softmax_ce_workspace_doubles(n * h * w)
                    ws = torch.empty(nws, dtype=torch.float64, device=x.device)
                    lse = torch.empty((n, h * w), dtype=torch.float32, device=x.device)
                    scalars = torch.empty(2, dtype=torch.float32, device=x.device)
                    _lib.call("hpri_softmax_ce_fwd", _p(x), _p(t), _TARGET_KIND[t.dtype], _p(weight), n, K, h * w, use_ignore, ignore,
                              0, _p(scalars[0]), _p(lse), _p(scalars[1]), _p(totals), _p(ws), nws, _stream())
                if segmap_dir is not None:
                    rgb = color_classmaps(image, classes, palette=palette, alpha=alpha, bands=bands, gamma=gamma).cpu().numpy()
                    for j in range(n):
                        paths.append(_write_picture(os.path.join(segmap_dir, f"{batch_names[j]}_seg"), rgb[j]))
                    if spread is not None:
                        maps = spread.cpu().numpy()
                        for j in range(n):
                            spread_paths.append(os.path.join(segmap_dir, f"{batch_names[j]}_spread.npy"))
                            np.save(spread_paths[-1], maps[j])
                names.extend(batch_names)
            if counts is None:
                raise ValueError("evaluate_multiclass: no batches")
            matrix = _split_counts(counts.tolist(), K)      # the host synchronisation
            loss_sum, weight_sum, _ = totals.tolist()
    finally:
        network.train(was_training)
    out: Dict[str, object] = {"ce_loss": loss_sum / weight_sum if weight_sum > 0 else float("nan")}
    out.update(multiclass_metrics_from_confusion(matrix))
    out["names"] = names
    if segmap_dir is not None:
        out["paths"] = paths
        if tta is not None and tta.spread:
            out["spread_paths"] = spread_paths
    return out


# ---------------------------------------------------------------------------------------------------
# Objects (csrc/components.hip, hyperpri_amd/components.py): clean a stored prediction, count and measure what it found
# ---------------------------------------------------------------------------------------------------
CLEAN_LOGIT = 16.0      # fp32 sigmoid(+-16) = 1 - 1.2e-7 and 1.1e-7: strictly inside (0, 1) and on either side of any threshold in [1e-6, 1 - 1e-6]


def _size_groups(pred: SplitPrediction) -> List[Tuple[int, int]]:
    """Runs [i, j) of consecutive images of one size, none holding 2^31 pixels or more."""
    groups, i = [], 0
    while i < len(pred):
        h, w = pred.sizes[i]
        limit = max(1, (2 ** 31 - 1) // (h * w))
        j = i + 1
        while j < len(pred) and pred.sizes[j] == (h, w) and j - i < limit:
            j += 1
        groups.append((i, j))
        i = j
    return groups


def clean_prediction(pred: SplitPrediction, threshold: float, min_area: int = 0, max_hole: int = 0,
                     connectivity: int = 8) -> Tuple[SplitPrediction, Dict[str, int]]:
    """Drop the specks and close the pinholes of a stored split on the device (``components.clean_mask``'s kernels): the decision
    ``sigmoid(logits) > threshold`` of every image loses its foreground components (``connectivity``) of fewer than ``min_area``
    pixels and gains its background components (the dual connectivity) of at most ``max_hole`` pixels that touch no image edge.
    Consecutive images of equal size are cleaned in one launch sequence.  Returns ``(cleaned, stats)``:

    * ``cleaned``: a ``SplitPrediction`` with the same masks, offsets, sizes, names (and spread) whose ``logits`` are
      ``+CLEAN_LOGIT`` where the cleaned decision is foreground and ``-CLEAN_LOGIT`` elsewhere.  fp32 sigmoid(+-16) lies strictly
      inside (0, 1), so ``test_net(cleaned, thr)``, ``write_segmaps(dir, cleaned, batches, thr)`` and ``SegCounts`` reproduce the
      cleaned decision for ANY threshold in [1e-6, 1 - 1e-6], unchanged.  With ``min_area=0, max_hole=0`` the decisions are those
      of ``pred`` at ``threshold``.
    * ``stats``: ``components_removed``, ``pixels_removed``, ``holes_filled``, ``pixels_filled`` over the split (reading them is
      the one host synchronisation).

    A cleaned prediction holds two logit values, so its ``avg_prec`` and its PR curve (``validate_net``) are degenerate: ranking
    metrics and the threshold search belong to the raw prediction; clean at the threshold they picked."""
    from . import components as C
    _require_cuda(pred.logits, "prediction to clean")
    min_area, max_hole, connectivity = C._check_clean_args(min_area, max_hole, connectivity)
    with torch.cuda.device(pred.logits.device):
        src = pred.logits.detach().contiguous()
        out = torch.empty_like(src)
        stats = torch.zeros(4, dtype=torch.int64, device=src.device)
        for i, j in _size_groups(pred):
            a, b, (h, w) = pred.offsets[i], pred.offsets[j], pred.sizes[i]
            C._clean_launch(src[a:b].view(j - i, h, w), 0, float(threshold), True, min_area, max_hole, connectivity, stats,
                            logits_out=out[a:b], logit=CLEAN_LOGIT)
        cleaned = SplitPrediction(out, pred.masks, list(pred.offsets), list(pred.sizes), list(pred.names), pred.spread)
        return cleaned, C.stats_dict(stats)


def _to_measure(pred: SplitPrediction, threshold: float, min_area: int, connectivity: int = 8) -> Tuple[SplitPrediction, float, torch.Tensor]:
    """What the object, surface, trait and centerline metrics read: the split and the threshold to decide it at -- after
    ``clean_prediction(pred, threshold, min_area)`` when ``min_area > 0``, whose logits any threshold decides alike -- and the
    masks as fp32."""
    _require_cuda(pred.logits, "prediction to measure")
    _require_device(pred.masks, "evaluation mask")
    if int(min_area) > 0:
        pred, threshold = clean_prediction(pred, threshold, min_area, 0, connectivity)[0], 0.5
    return pred, threshold, _as_f32(pred.masks)


def object_metrics(pred: SplitPrediction, threshold: float, connectivity: int = 8, min_area: int = 0) -> Dict[str, object]:
    """Count and measure the objects of a stored split: the components of ``sigmoid(logits) > threshold`` (after
    ``clean_prediction(pred, threshold, min_area)`` when ``min_area > 0``) and those of the masks (``int(mask) != 0``), labelled the
    same way.  Returns

    * ``pred_objects``, ``pred_objects_hit`` (predicted components with at least one true pixel);
    * ``truth_objects``, ``truth_objects_hit`` (true components with at least one predicted pixel);
    * ``object_precision`` = hit / predicted, ``object_recall`` = hit / true, ``object_f1`` = 2PR / (P + R) (NaN on a zero
      denominator, as the pixel metrics);
    * ``pred_areas``, ``truth_areas``: per image the areas of its components in label order.

    Labelling and measuring run on the device; one small table per group of equal-sized images comes to the host."""
    from . import components as C
    pred, threshold, masks = _to_measure(pred, threshold, min_area, connectivity)      # (refuses a bad connectivity when it cleans)
    connectivity = C._check_connectivity(connectivity)
    tot = {"pred_objects": 0, "pred_objects_hit": 0, "truth_objects": 0, "truth_objects_hit": 0}
    pred_areas: List[List[int]] = []
    truth_areas: List[List[int]] = []
    for i, j in _size_groups(pred):
        a, b, (h, w) = pred.offsets[i], pred.offsets[j], pred.sizes[i]
        x, m = pred.logits[a:b].view(j - i, h, w), masks[a:b].view(j - i, h, w)
        lp, cp = C.label_components(x, float(threshold), True, connectivity)
        lt, ct = C._label_truth(m, connectivity)
        tp, tt = C.component_table(lp, cp, truth=m), C.component_table(lt, ct, truth=lp)
        tot["pred_objects"] += len(tp["area"])
        tot["pred_objects_hit"] += int((tp["overlap"] > 0).sum())
        tot["truth_objects"] += len(tt["area"])
        tot["truth_objects_hit"] += int((tt["overlap"] > 0).sum())
        for n in range(j - i):
            pred_areas.append([int(v) for v in tp["area"][tp["image"] == n]])
            truth_areas.append([int(v) for v in tt["area"][tt["image"] == n]])
    nan = float("nan")
    p = tot["pred_objects_hit"] / tot["pred_objects"] if tot["pred_objects"] else nan
    r = tot["truth_objects_hit"] / tot["truth_objects"] if tot["truth_objects"] else nan
    out: Dict[str, object] = dict(tot)
    out.update(object_precision=p, object_recall=r, object_f1=2 * p * r / (p + r) if p + r > 0 else nan,
               pred_areas=pred_areas, truth_areas=truth_areas)
    return out


# ---------------------------------------------------------------------------------------------------
# Distances (csrc/distance.hip, hyperpri_amd/distance.py): how far the predicted boundary lies from the true one, and the traits
# ---------------------------------------------------------------------------------------------------
def _mean_defined(values: Sequence[float]) -> float:
    """The mean over the images that have a value (NaN = undefined, as the pixel metrics treat zero denominators)."""
    v = np.asarray(values, dtype=np.float64)
    ok = ~np.isnan(v)
    return float(v[ok].mean()) if ok.any() else float("nan")


def surface_metrics(pred: SplitPrediction, threshold: float, tolerances: Sequence[float] = (1.0, 2.0),
                    min_area: int = 0) -> Dict[str, object]:
    """Boundary distances over a stored split (``distance.surface_distances`` + ``surface_metrics_from_hist`` per group of
    equal-sized images): the boundary of ``sigmoid(logits) > threshold`` (after ``clean_prediction(pred, threshold, min_area)`` when
    ``min_area > 0``) against the boundary of the masks (``int(mask) != 0``).  Returns

    * ``hd``, ``hd95``, ``assd`` and ``surface_dice`` (a dict over ``tolerances``): the means over the images that have a value;
    * ``per_image``: the same keys as lists in the split's order, NaN where either map of an image has no boundary;
    * ``images_undefined``: the number of such images; ``names``.

    The distance transforms and histograms run on the device; one histogram per image and direction comes to the host."""
    from . import distance as D
    pred, threshold, masks = _to_measure(pred, threshold, min_area)
    tol = [float(t) for t in tolerances]
    per = {"hd": [], "hd95": [], "assd": [], "surface_dice": {t: [] for t in tol}}
    undefined = 0
    for i, j in _size_groups(pred):
        a, b, (h, w) = pred.offsets[i], pred.offsets[j], pred.sizes[i]
        sd = D.surface_distances(pred.logits[a:b].view(j - i, h, w), float(threshold), masks[a:b].view(j - i, h, w))
        m = D.surface_metrics_from_hist(sd["hist"], tol)
        undefined += m["images_undefined"]
        for key in ("hd", "hd95", "assd"):
            per[key].extend(float(v) for v in m[key])
        for t in tol:
            per["surface_dice"][t].extend(float(v) for v in m["surface_dice"][t])
    out: Dict[str, object] = {key: _mean_defined(per[key]) for key in ("hd", "hd95", "assd")}
    out["surface_dice"] = {t: _mean_defined(per["surface_dice"][t]) for t in tol}
    out.update(per_image=per, images_undefined=undefined, names=list(pred.names))
    return out


def root_traits(pred: SplitPrediction, threshold: float, min_area: int = 0) -> Dict[str, object]:
    """Root length and diameter over a stored split (``distance.root_traits`` per group of equal-sized images), for the prediction
    ``sigmoid(logits) > threshold`` (after ``clean_prediction(pred, threshold, min_area)`` when ``min_area > 0``) and for the masks
    (``int(mask) != 0``): per image, in the split's order, ``area``, ``skeleton_pixels``, ``links_straight``, ``links_diagonal``,
    ``length_px``, ``diameter_mean_px``, ``diameter_median_px`` and ``diameter_hist``; the same keys of the masks under ``"truth"``;
    ``names``."""
    from . import distance as D
    pred, threshold, masks = _to_measure(pred, threshold, min_area)
    out: Dict[str, object] = {name: [] for name in D.TRAIT_NAMES}
    out["truth"] = {name: [] for name in D.TRAIT_NAMES}
    for i, j in _size_groups(pred):
        a, b, (h, w) = pred.offsets[i], pred.offsets[j], pred.sizes[i]
        t = D.root_traits(pred.logits[a:b].view(j - i, h, w), float(threshold), truth=masks[a:b].view(j - i, h, w))
        for name in D.TRAIT_NAMES:
            out[name].extend(t[name])
            out["truth"][name].extend(t["truth"][name])
    out["names"] = list(pred.names)
    return out


def centerline_metrics(pred: SplitPrediction, threshold: float, min_area: int = 0) -> Dict[str, object]:
    """The hard clDice over a stored split (``distance.centerline_counts`` per group of equal-sized images): with ``P`` the decision
    ``sigmoid(logits) > threshold`` (after ``clean_prediction(pred, threshold, min_area)`` when ``min_area > 0``), ``T`` the masks
    (``int(mask) != 0``) and ``skel`` the Zhang-Suen ``skeletonize``

    * ``tprec`` = ``|skel(P) & T| / |skel(P)|``, ``tsens`` = ``|skel(T) & P| / |skel(T)|`` and ``cldice`` = their harmonic mean,
      pooled over the split (from the summed counts; NaN on a zero denominator, as the pixel metrics);
    * ``per_image``: the same three as lists in the split's order, and ``counts``, the four integers of every image (``|skel(P)|``,
      ``|skel(P) & T|``, ``|skel(T)|``, ``|skel(T) & P|``); ``names``.

    Decisions, thinning and counting run on the device; four integers per image come to the host."""
    from . import distance as D
    pred, threshold, masks = _to_measure(pred, threshold, min_area)
    rows = []
    for i, j in _size_groups(pred):
        a, b, (h, w) = pred.offsets[i], pred.offsets[j], pred.sizes[i]
        rows.append(D.centerline_counts(pred.logits[a:b].view(j - i, h, w), float(threshold), masks[a:b].view(j - i, h, w)))
    m = D.centerline_from_counts(np.concatenate(rows) if rows else np.zeros((0, 4), dtype=np.int64))
    out: Dict[str, object] = dict(m["pooled"])
    out["per_image"] = {"tprec": [float(v) for v in m["tprec"]], "tsens": [float(v) for v in m["tsens"]],
                        "cldice": [float(v) for v in m["cldice"]], "counts": [[int(v) for v in r] for r in m["counts"]]}
    out["names"] = list(pred.names)
    return out
