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

Lightning-free and torchmetrics-free like ``trainer.py``, whose device pieces this module composes (``hpri_bce_logits_fwd``,
``SegCounts``, ``PRCurve``, ``best_dice_threshold``, ``average_precision``); the maps are one kernel of their own
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
from .engine import _p, _require_cuda, _stream
from .trainer import PRCurve, SegCounts, average_precision, best_dice_threshold

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

    def __len__(self) -> int:
        return len(self.names)

    def image(self, i: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(logits, mask) of image i as (h, w) views of the store."""
        a, b, (h, w) = self.offsets[i], self.offsets[i + 1], self.sizes[i]
        return self.logits[a:b].view(h, w), self.masks[a:b].view(h, w)


def _require_device(t: torch.Tensor, what: str) -> None:
    """``_require_cuda`` for masks, which may be integer tensors: only the placement is checked."""
    if not t.is_cuda:
        raise RuntimeError(f"hyperpri_amd: {what} is on {t.device}; evaluation exists only as HIP kernels for MI355X "
                           "(no CPU fallback). Move the batches to a ROCm device.")


def _names(index, n: int) -> List[object]:
    if index is None:
        return [None] * n
    if isinstance(index, torch.Tensor):
        index = index.tolist()
    names = list(index) if isinstance(index, (list, tuple)) else [index]
    if len(names) != n:
        raise ValueError(f"evaluate: a batch of {n} images carries {len(names)} names")
    return names


def predict_split(network: nn.Module, batches: Iterable[dict]) -> SplitPrediction:
    """``pl_trainer.predict(pl_model, loader)`` (PLTrainer.py:530-532, 626-629) without the host: the network runs in ``eval()``
    under ``torch.inference_mode()`` over ``batches`` -- any iterable of ``{'image', 'mask', 'index'}`` dicts with device tensors,
    ``CubeCache.epoch(batch_size, shuffle=False)`` or a DataLoader whose batches were moved to the card -- and every batch's
    logits and mask are kept on the device, where ``predict_step`` does ``.cpu()``.  ``(pred, features)`` of ``analyze=True``
    networks is unwrapped; a ragged last batch and images of different sizes are fine.  The previous train / eval mode of the
    network is restored afterwards."""
    was_training = network.training
    logits: List[torch.Tensor] = []
    masks: List[torch.Tensor] = []
    offsets, sizes, names = [0], [], []
    network.eval()
    try:
        with torch.inference_mode():
            for batch in batches:
                image, mask = batch["image"], batch["mask"]
                _require_cuda(image, "evaluation image")
                _require_device(mask, "evaluation mask")
                pred = network(image)
                if isinstance(pred, tuple):                  # analyze=True networks return (pred, features)
                    pred = pred[0]
                n = int(pred.shape[0])
                h, w = int(pred.shape[-2]), int(pred.shape[-1])
                if pred.numel() != n * h * w or mask.numel() != n * h * w:
                    raise ValueError(f"evaluate: need one logit and one mask value per pixel, got logits {tuple(pred.shape)} "
                                     f"and a mask {tuple(mask.shape)}")
                # copies: a cache hands out views of buffers it rewrites two batches later
                logits.append(pred.detach().to(torch.float32).reshape(-1).clone())
                masks.append(mask.to(torch.float32).reshape(-1).clone())
                names.extend(_names(batch.get("index"), n))
                for _ in range(n):
                    offsets.append(offsets[-1] + h * w)
                    sizes.append((h, w))
            if not logits:
                raise ValueError("predict_split: no batches")
            return SplitPrediction(torch.cat(logits), torch.cat(masks), offsets, sizes, names)
    finally:
        network.train(was_training)


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
    if image.dim() == 5:                # CubeNET cube (N,1,C,h,w) -> (N,C,h,w), as autograd._as4d
        if image.shape[1] != 1:
            raise RuntimeError("hyperpri_amd: 5-D input must be (N,1,D,H,W)")
        image = image.reshape(image.shape[0], image.shape[2], image.shape[3], image.shape[4])
    if image.dim() != 4:
        raise ValueError(f"color_segmaps: need a (N,C,h,w) image or a (N,1,C,h,w) cube, got {tuple(image.shape)}")
    N, C, h, w = (int(s) for s in image.shape)
    if logits.numel() != N * h * w or mask.numel() != N * h * w:
        raise ValueError(f"color_segmaps: need {N}x{h}x{w} predictions and mask values, got {tuple(logits.shape)} and "
                         f"{tuple(mask.shape)}")
    if bands is None:
        bands = HSI_BANDS if C > 3 else RGB_BANDS
    if gamma is None:
        gamma = HSI_GAMMA if C > 3 else RGB_GAMMA
    bands = [int(b) for b in bands]
    pal = [float(v) for colour in (PALETTE if palette is None else palette) for v in colour]
    if len(bands) != 3 or len(pal) != 9:
        raise ValueError("color_segmaps: need three band indices and a palette of three R, G, B colours")
    gamma = float(gamma)
    with torch.cuda.device(image.device):
        x = logits.detach().reshape(N, h, w).contiguous()
        y = (mask if mask.dtype == torch.float32 else mask.to(torch.float32)).reshape(N, h, w).contiguous()
        rgb = torch.empty((N, h, w, 3), dtype=torch.uint8, device=image.device)
        classes = torch.empty((N, h, w), dtype=torch.uint8, device=image.device) if return_classes else None
        sn, sc, sy, sx = image.stride()
        _lib.call("hpri_segmap_overlay", _p(image), sn, sc, sy, sx, C, bands[0], bands[1], bands[2], _p(x), _p(y), N, h, w,
                  float(threshold), 1, gamma, 1.0 / gamma if gamma > 0 else 0.0, float(alpha), *pal,
                  _p(rgb), _p(classes), _stream())
    return (rgb, classes) if return_classes else rgb


def write_segmaps(directory: str, split_pred: SplitPrediction, batches: Iterable[dict], threshold: float, **overlay) -> List[str]:
    """The second pass of ``validate_net(save_segmaps=True)`` / ``test_net(save_segmaps=True)`` (PLTrainer.py:602-606, 622) without
    running the network again: ``batches`` serves the split once more in the order ``predict_split`` saw it, each batch's
    images are paired with the stored logits and masks and rendered by ``color_segmaps`` (``overlay``: its ``bands``, ``gamma``,
    ``alpha``, ``palette``), and 3 bytes per pixel go to the host.  Writes ``<name>_seg.png`` with PIL when PIL is importable,
    ``<name>_seg.npy`` (uint8 (h, w, 3)) otherwise; returns the paths."""
    try:
        from PIL import Image
    except ImportError:
        Image = None
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
            stem = os.path.join(directory, f"{split_pred.names[i + j]}_seg")
            if Image is not None:
                Image.fromarray(rgb[j]).save(stem + ".png")
                paths.append(stem + ".png")
            else:
                np.save(stem + ".npy", rgb[j])
                paths.append(stem + ".npy")
        i += n
    if i != len(split_pred):
        raise ValueError(f"write_segmaps: the batches held {i} of the {len(split_pred)} stored images")
    return paths
