"""Segmentation metrics accumulated on the device: binary counts, the multi-class confusion matrix, the PR curve.

Names and semantics follow the torchmetrics objects of ``RootLightningModel`` (PLTrainer.py:62-68, 88-91) and of its evaluation
helpers (:542-559), without torchmetrics: every per-pixel pass is one launch of the HIP library (``csrc/step.hip``,
``csrc/multiclass.hip``) and nothing synchronises with the host until a value is read.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._args import (MAX_CLASSES, _TARGET_KIND, _as_f32, _class_logits, _class_target, _flat, _ignore_args, _p, _require_cuda,
                    _require_placed, _stream)


# ---------------------------------------------------------------------------------------------------
# Accuracy / JaccardIndex / Dice from one confusion count (PLTrainer.py:62-68, 88-91)
# ---------------------------------------------------------------------------------------------------
def _counts_inputs(pred: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """A prediction and its mask -> the contiguous fp32 pair of equal size that ``_counts_pass`` reads."""
    x = _flat(pred.detach(), "prediction")
    y = _flat(_as_f32(mask), "mask")
    if x.numel() != y.numel():
        raise ValueError("prediction and mask differ in size")
    return x, y


def _counts_pass(x: torch.Tensor, y: torch.Tensor, threshold: float, is_logits: bool, counts: torch.Tensor) -> None:
    """One ``hpri_seg_counts`` launch on prepared tensors (``_counts_inputs``): TP, FP, FN, TN are added to ``counts`` (4 int64)."""
    _lib.call("hpri_seg_counts", _p(x), _p(y), x.numel(), threshold, int(is_logits), _p(counts), _stream())


class SegCounts:
    """TP/FP/FN/TN of ``sigmoid(pred) > threshold`` against ``mask.to(int32)``, accumulated on the device.

    ``compute()`` returns what the reference logs: pixel accuracy (``Accuracy(task='binary')``), positive-class
    Dice (``Dice(num_classes=2, ignore_index=0, zero_division=1e-12)``) and +IoU (``JaccardIndex('binary')``).
    """

    def __init__(self, threshold: float = 0.5, device=None):
        self.threshold = float(threshold)
        self.counts = None if device is None else torch.zeros(4, dtype=torch.int64, device=device)

    def reset(self) -> None:
        if self.counts is not None:
            self.counts.zero_()

    def update(self, pred: torch.Tensor, mask: torch.Tensor, is_logits: bool = True) -> None:
        _require_cuda(pred, "prediction")
        with torch.cuda.device(pred.device):
            x, y = _counts_inputs(pred, mask)
            if self.counts is None:
                self.counts = torch.zeros(4, dtype=torch.int64, device=x.device)
            _counts_pass(x, y, self.threshold, is_logits, self.counts)

    def compute(self) -> Dict[str, float]:
        tp, fp, fn, tn = (float(v) for v in self.counts.tolist())     # the one host synchronisation
        return metrics_from_counts(tp, fp, fn, tn)


def metrics_from_counts(tp: float, fp: float, fn: float, tn: float) -> Dict[str, float]:
    total = tp + fp + fn + tn
    return {
        "acc": (tp + tn) / total if total > 0 else 0.0,
        "dice": (2 * tp) / (2 * tp + fp + fn) if (2 * tp + fp + fn) > 0 else 1e-12,
        "pos_iou": tp / (tp + fp + fn) if (tp + fp + fn) > 0 else 0.0,
        "tp": tp, "fp": fp, "fn": fn, "tn": tn,
    }


# ---------------------------------------------------------------------------------------------------
# The multi-class tail (csrc/multiclass.hip): argmax + confusion matrix, the metrics it reduces to
# ---------------------------------------------------------------------------------------------------
def _confusion_pass(logits: torch.Tensor, target: Optional[torch.Tensor], ignore_index: Optional[int],
                    counts: Optional[torch.Tensor], classes: Optional[torch.Tensor]) -> None:
    """One ``hpri_seg_confusion`` launch on prepared tensors (``_class_logits`` / ``_class_target``)."""
    N, K, h, w = (int(v) for v in logits.shape)
    use_ignore, ignore = _ignore_args(ignore_index)
    _lib.call("hpri_seg_confusion", _p(logits), _p(target), 0 if target is None else _TARGET_KIND[target.dtype], N, K, h * w,
              use_ignore, ignore, _p(counts), _p(classes), _stream())


def argmax_classes(logits: torch.Tensor) -> torch.Tensor:
    """``torch.argmax(logits, 1)`` of (N, K, h, w) fp32 logits as a uint8 class map (N, h, w): the lowest index among equal maxima,
    a NaN counts as the maximum."""
    x = _class_logits(logits.detach(), "argmax_classes input")
    with torch.cuda.device(x.device):
        classes = torch.empty((x.shape[0], x.shape[2], x.shape[3]), dtype=torch.uint8, device=x.device)
        _confusion_pass(x, None, None, None, classes)
    return classes


def multiclass_metrics_from_confusion(matrix) -> Dict[str, object]:
    """Metrics of a K x K confusion matrix C[truth][prediction] (anything ``numpy.asarray`` takes), on the host:

    * ``acc`` = trace / total;
    * per class, from its row sum (truth), column sum (prediction) and diagonal entry: ``iou_per_class`` = C_cc / (row + col - C_cc),
      ``dice_per_class`` = 2 C_cc / (row + col); a class with a zero denominator -- absent from truth and prediction -- is ``nan``;
    * ``mean_iou`` / ``mean_dice``: the mean over the classes that are not ``nan`` (``nan`` when none is left);
    * ``confusion``: the matrix itself (int64 numpy array).

    These definitions are this project's own."""
    import numpy as np
    c = np.asarray(matrix.cpu() if isinstance(matrix, torch.Tensor) else matrix).astype(np.int64)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f"multiclass_metrics_from_confusion: need a square matrix, got shape {c.shape}")
    nan = float("nan")
    diag = [int(v) for v in np.diag(c)]
    both = [int(r) + int(k) for r, k in zip(c.sum(axis=1), c.sum(axis=0))]
    total = int(c.sum())
    iou = [d / (b - d) if b - d > 0 else nan for d, b in zip(diag, both)]
    dice = [2 * d / b if b > 0 else nan for d, b in zip(diag, both)]

    def mean(vals):
        kept = [v for v in vals if v == v]
        return sum(kept) / len(kept) if kept else nan
    return {"acc": sum(diag) / total if total > 0 else nan, "iou_per_class": iou, "dice_per_class": dice,
            "mean_iou": mean(iou), "mean_dice": mean(dice), "confusion": c}


def _split_counts(row: List[int], K: int):
    """A K*K + 1 count row -> the K x K matrix; raises if the row's invalid-target counter is set."""
    if row[K * K]:
        raise ValueError(f"{row[K * K]} target values were neither inside [0, {K}) nor the ignore_index")
    return [row[i * K:(i + 1) * K] for i in range(K)]


class SegConfusion:
    """The K x K confusion matrix of ``argmax(logits, 1)`` against a class-index target, accumulated on the device
    (int64, ``counts[t*K + p]``; one more entry counts invalid targets).  ``compute()`` is the one host synchronisation: it raises
    ``ValueError`` if any target was neither inside [0, K) nor ``ignore_index``, and returns ``multiclass_metrics_from_confusion``."""

    def __init__(self, num_classes: int, ignore_index: Optional[int] = None, device=None):
        self.num_classes = int(num_classes)
        if not 2 <= self.num_classes <= MAX_CLASSES:
            raise ValueError(f"SegConfusion: the number of classes must lie in [2, {MAX_CLASSES}], got {num_classes}")
        self.ignore_index = ignore_index
        self.counts = None if device is None else torch.zeros(self.num_classes ** 2 + 1, dtype=torch.int64, device=device)

    def reset(self) -> None:
        if self.counts is not None:
            self.counts.zero_()

    def update(self, logits: torch.Tensor, target: torch.Tensor, classes: Optional[torch.Tensor] = None) -> None:
        """``classes``: optional uint8 (N, h, w) tensor that receives the predicted class map in the same pass."""
        x = _class_logits(logits.detach(), "SegConfusion prediction")
        if int(x.shape[1]) != self.num_classes:
            raise ValueError(f"SegConfusion: built for {self.num_classes} classes, got logits {tuple(x.shape)}")
        with torch.cuda.device(x.device):
            t = _class_target(target, x, "SegConfusion target")
            if self.counts is None:
                self.counts = torch.zeros(self.num_classes ** 2 + 1, dtype=torch.int64, device=x.device)
            _confusion_pass(x, t, self.ignore_index, self.counts, classes)

    def matrix(self) -> List[List[int]]:
        if self.counts is None:
            raise ValueError("SegConfusion: no update yet")
        return _split_counts(self.counts.tolist(), self.num_classes)      # the one host synchronisation

    def compute(self) -> Dict[str, object]:
        return multiclass_metrics_from_confusion(self.matrix())


class _StepRows:
    """One int64 count row per step of ``SegmentationModel``, kept on the device ([capacity, width], zero-filled; no host sync until
    ``rows()``), and the step's weight -- its batch size -- on the host.  A full buffer doubles; the rows so far are copied."""

    def __init__(self, width: int, device, capacity: int = 256, as_float: bool = False):
        self.buf = torch.zeros((capacity, width), dtype=torch.int64, device=device)
        self.weights: List[int] = []
        self.n = 0
        self.as_float = as_float

    def reset(self) -> None:
        self.buf.zero_()
        self.weights.clear()
        self.n = 0

    def add(self, weight: int, fill: Callable[[torch.Tensor], None]) -> None:
        """``fill(row)`` writes the next row; the row counts once ``fill`` has returned."""
        if self.n == self.buf.shape[0]:
            grown = torch.zeros((2 * self.n, self.buf.shape[1]), dtype=torch.int64, device=self.buf.device)
            grown[:self.n].copy_(self.buf)
            self.buf = grown
        fill(self.buf[self.n])
        self.weights.append(int(weight))
        self.n += 1

    def rows(self) -> Tuple[List[list], List[int]]:
        rows = self.buf[:self.n].tolist()
        return ([[float(v) for v in r] for r in rows] if self.as_float else rows), list(self.weights)


class _StepCounts(_StepRows):
    """One (TP, FP, FN, TN) row per step; ``rows()`` gives floats, what ``metrics_from_counts`` takes."""

    def __init__(self, threshold: float, device, capacity: int = 256):
        super().__init__(4, device, capacity, as_float=True)
        self.threshold = float(threshold)

    def update(self, pred: torch.Tensor, mask: torch.Tensor) -> None:
        _require_cuda(pred, "prediction")
        with torch.cuda.device(pred.device):
            x, y = _counts_inputs(pred, mask)
            self.add(pred.shape[0], lambda row: _counts_pass(x, y, self.threshold, True, row))


class _StepConfusion(_StepRows):
    """One K*K + 1 count row per step; ``rows()`` gives ints, what ``_split_counts`` takes."""

    def __init__(self, num_classes: int, ignore_index: Optional[int], device, capacity: int = 256):
        self.K, self.ignore_index = int(num_classes), ignore_index
        super().__init__(self.K ** 2 + 1, device, capacity)

    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        x = _class_logits(pred.detach(), "prediction")
        if int(x.shape[1]) != self.K:
            raise ValueError(f"SegmentationModel: built for {self.K} classes, got logits {tuple(x.shape)}")
        with torch.cuda.device(x.device):
            t = _class_target(target, x, "mask")
            self.add(pred.shape[0], lambda row: _confusion_pass(x, t, self.ignore_index, row, None))


# ---------------------------------------------------------------------------------------------------
# PrecisionRecallCurve('binary', thresholds=500) and the best-Dice threshold (PLTrainer.py:542-556)
# ---------------------------------------------------------------------------------------------------
class PRCurve:
    """Binned binary precision-recall curve (torchmetrics 1.2.0 semantics: ``pred >= threshold``, thresholds =
    ``torch.linspace(0, 1, T)``).  The per-pixel work is one histogram pass; the T confusion matrices are suffix
    sums of the two class histograms."""

    def __init__(self, thresholds: int = 500, device=None):
        self.T = int(thresholds)
        self.device = device
        self.thresholds = None
        self.hist = None

    def _ensure(self, device):
        if self.hist is None:
            self.thresholds = torch.linspace(0, 1, self.T, dtype=torch.float32).to(device)
            self.hist = torch.zeros(2 * (self.T + 1), dtype=torch.int64, device=device)

    def update(self, pred: torch.Tensor, target: torch.Tensor, is_logits: bool = False) -> None:
        _require_cuda(pred, "prediction")
        with torch.cuda.device(pred.device):
            x = _flat(pred.detach().reshape(-1), "prediction")
            y = _flat(_as_f32(target).reshape(-1), "target")
            if x.numel() != y.numel():
                raise ValueError("prediction and target differ in size")
            self._ensure(x.device)
            _lib.call("hpri_pr_curve_hist", _p(x), _p(y), x.numel(), _p(self.thresholds), self.T, int(is_logits),
                      _p(self.hist), _stream())

    def confusion(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(tp, fp, fn, tn) per threshold, int64, on the host."""
        h = self.hist.cpu().view(2, self.T + 1)
        # bin b holds pixels with exactly b thresholds <= p, so pred >= t_k  <=>  b > k
        ge = torch.flip(torch.cumsum(torch.flip(h, dims=[1]), dim=1), dims=[1])[:, 1:]     # [class][k] = #{b > k}
        tot = h.sum(dim=1, keepdim=True)
        tp, fp = ge[1], ge[0]
        return tp, fp, tot[1] - tp, tot[0] - fp

    def compute(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(precision[T+1], recall[T+1], thresholds[T]) exactly as torchmetrics returns them."""
        tp, fp, fn, _ = self.confusion()
        tp, fp, fn = tp.to(torch.float32), fp.to(torch.float32), fn.to(torch.float32)

        def safe_div(a, b):
            b = torch.where(b == 0, torch.ones_like(b), b)
            return a / b

        precision = torch.cat([safe_div(tp, tp + fp), torch.ones(1)])
        recall = torch.cat([safe_div(tp, tp + fn), torch.zeros(1)])
        return precision, recall, self.thresholds.cpu()


def best_dice_threshold(precision: torch.Tensor, recall: torch.Tensor, thresholds: torch.Tensor):
    """The threshold pick of ``model_eval`` (PLTrainer.py:546-556): drop the top and bottom 1 % of the curve,
    Dice = 2PR/(P+R), arg-max, threshold rounded to 2 decimals.  Returns (threshold, precision, recall)."""
    crop = int(len(precision) // 100)
    p, r, t = precision[crop:-crop], recall[crop:-crop], thresholds[crop:-crop]
    dice = 2 * p * r / (p + r)
    i = int(torch.argmax(dice))
    return float(torch.round(t[i].to(torch.float), decimals=2)), float(p[i]), float(r[i])


def average_precision(pred: torch.Tensor, target: torch.Tensor) -> float:
    """``AveragePrecision(task='binary')`` of ``model_eval`` (PLTrainer.py:558-559, 650-651; torchmetrics 1.2.0 with
    ``thresholds=None``): AP = sum_n (R_n - R_{n-1}) P_n over the distinct prediction values in descending order --
    the same definition as ``sklearn.metrics.average_precision_score``.  Exact (no binning): one device sort and two
    cumulative sums with torch's own kernels (plumbing, not the hot path); ties share one threshold."""
    _require_cuda(pred, "prediction")
    p = pred.detach().reshape(-1).to(torch.float32)
    t = (target.reshape(-1).to(torch.int32) != 0)
    order = torch.argsort(p, descending=True, stable=True)
    ps, ts = p[order], t[order]
    tp = torch.cumsum(ts.to(torch.float64), 0)
    fp = torch.cumsum((~ts).to(torch.float64), 0)
    last = torch.ones_like(ps, dtype=torch.bool)            # last element of every run of equal predictions
    last[:-1] = ps[1:] != ps[:-1]
    tp, fp = tp[last], fp[last]
    npos = tp[-1]
    if float(npos) == 0.0:
        return float("nan")
    precision = tp / (tp + fp)
    recall = tp / npos
    prev = torch.cat([torch.zeros(1, dtype=torch.float64, device=recall.device), recall[:-1]])
    return float(((recall - prev) * precision).sum())


# ---------------------------------------------------------------------------------------------------
# The device sort and the exact ranking metrics on it (csrc/sort.hip)
# ---------------------------------------------------------------------------------------------------
def sort_scores(keys: torch.Tensor, descending: bool = True, groups: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """A stable sort of fp32 device keys, read as ``groups`` contiguous groups of equal length: ``(perm, sorted_keys)``, both of
    shape (groups, L).  ``perm[g]`` holds int32 indices inside group ``g`` and equals, bit for bit, the indices of
    ``torch.sort(keys[g], descending=descending, stable=True)``: NaN ranks above +inf, -0.0 equals +0.0, ties keep their index
    order; ``sorted_keys`` are the keys in that order with their original bits.  A radix sort in HIP (15 launches for every size),
    no host synchronisation."""
    _require_cuda(keys, "sort_scores keys")
    groups = int(groups)
    if groups < 1 or keys.numel() == 0 or keys.numel() % groups:
        raise ValueError(f"sort_scores: {keys.numel()} keys do not make {groups} non-empty groups of equal length")
    with torch.cuda.device(keys.device):
        k = _flat(keys.detach(), "sort_scores keys").reshape(groups, -1)
        L = int(k.shape[1])
        nws = _lib.load().hpri_sort_workspace_bytes(groups, L) if k.numel() < 2 ** 31 else 0
        if nws == 0:
            raise ValueError(f"sort_scores: at most 65535 groups and fewer than 2^31 keys, got {groups} groups of {L}")
        ws = torch.empty(nws, dtype=torch.uint8, device=k.device)
        perm = torch.empty((groups, L), dtype=torch.int32, device=k.device)
        out = torch.empty_like(k)
        _lib.call("hpri_sort_keys_f32", _p(k), groups, L, int(bool(descending)), _p(perm), _p(out), _p(ws), nws, _stream())
    return perm, out


def ranking_metrics(scores: torch.Tensor, target: torch.Tensor) -> Dict[str, float]:
    """The exact ranking metrics of a whole split from ONE device sort of its scores (``csrc/sort.hip``; 17 launches, no ATen kernel
    beyond the allocations, one 24-byte read at the end)::

        avg_prec  sum over the runs of equal scores, in descending order, of (R_n - R_{n-1}) P_n: the definition ``average_precision``
                  documents, accumulated in fp64 as sum_runs p_run * tp / (tp + fp), divided by the positives on the host
        roc_auc   the Mann-Whitney statistic with ties counted half: sum_runs p_run * (2 * negatives ranked below + negatives of the
                  run) / (2 P N); the numerator is an exact integer (uint64), divided on the host

    ``scores``: fp32 of any shape (the flat tensors of a ``SplitPrediction``; pass ``torch.sigmoid(logits)`` where parity with the
    reference's AP is wanted: the fp32 sigmoid merges scores into ties, and ties change AP).  ``target``: the same number of
    elements, non-zero = positive; fp32, uint8 and bool are read as they are, other types are converted once.  ``avg_prec`` is NaN
    without a positive, ``roc_auc`` when a class is empty.  -0.0 and +0.0 are one score, and so are all NaNs."""
    _require_cuda(scores, "ranking_metrics scores")
    with torch.cuda.device(scores.device):
        s = _flat(scores.detach(), "ranking_metrics scores").reshape(-1)
        _require_placed(target, "ranking_metrics target")
        t = target.detach().reshape(-1)
        if t.dtype == torch.bool:
            t = t.contiguous().view(torch.uint8)
        elif t.dtype not in (torch.float32, torch.uint8):
            t = t.to(torch.float32)
        t = t.contiguous()
        n = s.numel()
        if n == 0 or t.numel() != n:
            raise ValueError(f"ranking_metrics: need as many targets as scores and at least one, got {n} and {t.numel()}")
        nws = _lib.load().hpri_ranking_workspace_bytes(n)
        if nws == 0:
            raise ValueError(f"ranking_metrics: fewer than 2^31 scores, got {n}")
        ws = torch.empty(nws, dtype=torch.uint8, device=s.device)
        out = torch.empty(3, dtype=torch.int64, device=s.device)
        _lib.call("hpri_ranking_sums", _p(s), _p(t), 0 if t.dtype == torch.float32 else 1, n, _p(out), _p(ws), nws, _stream())
        host = out.cpu()
    ap_num = float(host[:1].view(torch.float64)[0])
    u, p = int(host[1]), int(host[2])
    return _ranking_from_sums(ap_num, u, p, n)


def _ranking_from_sums(ap_num: float, u: int, p: int, n: int) -> Dict[str, float]:
    neg = n - p
    return {"avg_prec": ap_num / p if p else float("nan"), "roc_auc": u / (2 * p * neg) if p and neg else float("nan")}


def ranking_reference(scores, target) -> Dict[str, float]:
    """``ranking_metrics`` restated in numpy on the host: integer counts over the runs of equal fp32 scores (the AUC numerator in
    Python integers, the AP sum in fp64 in run order)."""
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    t = np.asarray(target).reshape(-1) != 0
    order = np.argsort(-s.astype(np.float64), kind="stable")
    ss, ts = s[order], t[order]
    ends = np.nonzero(np.append(ss[1:] != ss[:-1], True))[0]
    tp = np.cumsum(ts.astype(np.int64))[ends]
    fp = (ends + 1) - tp
    p_run = np.diff(tp, prepend=0)
    q_run = np.diff(fp, prepend=0)
    p, n = int(ts.sum()), int(s.size)
    u = sum(int(a) * (2 * ((n - p) - int(b)) + int(c)) for a, b, c in zip(p_run, fp, q_run))
    ap_num = float(np.sum(p_run.astype(np.float64) * (tp.astype(np.float64) / (tp + fp).astype(np.float64))))
    return _ranking_from_sums(ap_num, u, p, n)
