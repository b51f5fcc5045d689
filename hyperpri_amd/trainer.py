"""The caller-side tail of a step on the GPU: the fused loss, the step logic of the reference's model, checkpoints.

SURVEY.md 8f rank 2-4.  Names and semantics follow ``RootLightningModel`` (PLTrainer.py:34-183) and its checkpoint helpers
(:186-216, :270-330), without Lightning or torchmetrics.  The criteria live in ``losses.py``, the device-side metrics in
``metrics.py``, the fused optimizers in ``optim.py``; their names are importable from here as before.

    model = SegmentationModel(net, DiceBCELoss(pos_weight=3.0), optimizer="Adam", lr=1e-3)
    loss = model.training_step({"image": x, "mask": m})

There is no CPU fallback: tensors must be fp32 on a ROCm device.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import _lib  # noqa: F401
from . import engine as _engine
from ._args import (MAX_CLASSES, _TARGET_KIND, _as_f32, _class_logits, _class_target, _flat, _ignore_args, _planes,  # noqa: F401
                    _require_cuda, _scalar)
# every name that lived in this module before it was split stays importable from it
from .losses import (MAX_SKELETON_ITERS, BCEWithLogitsLoss, CrossEntropyLoss, DiceBCELoss, DiceLoss, FocalLoss, LovaszHingeLoss,  # noqa: F401
                     SegLoss, TverskyLoss, _LovaszHingeFn, lovasz_hinge_reference, _BCEFn, _CEFn, _check_iters, _clDiceFn, _FusedLossFn, _SegLossFn, _SoftSkeletonFn, _takes_fused_head,
                     clDiceLoss, soft_skeleton)
from .metrics import (PRCurve, SegConfusion, SegCounts, _confusion_pass, _split_counts, _StepConfusion, _StepCounts,  # noqa: F401
                      argmax_classes, average_precision, best_dice_threshold, metrics_from_counts, multiclass_metrics_from_confusion,
                      ranking_metrics, ranking_reference, sort_scores)
from .optim import FusedAdam, FusedSGD, _ptr_array  # noqa: F401


def forward_loss(network: nn.Module, image: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``pred = network(image); loss = nn.BCEWithLogitsLoss()(pred, target)`` (PLTrainer.py:85-86) as one call, so that the
    loss is computed inside the network's last layer (forward: the 1x1 head also leaves the BCE partial sums; backward:
    the head's gradient kernels form (sigmoid(pred) - target)/n themselves).  Same values as the two-call form up to
    fp32 summation order inside the head's weight gradient; falls back to the two-call form when the network's head does
    not take the offer (hooks, ``fused_tape = False``, no gradient recording).

    What differs from the two-call form, by design: the autograd edge from the loss to ``pred`` carries an all-zero stride-0
    marker, not ``(sigmoid(pred) - target) / n`` -- the head's backward kernels form that product themselves.  So
    ``torch.autograd.grad(loss, pred)``, ``pred.retain_grad()`` and tensor hooks on ``pred`` see zeros for the loss's share
    (parameter and input gradients are complete and bit-identical to the two-call form).  Code that inspects dLoss/dLogits should
    call ``criterion(network(image), target)`` instead.  The logits and the target are re-read in backward: an in-place write to
    either in between raises, as it would for tensors saved by ``nn.BCEWithLogitsLoss``."""
    _require_cuda(image, "input tensor")
    with torch.cuda.device(image.device):
        tgt = _flat(_as_f32(target), "BCEWithLogitsLoss target")
    with _engine.pending_bce(tgt) as slot:
        pred = network(image)
    if isinstance(pred, tuple):                      # analyze=True networks return (pred, features)
        pred = pred[0]
    if pred.shape != target.shape:
        # nn.BCEWithLogitsLoss (and _BCEFn) refuse e.g. an (N,H,W) mask against (N,1,H,W) logits; so does the fused form, whose
        # kernels only ever compared element counts
        if slot.holder is not None:
            slot.holder.clear()
        raise ValueError(f"Target size ({tuple(target.shape)}) must be the same as input size ({tuple(pred.shape)})")
    if slot.used and slot.holder is not None and pred.requires_grad and pred.numel() == tgt.numel():
        return pred, _FusedLossFn.apply(pred, slot)
    return pred, _BCEFn.apply(pred, target)


# ---------------------------------------------------------------------------------------------------
# RootLightningModel without Lightning (PLTrainer.py:34-183)
# ---------------------------------------------------------------------------------------------------
class SegmentationModel(nn.Module):
    """The step logic of ``RootLightningModel``: same attribute names (``m_network``, ``f_criterion``,
    ``threshold``, ``predict_labels``), same step methods, metrics accumulated on the device and read by
    ``epoch_metrics`` (the ``on_epoch=True`` logging of the reference)."""

    def __init__(self, network: nn.Module, criterion: Optional[nn.Module] = None, optimizer: str = "Adam",
                 lr: float = 1e-3, weight_decay: float = 0.0, momentum: float = 0.9, threshold: float = 0.5,
                 task: str = "binary", num_classes: int = 1):
        super().__init__()
        if task not in ("binary", "multiclass"):
            raise ValueError(f"SegmentationModel: task must be 'binary' or 'multiclass', got {task!r}")
        if task == "multiclass" and not 2 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"SegmentationModel: a multiclass task needs 2 <= num_classes <= {MAX_CLASSES}, got {num_classes}")
        self.task, self.num_classes = task, int(num_classes)
        self.m_network = network
        if criterion is None:
            criterion = BCEWithLogitsLoss() if task == "binary" else CrossEntropyLoss()
        self.f_criterion = criterion
        self.p_optimizer, self.p_learn_rate, self.p_decay, self.p_momentum = optimizer, lr, weight_decay, momentum
        self.threshold = threshold
        self.predict_labels: List[torch.Tensor] = []
        self._counts: Dict[str, "_StepCounts"] = {}
        self._loss: Dict[str, List[torch.Tensor]] = {}

    # -- PLTrainer.py:166-183
    def configure_optimizers(self):
        name = self.p_optimizer.upper()
        if name == "ADAM":
            return FusedAdam(self.m_network.parameters(), lr=self.p_learn_rate, weight_decay=self.p_decay)
        if name == "SGD":
            return FusedSGD(self.m_network.parameters(), lr=self.p_learn_rate, momentum=self.p_momentum,
                            weight_decay=self.p_decay)
        raise RuntimeError(f"Optimizer {self.p_optimizer} not supported")

    def _forward(self, image: torch.Tensor) -> torch.Tensor:
        if getattr(self.m_network, "analyze", False):
            pred, _ = self.m_network(image)
            return pred
        return self.m_network(image)

    def _step(self, stage: str, batch, threshold: float) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.task == "multiclass":                # the threshold plays no part: the prediction is the argmax
            pred = self._forward(batch["image"])
            loss = self.f_criterion(pred, batch["mask"])
            c = self._counts.get(stage)
            if c is None:
                c = self._counts[stage] = _StepConfusion(self.num_classes, getattr(self.f_criterion, "ignore_index", None), pred.device)
            c.update(pred, batch["mask"])
            self._loss.setdefault(stage, []).append(loss.detach())
            return pred, loss
        if _takes_fused_head(self.f_criterion) and torch.is_grad_enabled():
            pred, loss = forward_loss(self.m_network, batch["image"], batch["mask"])      # loss inside the head's kernels
        else:
            pred = self._forward(batch["image"])
            loss = self.f_criterion(pred, batch["mask"])
        c = self._counts.get(stage)
        if c is None or c.threshold != threshold:
            c = self._counts[stage] = _StepCounts(threshold, pred.device)
        c.update(pred, batch["mask"])
        self._loss.setdefault(stage, []).append(loss.detach())
        return pred, loss

    def training_step(self, batch, batch_idx: int = 0) -> torch.Tensor:       # PLTrainer.py:79-98
        return self._step("tr", batch, self.threshold)[1]

    def validation_step(self, batch, batch_idx: int = 0) -> None:             # PLTrainer.py:100-118 (threshold 0.5)
        self._step("val", batch, 0.5)

    def test_step(self, batch, batch_idx: int = 0) -> torch.Tensor:           # PLTrainer.py:120-140
        return self._step("test", batch, self.threshold)[0]

    def predict_step(self, batch, batch_idx: int = 0) -> torch.Tensor:        # PLTrainer.py:142-162
        self.predict_labels.append(batch["mask"].cpu())
        return self._forward(batch["image"]).cpu()

    def epoch_metrics(self, stage: str, reset: bool = True) -> Dict[str, float]:
        """{'<stage>_loss', '<stage>_acc', '<stage>_dice', '<stage>_pos_iou'} over the steps since the last reset, as
        the reference logs them: every step computes its own Accuracy / Dice / +IoU and ``self.log(..., on_epoch=True)``
        averages the per-step VALUES weighted by batch size (PLTrainer.py:88-96, 113-118) -- a mean of ratios, which is
        what ``ModelCheckpoint(monitor='val_dice')`` (PLTrainer.py:352) ranks checkpoints by.  The ratio of the epoch's
        summed counts (what one would report for the whole split) is returned beside it under ``<stage>_*_pooled``.

        ``task="multiclass"``: '<stage>_loss', '_acc', '_mean_iou', '_mean_dice' by the same rule -- every step's own
        ``multiclass_metrics_from_confusion`` values (and its loss), averaged weighted by batch size -- beside
        '<stage>_acc_pooled', '_mean_iou_pooled', '_mean_dice_pooled' and '_iou_per_class_pooled' from the summed matrix.  Raises
        ``ValueError`` if a step met a target outside [0, num_classes) that was not the criterion's ``ignore_index``."""
        if self.task == "multiclass":
            return self._epoch_metrics_multiclass(stage, reset)
        out: Dict[str, float] = {}
        if stage in self._loss and self._loss[stage]:
            out[f"{stage}_loss"] = float(torch.stack(self._loss[stage]).mean())
        if stage in self._counts and self._counts[stage].n:
            steps, weights = self._counts[stage].rows()      # the one host synchronisation
            wsum = float(sum(weights))
            per = [metrics_from_counts(*r) for r in steps]
            for k in ("acc", "dice", "pos_iou"):
                out[f"{stage}_{k}"] = sum(w * m[k] for w, m in zip(weights, per)) / wsum
            pooled = metrics_from_counts(*[sum(r[j] for r in steps) for j in range(4)])
            out.update({f"{stage}_acc_pooled": pooled["acc"], f"{stage}_dice_pooled": pooled["dice"],
                        f"{stage}_pos_iou_pooled": pooled["pos_iou"]})
        if reset:
            self._loss.pop(stage, None)
            if stage in self._counts:
                self._counts[stage].reset()
        return out

    def _epoch_metrics_multiclass(self, stage: str, reset: bool) -> Dict[str, object]:
        out: Dict[str, object] = {}
        c = self._counts.get(stage)
        if c is not None and c.n:
            try:
                rows, weights = c.rows()                     # the one host synchronisation
                wsum = float(sum(weights))
                K = self.num_classes
                per = [multiclass_metrics_from_confusion(_split_counts(r, K)) for r in rows]
                losses = self._loss.get(stage) or []
                if len(losses) == len(weights):
                    out[f"{stage}_loss"] = sum(w * v for w, v in zip(weights, torch.stack(losses).tolist())) / wsum
                for k in ("acc", "mean_iou", "mean_dice"):
                    out[f"{stage}_{k}"] = sum(w * m[k] for w, m in zip(weights, per)) / wsum
                pooled = multiclass_metrics_from_confusion([[sum(r[i * K + j] for r in rows) for j in range(K)] for i in range(K)])
                out.update({f"{stage}_acc_pooled": pooled["acc"], f"{stage}_mean_iou_pooled": pooled["mean_iou"],
                            f"{stage}_mean_dice_pooled": pooled["mean_dice"], f"{stage}_iou_per_class_pooled": pooled["iou_per_class"]})
            finally:
                if reset:
                    self._loss.pop(stage, None)
                    c.reset()
        elif reset:
            self._loss.pop(stage, None)
        return out


# ---------------------------------------------------------------------------------------------------
# checkpoint formats (PLTrainer.py:186-216, 270-330)
# ---------------------------------------------------------------------------------------------------
def network_state_dict(raw: dict) -> "OrderedDict[str, torch.Tensor]":
    """Whatever ``load_val_model`` accepts -> the network's own ``state_dict`` keys.

    * Lightning ``.ckpt`` (has ``'pytorch-lightning_version'``; weights under ``state_dict`` as ``m_network.<key>``),
    * raw ``best_wts.pt`` (plain keys, or ``module.<key>`` from ``nn.DataParallel``/DDP),
    * consolidated DeepSpeed ZeRO-2 (``_forward_module.m_network.<key>``; ``feat_ext`` entries dropped,
      PLTrainer.py:203-211).
    """
    sd = raw["state_dict"] if "pytorch-lightning_version" in raw else raw
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for k, v in sd.items():
        k = k.replace("_forward_module.m_network.", "")
        if "feat_ext" in k:
            continue
        if k.startswith("m_network."):
            k = k[len("m_network."):]
        elif "module." in k:
            k = k.replace("module.", "", 1)
        out[k] = v
    return out


def load_checkpoint(network: nn.Module, path: str) -> nn.Module:
    network.load_state_dict(network_state_dict(torch.load(path, map_location="cpu")))
    return network
