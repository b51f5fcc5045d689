"""The criteria of a step on the GPU: BCE, the imbalance-aware binary family, clDice and cross-entropy.

    crit = BCEWithLogitsLoss()                       # drop-in for nn.BCEWithLogitsLoss() (params_HyperPRI.py:60)
    crit = DiceBCELoss(pos_weight=3.0)               # or an imbalance-aware one (csrc/segloss.hip): SegLoss, DiceLoss, TverskyLoss, FocalLoss
    crit = clDiceLoss(iters=3, base=DiceLoss())      # or with the centerline term for thin roots (csrc/skeleton.hip)
    crit = LovaszHingeLoss()                         # or the convex surrogate of +IoU itself (csrc/sort.hip)
    crit = CrossEntropyLoss(ignore_index=255)        # multi-class (csrc/multiclass.hip)

Each is an autograd function around the HIP library's forward and backward entry points; nothing synchronises with the host.
There is no CPU fallback: tensors must be fp32 on a ROCm device.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib
from ._args import (_TARGET_KIND, _as_f32, _class_logits, _class_target, _flat, _grad_f32, _ignore_args, _p, _planes, _require_cuda,
                    _scalar, _stream)


# ---------------------------------------------------------------------------------------------------
# nn.BCEWithLogitsLoss() (mean)
# ---------------------------------------------------------------------------------------------------
class _BCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred: torch.Tensor, target: torch.Tensor):
        _require_cuda(pred, "BCEWithLogitsLoss input")
        with torch.cuda.device(pred.device):
            x, y = _flat(pred, "BCEWithLogitsLoss input"), _flat(target, "BCEWithLogitsLoss target")
            if x.shape != y.shape:
                raise ValueError(f"Target size ({tuple(y.shape)}) must be the same as input size ({tuple(x.shape)})")
            n = x.numel()
            nws = _lib.load().hpri_bce_workspace_doubles(n)
            ws = torch.empty(nws, dtype=torch.float64, device=x.device)
            loss = torch.empty((), dtype=torch.float32, device=x.device)
            _lib.call("hpri_bce_logits_fwd", _p(x), _p(y), n, _p(loss), _p(ws), nws, _stream())
            ctx.save_for_backward(x, y)
            ctx.shape = pred.shape
        return loss

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        x, y = ctx.saved_tensors
        with torch.cuda.device(x.device):
            g = _grad_f32(gout)
            dx = torch.empty_like(x)
            _lib.call("hpri_bce_logits_bwd", _p(x), _p(y), x.numel(), _p(g), _p(dx), _stream())
        return dx.view(ctx.shape), None


class _FusedLossFn(torch.autograd.Function):
    """The autograd edge between the logits and a loss the head's kernel has already computed (engine.out_conv with a
    pending target).  Backward hands the scalar gradient to the head's backward kernels through the tape's holder and
    returns an all-zero stride-0 marker instead of a gradient tensor: no pass over the logits happens here."""

    @staticmethod
    def forward(ctx, logits: torch.Tensor, slot):
        ctx.holder, ctx.shape = slot.holder, logits.shape
        return slot.loss

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        with torch.cuda.device(gout.device):
            g = _grad_f32(gout)
            marker = torch.zeros(1, dtype=torch.float32, device=g.device).expand(ctx.shape)
        ctx.holder["bce_g"], ctx.holder["bce_marker"] = g, marker
        return marker, None


# ---------------------------------------------------------------------------------------------------
# Imbalance-aware binary losses (csrc/segloss.hip): pos_weight, focal, Dice, Tversky and their weighted sums
# ---------------------------------------------------------------------------------------------------
class _SegLossFn(torch.autograd.Function):
    """cfg = (w_point, pos_weight, focal_gamma, focal_alpha, mean, w_overlap, alpha, beta, s, tversky_gamma, per_image): the scalar
    arguments of hpri_seg_loss_fwd in its order.  Returns (loss, terms); terms carries no gradient."""

    @staticmethod
    def forward(ctx, pred: torch.Tensor, target: torch.Tensor, cfg: tuple):
        _require_cuda(pred, "SegLoss input")
        with torch.cuda.device(pred.device):
            x, y = _flat(pred, "SegLoss input"), _flat(_as_f32(target), "SegLoss target")
            if x.shape != y.shape:
                raise ValueError(f"Target size ({tuple(y.shape)}) must be the same as input size ({tuple(x.shape)})")
            if x.dim() < 1 or x.numel() == 0:
                raise ValueError(f"SegLoss: need (N, ...) logits with at least one element, got {tuple(x.shape)}")
            n_img = int(x.shape[0])
            hw = x.numel() // n_img
            w_point, pos_weight, focal_gamma, focal_alpha, mean, w_overlap, alpha, beta, s, gamma_t, per_image = cfg
            lib = _lib.load()
            nws, nst = lib.hpri_seg_loss_workspace_doubles(n_img, hw), lib.hpri_seg_loss_state_doubles(n_img, int(per_image))
            ws = torch.empty(nws, dtype=torch.float64, device=x.device)
            state = torch.empty(nst, dtype=torch.float64, device=x.device)
            loss = torch.empty((), dtype=torch.float32, device=x.device)
            terms = torch.empty(3, dtype=torch.float32, device=x.device)
            _lib.call("hpri_seg_loss_fwd", _p(x), _p(y), n_img, hw, w_point, pos_weight, focal_gamma, focal_alpha, int(mean), w_overlap,
                      alpha, beta, s, gamma_t, int(per_image), _p(loss), _p(state), nst, _p(terms), _p(ws), nws, _stream())
            ctx.save_for_backward(x, y, state)
            ctx.cfg, ctx.shape = cfg, pred.shape
            ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, gout: torch.Tensor, _gterms=None):
        x, y, state = ctx.saved_tensors
        w_point, pos_weight, focal_gamma, focal_alpha, _, w_overlap, _, _, _, _, per_image = ctx.cfg
        with torch.cuda.device(x.device):
            g = _grad_f32(gout)
            dx = torch.empty_like(x)
            n_img = int(x.shape[0])
            _lib.call("hpri_seg_loss_bwd", _p(x), _p(y), n_img, x.numel() // n_img, w_point, pos_weight, focal_gamma, focal_alpha,
                      w_overlap, int(per_image), _p(state), state.numel(), _p(g), _p(dx), _stream())
        return dx.view(ctx.shape), None, None


class SegLoss(nn.Module):
    """The binary loss family of ``csrc/segloss.hip`` over fp32 logits ``x`` of any shape (N, ...) and a target ``y`` in [0, 1] of the
    same shape (soft labels allowed; other dtypes are converted once)::

        loss = bce_weight * R[ a_t * (1 - p_t)^focal_gamma * ce(x, y) ] + overlap_weight * mean_groups[ (1 - T_g)^tversky_gamma ]
        ce   = pos_weight * y * softplus(-x) + (1 - y) * softplus(x)        a_t = focal_alpha*y + (1 - focal_alpha)(1 - y)  (None: 1)
        T_g  = (I + smooth) / (I + tversky_alpha*(P - I) + tversky_beta*(Y - I) + smooth),   I = sum p*y, P = sum p, Y = sum y

    ``R``: ``reduction`` "mean" or "sum" over all elements; a group is one image (``per_image=True``) or the whole batch.  ``smooth``
    is the ``s`` of that formula: the usual Dice ``(2I + smooth) / (P + Y + smooth)`` is ``tversky_alpha = tversky_beta = 0.5`` with
    half its ``smooth`` (what ``DiceLoss`` passes).  A weight of 0 drops its term: the kernels do not evaluate it.  One pass forward
    (fp64 partial sums in a fixed order -> bit-reproducible), one pass backward, no host synchronisation; the module sits outside the
    network's tape, so it works in every precision mode.  ``last_terms``: the last call's pointwise term, overlap term (both before
    their weights) and mean ``T`` as a 3-element device tensor.  A group without any mass (``D == 0``) counts as ``T = 1``; ``T >= 1``
    contributes 0 with a zero gradient."""

    def __init__(self, bce_weight: float = 1.0, pos_weight=None, focal_gamma: float = 0.0, focal_alpha: Optional[float] = None,
                 overlap_weight: float = 0.0, tversky_alpha: float = 0.5, tversky_beta: float = 0.5, smooth: float = 1.0,
                 tversky_gamma: float = 1.0, per_image: bool = False, reduction: str = "mean"):
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise ValueError(f"SegLoss: reduction must be 'mean' or 'sum', got {reduction!r}")
        self.bce_weight, self.overlap_weight = float(bce_weight), float(overlap_weight)
        self.pos_weight = 1.0 if pos_weight is None else _scalar(pos_weight, "pos_weight")
        self.focal_gamma = float(focal_gamma)
        self.focal_alpha = None if focal_alpha is None else float(focal_alpha)
        self.tversky_alpha, self.tversky_beta = float(tversky_alpha), float(tversky_beta)
        self.smooth, self.tversky_gamma = float(smooth), float(tversky_gamma)
        self.per_image, self.reduction = bool(per_image), reduction
        # (the launchers refuse the same values; here they are refused when the criterion is built)
        if not self.pos_weight > 0:
            raise ValueError(f"SegLoss: pos_weight must be positive, got {self.pos_weight}")
        if not self.focal_gamma >= 0:
            raise ValueError(f"SegLoss: focal_gamma must not be negative, got {self.focal_gamma}")
        if self.focal_alpha is not None and not 0 <= self.focal_alpha <= 1:
            raise ValueError(f"SegLoss: focal_alpha must lie in [0, 1] (None: no class balance), got {self.focal_alpha}")
        if not (self.tversky_alpha >= 0 and self.tversky_beta >= 0 and self.tversky_alpha + self.tversky_beta > 0):
            raise ValueError("SegLoss: tversky_alpha and tversky_beta must not be negative and not both 0")
        if not self.smooth >= 0:
            raise ValueError(f"SegLoss: smooth must not be negative, got {self.smooth}")
        if not self.tversky_gamma > 0:
            raise ValueError(f"SegLoss: tversky_gamma must be positive, got {self.tversky_gamma}")
        if not (self.bce_weight == self.bce_weight and self.overlap_weight == self.overlap_weight) \
                or (self.bce_weight == 0 and self.overlap_weight == 0):
            raise ValueError("SegLoss: bce_weight and overlap_weight are both 0: nothing to compute")
        self.last_terms: Optional[torch.Tensor] = None

    def config(self) -> tuple:
        """The scalar arguments of ``hpri_seg_loss_fwd``, in its order."""
        return (self.bce_weight, self.pos_weight, self.focal_gamma, -1.0 if self.focal_alpha is None else self.focal_alpha,
                self.reduction == "mean", self.overlap_weight, self.tversky_alpha, self.tversky_beta, self.smooth, self.tversky_gamma,
                self.per_image)

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:   # noqa: A002 (torch's names)
        loss, self.last_terms = _SegLossFn.apply(input, target, self.config())
        return loss

    def extra_repr(self) -> str:
        return ", ".join(f"{k}={getattr(self, k)}" for k in ("bce_weight", "pos_weight", "focal_gamma", "focal_alpha", "overlap_weight",
                                                             "tversky_alpha", "tversky_beta", "smooth", "tversky_gamma", "per_image",
                                                             "reduction"))


class DiceLoss(SegLoss):
    """Soft Dice, ``1 - (2 I + smooth) / (P + Y + smooth)`` over the batch (or the mean over the images: ``per_image``)."""

    def __init__(self, smooth: float = 1.0, per_image: bool = False):
        super().__init__(bce_weight=0.0, overlap_weight=1.0, tversky_alpha=0.5, tversky_beta=0.5, smooth=float(smooth) / 2, per_image=per_image)


class TverskyLoss(SegLoss):
    """``(1 - T)^gamma`` with ``T = (I + smooth) / (I + alpha * FP + beta * FN + smooth)``, FP = P - I, FN = Y - I; ``gamma != 1``: the
    focal Tversky loss."""

    def __init__(self, alpha: float = 0.5, beta: float = 0.5, smooth: float = 1.0, gamma: float = 1.0, per_image: bool = False):
        super().__init__(bce_weight=0.0, overlap_weight=1.0, tversky_alpha=alpha, tversky_beta=beta, smooth=smooth, tversky_gamma=gamma,
                         per_image=per_image)


class FocalLoss(SegLoss):
    """torchvision's ``sigmoid_focal_loss(input, target, alpha, gamma, reduction)``; a negative ``alpha`` (or None) switches the class
    balance off, as there."""

    def __init__(self, gamma: float = 2.0, alpha: Optional[float] = 0.25, reduction: str = "mean"):
        super().__init__(focal_gamma=gamma, focal_alpha=None if alpha is None or alpha < 0 else alpha, reduction=reduction)


class DiceBCELoss(SegLoss):
    """``bce_weight * BCEWithLogits(pos_weight) + dice_weight * Dice(smooth)`` in the same two passes."""

    def __init__(self, bce_weight: float = 1.0, dice_weight: float = 1.0, pos_weight=None, smooth: float = 1.0, per_image: bool = False):
        super().__init__(bce_weight=bce_weight, pos_weight=pos_weight, overlap_weight=dice_weight, smooth=float(smooth) / 2,
                         per_image=per_image)


class BCEWithLogitsLoss(nn.Module):
    """``nn.BCEWithLogitsLoss(pos_weight=None, reduction="mean")`` (params_HyperPRI.py:60,223): one fused pass forward
    (fp64 partial sums in a fixed order -> bit-reproducible), one pass backward.  ``pos_weight``: a float or a one-element tensor;
    ``reduction``: "mean" or "sum".  With the defaults this is the unweighted mean of ``csrc/step.hip`` -- the one form the network's
    head can compute itself (``forward_loss``; ``fusable``); any other argument runs ``SegLoss``.  "Default" means the arguments
    left at their defaults: ``pos_weight=1.0`` (or a tensor holding 1) is the same loss mathematically but is taken as a weighted
    one -- it runs ``SegLoss`` (another summation order, so other last bits) and ``SegmentationModel`` does not hand it to the fused
    head.  Pass ``pos_weight=None`` to keep the fused head."""

    def __init__(self, pos_weight=None, reduction: str = "mean"):
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise ValueError(f"BCEWithLogitsLoss: reduction must be 'mean' or 'sum', got {reduction!r}")
        self.pos_weight = None if pos_weight is None else _scalar(pos_weight, "pos_weight")
        self.reduction = reduction
        self._seg = None if pos_weight is None and reduction == "mean" else SegLoss(pos_weight=self.pos_weight, reduction=reduction)

    @property
    def fusable(self) -> bool:
        """True for the default configuration only: the loss ``forward_loss`` computes inside the head's kernels."""
        return self._seg is None

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:   # noqa: A002 (torch's names)
        if self._seg is not None:
            return self._seg(input, target)
        return _BCEFn.apply(input, target)


# ---------------------------------------------------------------------------------------------------
# Soft skeletons and the centerline loss clDice (csrc/skeleton.hip)
# ---------------------------------------------------------------------------------------------------
MAX_SKELETON_ITERS = 32


def _check_iters(iters, who: str) -> int:
    if isinstance(iters, bool) or int(iters) != iters or not 0 <= int(iters) <= MAX_SKELETON_ITERS:
        raise ValueError(f"{who}: iters must be an integer in [0, {MAX_SKELETON_ITERS}], got {iters!r}")
    return int(iters)


class _SoftSkeletonFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p: torch.Tensor, iters: int):
        _require_cuda(p, "soft_skeleton input")
        N, h, w = _planes(p, "soft_skeleton")
        with torch.cuda.device(p.device):
            x = _flat(p, "soft_skeleton input")
            S = torch.empty_like(x)
            saved, nsv = None, 0
            if ctx.needs_input_grad[0]:
                nsv = _lib.load().hpri_soft_skeleton_saved_floats(N, h, w, iters)
                saved = torch.empty(nsv, dtype=torch.float32, device=x.device)
            _lib.call("hpri_soft_skeleton_fwd", _p(x), N, h, w, iters, _p(S), None if saved is None else _p(saved), nsv, _stream())
            if saved is not None:
                ctx.save_for_backward(x, saved)
            ctx.geom = (N, h, w, iters)
        return S

    @staticmethod
    def backward(ctx, gS: torch.Tensor):
        x, saved = ctx.saved_tensors
        N, h, w, iters = ctx.geom
        with torch.cuda.device(x.device):
            g = _grad_f32(gS)
            nws = _lib.load().hpri_soft_skeleton_workspace_floats(N, h, w)
            ws = torch.empty(nws, dtype=torch.float32, device=x.device)
            gp = torch.empty_like(x)
            _lib.call("hpri_soft_skeleton_bwd", _p(x), _p(saved), saved.numel(), _p(g), N, h, w, iters, _p(gp), _p(ws), nws, _stream())
        return gp, None


def soft_skeleton(p: torch.Tensor, iters: int) -> torch.Tensor:
    """The soft skeleton of clDice (Shit et al., CVPR 2021) of fp32 device planes ``p`` (N, ..., h, w) with values in [0, 1]::

        I_0 = p,  I_{j+1} = E(I_j),  d_j = I_j - D(I_{j+1}),  S_0 = relu(d_0),  S_j = S_{j-1} + relu(d_j - S_{j-1} * d_j),  j <= iters

    ``E``: the minimum over the plus neighbourhood, ``D``: the maximum over the 3x3 neighbourhood, both over their in-image part
    (``soft_erode`` / ``soft_dilate`` of the published code).  One launch forward for all levels, ``iters + 1`` launches backward;
    a min or a max sends its gradient to its first optimum in scan order (``soft_skeleton_reference`` restates the rule), gathered
    without atomics: bit-reproducible.  With a gradient the forward keeps ``2 * iters + 1`` planes of ``p``'s size."""
    return _SoftSkeletonFn.apply(p, _check_iters(iters, "soft_skeleton"))


class _clDiceFn(torch.autograd.Function):
    """cfg = (iters, smooth, per_image, weight, base_weight).  Returns (loss, terms) with loss = weight * cl + base_weight * base_loss
    (``base_loss``: a device scalar or None); terms = (cl, tprec, tsens) carries no gradient."""

    @staticmethod
    def forward(ctx, pred: torch.Tensor, target: torch.Tensor, base_loss: Optional[torch.Tensor], cfg: tuple):
        _require_cuda(pred, "clDiceLoss input")
        with torch.cuda.device(pred.device):
            x, y = _flat(pred, "clDiceLoss input"), _flat(_as_f32(target), "clDiceLoss target")
            if x.shape != y.shape:
                raise ValueError(f"Target size ({tuple(y.shape)}) must be the same as input size ({tuple(x.shape)})")
            N, h, w = _planes(x, "clDiceLoss")
            iters, smooth, per_image, weight, base_weight = cfg
            lib = _lib.load()
            nsv, nws = lib.hpri_soft_skeleton_saved_floats(N, h, w, iters), lib.hpri_cldice_workspace_doubles(N, h, w)
            nst = lib.hpri_cldice_state_doubles(N, int(per_image))
            saved = torch.empty(nsv, dtype=torch.float32, device=x.device)
            p, Sy = torch.empty_like(x), torch.empty_like(x)
            ws = torch.empty(nws, dtype=torch.float64, device=x.device)
            state = torch.empty(nst, dtype=torch.float64, device=x.device)
            loss = torch.empty((), dtype=torch.float32, device=x.device)
            terms = torch.empty(3, dtype=torch.float32, device=x.device)
            base = None if base_loss is None else base_loss.detach().to(torch.float32).contiguous()
            _lib.call("hpri_cldice_fwd", _p(x), _p(y), N, h, w, iters, smooth, int(per_image), weight, None if base is None else _p(base),
                      base_weight, _p(p), None, _p(Sy), _p(saved), nsv, _p(loss), _p(terms), _p(state), nst, _p(ws), nws, _stream())
            ctx.save_for_backward(x, y, p, Sy, saved, state)
            ctx.cfg, ctx.geom, ctx.shape, ctx.has_base = cfg, (N, h, w), pred.shape, base_loss is not None
            ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, gout: torch.Tensor, _gterms=None):
        x, y, p, Sy, saved, state = ctx.saved_tensors
        iters, _, per_image, _, base_weight = ctx.cfg
        N, h, w = ctx.geom
        with torch.cuda.device(x.device):
            g = _grad_f32(gout)
            nws = _lib.load().hpri_soft_skeleton_workspace_floats(N, h, w)
            ws = torch.empty(nws, dtype=torch.float32, device=x.device)
            dx = torch.empty_like(x)
            gbase = torch.empty((), dtype=torch.float32, device=x.device) if ctx.has_base else None
            _lib.call("hpri_cldice_bwd", _p(x), _p(y), _p(p), _p(Sy), _p(saved), saved.numel(), N, h, w, iters, int(per_image), _p(state),
                      state.numel(), _p(g), base_weight, None if gbase is None else _p(gbase), _p(dx), _p(ws), nws, _stream())
        return dx.view(ctx.shape), None, gbase, None


class clDiceLoss(nn.Module):
    """``(1 - alpha) * base(x, y) + alpha * cl(x, y)`` over fp32 logits ``x`` (N, ..., h, w) and a target of the same shape, with the
    centerline term of clDice (Shit et al., CVPR 2021; ``csrc/skeleton.hip``)::

        Sp = soft_skeleton(sigmoid(x), iters),  Sy = soft_skeleton(y, iters)          (no gradient into y)
        tprec = (sum Sp*y + smooth) / (sum Sp + smooth),  tsens = (sum Sy*p + smooth) / (sum Sy + smooth)
        cl = mean over groups of 1 - 2 * tprec * tsens / (tprec + tsens)

    A group is one plane (``per_image=True``) or the whole batch.  ``base``: a ``SegLoss`` (any of its family) or a
    ``BCEWithLogitsLoss``; default ``DiceLoss(smooth, per_image)``.  It runs through its own path untouched; the weighted sum is
    formed inside the centerline term's finalize kernel and the base's upstream gradient inside its last backward launch, so no
    other kernel than the two losses' own is launched (autograd adds their two logit gradients).  ``alpha = 0`` is ``base`` alone, bit
    for bit, without any skeleton launch; ``alpha = 1`` does not evaluate ``base``.  Forward: one launch for both skeletons and the
    sums plus a finalize; backward: ``iters + 1`` launches; fp64 sums in a fixed order, gathers instead of atomics: bit-reproducible,
    no host synchronisation.  The forward keeps ``2 * iters + 3`` planes of the logits' size for the backward.  The module sits
    outside the network's tape, like ``SegLoss``, so it works in every precision mode.  A ratio whose denominator is 0 (``smooth = 0``
    and an empty skeleton) counts as 0; ``tprec + tsens == 0`` gives ``cl = 1`` with a zero gradient.  ``last_terms``: the last
    call's ``cl``, mean ``tprec`` and mean ``tsens`` as a 3-element device tensor."""

    def __init__(self, iters: int = 3, alpha: float = 0.5, smooth: float = 1.0, base: Optional[nn.Module] = None, per_image: bool = False):
        super().__init__()
        self.iters = _check_iters(iters, "clDiceLoss")
        self.alpha, self.smooth, self.per_image = float(alpha), float(smooth), bool(per_image)
        if not 0 <= self.alpha <= 1:
            raise ValueError(f"clDiceLoss: alpha must lie in [0, 1], got {self.alpha}")
        if not self.smooth >= 0:
            raise ValueError(f"clDiceLoss: smooth must not be negative, got {self.smooth}")
        if base is None:
            base = DiceLoss(self.smooth, self.per_image)
        if not isinstance(base, (SegLoss, BCEWithLogitsLoss)):
            raise TypeError(f"clDiceLoss: base must be a SegLoss or a BCEWithLogitsLoss, got {type(base).__name__}")
        self.base = base
        self.last_terms: Optional[torch.Tensor] = None

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:   # noqa: A002 (torch's names)
        if self.alpha == 0:
            return self.base(input, target)
        base_loss = None if self.alpha == 1 else self.base(input, target)
        loss, self.last_terms = _clDiceFn.apply(input, target, base_loss, (self.iters, self.smooth, self.per_image, self.alpha, 1.0 - self.alpha))
        return loss

    def extra_repr(self) -> str:
        return ", ".join(f"{k}={getattr(self, k)}" for k in ("iters", "alpha", "smooth", "per_image"))


# ---------------------------------------------------------------------------------------------------
# The Lovasz hinge on the device sort (csrc/sort.hip)
# ---------------------------------------------------------------------------------------------------
def _check_ignore_index(ignore_index, who: str) -> Optional[int]:
    if ignore_index is None:
        return None
    if isinstance(ignore_index, bool) or int(ignore_index) != ignore_index or abs(int(ignore_index)) >= 2 ** 24:
        raise ValueError(f"{who}: ignore_index must be None or an integer an fp32 target can hold exactly, got {ignore_index!r}")
    return int(ignore_index)


class _LovaszHingeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred: torch.Tensor, target: torch.Tensor, per_image: bool, ignore_index: Optional[int]):
        _require_cuda(pred, "LovaszHingeLoss input")
        with torch.cuda.device(pred.device):
            x, y = _flat(pred, "LovaszHingeLoss input"), _flat(_as_f32(target), "LovaszHingeLoss target")
            if x.shape != y.shape:
                raise ValueError(f"Target size ({tuple(y.shape)}) must be the same as input size ({tuple(x.shape)})")
            if x.dim() < 1 or x.numel() == 0:
                raise ValueError(f"LovaszHingeLoss: need (N, ...) logits with at least one element, got {tuple(x.shape)}")
            n_img = int(x.shape[0])
            hw = x.numel() // n_img
            use_ignore, ignore = _ignore_args(ignore_index)
            nws = _lib.load().hpri_lovasz_hinge_workspace_bytes(n_img, hw, int(per_image))
            if nws == 0:
                raise ValueError(f"LovaszHingeLoss: at most 65535 images and fewer than 2^31 elements, got {tuple(x.shape)}")
            ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
            loss = torch.empty((), dtype=torch.float32, device=x.device)
            coef = torch.empty_like(x)
            _lib.call("hpri_lovasz_hinge_fwd", _p(x), _p(y), n_img, hw, int(per_image), use_ignore, ignore, _p(loss), _p(coef), _p(ws),
                      nws, _stream())
            ctx.save_for_backward(coef)
            ctx.shape = pred.shape
        return loss

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        coef, = ctx.saved_tensors
        with torch.cuda.device(coef.device):
            g = _grad_f32(gout)
            dx = torch.empty_like(coef)
            _lib.call("hpri_lovasz_hinge_bwd", _p(coef), coef.numel(), _p(g), _p(dx), _stream())
        return dx.view(ctx.shape), None, None, None


class LovaszHingeLoss(nn.Module):
    """The Lovasz hinge (Berman et al., CVPR 2018), the convex surrogate of the Jaccard index (+IoU) the reference scores by, over
    fp32 logits ``x`` of any shape (N, ...) and a target ``y`` of the same shape (``csrc/sort.hip``)::

        s_i = +1 if y_i >= 0.5 else -1,   e_i = 1 - x_i * s_i                                         (fp32)
        per group: the pixels by e descending, ties in index order;  G1 = the group's positives
        at rank r:  P_r = positives among ranks 0..r,  I_r = G1 - P_r,  U_r = G1 + (r + 1 - P_r),  J_r = 1 - I_r / U_r
        loss_g = sum_r relu(e_(r)) * (J_r - J_{r-1}),   loss = mean over the groups

    A group is one image (``per_image=True``, the default of the published code) or the whole batch.  ``ignore_index``: pixels
    whose target equals it are left out of the order, the counts and the gradient; a group with nothing left contributes 0.  The
    weights ``J_r - J_{r-1}`` are evaluated without cancellation in fp64 from integer counts (``1 / U_r`` for a positive pixel,
    ``I_r / ((U_r - 1) U_r)`` for a negative one; ``G1 == 0``: all weight on rank 0) and are constants of the gradient, as in the
    published code: ``d loss / d x_i = -s_i * w_rank(i) / groups`` where ``e_i > 0`` and exactly 0 elsewhere.  The forward sorts on
    the device (17 launches, fp64 sums in a fixed order -> bit-reproducible, no host synchronisation) and leaves one coefficient per
    pixel; the backward is one elementwise launch.  The module sits outside the network's tape, like ``SegLoss``, so it works in
    every precision mode and as ``SegmentationModel(net, criterion=LovaszHingeLoss())``.  No double backward."""

    def __init__(self, per_image: bool = True, ignore_index: Optional[int] = None):
        super().__init__()
        self.per_image = bool(per_image)
        self.ignore_index = _check_ignore_index(ignore_index, "LovaszHingeLoss")

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:   # noqa: A002 (torch's names)
        return _LovaszHingeFn.apply(input, target, self.per_image, self.ignore_index)

    def extra_repr(self) -> str:
        return f"per_image={self.per_image}, ignore_index={self.ignore_index}"


def lovasz_hinge_reference(x, y, per_image: bool = True, ignore_index: Optional[int] = None) -> Tuple[float, np.ndarray]:
    """``LovaszHingeLoss`` restated in numpy: (loss, d loss / d x) in fp64 for arrays ``x``, ``y`` of one shape (N, ...).  The errors
    ``e`` are formed in fp32, as the kernels form them; the order is a stable descending sort; the weights are the closed form."""
    x32, y32 = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
    if x32.shape != y32.shape or x32.ndim < 1 or x32.size == 0:
        raise ValueError(f"lovasz_hinge_reference: need x and y of one shape (N, ...), got {x32.shape} and {y32.shape}")
    rows = x32.shape[0] if per_image else 1
    xs, ys = x32.reshape(rows, -1), y32.reshape(rows, -1)
    grad = np.zeros(xs.shape, dtype=np.float64)
    total = 0.0
    for g in range(rows):
        keep = np.ones(xs.shape[1], dtype=bool) if ignore_index is None else ys[g] != np.float32(ignore_index)
        at = np.nonzero(keep)[0]
        if at.size == 0:
            continue
        pos = ys[g][at] >= np.float32(0.5)
        s = np.where(pos, np.float32(1), np.float32(-1)).astype(np.float32)
        e = (np.float32(1) - xs[g][at] * s).astype(np.float32)
        order = np.argsort(-e.astype(np.float64), kind="stable")
        es, ps = e[order].astype(np.float64), pos[order]
        G1 = int(ps.sum())
        P = np.cumsum(ps.astype(np.int64))
        r = np.arange(at.size, dtype=np.int64)
        U = (G1 + (r + 1 - P)).astype(np.float64)
        I = (G1 - P).astype(np.float64)                                   # noqa: E741
        if G1 == 0:
            w = np.zeros(at.size, dtype=np.float64)
            w[0] = 1.0
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                w = np.where(ps, 1.0 / U, I / ((U - 1.0) * U))
        on = es > 0
        total += float(np.sum(np.where(on, es, 0.0) * w))
        grad[g, at[order]] = np.where(on, -s[order].astype(np.float64) * w / rows, 0.0)
    return total / rows, grad.reshape(x32.shape)


def _takes_fused_head(criterion: nn.Module) -> bool:
    """Only a default-configured ``BCEWithLogitsLoss`` (no subclass) is what ``forward_loss`` computes: a weighted or sum-reduced one
    must never be replaced by the unweighted fused loss."""
    return type(criterion) is BCEWithLogitsLoss and criterion.fusable


# ---------------------------------------------------------------------------------------------------
# nn.CrossEntropyLoss (csrc/multiclass.hip)
# ---------------------------------------------------------------------------------------------------
class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor], ignore_index: Optional[int], mean: bool):
        x = _class_logits(pred, "CrossEntropyLoss input")
        with torch.cuda.device(x.device):
            t = _class_target(target, x, "CrossEntropyLoss target")
            N, K, h, w = (int(v) for v in x.shape)
            if weight is not None:
                _require_cuda(weight, "CrossEntropyLoss weight")
                if tuple(weight.shape) != (K,):
                    raise ValueError(f"CrossEntropyLoss: weight must have shape ({K},), got {tuple(weight.shape)}")
                weight = weight.contiguous()
            use_ignore, ignore = _ignore_args(ignore_index)
            nws = _lib.load().hpri_softmax_ce_workspace_doubles(N * h * w)
            ws = torch.empty(nws, dtype=torch.float64, device=x.device)
            lse = torch.empty((N, h * w), dtype=torch.float32, device=x.device)
            loss = torch.empty((), dtype=torch.float32, device=x.device)
            denom = torch.empty((), dtype=torch.float32, device=x.device)
            _lib.call("hpri_softmax_ce_fwd", _p(x), _p(t), _TARGET_KIND[t.dtype], _p(weight), N, K, h * w, use_ignore, ignore,
                      int(mean), _p(loss), _p(lse), _p(denom), None, _p(ws), nws, _stream())
            ctx.save_for_backward(x, lse, t, denom, *(() if weight is None else (weight,)))
            ctx.ignore, ctx.shape = (use_ignore, ignore), pred.shape
        return loss

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        x, lse, t, denom, *rest = ctx.saved_tensors
        weight = rest[0] if rest else None
        with torch.cuda.device(x.device):
            g = _grad_f32(gout)
            N, K, h, w = (int(v) for v in x.shape)
            dx = torch.empty_like(x)
            _lib.call("hpri_softmax_ce_bwd", _p(x), _p(lse), _p(t), _TARGET_KIND[t.dtype], _p(weight), N, K, h * w, *ctx.ignore,
                      _p(denom), _p(g), _p(dx), _stream())
        return dx.view(ctx.shape), None, None, None, None


class CrossEntropyLoss(nn.Module):
    """``nn.CrossEntropyLoss(weight, ignore_index, reduction)`` over (N, K, h, w) fp32 logits, 2 <= K <= 64, and one class index per
    pixel -- (N, h, w) or (N, 1, h, w), fp32 holding integers (what ``CubeCache`` emits), uint8 or int64; other integer types are
    converted.  One pass forward (log-sum-exp per pixel, fp64 partial sums in a fixed order -> bit-reproducible), one pass
    backward.  ``reduction``: "mean" (the loss sum over the weight sum of the pixels that count, as torch) or "sum".

    A target outside [0, K) that is not ``ignore_index`` cannot raise without a host synchronisation: it makes the loss NaN
    (and leaves zeros in that pixel's gradient) instead of faulting.  An all-ignored "mean" batch is NaN, as in torch."""

    def __init__(self, weight: Optional[torch.Tensor] = None, ignore_index: Optional[int] = -100, reduction: str = "mean"):
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise ValueError(f"CrossEntropyLoss: reduction must be 'mean' or 'sum', got {reduction!r}")
        if weight is not None and weight.dim() != 1:
            raise ValueError(f"CrossEntropyLoss: weight must be a (K,) tensor, got {tuple(weight.shape)}")
        self.register_buffer("weight", None if weight is None else weight.detach().to(torch.float32).clone())
        self.ignore_index = ignore_index
        self.reduction = reduction

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:   # noqa: A002 (torch's names)
        return _CEFn.apply(input, target, self.weight, self.ignore_index, self.reduction == "mean")
