"""The caller-side tail of a step on the GPU: loss, segmentation metrics, PR curve, optimizer, checkpoints.

SURVEY.md 8f rank 2-4.  Everything here mirrors what ``src/PLTrainer.py`` does around the network call --
names and semantics follow ``RootLightningModel`` (PLTrainer.py:34-183) and its evaluation helpers
(:270-330, :525-562) -- but none of it needs Lightning or torchmetrics, and every reduction runs in the HIP
library (``csrc/step.hip``) without a host synchronisation until a value is actually read.

    crit = BCEWithLogitsLoss()                       # drop-in for nn.BCEWithLogitsLoss() (params_HyperPRI.py:60)
    crit = DiceBCELoss(pos_weight=3.0)               # or an imbalance-aware one (csrc/segloss.hip): SegLoss, DiceLoss, TverskyLoss, FocalLoss
    crit = clDiceLoss(iters=3, base=DiceLoss())      # or with the centerline term for thin roots (csrc/skeleton.hip)
    opt  = FusedAdam(net.parameters(), lr=1e-3)      # drop-in for optim.Adam (PLTrainer.py:171-174)
    model = SegmentationModel(net, crit, optimizer="Adam", lr=1e-3)
    loss = model.training_step({"image": x, "mask": m})

There is no CPU fallback: tensors must be fp32 on a ROCm device.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict
from typing import Dict, Iterable, List, Optional, Tuple

import torch
from torch import nn

from . import _lib
from . import engine as _engine
from .engine import _p, _require_cuda, _stream, bump_param_epoch


def _flat(t: torch.Tensor, what: str) -> torch.Tensor:
    _require_cuda(t, what)
    return t if t.is_contiguous() else t.contiguous()


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
            g = gout.contiguous().to(torch.float32)
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
            g = gout.contiguous().to(torch.float32)
            marker = torch.zeros(1, dtype=torch.float32, device=g.device).expand(ctx.shape)
        ctx.holder["bce_g"], ctx.holder["bce_marker"] = g, marker
        return marker, None


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
        tgt = _flat(target if target.dtype == torch.float32 else target.to(torch.float32), "BCEWithLogitsLoss target")
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
    if pred.shape != target.shape:
        raise ValueError(f"Target size ({tuple(target.shape)}) must be the same as input size ({tuple(pred.shape)})")
    return pred, _BCEFn.apply(pred, target)


# ---------------------------------------------------------------------------------------------------
# Imbalance-aware binary losses (csrc/segloss.hip): pos_weight, focal, Dice, Tversky and their weighted sums
# ---------------------------------------------------------------------------------------------------
def _scalar(v, what: str) -> float:
    """A float, or a one-element tensor read once (at construction, never inside a step)."""
    if isinstance(v, torch.Tensor):
        if v.numel() != 1:
            raise ValueError(f"{what} must be a float or a one-element tensor, got shape {tuple(v.shape)}")
        return float(v.detach().reshape(()).cpu())
    return float(v)


class _SegLossFn(torch.autograd.Function):
    """cfg = (w_point, pos_weight, focal_gamma, focal_alpha, mean, w_overlap, alpha, beta, s, tversky_gamma, per_image): the scalar
    arguments of hpri_seg_loss_fwd in its order.  Returns (loss, terms); terms carries no gradient."""

    @staticmethod
    def forward(ctx, pred: torch.Tensor, target: torch.Tensor, cfg: tuple):
        _require_cuda(pred, "SegLoss input")
        with torch.cuda.device(pred.device):
            if target.dtype != torch.float32:
                target = target.to(torch.float32)
            x, y = _flat(pred, "SegLoss input"), _flat(target, "SegLoss target")
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
            g = gout.contiguous().to(torch.float32)
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


def _planes(t: torch.Tensor, who: str) -> Tuple[int, int, int]:
    """(N, h, w) of a (N, ..., h, w) tensor read as planes."""
    if t.dtype != torch.float32:
        raise ValueError(f"{who}: need float32, got {t.dtype}")
    if t.dim() < 2 or t.numel() == 0:
        raise ValueError(f"{who}: need (N, ..., h, w) planes with at least one element, got {tuple(t.shape)}")
    h, w = int(t.shape[-2]), int(t.shape[-1])
    return t.numel() // (h * w), h, w


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
            g = gS.contiguous().to(torch.float32)
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
            if target.dtype != torch.float32:
                target = target.to(torch.float32)
            x, y = _flat(pred, "clDiceLoss input"), _flat(target, "clDiceLoss target")
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
            g = gout.contiguous().to(torch.float32)
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


def _takes_fused_head(criterion: nn.Module) -> bool:
    """Only a default-configured ``BCEWithLogitsLoss`` (no subclass) is what ``forward_loss`` computes: a weighted or sum-reduced one
    must never be replaced by the unweighted fused loss."""
    return type(criterion) is BCEWithLogitsLoss and criterion.fusable


# ---------------------------------------------------------------------------------------------------
# Accuracy / JaccardIndex / Dice from one confusion count (PLTrainer.py:62-68, 88-91)
# ---------------------------------------------------------------------------------------------------
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
            x = _flat(pred.detach(), "prediction")
            y = _flat(mask if mask.dtype == torch.float32 else mask.to(torch.float32), "mask")
            if x.numel() != y.numel():
                raise ValueError("prediction and mask differ in size")
            if self.counts is None:
                self.counts = torch.zeros(4, dtype=torch.int64, device=x.device)
            _lib.call("hpri_seg_counts", _p(x), _p(y), x.numel(), self.threshold, int(is_logits), _p(self.counts), _stream())

    def compute(self) -> Dict[str, float]:
        tp, fp, fn, tn = (float(v) for v in self.counts.tolist())     # the one host synchronisation
        return metrics_from_counts(tp, fp, fn, tn)


class _StepCounts:
    """One (TP, FP, FN, TN) row per step, kept on the device ([capacity, 4] int64, no host sync until ``rows()``)."""

    def __init__(self, threshold: float, device, capacity: int = 256):
        self.threshold = float(threshold)
        self.buf = torch.zeros((capacity, 4), dtype=torch.int64, device=device)
        self.weights: List[int] = []
        self.n = 0

    def reset(self) -> None:
        self.buf.zero_()
        self.weights.clear()
        self.n = 0

    def update(self, pred: torch.Tensor, mask: torch.Tensor) -> None:
        _require_cuda(pred, "prediction")
        with torch.cuda.device(pred.device):
            if self.n == self.buf.shape[0]:
                grown = torch.zeros((2 * self.n, 4), dtype=torch.int64, device=self.buf.device)
                grown[:self.n].copy_(self.buf)
                self.buf = grown
            x = _flat(pred.detach(), "prediction")
            y = _flat(mask if mask.dtype == torch.float32 else mask.to(torch.float32), "mask")
            if x.numel() != y.numel():
                raise ValueError("prediction and mask differ in size")
            row = self.buf[self.n]
            _lib.call("hpri_seg_counts", _p(x), _p(y), x.numel(), self.threshold, 1, _p(row), _stream())
            self.weights.append(int(pred.shape[0]))
            self.n += 1

    def rows(self) -> Tuple[List[List[float]], List[int]]:
        return [[float(v) for v in r] for r in self.buf[:self.n].tolist()], list(self.weights)


def metrics_from_counts(tp: float, fp: float, fn: float, tn: float) -> Dict[str, float]:
    total = tp + fp + fn + tn
    return {
        "acc": (tp + tn) / total if total > 0 else 0.0,
        "dice": (2 * tp) / (2 * tp + fp + fn) if (2 * tp + fp + fn) > 0 else 1e-12,
        "pos_iou": tp / (tp + fp + fn) if (tp + fp + fn) > 0 else 0.0,
        "tp": tp, "fp": fp, "fn": fn, "tn": tn,
    }


# ---------------------------------------------------------------------------------------------------
# The multi-class tail (csrc/multiclass.hip): nn.CrossEntropyLoss, argmax + confusion matrix, the metrics it reduces to
# ---------------------------------------------------------------------------------------------------
MAX_CLASSES = 64
_TARGET_KIND = {torch.float32: 0, torch.uint8: 1, torch.int64: 2}      # hpri_softmax_ce_fwd / hpri_seg_confusion: target_kind


def _class_logits(pred: torch.Tensor, what: str) -> torch.Tensor:
    _require_cuda(pred, what)
    if pred.dim() != 4:
        raise ValueError(f"{what}: need (N, K, h, w) logits, got {tuple(pred.shape)}")
    if not 2 <= int(pred.shape[1]) <= MAX_CLASSES:
        raise ValueError(f"{what}: the number of classes must lie in [2, {MAX_CLASSES}], got {int(pred.shape[1])}")
    return pred if pred.is_contiguous() else pred.contiguous()


def _class_target(target: torch.Tensor, x: torch.Tensor, what: str) -> torch.Tensor:
    """(N, h, w) or (N, 1, h, w) class indices -> contiguous fp32 / uint8 / int64 on the logits' device (other integer types
    become int64, other floating types fp32)."""
    if not target.is_cuda:
        raise RuntimeError(f"hyperpri_amd: {what} is on {target.device}; the hot path exists only as HIP kernels for MI355X "
                           "(no CPU fallback). Move the module and its inputs to a ROCm device.")
    N, _, h, w = x.shape
    if tuple(target.shape) not in ((N, h, w), (N, 1, h, w)):
        raise ValueError(f"{what}: expected a target of shape {(N, h, w)} or {(N, 1, h, w)} for logits {tuple(x.shape)}, got "
                         f"{tuple(target.shape)}")
    if target.dtype not in _TARGET_KIND:
        target = target.to(torch.float32 if target.is_floating_point() else torch.int64)
    return target if target.is_contiguous() else target.contiguous()


def _ignore_args(ignore_index: Optional[int]) -> Tuple[int, int]:
    return (0, 0) if ignore_index is None else (1, int(ignore_index))


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
            g = gout.contiguous().to(torch.float32)
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


class _StepConfusion:
    """One K*K + 1 count row per step, kept on the device like ``_StepCounts``."""

    def __init__(self, num_classes: int, ignore_index: Optional[int], device, capacity: int = 256):
        self.K, self.ignore_index = int(num_classes), ignore_index
        self.buf = torch.zeros((capacity, self.K ** 2 + 1), dtype=torch.int64, device=device)
        self.weights: List[int] = []
        self.n = 0

    def reset(self) -> None:
        self.buf.zero_()
        self.weights.clear()
        self.n = 0

    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        x = _class_logits(pred.detach(), "prediction")
        if int(x.shape[1]) != self.K:
            raise ValueError(f"SegmentationModel: built for {self.K} classes, got logits {tuple(x.shape)}")
        with torch.cuda.device(x.device):
            if self.n == self.buf.shape[0]:
                grown = torch.zeros((2 * self.n, self.buf.shape[1]), dtype=torch.int64, device=self.buf.device)
                grown[:self.n].copy_(self.buf)
                self.buf = grown
            _confusion_pass(x, _class_target(target, x, "mask"), self.ignore_index, self.buf[self.n], None)
            self.weights.append(int(pred.shape[0]))
            self.n += 1

    def rows(self) -> Tuple[List[List[int]], List[int]]:
        return self.buf[:self.n].tolist(), list(self.weights)


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
            y = _flat((target if target.dtype == torch.float32 else target.to(torch.float32)).reshape(-1), "target")
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
# optim.Adam / optim.SGD as one multi-tensor launch
# ---------------------------------------------------------------------------------------------------
def _ptr_array(ts: List[Optional[torch.Tensor]]):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (amsgrad/maximize off -- the reference uses the
    defaults, PLTrainer.py:171-174) with every parameter tensor of a group updated by ONE kernel launch.
    ``grad_scale``: optional device scalar multiplied into the gradients (e.g. 1/world_size)."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("FusedAdam: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None, grad_scale: Optional[torch.Tensor] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            for p in ps:
                _require_cuda(p, "parameter")
                if p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or not p.is_contiguous():
                    raise RuntimeError("FusedAdam: parameters and gradients must be contiguous fp32")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            by_step: Dict[int, List[torch.Tensor]] = OrderedDict()
            for p in ps:
                self.state[p]["step"] += 1
                by_step.setdefault(self.state[p]["step"], []).append(p)
            b1, b2 = group["betas"]
            for step, plist in by_step.items():
                with torch.cuda.device(plist[0].device):
                    n = (ctypes.c_longlong * len(plist))(*[p.numel() for p in plist])
                    _lib.call("hpri_adam_step", _ptr_array(plist), _ptr_array([p.grad for p in plist]),
                              _ptr_array([self.state[p]["exp_avg"] for p in plist]),
                              _ptr_array([self.state[p]["exp_avg_sq"] for p in plist]), n, len(plist),
                              float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                              int(step), _p(grad_scale), _stream())
        bump_param_epoch()      # parameters were written through raw pointers: packed-weight caches are stale
        return loss


class FusedSGD(torch.optim.Optimizer):
    """``torch.optim.SGD(params, lr, momentum, weight_decay)`` (dampening 0, no Nesterov; PLTrainer.py:176-180)."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, weight_decay: float = 0.0):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("FusedSGD: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None, grad_scale: Optional[torch.Tensor] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            mom = float(group["momentum"])
            fresh, old = [], []
            for p in ps:
                _require_cuda(p, "parameter")
                if p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or not p.is_contiguous():
                    raise RuntimeError("FusedSGD: parameters and gradients must be contiguous fp32")
                st = self.state[p]
                if mom != 0.0 and "momentum_buffer" not in st:
                    st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.preserve_format)
                    fresh.append(p)
                else:
                    old.append(p)
            for first, plist in ((1, fresh), (0, old)):
                if not plist:
                    continue
                with torch.cuda.device(plist[0].device):
                    n = (ctypes.c_longlong * len(plist))(*[p.numel() for p in plist])
                    bufs = _ptr_array([self.state[p]["momentum_buffer"] for p in plist]) if mom != 0.0 else None
                    _lib.call("hpri_sgd_step", _ptr_array(plist), _ptr_array([p.grad for p in plist]), bufs, n, len(plist),
                              float(group["lr"]), mom, float(group["weight_decay"]), first, _p(grad_scale), _stream())
        bump_param_epoch()
        return loss


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
