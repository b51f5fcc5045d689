"""The argument rules the tail wrappers share (losses, metrics, optimizers, evaluation, components, distances, spectra, cache), each
stated once.  The leaf of the tail: it imports none of those modules, and it is where they take ``_p``, ``_stream``, ``_rup`` and
``_require_cuda`` from (defined in ``engine.py``, whose item queues ``_stream`` registers).  DESIGN.md lists the rules."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .engine import _p, _require_cuda, _rup, _stream  # noqa: F401  (re-exported)

MAX_CLASSES = 64
_TARGET_KIND = {torch.float32: 0, torch.uint8: 1, torch.int64: 2}      # hpri_softmax_ce_fwd / hpri_seg_confusion: target_kind


def _require_placed(t: torch.Tensor, what: str, feature: str = "the hot path exists",
                    advice: str = "Move the module and its inputs to a ROCm device.") -> None:
    """``_require_cuda`` for tensors that may be integer: only the placement is checked."""
    if not t.is_cuda:
        raise RuntimeError(f"hyperpri_amd: {what} is on {t.device}; {feature} only as HIP kernels for MI355X (no CPU fallback). {advice}")


def _require_device(t: torch.Tensor, what: str) -> None:
    """The placement check in the words of ``components.py`` and ``distance.py``."""
    _require_placed(t, what, "connected components exist", "Move the tensors to a ROCm device.")


def _flat(t: torch.Tensor, what: str) -> torch.Tensor:
    _require_cuda(t, what)
    return t if t.is_contiguous() else t.contiguous()


def _as_f32(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself when it is fp32 already (nothing is allocated), else a converted copy."""
    return t if t.dtype == torch.float32 else t.to(torch.float32)


def _grad_f32(gout: torch.Tensor) -> torch.Tensor:
    """An upstream gradient as the backward kernels read it: contiguous fp32."""
    return gout.contiguous().to(torch.float32)


def _scalar(v, what: str) -> float:
    """A float, or a one-element tensor read once (at construction, never inside a step)."""
    if isinstance(v, torch.Tensor):
        if v.numel() != 1:
            raise ValueError(f"{what} must be a float or a one-element tensor, got shape {tuple(v.shape)}")
        return float(v.detach().reshape(()).cpu())
    return float(v)


def _planes(t: torch.Tensor, who: str) -> Tuple[int, int, int]:
    """(N, h, w) of a (N, ..., h, w) tensor read as planes."""
    if t.dtype != torch.float32:
        raise ValueError(f"{who}: need float32, got {t.dtype}")
    if t.dim() < 2 or t.numel() == 0:
        raise ValueError(f"{who}: need (N, ..., h, w) planes with at least one element, got {tuple(t.shape)}")
    h, w = int(t.shape[-2]), int(t.shape[-1])
    return t.numel() // (h * w), h, w


def _map3d(t: torch.Tensor, who: str) -> torch.Tensor:
    """(h, w), (N, h, w) or (N, 1, h, w) -> contiguous (N, h, w)."""
    if t.dim() == 2:
        t = t.unsqueeze(0)
    elif t.dim() == 4 and t.shape[1] == 1:
        t = t.reshape(t.shape[0], t.shape[2], t.shape[3])
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{who}: need a non-empty (N, h, w), (N, 1, h, w) or (h, w) map, got {tuple(t.shape)}")
    if t.numel() >= 2 ** 31:
        raise ValueError(f"{who}: N*h*w must be below 2^31, got {t.numel()}")
    return t.contiguous()


def _image4d(image: torch.Tensor, who: str) -> torch.Tensor:
    if image.dim() == 5:                # CubeNET cube (N,1,C,h,w) -> (N,C,h,w), as autograd._as4d
        if image.shape[1] != 1:
            raise RuntimeError("hyperpri_amd: 5-D input must be (N,1,D,H,W)")
        image = image.reshape(image.shape[0], image.shape[2], image.shape[3], image.shape[4])
    if image.dim() != 4:
        raise ValueError(f"{who}: need a (N,C,h,w) image or a (N,1,C,h,w) cube, got {tuple(image.shape)}")
    return image


def _as_images(binary) -> Tuple[np.ndarray, bool]:
    """A (h, w) or (N, h, w) map of the numpy restatements -> (boolean (N, h, w), whether it was a single image)."""
    a = np.asarray(binary) != 0
    if a.ndim == 2:
        return a[None], True
    if a.ndim != 3:
        raise ValueError(f"components: need a (h, w) or (N, h, w) map, got {a.shape}")
    return a, False


def _decision_input(pred: torch.Tensor, threshold: Optional[float], who: str) -> Tuple[torch.Tensor, int, float]:
    """A binary decision map as the kernels read it: (contiguous (N, h, w) tensor, kind, threshold) -- fp32 predictions with a
    threshold (kind 0), or a uint8 / bool map without one (kind 1)."""
    if threshold is None:
        _require_device(pred, f"{who} map")
        if pred.dtype == torch.bool:
            pred = pred.view(torch.uint8)
        if pred.dtype != torch.uint8:
            raise ValueError(f"{who}: without a threshold the input must be a uint8 or bool map, got {pred.dtype}")
        return _map3d(pred, who), 1, 0.0
    _require_cuda(pred, f"{who} prediction")
    return _map3d(pred.detach(), who), 0, float(threshold)


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
    _require_placed(target, what)
    N, _, h, w = x.shape
    if tuple(target.shape) not in ((N, h, w), (N, 1, h, w)):
        raise ValueError(f"{what}: expected a target of shape {(N, h, w)} or {(N, 1, h, w)} for logits {tuple(x.shape)}, got "
                         f"{tuple(target.shape)}")
    if target.dtype not in _TARGET_KIND:
        target = target.to(torch.float32 if target.is_floating_point() else torch.int64)
    return target if target.is_contiguous() else target.contiguous()


def _ignore_args(ignore_index: Optional[int]) -> Tuple[int, int]:
    return (0, 0) if ignore_index is None else (1, int(ignore_index))


FILTER_DOMAINS = ("linear", "prob")


def _int_arg(v, lo: int, hi: int, what: str, who: str) -> int:
    """An integer parameter of a windowed filter (a radius, a number of iterations) in [lo, hi]; a bool is none."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError(f"{who}: {what} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def _weight_arg(v, what: str, who: str) -> float:
    """A weight as the fp32 value a launch receives: non-negative and finite."""
    x = float(np.float32(_scalar(v, f"{who}: {what}")))
    if not (x >= 0.0 and np.isfinite(x)):
        raise ValueError(f"{who}: {what} must be non-negative and finite as an fp32 value, got {v!r}")
    return x


def _guide_frame(guide: torch.Tensor, max_guides: int, who: str, min_guides: int = 1) -> torch.Tensor:
    """A guide (N, K, h, w) or (N, 1, K, h, w) with K in [min_guides, max_guides] -> its 4-d view."""
    g = guide
    if g.dim() == 5:
        if g.shape[1] != 1:
            raise ValueError(f"{who}: a 5-d guide must be (N, 1, K, h, w), got {tuple(g.shape)}")
        g = g[:, 0]
    if g.dim() != 4 or not min_guides <= int(g.shape[1]) <= max_guides:
        raise ValueError(f"{who}: need a guide (N, K, h, w) or (N, 1, K, h, w) with K in [{min_guides}, {max_guides}], got {tuple(guide.shape)}")
    return g


def _filter_args(radius, eps, domain, max_radius: int, who: str) -> Tuple[int, float, int]:
    """The parameters of an edge-preserving filter as its kernels take them: (radius in [1, max_radius], eps as the fp32 value the
    launch receives -- positive and finite --, the code of ``domain``)."""
    _int_arg(radius, 1, max_radius, "radius", who)
    e = float(np.float32(_scalar(eps, f"{who}: eps")))
    if not (e > 0.0 and np.isfinite(e)):
        raise ValueError(f"{who}: eps must be positive and finite as an fp32 value, got {eps!r}")
    if domain not in FILTER_DOMAINS:
        raise ValueError(f"{who}: domain must be one of {FILTER_DOMAINS}, got {domain!r}")
    return int(radius), e, FILTER_DOMAINS.index(domain)
