"""Test-time augmentation: the eight dihedral views of a frame, the ``TTA`` settings and the restatement of the merge.

Host-side and pure Python (numpy, torch only for tensors handed in): the device pieces are ``CubeCache.view`` /
``CubeCache.epoch_views`` (the views, made by the gathers that read the cube anyway), ``csrc/tta.hip`` (``hpri_tta_merge``: every
view's logits back in the original frame and merged, one launch per batch) and ``evaluate.predict_split(tta=...)`` /
``evaluate.evaluate_multiclass(tta=...)``:

    tta  = TTA()                                                  # id, flip_w, flip_h, rot180; mean probability
    pred = predict_split(net, cache.epoch_views(2, tta.views), tta=tta)
    val  = validate_net(pred)                                     # pred.logits are still logits

A view of an ``(h, w)`` frame ``a``, its integer code (the one ``hpri_tta_merge`` takes) and its index map:

    0 id              v[i, j] = a[i, j]                     4 rot90          v[i, j] = a[j, w-1-i]      (w, h)
    1 flip_h          v[i, j] = a[h-1-i, j]                 5 rot270         v[i, j] = a[h-1-j, i]      (w, h)
    2 flip_w          v[i, j] = a[i, w-1-j]                 6 transpose      v[i, j] = a[j, i]          (w, h)
    3 rot180          v[i, j] = a[h-1-i, w-1-j]             7 antitranspose  v[i, j] = a[h-1-j, w-1-i]  (w, h)

``rot90`` is ``torch.rot90(x, 1, (-2, -1))`` (= ``numpy.rot90``: a quarter turn counter-clockwise), ``rot270`` three of them.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

VIEW_NAMES: Tuple[str, ...] = ("id", "flip_h", "flip_w", "rot180", "rot90", "rot270", "transpose", "antitranspose")
VIEW_CODES = {name: code for code, name in enumerate(VIEW_NAMES)}
_INVERSE = {"id": "id", "flip_h": "flip_h", "flip_w": "flip_w", "rot180": "rot180", "rot90": "rot270", "rot270": "rot90",
            "transpose": "transpose", "antitranspose": "antitranspose"}
FLT_MIN = float(np.finfo(np.float32).tiny)


def _check(name: str) -> str:
    if name not in VIEW_CODES:
        raise ValueError(f"unknown view {name!r}; the views are {', '.join(VIEW_NAMES)}")
    return name


def view_code(name: str) -> int:
    return VIEW_CODES[_check(name)]


def view_transposes(name: str) -> bool:
    """True for the four views that turn an (h, w) frame into a (w, h) one."""
    return VIEW_CODES[_check(name)] >= 4


def view_shape(name: str, h: int, w: int) -> Tuple[int, int]:
    return (w, h) if view_transposes(name) else (h, w)


def forward_index(name: str, h: int, w: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(rows, cols)``, int64 arrays of the view's shape: ``view[i, j] = frame[rows[i, j], cols[i, j]]``."""
    hv, wv = view_shape(name, h, w)
    i, j = np.meshgrid(np.arange(hv, dtype=np.int64), np.arange(wv, dtype=np.int64), indexing="ij")
    return {"id": (i, j), "flip_h": (h - 1 - i, j), "flip_w": (i, w - 1 - j), "rot180": (h - 1 - i, w - 1 - j),
            "rot90": (j, w - 1 - i), "rot270": (h - 1 - j, i), "transpose": (j, i), "antitranspose": (h - 1 - j, w - 1 - i)}[name]


def inverse_index(name: str, h: int, w: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(rows, cols)``, int64 arrays of shape (h, w): ``frame[y, x] = view[rows[y, x], cols[y, x]]`` -- where the view keeps
    frame pixel (y, x)."""
    _check(name)
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    return {"id": (y, x), "flip_h": (h - 1 - y, x), "flip_w": (y, w - 1 - x), "rot180": (h - 1 - y, w - 1 - x),
            "rot90": (w - 1 - x, y), "rot270": (x, h - 1 - y), "transpose": (x, y), "antitranspose": (w - 1 - x, h - 1 - y)}[name]


def apply_view(array, name: str):
    """The view ``name`` of a numpy array or a torch tensor over its last two axes (a strided view where the library makes
    one; call ``.contiguous()`` / ``numpy.ascontiguousarray`` for a dense copy)."""
    _check(name)
    if isinstance(array, np.ndarray):
        if array.ndim < 2:
            raise ValueError("apply_view: need at least two axes")
        return {"id": lambda a: a, "flip_h": lambda a: np.flip(a, -2), "flip_w": lambda a: np.flip(a, -1),
                "rot180": lambda a: np.flip(a, (-2, -1)), "rot90": lambda a: np.rot90(a, 1, (-2, -1)),
                "rot270": lambda a: np.rot90(a, 3, (-2, -1)), "transpose": lambda a: np.swapaxes(a, -2, -1),
                "antitranspose": lambda a: np.swapaxes(np.flip(a, (-2, -1)), -2, -1)}[name](array)
    import torch
    if array.dim() < 2:
        raise ValueError("apply_view: need at least two axes")
    return {"id": lambda a: a, "flip_h": lambda a: a.flip(-2), "flip_w": lambda a: a.flip(-1), "rot180": lambda a: a.flip(-2, -1),
            "rot90": lambda a: torch.rot90(a, 1, (-2, -1)), "rot270": lambda a: torch.rot90(a, 3, (-2, -1)),
            "transpose": lambda a: a.transpose(-2, -1), "antitranspose": lambda a: a.flip(-2, -1).transpose(-2, -1)}[name](array)


def invert_view(array, name: str):
    """Undo ``apply_view(., name)``: ``invert_view(apply_view(a, v), v)`` equals ``a``."""
    return apply_view(array, _INVERSE[_check(name)])


@dataclass(frozen=True)
class TTA:
    """What ``predict_split`` / ``evaluate_multiclass`` do with ``tta=``: the network sees every view in ``views`` (1 to 8 of
    ``VIEW_NAMES``, no duplicates; the default four need no transposed frame), and the views' logits are merged -- ``"prob"``: the
    logit (binary) or the log (multi-class) of the mean probability, ``"logit"``: the mean of the logits.  ``spread`` also keeps
    the per-pixel disagreement of the views (``hpri_tta_merge``).  Needs no device."""
    views: Tuple[str, ...] = ("id", "flip_w", "flip_h", "rot180")
    merge: str = "prob"
    spread: bool = False

    def __post_init__(self):
        views = (self.views,) if isinstance(self.views, str) else tuple(self.views)
        if not 1 <= len(views) <= len(VIEW_NAMES):
            raise ValueError(f"TTA: need 1 to {len(VIEW_NAMES)} views, got {len(views)}")
        for v in views:
            if v not in VIEW_CODES:
                raise ValueError(f"TTA: unknown view {v!r}; the views are {', '.join(VIEW_NAMES)}")
        if len(set(views)) != len(views):
            raise ValueError(f"TTA: a view is listed twice in {views!r}")
        if self.merge not in ("prob", "logit"):
            raise ValueError(f"TTA: merge must be 'prob' or 'logit', got {self.merge!r}")
        object.__setattr__(self, "views", views)
        object.__setattr__(self, "spread", bool(self.spread))

    @property
    def codes(self) -> List[int]:
        return [VIEW_CODES[v] for v in self.views]

    @property
    def mode(self) -> int:
        """``hpri_tta_merge``'s mode: 0 logit, 1 prob."""
        return 1 if self.merge == "prob" else 0


def tta_merge_reference(view_logits: Sequence[np.ndarray], views: Sequence[str], merge: str = "prob", spread: bool = False,
                        dtype=np.float64) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """The contract of ``hpri_tta_merge`` in numpy: ``view_logits[v]`` is the (N, K, hv, wv) output of the network for view
    ``views[v]``; returns ``(out, spread)`` with ``out`` (N, K, h, w) and ``spread`` (N, h, w) or None, both of ``dtype``.

    * ``"logit"``: ``(((s_0 + s_1) + ...) + s_{V-1}) * (1 / V)`` -- a loop in view order in ``dtype``, the quotient ``1 / V`` formed
      in ``dtype`` too: with ``dtype=numpy.float32`` this is the kernel bit for bit;
    * ``"prob"``, K = 1: ``log(max(mean p, FLT_MIN)) - log(max(mean q, FLT_MIN))`` with ``p = 1 / (1 + exp(-s))`` and
      ``q = 1 / (1 + exp(s))``; K > 1: ``log(max(mean softmax(s), FLT_MIN))``;
    * ``spread``, K = 1: the population standard deviation of ``p`` over the views; K > 1: the fraction of views whose argmax
      (lowest index on ties) differs from the argmax of ``out``."""
    if merge not in ("prob", "logit"):
        raise ValueError(f"tta_merge_reference: merge must be 'prob' or 'logit', got {merge!r}")
    V = len(views)
    if not 1 <= V <= len(VIEW_NAMES) or len(view_logits) != V:
        raise ValueError("tta_merge_reference: need 1 to 8 views and one array per view")
    s = [np.ascontiguousarray(invert_view(np.asarray(a), v)).astype(dtype) for a, v in zip(view_logits, views)]
    if any(a.ndim != 4 or a.shape != s[0].shape for a in s):
        raise ValueError("tta_merge_reference: every view must be (N, K, hv, wv) and map back to the same frame")
    K = s[0].shape[1]
    inv = dtype(1) / dtype(V)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        def mean(parts):
            acc = parts[0].copy()
            for a in parts[1:]:
                acc = acc + a
            return acc * inv
        if K == 1:
            p = [1 / (1 + np.exp(-a)) for a in s]
        if merge == "logit":
            out = mean(s)
        elif K == 1:
            out = np.log(np.maximum(mean(p), FLT_MIN)) - np.log(np.maximum(mean([1 / (1 + np.exp(a)) for a in s]), FLT_MIN))
        else:
            soft = []
            for a in s:
                e = np.exp(a - a.max(axis=1, keepdims=True))
                soft.append(e * (1 / e.sum(axis=1, keepdims=True)))
            out = np.log(np.maximum(mean(soft), FLT_MIN))
        sp = None
        if spread and K == 1:
            pm = mean(p)
            sp = np.sqrt(mean([(a - pm) ** 2 for a in p]))[:, 0]
        elif spread:
            best = out.argmax(axis=1)
            sp = (sum((a.argmax(axis=1) != best).astype(np.int64) for a in s).astype(dtype) / dtype(V))
    return out.astype(dtype, copy=False), None if sp is None else sp.astype(dtype, copy=False)
