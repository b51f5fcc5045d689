"""Spectral detectors on the device (``csrc/detect.hip``): RX, the spectral matched filter, ACE and SAM from the band statistics.

``spectral.py`` fits the soil mean and covariance and the mean root spectrum of a cached split; this module turns a cube plus those
statistics into score maps, the classical baselines a learned segmenter is compared against:

* ``rx``   the Mahalanobis anomaly score ``q = (x - mu)^T Sr^-1 (x - mu)``;
* ``smf``  the spectral matched filter ``s^^T x^ / |s^|^2`` (``x^ = W x + b`` the whitened pixel, ``s^`` the whitened target): the target
  itself scores 1, the background mean 0.  (The unnormalised variant ``s^^T x^ / |s^|`` differs by the constant ``|s^|``.)
* ``ace``  the adaptive cosine estimator ``s^^T x^ / (|s^| |x^|)``, the cosine of the whitened pixel and the whitened target;
* ``sam``  the spectral angle mapper's cosine ``s^T x / (|s| |x|)``: ACE under the identity metric, no statistics.

The contract of the kernel (include/hyperpri_hip.h states it in full): the weight holds ``Kq`` *quadratic* rows (the whitener
``W``, ``b = -W mu``) and then ``T <= 8`` *filter* rows; per pixel

    z[k] = fmaf(W[k, cend-1], x[cend-1], ... fmaf(W[k, 0], x[0], b[k]))      q = sum_{k < Kq} z[k]^2      t[j] = z[Kq + j]

with a column extent ``cend`` per block of 16 rows (derived here from the zero pattern of the weight: a Cholesky whitener is lower
triangular and costs about half the MFMAs).  The filter row of target ``s`` is ``f = W^T s^ / |s^|`` with ``g = b . s^ / |s^|``
(ACE; ``|s^|^2`` for SMF), so ``t = f . x + g`` is the whitened inner product without a second pass over the whitened pixel.  The
epilogue writes ``t``, the cosine ``t * rsqrt(q)`` or the logit of either; nothing of size P x K is ever written.

``detect_reference`` restates the contract in fp64 numpy on the same fp32 inputs (the oracle of the GPU tests), ``whitener_reference``
restates the fit.  There is no CPU fallback: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._args import _p, _rup, _stream
from .spectral import SpectralStats, _band_input, band_statistics, class_spectra, max_channel_stride, pca_basis

SCORES = ("ace", "smf", "sam", "rx")
WHITENERS = ("cholesky", "pca", "identity")
P_LO, P_HI = 2.0 ** -24, 1.0 - 2.0 ** -24          # the clamp of the logit form


def max_targets() -> int:
    """The largest number of targets a detector holds (``hpri_band_detect_max_targets``)."""
    return int(_lib.load().hpri_band_detect_max_targets())


# ---------------------------------------------------------------------------------------------------
# The fit, fp64 on the host
# ---------------------------------------------------------------------------------------------------
def _regularised(cov, shrink: float) -> np.ndarray:
    cov = np.asarray(cov, dtype=np.float64)
    cov = 0.5 * (cov + cov.T)
    C = cov.shape[0]
    return cov + float(shrink) * np.trace(cov) / C * np.eye(C)


def _whitener(mean, cov, whitener: str, shrink: float, rank: Optional[int]) -> Tuple[np.ndarray, np.ndarray]:
    """fp64 ``(W (Kq, C), b (Kq,))`` with ``W Sr W^T = I``: ``cholesky``: ``Sr = L L^T``, ``W = L^-1`` by forward substitution (exact
    zeros above the diagonal); ``pca``: the whitened principal axes of ``pca_basis``' rule, ``eps = shrink tr(S) / C``."""
    mean = np.asarray(mean, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    C = cov.shape[0]
    if not (np.isfinite(cov).all() and np.isfinite(mean).all()):
        raise ValueError("SpectralDetector: the statistics are not finite (shrink cannot repair that)")
    if whitener == "cholesky":
        if rank is not None and int(rank) != C:
            raise ValueError("SpectralDetector: the cholesky whitener has full rank; use whitener='pca' for a rank")
        try:
            L = np.linalg.cholesky(_regularised(cov, shrink))
        except np.linalg.LinAlgError:
            raise ValueError(f"SpectralDetector: the regularised covariance is not positive definite at shrink={shrink}; raise shrink") from None
        dl = np.diag(L)
        if not dl.min() ** 2 > 1e-14 * dl.max() ** 2:        # (a semi-definite matrix can pass LAPACK on rounding alone)
            raise ValueError(f"SpectralDetector: the regularised covariance is not positive definite at shrink={shrink}; raise shrink")
        W = np.zeros((C, C))
        for i in range(C):
            W[i, i] = 1.0
            W[i, :i] = -(L[i, :i] @ W[:i, :i])
            W[i, :i + 1] /= L[i, i]
        if not np.isfinite(W).all():
            raise ValueError(f"SpectralDetector: the regularised covariance is not positive definite at shrink={shrink}; raise shrink")
    elif whitener == "pca":
        k = C if rank is None else int(rank)
        if not 1 <= k <= C:
            raise ValueError(f"SpectralDetector: rank must lie in [1, {C}], got {rank}")
        sym = 0.5 * (cov + cov.T)
        eps = float(shrink) * np.trace(sym) / C
        lam, vec = np.linalg.eigh(sym)
        order = np.argsort(lam, kind="stable")[::-1][:k]
        lam, W = lam[order], vec[:, order].T.copy()
        for i in range(k):
            j = int(np.argmax(np.abs(W[i])))
            if W[i, j] < 0:
                W[i] = -W[i]
        if not (lam + eps > 1e-14 * max(abs(lam[0]), 1e-300)).all():
            raise ValueError(f"SpectralDetector: the regularised covariance is not positive definite at shrink={shrink}; raise shrink or lower rank")
        W = W / np.sqrt(lam + eps)[:, None]
    else:
        raise ValueError(f"SpectralDetector: whitener must be 'cholesky' or 'pca', got {whitener!r}")
    return W, -(W @ mean)


def filter_rows(W, b, targets, kind: str = "ace") -> Tuple[np.ndarray, np.ndarray]:
    """fp64 filter rows ``(f (T, C), g (T,))`` of ``targets`` (T, C) under the whitener ``(W, b)``: with ``s^ = W s + b``,
    ``f = W^T s^ / n`` and ``g = b . s^ / n``, ``n = |s^|`` for ``ace`` and ``|s^|^2`` for ``smf``."""
    W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)
    S = np.asarray(targets, dtype=np.float64) @ W.T + b          # (T, Kq)
    n = np.sqrt((S * S).sum(axis=1))
    if kind == "smf":
        n = n * n
    elif kind != "ace":
        raise ValueError(f"filter_rows: kind must be 'ace' or 'smf', got {kind!r}")
    scale = np.abs(np.asarray(targets, dtype=np.float64)) @ np.abs(W).T + np.abs(b)
    if not (np.sqrt((S * S).sum(axis=1)) > 1e-10 * np.sqrt((scale * scale).sum(axis=1))).all():
        raise ValueError("SpectralDetector: a target coincides with the background mean (its whitened spectrum is zero)")
    return (S @ W) / n[:, None], (S @ b) / n


def whitener_reference(mean, cov, whitener: str = "cholesky", shrink: float = 0.0, rank: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The fit restated with library calls, fp64 ``(W, b)``: ``cholesky``: ``inv(cholesky(Sr))``; ``pca``: ``eigh`` of ``S``, rows
    ``v_i / sqrt(lambda_i + shrink tr(S) / C)`` by descending eigenvalue (signs as ``pca_basis`` fixes them).  ``b = -W mean``."""
    mean, cov = np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    C = cov.shape[0]
    if whitener == "cholesky":
        W = np.tril(np.linalg.inv(np.linalg.cholesky(_regularised(cov, shrink))))
    elif whitener == "pca":
        k = C if rank is None else int(rank)
        W32, _, lam = pca_basis(SpectralStats(2, mean, cov), k)
        lam_all, vec = np.linalg.eigh(0.5 * (cov + cov.T))
        V = vec[:, ::-1].T[:k]
        V = V * np.sign((V * W32.astype(np.float64)).sum(axis=1))[:, None]
        W = V / np.sqrt(lam_all[::-1][:k] + float(shrink) * np.trace(cov) / C)[:, None]
    else:
        raise ValueError(f"whitener_reference: whitener must be 'cholesky' or 'pca', got {whitener!r}")
    return W, -(W @ mean)


def column_extents(weight: np.ndarray, cs: int) -> np.ndarray:
    """The ``cend`` table of a padded ``(ks, cs)`` weight: per block of 16 rows the position after its last non-zero column, rounded
    up to a multiple of 8 (at least 8)."""
    w = np.asarray(weight)
    ks = w.shape[0]
    out = []
    for r0 in range(0, ks, 16):
        nz = np.nonzero(np.any(w[r0:r0 + 16] != 0, axis=0))[0]
        last = int(nz[-1]) + 1 if nz.size else 0
        out.append(min(int(cs), max(8, _rup(last, 8))))
    return np.asarray(out, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------
# The module
# ---------------------------------------------------------------------------------------------------
def _f32(a) -> torch.Tensor:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32)))


class SpectralDetector(torch.nn.Module):
    """RX, SMF, ACE and SAM score maps of a device image.  Buffers (a checkpoint carries them): ``weight`` (Kq, C) and ``bias`` (Kq,)
    the whitener, ``targets`` (T, C), the filter rows ``ace_weight`` / ``smf_weight`` (T, C) with ``ace_bias`` / ``smf_bias`` (T,),
    ``sam_weight`` (T, C) = the unit targets, and ``meta`` = (whitener code, shrink, rank).  Everything is fitted in fp64 on the host
    and rounded once to fp32.

    ``detector(x, score="ace" | "smf" | "sam" | "rx", logit=False)`` takes what ``SpectralProjection`` takes -- an image in either
    logical shape, ``(N, 1, C, h, w)`` or ``(N, C, h, w)``, or the cache's batch dict (its ``'image'``), zero-copy where the layout
    allows and through one layout pass otherwise -- and returns an fp32 ``(N, T, h, w)`` map, ``(N, 1, h, w)`` for ``rx`` (a view of
    ``(T, N, h, w)`` planes).  ``logit=True`` returns ``log(p) - log1p(-p)`` of ``p = clamp(score, 2^-24, 1 - 2^-24)`` (``rx``:
    ``p = q / (q + Kq)``): a map ``validate_net`` and ``test_net`` read as a network's logits.  No autograd: an input that requires
    grad raises.  A ``sam()`` detector has no whitener and answers ``sam`` only."""

    def __init__(self, weight, bias, targets, ace=None, smf=None, whitener: str = "cholesky", shrink: float = 0.0, rank: Optional[int] = None):
        super().__init__()
        t = _f32(targets)
        if t.dim() != 2 or t.shape[0] == 0 or t.shape[1] == 0:
            raise ValueError(f"SpectralDetector: need targets (T, C), got {tuple(t.shape)}")
        T, C = int(t.shape[0]), int(t.shape[1])
        if T > max_targets():
            raise ValueError(f"SpectralDetector: T = {T} exceeds the {max_targets()} targets the kernel holds")
        if whitener not in WHITENERS:
            raise ValueError(f"SpectralDetector: whitener must be one of {WHITENERS}, got {whitener!r}")
        if whitener == "identity":
            w, b = torch.zeros((0, C)), torch.zeros(0)
            ace = smf = (np.zeros((T, C)), np.zeros(T))
        else:
            w, b = _f32(weight), _f32(bias)
            if w.dim() != 2 or b.dim() != 1 or w.shape[0] != b.shape[0] or w.shape[0] == 0:
                raise ValueError(f"SpectralDetector: need weight (Kq, C) and bias (Kq,), got {tuple(w.shape)} and {tuple(b.shape)}")
            if w.shape[1] != C:
                raise ValueError(f"SpectralDetector: the targets have {C} bands, the whitener {int(w.shape[1])}")
            if w.shape[0] > C:
                raise ValueError(f"SpectralDetector: Kq = {int(w.shape[0])} exceeds the {C} bands")
            if ace is None or smf is None:
                W64, b64 = w.numpy().astype(np.float64), b.numpy().astype(np.float64)
                ace = filter_rows(W64, b64, t.numpy(), "ace") if ace is None else ace
                smf = filter_rows(W64, b64, t.numpy(), "smf") if smf is None else smf
        norm = np.sqrt((t.numpy().astype(np.float64) ** 2).sum(axis=1))
        if not (norm > 0).all():
            raise ValueError("SpectralDetector: a target spectrum is zero")
        bufs = {"weight": w, "bias": b, "targets": t, "ace_weight": _f32(ace[0]), "ace_bias": _f32(ace[1]), "smf_weight": _f32(smf[0]),
                "smf_bias": _f32(smf[1]), "sam_weight": _f32(t.numpy().astype(np.float64) / norm[:, None]),
                "meta": torch.tensor([float(WHITENERS.index(whitener)), float(shrink), float(-1 if rank is None else rank)], dtype=torch.float64)}
        for name, v in bufs.items():
            if not bool(torch.isfinite(v).all()):
                raise ValueError(f"SpectralDetector: {name} must be finite")
            self.register_buffer(name, v.clone())
        self._padded = {}               # kind -> (key, tensors on the device, cend), rebuilt when the buffers or cs change

    # ---- constructors -------------------------------------------------------------------------------
    @classmethod
    def from_statistics(cls, stats: SpectralStats, targets, whitener: str = "cholesky", shrink: float = 1e-4,
                        rank: Optional[int] = None) -> "SpectralDetector":
        """From a ``SpectralStats`` (``band_statistics``, or ``merge_statistics`` across ranks) and ``targets`` (T, C) or (C,).
        ``cholesky``: ``Sr = S + shrink tr(S)/C I = L L^T``, ``W = L^-1`` (lower triangular), ``b = -W mu``; ``pca``: the first ``rank``
        whitened principal axes, ``eps = shrink tr(S)/C``.  A non-finite or non-positive-definite ``Sr`` raises ``ValueError`` naming
        ``shrink``."""
        tg = np.atleast_2d(np.asarray(targets.detach().cpu() if isinstance(targets, torch.Tensor) else targets, dtype=np.float64))
        C = int(np.asarray(stats.mean).shape[0])
        if tg.ndim != 2 or tg.shape[1] != C:
            raise ValueError(f"SpectralDetector: the targets have {tg.shape[-1]} bands, the statistics {C}")
        if tg.shape[0] > max_targets():
            raise ValueError(f"SpectralDetector: T = {tg.shape[0]} exceeds the {max_targets()} targets the kernel holds")
        if not np.isfinite(tg).all():
            raise ValueError("SpectralDetector: the targets must be finite")
        W, b = _whitener(stats.mean, stats.cov, whitener, shrink, rank)
        return cls(W, b, tg, ace=filter_rows(W, b, tg, "ace"), smf=filter_rows(W, b, tg, "smf"), whitener=whitener, shrink=shrink, rank=rank)

    @classmethod
    def fit(cls, cache, targets=None, slots: Optional[Sequence[int]] = None, background: str = "background", whitener: str = "cholesky",
            shrink: float = 1e-4, rank: Optional[int] = None) -> "SpectralDetector":
        """``band_statistics(cache, slots, select=background)`` supplies mu and S; ``targets`` defaults to the foreground mean of
        ``class_spectra``.  The detector is placed on the cache's device."""
        stats = band_statistics(cache, slots, select=background)
        if targets is None:
            targets = class_spectra(cache, slots)["foreground"]["mean"]
        return cls.from_statistics(stats, targets, whitener=whitener, shrink=shrink, rank=rank).to(cache.device)

    @classmethod
    def sam(cls, targets) -> "SpectralDetector":
        """The identity metric: no statistics, ``score="sam"`` only."""
        tg = np.atleast_2d(np.asarray(targets.detach().cpu() if isinstance(targets, torch.Tensor) else targets, dtype=np.float64))
        return cls(None, None, tg, whitener="identity")

    @classmethod
    def blank(cls, bands: int, targets: int, rank: Optional[int] = None, whitener: str = "cholesky") -> "SpectralDetector":
        """A detector of the given shapes for ``load_state_dict`` to fill."""
        tg = np.ones((targets, bands))
        if whitener == "identity":
            return cls(None, None, tg, whitener="identity")
        k = bands if rank is None else int(rank)
        z = (np.zeros((targets, bands)), np.zeros(targets))
        return cls(np.eye(k, bands), np.zeros(k), tg, ace=z, smf=z, whitener=whitener)

    # ---- properties -----------------------------------------------------------------------------------
    @property
    def in_channels(self) -> int:
        return int(self.targets.shape[1])

    @property
    def num_targets(self) -> int:
        return int(self.targets.shape[0])

    @property
    def rank(self) -> int:
        return int(self.weight.shape[0])

    @property
    def whitener(self) -> str:
        return WHITENERS[int(self.meta[0])]

    def host_weights(self, kind: str, cs: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The padded ``(ks, cs)`` weight, ``(ks,)`` bias and the ``cend`` table of the launch for ``kind`` in ('ace', 'smf', 'rx')."""
        Kq, T, C = self.rank, (0 if kind == "rx" else self.num_targets), self.in_channels
        ks = _rup(Kq + T, 8)
        w = np.zeros((ks, cs), dtype=np.float32)
        b = np.zeros(ks, dtype=np.float32)
        w[:Kq, :C] = self.weight.detach().cpu().numpy()
        b[:Kq] = self.bias.detach().cpu().numpy()
        if T:
            w[Kq:Kq + T, :C] = getattr(self, kind + "_weight").detach().cpu().numpy()
            b[Kq:Kq + T] = getattr(self, kind + "_bias").detach().cpu().numpy()
        return w, b, column_extents(w[:_rup(Kq + T, 16)], cs)[:(Kq + T + 15) // 16]

    def _device_weights(self, device, cs: int, kind: str):
        names = ("sam_weight",) if kind == "sam" else ("weight", "bias") + (() if kind == "rx" else (kind + "_weight", kind + "_bias"))
        key = (str(device), cs) + tuple((getattr(self, n)._version, getattr(self, n).data_ptr()) for n in names)
        hit = self._padded.get(kind)
        if hit is None or hit[0] != key:
            if kind == "sam":
                f = torch.zeros((self.num_targets, cs), dtype=torch.float32, device=device)
                f[:, :self.in_channels] = self.sam_weight.to(device)
                hit = (key, (f,), None)
            else:
                w, b, cend = self.host_weights(kind, cs)
                hit = (key, (torch.from_numpy(w).to(device), torch.from_numpy(b).to(device)), (ctypes.c_int * len(cend))(*[int(c) for c in cend]))
            self._padded[kind] = hit
        return hit[1], hit[2]

    def forward(self, x, score: str = "ace", logit: bool = False):
        if isinstance(x, dict):
            x = x['image']
        if score not in SCORES:
            raise ValueError(f"SpectralDetector: score must be one of {SCORES}, got {score!r}")
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("hyperpri_amd: SpectralDetector needs a tensor on a ROCm device; there is no CPU fallback")
        if x.requires_grad:
            raise RuntimeError("SpectralDetector: no autograd -- the input must not require grad")
        if x.dtype != torch.float32:
            raise ValueError(f"SpectralDetector: need a float32 image, got {x.dtype}")
        if self.rank == 0 and score != "sam":
            raise ValueError(f"SpectralDetector: a sam() detector has no statistics; score={score!r} needs fit() or from_statistics()")
        five = x.dim() == 5
        if five and x.shape[1] != 1 or x.dim() not in (4, 5):
            raise ValueError(f"SpectralDetector: need an (N, 1, C, h, w) or (N, C, h, w) image, got {tuple(x.shape)}")
        t = x[:, 0] if five else x
        if getattr(x, "_hpri_zero_padded", False):
            t._hpri_zero_padded = True
        N, C, h, w = (int(s) for s in t.shape)
        if C != self.in_channels:
            raise ValueError(f"SpectralDetector: the image has {C} bands, the detector {self.in_channels}")
        if N * h * w == 0:
            raise ValueError("SpectralDetector: empty image")
        P = N * h * w
        with torch.cuda.device(x.device):
            src, cs = _band_input(t)
            if cs > max_channel_stride():
                raise ValueError(f"SpectralDetector: a channel stride of {cs} exceeds the {max_channel_stride()} the kernels take")
            tens, cend = self._device_weights(x.device, cs, score)
            lg = 2 if logit else 0
            if score == "rx":
                q = torch.empty((1, N, h, w), dtype=torch.float32, device=x.device)
                _lib.call("hpri_band_detect", _p(src), P, cs, _p(tens[0]), _p(tens[1]), int(tens[0].shape[0]), self.rank, 0, None,
                          ctypes.cast(cend, ctypes.c_void_p), lg, _p(q), None, _stream())
                return q.permute(1, 0, 2, 3)
            T = self.num_targets
            out = torch.empty((T, N, h, w), dtype=torch.float32, device=x.device)
            if score == "sam":
                _lib.call("hpri_band_detect", _p(src), P, cs, None, None, 0, 0, T, _p(tens[0]), None, 1 + lg, None, _p(out), _stream())
            else:
                _lib.call("hpri_band_detect", _p(src), P, cs, _p(tens[0]), _p(tens[1]), int(tens[0].shape[0]), self.rank, T, None,
                          ctypes.cast(cend, ctypes.c_void_p), (1 if score == "ace" else 0) + lg, None, _p(out), _stream())
        return out.permute(1, 0, 2, 3)


# ---------------------------------------------------------------------------------------------------
# The contract restated in numpy: the oracle of the GPU tests
# ---------------------------------------------------------------------------------------------------
def logit_reference(s) -> np.ndarray:
    p = np.clip(np.asarray(s, dtype=np.float64), P_LO, P_HI)
    return np.log(p) - np.log1p(-p)


def detect_reference(x, weight, bias, Kq: int, filters=None, score: int = 0, logit: bool = False):
    """``hpri_band_detect`` in fp64 numpy on (..., C) pixels: ``(q (...), scores (T, ...))``.  ``weight`` (Kq + T, C) with ``bias``
    (Kq + T,): ``z = x W^T + b``, ``q = sum z[:Kq]^2``, ``t = z[Kq:]``.  ``weight=None``: the identity metric, ``q = sum x^2`` and
    ``t = x F^T (+ bias)`` with ``filters`` = F (T, C).  ``score`` 0: t; 1: ``t / sqrt(q)``, 0 where q == 0.  ``logit``: the logit of
    the clamped score, and of ``q / (q + Kq)`` for q (the identity metric's q stays raw)."""
    x = np.asarray(x, dtype=np.float64)
    if weight is None:
        F = np.zeros((0, x.shape[-1])) if filters is None else np.asarray(filters, dtype=np.float64)
        q = (x * x).sum(axis=-1)
        t = x @ F.T + (0.0 if bias is None else np.asarray(bias, dtype=np.float64))
    else:
        z = x @ np.asarray(weight, dtype=np.float64).T + np.asarray(bias, dtype=np.float64)
        q = (z[..., :Kq] ** 2).sum(axis=-1)
        t = z[..., Kq:]
    if score == 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(q[..., None] == 0, 0.0, t / np.sqrt(q)[..., None])
    elif score != 0:
        raise ValueError("detect_reference: score must be 0 (raw) or 1 (cosine)")
    t = np.moveaxis(t, -1, 0)
    if logit:
        t = logit_reference(t)
        if weight is not None:
            q = logit_reference(q / (q + Kq))
    return q, t


__all__ = ["SpectralDetector", "detect_reference", "whitener_reference", "filter_rows", "column_extents", "logit_reference", "max_targets",
           "SCORES"]
