"""Spectral statistics and projection on the device (``csrc/spectral.hip``): the band axis of a ``CubeCache``.

Everything else in this package works on pixels and objects; this module works on the axis that makes the cubes hyperspectral.
A fold's training split sits in HBM as the cache's slots -- ``(capacity, H, W, cs)`` fp32 or fp16 beside uint8 masks -- and here it
answers, without a trip through the host:

* ``band_statistics``: count, per-band mean and the band covariance of the selected pixels (all / foreground / background);
* ``class_spectra``: the mean and standard deviation spectrum of roots and of soil;
* ``SpectralProjection``: standardised bands or the first K principal components of every batch, in the layout the networks
  consume in place.

The contract of the kernels (include/hyperpri_hip.h states it in full):

  moments   n = number of selected pixels (int64, exact) and sums[c] = sum of x[p, c] (fp64)
  gram      G[i, j] = sum over the selected pixels of d[p, i] * d[p, j],  d = fp32(x - pivot)  (fp64, exactly symmetric, pad = 0)
  project   y[p, k] = fmaf(W[k, cs-1], x[p, cs-1], ... fmaf(W[k, 0], x[p, 0], b[k]))           (fp32 MFMA: bitwise this chain)
  affine    y[p, c] = fmaf(x[p, c], s[c], t[c])

A sum spends at most ``FP32_RUN`` pixels in fp32 -- one *run*: run r of a slot covers its pixels ``[r * FP32_RUN, (r + 1) *
FP32_RUN)`` in row-major order -- and is then added into an fp64 partial accumulator; partial a owns the runs a, a + PARTS, ... of
the launch, and the partials are added in ascending order.  PARTS is a constant (2048 for the moments, 256 for the Gram matrix),
not the CU count, and there is no floating-point atomic: the same arguments give the same bits on any gfx950 part.  Inside a run
the Gram kernel adds the pixels in ascending order (an fmaf chain on ``v_mfma_f32_32x32x2_f32``); the moments kernel adds
``256 // (cs / 4)`` interleaved sub-sums.  The scratch (``hpri_band_workspace_bytes(cs)``) depends on cs alone.

``band_statistics`` takes ``pivot = fp32(mean)`` from the moments pass, so the Gram pass sums products of small differences, and
undoes the pivot's rounding on the host in fp64:  ``cov = (G - n d d^T) / (n - 1)`` with ``d = mean64 - pivot``.

``moments_reference``, ``gram_reference`` and ``project_reference`` restate the contract in fp64 numpy (no scipy) on the same
fp32 / fp16-quantised inputs; they are the oracles of the GPU tests.  There is no CPU fallback: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .cache import _DT, CubeCache
from ._args import _p, _rup, _stream

FP32_RUN = 2048             # pixels a sum spends in fp32 before it is promoted (csrc/spectral.hip: BAND_FP32_RUN; hpri_band_fp32_run)
SELECT = {"all": 0, "foreground": 1, "background": 2}


def fp32_run() -> int:
    return int(_lib.load().hpri_band_fp32_run())


def max_channel_stride() -> int:
    """The largest channel stride the family takes (``hpri_band_max_cs``: ten 32-band blocks)."""
    return int(_lib.load().hpri_band_max_cs())


def project_max_k() -> int:
    """The largest number of output channels of ``SpectralProjection`` (``hpri_band_project_max_k``)."""
    return int(_lib.load().hpri_band_project_max_k())


def workspace_bytes(cs: int) -> int:
    """Scratch the moments and Gram passes need at channel stride ``cs`` (``hpri_band_workspace_bytes``): a function of cs alone."""
    return int(_lib.load().hpri_band_workspace_bytes(int(cs)))


def _check_select(select: str) -> int:
    if select not in SELECT:
        raise ValueError(f"spectral: select must be one of {tuple(SELECT)}, got {select!r}")
    return SELECT[select]


@dataclass
class SpectralStats:
    """Count, per-band mean (C,) and band covariance (C, C, unbiased) of the selected pixels, fp64 on the host."""
    count: int
    mean: np.ndarray
    cov: np.ndarray
    select: str = "all"

    def std(self) -> np.ndarray:
        return np.sqrt(np.clip(np.diag(self.cov), 0.0, None))

    def correlation(self) -> np.ndarray:
        """``cov / (std std^T)``; a band without variance has NaN in its row and column (and 1 is not forced on the diagonal)."""
        s = self.std()
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.cov / np.outer(s, s)


# ---------------------------------------------------------------------------------------------------
# Launchers
# ---------------------------------------------------------------------------------------------------
def _slot_list(cache: CubeCache, slots: Optional[Sequence[int]]) -> list:
    if not isinstance(cache, CubeCache):
        raise TypeError("spectral: need a CubeCache")
    idx = [i for i in range(cache.capacity) if cache._filled[i]] if slots is None else [int(i) for i in slots]
    if not idx:
        raise ValueError("spectral: no slots")
    cache._check_filled(idx)
    if cache.cs > max_channel_stride():
        raise ValueError(f"spectral: a channel stride of {cache.cs} exceeds the {max_channel_stride()} the kernels take")
    return idx


class _Pass:
    """The arguments every statistics launch shares: the cache's slots, the slot table on the device, the workspace."""

    def __init__(self, cache: CubeCache, idx: Sequence[int]):
        self.cache = cache
        self.table = torch.tensor(list(idx), dtype=torch.int32).to(cache.device)
        self.nbytes = workspace_bytes(cache.cs)
        self.work = torch.empty(self.nbytes, dtype=torch.uint8, device=cache.device)
        self.head = (_p(cache._cubes), _DT[cache.store_dtype], cache.capacity, cache.H, cache.W, cache.cs, _p(cache._masks), _p(self.table),
                     len(idx))

    def moments(self, select: int, pivot: Optional[torch.Tensor] = None):
        c = self.cache
        count = torch.empty(1, dtype=torch.int64, device=c.device)
        sums = torch.empty(c.cs, dtype=torch.float64, device=c.device)
        sq = torch.empty(c.cs, dtype=torch.float64, device=c.device) if pivot is not None else None
        _lib.call("hpri_band_moments", *self.head, select, _p(pivot), _p(self.work), self.nbytes, _p(count), _p(sums), _p(sq), _stream())
        return int(count.item()), sums.cpu().numpy(), None if sq is None else sq.cpu().numpy()

    def gram(self, select: int, pivot: torch.Tensor) -> np.ndarray:
        c = self.cache
        g = torch.empty((c.cs, c.cs), dtype=torch.float64, device=c.device)
        _lib.call("hpri_band_gram", *self.head, select, _p(pivot), _p(self.work), self.nbytes, _p(g), _stream())
        return g.cpu().numpy()

    def pivot(self, values) -> torch.Tensor:
        """A (C,) vector as the kernels take it: fp32 (cs,) on the device with zero pad entries."""
        c = self.cache
        v = np.zeros(c.cs, dtype=np.float32)
        v[:c.C] = np.asarray(values, dtype=np.float64).astype(np.float32)
        return torch.from_numpy(v).to(c.device)


def band_moments(cache: CubeCache, slots: Optional[Sequence[int]] = None, select: str = "all") -> Tuple[int, np.ndarray]:
    """``(count, sums)`` of the selected pixels of ``slots`` (``hpri_band_moments``): the exact count and the fp64 per-band sums,
    (cs,) with zero pad entries."""
    code = _check_select(select)
    idx = _slot_list(cache, slots)
    with torch.cuda.device(cache.device):
        n, sums, _ = _Pass(cache, idx).moments(code)
    return n, sums


def band_gram(cache: CubeCache, pivot, slots: Optional[Sequence[int]] = None, select: str = "all") -> np.ndarray:
    """The fp64 (cs, cs) Gram matrix of ``x - pivot`` over the selected pixels (``hpri_band_gram``); ``pivot``: (C,) values, rounded
    once to fp32."""
    code = _check_select(select)
    idx = _slot_list(cache, slots)
    with torch.cuda.device(cache.device):
        ps = _Pass(cache, idx)
        return ps.gram(code, ps.pivot(pivot))


def band_statistics(cache: CubeCache, slots: Optional[Sequence[int]] = None, select: str = "all") -> SpectralStats:
    """Count, mean and covariance of the selected pixels of ``slots`` (default: every filled slot): the moments pass, then the Gram
    pass about ``pivot = fp32(mean)``, then ``cov = (G - n d d^T) / (n - 1)`` with ``d = mean64 - pivot`` in fp64 on the host.
    Two host synchronisations.  Fewer than two selected pixels raise ``ValueError``."""
    code = _check_select(select)
    idx = _slot_list(cache, slots)
    C = cache.C
    with torch.cuda.device(cache.device):
        ps = _Pass(cache, idx)
        n, sums, _ = ps.moments(code)
        if n < 2:
            raise ValueError(f"band_statistics: {n} selected pixel(s); a covariance needs two")
        mean = sums[:C] / n
        pivot = ps.pivot(mean)
        G = ps.gram(code, pivot)[:C, :C]
    d = mean - pivot.cpu().numpy()[:C].astype(np.float64)
    cov = (G - n * np.outer(d, d)) / (n - 1)
    return SpectralStats(n, mean, cov, select)


def class_spectra(cache: CubeCache, slots: Optional[Sequence[int]] = None) -> Dict[str, Dict[str, object]]:
    """Mean and standard deviation per band for the foreground (``mask != 0``) and the background: ``{"foreground": {"count",
    "mean", "std"}, "background": {...}}``, fp64 (C,) arrays.

    Per class two moments passes and no Gram pass -- the diagonal needs no matrix unit and the moments kernel is memory-bound
    already: the first gives the mean, the second (``hpri_band_moments`` with a pivot) the sums of ``d`` and ``d * d`` about
    ``pivot = fp32(mean)``, and ``var = (sum d^2 - (sum d)^2 / n) / (n - 1)``.  A class with no pixel has NaN spectra, one with a
    single pixel a NaN deviation."""
    idx = _slot_list(cache, slots)
    C = cache.C
    out: Dict[str, Dict[str, object]] = {}
    with torch.cuda.device(cache.device):
        ps = _Pass(cache, idx)
        for name in ("foreground", "background"):
            n, sums, _ = ps.moments(SELECT[name])
            mean = sums[:C] / n if n else np.full(C, np.nan)
            std = np.full(C, np.nan)
            if n >= 2:
                _, sd, sq = ps.moments(SELECT[name], ps.pivot(mean))
                std = np.sqrt(np.clip((sq[:C] - sd[:C] * sd[:C] / n) / (n - 1), 0.0, None))
            out[name] = {"count": n, "mean": mean, "std": std}
    return out


def merge_statistics(a: SpectralStats, b: SpectralStats) -> SpectralStats:
    """The statistics of the union of two disjoint pixel sets (two caches, two ranks) from their statistics: Chan's merge in fp64
    on the host.  ``mean = mean_a + delta n_b / n``, ``M = M_a + M_b + delta delta^T n_a n_b / n`` with ``delta = mean_b - mean_a``
    and ``M = cov (n - 1)``."""
    if a.mean.shape != b.mean.shape:
        raise ValueError("merge_statistics: the band counts differ")
    na, nb = int(a.count), int(b.count)
    n = na + nb
    delta = np.asarray(b.mean, dtype=np.float64) - np.asarray(a.mean, dtype=np.float64)
    mean = np.asarray(a.mean, dtype=np.float64) + delta * (nb / n)
    M = np.asarray(a.cov, dtype=np.float64) * (na - 1) + np.asarray(b.cov, dtype=np.float64) * (nb - 1) + np.outer(delta, delta) * (na * nb / n)
    return SpectralStats(n, mean, M / (n - 1), a.select if a.select == b.select else "mixed")


def pca_basis(stats: SpectralStats, k: int, whiten: bool = False, eps: float = 0.0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(W (k, C) fp32, b (k,) fp32, explained_variance (k,) fp64)`` of the first ``k`` principal components: fp64 ``eigh`` of the
    covariance on the host, eigenvalues descending.  Every component's sign is fixed so that its entry of largest magnitude is
    positive (a tie goes to the lowest index).  ``whiten`` scales row i by ``1 / sqrt(lambda_i + eps)``.  ``b = -W64 mean64``,
    rounded once to fp32, so that ``W x + b`` is the projection of the centred pixel."""
    cov = np.asarray(stats.cov, dtype=np.float64)
    C = cov.shape[0]
    if not 1 <= int(k) <= C:
        raise ValueError(f"pca_basis: k must lie in [1, {C}], got {k}")
    k = int(k)
    lam, vec = np.linalg.eigh(0.5 * (cov + cov.T))
    order = np.argsort(lam, kind="stable")[::-1][:k]
    lam, W = lam[order], vec[:, order].T.copy()
    for i in range(k):
        j = int(np.argmax(np.abs(W[i])))            # (argmax returns the lowest index of a tie)
        if W[i, j] < 0:
            W[i] = -W[i]
    if whiten:
        scale = lam + float(eps)
        if not (scale > 0).all():
            raise ValueError("pca_basis: whitening needs positive eigenvalues (raise eps or lower k)")
        W = W / np.sqrt(scale)[:, None]
    b = -(W @ np.asarray(stats.mean, dtype=np.float64))
    return W.astype(np.float32), b.astype(np.float32), lam


# ---------------------------------------------------------------------------------------------------
# Projection
# ---------------------------------------------------------------------------------------------------
def _band_input(t: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """(N, C, h, w) -> a tensor whose memory is the (N, h, w, cs) zero-padded channels-last buffer, and cs (shared by
    ``SpectralProjection`` and ``detect.SpectralDetector``: the zero-copy fast path, else one layout pass plus the pad)."""
    N, C, h, w = (int(s) for s in t.shape)
    st = t.stride()
    cs = int(st[3]) if w > 1 else (int(st[2]) if h > 1 else _rup(C, 8))
    zero_pad = cs == C or bool(getattr(t, "_hpri_zero_padded", False))
    if (st[1] == 1 and cs >= C and cs % 8 == 0 and zero_pad and (w == 1 or st[3] == cs) and (h == 1 or st[2] == w * cs)
            and (N == 1 or st[0] == h * w * cs) and t.data_ptr() % 16 == 0):
        return t, cs
    cs = _rup(C, 8)                                              # the slow path: one layout pass, then the pad
    buf = torch.zeros((N, h, w, cs), dtype=torch.float32, device=t.device)
    buf[..., :C] = t.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    return buf, cs


class SpectralProjection(torch.nn.Module):
    """``y = W x + b`` along the band axis of a device image, as a preprocessing step in front of a network.

    ``weight`` (K, C) with ``bias`` (K,): the projection kernel (``hpri_band_project``, fp32 MFMA, the weights in LDS).  ``weight``
    (C,) with ``bias`` (C,): the diagonal case ``y[c] = fmaf(x[c], weight[c], bias[c])`` (``hpri_band_affine``), K = C.

    Callable on an image in either logical shape the cache hands out, ``(N, 1, C, h, w)`` or ``(N, C, h, w)``, or on the cache's
    batch dict (``'image'`` is replaced, ``'mask'`` and ``'index'`` are left alone).  The zero-copy input is what
    ``Act.from_tensor`` takes zero-copy: channels-last strides over a buffer whose channel stride is a multiple of 8 with zeros
    above C (``CubeCache`` batches are; a plain channels-last tensor with ``C % 8 == 0`` is).  Anything else goes through one
    ``.contiguous(memory_format=channels_last)`` plus padding -- the slow path.  The output has the input's logical shape with K
    channels: a channels-last strided view of a fresh ``(N, h, w, roundup(K, 8))`` buffer (``torch.empty``, current stream) whose
    pad channels are exact zeros, marked ``_hpri_zero_padded``.  No autograd: an input that requires grad raises.  ``weight`` and
    ``bias`` are buffers, so ``state_dict()`` / ``load_state_dict()`` carry the preprocessing with a checkpoint."""

    def __init__(self, weight, bias):
        super().__init__()
        w = torch.as_tensor(np.asarray(weight.detach().cpu() if isinstance(weight, torch.Tensor) else weight, dtype=np.float32))
        b = torch.as_tensor(np.asarray(bias.detach().cpu() if isinstance(bias, torch.Tensor) else bias, dtype=np.float32))
        if w.dim() not in (1, 2) or b.dim() != 1 or b.shape[0] != w.shape[0] or w.numel() == 0:
            raise ValueError(f"SpectralProjection: need weight (K, C) or (C,) and bias of its first size, got {tuple(w.shape)} and {tuple(b.shape)}")
        if not (bool(torch.isfinite(w).all()) and bool(torch.isfinite(b).all())):
            raise ValueError("SpectralProjection: weight and bias must be finite")
        if w.dim() == 2 and w.shape[0] > project_max_k():
            raise ValueError(f"SpectralProjection: K = {w.shape[0]} exceeds the {project_max_k()} output channels the kernel holds")
        self.register_buffer("weight", w.clone())
        self.register_buffer("bias", b.clone())
        self._padded = None             # (key, weight (ks, cs), bias (ks)) on the device, rebuilt when the buffers or cs change

    @classmethod
    def pca(cls, stats: SpectralStats, k: int, whiten: bool = False, eps: float = 0.0) -> "SpectralProjection":
        W, b, lam = pca_basis(stats, k, whiten=whiten, eps=eps)
        proj = cls(W, b)
        proj.explained_variance = lam
        return proj

    @classmethod
    def standardize(cls, stats: SpectralStats, eps: float = 1e-6) -> "SpectralProjection":
        """Per band ``(x - mean) / sqrt(var + eps)`` as one fmaf: ``s = 1 / sqrt(var + eps)``, ``t = -mean s``."""
        s = 1.0 / np.sqrt(np.diag(np.asarray(stats.cov, dtype=np.float64)) + float(eps))
        return cls(s, -np.asarray(stats.mean, dtype=np.float64) * s)

    @property
    def diagonal(self) -> bool:
        return self.weight.dim() == 1

    @property
    def in_channels(self) -> int:
        return int(self.weight.shape[-1])

    @property
    def out_channels(self) -> int:
        return int(self.weight.shape[0])

    def _device_weights(self, device, cs: int):
        key = (str(device), cs, self.weight._version, self.bias._version, self.weight.data_ptr())
        if self._padded is None or self._padded[0] != key:
            K, C = self.out_channels, self.in_channels
            if self.diagonal:
                w, b = self.weight.to(device).contiguous(), self.bias.to(device).contiguous()
            else:
                ks = _rup(K, 8)
                w = torch.zeros((ks, cs), dtype=torch.float32, device=device)
                b = torch.zeros(ks, dtype=torch.float32, device=device)
                w[:K, :C] = self.weight.to(device)
                b[:K] = self.bias.to(device)
            self._padded = (key, w, b)
        return self._padded[1], self._padded[2]

    def _input(self, t: torch.Tensor) -> Tuple[torch.Tensor, int]:
        return _band_input(t)

    def forward(self, x):
        if isinstance(x, dict):
            out = dict(x)
            out['image'] = self.forward(x['image'])
            return out
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("hyperpri_amd: SpectralProjection needs a tensor on a ROCm device; there is no CPU fallback")
        if x.requires_grad:
            raise RuntimeError("SpectralProjection: no autograd -- the input must not require grad")
        if x.dtype != torch.float32:
            raise ValueError(f"SpectralProjection: need a float32 image, got {x.dtype}")
        five = x.dim() == 5
        if five and x.shape[1] != 1 or x.dim() not in (4, 5):
            raise ValueError(f"SpectralProjection: need an (N, 1, C, h, w) or (N, C, h, w) image, got {tuple(x.shape)}")
        t = x[:, 0] if five else x
        if getattr(x, "_hpri_zero_padded", False):
            t._hpri_zero_padded = True
        N, C, h, w = (int(s) for s in t.shape)
        if C != self.in_channels:
            raise ValueError(f"SpectralProjection: the image has {C} bands, the weights {self.in_channels}")
        if N * h * w == 0:
            raise ValueError("SpectralProjection: empty image")
        with torch.cuda.device(x.device):
            src, cs = self._input(t)
            if cs > max_channel_stride():
                raise ValueError(f"SpectralProjection: a channel stride of {cs} exceeds the {max_channel_stride()} the kernels take")
            wd, bd = self._device_weights(x.device, cs)
            K = self.out_channels
            ks = cs if self.diagonal else _rup(K, 8)
            y = torch.empty((N, h, w, ks), dtype=torch.float32, device=x.device)
            if self.diagonal:
                _lib.call("hpri_band_affine", _p(src), N * h * w, cs, C, _p(wd), _p(bd), _p(y), _stream())
            else:
                _lib.call("hpri_band_project", _p(src), N * h * w, cs, _p(wd), _p(bd), K, _p(y), _stream())
        out = y[..., :K].permute(0, 3, 1, 2)
        if five:
            out = out.unsqueeze(1)
        out._hpri_zero_padded = True
        return out


# ---------------------------------------------------------------------------------------------------
# The contract restated in numpy (no scipy): the oracles of the GPU tests
# ---------------------------------------------------------------------------------------------------
def _selected_pixels(cubes, masks, select: str) -> np.ndarray:
    """(n, H, W, C) cubes (or a list of (H, W, C)) -> the selected pixels as an fp64 (P, C) array, in slot-list and row-major order."""
    _check_select(select)
    x = np.asarray(cubes)
    x = x.reshape(-1, x.shape[-1]).astype(np.float64)
    if select == "all":
        return x
    if masks is None:
        raise ValueError("spectral: a selection needs the masks")
    m = np.asarray(masks).reshape(-1) != 0
    return x[m if select == "foreground" else ~m]


def moments_reference(cubes, masks=None, select: str = "all") -> Tuple[int, np.ndarray]:
    """``hpri_band_moments`` in fp64 numpy: ``(count, sums (C,))`` over the selected pixels of (n, H, W, C) ``cubes`` (fp32 or
    fp16 as the cache stores them) and (n, H, W) ``masks``."""
    x = _selected_pixels(cubes, masks, select)
    return int(x.shape[0]), x.sum(axis=0)


def gram_reference(cubes, pivot, masks=None, select: str = "all") -> np.ndarray:
    """``hpri_band_gram`` in fp64 numpy: ``D^T D`` with ``D = X - pivot`` over the selected pixels (the device rounds the
    difference once to fp32; this does not)."""
    d = _selected_pixels(cubes, masks, select) - np.asarray(pivot, dtype=np.float64)[None, :]
    return d.T @ d


def statistics_reference(cubes, masks=None, select: str = "all") -> SpectralStats:
    """``band_statistics`` in fp64 numpy: the two-pass mean and unbiased covariance of the selected pixels."""
    x = _selected_pixels(cubes, masks, select)
    n = int(x.shape[0])
    if n < 2:
        raise ValueError(f"statistics_reference: {n} selected pixel(s); a covariance needs two")
    mean = x.mean(axis=0)
    d = x - mean
    return SpectralStats(n, mean, d.T @ d / (n - 1), select)


def project_reference(x, weight, bias) -> np.ndarray:
    """``hpri_band_project`` / ``hpri_band_affine`` in fp64 numpy on (..., C) pixels: ``x W^T + b`` for a (K, C) weight,
    ``x * w + b`` for a (C,) weight."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(weight, dtype=np.float64)
    b = np.asarray(bias, dtype=np.float64)
    return x * w + b if w.ndim == 1 else x @ w.T + b


__all__ = ["FP32_RUN", "SELECT", "SpectralStats", "SpectralProjection", "band_moments", "band_gram", "band_statistics", "class_spectra",
           "merge_statistics", "pca_basis", "moments_reference", "gram_reference", "statistics_reference", "project_reference",
           "workspace_bytes", "project_max_k", "max_channel_stride", "fp32_run"]
