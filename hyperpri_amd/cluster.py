"""Spectral k-means on the device (``csrc/cluster.hip``): Lloyd's algorithm on the pixels' spectra of a cached split, label maps.

``spectral.py`` fits the statistics of a split and ``detect.py`` the supervised baselines; this module is the unsupervised one: do
roots and soil separate without labels, which soil types does a rhizotron hold, pseudo-labels.  The split stays in HBM.

The contract of the kernels (include/hyperpri_hip.h states it in full), a generic argmin of K affine scores:

    d[c]  = fp32(x[c] - pivot[c])                                    rounded once, as the Gram pass rounds it
    z[k]  = fmaf(W[k, cs-1], d[cs-1], ... fmaf(W[k, 0], d[0], b[k]))  the chain of ``hpri_band_project``, fp32 MFMA
    label = the lowest k < K with z[k] == min z,    zmin = z[label]

For centroids ``g_k`` (relative to the pivot) this module passes ``W[k] = -g_k`` and ``b[k] = fp32(|g_k|^2 / 2)`` (computed in fp64), so
``2 z[k] + |d|^2`` is the squared distance to centroid k.  ``hpri_band_assign`` labels a batch (labels, ``zmin``, the squared distance
``max(0, 2 zmin + |d|^2)`` or a looked-up value per label); ``hpri_band_cluster_sums`` is one fitting pass over the cache's slots:
per cluster the exact count and the fp64 sum of ``d``, plus the sums of ``zmin`` and ``|d|^2``, by the family's summation rule (fp32
inside a run of ``FP32_RUN`` pixels -- a chain over the run's pixels in ascending order --, fp64 partials in a fixed order, no
floating-point atomic).  The labels inside that pass are bit for bit those of ``hpri_band_assign``.

``assign_reference``, ``cluster_step_reference`` and ``kmeans_reference`` restate the contract and the Lloyd loop in fp64 numpy on the
same fp32 inputs (no scipy, no sklearn); they are the oracles of the GPU tests.  No autograd, no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .cache import _DT, CubeCache
from ._args import _p, _rup, _stream
from .detect import P_HI, P_LO
from .spectral import _band_input, _check_select, _selected_pixels, _slot_list, band_moments, max_channel_stride

MAX_K = 64                  # hpri_band_cluster_max_k
SAMPLE = 4096               # pixels the initialisation reads from the cache
INITS = ("k-means++", "sample")
OUTPUTS = ("labels", "distance", "score", "logit")
U = 2.0 ** -24


def max_k() -> int:
    """The largest number of clusters the kernels take (``hpri_band_cluster_max_k``)."""
    return int(_lib.load().hpri_band_cluster_max_k())


def cluster_parts() -> int:
    """The number of fp64 partial accumulators of the fitting pass (``hpri_band_cluster_parts``): a constant."""
    return int(_lib.load().hpri_band_cluster_parts())


def workspace_bytes(cs: int, k: int) -> int:
    """Scratch of the fitting pass (``hpri_band_cluster_workspace_bytes``): a function of ``cs`` and ``k`` alone."""
    return int(_lib.load().hpri_band_cluster_workspace_bytes(int(cs), int(k)))


@dataclass
class ClusterSums:
    """What one fitting pass returns: per cluster the count and the fp64 sum of ``d = fp32(x - pivot)`` over its pixels, the sum of
    the winning scores and the sum of ``|d|^2`` over all selected pixels."""
    counts: np.ndarray          # (K,) int64
    sums: np.ndarray            # (K, C) fp64
    score_sum: float
    sq_sum: float

    @property
    def inertia(self) -> float:
        """The sum of squared distances to the nearest centroid: ``sum |d|^2 + 2 sum zmin``."""
        return self.sq_sum + 2.0 * self.score_sum


def merge_cluster_sums(a: ClusterSums, b: ClusterSums) -> ClusterSums:
    """The sums of the union of two disjoint pixel sets (two caches, two ranks) under the same pivot and centres."""
    if a.sums.shape != b.sums.shape or a.counts.shape != b.counts.shape:
        raise ValueError("merge_cluster_sums: the shapes differ")
    return ClusterSums(a.counts + b.counts, a.sums + b.sums, a.score_sum + b.score_sum, a.sq_sum + b.sq_sum)


# ---------------------------------------------------------------------------------------------------
# Host-side operands
# ---------------------------------------------------------------------------------------------------
def _centers32(centers, bands: Optional[int] = None, who: str = "cluster") -> np.ndarray:
    c = centers.detach().cpu().numpy() if isinstance(centers, torch.Tensor) else np.asarray(centers)
    if c.ndim != 2 or c.shape[0] == 0 or c.shape[1] == 0:
        raise ValueError(f"{who}: need centers (K, C), got {tuple(c.shape)}")
    if c.shape[0] > MAX_K:
        raise ValueError(f"{who}: K = {c.shape[0]} exceeds the {MAX_K} clusters the kernels take")
    if bands is not None and c.shape[1] != bands:
        raise ValueError(f"{who}: the centers have {c.shape[1]} bands, the data {bands}")
    c = np.ascontiguousarray(c.astype(np.float64).astype(np.float32))
    if not np.isfinite(c).all():
        raise ValueError(f"{who}: the centers must be finite")
    return c


def _vector32(v, bands: int, who: str) -> np.ndarray:
    v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    if v.shape != (bands,):
        raise ValueError(f"{who}: need a pivot ({bands},), got {tuple(v.shape)}")
    v = v.astype(np.float64).astype(np.float32)
    if not np.isfinite(v).all():
        raise ValueError(f"{who}: the pivot must be finite")
    return v


def score_rows(centers) -> Tuple[np.ndarray, np.ndarray]:
    """The kernel's operands of (K, C) fp32 centres (centroids minus pivot): ``(W, b)`` with ``W = -centers`` (fp32, exact) and
    ``b = fp32(|center|^2 / 2)``, the square computed in fp64."""
    c = _centers32(centers)
    return -c, (0.5 * (c.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)


def _padded_rows(centers32: np.ndarray, cs: int) -> Tuple[np.ndarray, np.ndarray]:
    K, C = centers32.shape
    ks = _rup(K, 8)
    w = np.zeros((ks, cs), dtype=np.float32)
    b = np.zeros(ks, dtype=np.float32)
    w[:K, :C], b[:K] = score_rows(centers32)
    return w, b


# ---------------------------------------------------------------------------------------------------
# The fitting pass
# ---------------------------------------------------------------------------------------------------
class _FitPass:
    """What the passes of one fit share: the slot table, the pivot and the workspace on the device, the packed result buffer (one
    copy to the host, one synchronisation per pass)."""

    def __init__(self, cache: CubeCache, idx: Sequence[int], pivot32: np.ndarray, k: int):
        self.cache, self.k = cache, int(k)
        dev, cs = cache.device, cache.cs
        self.table = torch.tensor(list(idx), dtype=torch.int32).to(dev)
        pv = np.zeros(cs, dtype=np.float32)
        pv[:cache.C] = pivot32
        self.pivot = torch.from_numpy(pv).to(dev)
        self.nbytes = workspace_bytes(cs, k)
        self.work = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.out = torch.empty(k + k * cs + 2, dtype=torch.float64, device=dev)        # counts (as int64) | sums | totals
        self.head = (_p(cache._cubes), _DT[cache.store_dtype], cache.capacity, cache.H, cache.W, cs, _p(cache._masks), _p(self.table), len(idx))

    def step(self, centers32: np.ndarray, select: int) -> ClusterSums:
        c, k = self.cache, self.k
        w, b = _padded_rows(centers32, c.cs)
        wd, bd = torch.from_numpy(w).to(c.device), torch.from_numpy(b).to(c.device)
        base = self.out.data_ptr()
        _lib.call("hpri_band_cluster_sums", *self.head, select, _p(self.pivot), _p(wd), _p(bd), k, _p(self.work), self.nbytes, base,
                  base + 8 * k, base + 8 * (k + k * c.cs), _stream())
        host = self.out.cpu().numpy()
        sums = host[k:k + k * c.cs].reshape(k, c.cs)[:, :c.C].copy()
        return ClusterSums(host[:k].view(np.int64).copy(), sums, float(host[-2]), float(host[-1]))


def cluster_step(cache: CubeCache, pivot, centers, slots: Optional[Sequence[int]] = None, select: str = "all") -> ClusterSums:
    """One fitting pass (``hpri_band_cluster_sums``) over the selected pixels of ``slots`` (default: every filled slot).  ``pivot``
    (C,) and ``centers`` (K, C) = *centroids minus pivot*, both as fp32 values; the operands are ``score_rows(centers)``.  One host
    synchronisation."""
    code = _check_select(select)
    if not isinstance(cache, CubeCache):
        raise TypeError("cluster: need a CubeCache")
    c32 = _centers32(centers, cache.C, "cluster_step")
    pv = _vector32(pivot, cache.C, "cluster_step")
    idx = _slot_list(cache, slots)
    with torch.cuda.device(cache.device):
        return _FitPass(cache, idx, pv, c32.shape[0]).step(c32, code)


# ---------------------------------------------------------------------------------------------------
# Initialisation and the Lloyd loop (shared by the fit and its restatement)
# ---------------------------------------------------------------------------------------------------
def init_centers(sample, k: int, init: str = "k-means++", seed: int = 0) -> np.ndarray:
    """``k`` starting centres from an (m, C) fp64 ``sample`` of pixels: ``"k-means++"`` -- the first uniformly, each next with
    probability proportional to the squared distance to the nearest centre chosen so far (D^2 sampling, fp64) --, or ``"sample"``:
    k distinct rows.  Deterministic for a given seed (``numpy.random.default_rng(seed)``)."""
    x = np.asarray(sample, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < int(k) or int(k) < 1:
        raise ValueError(f"init_centers: need at least k = {k} sample pixels (m, C), got {tuple(x.shape)}")
    rng = np.random.default_rng(int(seed))
    m = x.shape[0]
    if init == "sample":
        return x[np.sort(rng.choice(m, size=int(k), replace=False))].copy()
    if init != "k-means++":
        raise ValueError(f"init_centers: init must be one of {INITS} or a (k, C) array, got {init!r}")
    picks = [int(rng.integers(m))]
    dist = ((x - x[picks[0]]) ** 2).sum(axis=1)
    for _ in range(1, int(k)):
        tot = float(dist.sum())
        if tot > 0:
            j = min(int(np.searchsorted(np.cumsum(dist), rng.random() * tot, side="right")), m - 1)
        else:                                               # every pixel coincides with a centre: any row
            j = int(rng.integers(m))
        picks.append(j)
        dist = np.minimum(dist, ((x - x[j]) ** 2).sum(axis=1))
    return x[picks].copy()


def _lloyd(step: Callable[[np.ndarray], ClusterSums], centers32: np.ndarray, bands: int, max_iter: int, tol: float):
    """Lloyd's loop on (K, C) fp32 centres: per iteration one ``step``; ``center_k = sums_k / counts_k`` in fp64, rounded once to
    fp32 (an empty cluster keeps its centre); stop when ``sum_k |delta center_k|^2 <= tol * sq_sum / (n C)`` -- the mean band
    variance about the pivot, from the first pass -- or at ``max_iter``; a last pass fixes counts and inertia.  Returns
    ``(centers, final ClusterSums, n_iter, converged)``."""
    if int(max_iter) < 1:
        raise ValueError(f"k-means: max_iter must be at least 1, got {max_iter}")
    centers = centers32.copy()
    scale, converged, n_iter = None, False, 0
    for it in range(1, int(max_iter) + 1):
        s = step(centers)
        n = int(s.counts.sum())
        if n == 0:
            raise ValueError("k-means: no selected pixel")
        if scale is None:
            scale = s.sq_sum / (n * bands)
        new = centers.copy()
        nz = s.counts > 0
        new[nz] = (s.sums[nz] / s.counts[nz, None]).astype(np.float32)
        shift = float(((new.astype(np.float64) - centers.astype(np.float64)) ** 2).sum())
        centers, n_iter = new, it
        if shift <= float(tol) * scale:
            converged = True
            break
    return centers, step(centers), n_iter, converged


def _sample_pixels(cache: CubeCache, idx: Sequence[int], select: int, seed: int, limit: int = SAMPLE) -> np.ndarray:
    """At most ``limit`` selected pixels of the listed slots as an fp64 (m, C) array, chosen by ``default_rng(seed)`` without
    replacement and read from the cache in ascending position."""
    P = cache.H * cache.W
    rng = np.random.default_rng(int(seed))
    slot = torch.tensor(list(idx), dtype=torch.int64, device=cache.device)
    if select == 0:
        total = len(idx) * P
        pick = torch.from_numpy(np.sort(rng.choice(total, size=min(limit, total), replace=False)).astype(np.int64)).to(cache.device)
    else:
        m = cache._masks.reshape(cache.capacity, P)[slot].reshape(-1)
        sel = torch.nonzero((m != 0) == (select == 1)).reshape(-1)
        if sel.numel() == 0:
            raise ValueError("SpectralKMeans: no selected pixel")
        pick = sel[torch.from_numpy(np.sort(rng.choice(int(sel.numel()), size=min(limit, int(sel.numel())), replace=False)).astype(np.int64)).to(cache.device)]
    rows = cache._cubes.reshape(cache.capacity * P, cache.cs)[slot[pick // P] * P + pick % P]
    return rows[:, :cache.C].to(torch.float64).cpu().numpy()


# ---------------------------------------------------------------------------------------------------
# The module
# ---------------------------------------------------------------------------------------------------
class SpectralKMeans(torch.nn.Module):
    """K spectral clusters of a cached split and their label maps.  Buffers (a checkpoint carries the model): ``pivot`` (C,) fp32,
    ``centers`` (K, C) fp32 = centroids minus pivot, ``bias`` (K,) fp32 = ``|center|^2 / 2``, ``counts`` (K,) int64 of the fitted
    pixels, ``foreground_share`` (K,) fp64 -- NaN until ``calibrate`` -- and ``meta`` = (iterations, inertia, converged) fp64.

    ``model(x, output=...)`` takes what ``SpectralDetector`` takes -- an image in either logical shape, ``(N, 1, C, h, w)`` or
    ``(N, C, h, w)``, or the cache's batch dict -- and returns an ``(N, 1, h, w)`` map: ``"labels"`` uint8, ``"distance"`` the fp32
    squared distance to the nearest centroid, ``"score"`` the winning score ``zmin``, ``"logit"`` the logit of the label's foreground
    share (clamped to ``[2^-24, 1 - 2^-24]`` as ``detect.py`` clamps), which the evaluation functions read as a network's output.
    No autograd: an input that requires grad raises."""

    def __init__(self, pivot, centers, counts=None, foreground_share=None, meta=None):
        super().__init__()
        c = _centers32(centers, who="SpectralKMeans")
        K, C = c.shape
        pv = _vector32(pivot, C, "SpectralKMeans")
        cnt = np.zeros(K, dtype=np.int64) if counts is None else np.asarray(counts, dtype=np.int64)
        share = np.full(K, np.nan) if foreground_share is None else np.asarray(foreground_share, dtype=np.float64)
        if cnt.shape != (K,) or share.shape != (K,):
            raise ValueError(f"SpectralKMeans: counts and foreground_share must have shape ({K},)")
        self.register_buffer("pivot", torch.from_numpy(pv.copy()))
        self.register_buffer("centers", torch.from_numpy(c.copy()))
        self.register_buffer("bias", torch.from_numpy(score_rows(c)[1].copy()))
        self.register_buffer("counts", torch.from_numpy(cnt.copy()))
        self.register_buffer("foreground_share", torch.from_numpy(share.copy()))
        self.register_buffer("meta", torch.tensor([0.0, float("nan"), 0.0] if meta is None else [float(v) for v in meta], dtype=torch.float64))
        self._padded = None             # (key, pivot (cs), rows (ks, cs), bias (ks)) on the device, rebuilt when the buffers or cs change
        self._lut = None                # (key, lut (K,)) on the device

    @classmethod
    def blank(cls, bands: int, k: int) -> "SpectralKMeans":
        """A model of the given shapes for ``load_state_dict`` to fill."""
        return cls(np.zeros(int(bands)), np.zeros((int(k), int(bands))))

    # ---- properties ---------------------------------------------------------------------------------
    @property
    def k(self) -> int:
        return int(self.centers.shape[0])

    @property
    def in_channels(self) -> int:
        return int(self.centers.shape[1])

    @property
    def centroids(self) -> np.ndarray:
        """``pivot + centers`` in fp64, (K, C)."""
        return self.pivot.detach().cpu().numpy().astype(np.float64)[None, :] + self.centers.detach().cpu().numpy().astype(np.float64)

    @property
    def n_iter_(self) -> int:
        return int(self.meta[0])

    @property
    def inertia_(self) -> float:
        return float(self.meta[1])

    @property
    def converged_(self) -> bool:
        return bool(self.meta[2] != 0)

    # ---- the fit ------------------------------------------------------------------------------------
    @classmethod
    def fit(cls, cache: CubeCache, k: int, slots: Optional[Sequence[int]] = None, select: str = "all", init="k-means++", n_init: int = 1,
            max_iter: int = 50, tol: float = 1e-4, seed: int = 0, merge: Optional[Callable[[ClusterSums], ClusterSums]] = None,
            pivot=None) -> "SpectralKMeans":
        """Lloyd's k-means on the selected pixels of ``slots``.  ``pivot = fp32(mean)`` from one ``band_moments`` pass, unless a
        (C,) ``pivot`` is given: the ranks of a multi-rank fit must share one, as sums of ``x - pivot`` add up only about the same
        pivot (give every rank the fp32 mean of the whole split, from ``merge_statistics`` or an all-reduced ``band_moments``).  ``init``:
        ``"k-means++"`` (D^2 sampling in fp64 numpy on a seeded sample of at most 4096 selected pixels read from the cache),
        ``"sample"`` (k seeded pixels) or a (k, C) array of centroids.  Per iteration one ``cluster_step`` -- through ``merge`` if
        given, a callable ``ClusterSums -> ClusterSums`` that adds the other ranks' sums (every rank then needs the same ``pivot``
        and the same starting centres: an explicit init) --, the update in fp64 on the host, one host synchronisation.  Stops
        as ``_lloyd`` states; ``n_init`` restarts (seeds ``seed``, ``seed + 1``, ...) keep the lowest inertia.  The model is placed
        on the cache's device with ``n_iter_``, ``inertia_``, ``converged_`` and ``counts`` of the final pass."""
        code = _check_select(select)
        if not isinstance(cache, CubeCache):
            raise TypeError("cluster: need a CubeCache")
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"SpectralKMeans: k must lie in [1, {MAX_K}], got {k}")
        explicit = not isinstance(init, str)
        if not explicit and init not in INITS:
            raise ValueError(f"SpectralKMeans: init must be one of {INITS} or a (k, C) array, got {init!r}")
        if explicit:
            start = init.detach().cpu().numpy() if isinstance(init, torch.Tensor) else np.asarray(init)
            if start.shape != (k, cache.C):
                raise ValueError(f"SpectralKMeans: an explicit init must have shape ({k}, {cache.C}), got {tuple(start.shape)}")
            if not np.isfinite(start).all():
                raise ValueError("SpectralKMeans: the init must be finite")
        if int(n_init) < 1 or int(max_iter) < 1 or not float(tol) >= 0:
            raise ValueError("SpectralKMeans: n_init and max_iter must be at least 1 and tol non-negative")
        idx = _slot_list(cache, slots)
        C = cache.C
        n, sums = band_moments(cache, idx, select)
        if n < k:
            raise ValueError(f"SpectralKMeans: {n} selected pixel(s) for k = {k}")
        pivot = (sums[:C] / n).astype(np.float32) if pivot is None else _vector32(pivot, C, "SpectralKMeans")
        p64 = pivot.astype(np.float64)
        best = None
        with torch.cuda.device(cache.device):
            ps = _FitPass(cache, idx, pivot, k)

            def step(c32: np.ndarray) -> ClusterSums:
                s = ps.step(c32, code)
                return s if merge is None else merge(s)
            for trial in range(1 if explicit else int(n_init)):
                if explicit:
                    c0 = start.astype(np.float64) - p64
                else:
                    c0 = init_centers(_sample_pixels(cache, idx, code, int(seed) + trial) - p64, k, init, int(seed) + trial)
                got = _lloyd(step, c0.astype(np.float32), C, max_iter, tol)
                if best is None or got[1].inertia < best[1].inertia:
                    best = got
        centers, final, n_iter, converged = best
        return cls(pivot, centers, counts=final.counts, meta=(n_iter, final.inertia, 1.0 if converged else 0.0)).to(cache.device)

    def calibrate(self, cache: CubeCache, slots: Optional[Sequence[int]] = None) -> np.ndarray:
        """Two fitting passes over the masks' classes: the (K, 2) int64 contingency table (column 0 background, 1 foreground) of label
        against mask, and ``foreground_share[k] = foreground / (foreground + background)`` of cluster k; a cluster that no
        calibration pixel falls into takes the overall foreground share.  Returns the table."""
        pv, c = self.pivot.detach().cpu().numpy(), self.centers.detach().cpu().numpy()
        fg = cluster_step(cache, pv, c, slots, "foreground").counts
        bg = cluster_step(cache, pv, c, slots, "background").counts
        table = np.stack([bg, fg], axis=1).astype(np.int64)
        tot = table.sum(axis=1)
        if tot.sum() == 0:
            raise ValueError("SpectralKMeans.calibrate: no pixel")
        share = np.where(tot > 0, fg / np.maximum(tot, 1), fg.sum() / tot.sum())
        self.foreground_share.copy_(torch.from_numpy(share.astype(np.float64)))
        return table

    # ---- prediction ---------------------------------------------------------------------------------
    def _device_rows(self, device, cs: int):
        key = (str(device), cs) + tuple((b._version, b.data_ptr()) for b in (self.pivot, self.centers, self.bias))
        if self._padded is None or self._padded[0] != key:
            K, C = self.k, self.in_channels
            pv = torch.zeros(cs, dtype=torch.float32, device=device)
            w = torch.zeros((_rup(K, 8), cs), dtype=torch.float32, device=device)
            b = torch.zeros(_rup(K, 8), dtype=torch.float32, device=device)
            pv[:C] = self.pivot.to(device)
            w[:K, :C] = -self.centers.to(device)
            b[:K] = self.bias.to(device)
            self._padded = (key, pv, w, b)
        return self._padded[1:]

    def _device_lut(self, device):
        key = (str(device), self.foreground_share._version, self.foreground_share.data_ptr())
        if self._lut is None or self._lut[0] != key:
            share = self.foreground_share.detach().cpu().numpy()
            if not np.isfinite(share).all():
                raise RuntimeError("SpectralKMeans: output='logit' needs foreground shares; run calibrate() first")
            p = np.clip(share, P_LO, P_HI)
            self._lut = (key, torch.from_numpy((np.log(p) - np.log1p(-p)).astype(np.float32)).to(device))
        return self._lut[1]

    def forward(self, x, output: str = "labels"):
        if isinstance(x, dict):
            x = x['image']
        if output not in OUTPUTS:
            raise ValueError(f"SpectralKMeans: output must be one of {OUTPUTS}, got {output!r}")
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("hyperpri_amd: SpectralKMeans needs a tensor on a ROCm device; there is no CPU fallback")
        if x.requires_grad:
            raise RuntimeError("SpectralKMeans: no autograd -- the input must not require grad")
        if x.dtype != torch.float32:
            raise ValueError(f"SpectralKMeans: need a float32 image, got {x.dtype}")
        five = x.dim() == 5
        if five and x.shape[1] != 1 or x.dim() not in (4, 5):
            raise ValueError(f"SpectralKMeans: need an (N, 1, C, h, w) or (N, C, h, w) image, got {tuple(x.shape)}")
        t = x[:, 0] if five else x
        if getattr(x, "_hpri_zero_padded", False):
            t._hpri_zero_padded = True
        N, C, h, w = (int(s) for s in t.shape)
        if C != self.in_channels:
            raise ValueError(f"SpectralKMeans: the image has {C} bands, the model {self.in_channels}")
        if N * h * w == 0:
            raise ValueError("SpectralKMeans: empty image")
        with torch.cuda.device(x.device):
            src, cs = _band_input(t)
            if cs > max_channel_stride():
                raise ValueError(f"SpectralKMeans: a channel stride of {cs} exceeds the {max_channel_stride()} the kernels take")
            pv, wd, bd = self._device_rows(x.device, cs)
            lut = self._device_lut(x.device) if output == "logit" else None
            out = torch.empty((N, 1, h, w), dtype=torch.uint8 if output == "labels" else torch.float32, device=x.device)
            ptr = [None, None, None, None]
            ptr[OUTPUTS.index(output)] = _p(out)
            labels, dist2, zmin, value = ptr
            _lib.call("hpri_band_assign", _p(src), N * h * w, cs, _p(pv), _p(wd), _p(bd), self.k, _p(lut), labels, zmin, dist2, value, _stream())
        return out


# ---------------------------------------------------------------------------------------------------
# The contract restated in numpy: the oracles of the GPU tests
# ---------------------------------------------------------------------------------------------------
def _centred(x, pivot) -> np.ndarray:
    """``d = fp32(x - pivot)`` as the device rounds it (one IEEE subtraction in fp32), widened to fp64."""
    x32 = np.asarray(x).astype(np.float32)
    if pivot is None:
        return x32.astype(np.float64)
    return (x32 - np.asarray(pivot).astype(np.float32)).astype(np.float64)


def score_bound(x, pivot, centers, bias, cs: Optional[int] = None) -> np.ndarray:
    """``E[p, k] = (cs + 1) u (|bias[k]| + sum_c |centers[k, c]| |d[p, c]|)``, ``u = 2^-24``: the project's bound for a chain of ``cs``
    fused multiply-adds (``cs`` defaults to the band count rounded up to 8)."""
    d = _centred(x, pivot).reshape(-1, np.asarray(x).shape[-1])
    w, b = np.asarray(centers, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    cs = _rup(d.shape[1], 8) if cs is None else int(cs)
    return (cs + 1) * U * (np.abs(b)[None, :] + np.abs(d) @ np.abs(w).T)


def assign_reference(x, pivot, centers, bias, cs: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``hpri_band_assign`` in fp64 numpy on (..., C) fp32 pixels: ``(labels (P,) int64, z (P, K) fp64, ambiguous (P,) bool)`` with
    ``z = d W^T + b`` for the kernel's operands ``centers`` = W (K, C) and ``bias`` = b (K,), ``d = fp32(x - pivot)``; the label is
    the lowest index of the minimum.  ``ambiguous[p]`` is true where some ``k != label`` has ``z[k] - zmin <= E[k] + E[label]``
    (``score_bound``): fp32 rounding may then prefer k."""
    d = _centred(x, pivot).reshape(-1, np.asarray(x).shape[-1])
    w, b = np.asarray(centers, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    z = d @ w.T + b
    labels = np.argmin(z, axis=1)                        # (the first, that is the lowest, index of the minimum)
    E = score_bound(x, pivot, centers, bias, cs)
    rows = np.arange(z.shape[0])
    close = z - z[rows, labels][:, None] <= E + E[rows, labels][:, None]
    close[rows, labels] = False
    return labels.astype(np.int64), z, close.any(axis=1)


def cluster_step_reference(cubes, pivot, centers, masks=None, select: str = "all", return_ambiguous: bool = False):
    """``cluster_step`` in fp64 numpy on (n, H, W, C) ``cubes`` as the cache stores them: ``centers`` (K, C) = centroids minus
    pivot as fp32 values, the operands ``score_rows(centers)``; sums of ``d = fp32(x - pivot)`` in fp64.  With
    ``return_ambiguous``: ``(ClusterSums, labels, ambiguous)`` over the selected pixels in slot-list and row-major order."""
    x = _selected_pixels(cubes, masks, select)
    c32 = _centers32(centers, x.shape[1], "cluster_step_reference")
    w, b = score_rows(c32)
    labels, z, amb = assign_reference(x, pivot, w, b)
    d = _centred(x, pivot)
    K = c32.shape[0]
    sums = np.zeros((K, x.shape[1]))
    np.add.at(sums, labels, d)
    out = ClusterSums(np.bincount(labels, minlength=K).astype(np.int64), sums, float(z[np.arange(len(labels)), labels].sum()), float((d * d).sum()))
    return (out, labels, amb) if return_ambiguous else out


@dataclass
class KMeansReference:
    pivot: np.ndarray           # (C,) fp32
    centers: np.ndarray         # (K, C) fp32, centroids minus pivot
    final: ClusterSums
    labels: np.ndarray          # of the final pass, over the selected pixels
    n_iter: int
    converged: bool
    ambiguous: int              # pixels flagged ambiguous, summed over every pass


def kmeans_reference(cubes, init, masks=None, select: str = "all", max_iter: int = 50, tol: float = 1e-4, pivot=None) -> KMeansReference:
    """``SpectralKMeans.fit`` from an explicit (k, C) ``init`` of centroids, in fp64 numpy: the same pivot rule (``fp32(mean)`` of the
    selected pixels unless ``pivot`` is given), the same Lloyd loop and stopping rule (``_lloyd``)."""
    x = _selected_pixels(cubes, masks, select)
    pv = x.mean(axis=0).astype(np.float32) if pivot is None else _vector32(pivot, x.shape[1], "kmeans_reference")
    state = {"ambiguous": 0, "labels": None}

    def step(c32: np.ndarray) -> ClusterSums:
        s, labels, amb = cluster_step_reference(cubes, pv, c32, masks, select, return_ambiguous=True)
        state["ambiguous"] += int(amb.sum())
        state["labels"] = labels
        return s
    c0 = (np.asarray(init, dtype=np.float64) - pv.astype(np.float64)).astype(np.float32)
    centers, final, n_iter, converged = _lloyd(step, _centers32(c0, x.shape[1], "kmeans_reference"), x.shape[1], max_iter, tol)
    return KMeansReference(pv, centers, final, state["labels"], n_iter, converged, state["ambiguous"])


__all__ = ["SpectralKMeans", "ClusterSums", "KMeansReference", "merge_cluster_sums", "cluster_step", "init_centers", "score_rows", "score_bound",
           "assign_reference", "cluster_step_reference", "kmeans_reference", "workspace_bytes", "max_k", "cluster_parts", "MAX_K", "INITS",
           "OUTPUTS"]
