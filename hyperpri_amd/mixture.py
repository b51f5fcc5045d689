"""Spectral Gaussian mixtures on the device (``csrc/mixture.hip``): the Gaussian maximum-likelihood classifier, its mixture form and EM
with full covariances on the pixels' spectra of a cached split.

``detect.py`` needs one target spectrum, ``cluster.py`` is hard and spherical, ``unmix.py`` linear; this module learns a density per
class from the masks: one Gaussian per class (QDA), several (mixture discriminant analysis), or an unsupervised soft clustering with
responsibilities and a per-pixel negative log-likelihood as an anomaly map.  The class log-likelihoods are ``(N, C, h, w)`` unaries
for ``dense_crf`` / ``CRFLayer`` and ``CrossEntropyLoss``.  The split stays in HBM.

The model: a shared projection to ``q <= 32`` dimensions (typically ``SpectralProjection.pca(stats, q, whiten=True).weight``: full-band
covariances are ill-conditioned), then ``K <= 8`` Gaussians there, each of one of ``C <= 8`` classes.  include/hyperpri_hip.h states the
contract of the kernels (``z``, ``u_k = A_k z + a_k`` with ``A_k = L_k^-1``, ``m_k``, ``l_k``, ``L_c``, ``r_k``, the sums ``N_k``, ``S_k``,
``Q_k`` about the current means, ``LL``); ``_terms`` below restates it.

``gmm_score_reference``, ``gmm_step_reference`` and ``gmm_reference`` restate the contract and the EM loop in fp64 numpy on the same
fp32 operands; ``gmm_bound`` derives what fp32 rounding may do to every output.  No autograd, no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .cache import _DT, CubeCache
from ._args import _p, _rup, _stream
from .cluster import _sample_pixels, _vector32, init_centers
from .spectral import (FP32_RUN, SpectralProjection, _band_input, _check_select, _selected_pixels, _slot_list, band_moments,
                       max_channel_stride)

MAX_K = 8                   # hpri_band_gmm_max_components (components, and classes)
MAX_Q = 32                  # hpri_band_gmm_max_dims
OUTPUTS = ("logit", "loglik", "labels", "resp", "nll")
U = 2.0 ** -24
# HIP's math API lists expf and logf within 1 ulp of the exact result; the bounds allow 2 (1 ulp is at most 2 u relative).
EXP_ULP = 2.0
LOG_ULP = 2.0
LOG_2PI = math.log(2.0 * math.pi)


def gmm_parts() -> int:
    """The number of fp64 partial accumulators of the fitting pass (``hpri_band_gmm_parts``): a constant."""
    return int(_lib.load().hpri_band_gmm_parts())


def workspace_bytes(cs: int, q: int, k: int) -> int:
    """Scratch of the fitting pass (``hpri_band_gmm_workspace_bytes``): a function of its arguments alone."""
    return int(_lib.load().hpri_band_gmm_workspace_bytes(int(cs), int(q), int(k)))


# ---------------------------------------------------------------------------------------------------
# Operands and sums
# ---------------------------------------------------------------------------------------------------
@dataclass
class GmmOperands:
    """What the kernels take, as the fp32 values they receive: ``pivot`` (C,), ``weight`` (q, C), ``A`` (K, q, q), ``a`` (K, q), ``c``
    (K,), ``means`` (K, q) and the class of every component (K,) int64."""
    pivot: np.ndarray
    weight: np.ndarray
    A: np.ndarray
    a: np.ndarray
    c: np.ndarray
    means: np.ndarray
    classes: np.ndarray

    @property
    def k(self) -> int:
        return int(self.A.shape[0])

    @property
    def q(self) -> int:
        return int(self.weight.shape[0])

    @property
    def n_classes(self) -> int:
        return int(self.classes.max()) + 1


def _np(v) -> np.ndarray:
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def gmm_operands(pivot, weight, means, covariances, weights, classes=None) -> GmmOperands:
    """The kernels' operands of a model, derived in fp64 and rounded once: ``L_k`` the Cholesky factor of ``covariances[k]``,
    ``A_k = L_k^-1``, ``a_k = -A_k m_k`` for the fp32 means, ``c_k = log weights[k] - sum log diag L_k - (q / 2) log 2 pi``."""
    w = np.ascontiguousarray(_np(weight).astype(np.float64).astype(np.float32))
    if w.ndim != 2 or w.shape[0] < 1 or w.shape[0] > MAX_Q:
        raise ValueError(f"SpectralGMM: need a projection weight (q, C) with q in [1, {MAX_Q}], got {tuple(w.shape)}")
    q, C = w.shape
    pv = _vector32(pivot, C, "SpectralGMM")
    m = np.ascontiguousarray(_np(means).astype(np.float64).astype(np.float32))
    if m.ndim != 2 or m.shape[1] != q or not 1 <= m.shape[0] <= MAX_K:
        raise ValueError(f"SpectralGMM: need means (K, {q}) with K in [1, {MAX_K}], got {tuple(m.shape)}")
    K = m.shape[0]
    cov = _np(covariances).astype(np.float64)
    pi = _np(weights).astype(np.float64)
    cls = np.zeros(K, dtype=np.int64) if classes is None else _np(classes).astype(np.int64)
    if cov.shape != (K, q, q) or pi.shape != (K,) or cls.shape != (K,):
        raise ValueError(f"SpectralGMM: need covariances ({K}, {q}, {q}), weights ({K},) and classes ({K},)")
    if not (np.isfinite(w).all() and np.isfinite(m).all() and np.isfinite(cov).all() and (pi > 0).all() and np.isfinite(pi).all()):
        raise ValueError("SpectralGMM: the parameters must be finite and the weights positive")
    if cls.min() < 0 or cls.max() >= MAX_K:
        raise ValueError(f"SpectralGMM: the classes must lie in [0, {MAX_K})")
    L = np.linalg.cholesky(0.5 * (cov + cov.transpose(0, 2, 1)))                  # (raises on a covariance that is not positive definite)
    A = np.tril(np.linalg.inv(L))
    a = -np.einsum("kij,kj->ki", A, m.astype(np.float64))
    c = np.log(pi) - np.log(np.diagonal(L, axis1=1, axis2=2)).sum(axis=1) - 0.5 * q * LOG_2PI
    return GmmOperands(pv, w, A.astype(np.float32), a.astype(np.float32), c.astype(np.float32), m, cls)


@dataclass
class GmmSums:
    """What one fitting pass returns: the count of selected pixels, ``N`` (K,), ``S`` (K, q), ``Q`` (K, q, q) in fp64 about the means
    the pass was given, and ``LL``, the sum of the pixels' log-likelihoods."""
    count: int
    N: np.ndarray
    S: np.ndarray
    Q: np.ndarray
    LL: float


def merge_gmm_sums(a: GmmSums, b: GmmSums) -> GmmSums:
    """The sums of the union of two disjoint pixel sets (two caches, two ranks) under the same pivot, projection and parameters."""
    if a.Q.shape != b.Q.shape:
        raise ValueError("merge_gmm_sums: the shapes differ")
    return GmmSums(a.count + b.count, a.N + b.N, a.S + b.S, a.Q + b.Q, a.LL + b.LL)


def _device_operands(ops: GmmOperands, device, cs: int) -> Tuple[torch.Tensor, ...]:
    """(pivot (cs), weight (qp, cs), A (K, qp, qp), a (K, qp), c (K), means (K, qp)) zero-padded on the device."""
    q, C, K = ops.q, ops.weight.shape[1], ops.k
    qp = _rup(q, 8)
    pv = np.zeros(cs, np.float32)
    pv[:C] = ops.pivot
    w = np.zeros((qp, cs), np.float32)
    w[:q, :C] = ops.weight
    A = np.zeros((K, qp, qp), np.float32)
    A[:, :q, :q] = ops.A
    a = np.zeros((K, qp), np.float32)
    a[:, :q] = ops.a
    m = np.zeros((K, qp), np.float32)
    m[:, :q] = ops.means
    return tuple(torch.from_numpy(np.ascontiguousarray(v)).to(device) for v in (pv, w, A, a, ops.c.astype(np.float32), m))


class _GmmPass:
    """What the passes of one fit share: the slot table and the workspace on the device, the packed result buffer (one copy to the
    host, one synchronisation per pass)."""

    def __init__(self, cache: CubeCache, idx: Sequence[int], q: int, k: int):
        self.cache, self.q, self.k = cache, int(q), int(k)
        dev, cs = cache.device, cache.cs
        self.qp = _rup(self.q, 8)
        self.table = torch.tensor(list(idx), dtype=torch.int32).to(dev)
        self.nbytes = workspace_bytes(cs, q, k)
        self.work = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.out = torch.empty(2 + k * (1 + self.qp + self.qp * self.qp), dtype=torch.float64, device=dev)   # count | N | S | Q | LL
        self.head = (_p(cache._cubes), _DT[cache.store_dtype], cache.capacity, cache.H, cache.W, cs, _p(cache._masks), _p(self.table), len(idx))

    def step(self, ops: GmmOperands, select: int) -> GmmSums:
        c, k, q, qp = self.cache, self.k, self.q, self.qp
        if ops.k != k or ops.q != q or ops.weight.shape[1] != c.C:
            raise ValueError("gmm_step: the operands do not fit the pass")
        pv, w, A, a, cst, m = _device_operands(ops, c.device, c.cs)
        base = self.out.data_ptr()
        oN, oS, oQ = base + 8, base + 8 * (1 + k), base + 8 * (1 + k + k * qp)
        oLL = oQ + 8 * k * qp * qp
        _lib.call("hpri_band_gmm_sums", *self.head, select, _p(pv), _p(w), q, _p(A), _p(a), _p(cst), _p(m), k, _p(self.work), self.nbytes,
                  base, oN, oS, oQ, oLL, _stream())
        host = self.out.cpu().numpy()
        N = host[1:1 + k].copy()
        S = host[1 + k:1 + k + k * qp].reshape(k, qp)[:, :q].copy()
        Q = host[1 + k + k * qp:1 + k + k * qp + k * qp * qp].reshape(k, qp, qp)[:, :q, :q].copy()
        return GmmSums(int(host[:1].view(np.int64)[0]), N, S, Q, float(host[-1]))


def gmm_step(cache: CubeCache, operands: GmmOperands, slots: Optional[Sequence[int]] = None, select: str = "all") -> GmmSums:
    """One fitting pass (``hpri_band_gmm_sums``) over the selected pixels of ``slots`` (default: every filled slot) at the given
    operands.  One host synchronisation."""
    code = _check_select(select)
    if not isinstance(cache, CubeCache):
        raise TypeError("mixture: need a CubeCache")
    idx = _slot_list(cache, slots)
    with torch.cuda.device(cache.device):
        return _GmmPass(cache, idx, operands.q, operands.k).step(operands, code)


# ---------------------------------------------------------------------------------------------------
# EM (shared by the fit and its restatement)
# ---------------------------------------------------------------------------------------------------
@dataclass
class GmmFit:
    means: np.ndarray           # (K, q) fp32
    covariances: np.ndarray     # (K, q, q) fp64
    weights: np.ndarray         # (K,) fp64
    history: List[float]        # the mean log-likelihood at the parameters of every pass
    n_iter: int
    converged: bool
    starved: List[int]          # components that kept their parameters in some iteration
    count: int


def _em(step: Callable[[np.ndarray, np.ndarray, np.ndarray], GmmSums], means, covariances, weights, max_iter: int, tol: float,
        reg_covar: float) -> GmmFit:
    """EM on (K, q) fp32 means, (K, q, q) fp64 covariances and (K,) fp64 weights: per iteration one ``step`` at the current parameters,
    then the M-step in fp64 -- ``m' = fp32(m + S / N)``, ``Sigma' = Q / N - (S / N)(S / N)^T + reg_covar I``, ``pi' = N / sum N`` --; a
    component with ``N_k < q + 1`` keeps mean and covariance and is listed.  Stops after the M-step of the first pass whose mean
    log-likelihood gained less than ``tol`` over the previous pass', or at ``max_iter``."""
    if int(max_iter) < 1 or not float(tol) >= 0 or not float(reg_covar) >= 0:
        raise ValueError("SpectralGMM: max_iter must be at least 1, tol and reg_covar non-negative")
    m = np.asarray(means, dtype=np.float32).copy()
    cov = np.asarray(covariances, dtype=np.float64).copy()
    pi = np.asarray(weights, dtype=np.float64).copy()
    K, q = m.shape
    history, starved, converged, n_iter, count = [], set(), False, 0, 0
    for it in range(1, int(max_iter) + 1):
        s = step(m, cov, pi)
        if s.count == 0:
            raise ValueError("SpectralGMM: no selected pixel")
        count, n_iter = s.count, it
        history.append(s.LL / s.count)
        for k in range(K):
            if not s.N[k] >= q + 1:
                starved.add(k)
                continue
            mu = s.S[k] / s.N[k]
            cov[k] = s.Q[k] / s.N[k] - np.outer(mu, mu) + float(reg_covar) * np.eye(q)
            m[k] = (m[k].astype(np.float64) + mu).astype(np.float32)
        pi = np.maximum(s.N, 1e-300) / np.maximum(s.N, 1e-300).sum()
        if len(history) >= 2 and history[-1] - history[-2] < float(tol):
            converged = True
            break
    return GmmFit(m, cov, pi, history, n_iter, converged, sorted(starved), count)


def hard_init(z, means, reg_covar: float = 1e-6) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Starting parameters from (n, q) fp64 points ``z`` and (K, q) means: every point goes to its nearest mean; a component's
    covariance is that of its points about the given mean plus ``reg_covar I`` (the covariance of all points where it has fewer than
    q + 1), its weight its share (at least one point's)."""
    z = np.asarray(z, dtype=np.float64)
    m = np.asarray(means, dtype=np.float64)
    K, q = m.shape
    lab = np.argmin(((z[:, None, :] - m[None, :, :]) ** 2).sum(axis=2), axis=1)
    whole = np.cov(z.T).reshape(q, q) + reg_covar * np.eye(q)
    cov = np.zeros((K, q, q))
    pi = np.zeros(K)
    for k in range(K):
        e = z[lab == k] - m[k]
        cov[k] = e.T @ e / len(e) + reg_covar * np.eye(q) if len(e) >= q + 1 else whole
        pi[k] = max(len(e), 1)
    return m.astype(np.float32), cov, pi / pi.sum()


# ---------------------------------------------------------------------------------------------------
# The module
# ---------------------------------------------------------------------------------------------------
def _projection(projection, bands: int) -> np.ndarray:
    w = projection.weight if isinstance(projection, SpectralProjection) else projection
    w = _np(w)
    if w.ndim != 2 or w.shape[1] != bands or not 1 <= w.shape[0] <= MAX_Q:
        raise ValueError(f"SpectralGMM: need a projection (q, {bands}) with q in [1, {MAX_Q}], got {tuple(w.shape)}")
    return np.ascontiguousarray(w.astype(np.float64).astype(np.float32))


class SpectralGMM(torch.nn.Module):
    """K Gaussians in a q-dimensional projection of the spectrum, each of one class.  Buffers (a checkpoint carries the model):
    ``pivot`` (C,) fp32, ``weight`` (q, C) fp32, ``means`` (K, q) fp32, ``covariances`` (K, q, q) fp64, ``weights`` (K,) fp64 -- the
    joint weights: class prior times the weight inside the class --, ``classes`` (K,) int64 and ``meta`` = (iterations, mean
    log-likelihood, converged, bit set of starved components) fp64.  The kernels' operands are derived in fp64 whenever the buffers
    change (``operands``).

    ``model(x, output=...)`` takes what ``SpectralKMeans`` takes and returns ``"logit"`` (N, 1, h, w) = ``L_1 - L_0`` (two classes
    only: the log posterior odds of the foreground, which the evaluation functions read as a network's output), ``"loglik"``
    (N, C, h, w) = the joint log-likelihood of every class, ``"labels"`` (N, 1, h, w) uint8, ``"resp"`` (N, K, h, w) or ``"nll"``
    (N, 1, h, w) = minus the log-likelihood under the whole mixture.  No autograd: an input that requires grad raises."""

    def __init__(self, pivot, weight, means, covariances, weights, classes=None, meta=None):
        super().__init__()
        ops = gmm_operands(pivot, weight, means, covariances, weights, classes)
        K = ops.k
        self.register_buffer("pivot", torch.from_numpy(ops.pivot.copy()))
        self.register_buffer("weight", torch.from_numpy(ops.weight.copy()))
        self.register_buffer("means", torch.from_numpy(ops.means.copy()))
        self.register_buffer("covariances", torch.from_numpy(_np(covariances).astype(np.float64).copy()))
        self.register_buffer("weights", torch.from_numpy(_np(weights).astype(np.float64).copy()))
        self.register_buffer("classes", torch.from_numpy(ops.classes.copy()))
        self.register_buffer("meta", torch.tensor([0.0, float("nan"), 0.0, 0.0] if meta is None else [float(v) for v in meta], dtype=torch.float64))
        assert self.classes.shape == (K,)
        self._ops = None                # (key, GmmOperands)
        self._dev = None                # (key, device operands)

    @classmethod
    def blank(cls, bands: int, q: int, k: int, n_classes: int = 1) -> "SpectralGMM":
        """A model of the given shapes for ``load_state_dict`` to fill."""
        q, k = int(q), int(k)
        if not 1 <= int(n_classes) <= min(k, MAX_K):
            raise ValueError(f"SpectralGMM: need between one class and one per component, got {n_classes}")
        return cls(np.zeros(int(bands)), np.zeros((q, int(bands))), np.zeros((k, q)), np.tile(np.eye(q), (k, 1, 1)), np.full(k, 1.0 / k),
                   np.minimum(np.arange(k), int(n_classes) - 1))

    # ---- properties ---------------------------------------------------------------------------------
    k = property(lambda self: int(self.means.shape[0]))
    q = property(lambda self: int(self.weight.shape[0]))
    in_channels = property(lambda self: int(self.weight.shape[1]))
    n_classes = property(lambda self: int(self.classes.max()) + 1)
    n_iter_ = property(lambda self: int(self.meta[0]))
    log_likelihood_ = property(lambda self: float(self.meta[1]))
    converged_ = property(lambda self: bool(self.meta[2] != 0))
    starved_ = property(lambda self: [k for k in range(self.k) if int(self.meta[3]) >> k & 1])

    def _key(self):
        return tuple((b._version, b.data_ptr()) for b in (self.pivot, self.weight, self.means, self.covariances, self.weights, self.classes))

    @property
    def operands(self) -> GmmOperands:
        key = self._key()
        if self._ops is None or self._ops[0] != key:
            self._ops = (key, gmm_operands(self.pivot, self.weight, self.means, self.covariances, self.weights, self.classes))
        return self._ops[1]

    # ---- the fits -----------------------------------------------------------------------------------
    @classmethod
    def _fit_one(cls, cache, ps, idx, code, pivot, w32, k, init, max_iter, tol, reg_covar, seed, merge, callback) -> GmmFit:
        q = w32.shape[0]
        if isinstance(init, str):
            if init != "k-means++":
                raise ValueError(f"SpectralGMM: init must be 'k-means++', (k, q) means or (means, covariances[, weights]), got {init!r}")
            z = (_sample_pixels(cache, idx, code, seed) - pivot.astype(np.float64)) @ w32.astype(np.float64).T
            start = hard_init(z, init_centers(z, k, "k-means++", seed), max(reg_covar, 1e-12))
        elif isinstance(init, (tuple, list)) and len(init) in (2, 3) and np.ndim(init[1]) == 3:
            pi0 = np.full(k, 1.0 / k) if len(init) == 2 else np.asarray(init[2], dtype=np.float64)
            start = (np.asarray(_np(init[0]), dtype=np.float32), np.asarray(_np(init[1]), dtype=np.float64), pi0)
        else:
            z = (_sample_pixels(cache, idx, code, seed) - pivot.astype(np.float64)) @ w32.astype(np.float64).T
            start = hard_init(z, _np(init), max(reg_covar, 1e-12))
        if start[0].shape != (k, q) or start[1].shape != (k, q, q) or start[2].shape != (k,):
            raise ValueError(f"SpectralGMM: the init must give {k} components of {q} dimensions")
        cls0 = np.zeros(k, dtype=np.int64)

        def step(m, cov, pi):
            ops = gmm_operands(pivot, w32, m, cov, pi, cls0)
            s = ps.step(ops, code)
            s = s if merge is None else merge(s)
            if callback is not None:
                callback(ops, s)
            return s
        return _em(step, *start, max_iter=1 if k == 1 else max_iter, tol=tol, reg_covar=reg_covar)

    @classmethod
    def fit(cls, cache: CubeCache, projection, k: int, slots: Optional[Sequence[int]] = None, select: str = "all", init="k-means++",
            max_iter: int = 100, tol: float = 1e-4, reg_covar: float = 1e-6, seed: int = 0, pivot=None,
            merge: Optional[Callable[[GmmSums], GmmSums]] = None, callback: Optional[Callable[[GmmOperands, GmmSums], None]] = None) -> "SpectralGMM":
        """EM on the selected pixels of ``slots`` in ``projection`` (a ``SpectralProjection`` -- its weight is used -- or a (q, C) array).
        ``pivot``: the fp32 mean of the selected pixels from one ``band_moments`` pass unless given (the ranks of a multi-rank fit
        share one).  ``init``: ``"k-means++"`` (D^2 sampling on a seeded sample of at most 4096 selected pixels, then ``hard_init``),
        (k, q) means in the projection (``hard_init`` on the same sample) or ``(means, covariances[, weights])``.  Per iteration one
        ``gmm_step`` -- through ``merge`` if given, which adds the other ranks' sums --, the M-step in fp64 on the host (``_em``) and
        one host synchronisation; ``callback(operands, sums)`` sees every pass.  One component needs exactly one pass.  One class;
        ``fit_classes`` fits one mixture per mask class."""
        code = _check_select(select)
        idx = _slot_list(cache, slots)
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"SpectralGMM: k must lie in [1, {MAX_K}], got {k}")
        w32 = _projection(projection, cache.C)
        if pivot is None:
            n, sums = band_moments(cache, idx, select)
            if n < k:
                raise ValueError(f"SpectralGMM: {n} selected pixel(s) for k = {k}")
            pivot = (sums[:cache.C] / n).astype(np.float32)
        pivot = _vector32(pivot, cache.C, "SpectralGMM")
        with torch.cuda.device(cache.device):
            ps = _GmmPass(cache, idx, w32.shape[0], k)
            f = cls._fit_one(cache, ps, idx, code, pivot, w32, k, init, max_iter, tol, reg_covar, int(seed), merge, callback)
        return cls(pivot, w32, f.means, f.covariances, f.weights, None, _meta(f)).to(cache.device)

    @classmethod
    def fit_classes(cls, cache: CubeCache, projection, components: Tuple[int, int] = (1, 1), slots: Optional[Sequence[int]] = None,
                    init="k-means++", max_iter: int = 100, tol: float = 1e-4, reg_covar: float = 1e-6, seed: int = 0, pivot=None,
                    callback: Optional[Callable[[int, GmmOperands, GmmSums], None]] = None) -> "SpectralGMM":
        """One mixture per mask class: ``components = (k_background, k_foreground)`` fitted on the background and the foreground
        pixels (``fit`` with that ``select``; ``init`` a pair of inits or one string), concatenated into one model with classes 0
        and 1 whose weights are the class priors -- the pixel counts' shares -- times the weights inside the class.  ``(1, 1)`` is the
        Gaussian maximum-likelihood classifier: exactly one pass per class.  ``pivot`` defaults to the fp32 mean of all pixels.
        ``callback(class, operands, sums)`` sees every pass."""
        idx = _slot_list(cache, slots)
        if len(components) != 2 or sum(int(k) for k in components) > MAX_K or min(int(k) for k in components) < 1:
            raise ValueError(f"SpectralGMM: components must be (k_background, k_foreground) with at most {MAX_K} in all, got {components!r}")
        w32 = _projection(projection, cache.C)
        if pivot is None:
            n, sums = band_moments(cache, idx, "all")
            pivot = (sums[:cache.C] / n).astype(np.float32)
        pivot = _vector32(pivot, cache.C, "SpectralGMM")
        inits = (init, init) if isinstance(init, str) else tuple(init)
        if len(inits) != 2:
            raise ValueError("SpectralGMM: fit_classes needs one init per class")
        fits = []
        with torch.cuda.device(cache.device):
            for c, select in enumerate(("background", "foreground")):
                k = int(components[c])
                ps = _GmmPass(cache, idx, w32.shape[0], k)
                cb = None if callback is None else (lambda ops, s, c=c: callback(c, ops, s))
                fits.append(cls._fit_one(cache, ps, idx, _check_select(select), pivot, w32, k, inits[c], max_iter, tol, reg_covar,
                                         int(seed) + c, None, cb))
        return cls(pivot, w32, *_concatenate(fits)).to(cache.device)

    # ---- prediction ---------------------------------------------------------------------------------
    def _device(self, device, cs: int):
        key = (str(device), cs) + self._key()
        if self._dev is None or self._dev[0] != key:
            self._dev = (key, _device_operands(self.operands, device, cs))
        return self._dev[1]

    def forward(self, x, output: str = "logit"):
        if isinstance(x, dict):
            x = x['image']
        if output not in OUTPUTS:
            raise ValueError(f"SpectralGMM: output must be one of {OUTPUTS}, got {output!r}")
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("hyperpri_amd: SpectralGMM needs a tensor on a ROCm device; there is no CPU fallback")
        if x.requires_grad:
            raise RuntimeError("SpectralGMM: no autograd -- the input must not require grad")
        if x.dtype != torch.float32:
            raise ValueError(f"SpectralGMM: need a float32 image, got {x.dtype}")
        five = x.dim() == 5
        if five and x.shape[1] != 1 or x.dim() not in (4, 5):
            raise ValueError(f"SpectralGMM: need an (N, 1, C, h, w) or (N, C, h, w) image, got {tuple(x.shape)}")
        t = x[:, 0] if five else x
        if getattr(x, "_hpri_zero_padded", False):
            t._hpri_zero_padded = True
        N, C, h, w = (int(s) for s in t.shape)
        if C != self.in_channels:
            raise ValueError(f"SpectralGMM: the image has {C} bands, the model {self.in_channels}")
        if N * h * w == 0:
            raise ValueError("SpectralGMM: empty image")
        ops = self.operands
        nc = ops.n_classes
        if output == "logit" and nc != 2:
            raise ValueError(f"SpectralGMM: output='logit' needs exactly two classes, the model has {nc}")
        with torch.cuda.device(x.device):
            src, cs = _band_input(t)
            if cs > max_channel_stride():
                raise ValueError(f"SpectralGMM: a channel stride of {cs} exceeds the {max_channel_stride()} the kernels take")
            pv, wd, A, a, cst, _ = self._device(x.device, cs)
            planes = {"loglik": nc, "resp": self.k}.get(output, 1)
            out = torch.empty((N, planes, h, w), dtype=torch.uint8 if output == "labels" else torch.float32, device=x.device)
            ptr = {name: None for name in OUTPUTS}
            ptr[output] = _p(out)
            classes = (ctypes.c_int * self.k)(*[int(v) for v in ops.classes])
            _lib.call("hpri_band_gmm_score", _p(src), N * h * w, h * w, cs, _p(pv), _p(wd), self.q, _p(A), _p(a), _p(cst),
                      ctypes.cast(classes, ctypes.c_void_p), self.k, nc, ptr["loglik"], ptr["logit"], ptr["labels"], ptr["resp"], ptr["nll"],
                      _stream())
        return out


def _meta(f: GmmFit):
    return (f.n_iter, f.history[-1], 1.0 if f.converged else 0.0, float(sum(1 << k for k in f.starved)))


def _concatenate(fits: Sequence[GmmFit]):
    """(means, covariances, joint weights, classes, meta) of one model from one fit per class: the priors are the counts' shares."""
    total = float(sum(f.count for f in fits))
    means = np.concatenate([f.means for f in fits])
    cov = np.concatenate([f.covariances for f in fits])
    pi = np.concatenate([f.weights * (f.count / total) for f in fits])
    classes = np.concatenate([np.full(len(f.means), c, dtype=np.int64) for c, f in enumerate(fits)])
    starved, base = 0, 0
    for f in fits:
        starved |= sum(1 << (base + k) for k in f.starved)
        base += len(f.means)
    meta = (max(f.n_iter for f in fits), sum(f.history[-1] * f.count for f in fits) / total, float(all(f.converged or len(f.means) == 1 for f in fits)),
            float(starved))
    return means, cov, pi, classes, meta


# ---------------------------------------------------------------------------------------------------
# The contract restated in numpy: the oracles of the GPU tests, and what fp32 rounding may do
# ---------------------------------------------------------------------------------------------------
def _lse(l: np.ndarray) -> np.ndarray:
    mx = l.max(axis=1)
    return mx + np.log(np.exp(l - mx[:, None]).sum(axis=1))


def _terms(x, ops: GmmOperands, cs: Optional[int] = None, bounds: bool = False) -> Dict[str, np.ndarray]:
    """Every quantity of the contract on (..., C) fp32 pixels in fp64 and, with ``bounds``, what fp32 rounding may do to it."""
    x = np.asarray(x)
    C = x.shape[-1]
    q, K = ops.q, ops.k
    qp = _rup(q, 8)
    cs = _rup(C, 8) if cs is None else int(cs)
    d = (x.reshape(-1, C).astype(np.float32) - ops.pivot).astype(np.float64)                 # one IEEE subtraction in fp32, as the device's
    W, A, a, c = (v.astype(np.float64) for v in (ops.weight, ops.A, ops.a, ops.c))
    z = d @ W.T
    u = np.einsum("kij,pj->pki", A, z) + a[None]
    m = (u * u).sum(axis=2)
    l = c[None] - 0.5 * m
    out = {"d": d, "z": z, "u": u, "m": m, "l": l, "nll": -_lse(l)}
    nc = ops.n_classes
    L = np.full((len(d), nc), -np.inf)
    for cl in range(nc):
        members = np.nonzero(ops.classes == cl)[0]
        if len(members):
            L[:, cl] = _lse(l[:, members])
    out["loglik"] = L
    out["labels"] = np.argmax(L, axis=1).astype(np.int64)                                       # (the first, that is the lowest, index of the maximum)
    out["resp"] = np.exp(l + out["nll"][:, None])
    if nc == 2:
        out["logit"] = L[:, 1] - L[:, 0]
    if not bounds:
        return out
    Ez = (cs + 1) * U * (np.abs(d) @ np.abs(W).T)                                                # a chain of cs fused multiply-adds
    zz = np.abs(z) + Ez
    Eu = (qp + 1) * U * (np.abs(a)[None] + np.einsum("kij,pj->pki", np.abs(A), zz)) + np.einsum("kij,pj->pki", np.abs(A), Ez)
    uu = np.abs(u) + Eu
    Em = (Eu * (2 * np.abs(u) + Eu)).sum(axis=2) + (qp + 3) * U * (uu * uu).sum(axis=2)        # at most 8 + 2 roundings per sum
    El = 0.5 * Em + U * (np.abs(l) + 0.5 * Em)

    def lse_bound(cols, value):
        # log-sum-exp is 1-Lipschitz in the sup norm; its evaluation: the argument l - mx rounds once, expf, a sum of n positive
        # terms, logf of a sum in [1, n], the last addition; 2^-140 covers terms that underflow
        ll, ee = l[:, cols], El[:, cols]
        emax = ee.max(axis=1)
        spread = ll.max(axis=1) - ll.min(axis=1) + 2 * emax
        delta = np.expm1(U * spread) + 2 * U * EXP_ULP + (len(cols) - 1) * U
        elog = 1.01 * delta + 2 * U * LOG_ULP * math.log(max(len(cols), 2)) + 2.0 ** -140
        return emax + elog + U * (np.abs(value) + emax + elog)
    EL = np.zeros_like(L)
    for cl in range(nc):
        members = np.nonzero(ops.classes == cl)[0]
        if len(members):
            EL[:, cl] = lse_bound(members, L[:, cl])
    Eall = lse_bound(np.arange(K), out["nll"])
    # r_k = e_k / sum e_j: every e_j = expf(l_j - mx) carries the error of l_j, of mx, of the rounded difference and of expf; the
    # ratio at most doubles the largest; then K - 1 additions and a division (within 2 ulp)
    arg = El + El.max(axis=1)[:, None] + U * (l.max(axis=1)[:, None] - l + 2 * El.max(axis=1)[:, None])
    delta = (np.expm1(arg) + 2 * U * EXP_ULP * np.exp(arg)).max(axis=1)
    Er = out["resp"] * ((1 + delta) / (1 - delta) - 1 + (K + 4) * U * (1 + 4 * delta))[:, None] + 2.0 ** -140
    out.update({"Ez": Ez, "Eu": Eu, "Em": Em, "El": El, "Eloglik": EL, "Enll": Eall, "Eresp": Er})
    if nc == 2:
        out["Elogit"] = (EL[:, 0] + EL[:, 1]) * (1 + U) + U * np.abs(out["logit"])
    # a label the bound cannot flip: the runner-up lies further below than both bounds together
    rows = np.arange(len(d))
    gap = L[rows, out["labels"]][:, None] - L
    close = gap <= EL + EL[rows, out["labels"]][:, None]
    close[rows, out["labels"]] = False
    out["ambiguous"] = close.any(axis=1)
    return out


def gmm_score_reference(x, operands: GmmOperands) -> Dict[str, np.ndarray]:
    """``hpri_band_gmm_score`` in fp64 numpy on (..., C) fp32 pixels, from the fp32 operands the kernel receives: ``z`` (P, q), ``m``
    and ``l`` (P, K), ``loglik`` (P, C), ``labels`` (P,) -- the lowest class at the maximum --, ``resp`` (P, K), ``nll`` (P,) and, with
    two classes, ``logit`` (P,)."""
    return _terms(x, operands)


def gmm_bound(x, operands: GmmOperands, cs: Optional[int] = None) -> Dict[str, np.ndarray]:
    """``gmm_score_reference`` plus elementwise bounds on what the device may return, derived from the fp32 rounding model
    (``u = 2^-24``; a chain of n fused multiply-adds: ``(n + 1) u`` times the sum of the magnitudes, as ``score_bound``): ``Ez``, ``Em``,
    ``El``, ``Eloglik``, ``Elogit``, ``Eresp``, ``Enll``, and ``ambiguous`` -- the pixels whose label the bound can flip.  The device's
    ``expf`` and ``logf`` enter with ``EXP_ULP`` and ``LOG_ULP`` units in the last place."""
    return _terms(x, operands, cs, bounds=True)


def gmm_sums_bound(x, operands: GmmOperands, cs: Optional[int] = None) -> GmmSums:
    """Bounds on the sums of ``gmm_step_reference`` over the (P, C) selected pixels ``x``, as a ``GmmSums`` (count 0): per pixel the
    error of ``e = fp32(z - m)``, of ``fp32(r e)`` and of their product, from ``gmm_bound``; the fp32 chain of a run adds
    ``FP32_RUN u`` times the magnitudes, the fp64 partials 1e-12 times them."""
    t = _terms(x, operands, cs, bounds=True)
    q, K = operands.q, operands.k
    mk = operands.means.astype(np.float64)
    e = t["z"][:, None, :] - mk[None]                                                         # (P, K, q)
    Ee = t["Ez"][:, None, :] + U * (np.abs(e) + t["Ez"][:, None, :])
    r, Er = t["resp"], t["Eresp"]
    ea = np.abs(e) + Ee
    Ere = Er[..., None] * ea + r[..., None] * Ee + U * (r + Er)[..., None] * ea              # of fp32(r e)
    re = r[..., None] * np.abs(e) + Ere
    chain = FP32_RUN * U + 1e-12
    EQ = np.einsum("pki,pkj->kij", Ere, ea) + np.einsum("pki,pkj->kij", r[..., None] * np.abs(e), Ee) + chain * np.einsum("pki,pkj->kij", re, ea)
    ES = (Ere + Er[..., None] * ea).sum(axis=0) + chain * re.sum(axis=0)
    EN = Er.sum(axis=0) + chain * (r + Er).sum(axis=0)
    ELL = t["Enll"].sum() + 1e-12 * np.abs(t["nll"]).sum()
    return GmmSums(0, EN, ES, EQ, float(ELL))


def gmm_step_reference(cubes, operands: GmmOperands, masks=None, select: str = "all") -> GmmSums:
    """``gmm_step`` in fp64 numpy on (n, H, W, C) ``cubes`` as the cache stores them."""
    x = _selected_pixels(cubes, masks, select)
    t = _terms(x, operands)
    e = t["z"][:, None, :] - operands.means.astype(np.float64)[None]
    r = t["resp"]
    return GmmSums(int(x.shape[0]), r.sum(axis=0), np.einsum("pk,pki->ki", r, e), np.einsum("pk,pki,pkj->kij", r, e, e), float(-t["nll"].sum()))


def gmm_reference(cubes, pivot, weight, init, masks=None, select: str = "all", max_iter: int = 100, tol: float = 1e-4,
                  reg_covar: float = 1e-6) -> GmmFit:
    """``SpectralGMM.fit`` from an explicit ``init = (means, covariances[, weights])``, in fp64 numpy: the same EM loop and stopping
    rule (``_em``)."""
    w32 = _projection(weight, np.asarray(cubes).shape[-1])
    pv = _vector32(pivot, w32.shape[1], "gmm_reference")
    k = len(init[0])
    pi0 = np.full(k, 1.0 / k) if len(init) == 2 else np.asarray(init[2], dtype=np.float64)

    def step(m, cov, pi):
        return gmm_step_reference(cubes, gmm_operands(pv, w32, m, cov, pi), masks, select)
    return _em(step, np.asarray(init[0], dtype=np.float32), np.asarray(init[1], dtype=np.float64), pi0, 1 if k == 1 else max_iter, tol, reg_covar)


def gmm_classes_reference(cubes, masks, pivot, weight, inits, max_iter: int = 100, tol: float = 1e-4, reg_covar: float = 1e-6):
    """``SpectralGMM.fit_classes`` from explicit inits (background, foreground), in fp64 numpy: ``(operands of the joint model, [fit of
    the background, fit of the foreground])``."""
    fits = [gmm_reference(cubes, pivot, weight, inits[c], masks, select, max_iter, tol, reg_covar)
            for c, select in enumerate(("background", "foreground"))]
    means, cov, pi, classes, _ = _concatenate(fits)
    return gmm_operands(pivot, _projection(weight, np.asarray(cubes).shape[-1]), means, cov, pi, classes), fits


__all__ = ["SpectralGMM", "GmmOperands", "GmmSums", "GmmFit", "gmm_operands", "merge_gmm_sums", "gmm_step", "hard_init", "gmm_score_reference",
           "gmm_step_reference", "gmm_reference", "gmm_classes_reference", "gmm_bound", "gmm_sums_bound", "workspace_bytes", "gmm_parts", "MAX_K", "MAX_Q", "OUTPUTS"]
