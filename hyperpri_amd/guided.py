"""Edge-preserving filtering of score maps (``csrc/guided.hip``): the guided filter of He, Sun and Tang.

The detectors, k-means and the unmixer judge a pixel by its own spectrum; their maps are speckled.  The standard answer in hyperspectral
classification smooths the per-pixel probability maps with a guided filter whose guide is the first one to three principal components
of the cube: a pixel's score is pulled towards its neighbours' only where the cube itself shows no edge.  ``band_statistics``,
``SpectralProjection.pca`` make the guide, the ``*_split`` functions the maps; this module is the filter between them, and
``evaluate.refine_split`` applies it to a stored split.  It also refines a network's logits, abundance planes and softmax planes: the
filter preserves sums, so filtered planes of a partition of unity still sum to one.

The contract (include/hyperpri_hip.h states it in full).  A guide ``I`` with K <= 3 channels, T maps ``p`` on the same frame, a radius
``1 <= r <= 8``, ``eps > 0``; the window of a pixel is the (2r+1)^2 square clipped to the image, ``n`` its in-image pixels:

    stage 1, per pixel k, centred on k itself:   dI_j = fp32(I_j - I_k),  dp_j = fp32(p_j - p_k)
        S1 = sum dI_j   S2 = sum dI_j dI_j^T   s = sum dp_j   Sp = sum dI_j dp_j          fp32, the window row by row
        fp64:  m = S1/n;  C = S2/n - m m^T;  c = Sp/n - m s/n;  a = (C + eps Id)^-1 c       (Cholesky; K = 1: one division)
        fp32 planes:  a (K),  mI = I_k + m (K),  mp = p_k + s/n
    stage 2, per pixel i:   q_i = (1/n_i) sum over k in window(i) of [ mp_k + a_k . (I_i - mI_k) ]      fp32, the same order

The usual route forms ``E[I I^T] - E[I] E[I]^T`` in fp32; a principal-component score has a mean far larger than its local variation and
that subtraction cancels.  Centred on the window's own centre pixel the differences are small and exact, and nothing cancels; stage 2
uses ``mp + a . (I - mI)`` and not ``mean(a) . I + mean(b)`` for the same reason.  ``domain="prob"`` reads ``sigmoid`` of stored logits
and writes ``logit(clamp(q, 2^-24, 1 - 2^-24))``, the clamp of the detectors and the unmixer.

``guided_reference`` restates the contract in fp64 numpy on the same fp32 inputs, ``guided_bruteforce`` is the independent oracle (a
ridge regression per window through ``numpy.linalg.lstsq``), ``guided_bound`` the rounding-model bound.  No autograd, no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib
from ._args import FILTER_DOMAINS, _filter_args, _guide_frame, _p, _stream

MAX_RADIUS = 8              # hpri_guided_max_radius
MAX_GUIDES = 3              # hpri_guided_max_guides
U = 2.0 ** -24
U64 = 2.0 ** -53
P_LO, P_HI = 2.0 ** -24, 1.0 - 2.0 ** -24
SIGMOID_ULPS = 4            # the device's fp32 sigmoid against the exact one: expf, an addition, a division, a product


def max_radius() -> int:
    """The largest radius the kernels take (``hpri_guided_max_radius``)."""
    return int(_lib.load().hpri_guided_max_radius())


def max_guides() -> int:
    """The most guide channels the kernels take (``hpri_guided_max_guides``)."""
    return int(_lib.load().hpri_guided_max_guides())


def tile_shape() -> Tuple[int, int]:
    """(rows, columns) of the tile a workgroup owns (``hpri_guided_tile_h``, ``hpri_guided_tile_w``)."""
    lib = _lib.load()
    return int(lib.hpri_guided_tile_h()), int(lib.hpri_guided_tile_w())


# ---------------------------------------------------------------------------------------------------
# The filter
# ---------------------------------------------------------------------------------------------------
def _guide_input(t: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """(N, K, h, w) -> a tensor whose memory is a channels-last (N, h, w, gs) buffer with the guide in its first K channels, and gs.
    Zero-copy on the strides ``_band_input`` takes zero-copy (a ``SpectralProjection`` output: gs = 8) and, as the kernels read the
    first K channels only, on any channels-last view and on a contiguous single plane (gs = 1); else one layout pass (gs = K)."""
    N, K, h, w = (int(s) for s in t.shape)
    st = t.stride()
    gs = int(st[3]) if w > 1 else (int(st[2]) if h > 1 else (int(st[0]) if N > 1 else K))
    if (gs >= K and (K == 1 or st[1] == 1) and (w == 1 or st[3] == gs) and (h == 1 or st[2] == w * gs)
            and (N == 1 or st[0] == h * w * gs) and t.data_ptr() % 4 == 0):
        return t, gs
    return t.permute(0, 2, 3, 1).contiguous(), K


def guided_filter(guide: torch.Tensor, maps: torch.Tensor, radius: int, eps: float, domain: str = "linear",
                  return_coefficients: bool = False):
    """The guided filter of ``maps`` under ``guide``: two launches (``hpri_guided_coeffs``, ``hpri_guided_apply``).

    ``guide``: fp32 ``(N, K, h, w)`` or ``(N, 1, K, h, w)`` with K <= 3 on a ROCm device -- a ``SpectralProjection`` output is read
    zero-copy, as is any channels-last view or a contiguous ``(N, 1, h, w)`` plane; anything else goes through one layout pass.
    ``maps``: fp32 ``(N, h, w)`` or ``(N, T, h, w)``; the output has their shape.  ``domain="prob"``: the maps are logits, filtered as
    probabilities and returned as logits.  ``return_coefficients``: also the fp32 ``(N, T, 2K+1, h, w)`` planes ``a | mI | mp`` of
    stage 1.  No autograd: an input that requires grad raises."""
    r, e, code = _filter_args(radius, eps, domain, MAX_RADIUS, "guided_filter")
    for t, what in ((guide, "guide"), (maps, "maps")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"guided_filter: the {what} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"guided_filter: need float32 {what}, got {t.dtype}")
    g = _guide_frame(guide, MAX_GUIDES, "guided_filter")
    N, K, h, w = (int(s) for s in g.shape)
    if maps.dim() not in (3, 4) or (int(maps.shape[0]), int(maps.shape[-2]), int(maps.shape[-1])) != (N, h, w):
        raise ValueError(f"guided_filter: need maps (N, h, w) or (N, T, h, w) on the guide's frame {(N, h, w)}, got {tuple(maps.shape)}")
    T = int(maps.shape[1]) if maps.dim() == 4 else 1
    if N * T * h * w == 0:
        raise ValueError("guided_filter: empty maps")
    if not (guide.is_cuda and maps.is_cuda):
        raise RuntimeError("hyperpri_amd: guided_filter needs tensors on a ROCm device; there is no CPU fallback")
    if guide.device != maps.device:
        raise ValueError(f"guided_filter: the guide is on {guide.device}, the maps on {maps.device}")
    if guide.requires_grad or maps.requires_grad:
        raise RuntimeError("guided_filter: no autograd -- the inputs must not require grad")
    nbytes = int(_lib.load().hpri_guided_workspace_bytes(N, T, h, w, K))
    if nbytes == 0:
        raise ValueError(f"guided_filter: a frame of {(N, T, h, w)} exceeds the sizes the kernels take")
    with torch.cuda.device(maps.device):
        src, gs = _guide_input(g)
        p = maps if maps.is_contiguous() else maps.contiguous()
        work = torch.empty((N, T, 2 * K + 1, h, w), dtype=torch.float32, device=maps.device)
        out = torch.empty(tuple(maps.shape), dtype=torch.float32, device=maps.device)
        _lib.call("hpri_guided_coeffs", _p(src), gs, K, _p(p), N, T, h, w, r, e, code, _p(work), nbytes, _stream())
        _lib.call("hpri_guided_apply", _p(src), gs, K, N, T, h, w, r, code, _p(work), nbytes, _p(out), _stream())
    return (out, work) if return_coefficients else out


class GuidedFilter(torch.nn.Module):
    """``guided_filter`` with its parameters fixed: ``GuidedFilter(radius, eps, domain)(guide, maps)``.  The parameters travel in
    ``state_dict()`` (as the module's extra state: no tensor, nothing to move to a device)."""

    def __init__(self, radius: int, eps: float, domain: str = "linear"):
        super().__init__()
        self.radius, self.eps, _ = _filter_args(radius, eps, domain, MAX_RADIUS, "GuidedFilter")
        self.domain = domain

    def get_extra_state(self):
        return {"radius": self.radius, "eps": self.eps, "domain": self.domain}

    def set_extra_state(self, state):
        self.radius, self.eps, _ = _filter_args(state["radius"], state["eps"], state["domain"], MAX_RADIUS, "GuidedFilter")
        self.domain = state["domain"]

    def extra_repr(self) -> str:
        return f"radius={self.radius}, eps={self.eps:g}, domain={self.domain!r}"

    def forward(self, guide: torch.Tensor, maps: torch.Tensor, return_coefficients: bool = False):
        return guided_filter(guide, maps, self.radius, self.eps, self.domain, return_coefficients)


# ---------------------------------------------------------------------------------------------------
# The contract restated in numpy: the oracles of the tests
# ---------------------------------------------------------------------------------------------------
def _frames(guide, maps) -> Tuple[np.ndarray, np.ndarray, bool]:
    """fp32 inputs as fp64 arrays: the guide as (N, h, w, K), the maps as (N, h, w, T), and whether the maps came without T."""
    I = np.asarray(guide.detach().cpu().numpy() if isinstance(guide, torch.Tensor) else guide)
    p = np.asarray(maps.detach().cpu().numpy() if isinstance(maps, torch.Tensor) else maps)
    if I.ndim == 5 and I.shape[1] == 1:
        I = I[:, 0]
    if I.ndim != 4 or not 1 <= I.shape[1] <= MAX_GUIDES:
        raise ValueError(f"guided: need a guide (N, K, h, w) or (N, 1, K, h, w) with K in [1, {MAX_GUIDES}], got {I.shape}")
    single = p.ndim == 3
    if single:
        p = p[:, None]
    if p.ndim != 4 or (p.shape[0],) + p.shape[2:] != (I.shape[0],) + I.shape[2:] or p.size == 0:
        raise ValueError(f"guided: need maps (N, h, w) or (N, T, h, w) on the guide's frame, got {p.shape} for a guide {I.shape}")
    I = I.astype(np.float32).astype(np.float64).transpose(0, 2, 3, 1)
    p = p.astype(np.float32).astype(np.float64).transpose(0, 2, 3, 1)
    return np.ascontiguousarray(I), np.ascontiguousarray(p), single


def _shift(X: np.ndarray, dy: int, dx: int) -> np.ndarray:
    """``X[:, y + dy, x + dx]`` of an (N, h, w, ...) array, zeros where that lies outside the image."""
    h, w = X.shape[1], X.shape[2]
    out = np.zeros_like(X)
    ys, xs = slice(max(0, -dy), max(0, min(h, h - dy))), slice(max(0, -dx), max(0, min(w, w - dx)))
    yt, xt = slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx)
    if ys.stop > ys.start and xs.stop > xs.start:
        out[:, ys, xs] = X[:, yt, xt]
    return out


def _window(h: int, w: int, r: int):
    """The window's offsets in the contract's order with, per offset, the (h, w) mask of the pixels whose neighbour is inside."""
    inside = np.ones((1, h, w), dtype=np.float64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            v = _shift(inside, dy, dx)[0] != 0
            if v.any():
                yield dy, dx, v


def _counts(h: int, w: int, r: int) -> np.ndarray:
    ny = np.minimum(np.arange(h) + r, h - 1) - np.maximum(np.arange(h) - r, 0) + 1
    nx = np.minimum(np.arange(w) + r, w - 1) - np.maximum(np.arange(w) - r, 0) + 1
    return (ny[:, None] * nx[None, :]).astype(np.float64)


def _sigmoid(z: np.ndarray) -> np.ndarray:
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _logit(q: np.ndarray) -> np.ndarray:
    c = np.clip(q, P_LO, P_HI)
    return np.log(c) - np.log1p(-c)


def _stage1_sums(I, p, r: int, dtype, ep=None) -> Dict[str, np.ndarray]:
    """The centred window sums in ``dtype`` (differences, products and running sums), with the sums of the absolute terms in fp64
    (what ``guided_bound`` multiplies the chain's unit by) and, with ``ep`` (N, h, w, T) -- the error the maps come with --, ``Ep = sum
    (ep_j + ep_k)`` and ``EIp = sum |dI_j| (ep_j + ep_k)``."""
    N, h, w, K = I.shape
    T = p.shape[3]
    Iw, pw = I.astype(dtype), p.astype(dtype)
    S1, S2 = np.zeros((N, h, w, K), dtype), np.zeros((N, h, w, K, K), dtype)
    s, Sp = np.zeros((N, h, w, T), dtype), np.zeros((N, h, w, T, K), dtype)
    A1, A2, As, Ap = (np.zeros(S1.shape), np.zeros(S2.shape), np.zeros(s.shape), np.zeros(Sp.shape))
    Ep, EIp = np.zeros(s.shape), np.zeros(Sp.shape)
    for dy, dx, v in _window(h, w, r):
        dI = np.where(v[None, :, :, None], _shift(Iw, dy, dx) - Iw, dtype(0))
        dp = np.where(v[None, :, :, None], _shift(pw, dy, dx) - pw, dtype(0))
        S1 += dI
        S2 += dI[..., :, None] * dI[..., None, :]
        s += dp
        Sp += dp[..., :, None] * dI[..., None, :]
        aI, ap = np.abs(dI.astype(np.float64)), np.abs(dp.astype(np.float64))
        A1 += aI
        A2 += aI[..., :, None] * aI[..., None, :]
        As += ap
        Ap += ap[..., :, None] * aI[..., None, :]
        if ep is not None:
            e = np.where(v[None, :, :, None], _shift(ep, dy, dx) + ep, 0.0)
            Ep += e
            EIp += e[..., :, None] * aI[..., None, :]
    return {"S1": S1.astype(np.float64), "S2": S2.astype(np.float64), "s": s.astype(np.float64), "Sp": Sp.astype(np.float64),
            "A1": A1, "A2": A2, "As": As, "Ap": Ap, "Ep": Ep, "EIp": EIp}


def _solve(S: Dict[str, np.ndarray], n: np.ndarray, eps: float):
    """The fp64 part of stage 1, operation by operation as the kernel performs it: ``(a (N, h, w, T, K), m (N, h, w, K), sn (N, h, w,
    T), C (N, h, w, K, K))``."""
    K, T = S["S1"].shape[-1], S["s"].shape[-1]
    nd = n[None, :, :]
    m = S["S1"] / nd[..., None]
    sn = S["s"] / nd[..., None]
    C = S["S2"] / nd[..., None, None] - m[..., :, None] * m[..., None, :]
    L = np.zeros(C.shape)
    for j in range(K):
        d = C[..., j, j] + eps
        for k in range(j):
            d = d - L[..., j, k] * L[..., j, k]
        L[..., j, j] = d if K == 1 else np.sqrt(d)
        for i in range(j + 1, K):
            e = C[..., j, i]
            for k in range(j):
                e = e - L[..., i, k] * L[..., j, k]
            L[..., i, j] = e / L[..., j, j]
    a = np.zeros(S["Sp"].shape)
    for t in range(T):
        z = [None] * K
        for i in range(K):
            z[i] = S["Sp"][..., t, i] / nd - m[..., i] * sn[..., t]
            for k in range(i):
                z[i] = z[i] - L[..., i, k] * z[k]
            z[i] = z[i] / L[..., i, i]                  # (K = 1: L holds A itself: one division)
        if K > 1:
            for i in range(K - 1, -1, -1):
                for k in range(i + 1, K):
                    z[i] = z[i] - L[..., k, i] * z[k]
                z[i] = z[i] / L[..., i, i]
        for i in range(K):
            a[..., t, i] = z[i]
    return a, m, sn, C


def _stage2(I, a, mI, mp, n, r: int, dtype) -> np.ndarray:
    """``q`` (N, h, w, T) from planes ``a`` (N, h, w, T, K), ``mI`` (N, h, w, K), ``mp`` (N, h, w, T) in ``dtype``."""
    N, h, w, K = I.shape
    Iw, aw, mIw, mpw = (x.astype(dtype) for x in (I, a, mI, mp))
    acc = np.zeros(mp.shape, dtype)
    for dy, dx, v in _window(h, w, r):
        ak, mIk, t = _shift(aw, dy, dx), _shift(mIw, dy, dx), _shift(mpw, dy, dx)
        for c in range(K):
            t = t + ak[..., c] * (Iw[..., c] - mIk[..., c])[..., None]
        acc += np.where(v[None, :, :, None], t, dtype(0))
    return (acc / n.astype(dtype)[None, :, :, None]).astype(np.float64)


def _planes(a, mI, mp) -> np.ndarray:
    """(N, T, 2K+1, h, w): the workspace's layout."""
    N, h, w, T, K = a.shape
    out = np.empty((N, T, 2 * K + 1, h, w))
    out[:, :, :K] = a.transpose(0, 3, 4, 1, 2)
    out[:, :, K:2 * K] = mI.transpose(0, 3, 1, 2)[:, None]
    out[:, :, 2 * K] = mp.transpose(0, 3, 1, 2)
    return out


def _reference_args(radius, eps, domain, who: str):
    r, e, code = _filter_args(radius, eps, domain, MAX_RADIUS, who)
    return r, e, bool(code)


def guided_reference(guide, maps, radius: int, eps: float, domain: str = "linear", dtype=np.float64) -> Dict[str, np.ndarray]:
    """The contract line by line in fp64 numpy on the same fp32 inputs (``eps`` as the fp32 value the launch receives); nothing is
    rounded to fp32 on the way.  ``{"q": the output in the maps' shape (domain "prob": the logit), "value": q before the logit (the
    same array in the linear domain), "planes": (N, T, 2K+1, h, w) = a | mI | mp, "count": (h, w) n}``.

    ``dtype=numpy.float32``: every window sum -- the differences, products and running sums of stage 1, the planes, terms and the
    running sum of stage 2 -- in fp32, everything else in fp64: an emulation of the device that ``guided_bound`` must cover."""
    r, e, prob = _reference_args(radius, eps, domain, "guided_reference")
    I, p, single = _frames(guide, maps)
    if prob:
        p = _sigmoid(p)
        if dtype is np.float32:
            p = p.astype(np.float32).astype(np.float64)
    n = _counts(I.shape[1], I.shape[2], r)
    a, m, sn, _ = _solve(_stage1_sums(I, p, r, dtype), n, e)
    mI, mp = I + m, p + sn
    value = _stage2(I, a, mI, mp, n, r, dtype).transpose(0, 3, 1, 2)
    q = _logit(value) if prob else value
    if single:
        q, value = q[:, 0], value[:, 0]
    return {"q": q, "value": value, "planes": _planes(a, mI, mp), "count": n}


def guided_apply_reference(guide, planes, radius: int) -> np.ndarray:
    """Stage 2 alone in fp64 on given (N, T, 2K+1, h, w) planes (the device's, for instance): ``q`` (N, T, h, w), linear domain."""
    planes = np.asarray(planes, dtype=np.float64)
    I, _, _ = _frames(guide, planes[:, :, 0])
    K = I.shape[3]
    a = planes[:, :, :K].transpose(0, 3, 4, 1, 2)
    mI = planes[:, 0, K:2 * K].transpose(0, 2, 3, 1)
    mp = planes[:, :, 2 * K].transpose(0, 2, 3, 1)
    n = _counts(I.shape[1], I.shape[2], int(radius))
    return _stage2(I, a, mI, mp, n, int(radius), np.float64).transpose(0, 3, 1, 2)


def guided_bruteforce(guide, maps, radius: int, eps: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The independent oracle, linear domain: per window the ridge regression ``min sum_j (a . I_j + b - p_j)^2 + eps n |a|^2`` through
    ``numpy.linalg.lstsq`` of the augmented system, then ``q_i`` = the mean over the window of ``a_k . I_i + b_k``.  ``(q (N, T, h,
    w), a (N, h, w, T, K), b (N, h, w, T))``; a Python loop over the pixels, for small images."""
    r, e, _ = _reference_args(radius, eps, "linear", "guided_bruteforce")
    I, p, _ = _frames(guide, maps)
    N, h, w, K = I.shape
    T = p.shape[3]
    a, b = np.zeros((N, h, w, T, K)), np.zeros((N, h, w, T))
    for i in range(N):
        for y in range(h):
            for x in range(w):
                ys, xs = slice(max(0, y - r), min(h, y + r + 1)), slice(max(0, x - r), min(w, x + r + 1))
                X, P = I[i, ys, xs].reshape(-1, K), p[i, ys, xs].reshape(-1, T)
                n = X.shape[0]
                A = np.zeros((n + K, K + 1))
                A[:n, :K], A[:n, K] = X, 1.0
                A[n:, :K] = np.sqrt(e * n) * np.eye(K)
                sol = np.linalg.lstsq(A, np.concatenate([P, np.zeros((K, T))]), rcond=None)[0]
                a[i, y, x], b[i, y, x] = sol[:K].T, sol[K]
    q = np.zeros((N, h, w, T))
    for i in range(N):
        for y in range(h):
            for x in range(w):
                ys, xs = slice(max(0, y - r), min(h, y + r + 1)), slice(max(0, x - r), min(w, x + r + 1))
                q[i, y, x] = (a[i, ys, xs] @ I[i, y, x] + b[i, ys, xs]).reshape(-1, T).mean(axis=0)
    return q.transpose(0, 3, 1, 2), a, b


def _gamma(k) -> np.ndarray:
    """k u / (1 - k u): k fp32 roundings in a row."""
    return k * U / (1.0 - k * U)


def guided_bound(guide, maps, radius: int, eps: float, domain: str = "linear") -> Dict[str, np.ndarray]:
    """The rounding-model bound on the device against ``guided_reference``: ``{"planes": (N, T, 2K+1, h, w), "value": the maps'
    shape}`` -- on the coefficient planes and on q before the logit (the logit's own slope is the test's, as for the detectors).
    Three kinds of terms, u = 2^-24:

    * chains: an fp32 sum of n terms, each a difference or a product of differences, is off by at most ``gamma(n + 3) sum |terms|``
      (the sums of absolute terms are computed here).  Domain "prob" adds what the maps come with: the device's sigmoid is within
      ``4 u p`` of the exact one, and ``dp`` carries that of both its pixels.
    * the solve: the errors of the sums pass through ``m = S1/n``, ``C = S2/n - m m^T``, ``c = Sp/n - m s/n`` term by term (the fp64
      cancellation there: ``4 2^-53`` of the terms), then ``|da|_2 <= |A^-1| (|dc|_2 + |dC|_F |a|_2) / (1 - |A^-1| |dC|_F)`` with
      ``|A^-1| = 1 / (lambda_min(C) + eps)``, plus the fp64 Cholesky solve itself, ``8 K^2 2^-53 cond(A) (1 + |a|_2)`` with
      ``cond(A) <= (tr C + eps) |A^-1| <= (tr C + eps) / eps``.
    * final roundings: each plane is rounded once (``u |value|``); in stage 2 the planes' errors pass through ``mp + a . (I - mI)``
      term by term (the subtraction ``I_i - mI_k`` rounds once, the K fmaf round once each), the n-term chain again, the division."""
    r, e, prob = _reference_args(radius, eps, domain, "guided_bound")
    I, p, single = _frames(guide, maps)
    ep = None
    if prob:
        p = _sigmoid(p)
        ep = SIGMOID_ULPS * U * p
    N, h, w, K = I.shape
    n = _counts(h, w, r)
    nd = n[None, :, :, None]
    S = _stage1_sums(I, p, r, np.float64, ep)
    a, m, sn, C = _solve(S, n, e)
    mI, mp = I + m, p + sn
    g = _gamma(n + 3)[None, :, :, None]
    eS1, eS2 = g * S["A1"], g[..., None] * S["A2"]
    es, eSp = g * S["As"] + (1 + g) * S["Ep"], g[..., None] * S["Ap"] + (1 + g[..., None]) * S["EIp"]
    em, esn = eS1 / nd, es / nd
    am = np.abs(m)
    eC = (eS2 / nd[..., None] + am[..., :, None] * em[..., None, :] + em[..., :, None] * am[..., None, :] + em[..., :, None] * em[..., None, :]
          + 4 * U64 * (np.abs(S["S2"]) / nd[..., None] + am[..., :, None] * am[..., None, :]))
    ec = (eSp / nd[..., None] + am[..., None, :] * esn[..., None] + np.abs(sn)[..., None] * em[..., None, :] + em[..., None, :] * esn[..., None]
          + 4 * U64 * (np.abs(S["Sp"]) / nd[..., None] + am[..., None, :] * np.abs(sn)[..., None]))
    lam = np.maximum(np.linalg.eigvalsh(C)[..., 0], 0.0)
    ainv = 1.0 / (lam + e)                                                          # (N, h, w)
    nE = np.sqrt((eC * eC).sum(axis=(-1, -2)))
    na = np.sqrt((a * a).sum(axis=-1))                                              # (N, h, w, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        shrink = np.where(ainv * nE < 1, 1.0 / (1.0 - ainv * nE), np.inf)
        ea = (ainv * shrink)[..., None] * (np.sqrt((ec * ec).sum(axis=-1)) + nE[..., None] * na)
    ea = ea + 8 * K * K * U64 * ((np.trace(C, axis1=-2, axis2=-1) + e) * ainv)[..., None] * (1 + na)
    # the planes as stored: one rounding each
    Ea = ea[..., None] + U * (np.abs(a) + ea[..., None])                            # (N, h, w, T, K)
    EmI = em + U * (np.abs(mI) + em)                                                # (N, h, w, K)
    Emp = esn + (ep if prob else 0.0)
    Emp = Emp + U * (np.abs(mp) + Emp)                                              # (N, h, w, T)
    # stage 2
    gK = _gamma(K)
    err, mag = np.zeros(mp.shape), np.zeros(mp.shape)
    for dy, dx, v in _window(h, w, r):
        ak, Eak = np.abs(_shift(a, dy, dx)), _shift(Ea, dy, dx)
        mIk, EmIk = _shift(mI, dy, dx), _shift(EmI, dy, dx)
        d = np.abs(I - mIk)                                                         # (N, h, w, K)
        Ed = EmIk + U * (d + EmIk)
        lin = (ak * d[..., None, :]).sum(axis=-1)
        tm = np.abs(_shift(mp, dy, dx)) + lin
        te = _shift(Emp, dy, dx) + (Eak * (d + Ed)[..., None, :] + ak * Ed[..., None, :]).sum(axis=-1) + gK * tm
        vv = v[None, :, :, None]
        err += np.where(vv, te, 0.0)
        mag += np.where(vv, tm + te, 0.0)
    gn = _gamma(n + 1)[None, :, :, None]
    eq = (err + gn * mag) / nd
    eq = eq + U * (np.abs(_stage2(I, a, mI, mp, n, r, np.float64)) + eq)
    eq = eq.transpose(0, 3, 1, 2)
    return {"planes": _planes(Ea, EmI, Emp), "value": eq[:, 0] if single else eq}


__all__ = ["guided_filter", "GuidedFilter", "guided_reference", "guided_apply_reference", "guided_bruteforce", "guided_bound", "tile_shape",
           "max_radius", "max_guides", "MAX_RADIUS", "MAX_GUIDES", "FILTER_DOMAINS"]
