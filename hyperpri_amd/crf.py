"""Dense CRF refinement of score maps (``csrc/crf.hip``): windowed mean-field inference.

The guided filter smooths one map at a time and is linear in it.  A conditional random field iterates on the label distribution itself:
every pixel receives, from the neighbours that lie close and look alike, what they currently believe, the classes are coupled through a
compatibility matrix, and the softmax after each round sharpens as it smooths.  This is the fully connected CRF of Kraehenbuehl and
Koltun restricted to a (2r+1)^2 window -- the convolutional CRF of Teichmann and Cipolla --, exact inside the window: no permutohedral
lattice.  ``SpectralProjection`` makes the appearance features (one standardised principal component works best on the project's scenes),
the detectors, the unmixer or a network the unaries; ``evaluate.crf_split`` applies it to a stored split.

The contract (include/hyperpri_hip.h states it in full).  Unaries ``U`` (N, C, h, w) with 2 <= C <= 8, or binary logits ``z`` (N, h, w)
*defined* as ``U = (0, z)``; a guide ``I`` with K <= 3 channels (none: K = 0, and then ``w_appearance = 0``); ``1 <= r <= 8``,
``1 <= T <= 16``.  Host side, in fp64 rounded once to fp32: ``ta[d] = exp(-d^2 / 2 theta_alpha^2)``, ``tg[d] = exp(-d^2 / 2 theta_gamma^2)``,
``b = 1 / 2 theta_beta^2``.  Device side, fp32 in a fixed order:

    Q^0 = softmax(U)                        e_l = expf(L_l - max L), summed in class order, one division per class
    per iteration, pixel i, neighbour j = i + (dy, dx), dy ascending, dx ascending inside a row, the centre skipped, outside the image +0.0:
        s = fmaf(dI_c, dI_c, s), dI_c = I_j,c - I_i,c;   e = expf(-(s * b));   k = fmaf(ga, e, gs_)
        ga = (w_a ta[|dy|]) ta[|dx|],  gs_ = (w_s tg[|dy|]) tg[|dx|];          M_l = fmaf(k, Q_j(l), M_l)
    m_l = M_l / (float)(n - 1)              n the clipped window's pixels; n = 1: m = 0
    L_l = U_l - sum_l' mu(l, l') m_l'       Potts, mu = -Id: L_l = U_l + m_l
    Q^t = softmax(L)

The centre is skipped because mean field sums the messages of the *other* pixels; dividing by their number n - 1 makes ``w_appearance``
and ``w_smooth`` mean the same in a corner, at a border and inside.  ``crf_reference`` restates the contract in numpy on the same fp32
inputs, ``crf_bruteforce`` is the independent oracle (an explicit pairwise matrix and fp64 matrix products), ``crf_bound`` the
rounding-model bound.  No autograd, no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._args import _guide_frame, _int_arg, _p, _stream, _weight_arg
from .guided import SIGMOID_ULPS, U, _counts, _gamma, _guide_input, _shift

MAX_RADIUS = 8              # hpri_crf_max_radius
MAX_CLASSES = 8             # hpri_crf_max_classes
MAX_GUIDES = 3              # hpri_crf_max_guides
MAX_ITERATIONS = 16         # hpri_crf_max_iterations
CRF_OUTPUTS = ("logit", "prob")
TINY = 2.0 ** -126          # below the smallest normal fp32 number a result may be flushed or lose bits: an absolute allowance


def max_radius() -> int:
    """The largest radius the kernel takes (``hpri_crf_max_radius``)."""
    return int(_lib.load().hpri_crf_max_radius())


def max_classes() -> int:
    """The most classes the kernel takes (``hpri_crf_max_classes``)."""
    return int(_lib.load().hpri_crf_max_classes())


def max_guides() -> int:
    """The most guide channels the kernel takes (``hpri_crf_max_guides``)."""
    return int(_lib.load().hpri_crf_max_guides())


def max_iterations() -> int:
    """The most mean-field iterations of one call (``hpri_crf_max_iterations``)."""
    return int(_lib.load().hpri_crf_max_iterations())


def tile_shape() -> Tuple[int, int]:
    """(rows, columns) of the tile a workgroup owns (``hpri_crf_tile_h``, ``hpri_crf_tile_w``)."""
    lib = _lib.load()
    return int(lib.hpri_crf_tile_h()), int(lib.hpri_crf_tile_w())


# ---------------------------------------------------------------------------------------------------
# Arguments and host constants
# ---------------------------------------------------------------------------------------------------
def crf_tables(radius: int, theta_alpha: float, theta_beta: float, theta_gamma: float) -> Tuple[np.ndarray, np.ndarray, float]:
    """The host constants of the contract, made in fp64 and rounded once to fp32: ``(ta (r+1,), tg (r+1,), b)``."""
    d = np.arange(int(radius) + 1, dtype=np.float64)
    with np.errstate(over="ignore"):
        ta = np.exp(-(d * d) / (2.0 * float(theta_alpha) ** 2)).astype(np.float32)
        tg = np.exp(-(d * d) / (2.0 * float(theta_gamma) ** 2)).astype(np.float32)
        b = float(np.float32(1.0 / (2.0 * float(theta_beta) ** 2)))
    return ta, tg, b


def _crf_args(radius, iterations, theta_alpha, theta_beta, theta_gamma, w_appearance, w_smooth, output, who: str) -> dict:
    """The parameters as the launch takes them (the thetas stay Python floats: the tables are made from them in fp64)."""
    r = _int_arg(radius, 1, MAX_RADIUS, "radius", who)
    T = _int_arg(iterations, 1, MAX_ITERATIONS, "iterations", who)
    th = {}
    for name, v, inf in (("theta_alpha", theta_alpha, True), ("theta_beta", theta_beta, False), ("theta_gamma", theta_gamma, True)):
        x = float(v)
        if np.isnan(x) or x <= 0.0 or (np.isinf(x) and not inf):
            raise ValueError(f"{who}: {name} must be positive" + (" (inf is allowed)" if inf else " and finite") + f", got {v!r}")
        th[name] = x
    wa = _weight_arg(w_appearance, "w_appearance", who)
    ws = _weight_arg(w_smooth, "w_smooth", who)
    if output not in CRF_OUTPUTS:
        raise ValueError(f"{who}: output must be one of {CRF_OUTPUTS}, got {output!r}")
    ta, tg, b = crf_tables(r, th["theta_alpha"], th["theta_beta"], th["theta_gamma"])
    if not (b > 0.0 and np.isfinite(b)):
        raise ValueError(f"{who}: 1 / (2 theta_beta^2) must be positive and finite as an fp32 value, got theta_beta = {theta_beta!r}")
    return {"radius": r, "iterations": T, "w_appearance": wa, "w_smooth": ws, "output": output, "ta": ta, "tg": tg, "b": b, **th}


def _compat(compat, C: Optional[int], who: str) -> Optional[np.ndarray]:
    """``None`` (Potts) or a finite fp32 (C, C) matrix on the host."""
    if compat is None:
        return None
    mu = np.ascontiguousarray(compat.detach().cpu().numpy() if isinstance(compat, torch.Tensor) else compat, dtype=np.float32)
    if mu.ndim != 2 or mu.shape[0] != mu.shape[1] or not 2 <= mu.shape[0] <= MAX_CLASSES or (C is not None and mu.shape[0] != C):
        raise ValueError(f"{who}: compat must be a (C, C) matrix for C = {C if C is not None else f'2..{MAX_CLASSES}'} classes, got {mu.shape}")
    if not np.isfinite(mu).all():
        raise ValueError(f"{who}: compat must be finite")
    return mu


# ---------------------------------------------------------------------------------------------------
# The launch
# ---------------------------------------------------------------------------------------------------
def dense_crf(unary: torch.Tensor, guide: Optional[torch.Tensor], radius: int, iterations: int, theta_alpha: float, theta_beta: float,
              theta_gamma: float, w_appearance: float, w_smooth: float, compat=None, output: str = "logit") -> torch.Tensor:
    """Mean-field refinement of ``unary`` under ``guide``: ``iterations`` launches of ``hpri_dense_crf``'s kernel, nothing else.

    ``unary``: fp32 logits ``(N, C, h, w)`` with 2 <= C <= 8 on a ROCm device, or binary logits ``(N, h, w)`` (the two-class problem
    ``(0, z)``).  ``guide``: fp32 ``(N, K, h, w)`` or ``(N, 1, K, h, w)`` with K <= 3, in the layouts ``guided_filter`` reads (a
    ``SpectralProjection`` output zero-copy), or ``None`` (then ``w_appearance`` must be 0).  ``theta_alpha`` and ``theta_gamma`` may be
    ``inf``.  ``compat``: ``None`` for Potts, else a host-side (C, C) matrix.  ``output="logit"``: the last ``L`` in the unaries' shape
    (binary: ``L_1 - L_0``); ``"prob"``: the last ``Q`` (binary: ``Q_1``).  No autograd: an input that requires grad raises."""
    a = _crf_args(radius, iterations, theta_alpha, theta_beta, theta_gamma, w_appearance, w_smooth, output, "dense_crf")
    for t, what in ((unary, "unary"),) + (((guide, "guide"),) if guide is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"dense_crf: the {what} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"dense_crf: need float32 {what}, got {t.dtype}")
    binary = unary.dim() == 3
    if unary.dim() not in (3, 4) or (not binary and not 2 <= int(unary.shape[1]) <= MAX_CLASSES):
        raise ValueError(f"dense_crf: need unaries (N, C, h, w) with C in [2, {MAX_CLASSES}] or binary logits (N, h, w), got {tuple(unary.shape)}")
    N, h, w = int(unary.shape[0]), int(unary.shape[-2]), int(unary.shape[-1])
    C = 2 if binary else int(unary.shape[1])
    g, K = None, 0
    if guide is not None:
        g = _guide_frame(guide, MAX_GUIDES, "dense_crf", min_guides=0)
        K = int(g.shape[1])
        if (int(g.shape[0]), int(g.shape[2]), int(g.shape[3])) != (N, h, w):
            raise ValueError(f"dense_crf: need a guide on the unaries' frame {(N, h, w)}, got {tuple(guide.shape)}")
    if K == 0 and a["w_appearance"] != 0.0:
        raise ValueError("dense_crf: without a guide w_appearance must be 0")
    mu = _compat(compat, C, "dense_crf")
    if N * h * w == 0:
        raise ValueError("dense_crf: empty unaries")
    if not (unary.is_cuda and (K == 0 or guide.is_cuda)):
        raise RuntimeError("hyperpri_amd: dense_crf needs tensors on a ROCm device; there is no CPU fallback")
    if K and guide.device != unary.device:
        raise ValueError(f"dense_crf: the guide is on {guide.device}, the unaries on {unary.device}")
    if unary.requires_grad or (K and guide.requires_grad):
        raise RuntimeError("dense_crf: no autograd -- the inputs must not require grad")
    nbytes = int(_lib.load().hpri_crf_workspace_bytes(N, C, h, w))
    if nbytes == 0:
        raise ValueError(f"dense_crf: a frame of {(N, C, h, w)} exceeds the sizes the kernel takes")
    with torch.cuda.device(unary.device):
        src, gs = _guide_input(g) if K else (None, 0)
        u = unary if unary.is_contiguous() else unary.contiguous()
        T = a["iterations"]
        work = torch.empty((2, N, C, h, w), dtype=torch.float32, device=unary.device) if T > 1 else None
        out = torch.empty(tuple(unary.shape), dtype=torch.float32, device=unary.device)
        _lib.call("hpri_dense_crf", _p(u), int(binary), _p(src) if K else None, gs, K, N, C, h, w, a["radius"], T, a["ta"].ctypes.data,
                  a["tg"].ctypes.data, a["b"], a["w_appearance"], a["w_smooth"], mu.ctypes.data if mu is not None else None,
                  CRF_OUTPUTS.index(output), _p(work) if T > 1 else None, nbytes if T > 1 else 0, _p(out), _stream())
    return out


_STATE = ("radius", "iterations", "theta_alpha", "theta_beta", "theta_gamma", "w_appearance", "w_smooth")


class DenseCRF(torch.nn.Module):
    """``dense_crf`` with its parameters fixed: ``DenseCRF(radius, iterations, theta_alpha, theta_beta, theta_gamma, w_appearance,
    w_smooth, compat, output)(unary, guide)``.  The parameters travel in ``state_dict()`` (as the module's extra state: no tensor,
    nothing to move to a device); ``compat`` as a list of rows, or ``None``."""

    def __init__(self, radius: int, iterations: int, theta_alpha: float, theta_beta: float, theta_gamma: float, w_appearance: float,
                 w_smooth: float, compat=None, output: str = "logit"):
        super().__init__()
        self._set(radius, iterations, theta_alpha, theta_beta, theta_gamma, w_appearance, w_smooth, compat, output)

    def _set(self, radius, iterations, theta_alpha, theta_beta, theta_gamma, w_appearance, w_smooth, compat, output):
        a = _crf_args(radius, iterations, theta_alpha, theta_beta, theta_gamma, w_appearance, w_smooth, output, "DenseCRF")
        mu = _compat(compat, None, "DenseCRF")
        for k in _STATE:
            setattr(self, k, a[k])
        self.output = output
        self.compat = None if mu is None else mu.tolist()

    def get_extra_state(self):
        return {**{k: getattr(self, k) for k in _STATE}, "compat": self.compat, "output": self.output}

    def set_extra_state(self, state):
        self._set(*(state[k] for k in _STATE), state["compat"], state["output"])

    def extra_repr(self) -> str:
        return (f"radius={self.radius}, iterations={self.iterations}, theta_alpha={self.theta_alpha:g}, theta_beta={self.theta_beta:g}, "
                f"theta_gamma={self.theta_gamma:g}, w_appearance={self.w_appearance:g}, w_smooth={self.w_smooth:g}, "
                f"compat={'potts' if self.compat is None else 'matrix'}, output={self.output!r}")

    def forward(self, unary: torch.Tensor, guide: Optional[torch.Tensor] = None) -> torch.Tensor:
        return dense_crf(unary, guide, self.radius, self.iterations, self.theta_alpha, self.theta_beta, self.theta_gamma,
                         self.w_appearance, self.w_smooth, self.compat, self.output)


# ---------------------------------------------------------------------------------------------------
# The contract restated in numpy: the oracles of the tests
# ---------------------------------------------------------------------------------------------------
def _frames(unary, guide) -> Tuple[np.ndarray, np.ndarray, bool]:
    """fp32 inputs as fp64 arrays: the unaries as (N, h, w, C) (binary logits as (0, z)), the guide as (N, h, w, K), and whether the
    unaries were binary."""
    Un = np.asarray(unary.detach().cpu().numpy() if isinstance(unary, torch.Tensor) else unary)
    binary = Un.ndim == 3
    if binary:
        Un = np.stack([np.zeros_like(Un), Un], axis=1)
    if Un.ndim != 4 or not 2 <= Un.shape[1] <= MAX_CLASSES or Un.size == 0:
        raise ValueError(f"crf: need unaries (N, C, h, w) with C in [2, {MAX_CLASSES}] or binary logits (N, h, w), got {Un.shape}")
    N, C, h, w = Un.shape
    if guide is None:
        I = np.zeros((N, 0, h, w), dtype=np.float32)
    else:
        I = np.asarray(guide.detach().cpu().numpy() if isinstance(guide, torch.Tensor) else guide)
        if I.ndim == 5 and I.shape[1] == 1:
            I = I[:, 0]
        if I.ndim != 4 or I.shape[1] > MAX_GUIDES or (I.shape[0],) + I.shape[2:] != (N, h, w):
            raise ValueError(f"crf: need a guide (N, K, h, w) or (N, 1, K, h, w) with K <= {MAX_GUIDES} on the unaries' frame, got {I.shape}")
    Un = Un.astype(np.float32).astype(np.float64).transpose(0, 2, 3, 1)
    I = I.astype(np.float32).astype(np.float64).transpose(0, 2, 3, 1)
    return np.ascontiguousarray(Un), np.ascontiguousarray(I), binary


def _fma(a, b, c, dtype):
    """``fmaf`` in ``dtype``: fp32 products are exact in fp64, so one fp64 addition and one rounding stand in for the single rounding."""
    if dtype is np.float32:
        return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)
    return a * b + c


def _softmax(L: np.ndarray, dtype) -> np.ndarray:
    """The contract's softmax over the last axis in ``dtype``: the maximum subtracted, the sum in class order, one division each."""
    L = L.astype(dtype)
    e = np.exp(L - L.max(axis=-1, keepdims=True))
    s = np.zeros(L.shape[:-1], dtype)
    for l in range(L.shape[-1]):
        s = s + e[..., l]
    return e / s[..., None]


def _pair_weights(a: dict) -> Tuple[np.ndarray, np.ndarray]:
    """``ga`` and ``gs_`` as (r+1, r+1) fp32 tables over (|dy|, |dx|): every product rounded, as the contract has it."""
    wa, ws = np.float32(a["w_appearance"]), np.float32(a["w_smooth"])
    return ((wa * a["ta"])[:, None] * a["ta"][None, :]).astype(np.float32), ((ws * a["tg"])[:, None] * a["tg"][None, :]).astype(np.float32)


def _offsets(r: int, centre: bool = False):
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy or dx or centre:
                yield dy, dx


def _kernels(I: np.ndarray, a: dict, dtype, centre: bool = False):
    """Per offset in the contract's order: ``(dy, dx, k, e, s b)`` with k (N, h, w) in ``dtype`` (a scalar without a guide)."""
    ga, gs_ = _pair_weights(a)
    Iw, K = I.astype(dtype), I.shape[3]
    out = []
    for dy, dx in _offsets(a["radius"], centre):
        A, S = dtype(ga[abs(dy), abs(dx)]), dtype(gs_[abs(dy), abs(dx)])
        if K:
            s = np.zeros(I.shape[:3], dtype)
            for c in range(K):
                d = _shift(Iw[..., c], dy, dx) - Iw[..., c]
                s = _fma(d, d, s, dtype)
            arg = s * dtype(a["b"])
            e = np.exp(-arg)
        else:
            arg, e = np.zeros(I.shape[:3], dtype), np.ones(I.shape[:3], dtype)
        out.append((dy, dx, _fma(A, e, S, dtype), e, arg))
    return out


def _mean_field(Un, I, a: dict, mu, dtype, variant: Optional[str] = None):
    """``(L, Q, [Q^1 .. Q^T])`` as (N, h, w, C) arrays in ``dtype``.  ``variant`` is for the tests that show the bound is not vacuous:
    "centre" includes the centre pixel, "n" divides by n instead of n - 1."""
    N, h, w, C = Un.shape
    Uw = Un.astype(dtype)
    kern = _kernels(I, a, dtype, centre=variant == "centre")
    den = _counts(h, w, a["radius"]) - (0.0 if variant == "n" else 1.0)
    Q, L, steps = _softmax(Uw, dtype), Uw, []
    for _ in range(a["iterations"]):
        M = np.zeros(Un.shape, dtype)
        for dy, dx, k, _, _ in kern:
            M = _fma(k[..., None], _shift(Q, dy, dx), M, dtype)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.where(den[None, :, :, None] > 0, M / den.astype(dtype)[None, :, :, None], dtype(0)).astype(dtype)
        if mu is None:
            L = Uw + m
        else:
            p = np.zeros(Un.shape, dtype)
            for k2 in range(C):
                p = _fma(mu[:, k2].astype(dtype), m[..., k2:k2 + 1], p, dtype)
            L = Uw - p
        Q = _softmax(L, dtype)
        steps.append(Q)
    return L, Q, steps


def _result(L, Q, steps, binary: bool, dtype) -> Dict[str, object]:
    def cf(x):
        return np.ascontiguousarray(x.astype(np.float64).transpose(0, 3, 1, 2))
    out = {"L": cf(L), "Q": cf(Q), "steps": [cf(q) for q in steps]}
    if binary:
        out["logit"] = (L[..., 1] - L[..., 0]).astype(np.float64)
        out["prob"] = out["Q"][:, 1]
    else:
        out["logit"], out["prob"] = out["L"], out["Q"]
    return out


def crf_reference(unary, guide, radius: int, iterations: int, theta_alpha: float, theta_beta: float, theta_gamma: float,
                  w_appearance: float, w_smooth: float, compat=None, dtype=np.float64, _variant: Optional[str] = None) -> Dict[str, object]:
    """The contract line by line in fp64 numpy on the same fp32 inputs and the same host constants (the fp32 tables, b and the rounded
    products ga and gs_); nothing else is rounded to fp32 on the way.  ``{"L": the last L (N, C, h, w), "Q": the last Q, "steps": [Q^1,
    .., Q^T], "logit" and "prob": what the launch returns for these inputs (binary: L_1 - L_0 and Q_1, (N, h, w))}``.

    ``dtype=numpy.float32``: the window sums (differences, fmaf chains, the exponential and its argument), the division, the update of
    L and the softmax in fp32: an emulation of the device that ``crf_bound`` must cover."""
    a = _crf_args(radius, iterations, theta_alpha, theta_beta, theta_gamma, w_appearance, w_smooth, "logit", "crf_reference")
    Un, I, binary = _frames(unary, guide)
    if I.shape[3] == 0 and a["w_appearance"] != 0.0:
        raise ValueError("crf_reference: without a guide w_appearance must be 0")
    mu = _compat(compat, Un.shape[3], "crf_reference")
    L, Q, steps = _mean_field(Un, I, a, mu, dtype, _variant)
    return _result(L, Q, steps, binary, dtype)


def crf_bruteforce(unary, guide, radius: int, iterations: int, theta_alpha: float, theta_beta: float, theta_gamma: float,
                   w_appearance: float, w_smooth: float, compat=None) -> Dict[str, object]:
    """The independent oracle for small images: per image an explicit (hw x hw) pairwise matrix from the closed-form kernels
    ``w_a exp(-|p_i - p_j|^2 / 2 theta_alpha^2 - |I_i - I_j|^2 / 2 theta_beta^2) + w_s exp(-|p_i - p_j|^2 / 2 theta_gamma^2)`` (the spatial
    factors and b as the host constants of the contract), zero outside the window and on the diagonal, then mean field as fp64 matrix
    products: ``Q <- softmax(U - ((P Q) / (row count)) mu^T)``.  The same keys as ``crf_reference``."""
    a = _crf_args(radius, iterations, theta_alpha, theta_beta, theta_gamma, w_appearance, w_smooth, "logit", "crf_bruteforce")
    Un, I, binary = _frames(unary, guide)
    N, h, w, C = Un.shape
    mu = _compat(compat, C, "crf_bruteforce")
    mu = -np.eye(C) if mu is None else mu.astype(np.float64)
    ga, gs_ = (t.astype(np.float64) for t in _pair_weights(a))
    r = a["radius"]
    yy, xx = (v.reshape(-1) for v in np.mgrid[0:h, 0:w])
    ady, adx = np.abs(yy[:, None] - yy[None, :]), np.abs(xx[:, None] - xx[None, :])
    win = (ady <= r) & (adx <= r) & ~np.eye(h * w, dtype=bool)
    cy, cx = np.minimum(ady, r), np.minimum(adx, r)
    cnt = win.sum(axis=1).astype(np.float64)
    Ls, Qs, steps = [], [], [[] for _ in range(a["iterations"])]
    for i in range(N):
        F = I[i].reshape(h * w, -1)
        d2 = ((F[:, None, :] - F[None, :, :]) ** 2).sum(axis=-1)
        P = np.where(win, ga[cy, cx] * np.exp(-d2 * a["b"]) + gs_[cy, cx], 0.0)
        Uf = Un[i].reshape(h * w, C)
        L = Uf
        Q = np.exp(Uf - Uf.max(axis=1, keepdims=True))
        Q /= Q.sum(axis=1, keepdims=True)
        for t in range(a["iterations"]):
            m = (P @ Q) / np.maximum(cnt, 1.0)[:, None]
            L = Uf - m @ mu.T
            Q = np.exp(L - L.max(axis=1, keepdims=True))
            Q /= Q.sum(axis=1, keepdims=True)
            steps[t].append(Q.reshape(h, w, C))
        Ls.append(L.reshape(h, w, C))
        Qs.append(Q.reshape(h, w, C))
    return _result(np.stack(Ls), np.stack(Qs), [np.stack(s) for s in steps], binary, np.float64)


def _softmax_rounding(L: np.ndarray) -> np.ndarray:
    """The relative error of the device's softmax of exact fp32 logits: ``x_l = L_l - max`` rounds once (``u |x_l|`` in the exponent),
    ``expf`` is allowed ``SIGMOID_ULPS u`` (the allowance of the project's sigmoid), the sum of C terms ``(C - 1) u``, the division u;
    a class carries its own exponential's error and the sum's, which is at most the largest of them."""
    x = np.abs(L - L.max(axis=-1, keepdims=True))
    d = (x + 1.0 + SIGMOID_ULPS) * U
    rel = d + d.max(axis=-1, keepdims=True) + (L.shape[-1] + 1) * U
    return rel / (1.0 - rel)


def _softmax_error(L: np.ndarray, Q: np.ndarray, eL: np.ndarray) -> np.ndarray:
    """The error of the device's Q against ``Q = softmax(L)`` when its logits are within ``eL``: ``Q'_l / Q_l = exp(d_l) / sum Q_l'
    exp(d_l')`` lies within ``exp(+-(eL_l + max eL))``, then the rounding of the softmax itself on top."""
    grow = np.expm1(eL + eL.max(axis=-1, keepdims=True))
    return Q * (grow + _softmax_rounding(L) * (1.0 + grow)) + TINY


def crf_bound(unary, guide, radius: int, iterations: int, theta_alpha: float, theta_beta: float, theta_gamma: float, w_appearance: float,
              w_smooth: float, compat=None) -> Dict[str, object]:
    """The rounding-model bound on the device against ``crf_reference``, iterated over t: ``{"L", "Q": (N, C, h, w), "steps": [the
    bound on Q^1 .. Q^T], "logit", "prob": in the launch's output shape}``.  With u = 2^-24:

    * Q^0: the softmax's own rounding (``_softmax_rounding``).
    * the kernel weight of a neighbour: the K differences round once and are squared (2 u each), the fmaf chain of K non-negative terms
      adds K u, the product ``s b`` u: the exponent ``a = s b`` is off by ``(K + 3) u a``, so ``e`` by ``e ((K + 3) a + SIGMOID_ULPS) u``
      with expf's allowance; ``k = fmaf(ga, e, gs_)`` carries ``ga`` times that and rounds once (``u k``).  ga and gs_ are the
      reference's own fp32 values.
    * ``M_l``: every term ``k Q_j`` carries ``ek (Q_j + eQ_j) + k eQ_j`` -- the previous iteration's error passes through the sum here --,
      and the chain of n - 1 fmaf over non-negative terms adds ``gamma(n - 1)`` times their sum.
    * the division rounds once; ``p_l`` is a chain of C fmaf (``gamma(C) sum |mu| (m + em)``; Potts: none, L = U + m is one addition),
      the subtraction rounds once.
    * the softmax passes ``eL`` on as ``Q expm1(eL_l + max eL)`` and adds its own rounding (``_softmax_error``)."""
    a = _crf_args(radius, iterations, theta_alpha, theta_beta, theta_gamma, w_appearance, w_smooth, "logit", "crf_bound")
    Un, I, binary = _frames(unary, guide)
    N, h, w, C = Un.shape
    K = I.shape[3]
    mu = _compat(compat, C, "crf_bound")
    amu = None if mu is None else np.abs(mu.astype(np.float64))
    kern = []
    for dy, dx, k, e, arg in _kernels(I, a, np.float64):
        ga = float(_pair_weights(a)[0][abs(dy), abs(dx)])
        ek = (ga * e * ((K + 3) * arg + SIGMOID_ULPS) * U if K else 0.0) + U * k
        kern.append((dy, dx, k, ek))
    cnt = _counts(h, w, a["radius"]) - 1.0
    den = np.maximum(cnt, 1.0)[None, :, :, None]
    gn = _gamma(cnt)[None, :, :, None]
    Q = _softmax(Un, np.float64)
    eQ = Q * _softmax_rounding(Un) + TINY
    L, eL, steps = Un, np.zeros(Un.shape), []
    for _ in range(a["iterations"]):
        M, eM, A = np.zeros(Un.shape), np.zeros(Un.shape), np.zeros(Un.shape)
        for dy, dx, k, ek in kern:
            Qj, eQj = _shift(Q, dy, dx), _shift(eQ, dy, dx)
            M += k[..., None] * Qj
            eM += ek[..., None] * (Qj + eQj) + k[..., None] * eQj
            A += (k + ek)[..., None] * (Qj + eQj)
        eM += gn * A
        live = (cnt > 0)[None, :, :, None]
        m = np.where(live, M / den, 0.0)
        em = np.where(live, eM / den + U * (m + eM / den), 0.0)
        if amu is None:
            L, ep = Un + m, em
        else:
            L = Un - m @ mu.astype(np.float64).T
            ep = em @ amu.T + _gamma(C) * ((m + em) @ amu.T)
        eL = ep + U * (np.abs(L) + ep)
        Q = _softmax(L, np.float64)
        eQ = _softmax_error(L, Q, eL)
        steps.append(eQ)
    out = _result(eL, eQ, steps, binary, np.float64)
    if binary:
        out["logit"] = eL[..., 0] + eL[..., 1] + U * (np.abs(L[..., 1] - L[..., 0]) + eL[..., 0] + eL[..., 1])
    return out


__all__ = ["dense_crf", "DenseCRF", "crf_reference", "crf_bruteforce", "crf_bound", "crf_tables", "tile_shape", "max_radius", "max_classes",
           "max_guides", "max_iterations", "MAX_RADIUS", "MAX_CLASSES", "MAX_GUIDES", "MAX_ITERATIONS", "CRF_OUTPUTS"]
