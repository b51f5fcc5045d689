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


# ---------------------------------------------------------------------------------------------------
# The trainable CRF: crf_layer (an autograd function over hpri_dense_crf_train_forward / _backward) and CRFLayer
# ---------------------------------------------------------------------------------------------------
def _device_weight(v, name: str, who: str) -> torch.Tensor:
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.dim() != 0:
        raise ValueError(f"{who}: {name} must be a 0-d float32 tensor on the unaries' device, got "
                         f"{tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}")
    return v


class _CRFFunction(torch.autograd.Function):
    """``hpri_dense_crf_train_forward`` and ``hpri_dense_crf_backward``.  The tensors: unary, w_a (or None), w_s, compat (or None), the
    guide's buffer (or None); ``cfg`` holds what the launches take besides."""

    @staticmethod
    def forward(ctx, unary, w_a, w_s, compat, src, cfg):
        N, C, h, w, T, keep = cfg["N"], cfg["C"], cfg["h"], cfg["w"], cfg["iterations"], cfg["keep"]
        lib = _lib.load()
        with torch.cuda.device(unary.device):
            if keep:
                nbytes = int(lib.hpri_crf_train_workspace_bytes(N, C, h, w, T))
                work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=unary.device)      # (8-byte aligned: the fp64 sums lie in front)
            else:
                nbytes = int(lib.hpri_crf_workspace_bytes(N, C, h, w)) if T > 1 else 0
                work = torch.empty(nbytes // 4, dtype=torch.float32, device=unary.device) if T > 1 else None
            out = torch.empty(tuple(unary.shape), dtype=torch.float32, device=unary.device)
            _lib.call("hpri_dense_crf_train_forward", _p(unary), cfg["binary"], _p(src) if cfg["K"] else None, cfg["gs"], cfg["K"], N, C, h, w,
                      cfg["radius"], T, cfg["ta"].ctypes.data, cfg["tg"].ctypes.data, cfg["b"], _p(w_a) if w_a is not None else None, _p(w_s),
                      _p(compat) if compat is not None else None, cfg["output"], int(keep), _p(work) if work is not None else None, nbytes,
                      _p(out), _stream())
        if keep:
            ctx.cfg = cfg
            ctx.save_for_backward(unary, w_a, w_s, compat, src, work)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        cfg = ctx.cfg
        unary, w_a, w_s, compat, src, work = ctx.saved_tensors
        N, C, h, w, T = cfg["N"], cfg["C"], cfg["h"], cfg["w"], cfg["iterations"]
        need = ctx.needs_input_grad
        g = grad_out.contiguous().to(torch.float32)
        with torch.cuda.device(unary.device):
            gu = torch.empty_like(unary)
            gwa = torch.empty((), dtype=torch.float32, device=unary.device) if need[1] else None
            gws = torch.empty((), dtype=torch.float32, device=unary.device) if need[2] else None
            gmu = torch.empty((C, C), dtype=torch.float32, device=unary.device) if need[3] else None
            _lib.call("hpri_dense_crf_backward", _p(g), _p(unary), cfg["binary"], _p(src) if cfg["K"] else None, cfg["gs"], cfg["K"], N, C, h, w,
                      cfg["radius"], T, cfg["ta"].ctypes.data, cfg["tg"].ctypes.data, cfg["b"], _p(w_a) if w_a is not None else None, _p(w_s),
                      _p(compat) if compat is not None else None, cfg["output"], _p(work), work.numel() * 8, _p(gu),
                      _p(gwa) if gwa is not None else None, _p(gws) if gws is not None else None, _p(gmu) if gmu is not None else None,
                      _stream())
        return (gu if need[0] else None), gwa, gws, gmu, None, None


def crf_layer(unary: torch.Tensor, guide: Optional[torch.Tensor], w_appearance: Optional[torch.Tensor], w_smooth: torch.Tensor,
              compat: Optional[torch.Tensor], radius: int, iterations: int, theta_alpha: float, theta_beta: float, theta_gamma: float,
              output: str = "logit") -> torch.Tensor:
    """``dense_crf`` as a differentiable layer: the same kernel and, at the same parameter values, the same bits, with gradients through
    all ``iterations`` to ``unary`` and to whichever of ``w_appearance``, ``w_smooth`` and ``compat`` require grad (``csrc/crf_grad.hip``).

    ``w_appearance`` and ``w_smooth``: 0-d fp32 tensors on the unaries' device, read from device memory -- no ``.item()``, no host
    synchronisation, no upload; any finite value is taken (a negative weight is a repulsive CRF).  ``compat``: an fp32 ``(C, C)`` device
    tensor, or ``None`` for Potts.  Without a guide ``w_appearance`` must be ``None``.  NOT differentiable: the guide (one that requires
    grad raises) and the thetas.  With nothing requiring grad this is the forward alone and keeps no stack.  A double backward raises."""
    who = "crf_layer"
    a = _crf_args(radius, iterations, theta_alpha, theta_beta, theta_gamma, 0.0, 0.0, output, who)
    for t, what in ((unary, "unary"),) + (((guide, "guide"),) if guide is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who}: the {what} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"{who}: need float32 {what}, got {t.dtype}")
    binary = unary.dim() == 3
    if unary.dim() not in (3, 4) or (not binary and not 2 <= int(unary.shape[1]) <= MAX_CLASSES):
        raise ValueError(f"{who}: need unaries (N, C, h, w) with C in [2, {MAX_CLASSES}] or binary logits (N, h, w), got {tuple(unary.shape)}")
    N, h, w = int(unary.shape[0]), int(unary.shape[-2]), int(unary.shape[-1])
    C = 2 if binary else int(unary.shape[1])
    g, K = None, 0
    if guide is not None:
        g = _guide_frame(guide, MAX_GUIDES, who, min_guides=0)
        K = int(g.shape[1])
        if (int(g.shape[0]), int(g.shape[2]), int(g.shape[3])) != (N, h, w):
            raise ValueError(f"{who}: need a guide on the unaries' frame {(N, h, w)}, got {tuple(guide.shape)}")
    if K == 0 and w_appearance is not None:
        raise ValueError(f"{who}: without a guide w_appearance must be None (there is no appearance kernel)")
    if K:
        _device_weight(w_appearance, "w_appearance", who)
    _device_weight(w_smooth, "w_smooth", who)
    if compat is not None and (not isinstance(compat, torch.Tensor) or compat.dtype != torch.float32 or tuple(compat.shape) != (C, C)):
        raise ValueError(f"{who}: compat must be a float32 (C, C) tensor for C = {C} classes or None, got "
                         f"{tuple(compat.shape) if isinstance(compat, torch.Tensor) else type(compat).__name__}")
    if N * h * w == 0:
        raise ValueError(f"{who}: empty unaries")
    tensors = [unary, w_smooth] + ([guide, w_appearance] if K else []) + ([compat] if compat is not None else [])
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("hyperpri_amd: crf_layer needs tensors on a ROCm device; there is no CPU fallback")
    if any(t.device != unary.device for t in tensors):
        raise ValueError(f"{who}: the guide, the weights and compat must be on the unaries' device {unary.device}")
    if K and guide.requires_grad:
        raise RuntimeError(f"{who}: the guide is not differentiable -- it must not require grad")
    if int(_lib.load().hpri_crf_train_workspace_bytes(N, C, h, w, a["iterations"])) == 0:
        raise ValueError(f"{who}: a frame of {(N, C, h, w)} exceeds the sizes the kernel takes")
    with torch.cuda.device(unary.device):
        src, gs = _guide_input(g) if K else (None, 0)
    u = unary if unary.is_contiguous() else unary.contiguous()
    mu = compat if compat is None or compat.is_contiguous() else compat.contiguous()
    keep = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (unary, w_appearance, w_smooth, compat))
    cfg = {"N": N, "C": C, "h": h, "w": w, "K": K, "gs": gs, "binary": int(binary), "radius": a["radius"], "iterations": a["iterations"],
           "ta": a["ta"], "tg": a["tg"], "b": a["b"], "output": CRF_OUTPUTS.index(output), "keep": keep}
    return _CRFFunction.apply(u, w_appearance if K else None, w_smooth, mu, src.detach() if K else None, cfg)


_LAYER_STATE = ("radius", "iterations", "theta_alpha", "theta_beta", "theta_gamma")


class CRFLayer(torch.nn.Module):
    """``crf_layer`` as a module: ``CRFLayer(radius, iterations, theta_alpha, theta_beta, theta_gamma, w_appearance, w_smooth, compat=None,
    output="logit", learn_compat=False)(unary, guide)``.  ``w_appearance`` and ``w_smooth`` are 0-d fp32 ``nn.Parameter`` s;
    ``w_appearance=None`` makes a layer without a guide (the weight is fixed at 0 and is no parameter).  ``compat`` is a parameter with
    ``learn_compat=True``, else it travels with the rest in the extra state.  ``frozen()`` returns the ``DenseCRF`` with the current
    values (non-negative weights only); ``CRFLayer.from_crf`` goes the other way."""

    def __init__(self, radius: int, iterations: int, theta_alpha: float, theta_beta: float, theta_gamma: float,
                 w_appearance: Optional[float], w_smooth: float, compat=None, output: str = "logit", learn_compat: bool = False):
        super().__init__()
        a = _crf_args(radius, iterations, theta_alpha, theta_beta, theta_gamma, 0.0, 0.0, output, "CRFLayer")
        for name, v in (("w_appearance", w_appearance), ("w_smooth", w_smooth)):
            if v is not None and not np.isfinite(float(np.float32(float(v)))):
                raise ValueError(f"CRFLayer: {name} must be finite as an fp32 value, got {v!r}")
        mu = _compat(compat, None, "CRFLayer")
        if learn_compat and mu is None:
            raise ValueError("CRFLayer: learn_compat needs a compat matrix to start from (Potts is -numpy.eye(C))")
        self.w_appearance = None if w_appearance is None else torch.nn.Parameter(torch.tensor(float(w_appearance), dtype=torch.float32))
        self.w_smooth = torch.nn.Parameter(torch.tensor(float(w_smooth), dtype=torch.float32))
        self.learn_compat = bool(learn_compat)
        if self.learn_compat:
            self.compat = torch.nn.Parameter(torch.from_numpy(mu.copy()))
        else:
            self.compat = None
            self.register_buffer("_fixed_compat", None if mu is None else torch.from_numpy(mu.copy()), persistent=False)
        self._set(a, output, None if mu is None or self.learn_compat else mu.tolist())

    def _set(self, a, output, fixed):
        for k in _LAYER_STATE:
            setattr(self, k, a[k])
        self.output = output
        self.fixed_compat = fixed

    def get_extra_state(self):
        return {**{k: getattr(self, k) for k in _LAYER_STATE}, "output": self.output, "learn_compat": self.learn_compat,
                "compat": self.fixed_compat}

    def set_extra_state(self, state):
        if bool(state["learn_compat"]) != self.learn_compat:
            raise ValueError(f"CRFLayer: the state was saved with learn_compat={state['learn_compat']}, this layer has {self.learn_compat}")
        a = _crf_args(*(state[k] for k in _LAYER_STATE), 0.0, 0.0, state["output"], "CRFLayer")
        mu = None if self.learn_compat else _compat(state["compat"], None, "CRFLayer")
        if not self.learn_compat:
            self._fixed_compat = None if mu is None else torch.from_numpy(mu.copy()).to(self.w_smooth.device)
        self._set(a, state["output"], None if mu is None else mu.tolist())

    def extra_repr(self) -> str:
        kind = "learned" if self.learn_compat else ("potts" if self.fixed_compat is None else "matrix")
        return (f"radius={self.radius}, iterations={self.iterations}, theta_alpha={self.theta_alpha:g}, theta_beta={self.theta_beta:g}, "
                f"theta_gamma={self.theta_gamma:g}, guide={self.w_appearance is not None}, compat={kind}, output={self.output!r}")

    def forward(self, unary: torch.Tensor, guide: Optional[torch.Tensor] = None) -> torch.Tensor:
        if (guide is None) != (self.w_appearance is None):
            raise ValueError("CRFLayer: a layer made with w_appearance takes a guide, one made with w_appearance=None takes none")
        return crf_layer(unary, guide, self.w_appearance, self.w_smooth, self.compat if self.learn_compat else self._fixed_compat,
                         self.radius, self.iterations, self.theta_alpha, self.theta_beta, self.theta_gamma, self.output)

    def frozen(self) -> "DenseCRF":
        """The ``DenseCRF`` with the layer's current values (read from the device once)."""
        mu = self.compat.detach().cpu().numpy() if self.learn_compat else self.fixed_compat
        return DenseCRF(self.radius, self.iterations, self.theta_alpha, self.theta_beta, self.theta_gamma,
                        0.0 if self.w_appearance is None else float(self.w_appearance.detach().cpu()), float(self.w_smooth.detach().cpu()),
                        mu, self.output)

    @classmethod
    def from_crf(cls, crf: "DenseCRF", guided: bool = True, learn_compat: bool = False) -> "CRFLayer":
        """The layer that starts at a ``DenseCRF``'s values; ``guided=False`` (only with ``w_appearance == 0``) makes one without a guide."""
        if not guided and crf.w_appearance != 0.0:
            raise ValueError("CRFLayer.from_crf: guided=False needs a DenseCRF with w_appearance = 0")
        return cls(crf.radius, crf.iterations, crf.theta_alpha, crf.theta_beta, crf.theta_gamma, crf.w_appearance if guided else None,
                   crf.w_smooth, crf.compat, crf.output, learn_compat)


# ---------------------------------------------------------------------------------------------------
# The backward's contract restated in numpy, and its rounding model
# ---------------------------------------------------------------------------------------------------
def _adjoint_kernels(I: np.ndarray, a: dict, dtype, centre: bool = False):
    """Per offset in the contract's order: ``(dy, dx, ka, ps, e, s b, pa)`` -- ``ka = (ta[|dy|] ta[|dx|]) e`` as (N, h, w) in ``dtype`` (0
    without a guide), ``ps = tg[|dy|] tg[|dx|]`` and ``pa = ta[|dy|] ta[|dx|]`` as fp32 scalars in ``dtype``."""
    PA = (a["ta"][:, None] * a["ta"][None, :]).astype(np.float32)
    PS = (a["tg"][:, None] * a["tg"][None, :]).astype(np.float32)
    out = []
    for dy, dx, _, e, arg in _kernels(I, a, dtype, centre):
        pa, ps = dtype(PA[abs(dy), abs(dx)]), dtype(PS[abs(dy), abs(dx)])
        ka = (pa * e).astype(dtype) if I.shape[3] else np.zeros(I.shape[:3], dtype)
        out.append((dy, dx, ka, ps, e, arg, pa))
    return out


def _grad_frames(grad_output, Un: np.ndarray, binary: bool, output: str) -> np.ndarray:
    """The output's gradient as the (N, h, w, C) vector the backward starts from: binary logit (-g, +g), binary prob (0, g)."""
    g = np.asarray(grad_output.detach().cpu().numpy() if isinstance(grad_output, torch.Tensor) else grad_output)
    g = g.astype(np.float32).astype(np.float64)
    N, h, w, C = Un.shape
    if g.shape != ((N, h, w) if binary else (N, C, h, w)):
        raise ValueError(f"crf: the output's gradient must have the output's shape {(N, h, w) if binary else (N, C, h, w)}, got {g.shape}")
    if binary:
        return np.stack([-g if output == "logit" else np.zeros_like(g), g], axis=-1)
    return np.ascontiguousarray(g.transpose(0, 2, 3, 1))


def _softmax_adjoint(Q, gQ, dtype, inner: bool = True):
    """``d = fmaf(Q_l, gQ_l, d)`` over l ascending; ``Q_l (gQ_l - d)``."""
    d = np.zeros(Q.shape[:-1], dtype)
    if inner:
        for l in range(Q.shape[-1]):
            d = _fma(Q[..., l], gQ[..., l], d, dtype)
    return (Q * (gQ - d[..., None])).astype(dtype)


def _mu_t(mu, X, dtype):
    """``-(fmaf(mu(l, k), X_l, .) over l ascending)`` for every k: ``-mu^T X``; Potts (``mu`` None): X itself."""
    if mu is None:
        return X
    out = np.zeros(X.shape, dtype)
    for k in range(X.shape[-1]):
        p = np.zeros(X.shape[:-1], dtype)
        for l in range(X.shape[-1]):
            p = _fma(dtype(mu[l, k]), X[..., l], p, dtype)
        out[..., k] = -p
    return out


def _dot(A, Q, dtype):
    s = np.zeros(Q.shape[:-1], dtype)
    for l in range(Q.shape[-1]):
        s = _fma(A[..., l], Q[..., l], s, dtype)
    return s


def crf_backward_reference(unary, guide, grad_output, radius: int, iterations: int, theta_alpha: float, theta_beta: float,
                           theta_gamma: float, w_appearance: float, w_smooth: float, compat=None, output: str = "logit", dtype=np.float64,
                           _variant: Optional[str] = None) -> Dict[str, object]:
    """The backward's contract (include/hyperpri_hip.h) line by line in fp64 numpy on ``crf_reference``'s inputs and constants, for the
    output's gradient ``grad_output``: ``{"unary": dL/dU in the unaries' shape, "w_appearance", "w_smooth": floats, "compat": (C, C) or
    None}``.  Any finite weight is taken.  ``dtype=numpy.float32`` emulates the device (the parameter sums in fp64, rounded once);
    ``_variant`` is for the tests that show the bound is not vacuous."""
    a = _crf_args(radius, iterations, theta_alpha, theta_beta, theta_gamma, 0.0, 0.0, output, "crf_backward_reference")
    wa32, ws32 = np.float32(w_appearance), np.float32(w_smooth)
    if not (np.isfinite(wa32) and np.isfinite(ws32)):
        raise ValueError("crf_backward_reference: the weights must be finite as fp32 values")
    a["w_appearance"], a["w_smooth"] = float(wa32), float(ws32)
    Un, I, binary = _frames(unary, guide)
    N, h, w, C = Un.shape
    K = I.shape[3]
    if K == 0 and a["w_appearance"] != 0.0:
        raise ValueError("crf_backward_reference: without a guide w_appearance must be 0")
    mu = _compat(compat, C, "crf_backward_reference")
    T = a["iterations"]
    _, _, steps = _mean_field(Un, I, a, mu, dtype)
    Qs = [_softmax(Un.astype(dtype), dtype)] + steps                                  # Q^0 .. Q^T
    gv = _grad_frames(grad_output, Un, binary, output).astype(dtype)
    gL = gv if output == "logit" else _softmax_adjoint(Qs[T], gv, dtype)
    kern = _adjoint_kernels(I, a, dtype, centre=_variant == "centre")
    den = _counts(h, w, a["radius"]) - 1.0
    live = (den > 0)[None, :, :, None]
    dend = np.maximum(den, 1.0).astype(dtype)[None, :, :, None]
    wa, ws = dtype(wa32), dtype(ws32)
    mu_b = mu if (mu is None or _variant != "mu") else mu.T.copy()
    gU, gwa, gws, gmu = None, 0.0, 0.0, np.zeros((C, C))
    for t in range(T, 1 if _variant == "short" else 0, -1):
        gU = gL if gU is None else (gU + gL).astype(dtype)
        b = gL if _variant == "nj" else np.where(live, gL / dend, dtype(0)).astype(dtype)
        GA, GS = np.zeros(Un.shape, dtype), np.zeros(Un.shape, dtype)
        for dy, dx, ka, ps, _, _, _ in kern:
            bi = _shift(b, dy, dx)
            if K:
                GA = _fma(ka[..., None], bi, GA, dtype)
            GS = _fma(ps, bi, GS, dtype)
        if _variant == "nj":
            GA, GS = (np.where(live, X / dend, dtype(0)).astype(dtype) for X in (GA, GS))
        H = _fma(wa, GA, (ws * GS).astype(dtype), dtype) if K else (ws * GS).astype(dtype)
        Q = Qs[t - 1]
        gQ = _mu_t(mu_b, H, dtype)
        gL = _softmax_adjoint(Q, gQ, dtype, inner=_variant != "no_inner")
        gwa += float(_dot(_mu_t(mu, GA, dtype), Q, dtype).astype(np.float64).sum()) if K else 0.0
        gws += float(_dot(_mu_t(mu, GS, dtype), Q, dtype).astype(np.float64).sum())
        if mu is not None:
            gmu += (-(H[..., :, None] * Q[..., None, :]).astype(dtype)).astype(np.float64).sum(axis=(0, 1, 2))
    if _variant != "no_gl0":
        gU = (gU + gL).astype(dtype)
    if dtype is np.float32:
        gwa, gws, gmu = float(np.float32(gwa)), float(np.float32(gws)), gmu.astype(np.float32).astype(np.float64)
    dU = gU[..., 1].astype(np.float64) if binary else np.ascontiguousarray(gU.astype(np.float64).transpose(0, 3, 1, 2))
    return {"unary": dU, "w_appearance": gwa, "w_smooth": gws, "compat": gmu if mu is not None else None}


def crf_grad_bound(unary, guide, grad_output, radius: int, iterations: int, theta_alpha: float, theta_beta: float, theta_gamma: float,
                   w_appearance: float, w_smooth: float, compat=None, output: str = "logit") -> Dict[str, object]:
    """The rounding-model bound on ``hpri_dense_crf_backward`` against ``crf_backward_reference``, in ``crf_bound``'s manner: ``{"unary":
    per element in the unaries' shape, "w_appearance", "w_smooth": floats, "compat": (C, C) or None}``.  With u = 2^-24: the forward's
    error arrives through Q^(t-1) (``crf_bound``'s per-iteration bounds); ``b`` and ``ka = pa e`` round once each, ``e`` with expf's
    argument and allowance as in the forward; the gathers are chains of n - 1 fmaf over SIGNED terms, ``gamma(n - 1) sum |k| |b|``; H
    rounds twice, ``-mu^T H`` is a chain of C fmaf; the softmax adjoint has its chain, one rounding of the difference and one of the
    product; gU rounds at every addition; the parameters' fp64 sums add ``2^-53`` per term and round once to fp32."""
    a = _crf_args(radius, iterations, theta_alpha, theta_beta, theta_gamma, 0.0, 0.0, output, "crf_grad_bound")
    wa, ws = float(np.float32(w_appearance)), float(np.float32(w_smooth))
    a["w_appearance"], a["w_smooth"] = wa, ws
    Un, I, binary = _frames(unary, guide)
    N, h, w, C = Un.shape
    K = I.shape[3]
    mu = _compat(compat, C, "crf_grad_bound")
    mu64 = None if mu is None else mu.astype(np.float64)
    amu = None if mu is None else np.abs(mu64)
    T = a["iterations"]
    if wa < 0 or ws < 0:
        raise ValueError("crf_grad_bound: the forward's rounding model (crf_bound) takes non-negative weights")
    fb = crf_bound(unary, guide, radius, iterations, theta_alpha, theta_beta, theta_gamma, wa, ws, compat)
    _, _, steps = _mean_field(Un, I, a, mu, np.float64)
    Q0 = _softmax(Un, np.float64)
    Qs = [Q0] + steps
    eQs = [Q0 * _softmax_rounding(Un) + TINY] + [np.ascontiguousarray(e.transpose(0, 2, 3, 1)) for e in fb["steps"]]
    gC = _gamma(C)

    def adjoint(Q, eQ, gQ, egQ):
        """(gL, egL) of Q (gQ - <Q, gQ>) with errors eQ and egQ on its inputs."""
        d = (Q * gQ).sum(axis=-1, keepdims=True)
        ed = (eQ * (np.abs(gQ) + egQ) + Q * egQ).sum(axis=-1, keepdims=True) + gC * ((Q + eQ) * (np.abs(gQ) + egQ)).sum(axis=-1, keepdims=True)
        x = gQ - d
        ex = egQ + ed + U * (np.abs(x) + egQ + ed)
        return Q * x, eQ * (np.abs(x) + ex) + Q * ex + U * (Q + eQ) * (np.abs(x) + ex) + TINY

    def mu_t(X, eX):
        """(|-mu^T X| bound pieces): value and error of the chain."""
        if mu is None:
            return X, eX
        return -(X @ mu64), eX @ amu + gC * ((np.abs(X) + eX) @ amu)

    gv = _grad_frames(grad_output, Un, binary, output)
    gL, egL = (gv, np.zeros(Un.shape)) if output == "logit" else adjoint(Qs[T], eQs[T], gv, np.zeros(Un.shape))
    kern = []
    for dy, dx, ka, ps, e, arg, pa in _adjoint_kernels(I, a, np.float64):
        eka = (pa * e * ((K + 3) * arg + SIGMOID_ULPS) * U + U * ka) if K else np.zeros(I.shape[:3])
        kern.append((dy, dx, ka, float(ps), eka))
    cnt = _counts(h, w, a["radius"]) - 1.0
    den = np.maximum(cnt, 1.0)[None, :, :, None]
    live = (cnt > 0)[None, :, :, None]
    gn = _gamma(cnt)[None, :, :, None]
    gU, egU = None, None
    tot = {"wa": [0.0, 0.0, 0.0], "ws": [0.0, 0.0, 0.0], "mu": [np.zeros((C, C)), np.zeros((C, C)), np.zeros((C, C))]}      # value, error, sum of |terms|
    for t in range(T, 0, -1):
        if gU is None:
            gU, egU = gL, egL
        else:
            gU = gU + gL
            egU = egU + egL + U * (np.abs(gU) + egU + egL)
        b = np.where(live, gL / den, 0.0)
        eb = np.where(live, egL / den + U * (np.abs(b) + egL / den), 0.0)
        GA, eGA, AA = np.zeros(Un.shape), np.zeros(Un.shape), np.zeros(Un.shape)
        GS, eGS, AS = np.zeros(Un.shape), np.zeros(Un.shape), np.zeros(Un.shape)
        for dy, dx, ka, ps, eka in kern:
            bi, ebi = _shift(b, dy, dx), _shift(eb, dy, dx)
            ab = np.abs(bi) + ebi
            if K:
                GA += ka[..., None] * bi
                eGA += eka[..., None] * ab + ka[..., None] * ebi
                AA += (ka + eka)[..., None] * ab
            GS += ps * bi
            eGS += ps * ebi
            AS += ps * ab
        eGA += gn * AA
        eGS += gn * AS
        H = wa * GA + ws * GS
        mag = abs(wa) * (np.abs(GA) + eGA) + abs(ws) * (np.abs(GS) + eGS)
        eH = abs(wa) * eGA + abs(ws) * eGS + 2 * U * mag + TINY
        Q, eQ = Qs[t - 1], eQs[t - 1]
        gQ, egQ = mu_t(H, eH)
        gL, egL = adjoint(Q, eQ, gQ, egQ)
        for key, X, eX in (("wa", GA, eGA), ("ws", GS, eGS)):
            v, ev = mu_t(X, eX)
            p = (v * Q).sum(axis=-1)
            ep = (ev * (Q + eQ) + np.abs(v) * eQ).sum(axis=-1) + gC * ((np.abs(v) + ev) * (Q + eQ)).sum(axis=-1) + TINY
            tot[key][0] += p.sum()
            tot[key][1] += ep.sum()
            tot[key][2] += (np.abs(p) + ep).sum()
        if mu is not None:
            P = -(H[..., :, None] * Q[..., None, :])
            eP = eH[..., :, None] * (Q + eQ)[..., None, :] + np.abs(H)[..., :, None] * eQ[..., None, :] + \
                U * ((np.abs(H) + eH)[..., :, None] * (Q + eQ)[..., None, :]) + TINY
            tot["mu"][0] += P.sum(axis=(0, 1, 2))
            tot["mu"][1] += eP.sum(axis=(0, 1, 2))
            tot["mu"][2] += (np.abs(P) + eP).sum(axis=(0, 1, 2))
    gU = gU + gL
    egU = egU + egL + U * (np.abs(gU) + egU + egL)
    th, tw = tile_shape()
    terms = T * N * (th * tw * -(-h // th) * -(-w // tw))                          # what the fp64 sums add, lanes outside the image included

    def total(v, e, s):
        e = e + 2.0 ** -53 * terms * s
        return e + U * (np.abs(v) + e) + TINY
    out = {"unary": egU[..., 1] if binary else np.ascontiguousarray(egU.transpose(0, 3, 1, 2)),
           "w_appearance": float(total(*tot["wa"])) if K else 0.0, "w_smooth": float(total(*tot["ws"])),
           "compat": total(*tot["mu"]) if mu is not None else None}
    return out



__all__ = ["dense_crf", "DenseCRF", "crf_layer", "CRFLayer", "crf_backward_reference", "crf_grad_bound", "crf_reference", "crf_bruteforce", "crf_bound", "crf_tables", "tile_shape", "max_radius", "max_classes",
           "max_guides", "max_iterations", "MAX_RADIUS", "MAX_CLASSES", "MAX_GUIDES", "MAX_ITERATIONS", "CRF_OUTPUTS"]
