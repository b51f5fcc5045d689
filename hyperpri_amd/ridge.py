"""Ridge filtering of score maps (``csrc/ridge.hip``): a multi-scale, scale-normalised Hessian ridge measure ("vesselness", after Frangi
et al. and Sato et al.).

Roots are tubes one to three pixels wide with the occasional tap root of ten; a ridge filter is the classical detector built for that
shape, and the baseline root and vessel papers compare against.  It is the companion of the guided filter: that one keeps edges, this
one keeps lines and suppresses blobs and flat soil, and its winning scale is a per-pixel width estimate.  The plane is anything on the
frame: a principal-component score (``SpectralProjection``: read in place at its channel stride), a detector's or a network's logits
(``domain="prob"``), an abundance plane; ``evaluate.ridge_split`` and ``evaluate.enhance_split`` store the result as a split.

The contract (include/hyperpri_hip.h states it in full).  Per scale ``sigma`` in [0.5, 4], ``R = ceil(3 sigma)``, three half-kernels for
``x = 1 .. R`` made once on the host (``ridge_taps``: fp64, rounded once to fp32), with ``w(x) = exp(-x^2 / 2 sigma^2)``:

    g0 = w / (1 + 2 sum w)      g1 = x w / (2 sum x^2 w)      g2 = q / sum x^2 q,  q = (x^2 / sigma^4 - 1 / sigma^2) w

No centre tap exists: every pass works on differences from its own centre (the implied centre taps are ``1 - 2 sum g0``, ``0`` and
``-2 sum g2``), so the kernels are exactly unit-sum or zero-sum whatever the rounding of the taps.  Borders: half-sample symmetric
reflection ``rho`` (``d c b a | a b c d``), of period 2n.

    row pass, fp32 from +0.0, c = I[y, x], j = 1 .. R:    dp = I[y, rho(x+j)] - c,   dm = I[y, rho(x-j)] - c
        s0 = fmaf(g0[j], dp + dm, s0)     r1 = fmaf(g1[j], dp - dm, r1)     r2 = fmaf(g2[j], dp + dm, r2)
    column pass, fp32 from +0.0, i = 1 .. R, +- the rows rho(y +- i):
        Hxx = (r2c + sum g0[i] ((r2+ - r2c) + (r2- - r2c))) sigma^2
        Hxy = (sum g1[i] (r1+ - r1-)) sigma^2
        Hyy = (sum g2[i] (e+ + e-)) sigma^2,      e+- = (I+- - Ic) + (s0+- - s0c)
    measure, fp64:   mu = (Hxx + Hyy) / 2,   d = sqrt(((Hxx - Hyy) / 2)^2 + Hxy^2)
        bright: l2 = mu - d, l1 = mu + d, gate mu < 0;   dark: l2 = mu + d, l1 = mu - d, gate mu > 0;   both: the eigenvalue of larger
        magnitude by the sign of mu (mu >= 0: mu + d), no gate
        frangi: V = exp(-(l1 / l2)^2 / (2 beta^2)) (-expm1(-(l1^2 + l2^2) / (2 c^2))) where the gate holds and l2 != 0, else 0
        sato:   V = max(-l2, 0) | max(l2, 0) | |l2|
    across scales: the maximum in the order given, the index of the first scale that attains it; ``output="logit"`` writes
    ``logit(clamp(p, 2^-24, 1 - 2^-24))`` of ``p = V`` (frangi) or ``V / (V + c)`` (sato).

Second-derivative taps are a zero-sum kernel; applied uncentred to a plane whose mean dwarfs its local variation they cancel, and a
form that rounds the smoothed plane ``I + s0`` to fp32 before differencing loses what the row pass kept.  Hence the differences
throughout and the two-difference form of ``e``.

``ridge_reference`` restates the contract in fp64 numpy on the same fp32 inputs, ``ridge_bruteforce`` is the independent oracle
(``scipy.ndimage.correlate1d`` with full kernels, ``numpy.linalg.eigvalsh``), ``ridge_bound`` the rounding-model bound.  No autograd,
no CPU fallback.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib
from ._args import FILTER_DOMAINS, _p, _scalar, _stream
from .guided import P_HI, P_LO, SIGMOID_ULPS, U, _gamma, _logit, _sigmoid

MAX_SCALES = 8              # hpri_ridge_max_scales
MAX_RADIUS = 12             # hpri_ridge_max_radius
SIGMA_MIN, SIGMA_MAX = 0.5, 4.0
MEASURES = ("frangi", "sato")
POLARITIES = ("bright", "dark", "both")
OUTPUTS = ("value", "logit")
FP64_SLACK = 1e-14          # exp, expm1 and sqrt of the device's fp64 library against numpy's, relative to values of at most one


def max_scales() -> int:
    """The most scales a launch takes (``hpri_ridge_max_scales``)."""
    return int(_lib.load().hpri_ridge_max_scales())


def max_radius() -> int:
    """The largest tap radius the kernel takes (``hpri_ridge_max_radius``)."""
    return int(_lib.load().hpri_ridge_max_radius())


def tile_shape() -> Tuple[int, int]:
    """(rows, columns) of the tile a workgroup owns (``hpri_ridge_tile_h``, ``hpri_ridge_tile_w``)."""
    lib = _lib.load()
    return int(lib.hpri_ridge_tile_h()), int(lib.hpri_ridge_tile_w())


# ---------------------------------------------------------------------------------------------------
# Arguments and taps
# ---------------------------------------------------------------------------------------------------
def _check_sigmas(sigmas, who: str) -> List[float]:
    """1 .. 8 scales, each the fp32 value the launch works with, in [0.5, 4]."""
    if isinstance(sigmas, torch.Tensor):
        sigmas = sigmas.detach().cpu().reshape(-1).tolist()
    elif np.isscalar(sigmas):
        sigmas = [sigmas]
    sig = [float(np.float32(_scalar(s, f"{who}: sigma"))) for s in sigmas]
    if not 1 <= len(sig) <= MAX_SCALES:
        raise ValueError(f"{who}: need 1 to {MAX_SCALES} scales, got {len(sig)}")
    for s in sig:
        if not (np.isfinite(s) and SIGMA_MIN <= s <= SIGMA_MAX):
            raise ValueError(f"{who}: every sigma must lie in [{SIGMA_MIN}, {SIGMA_MAX}], got {s!r}")
    return sig


def ridge_taps(sigma, dtype=np.float32) -> Tuple[int, np.ndarray, np.ndarray, np.ndarray]:
    """``(R, g0, g1, g2)``: the tap radius ``ceil(3 sigma)`` and the three half-kernels for ``x = 1 .. R``, made in fp64 from the fp32
    value of ``sigma`` and rounded once to ``dtype`` (fp32: what the launch receives and the references use; fp64: unrounded)."""
    s = _check_sigmas([sigma], "ridge_taps")[0]
    R = int(np.ceil(3.0 * s))
    x = np.arange(1, R + 1, dtype=np.float64)
    w = np.exp(-x * x / (2.0 * s * s))
    q = (x * x / s ** 4 - 1.0 / (s * s)) * w
    g0, g1, g2 = w / (1.0 + 2.0 * w.sum()), x * w / (2.0 * (x * x * w).sum()), q / (x * x * q).sum()
    return R, g0.astype(dtype), g1.astype(dtype), g2.astype(dtype)


def _ridge_args(sigmas, measure, polarity, beta, c, domain, output, who: str) -> dict:
    sig = _check_sigmas(sigmas, who)
    if measure not in MEASURES:
        raise ValueError(f"{who}: measure must be one of {MEASURES}, got {measure!r}")
    if polarity not in POLARITIES:
        raise ValueError(f"{who}: polarity must be one of {POLARITIES}, got {polarity!r}")
    if domain not in FILTER_DOMAINS:
        raise ValueError(f"{who}: domain must be one of {FILTER_DOMAINS}, got {domain!r}")
    if output not in OUTPUTS:
        raise ValueError(f"{who}: output must be one of {OUTPUTS}, got {output!r}")
    b, cc = float(np.float32(_scalar(beta, f"{who}: beta"))), float(np.float32(_scalar(c, f"{who}: c")))
    if not (b > 0.0 and np.isfinite(b)):
        raise ValueError(f"{who}: beta must be positive and finite as an fp32 value, got {beta!r}")
    if not (cc > 0.0 and np.isfinite(cc)):
        raise ValueError(f"{who}: c must be positive and finite as an fp32 value, got {c!r}")
    return {"sigmas": sig, "measure": measure, "polarity": polarity, "beta": b, "c": cc, "domain": domain, "output": output}


def _host_taps(sig: List[float]):
    """What the launcher takes: taps (S, 3, 12) fp32, radii (S,) int32, fp32(sigma^2) (S,).  Made once per scale list (a call costs
    more on the host than the launch on the device); the arrays are shared, read-only."""
    return _host_taps_of(tuple(sig))


@functools.lru_cache(maxsize=64)
def _host_taps_of(sig: tuple):
    taps, radii, sigma2 = _make_host_taps(sig)
    for a in (taps, radii, sigma2):
        a.setflags(write=False)
    return taps, radii, sigma2


def _make_host_taps(sig):
    taps = np.zeros((len(sig), 3, MAX_RADIUS), dtype=np.float32)
    radii = np.zeros(len(sig), dtype=np.int32)
    for k, s in enumerate(sig):
        R, g0, g1, g2 = ridge_taps(s)
        radii[k] = R
        taps[k, 0, :R], taps[k, 1, :R], taps[k, 2, :R] = g0, g1, g2
    return taps, radii, np.array([np.float32(s * s) for s in sig], dtype=np.float32)


# ---------------------------------------------------------------------------------------------------
# The filter
# ---------------------------------------------------------------------------------------------------
def _plane_input(t: torch.Tensor) -> Tuple[torch.Tensor, int, int, int]:
    """(N, T, h, w) -> a tensor whose memory the launch reads in place, with its image, plane and pixel stride in floats.  Zero-copy
    whenever a pixel stride describes the view -- a contiguous tensor, a single plane, the first T channels of any channels-last
    buffer (a ``SpectralProjection`` output: pixel stride 8) --, else one layout pass."""
    N, T, h, w = (int(s) for s in t.shape)
    st = [int(s) for s in t.stride()]
    sp = st[3] if w > 1 else (st[2] if h > 1 else 1)
    if (sp >= 1 and (h == 1 or w == 1 or st[2] == w * sp) and (N == 1 or st[0] >= 0) and (T == 1 or st[1] >= 0)
            and t.data_ptr() % 4 == 0):
        return t, (st[0] if N > 1 else 0), (st[1] if T > 1 else 0), sp
    t = t.contiguous()
    return t, T * h * w, h * w, 1


def ridge_filter(maps: torch.Tensor, sigmas, measure: str = "frangi", polarity: str = "bright", beta: float = 0.5, c: float = 0.5,
                 domain: str = "linear", output: str = "value", return_scale: bool = False, return_hessian: bool = False):
    """The multi-scale ridge measure of ``maps``: one launch (``hpri_ridge_filter``).

    ``maps``: fp32 ``(N, h, w)``, ``(N, T, h, w)`` or ``(N, 1, T, h, w)`` on a ROCm device -- a ``SpectralProjection`` output is read
    zero-copy, as is any channels-last view or a contiguous tensor; anything else goes through one layout pass.  The output has their
    shape.  ``sigmas``: 1 to 8 scales in [0.5, 4].  ``domain="prob"``: the maps are logits, filtered as probabilities.
    ``output="logit"``: the logit of the response (frangi) or of ``V / (V + c)`` (sato), what a ``SplitPrediction`` stores.
    ``return_scale``: also the uint8 index of the winning scale, a width estimate; ``return_hessian``: also the fp32
    ``(N, T, S, 3, h, w)`` planes ``Hxx | Hxy | Hyy``.  No autograd: an input that requires grad raises."""
    a = _ridge_args(sigmas, measure, polarity, beta, c, domain, output, "ridge_filter")
    if not isinstance(maps, torch.Tensor):
        raise ValueError(f"ridge_filter: the maps must be a tensor, got {type(maps).__name__}")
    if maps.dtype != torch.float32:
        raise ValueError(f"ridge_filter: need float32 maps, got {maps.dtype}")
    m = maps
    if m.dim() == 5:
        if m.shape[1] != 1:
            raise ValueError(f"ridge_filter: 5-d maps must be (N, 1, T, h, w), got {tuple(m.shape)}")
        m = m[:, 0]
    elif m.dim() == 3:
        m = m[:, None]
    if m.dim() != 4:
        raise ValueError(f"ridge_filter: need maps (N, h, w), (N, T, h, w) or (N, 1, T, h, w), got {tuple(maps.shape)}")
    N, T, h, w = (int(s) for s in m.shape)
    if N * T * h * w == 0:
        raise ValueError("ridge_filter: empty maps")
    if N * T * h * w >= 2 ** 31:
        raise ValueError(f"ridge_filter: N*T*h*w must be below 2^31, got {N * T * h * w}")
    if not maps.is_cuda:
        raise RuntimeError("hyperpri_amd: ridge_filter needs tensors on a ROCm device; there is no CPU fallback")
    if maps.requires_grad:
        raise RuntimeError("ridge_filter: no autograd -- the inputs must not require grad")
    taps, radii, sigma2 = _host_taps(a["sigmas"])
    S = len(a["sigmas"])
    with torch.cuda.device(maps.device):
        src, si, st, sp = _plane_input(m)
        out = torch.empty(tuple(maps.shape), dtype=torch.float32, device=maps.device)
        scale = torch.empty(tuple(maps.shape), dtype=torch.uint8, device=maps.device) if return_scale else None
        hess = torch.empty((N, T, S, 3, h, w), dtype=torch.float32, device=maps.device) if return_hessian else None
        _lib.call("hpri_ridge_filter", _p(src), si, st, sp, N, T, h, w, taps.ctypes.data, radii.ctypes.data, sigma2.ctypes.data, S,
                  a["beta"], a["c"], POLARITIES.index(polarity), MEASURES.index(measure), FILTER_DOMAINS.index(domain),
                  OUTPUTS.index(output), _p(out), _p(scale) if return_scale else None, _p(hess) if return_hessian else None, _stream())
    res = (out,) + ((scale,) if return_scale else ()) + ((hess,) if return_hessian else ())
    return res if len(res) > 1 else out


class RidgeFilter(torch.nn.Module):
    """``ridge_filter`` with its parameters fixed: ``RidgeFilter(sigmas, ...)(maps)``.  The parameters travel in ``state_dict()`` (as
    the module's extra state: no tensor, nothing to move to a device)."""

    def __init__(self, sigmas, measure: str = "frangi", polarity: str = "bright", beta: float = 0.5, c: float = 0.5,
                 domain: str = "linear", output: str = "value"):
        super().__init__()
        self.set_extra_state({"sigmas": sigmas, "measure": measure, "polarity": polarity, "beta": beta, "c": c, "domain": domain,
                              "output": output})

    def get_extra_state(self):
        return {"sigmas": list(self.sigmas), "measure": self.measure, "polarity": self.polarity, "beta": self.beta, "c": self.c,
                "domain": self.domain, "output": self.output}

    def set_extra_state(self, state):
        a = _ridge_args(state["sigmas"], state["measure"], state["polarity"], state["beta"], state["c"], state["domain"],
                        state["output"], "RidgeFilter")
        self.sigmas, self.measure, self.polarity, self.beta, self.c = a["sigmas"], a["measure"], a["polarity"], a["beta"], a["c"]
        self.domain, self.output = a["domain"], a["output"]

    def extra_repr(self) -> str:
        return (f"sigmas={tuple(self.sigmas)}, measure={self.measure!r}, polarity={self.polarity!r}, beta={self.beta:g}, c={self.c:g}, "
                f"domain={self.domain!r}, output={self.output!r}")

    def forward(self, maps: torch.Tensor, return_scale: bool = False, return_hessian: bool = False):
        return ridge_filter(maps, self.sigmas, self.measure, self.polarity, self.beta, self.c, self.domain, self.output, return_scale,
                            return_hessian)


# ---------------------------------------------------------------------------------------------------
# The contract restated in numpy: the oracles of the tests
# ---------------------------------------------------------------------------------------------------
def _frames(maps) -> Tuple[np.ndarray, tuple]:
    """fp32 inputs as an fp64 (N, T, h, w) array, and the shape they came in."""
    I = np.asarray(maps.detach().cpu().numpy() if isinstance(maps, torch.Tensor) else maps)
    shape = I.shape
    if I.ndim == 5 and I.shape[1] == 1:
        I = I[:, 0]
    elif I.ndim == 3:
        I = I[:, None]
    if I.ndim != 4 or I.size == 0:
        raise ValueError(f"ridge: need non-empty maps (N, h, w), (N, T, h, w) or (N, 1, T, h, w), got {shape}")
    return np.ascontiguousarray(I.astype(np.float32).astype(np.float64)), shape


def _rho(i: np.ndarray, n: int) -> np.ndarray:
    """Half-sample symmetric reflection of any integer onto [0, n)."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _fma(g: float, x: np.ndarray, acc: np.ndarray, dtype) -> np.ndarray:
    """``fmaf(g, x, acc)`` in ``dtype``: the product of two fp32 values is exact in fp64, the sum is rounded to fp32."""
    if dtype is np.float32:
        return (np.float64(g) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return g * x + acc


def _hessian(I: np.ndarray, sigma: float, dtype) -> np.ndarray:
    """Both passes of one scale in ``dtype`` on (..., h, w) planes: (..., 3, h, w) = Hxx | Hxy | Hyy, as fp64."""
    R, g0, g1, g2 = ridge_taps(sigma)
    g0, g1, g2 = ([float(v) for v in g] for g in (g0, g1, g2))
    h, w = I.shape[-2:]
    xs, ys = np.arange(w), np.arange(h)
    Iw = I.astype(dtype)
    s0, r1, r2 = (np.zeros(I.shape, dtype) for _ in range(3))
    for j in range(1, R + 1):
        dp, dm = Iw[..., _rho(xs + j, w)] - Iw, Iw[..., _rho(xs - j, w)] - Iw
        sm = dp + dm
        s0, r1, r2 = _fma(g0[j - 1], sm, s0, dtype), _fma(g1[j - 1], dp - dm, r1, dtype), _fma(g2[j - 1], sm, r2, dtype)
    axx, axy, ayy = (np.zeros(I.shape, dtype) for _ in range(3))
    for i in range(1, R + 1):
        up, dn = _rho(ys + i, h), _rho(ys - i, h)
        ep = (Iw[..., up, :] - Iw) + (s0[..., up, :] - s0)
        em = (Iw[..., dn, :] - Iw) + (s0[..., dn, :] - s0)
        axx = _fma(g0[i - 1], (r2[..., up, :] - r2) + (r2[..., dn, :] - r2), axx, dtype)
        axy = _fma(g1[i - 1], r1[..., up, :] - r1[..., dn, :], axy, dtype)
        ayy = _fma(g2[i - 1], ep + em, ayy, dtype)
    s2 = dtype(np.float32(sigma * sigma))
    return np.stack([(r2 + axx) * s2, axy * s2, ayy * s2], axis=-3).astype(np.float64)


def _measure(H: np.ndarray, measure: str, polarity: str, beta: float, c: float) -> Dict[str, np.ndarray]:
    """The fp64 epilogue, operation by operation as the kernel performs it, on (..., 3, h, w) planes: ``V``, ``open`` (frangi: the
    formula without the gate), ``mu``, ``l1``, ``l2`` and ``gate``."""
    hxx, hxy, hyy = H[..., 0, :, :], H[..., 1, :, :], H[..., 2, :, :]
    mu, hd = (hxx + hyy) / 2.0, (hxx - hyy) / 2.0
    d = np.sqrt(hd * hd + hxy * hxy)
    gate = np.ones(mu.shape, dtype=bool)
    if polarity == "bright":
        l2, l1, gate = mu - d, mu + d, mu < 0.0
    elif polarity == "dark":
        l2, l1, gate = mu + d, mu - d, mu > 0.0
    else:
        pos = mu >= 0.0
        l2, l1 = np.where(pos, mu + d, mu - d), np.where(pos, mu - d, mu + d)
    if measure == "sato":
        x = -l2 if polarity == "bright" else (l2 if polarity == "dark" else np.abs(l2))
        V = np.where(x > 0.0, x, 0.0)
        return {"V": V, "open": V, "mu": mu, "l1": l1, "l2": l2, "gate": gate, "x": x}
    nz = l2 != 0.0
    rb = l1 / np.where(nz, l2, 1.0)
    two_beta2, two_c2 = 2.0 * beta * beta, 2.0 * c * c
    opened = np.where(nz, np.exp(-(rb * rb) / two_beta2) * (-np.expm1(-(l1 * l1 + l2 * l2) / two_c2)), 0.0)
    return {"V": np.where(gate, opened, 0.0), "open": opened, "mu": mu, "l1": l1, "l2": l2, "gate": gate, "x": None}


def ridge_reference(maps, sigmas, measure: str = "frangi", polarity: str = "bright", beta: float = 0.5, c: float = 0.5,
                    domain: str = "linear", dtype=np.float64) -> Dict[str, np.ndarray]:
    """The contract line by line in fp64 numpy on the same fp32 inputs (the taps, ``sigma^2``, ``beta`` and ``c`` as the fp32 values
    the launch receives); nothing is rounded to fp32 on the way.  ``{"hessian": (N, T, S, 3, h, w), "scales": V per scale (N, T, S, h,
    w), "open": the same without frangi's gate, "response" and "index" (uint8) and "prob" and "logit" in the maps' shape}``; ``prob``
    is what the logit is taken of, ``V`` (frangi) or ``V / (V + c)`` (sato).

    ``dtype=numpy.float32``: every operation of the two passes -- differences, sums, fmaf, the product by ``sigma^2`` -- in fp32 (and
    the sigmoid of ``domain="prob"`` rounded to fp32), the measure in fp64: an emulation of the device that ``ridge_bound`` must cover."""
    a = _ridge_args(sigmas, measure, polarity, beta, c, domain, "value", "ridge_reference")
    I, shape = _frames(maps)
    if a["domain"] == "prob":
        I = _sigmoid(I)
        if dtype is np.float32:
            I = I.astype(np.float32).astype(np.float64)
    H = np.stack([_hessian(I, s, dtype) for s in a["sigmas"]], axis=2)
    M = _measure(H, measure, polarity, a["beta"], a["c"])
    V = M["V"]
    index = V.argmax(axis=2).astype(np.uint8)                     # the first scale that attains the maximum
    response = V.max(axis=2)
    prob = response if measure == "frangi" else response / (response + a["c"])
    return {"hessian": H, "scales": V, "open": M["open"], "mu": M["mu"], "response": response.reshape(shape),
            "index": index.reshape(shape), "prob": prob.reshape(shape), "logit": _logit(prob).reshape(shape)}


def ridge_bruteforce(maps, sigmas, measure: str = "frangi", polarity: str = "bright", beta: float = 0.5, c: float = 0.5) -> Dict[str, np.ndarray]:
    """The independent oracle, linear domain: ``scipy.ndimage.correlate1d(mode="reflect")`` along each axis of the fp64 image with full
    kernels built from the fp32 taps and the implied centre taps, then the measure from a textbook 2 x 2 ``numpy.linalg.eigvalsh``.
    ``{"hessian", "scales", "response", "index"}`` as ``ridge_reference`` returns them."""
    from scipy.ndimage import correlate1d
    a = _ridge_args(sigmas, measure, polarity, beta, c, "linear", "value", "ridge_bruteforce")
    I, shape = _frames(maps)
    Hs, Vs = [], []
    for s in a["sigmas"]:
        R, g0, g1, g2 = (np.asarray(v, dtype=np.float64) for v in ridge_taps(s))
        k0 = np.concatenate([g0[::-1], [1.0 - 2.0 * g0.sum()], g0])
        k1 = np.concatenate([-g1[::-1], [0.0], g1])
        k2 = np.concatenate([g2[::-1], [-2.0 * g2.sum()], g2])
        s2 = float(np.float32(s * s))

        def sep(kx, ky):
            return correlate1d(correlate1d(I, kx, axis=-1, mode="reflect"), ky, axis=-2, mode="reflect") * s2
        H = np.stack([sep(k2, k0), sep(k1, k1), sep(k0, k2)], axis=2)                      # (N, T, 3, h, w)
        A = np.empty(H.shape[:2] + H.shape[3:] + (2, 2))
        A[..., 0, 0], A[..., 0, 1], A[..., 1, 0], A[..., 1, 1] = H[:, :, 0], H[:, :, 1], H[:, :, 1], H[:, :, 2]
        lo, hi = np.moveaxis(np.linalg.eigvalsh(A), -1, 0)
        trace = H[:, :, 0] + H[:, :, 2]
        if polarity == "bright":
            big, small, gate = lo, hi, trace < 0
        elif polarity == "dark":
            big, small, gate = hi, lo, trace > 0
        else:
            big, small, gate = np.where(trace >= 0, hi, lo), np.where(trace >= 0, lo, hi), np.ones(lo.shape, bool)
        if measure == "sato":
            V = np.maximum(-big, 0) if polarity == "bright" else (np.maximum(big, 0) if polarity == "dark" else np.abs(big))
        else:
            ok = gate & (big != 0)
            ratio = small / np.where(ok, big, 1.0)
            V = np.where(ok, np.exp(-ratio ** 2 / (2 * a["beta"] ** 2)) * (1.0 - np.exp(-(small ** 2 + big ** 2) / (2 * a["c"] ** 2))), 0.0)
        Hs.append(H)
        Vs.append(V)
    H, V = np.stack(Hs, axis=2), np.stack(Vs, axis=2)
    return {"hessian": H, "scales": V, "response": V.max(axis=2).reshape(shape), "index": V.argmax(axis=2).astype(np.uint8).reshape(shape)}


def _hessian_bound(I: np.ndarray, ep, sigma: float, unit=None) -> np.ndarray:
    """The bound on one scale's three planes: both passes in fp64 with the sums of the absolute terms beside the sums.  ``unit``: that
    relative error per pass in place of the chains' gamma (2^-24: what the rounding of the taps alone does to an exact evaluation)."""
    R, g0, g1, g2 = ridge_taps(sigma)
    a0, a1, a2 = (np.abs(np.asarray(g, dtype=np.float64)) for g in (g0, g1, g2))
    g0, g1, g2 = (np.asarray(g, dtype=np.float64) for g in (g0, g1, g2))
    h, w = I.shape[-2:]
    xs, ys = np.arange(w), np.arange(h)
    ep = np.zeros(I.shape) if ep is None else ep
    s0, r1, r2, A0, A1, A2, P0, P1, P2 = (np.zeros(I.shape) for _ in range(9))
    for j in range(1, R + 1):
        xp, xm = _rho(xs + j, w), _rho(xs - j, w)
        dp, dm = I[..., xp] - I, I[..., xm] - I
        mag, per = np.abs(dp) + np.abs(dm), ep[..., xp] + ep[..., xm] + 2 * ep
        s0, r1, r2 = s0 + g0[j - 1] * (dp + dm), r1 + g1[j - 1] * (dp - dm), r2 + g2[j - 1] * (dp + dm)
        A0, A1, A2 = A0 + a0[j - 1] * mag, A1 + a1[j - 1] * mag, A2 + a2[j - 1] * mag
        P0, P1, P2 = P0 + a0[j - 1] * per, P1 + a1[j - 1] * per, P2 + a2[j - 1] * per
    gr = _gamma(R + 2) if unit is None else unit                  # a difference, dp +- dm, R fmaf
    E0, E1, E2 = P0 + gr * (A0 + P0), P1 + gr * (A1 + P1), P2 + gr * (A2 + P2)
    pxx, mxx, pxy, mxy, pyy, myy = (np.zeros(I.shape) for _ in range(6))
    for i in range(1, R + 1):
        up, dn = _rho(ys + i, h), _rho(ys - i, h)
        pxx += a0[i - 1] * (E2[..., up, :] + E2[..., dn, :] + 2 * E2)
        mxx += a0[i - 1] * (np.abs(r2[..., up, :] - r2) + np.abs(r2[..., dn, :] - r2))
        pxy += a1[i - 1] * (E1[..., up, :] + E1[..., dn, :])
        mxy += a1[i - 1] * np.abs(r1[..., up, :] - r1[..., dn, :])
        pyy += a2[i - 1] * (E0[..., up, :] + E0[..., dn, :] + 2 * E0 + ep[..., up, :] + ep[..., dn, :] + 2 * ep)
        myy += a2[i - 1] * (np.abs(I[..., up, :] - I) + np.abs(s0[..., up, :] - s0) + np.abs(I[..., dn, :] - I) + np.abs(s0[..., dn, :] - s0))
    pxx, mxx = pxx + E2, mxx + np.abs(r2)
    s2 = float(np.float32(sigma * sigma))
    gxx, gxy, gyy = (_gamma(R + 4), _gamma(R + 2), _gamma(R + 4)) if unit is None else (unit, unit, unit)
    return s2 * np.stack([pxx + gxx * (mxx + pxx), pxy + gxy * (mxy + pxy), pyy + gyy * (myy + pyy)], axis=-3)


def ridge_bound(maps, sigmas, measure: str = "frangi", polarity: str = "bright", beta: float = 0.5, c: float = 0.5,
                domain: str = "linear") -> Dict[str, np.ndarray]:
    """The rounding-model bound on the device against ``ridge_reference``, u = 2^-24.

    * ``"hessian"`` (N, T, S, 3, h, w).  An fp32 chain ``sum tap * difference`` is off by at most ``gamma(k) sum |tap| |difference|``
      with k the roundings a term passes: R + 2 in the row pass (the difference, ``dp +- dm``, R fmaf), R + 4 for Hxx and Hyy (the
      difference, the sum of two, R fmaf, ``r2c + .`` or ``e+ + e-``, the product by ``sigma^2``), R + 2 for Hxy.  The row pass's
      errors enter the column pass as perturbations of its inputs, tap by tap.  The sums of absolute terms are computed here beside
      the sums.  Domain "prob" adds what the planes come with: the device's sigmoid is within ``4 u p`` of the exact one.
    * ``"scales"`` (N, T, S, h, w), on V per scale.  ``|d mu| <= (Exx + Eyy) / 2``; d is a norm, so ``|d d| <= |(d mu, Exy)|``; both
      eigenvalues move by at most ``El = |d mu| + |d d|``.  Sato: ``|dV| <= El``, and 0 where ``max(., 0)`` is decided.  Frangi:
      ``|dS| <= |dH|_F`` for the structure term B (slope at most ``min(e^-1/2 / c, S / c^2)``); the ratio term A has slope at most
      ``e^-1/2 / beta`` in ``l1 / l2``, which moves by at most ``2 El / (|l2| - El)``, and it is multiplied by ``B <= l2^2 / c^2``, which
      keeps the product finite as l2 -> 0; where ``|l2| <= 2 El`` both values lie in ``[0, (|l2| + 2 El)^2 / c^2]``.  0 where the gate is
      decided closed.
    * ``"value"`` and ``"prob"``, the maps' shape: the largest of the scales' bounds (a maximum is 1-Lipschitz) and the final rounding;
      ``prob``: through ``V / (V + c)`` for sato.
    * ``"gate"`` (N, T, S, h, w): ``|mu|`` within its bound under a gated polarity; ``"undecided"``: any scale's gate, where the response
      may be either branch's; ``"candidates"`` (N, T, S, h, w): the scales that may win, ``"undecided_index"``: more than one of them, or
      an undecided gate."""
    a = _ridge_args(sigmas, measure, polarity, beta, c, domain, "value", "ridge_bound")
    I, shape = _frames(maps)
    ep = None
    if a["domain"] == "prob":
        I = _sigmoid(I)
        ep = SIGMOID_ULPS * U * I
    be, cc = a["beta"], a["c"]
    H = np.stack([_hessian(I, s, np.float64) for s in a["sigmas"]], axis=2)
    EH = np.stack([_hessian_bound(I, ep, s) for s in a["sigmas"]], axis=2)
    M = _measure(H, measure, polarity, be, cc)
    Exx, Exy, Eyy = EH[:, :, :, 0], EH[:, :, :, 1], EH[:, :, :, 2]
    Emu = (Exx + Eyy) / 2.0
    El = Emu + np.sqrt(Emu * Emu + Exy * Exy)
    gate = np.zeros(M["mu"].shape, dtype=bool)
    if measure == "sato":
        EV = El if polarity == "both" else np.where(M["x"] < -El, 0.0, El)
    else:
        l1, l2 = M["l1"], M["l2"]
        ES, S = np.sqrt(Exx * Exx + 2 * Exy * Exy + Eyy * Eyy), np.sqrt(l1 * l1 + l2 * l2)
        dB = ES * np.minimum(np.exp(-0.5) / cc, (S + ES) / (cc * cc))
        B = -np.expm1(-(S * S) / (2.0 * cc * cc))
        al2 = np.abs(l2)
        cap = np.minimum(1.0, (al2 + 2 * El) ** 2 / (cc * cc))
        safe = al2 > 2 * El
        dA = np.exp(-0.5) / be * 2 * El / np.where(safe, al2 - El, 1.0)
        EV = np.where(safe, dA * np.minimum(cap, B + dB) + dB, cap)
        if polarity != "both":
            gate = (np.abs(M["mu"]) <= Emu) & (Emu > 0)
            EV = np.where(~M["gate"] & ~gate, 0.0, EV)
    V = M["V"]
    Vmax, EVmax = V.max(axis=2), EV.max(axis=2)
    value = EVmax + U * (Vmax + EVmax) + FP64_SLACK
    if measure == "frangi":
        prob = value
    else:
        p = Vmax / (Vmax + cc)
        prob = EVmax * cc / (np.maximum(Vmax - EVmax, 0.0) + cc) ** 2
        prob = prob + U * (p + prob) + FP64_SLACK
    first = V.argmax(axis=2)
    EVbest = np.take_along_axis(EV, first[:, :, None], axis=2)
    cand = (V + EV > Vmax[:, :, None] - EVbest) | (np.arange(V.shape[2])[None, None, :, None, None] == first[:, :, None])
    undecided = gate.any(axis=2)
    return {"hessian": EH, "scales": EV, "value": value.reshape(shape), "prob": prob.reshape(shape), "gate": gate,
            "undecided": undecided.reshape(shape), "candidates": cand | gate,
            "undecided_index": ((cand.sum(axis=2) > 1) | undecided).reshape(shape)}


__all__ = ["ridge_filter", "RidgeFilter", "ridge_taps", "ridge_reference", "ridge_bruteforce", "ridge_bound", "tile_shape", "max_scales",
           "max_radius", "MAX_SCALES", "MAX_RADIUS", "MEASURES", "POLARITIES", "OUTPUTS", "FILTER_DOMAINS", "P_LO", "P_HI"]
