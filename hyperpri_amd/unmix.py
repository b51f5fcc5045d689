"""Spectral unmixing on the device (``csrc/unmix.hip``): abundance maps under the linear mixing model, endmembers by ATGP.

``detect.py`` and ``cluster.py`` give every pixel a score or a label.  HyperPRI's roots are one to three pixels wide, so most root
pixels are *mixed*; the classical answer is ``x ~ E a`` with ``a >= 0`` and ``sum a = 1``: abundance maps, a reconstruction error and
a root-fraction map that reads as a soft baseline.  The split stays in HBM.

The fit happens in fp64 on the host and is rounded once (the rule of ``SpectralDetector``): ``E = Q R`` is the thin QR of the
``(C, M)`` endmember matrix with a positive diagonal of ``R``; the device receives the rows of ``Q^T`` and ``E^T`` as fp32 and ``R``
and ``G = R^T R`` as fp64.  The projection goes through ``Q``: root and soil spectra are strongly correlated, the Gram form
``E^T x`` would amplify the fp32 error of the projection by ``cond(E)^2``, the QR route amplifies it by ``cond(E)``.

The contract of the kernel (include/hyperpri_hip.h states it in full), per pixel:

    y[m] = fmaf(Q32[m, cs-1], x[cs-1], ... fmaf(Q32[m, 0], x[0], 0))          fp32 MFMA chain
    b = R^T y;  a = argmin 1/2 a^T G a - b^T a under the mode                  fp64: ucls | scls (sum a = 1) | ncls (a >= 0) | fcls (both)
    a32 = fp32(a);  r[c] = fmaf(-E32[M-1, c], a32[M-1], ... x[c]);  rmse = sqrt(sum r^2 / C)
    value = logit(clamp(sum of the foreground a32, 2^-24, 1 - 2^-24))

``ncls`` and ``fcls`` follow the active-set rule of Lawson and Hanson with the equality carried through (``unmix_reference`` restates
it line by line).  ``hpri_band_extreme`` is one step of ATGP, the automatic target generation process: the pixel of the cached split
with the largest residual after projecting out the rows found so far.

``unmix_reference``, ``unmix_bruteforce`` (every support enumerated, each solved in closed form: the independent oracle),
``unmix_bound`` and ``atgp_reference`` are fp64 numpy on the same fp32 inputs (no scipy).  No autograd, no CPU fallback.
"""
from __future__ import annotations

from itertools import combinations
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._args import _p, _rup, _stream
from .cache import _DT, CubeCache
from .spectral import _band_input, _check_select, _slot_list, class_spectra, max_channel_stride

MODES = ("ucls", "scls", "ncls", "fcls")
OUTPUTS = ("abundance", "rmse", "logit")
MAX_MEMBERS = 8             # hpri_band_unmix_max_members
RANK_TOL = 1e-6             # endmembers with sigma_min(R) <= RANK_TOL sigma_max(R) are refused
U = 2.0 ** -24
TAU = 2.0 ** -40


def max_members() -> int:
    """The largest number of endmembers the kernel takes (``hpri_band_unmix_max_members``)."""
    return int(_lib.load().hpri_band_unmix_max_members())


def _mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"unmix: mode must be one of {MODES}, got {mode!r}")
        return MODES.index(mode)
    if int(mode) not in (0, 1, 2, 3):
        raise ValueError(f"unmix: mode must be one of {MODES} or 0 .. 3, got {mode!r}")
    return int(mode)


# ---------------------------------------------------------------------------------------------------
# The fit, fp64 on the host
# ---------------------------------------------------------------------------------------------------
def _array64(a, who: str) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.asarray(a, dtype=np.float64)


def unmix_operands(endmembers) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``(E32 (M, C), Q32 (M, C), R (M, M), G (M, M))`` of (M, C) endmember spectra: the thin QR ``E = Q R`` of the (C, M) matrix in
    fp64, the diagonal of ``R`` made positive, ``G = R^T R``; ``E32`` and ``Q32`` are ``E^T`` and ``Q^T`` rounded once to fp32.
    ``ValueError`` for more than ``MAX_MEMBERS`` or more than C members, a non-finite entry and rank-deficient endmembers
    (``sigma_min(R) <= 1e-6 sigma_max(R)``)."""
    E = _array64(endmembers, "SpectralUnmixer")
    if E.ndim != 2 or E.shape[0] == 0 or E.shape[1] == 0:
        raise ValueError(f"SpectralUnmixer: need endmembers (M, C), got {tuple(E.shape)}")
    M, C = E.shape
    if M > MAX_MEMBERS:
        raise ValueError(f"SpectralUnmixer: M = {M} exceeds the {MAX_MEMBERS} endmembers the kernel takes")
    if M > C:
        raise ValueError(f"SpectralUnmixer: M = {M} endmembers cannot be independent in {C} bands")
    if not np.isfinite(E).all():
        raise ValueError("SpectralUnmixer: the endmembers must be finite")
    Q, R = np.linalg.qr(E.T)
    sign = np.where(np.diag(R) < 0, -1.0, 1.0)
    Q, R = Q * sign[None, :], R * sign[:, None]
    sv = np.linalg.svd(R, compute_uv=False)
    if not sv[-1] > RANK_TOL * sv[0]:
        col = np.sqrt((R * R).sum(axis=0))
        j = int(np.argmin(np.abs(np.diag(R)) / np.where(col > 0, col, 1.0)))
        raise ValueError(f"SpectralUnmixer: the endmembers are rank-deficient (sigma_min / sigma_max = {sv[-1] / max(sv[0], 1e-300):.2e}): "
                         f"column {j} is a combination of the columns before it")
    R = np.triu(R)
    return E.astype(np.float32), np.ascontiguousarray(Q.T).astype(np.float32), R, R.T @ R


def _atgp_row(spectrum: np.ndarray, rows: Sequence[np.ndarray]) -> np.ndarray:
    """The unit residual of ``spectrum`` against the orthonormal fp64 ``rows``, taken twice (re-orthogonalisation)."""
    r = np.asarray(spectrum, dtype=np.float64).copy()
    scale = np.sqrt((r * r).sum())
    if rows:
        B = np.stack(rows)
        for _ in range(2):
            r = r - B.T @ (B @ r)
    n = np.sqrt((r * r).sum())
    if not n > RANK_TOL * scale:
        raise ValueError("extract_endmembers: the selected pixels hold no further independent spectrum")
    return r / n


def extract_endmembers(cache: CubeCache, members: int, slots: Optional[Sequence[int]] = None, select: str = "all", return_values: bool = False):
    """ATGP over the selected pixels of ``slots`` (default: every filled slot): ``members`` steps of ``hpri_band_extreme``, each the
    pixel with the largest squared residual against the orthonormal rows found so far (the first: the largest norm; between equal
    residuals the lowest position).  After a step the host reads the winner's spectrum from the cache, takes its fp64 residual against
    the fp64 rows twice, normalises it and appends it, rounded to fp32, to the device's rows.  Returns ``(spectra (M, C) fp64 as the
    cache stores them, positions (M, 2) int64 = (list entry, pixel inside the slot))``, with ``return_values`` also the fp32 residuals
    the device found, (M,).  One host synchronisation per step."""
    code = _check_select(select)
    idx = _slot_list(cache, slots)
    M = int(members)
    if not 1 <= M <= MAX_MEMBERS:
        raise ValueError(f"extract_endmembers: members must lie in [1, {MAX_MEMBERS}], got {members}")
    if M > cache.C:
        raise ValueError(f"extract_endmembers: M = {M} endmembers cannot be independent in {cache.C} bands")
    dev, cs, C, P = cache.device, cache.cs, cache.C, cache.H * cache.W
    spectra, positions, rows, values = [], [], [], []
    with torch.cuda.device(dev):
        table = torch.tensor(list(idx), dtype=torch.int32).to(dev)
        nbytes = int(_lib.load().hpri_band_extreme_workspace_bytes())
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        basis = torch.zeros((16, cs), dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.int64, device=dev)               # position | the value's bits
        flat = cache._cubes.reshape(cache.capacity * P, cs)
        for k in range(M):
            _lib.call("hpri_band_extreme", _p(cache._cubes), _DT[cache.store_dtype], cache.capacity, cache.H, cache.W, cs, _p(cache._masks),
                      _p(table), len(idx), code, _p(basis), k, _p(work), nbytes, out.data_ptr() + 8, out.data_ptr(), _stream())
            host = out.cpu().numpy()
            pos = int(host[0])
            values.append(float(host[1:].view(np.float32)[0]))
            if pos < 0:
                raise ValueError("extract_endmembers: no selected pixel")
            e, px = divmod(pos, P)
            spec = flat[idx[e] * P + px, :C].to(torch.float64).cpu().numpy()
            rows.append(_atgp_row(spec, rows))
            basis[k, :C] = torch.from_numpy(rows[-1].astype(np.float32)).to(dev)
            spectra.append(spec)
            positions.append((e, px))
    if return_values:
        return np.stack(spectra), np.asarray(positions, dtype=np.int64), np.asarray(values, dtype=np.float32)
    return np.stack(spectra), np.asarray(positions, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------
# The module
# ---------------------------------------------------------------------------------------------------
class SpectralUnmixer(torch.nn.Module):
    """Abundance maps of a device image under the linear mixing model.  Buffers (a checkpoint carries them): ``endmembers`` (M, C)
    and ``basis`` (M, C) fp32 -- ``E^T`` and the rows of ``Q^T`` of the thin QR ``E = Q R`` --, ``tri`` = R and ``gram`` = ``R^T R``
    (M, M) fp64, ``foreground`` (M,) bool and ``meta`` (M, 2) fp64: the (list entry, pixel) an endmember was picked at, -1 otherwise.
    Everything is fitted in fp64 on the host and rounded once.

    ``unmixer(x, mode="fcls", output="abundance")`` takes what ``SpectralDetector`` takes -- an image in either logical shape,
    ``(N, 1, C, h, w)`` or ``(N, C, h, w)``, or the cache's batch dict, zero-copy where the layout allows -- and returns an fp32
    ``(N, M, h, w)`` abundance map (``members``: the planes to return, default all), the ``(N, 1, h, w)`` root-mean-square
    reconstruction error (``"rmse"``) or the logit of the clamped foreground fraction (``"logit"``; ``members``: the endmembers that
    count as foreground, default the ``foreground`` flags), which ``validate_net`` and ``test_net`` read as a network's output.  All
    are views of planes.  ``mode``: ``ucls`` (unconstrained), ``scls`` (sum to one), ``ncls`` (non-negative) or ``fcls`` (both).
    ``capped`` is the number of pixels of the last call that reached the iteration cap (``cap`` sub-solves, 0: 3 M), read lazily.
    No autograd: an input that requires grad raises."""

    def __init__(self, endmembers, foreground=None, positions=None):
        super().__init__()
        E32, Q32, R, G = unmix_operands(endmembers)
        M = E32.shape[0]
        fg = np.zeros(M, dtype=bool) if foreground is None else np.asarray(
            foreground.detach().cpu().numpy() if isinstance(foreground, torch.Tensor) else foreground).astype(bool)
        if fg.shape != (M,):
            raise ValueError(f"SpectralUnmixer: foreground must have shape ({M},), got {tuple(fg.shape)}")
        meta = np.full((M, 2), -1.0) if positions is None else np.asarray(positions, dtype=np.float64).reshape(M, 2)
        self.register_buffer("endmembers", torch.from_numpy(E32.copy()))
        self.register_buffer("basis", torch.from_numpy(Q32.copy()))
        self.register_buffer("tri", torch.from_numpy(R.copy()))
        self.register_buffer("gram", torch.from_numpy(G.copy()))
        self.register_buffer("foreground", torch.from_numpy(fg.copy()))
        self.register_buffer("meta", torch.from_numpy(meta.copy()))
        self._padded = None             # (key, basis (16, cs), members (M, cs), tri | gram (2 M M) fp64) on the device
        self._capped = None             # the counter of the last call, on the device

    # ---- constructors -------------------------------------------------------------------------------
    @classmethod
    def blank(cls, bands: int, members: int) -> "SpectralUnmixer":
        """An unmixer of the given shapes for ``load_state_dict`` to fill."""
        return cls(np.eye(int(members), int(bands)))

    @classmethod
    def from_class_spectra(cls, cache: CubeCache, slots: Optional[Sequence[int]] = None) -> "SpectralUnmixer":
        """Two endmembers, the mean root and the mean soil spectrum of ``class_spectra``; the root member is flagged foreground."""
        sp = class_spectra(cache, slots)
        return cls(np.stack([sp["foreground"]["mean"], sp["background"]["mean"]]), foreground=[True, False]).to(cache.device)

    @classmethod
    def from_kmeans(cls, model) -> "SpectralUnmixer":
        """The centroids of a calibrated ``SpectralKMeans`` as endmembers, foreground where ``foreground_share > 0.5``."""
        share = model.foreground_share.detach().cpu().numpy()
        if not np.isfinite(share).all():
            raise ValueError("SpectralUnmixer.from_kmeans: the model has no foreground shares; run calibrate() first")
        return cls(model.centroids, foreground=share > 0.5).to(model.centers.device)

    @classmethod
    def fit(cls, cache: CubeCache, members: int, slots: Optional[Sequence[int]] = None, select: str = "all",
            reference: Optional[Dict[str, Dict[str, object]]] = None) -> "SpectralUnmixer":
        """``extract_endmembers`` (ATGP) supplies the endmembers.  ``reference=class_spectra(...)`` flags an endmember foreground when
        its spectral angle to the root mean is smaller than its angle to the soil mean (host numpy); without it none is."""
        spectra, positions = extract_endmembers(cache, members, slots, select)
        fg = None
        if reference is not None:
            def cosine(t):
                t = np.asarray(t, dtype=np.float64)
                return spectra @ t / (np.sqrt((spectra * spectra).sum(axis=1)) * np.sqrt((t * t).sum()))
            fg = cosine(reference["foreground"]["mean"]) > cosine(reference["background"]["mean"])
        return cls(spectra, foreground=fg, positions=positions).to(cache.device)

    # ---- properties ---------------------------------------------------------------------------------
    @property
    def in_channels(self) -> int:
        return int(self.endmembers.shape[1])

    @property
    def num_members(self) -> int:
        return int(self.endmembers.shape[0])

    @property
    def capped(self) -> int:
        """Pixels of the last call that reached the iteration cap (one host synchronisation)."""
        return 0 if self._capped is None else int(self._capped[0].item())

    def _device_operands(self, device, cs: int):
        bufs = (self.endmembers, self.basis, self.tri, self.gram)
        key = (str(device), cs) + tuple((b._version, b.data_ptr()) for b in bufs)
        if self._padded is None or self._padded[0] != key:
            M, C = self.num_members, self.in_channels
            basis = torch.zeros((16, cs), dtype=torch.float32, device=device)
            members = torch.zeros((M, cs), dtype=torch.float32, device=device)
            basis[:M, :C] = self.basis.to(device)
            members[:, :C] = self.endmembers.to(device)
            tri = torch.cat([self.tri.reshape(-1), self.gram.reshape(-1)]).to(device=device, dtype=torch.float64).contiguous()
            self._padded = (key, basis, members, tri)
        return self._padded[1:]

    def forward(self, x, mode: str = "fcls", output: str = "abundance", members: Optional[Sequence[int]] = None, cap: int = 0):
        if isinstance(x, dict):
            x = x['image']
        code = _mode(mode)
        if output not in OUTPUTS:
            raise ValueError(f"SpectralUnmixer: output must be one of {OUTPUTS}, got {output!r}")
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("hyperpri_amd: SpectralUnmixer needs a tensor on a ROCm device; there is no CPU fallback")
        if x.requires_grad:
            raise RuntimeError("SpectralUnmixer: no autograd -- the input must not require grad")
        if x.dtype != torch.float32:
            raise ValueError(f"SpectralUnmixer: need a float32 image, got {x.dtype}")
        five = x.dim() == 5
        if five and x.shape[1] != 1 or x.dim() not in (4, 5):
            raise ValueError(f"SpectralUnmixer: need an (N, 1, C, h, w) or (N, C, h, w) image, got {tuple(x.shape)}")
        t = x[:, 0] if five else x
        if getattr(x, "_hpri_zero_padded", False):
            t._hpri_zero_padded = True
        N, C, h, w = (int(s) for s in t.shape)
        M = self.num_members
        if C != self.in_channels:
            raise ValueError(f"SpectralUnmixer: the image has {C} bands, the endmembers {self.in_channels}")
        if N * h * w == 0:
            raise ValueError("SpectralUnmixer: empty image")
        if int(cap) < 0:
            raise ValueError(f"SpectralUnmixer: cap must not be negative, got {cap}")
        picks = None if members is None else [int(m) for m in members]
        if picks is not None and (not picks or min(picks) < 0 or max(picks) >= M):
            raise ValueError(f"SpectralUnmixer: members must name endmembers in [0, {M}), got {members}")
        fg = 0
        if output == "logit":
            flagged = [m for m in range(M) if bool(self.foreground[m])] if picks is None else picks
            if not flagged:
                raise ValueError("SpectralUnmixer: output='logit' needs a foreground endmember (the foreground flags or members=)")
            for m in flagged:
                fg |= 1 << m
        with torch.cuda.device(x.device):
            src, cs = _band_input(t)
            if cs > max_channel_stride():
                raise ValueError(f"SpectralUnmixer: a channel stride of {cs} exceeds the {max_channel_stride()} the kernels take")
            basis, memb, tri = self._device_operands(x.device, cs)
            planes = torch.empty((M, N, h, w), dtype=torch.float32, device=x.device)
            extra = torch.empty((1, N, h, w), dtype=torch.float32, device=x.device) if output != "abundance" else None
            self._capped = torch.zeros(4, dtype=torch.int64, device=x.device)
            _lib.call("hpri_band_unmix", _p(src), N * h * w, cs, C, _p(basis), _p(memb), _p(tri), M, code, int(cap), fg, _p(planes),
                      _p(extra) if output == "rmse" else None, _p(extra) if output == "logit" else None, _p(self._capped), _stream())
        if output == "abundance":
            return (planes if picks is None else planes[picks]).permute(1, 0, 2, 3)
        return extra.permute(1, 0, 2, 3)


# ---------------------------------------------------------------------------------------------------
# The contract restated in numpy: the oracles of the tests
# ---------------------------------------------------------------------------------------------------
def _pixels(x, bands: int) -> np.ndarray:
    x = np.asarray(x)
    if x.shape[-1] != bands:
        raise ValueError(f"unmix: the pixels have {x.shape[-1]} bands, the basis {bands}")
    return x.astype(np.float32).astype(np.float64).reshape(-1, bands)


def _operands(basis32, tri) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    Q = np.asarray(basis32).astype(np.float32).astype(np.float64)
    R = np.triu(np.asarray(tri, dtype=np.float64))
    if Q.ndim != 2 or R.shape != (Q.shape[0], Q.shape[0]):
        raise ValueError(f"unmix: need a basis (M, C) and R (M, M), got {tuple(Q.shape)} and {tuple(R.shape)}")
    return Q, R, R.T @ R


def _subsolve(G: np.ndarray, b: np.ndarray, S: np.ndarray, eq: bool) -> Tuple[np.ndarray, np.ndarray]:
    """The minimiser on the supports ``S`` (P, M) (zero elsewhere) and its multiplier, as the kernel computes them: the Cholesky
    factor of ``G`` with the rows and columns outside the support replaced by the identity's, a zero right-hand side there."""
    P, M = b.shape
    L = np.zeros((P, M, M))
    inv = np.empty((P, M))
    for j in range(M):
        d = np.where(S[:, j], G[j, j], 1.0) - (L[:, j, :j] ** 2).sum(axis=1)
        inv[:, j] = 1.0 / np.sqrt(d)
        for i in range(j + 1, M):
            e = np.where(S[:, j] & S[:, i], G[i, j], 0.0) - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)
            L[:, i, j] = e * inv[:, j]

    def solve(rhs):
        z = rhs.copy()
        for i in range(M):
            z[:, i] = (z[:, i] - (L[:, i, :i] * z[:, :i]).sum(axis=1)) * inv[:, i]
        for i in range(M - 1, -1, -1):
            z[:, i] = (z[:, i] - (L[:, i + 1:, i] * z[:, i + 1:]).sum(axis=1)) * inv[:, i]
        return z
    u = solve(np.where(S, b, 0.0))
    lam = np.zeros(P)
    if eq:
        v = solve(np.where(S, 1.0, 0.0))
        lam = (u.sum(axis=1) - 1.0) / v.sum(axis=1)
        u = u - lam[:, None] * v
    return np.where(S, u, 0.0), lam


def unmix_reference(x, basis32, tri, mode, cap: int = 0, return_trace: bool = False):
    """``hpri_band_unmix`` in fp64 numpy on (..., C) fp32 pixels: ``(a (P, M), iterations (P,), removals (P,), capped (P,))``.
    ``basis32`` (M, C): the fp32 rows of ``Q^T``; ``tri`` = R.  ``y = x Q32^T`` and ``b = R^T y`` in fp64, then the contract's rule:

    * ``ucls`` / ``scls``: one sub-solve on the full support (``scls``: ``a = u - lambda v``, ``lambda = (sum u - 1) / sum v``).
    * ``ncls`` / ``fcls``: start from ``S = {}``, ``a = 0`` (``fcls``: ``S = {j}``, ``a = e_j``, ``j = argmax b - diag(G) / 2``).
      Sub-solve on ``S``; if ``s > 0`` on ``S``: ``a = s``, ``w = b - G a - lambda``, the largest ``w`` outside ``S`` joins if it
      exceeds ``tau = 2^-40 max diag(G) max(1, |y|_inf)``, else stop.  Otherwise ``alpha = min a / (a - s)`` over ``{i in S:
      s_i <= 0}`` (0 where ``a_i = 0``), ``a += alpha (s - a)``, whoever attains ``alpha`` or is not positive afterwards leaves
      ``S`` as an exact zero.  At most ``cap`` sub-solves (0: 3 M): a pixel that would need another keeps its ``a`` and is capped.

    ``iterations`` counts sub-solves, ``removals`` the steps of the second kind.  ``return_trace``: a fifth value, ``{"y", "b"}``."""
    code = _mode(mode)
    Q, R, G = _operands(basis32, tri)
    M = Q.shape[0]
    X = _pixels(x, Q.shape[1])
    P = X.shape[0]
    y = X @ Q.T
    b = y @ R
    eq, nonneg = bool(code & 1), bool(code & 2)
    cap = 3 * M if int(cap) == 0 else int(cap)
    its, rem, capped = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64), np.zeros(P, dtype=bool)
    if not nonneg:
        a, _ = _subsolve(G, b, np.ones((P, M), dtype=bool), eq)
        its += 1
    else:
        tau = TAU * np.diag(G).max() * np.maximum(1.0, np.abs(y).max(axis=1))
        S = np.zeros((P, M), dtype=bool)
        a = np.zeros((P, M))
        if eq:
            j = np.argmax(b - 0.5 * np.diag(G)[None, :], axis=1)           # (argmax returns the lowest index of a tie)
            S[np.arange(P), j] = True
            a[np.arange(P), j] = 1.0
        active = np.ones(P, dtype=bool)
        while active.any():
            hit = active & (its == cap)
            capped |= hit
            active &= ~hit
            rows = np.nonzero(active)[0]
            if rows.size == 0:
                break
            Sr, ar, br = S[rows], a[rows], b[rows]
            s, lam = _subsolve(G, br, Sr, eq)
            its[rows] += 1
            feasible = (~Sr | (s > 0)).all(axis=1)
            # the feasible rows
            w = np.where(Sr, -np.inf, br - s @ G - lam[:, None])
            j = np.argmax(w, axis=1)
            grow = feasible & (~Sr).any(axis=1) & (w[np.arange(rows.size), j] > tau[rows])
            # the others: a step towards s that stops at the first bound
            neg = Sr & (s <= 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(ar == 0, 0.0, ar / (ar - s))
            alpha = np.where(neg, ratio, np.inf).min(axis=1)
            alpha = np.where(np.isfinite(alpha), alpha, 0.0)
            n = ar + alpha[:, None] * (s - ar)
            out = (neg & (ratio == alpha[:, None])) | ~Sr | ~(n > 0)
            a[rows] = np.where(feasible[:, None], s, np.where(out, 0.0, n))
            Snew = np.where(feasible[:, None], Sr, Sr & ~out)
            Snew[np.nonzero(grow)[0], j[grow]] = True
            S[rows] = Snew
            rem[rows] += ~feasible
            active[rows] = grow | ~feasible
    if return_trace:
        return a, its, rem, capped, {"y": y, "b": b}
    return a, its, rem, capped


def _objective(G, b, a):
    return 0.5 * np.einsum("pi,ij,pj->p", a, G, a) - (a * b).sum(axis=1)


def unmix_bruteforce(x, basis32, tri, mode) -> np.ndarray:
    """The independent oracle: ``ucls`` is ``numpy.linalg.lstsq`` of ``R a = y``, ``scls`` the KKT system; ``ncls`` and ``fcls``
    enumerate every support, solve each in closed form (``numpy.linalg.solve`` of the restricted KKT system) and keep, per pixel,
    the non-negative candidate with the smallest objective ``1/2 a^T G a - b^T a``.  Pure numpy, for ``M <= 6``."""
    code = _mode(mode)
    Q, R, G = _operands(basis32, tri)
    M = Q.shape[0]
    if M > 6:
        raise ValueError(f"unmix_bruteforce: 2^M supports are enumerated; M = {M} exceeds 6")
    X = _pixels(x, Q.shape[1])
    P = X.shape[0]
    y = X @ Q.T
    b = y @ R
    eq, nonneg = bool(code & 1), bool(code & 2)

    def restricted(sup):
        k = len(sup)
        a = np.zeros((P, M))
        if k == 0:
            return a
        sup = list(sup)
        Gs = G[np.ix_(sup, sup)]
        if eq:
            K = np.zeros((k + 1, k + 1))
            K[:k, :k], K[:k, k], K[k, :k] = Gs, 1.0, 1.0
            rhs = np.concatenate([b[:, sup], np.ones((P, 1))], axis=1)
            a[:, sup] = np.linalg.solve(K, rhs.T).T[:, :k]
        else:
            a[:, sup] = np.linalg.solve(Gs, b[:, sup].T).T
        return a
    if not nonneg:
        if eq:
            return restricted(range(M))
        return np.linalg.lstsq(R, y.T, rcond=None)[0].T
    best = np.full((P, M), np.nan)
    best_f = np.full(P, np.inf)
    for k in range(0 if not eq else 1, M + 1):
        for sup in combinations(range(M), k):
            a = restricted(sup)
            f = np.where((a >= 0).all(axis=1), _objective(G, b, a), np.inf)
            take = f < best_f
            best[take], best_f[take] = a[take], f[take]
    return best


def unmix_bound(x, basis32, tri, a, cs: Optional[int] = None) -> np.ndarray:
    """The bound on ``|a_device - a_reference|_2`` per pixel.  With ``u = 2^-24`` and ``e_y = (cs + 1) u (|Q32| |x|)`` the error of
    the fp32 chain,

        |e_y|_2 / sigma_min(R)  +  8 M^2 2^-53 cond(G) (1 + |a|_2)  +  tau / sigma_min(R)^2  +  u |a|_2

    The first term: the constrained minimiser is the image under ``R^-1`` of the projection of ``y`` onto a convex set, and a
    projection is 1-Lipschitz, so it holds whichever active set either side ended on.  The second: the fp64 solve; the third: a
    variable the stopping threshold kept out; the last: the rounding of ``a`` to fp32."""
    Q, R, G = _operands(basis32, tri)
    M = Q.shape[0]
    X = _pixels(x, Q.shape[1])
    a = np.asarray(a, dtype=np.float64).reshape(X.shape[0], M)
    cs = _rup(Q.shape[1], 8) if cs is None else int(cs)
    sv = np.linalg.svd(R, compute_uv=False)
    ey = (cs + 1) * U * (np.abs(X) @ np.abs(Q).T)
    tau = TAU * np.diag(G).max() * np.maximum(1.0, np.abs(X @ Q.T).max(axis=1))
    na = np.sqrt((a * a).sum(axis=1))
    return (np.sqrt((ey * ey).sum(axis=1)) / sv[-1] + 8 * M * M * 2.0 ** -53 * (sv[0] / sv[-1]) ** 2 * (1 + na) + tau / sv[-1] ** 2 + U * na)


def extreme_reference(x, rows32, cs: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """One ATGP step's values in fp64 on (P, C) pixels against the fp32 ``rows32`` (K, C): ``(v (P,), bound (P,))`` with ``v`` the
    squared residual and ``bound`` the fp32 chains' error: ``e_y`` as in ``unmix_bound``; per band ``e_r = |Q32|^T e_y + (K + 1) u
    (|x| + |Q32|^T |y|)``; ``e_v = sum (2 |r| e_r + e_r^2) + (cs + 1) u sum (|r| + e_r)^2``."""
    X = np.asarray(x, dtype=np.float64)
    Q = np.asarray(rows32).astype(np.float32).astype(np.float64).reshape(-1, X.shape[1])
    K = Q.shape[0]
    cs = _rup(X.shape[1], 8) if cs is None else int(cs)
    y = X @ Q.T
    r = X - y @ Q
    ey = (cs + 1) * U * (np.abs(X) @ np.abs(Q).T)
    er = ey @ np.abs(Q) + (K + 1) * U * (np.abs(X) + np.abs(y) @ np.abs(Q))
    v = (r * r).sum(axis=1)
    return v, (2 * np.abs(r) * er + er * er).sum(axis=1) + (cs + 1) * U * ((np.abs(r) + er) ** 2).sum(axis=1)


def atgp_reference(cubes, members: int, masks=None, select: str = "all"):
    """``extract_endmembers`` in fp64 numpy on (n, H, W, C) ``cubes`` as the cache stores them: ``(picks (M, 2) int64 = (list entry,
    pixel), values (M,), gaps (M,))``.  A step takes the selected pixel with the largest ``v`` (the lowest position of a tie) and
    appends the row as the fit does.  ``gaps[k]``: the pick's ``v`` minus its bound, minus the largest ``v`` plus bound among the
    other selected pixels (``extreme_reference``) -- positive: fp32 rounding cannot change the pick."""
    _check_select(select)
    cubes = np.asarray(cubes)
    n, H, W, C = cubes.shape
    X = cubes.reshape(-1, C).astype(np.float64)
    if select == "all":
        sel = np.ones(X.shape[0], dtype=bool)
    else:
        if masks is None:
            raise ValueError("spectral: a selection needs the masks")
        m = np.asarray(masks).reshape(-1) != 0
        sel = m if select == "foreground" else ~m
    if not sel.any():
        raise ValueError("atgp_reference: no selected pixel")
    rows, rows32 = [], np.zeros((0, C), dtype=np.float32)
    picks, values, gaps = [], [], []
    for _ in range(int(members)):
        v, ev = extreme_reference(X, rows32)
        p = int(np.argmax(np.where(sel, v, -np.inf)))
        others = sel.copy()
        others[p] = False
        gaps.append((v[p] - ev[p]) - ((v + ev)[others].max() if others.any() else -np.inf))
        picks.append(divmod(p, H * W))
        values.append(v[p])
        rows.append(_atgp_row(X[p], rows))
        rows32 = np.stack(rows).astype(np.float32)
    return np.asarray(picks, dtype=np.int64), np.asarray(values), np.asarray(gaps)


__all__ = ["SpectralUnmixer", "extract_endmembers", "unmix_operands", "unmix_reference", "unmix_bruteforce", "unmix_bound", "extreme_reference",
           "atgp_reference", "max_members", "MODES", "OUTPUTS", "MAX_MEMBERS"]
