"""Distances on the device: the exact Euclidean distance transform, surface metrics and root traits (``csrc/distance.hip``).

Everything ``evaluate.py`` reported so far counts pixels or objects; this module knows how far things are from each other.  A
binary decision map -- the inputs of ``label_components``: fp32 with a threshold, decided bit for bit as ``SegCounts`` decides, or a
uint8 / bool map -- gets

* ``distance_transform``: the squared Euclidean distance of every pixel to the nearest *site*, an int32 map::

      d2[n, y, x] = min(FAR, min over the site pixels q of image n of (y - qy)**2 + (x - qx)**2),    FAR = h*h + w*w

  ``FAR`` exceeds every attainable value, so an image without a site is ``FAR`` everywhere.  ``sites="background"``: the pixels
  whose decision is 0 (``scipy.ndimage.distance_transform_edt(a) ** 2``); ``"foreground"``: the inverted form; ``"boundary"``:
  the foreground pixels with at least one of their four edge neighbours in the background or outside the image
  (``a & ~binary_erosion(a, cross, border_value=0)``, the surface of MedPy and of the DeepMind surface-distance code).
* ``surface_distances`` / ``surface_metrics_from_hist``: per image the histogram of the distances from the boundary of the
  prediction to the boundary of the truth and back, and from it Hausdorff, HD95, the average symmetric surface distance and
  surface Dice at a tolerance.
* ``skeletonize``: Zhang-Suen parallel thinning.  P2..P9 are the eight neighbours of a pixel numbered clockwise from north (N, NE,
  E, SE, S, SW, W, NW), everything outside the image is background, B is the number of foreground neighbours and A the number of
  0 -> 1 transitions around the ring P2, P3, ..., P9, P2.  Sub-iteration 1 deletes a foreground pixel when ``2 <= B <= 6``,
  ``A == 1``, ``P2*P4*P6 == 0`` and ``P4*P6*P8 == 0``; sub-iteration 2 when the same holds with ``P2*P4*P8 == 0`` and
  ``P2*P6*P8 == 0``.  Both read the previous map in full and write a new one; pairs repeat until one deletes nothing.  The known
  properties of the rule belong to the contract: a solid 2x2 block vanishes, some diagonals stay two pixels thick.
* ``skeleton_links`` / ``root_traits``: the skeleton's pixels S, its straight links E4 (horizontally or vertically adjacent pairs)
  and its diagonal links Ed (diagonally adjacent pairs whose two shared 4-neighbours are both off the skeleton, so a corner is not
  counted twice); length ``E4 + sqrt(2) * Ed``; the diameters ``2 * sqrt(d2) - 1`` at the skeleton pixels, ``d2`` the distance to
  the background.

All device results are integers and bit-reproducible; what follows them is fp64 arithmetic on the host over the distinct values
``sqrt(k)`` in ascending ``k``.  ``edt_reference``, ``boundary_reference``, ``surface_hist_reference``, ``thin_reference`` and
``links_reference`` restate the contract in plain numpy (no scipy); they are the oracles of the GPU tests.  There is no CPU
fallback: tensors must live on a ROCm device.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._args import _as_images, _decision_input, _map3d, _p, _require_device, _stream

SITES = {"background": 0, "foreground": 1, "boundary": 2}
COL_THREADS = 256           # columns one workgroup of the column pass sweeps (csrc/distance.hip: DT_THREADS)
ROW_THREADS = 256           # threads of the workgroup that owns one row in the row pass
ROWS_PER_GROUP = 1
HIST_LDS_BINS = 4096        # histograms up to this size are reduced in LDS first (DT_HIST_LDS_BINS)
THIN_CHECK_PAIRS = 8        # the host looks at the deletion counters after this many pairs of sub-iterations
TOLERANCES = (1.0, 2.0)


def edt_max_width() -> int:
    """The widest row ``distance_transform`` takes (``hpri_edt_max_width``: the LDS budget of the row pass)."""
    return int(_lib.load().hpri_edt_max_width())


def _check_sites(sites: str) -> int:
    if sites not in SITES:
        raise ValueError(f"distance_transform: sites must be one of {tuple(SITES)}, got {sites!r}")
    return SITES[sites]


def _check_edt_shape(h: int, w: int, who: str) -> int:
    if w > edt_max_width():
        raise ValueError(f"{who}: a row of {w} pixels exceeds the {edt_max_width()} the row pass holds in LDS")
    far = int(_lib.load().hpri_edt_far(h, w))
    if far < 0:
        raise ValueError(f"{who}: h*h + w*w must be below 2^31, got {h}x{w}")
    return far


def _truth_input(truth: torch.Tensor, who: str) -> Tuple[torch.Tensor, int]:
    """A truth map as the kernels read it: fp32 by ``int(mask) != 0`` (kind 2), uint8 / bool by ``value != 0`` (kind 1)."""
    _require_device(truth, f"{who} truth map")
    if truth.dtype == torch.bool:
        truth = truth.view(torch.uint8)
    if truth.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{who}: truth must be float32, uint8 or bool, got {truth.dtype}")
    return _map3d(truth.detach(), who), 2 if truth.dtype == torch.float32 else 1


def _edt_launch(x: torch.Tensor, kind: int, thr: float, is_logits: bool, sites: int) -> torch.Tensor:
    N, h, w = (int(s) for s in x.shape)
    d2 = torch.empty((N, h, w), dtype=torch.int32, device=x.device)
    _lib.call("hpri_edt", _p(x), kind, thr, int(bool(is_logits)), sites, N, h, w, _p(d2), _stream())
    return d2


def distance_transform(pred: torch.Tensor, threshold: Optional[float] = None, is_logits: bool = True,
                       sites: str = "background") -> torch.Tensor:
    """The exact squared Euclidean distance transform (``hpri_edt``): int32 (N, h, w), ``min(FAR, squared distance to the nearest
    site of the same image)`` with ``FAR = h*h + w*w``; a site itself holds 0, an image without a site ``FAR`` everywhere.

    ``pred`` / ``threshold`` / ``is_logits``: as ``label_components``.  ``sites``: ``"background"`` (decision 0), ``"foreground"``
    or ``"boundary"`` (foreground pixels with an edge neighbour in the background or outside the image).  Two launches on the
    current stream, nothing synchronises; ``w <= edt_max_width()`` and ``h*h + w*w < 2^31``."""
    code = _check_sites(sites)
    x, kind, thr = _decision_input(pred, threshold, "distance_transform")
    _check_edt_shape(int(x.shape[1]), int(x.shape[2]), "distance_transform")
    with torch.cuda.device(x.device):
        return _edt_launch(x, kind, thr, is_logits, code)


def select_hist(pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]],
                defined: Optional[Callable[[np.ndarray], np.ndarray]] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Histograms of int32 value maps over selections (``hpri_select_stats`` + ``hpri_select_hist``): ``pairs`` holds G
    ``(values, selector)`` pairs of (N, h, w) device maps of one shape -- ``values`` int32, ``selector`` uint8 (selected where
    non-zero) or int32 (selected where zero: the sites of a distance transform).  Returns host arrays ``(hist, counts, maxima)``:
    ``hist`` int64 (N, G, bins) with ``hist[n, g, k]`` the selected pixels of value k, ``counts`` and ``maxima`` int64 (N, G).
    ``bins`` is one more than the largest maximum over the images that count -- all of them, or those where ``defined(counts)``
    (a boolean array of length N) is true; the histograms of the others are zero, and a value beyond the histogram is not counted.
    Reading counts and maxima is the one host synchronisation."""
    first = pairs[0][0]
    for values, selector in pairs:
        _require_device(values, "value map")
        _require_device(selector, "selector map")
        if values.dtype != torch.int32 or selector.dtype not in (torch.uint8, torch.int32):
            raise ValueError("select_hist: need int32 values and a uint8 or int32 selector")
        if values.dim() != 3 or values.numel() == 0 or values.numel() >= 2 ** 31 or values.shape != first.shape or selector.shape != first.shape:
            raise ValueError(f"select_hist: need non-empty (N, h, w) maps of one shape below 2^31 elements, got {tuple(values.shape)} "
                             f"and {tuple(selector.shape)}")
    pairs = [(v.contiguous(), s.contiguous()) for v, s in pairs]
    G, N, per = len(pairs), int(first.shape[0]), int(first.shape[1]) * int(first.shape[2])
    with torch.cuda.device(first.device):
        stats = torch.zeros((N, G, 2), dtype=torch.int32, device=first.device)
        for g, (v, s) in enumerate(pairs):
            _lib.call("hpri_select_stats", _p(v), _p(s), 0 if s.dtype == torch.uint8 else 1, N, per, _p(stats[:, g]), 2 * G, _stream())
        st = np.asarray(stats.tolist(), dtype=np.int64).reshape(N, G, 2)
        counts, maxima = st[..., 0], st[..., 1]
        use = np.ones(N, dtype=bool) if defined is None else np.asarray(defined(counts), dtype=bool)
        bins = int(maxima[use].max()) + 1 if use.any() else 1
        hist = torch.zeros((N, G, bins), dtype=torch.int32, device=first.device)
        for g, (v, s) in enumerate(pairs):
            _lib.call("hpri_select_hist", _p(v), _p(s), 0 if s.dtype == torch.uint8 else 1, N, per, bins, _p(hist[:, g]), G * bins, _stream())
        out = hist.cpu().numpy().astype(np.int64)
    out[~use] = 0
    return out, counts, maxima


def surface_distances(pred: torch.Tensor, threshold: Optional[float], truth: torch.Tensor,
                      is_logits: bool = True) -> Dict[str, np.ndarray]:
    """The surface distances between a prediction and a truth, per image and in both directions, as exact histograms.  A point set
    is the boundary of one map (``sites="boundary"``), its values the squared distances to the boundary of the other map.  Returns
    host arrays: ``hist`` int64 (N, 2, bins) -- ``hist[n, 0, k]`` boundary pixels of the prediction at squared distance k from the
    truth's boundary, ``hist[n, 1, k]`` the way back --, ``counts`` int64 (N, 2), the boundary pixels of prediction and truth, and
    ``max_d2`` int64 (N, 2).  An image where either map has no boundary has no surface distance: its two histograms are zero, and
    ``bins`` is sized by the other images.

    ``pred`` / ``threshold`` / ``is_logits``: as ``label_components``; ``truth``: a device map of the same shape, fp32 (read as
    ``int(mask) != 0``) or uint8 / bool.  Two distance transforms and the two passes of ``select_hist``; one synchronisation."""
    x, kind, thr = _decision_input(pred, threshold, "surface_distances")
    t, tkind = _truth_input(truth, "surface_distances")
    if t.shape != x.shape:
        raise ValueError(f"surface_distances: truth {tuple(truth.shape)} does not match the prediction {tuple(pred.shape)}")
    _check_edt_shape(int(x.shape[1]), int(x.shape[2]), "surface_distances")
    with torch.cuda.device(x.device):
        dp = _edt_launch(x, kind, thr, is_logits, SITES["boundary"])
        dt = _edt_launch(t, tkind, 0.0, False, SITES["boundary"])
        # direction 0: at the prediction's boundary (dp == 0) the distance to the truth's; direction 1: the way back
        hist, counts, maxima = select_hist([(dt, dp), (dp, dt)], defined=lambda c: (c > 0).all(axis=1))
    return {"hist": hist, "counts": counts, "max_d2": maxima}


def _value_at_rank(cum: np.ndarray, roots: np.ndarray, rank: int) -> float:
    return float(roots[np.searchsorted(cum, rank, side="right")])


def surface_metrics_from_hist(hist, tolerances: Sequence[float] = TOLERANCES) -> Dict[str, object]:
    """The boundary metrics of ``surface_distances``' histograms (host, fp64): ``hist`` (N, 2, bins) or (2, bins).  Per image

    * ``hd``: the largest distance of either direction;
    * ``hd95``: ``numpy.percentile(concatenate(both directions), 95)`` with numpy's default linear interpolation (MedPy's
      ``hd95``), taken from the cumulative counts: with n distances the virtual index is ``0.95 * (n - 1)``, the result lies
      between the sorted values at its floor and its ceiling;
    * ``assd``: the mean of the two directed mean distances (MedPy's ``assd``);
    * ``surface_dice[t]`` for each tolerance: the boundary pixels of both maps with distance ``<= t`` over all boundary pixels
      of both.

    An image with an empty direction -- either map had no boundary -- is NaN everywhere and counted in ``images_undefined``.
    Returns arrays of length N (``surface_dice``: a dict of them) and ``images_undefined``."""
    h = np.asarray(hist, dtype=np.int64)
    h = h[None] if h.ndim == 2 else h
    if h.ndim != 3 or h.shape[1] != 2:
        raise ValueError(f"surface_metrics_from_hist: need (N, 2, bins) histograms, got {h.shape}")
    N, _, bins = h.shape
    roots = np.sqrt(np.arange(bins, dtype=np.float64))
    tol = [float(t) for t in tolerances]
    out = {"hd": np.full(N, np.nan), "hd95": np.full(N, np.nan), "assd": np.full(N, np.nan),
           "surface_dice": {t: np.full(N, np.nan) for t in tol}}
    undefined = 0
    for n in range(N):
        cnt = h[n].sum(axis=1)
        if (cnt == 0).any():
            undefined += 1
            continue
        both = h[n, 0] + h[n, 1]
        total = int(both.sum())
        out["hd"][n] = roots[np.nonzero(both)[0][-1]]
        cum = np.cumsum(both)
        virtual = 0.95 * (total - 1)
        lo = int(np.floor(virtual))
        a, b = _value_at_rank(cum, roots, lo), _value_at_rank(cum, roots, min(lo + 1, total - 1))
        out["hd95"][n] = a + (b - a) * (virtual - lo)
        means = []
        for d in range(2):                                  # over the distinct values only: the sum does not depend on ``bins``
            k = np.nonzero(h[n, d])[0]
            means.append(float((h[n, d, k] * roots[k]).sum()) / cnt[d])
        out["assd"][n] = 0.5 * (means[0] + means[1])
        for t in tol:
            out["surface_dice"][t][n] = int(both[roots <= t].sum()) / total
    out["images_undefined"] = undefined
    return out


def _decide(x: torch.Tensor, kind: int, thr: float, is_logits: bool) -> torch.Tensor:
    """The uint8 decision map of a ``_decision_input`` (``hpri_thin`` with no pair)."""
    N, h, w = (int(s) for s in x.shape)
    dec = torch.empty((N, h, w), dtype=torch.uint8, device=x.device)
    other = torch.empty_like(dec)
    _lib.call("hpri_thin", _p(x), kind, thr, int(bool(is_logits)), N, h, w, 1, 0, _p(dec), _p(other), None, _stream())
    return dec


def _thin(dec: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """Thin a uint8 (N, h, w) map to convergence; returns (skeleton, pairs that deleted something)."""
    N, h, w = (int(s) for s in dec.shape)
    skel, other = dec.clone(), torch.empty_like(dec)
    deleted = torch.empty((THIN_CHECK_PAIRS, N), dtype=torch.int32, device=dec.device)
    pairs = 0
    while True:
        deleted.zero_()
        _lib.call("hpri_thin", None, 1, 0.0, 0, N, h, w, 0, THIN_CHECK_PAIRS, _p(skel), _p(other), _p(deleted), _stream())
        busy = np.asarray(deleted.tolist()).reshape(THIN_CHECK_PAIRS, N).any(axis=1)       # the host looks every THIN_CHECK_PAIRS pairs
        pairs += int(busy.sum())                # (a pair that deletes nothing ends the thinning: the busy pairs come first)
        if not busy[-1]:
            return skel, pairs


def skeletonize(pred: torch.Tensor, threshold: Optional[float] = None, is_logits: bool = True, return_pairs: bool = False):
    """Zhang-Suen thinning of a decision map (``hpri_thin``; the rule is stated in the module's docstring): uint8 (N, h, w), 1 on
    the skeleton.  One launch is one sub-iteration over the batch; the host reads the per-pair deletion counters every
    ``THIN_CHECK_PAIRS`` pairs, and pairs past convergence change nothing, so the result does not depend on that number.
    ``pred`` / ``threshold`` / ``is_logits``: as ``label_components``.  ``return_pairs``: also the number of pairs that deleted a
    pixel."""
    x, kind, thr = _decision_input(pred, threshold, "skeletonize")
    with torch.cuda.device(x.device):
        skel, pairs = _thin(_decide(x, kind, thr, is_logits))
    return (skel, pairs) if return_pairs else skel


def skeleton_links(skeleton: torch.Tensor) -> np.ndarray:
    """``hpri_skeleton_links`` of a uint8 / bool device map: host int64 (N, 3) = per image S (pixels), E4 (horizontally or
    vertically adjacent pairs), Ed (diagonally adjacent pairs whose two shared 4-neighbours are both off the map)."""
    x, _, _ = _decision_input(skeleton, None, "skeleton_links")
    N, h, w = (int(s) for s in x.shape)
    with torch.cuda.device(x.device):
        links = torch.zeros((N, 3), dtype=torch.int32, device=x.device)
        _lib.call("hpri_skeleton_links", _p(x), N, h, w, _p(links), _stream())
        return np.asarray(links.tolist(), dtype=np.int64).reshape(N, 3)


def traits_from_counts(area: int, links: Sequence[int], d2_hist: np.ndarray) -> Dict[str, object]:
    """The traits of one image from its integers (host, fp64): ``links`` = (S, E4, Ed), ``d2_hist[k]`` = skeleton pixels at squared
    distance k from the background.  ``length_px = E4 + sqrt(2) * Ed``; the diameter at a skeleton pixel is ``2 * sqrt(d2) - 1``;
    ``diameter_median_px`` is ``numpy.median`` of the diameters (the mean of the two middle ones for an even number); NaN without a
    skeleton.  ``diameter_hist`` holds the distinct ``d2`` and their counts."""
    S, E4, Ed = (int(v) for v in links)
    hist = np.asarray(d2_hist, dtype=np.int64)
    k = np.nonzero(hist)[0]
    c = hist[k]
    diam = 2.0 * np.sqrt(k.astype(np.float64)) - 1.0
    total = int(c.sum())
    mean = median = float("nan")
    if total:
        cum = np.cumsum(c)
        mean = float((c * diam).sum()) / total
        median = 0.5 * (float(diam[np.searchsorted(cum, (total - 1) // 2, side="right")]) +
                        float(diam[np.searchsorted(cum, total // 2, side="right")]))
    return {"area": int(area), "skeleton_pixels": S, "links_straight": E4, "links_diagonal": Ed, "length_px": E4 + np.sqrt(2.0) * Ed,
            "diameter_mean_px": mean, "diameter_median_px": median, "diameter_hist": (k.copy(), c.copy())}


TRAIT_NAMES = ("area", "skeleton_pixels", "links_straight", "links_diagonal", "length_px", "diameter_mean_px", "diameter_median_px",
               "diameter_hist")


def _traits(x: torch.Tensor, kind: int, thr: float, is_logits: bool) -> Dict[str, list]:
    dec = _decide(x, kind, thr, is_logits)
    skel, _ = _thin(dec)
    d2 = _edt_launch(dec, 1, 0.0, False, SITES["background"])
    area, links = skeleton_links(dec)[:, 0], skeleton_links(skel)
    hist, _, _ = select_hist([(d2, skel)])
    rows = [traits_from_counts(area[n], links[n], hist[n, 0]) for n in range(int(x.shape[0]))]
    return {name: [r[name] for r in rows] for name in TRAIT_NAMES}


def root_traits(pred: torch.Tensor, threshold: Optional[float] = None, is_logits: bool = True,
                truth: Optional[torch.Tensor] = None) -> Dict[str, object]:
    """What a root segmentation is made for, per image (lists of length N): ``area`` (foreground pixels), ``skeleton_pixels``,
    ``links_straight`` (E4), ``links_diagonal`` (Ed), ``length_px = E4 + sqrt(2) * Ed``, ``diameter_mean_px`` and
    ``diameter_median_px`` over the skeleton pixels (diameter ``2 * sqrt(d2) - 1`` with ``d2`` the squared distance to the
    background) and ``diameter_hist``, the distinct ``d2`` with their counts.  With ``truth`` (a device map of the same shape, fp32
    read as ``int(mask) != 0`` or uint8 / bool) the result has a ``"truth"`` entry with the same traits of the masks.

    Decision, thinning, links, distance transform and histogram run on the device; a few integers per image come to the host."""
    x, kind, thr = _decision_input(pred, threshold, "root_traits")
    _check_edt_shape(int(x.shape[1]), int(x.shape[2]), "root_traits")
    if truth is not None:
        t, tkind = _truth_input(truth, "root_traits")
        if t.shape != x.shape:
            raise ValueError(f"root_traits: truth {tuple(truth.shape)} does not match the prediction {tuple(pred.shape)}")
    with torch.cuda.device(x.device):
        out: Dict[str, object] = _traits(x, kind, thr, is_logits)
        if truth is not None:
            out["truth"] = _traits(t, tkind, 0.0, False)
    return out


def centerline_counts(pred: torch.Tensor, threshold: Optional[float], truth: torch.Tensor, is_logits: bool = True) -> np.ndarray:
    """The integers of the hard clDice: host int64 (N, 4) = per image ``|skel(P)|``, ``|skel(P) & T|``, ``|skel(T)|``,
    ``|skel(T) & P|`` with ``skel`` the Zhang-Suen ``skeletonize``, ``P`` the decision of ``pred`` (as ``label_components`` takes it)
    and ``T`` the truth (a device map of the same shape, fp32 read as ``int(mask) != 0`` or uint8 / bool).  Decisions, thinning and
    counting (``hpri_centerline_counts``) run on the device; four integers per image come to the host."""
    x, kind, thr = _decision_input(pred, threshold, "centerline_counts")
    t, tkind = _truth_input(truth, "centerline_counts")
    if t.shape != x.shape:
        raise ValueError(f"centerline_counts: truth {tuple(truth.shape)} does not match the prediction {tuple(pred.shape)}")
    N, h, w = (int(s) for s in x.shape)
    with torch.cuda.device(x.device):
        dp, dt = _decide(x, kind, thr, is_logits), _decide(t, tkind, 0.0, False)
        sp, st = _thin(dp)[0], _thin(dt)[0]
        counts = torch.zeros((N, 4), dtype=torch.int32, device=x.device)
        _lib.call("hpri_centerline_counts", _p(sp), _p(st), _p(dp), _p(dt), N, h * w, _p(counts), _stream())
        return np.asarray(counts.tolist(), dtype=np.int64).reshape(N, 4)


def centerline_from_counts(counts) -> Dict[str, object]:
    """The hard clDice of ``centerline_counts``' integers (host, fp64): ``counts`` (N, 4) or (4,).  Per row ``tprec = |skel(P) & T| /
    |skel(P)|``, ``tsens = |skel(T) & P| / |skel(T)|`` and ``cldice = 2 tprec tsens / (tprec + tsens)``; NaN on a zero denominator,
    as the pixel metrics.  ``pooled``: the same three from the column sums."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 4)

    def ratios(sp, spt, st, stp):
        nan = float("nan")
        tp = spt / sp if sp else nan
        ts = stp / st if st else nan
        return tp, ts, (2 * tp * ts / (tp + ts) if tp + ts > 0 else nan)
    rows = [ratios(*(int(v) for v in r)) for r in c]
    pooled = ratios(*(int(v) for v in c.sum(axis=0)))
    return {"tprec": np.array([r[0] for r in rows]), "tsens": np.array([r[1] for r in rows]), "cldice": np.array([r[2] for r in rows]),
            "pooled": {"tprec": pooled[0], "tsens": pooled[1], "cldice": pooled[2]}, "counts": c}


def centerline_metrics(pred: torch.Tensor, threshold: Optional[float], truth: torch.Tensor, is_logits: bool = True) -> Dict[str, object]:
    """``centerline_from_counts(centerline_counts(...))``: the hard clDice of a prediction against a truth, per image and pooled."""
    return centerline_from_counts(centerline_counts(pred, threshold, truth, is_logits))


# ---------------------------------------------------------------------------------------------------
# The contract restated in numpy (no scipy): the oracles of the GPU tests
# ---------------------------------------------------------------------------------------------------
_SK_PLUS = ((-1, 0), (0, -1), (0, 0), (0, 1), (1, 0))                       # E's scan order: N, W, C, E, S
_SK_WINDOW = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))      # D's: the 3x3 window row by row


def _sk_stack(a: np.ndarray, offsets, fill: float) -> np.ndarray:
    """(K, N, h, w): a[n, y + dy, x + dx] for each offset, ``fill`` outside the image."""
    N, h, w = a.shape
    p = np.pad(a, ((0, 0), (1, 1), (1, 1)), constant_values=fill)
    return np.stack([p[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy, dx in offsets])


def _sk_route(g: np.ndarray, choice: np.ndarray, offsets) -> np.ndarray:
    """Every pixel sends g to the neighbour ``offsets[choice]`` it selected; the sum of what arrives (the gather of the kernels)."""
    N, h, w = g.shape
    off = np.asarray(offsets)
    n, y, x = np.meshgrid(np.arange(N), np.arange(h), np.arange(w), indexing="ij")
    out = np.zeros_like(g)
    np.add.at(out, (n, y + off[choice, 0], x + off[choice, 1]), g)
    return out


def soft_skeleton_reference(p, iters: int, grad=None, dtype=np.float64):
    """``soft_skeleton`` in numpy, the gradient contract included: ``p`` (..., h, w), computed in ``dtype``::

        I_0 = p,  I_{j+1} = E(I_j),  d_j = I_j - D(I_{j+1}),  t_j = d_j - S_{j-1} * d_j,  S_0 = relu(d_0),  S_j = S_{j-1} + relu(t_j)

    ``E``: the minimum over the in-image part of the plus neighbourhood, ``D``: the maximum over the in-image 3x3 (for float32 ``t_j``
    is formed in fp64 and rounded once, as the kernels' fma).  Returns ``S``; with ``grad`` (the gradient wrt ``S``, p's shape) the
    tuple ``(S, gp, A)``.  Backward, level by level from ``j = iters`` with ``gS`` (wrt ``S_j``) and ``gE`` (wrt ``I_{j+1}``)::

        gd = gS * (1 - S_{j-1}) * [t_j > 0]   (j = 0: gS * [d_0 > 0]),   gS <- gS * (1 - d_j * [t_j > 0])
        gI_j = gd + route_E(gE + route_D(-gd)),   gE <- gI_j,   gp = gI_0

    with ``relu'(t) = [t > 0]`` and a min or max sending its whole gradient to its FIRST optimum in scan order (E: N, W, C, E, S; D:
    the window row by row).  ``A`` is the same run with the absolute value of every routed term: the scale of the rounding error of
    ``gp``."""
    src = np.asarray(p)
    dtype = np.dtype(dtype).type
    a = np.ascontiguousarray(src, dtype=dtype).reshape((-1,) + src.shape[-2:])
    iters = int(iters)
    I, d, on, S = [a], [], [], []
    amin, amax = [], []
    for j in range(iters + 1):
        e = _sk_stack(I[j], _SK_PLUS, np.inf)
        amin.append(e.argmin(axis=0))
        I.append(e.min(axis=0))
        m = _sk_stack(I[j + 1], _SK_WINDOW, -np.inf)
        amax.append(m.argmax(axis=0))
        d.append(I[j] - m.max(axis=0))
        if j == 0:
            t = d[0]
            S.append(np.maximum(t, 0))
        else:
            t = (d[j].astype(np.float64) - S[j - 1].astype(np.float64) * d[j].astype(np.float64)).astype(dtype)
            S.append(S[j - 1] + np.maximum(t, 0))
        on.append(t > 0)
    out = S[iters].reshape(src.shape)
    if grad is None:
        return out
    gS = np.ascontiguousarray(np.asarray(grad), dtype=dtype).reshape(a.shape)
    aS = np.abs(gS)
    gE, aE = np.zeros_like(a), np.zeros_like(a)
    one = dtype(1)
    for j in range(iters, -1, -1):
        keep = one - S[j - 1] if j > 0 else np.ones_like(a)
        gd, ad = np.where(on[j], gS * keep, 0), np.where(on[j], aS * np.abs(keep), 0)
        fac = one - np.where(on[j], d[j], 0)
        gS, aS = gS * fac, aS * np.abs(fac)
        gE = gd + _sk_route(gE + _sk_route(-gd, amax[j], _SK_WINDOW), amin[j], _SK_PLUS)
        aE = ad + _sk_route(aE + _sk_route(ad, amax[j], _SK_WINDOW), amin[j], _SK_PLUS)
    return out, gE.reshape(src.shape), aE.reshape(src.shape)
def boundary_reference(binary) -> np.ndarray:
    """The boundary of a (h, w) or (N, h, w) map in numpy, bool of the input's shape: foreground pixels with at least one of their
    four edge neighbours in the background or outside the image."""
    a, single = _as_images(binary)
    p = np.pad(a, ((0, 0), (1, 1), (1, 1)))
    inner = p[:, :-2, 1:-1] & p[:, 2:, 1:-1] & p[:, 1:-1, :-2] & p[:, 1:-1, 2:]
    out = a & ~inner
    return out[0] if single else out


def _sites_reference(a: np.ndarray, sites: str) -> np.ndarray:
    _check_sites(sites)
    return ~a if sites == "background" else a if sites == "foreground" else boundary_reference(a)


def _edt_image(s: np.ndarray) -> np.ndarray:
    """One (h, w) boolean site map -> int64 squared distances, FAR = h*h + w*w where there is no site."""
    h, w = s.shape
    far, none = h * h + w * w, h + w
    g = np.full((h, w), none, dtype=np.int64)
    run = np.full(w, none, dtype=np.int64)
    for y in range(h):                                      # down: rows since the last site of the column
        run = np.where(s[y], 0, np.minimum(run + 1, none))
        g[y] = run
    run = np.full(w, none, dtype=np.int64)
    for y in range(h - 1, -1, -1):                          # up
        run = np.where(s[y], 0, np.minimum(run + 1, none))
        g[y] = np.minimum(g[y], run)
    f = np.where(g >= none, far, g * g)
    best = f.copy()
    rows = np.nonzero((f < far).any(axis=1))[0]             # (a row without any site in reach stays FAR)
    for k in range(1, w):                                   # the lower envelope of f[x'] + (x - x')^2, offset by offset
        rows = rows[best[rows].max(axis=1) > k * k]         # a row is finished once no farther column can win in it
        if len(rows) == 0:
            break
        b, fr = best[rows], f[rows]
        b[:, k:] = np.minimum(b[:, k:], fr[:, :-k] + k * k)
        b[:, :-k] = np.minimum(b[:, :-k], fr[:, k:] + k * k)
        best[rows] = b
    return best


def edt_reference(binary, sites: str = "background") -> np.ndarray:
    """``distance_transform`` in numpy (a separable pass, no scipy): ``binary`` (h, w) or (N, h, w), foreground where non-zero;
    int32 of the input's shape."""
    a, single = _as_images(binary)
    s = _sites_reference(a, sites)
    out = np.stack([_edt_image(s[n]) for n in range(a.shape[0])]).astype(np.int32)
    return out[0] if single else out


def surface_hist_reference(pred, truth) -> Dict[str, np.ndarray]:
    """``surface_distances`` in numpy from two binary maps (h, w) or (N, h, w): ``hist``, ``counts``, ``max_d2``."""
    a, _ = _as_images(pred)
    b, _ = _as_images(truth)
    N = a.shape[0]
    ba, bb = boundary_reference(a), boundary_reference(b)
    da, db = edt_reference(a, "boundary").astype(np.int64), edt_reference(b, "boundary").astype(np.int64)
    values = [[db[n][ba[n]], da[n][bb[n]]] for n in range(N)]
    counts = np.array([[len(v) for v in row] for row in values], dtype=np.int64).reshape(N, 2)
    maxima = np.array([[int(v.max()) if len(v) else 0 for v in row] for row in values], dtype=np.int64).reshape(N, 2)
    defined = (counts > 0).all(axis=1)
    bins = int(maxima[defined].max()) + 1 if defined.any() else 1
    hist = np.zeros((N, 2, bins), dtype=np.int64)
    for n in np.nonzero(defined)[0]:
        for d in range(2):
            hist[n, d] = np.bincount(values[n][d], minlength=bins)
    return {"hist": hist, "counts": counts, "max_d2": maxima}


def _thin_pass(a: np.ndarray, sub: int) -> np.ndarray:
    p = np.pad(a, ((0, 0), (1, 1), (1, 1))).astype(np.int64)
    c = p[:, 1:-1, 1:-1]
    p2, p3, p4, p5 = p[:, :-2, 1:-1], p[:, :-2, 2:], p[:, 1:-1, 2:], p[:, 2:, 2:]
    p6, p7, p8, p9 = p[:, 2:, 1:-1], p[:, 2:, :-2], p[:, 1:-1, :-2], p[:, :-2, :-2]
    ring = (p2, p3, p4, p5, p6, p7, p8, p9, p2)
    B = sum(ring[:8])
    A = sum((1 - ring[i]) * ring[i + 1] for i in range(8))
    first, second = (p2 * p4 * p6, p4 * p6 * p8) if sub == 0 else (p2 * p4 * p8, p2 * p6 * p8)
    delete = (c == 1) & (B >= 2) & (B <= 6) & (A == 1) & (first == 0) & (second == 0)
    return a & ~delete


def thin_reference(binary, return_pairs: bool = False):
    """``skeletonize`` in numpy: ``binary`` (h, w) or (N, h, w); uint8 of the input's shape.  Each image is thinned until a pair of
    sub-iterations deletes nothing; ``return_pairs``: also the largest number of deleting pairs an image took."""
    a, single = _as_images(binary)
    a, pairs = a.copy(), 0
    while True:
        nxt = _thin_pass(_thin_pass(a, 0), 1)
        if np.array_equal(nxt, a):
            break
        a, pairs = nxt, pairs + 1
    out = a.astype(np.uint8)
    out = out[0] if single else out
    return (out, pairs) if return_pairs else out


def links_reference(skeleton) -> np.ndarray:
    """``skeleton_links`` in numpy: int64 (N, 3) = S, E4, Ed per image ((3,) for a single (h, w) map)."""
    a, single = _as_images(skeleton)
    p = np.pad(a, ((0, 0), (0, 1), (1, 1)))
    c, right, left = p[:, :-1, 1:-1], p[:, :-1, 2:], p[:, :-1, :-2]
    down, down_right, down_left = p[:, 1:, 1:-1], p[:, 1:, 2:], p[:, 1:, :-2]
    S = c.sum(axis=(1, 2))
    E4 = (c & right).sum(axis=(1, 2)) + (c & down).sum(axis=(1, 2))
    Ed = (c & down_right & ~right & ~down).sum(axis=(1, 2)) + (c & down_left & ~left & ~down).sum(axis=(1, 2))
    out = np.stack([S, E4, Ed], axis=1).astype(np.int64)
    return out[0] if single else out


def traits_reference(binary) -> Dict[str, list]:
    """``root_traits`` in numpy from a binary (h, w) or (N, h, w) map, through the restatements above."""
    a, _ = _as_images(binary)
    skel = thin_reference(a).astype(bool)
    d2 = edt_reference(a, "background").astype(np.int64)
    links = links_reference(skel).reshape(-1, 3)
    rows = []
    for n in range(a.shape[0]):
        v = d2[n][skel[n]]
        rows.append(traits_from_counts(int(a[n].sum()), links[n], np.bincount(v, minlength=1)))
    return {name: [r[name] for r in rows] for name in TRAIT_NAMES}
