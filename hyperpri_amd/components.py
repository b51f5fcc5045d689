"""Connected components on the device: label a prediction, measure its objects, clean it (``csrc/components.hip``).

Every decision of ``evaluate.py`` is per pixel; this module knows what an *object* is.  A binary decision map -- fp32 predictions
with a threshold, decided exactly as ``SegCounts`` and ``color_segmaps`` decide, or a uint8 / bool map -- is labelled by a
union-find on the card (``label_components``), its components are measured in one pass (``component_table``: area, bounding box,
overlap with a truth map) and specks and pinholes are removed (``clean_mask``), all without the ``.cpu()`` +
``scipy.ndimage.label`` round trip.  All results are integers: labels are ``1..count`` per image in raster order of each
component's first pixel, which is the numbering of ``scipy.ndimage.label``.

``components_reference`` and ``clean_reference`` restate the contract in plain numpy (no scipy); they are the oracle of the GPU
tests.  There is no CPU fallback: tensors must live on a ROCm device.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._args import _as_images, _decision_input, _map3d, _p, _require_cuda, _require_device, _stream

TILE_H, TILE_W = 32, 64         # the tile one workgroup labels in LDS (csrc/components.hip: CC_TILE_H, CC_TILE_W)
_TRUTH_KIND = {torch.float32: 0, torch.uint8: 1, torch.int32: 2}       # hpri_cc_measure's truth_kind (int32: another label map)
STAT_NAMES = ("components_removed", "pixels_removed", "holes_filled", "pixels_filled")


def _check_connectivity(connectivity: int) -> int:
    if connectivity not in (4, 8):
        raise ValueError(f"components: connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def _workspace(x: torch.Tensor) -> torch.Tensor:
    N, h, w = (int(s) for s in x.shape)
    return torch.empty(_lib.load().hpri_cc_workspace_ints(N, h, w), dtype=torch.int32, device=x.device)


def label_components(pred: torch.Tensor, threshold: Optional[float] = None, is_logits: bool = True, connectivity: int = 8,
                     invert: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Label the foreground of a decision map (``hpri_cc_label``): returns ``(labels, counts)``, ``labels`` int32 (N, h, w) with 0
    for the background and ``1..counts[n]`` per image in raster order of each component's first pixel (the numbering of
    ``scipy.ndimage.label``), ``counts`` int32 (N,).  Images never connect to each other.

    ``pred``: a device tensor (N, h, w), (N, 1, h, w) or (h, w).  With a ``threshold`` it is fp32 and a pixel is foreground when
    ``(sigmoid(pred) if is_logits else pred) > threshold`` -- the decision ``SegCounts`` / ``color_segmaps`` take, bit for bit;
    with ``threshold=None`` it is a uint8 / bool map, foreground where non-zero.  ``invert`` labels the background instead.
    ``connectivity``: 4 or 8.  Nothing synchronises with the host; there is no CPU fallback."""
    connectivity = _check_connectivity(connectivity)
    x, kind, thr = _decision_input(pred, threshold, "label_components")
    return _label_launch(x, kind, thr, is_logits, invert, connectivity)


def _label_launch(x: torch.Tensor, kind: int, thr: float, is_logits: bool, invert: bool, connectivity: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """One ``hpri_cc_label`` over a contiguous (N, h, w) map."""
    N, h, w = (int(s) for s in x.shape)
    with torch.cuda.device(x.device):
        labels = torch.empty((N, h, w), dtype=torch.int32, device=x.device)
        counts = torch.empty((N,), dtype=torch.int32, device=x.device)
        ws = _workspace(x)
        _lib.call("hpri_cc_label", _p(x), kind, thr, int(bool(is_logits)), int(bool(invert)), N, h, w, connectivity, _p(labels),
                  _p(counts), _p(ws), ws.numel(), _stream())
    return labels, counts


def _label_truth(mask: torch.Tensor, connectivity: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``label_components`` of a fp32 truth map under the rule every kernel of the tail reads a mask by: ``int(mask) != 0``."""
    _require_cuda(mask, "truth map")
    return _label_launch(_map3d(mask.detach(), "label_components"), 2, 0.0, False, False, _check_connectivity(connectivity))


def component_table(labels: torch.Tensor, counts: torch.Tensor, truth: Optional[torch.Tensor] = None) -> Dict[str, np.ndarray]:
    """One row per component of ``label_components``' output, ordered by (image, label), as host numpy arrays: ``image``, ``label``,
    ``area``, ``y0``, ``x0``, ``y1``, ``x1`` (the inclusive bounding box) and, with ``truth`` (a device map of the labels' shape,
    fp32 or uint8 / bool), ``overlap``: the pixels of the component where ``int(truth) != 0``.  One pass over the labels on the
    device (``hpri_cc_measure``).  This is the host synchronisation of the module: the N counts come to the host first (they size
    the table), then the table itself -- six int32 per component."""
    _require_device(labels, "label map")
    _require_device(counts, "component counts")
    if labels.dtype != torch.int32 or counts.dtype != torch.int32:
        raise ValueError("component_table: labels and counts must be the int32 tensors of label_components")
    lab = _map3d(labels, "component_table")
    N, h, w = (int(s) for s in lab.shape)
    if counts.numel() != N:
        raise ValueError(f"component_table: {N} images of labels carry {counts.numel()} counts")
    kind, t = 0, None
    if truth is not None:
        _require_device(truth, "truth map")
        if truth.dtype == torch.bool:
            truth = truth.view(torch.uint8)
        if truth.dtype not in _TRUTH_KIND:
            raise ValueError(f"component_table: truth must be float32, uint8, bool or int32, got {truth.dtype}")
        if truth.numel() != lab.numel():
            raise ValueError(f"component_table: truth {tuple(truth.shape)} does not match labels {tuple(labels.shape)}")
        t = truth.reshape(N, h, w).contiguous()
        kind = _TRUTH_KIND[t.dtype]
    cnt = np.asarray(counts.tolist(), dtype=np.int64).reshape(N)
    rows = int(cnt.sum())
    with torch.cuda.device(lab.device):
        table = torch.empty((rows, 6), dtype=torch.int32, device=lab.device)
        offsets = torch.empty((N + 1,), dtype=torch.int32, device=lab.device)
        _lib.call("hpri_cc_measure", _p(lab), _p(counts.contiguous()), _p(t), kind, N, h, w, _p(table) if rows else None, rows,
                  _p(offsets), _stream())
        tab = table.cpu().numpy().astype(np.int64)
    out = {"image": np.repeat(np.arange(N, dtype=np.int64), cnt),
           "label": np.concatenate([np.arange(1, c + 1, dtype=np.int64) for c in cnt]) if N else np.zeros(0, np.int64)}
    for k, name in enumerate(("area", "y0", "x0", "y1", "x1")):
        out[name] = tab[:, k].copy()
    if truth is not None:
        out["overlap"] = tab[:, 5].copy()
    return out


def _clean_launch(x: torch.Tensor, kind: int, thr: float, is_logits: bool, min_area: int, max_hole: int, connectivity: int,
                  stats: torch.Tensor, logits_out: Optional[torch.Tensor] = None, logit: float = 0.0) -> torch.Tensor:
    """One ``hpri_cc_clean`` over a contiguous (N, h, w) map; ``stats`` (4 int64 on the device) accumulates."""
    N, h, w = (int(s) for s in x.shape)
    out = torch.empty((N, h, w), dtype=torch.uint8, device=x.device)
    ws = _workspace(x)
    _lib.call("hpri_cc_clean", _p(x), kind, thr, int(bool(is_logits)), N, h, w, connectivity, min_area, max_hole, _p(out),
              _p(logits_out), float(logit), _p(stats), _p(ws), ws.numel(), _stream())
    return out


def _check_clean_args(min_area: int, max_hole: int, connectivity: int) -> Tuple[int, int, int]:
    min_area, max_hole = int(min_area), int(max_hole)
    if min_area < 0 or max_hole < 0:
        raise ValueError(f"clean: min_area and max_hole must not be negative, got {min_area} and {max_hole}")
    return min(min_area, 2 ** 31 - 1), min(max_hole, 2 ** 31 - 1), _check_connectivity(connectivity)


def stats_dict(stats: torch.Tensor) -> Dict[str, int]:
    """The four counters of ``hpri_cc_clean`` as a dict (a host synchronisation)."""
    return dict(zip(STAT_NAMES, (int(v) for v in stats.tolist())))


def clean_mask(pred: torch.Tensor, threshold: Optional[float], min_area: int = 0, max_hole: int = 0, connectivity: int = 8,
               is_logits: bool = True) -> Tuple[torch.Tensor, Dict[str, int]]:
    """Drop specks and close pinholes (``hpri_cc_clean``): returns ``(mask, stats)``, ``mask`` the uint8 (N, h, w) cleaned decision.

    * a foreground component (``connectivity``) of fewer than ``min_area`` pixels becomes background;
    * a background component of at most ``max_hole`` pixels that touches no edge of its image becomes foreground; background
      components are labelled with the dual connectivity (4 for foreground 8, 8 for foreground 4), so with ``connectivity=8`` and
      an unbounded ``max_hole`` this is ``scipy.ndimage.binary_fill_holes``.

    Holes are found in the input decision, not after speck removal; the two edits act on disjoint pixels, so their order is
    immaterial.  ``min_area=0, max_hole=0`` returns the input decision.  ``pred`` / ``threshold`` / ``is_logits``: as
    ``label_components``.  ``stats``: ``components_removed``, ``pixels_removed``, ``holes_filled``, ``pixels_filled`` (reading them
    is the one host synchronisation)."""
    min_area, max_hole, connectivity = _check_clean_args(min_area, max_hole, connectivity)
    x, kind, thr = _decision_input(pred, threshold, "clean_mask")
    with torch.cuda.device(x.device):
        stats = torch.zeros(4, dtype=torch.int64, device=x.device)
        out = _clean_launch(x, kind, thr, is_logits, min_area, max_hole, connectivity, stats)
        return out, stats_dict(stats)


# ---------------------------------------------------------------------------------------------------
# The contract restated in numpy (no scipy): the oracle of the GPU tests
# ---------------------------------------------------------------------------------------------------
def _label_image(a: np.ndarray, connectivity: int) -> Tuple[np.ndarray, int]:
    """Union-find over one (h, w) boolean image with parent[i] <= i; labels = rank of the root in raster order."""
    h, w = a.shape
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    pairs = [(idx[:, 1:], idx[:, :-1], a[:, 1:] & a[:, :-1]), (idx[1:, :], idx[:-1, :], a[1:, :] & a[:-1, :])]
    if connectivity == 8:
        pairs += [(idx[1:, 1:], idx[:-1, :-1], a[1:, 1:] & a[:-1, :-1]), (idx[1:, :-1], idx[:-1, 1:], a[1:, :-1] & a[:-1, 1:])]
    parent = np.arange(h * w, dtype=np.int64)
    edges_a = np.concatenate([p[0][p[2]] for p in pairs])
    edges_b = np.concatenate([p[1][p[2]] for p in pairs])
    while True:                                             # label propagation to the minimum: every round lowers some parent
        root = parent
        while True:
            nxt = root[root]
            if np.array_equal(nxt, root):
                break
            root = nxt
        parent = root
        ra, rb = parent[edges_a], parent[edges_b]
        differ = ra != rb
        if not differ.any():
            break
        hi, lo = np.maximum(ra[differ], rb[differ]), np.minimum(ra[differ], rb[differ])
        np.minimum.at(parent, hi, lo)
    flat = a.reshape(-1)
    is_root = flat & (parent == np.arange(h * w))
    rank = np.cumsum(is_root)
    labels = np.where(flat, rank[parent], 0).astype(np.int32).reshape(h, w)
    return labels, int(is_root.sum())


def components_reference(binary, connectivity: int = 8) -> Tuple[np.ndarray, np.ndarray]:
    """``label_components`` in numpy: ``binary`` (h, w) or (N, h, w), foreground where non-zero; returns ``(labels, counts)`` --
    int32 labels of the input's shape, 0 the background, ``1..count`` per image in raster order of each component's first pixel;
    ``counts`` int32 (N,) (one entry for a single image).  A union-find whose roots are the smallest linear index; no scipy."""
    connectivity = _check_connectivity(connectivity)
    a, single = _as_images(binary)
    labels = np.zeros(a.shape, dtype=np.int32)
    counts = np.zeros(a.shape[0], dtype=np.int32)
    for n in range(a.shape[0]):
        labels[n], counts[n] = _label_image(a[n], connectivity)
    return (labels[0] if single else labels), counts


def table_reference(labels, counts, truth=None) -> Dict[str, np.ndarray]:
    """``component_table`` in numpy, from the labels of ``components_reference``."""
    lab = np.asarray(labels)
    lab = lab[None] if lab.ndim == 2 else lab
    tr = None if truth is None else np.asarray(truth).reshape(lab.shape).astype(np.int64) != 0
    names = ("image", "label", "area", "y0", "x0", "y1", "x1", "overlap")
    cols = {k: [] for k in names}
    big = np.iinfo(np.int64).max
    for n in range(lab.shape[0]):
        cnt = int(np.asarray(counts).reshape(-1)[n])
        ys, xs = np.nonzero(lab[n])
        k = lab[n][ys, xs].astype(np.int64) - 1
        lo_y, lo_x = np.full(cnt, big), np.full(cnt, big)
        hi_y, hi_x = np.full(cnt, -1, dtype=np.int64), np.full(cnt, -1, dtype=np.int64)
        np.minimum.at(lo_y, k, ys); np.minimum.at(lo_x, k, xs); np.maximum.at(hi_y, k, ys); np.maximum.at(hi_x, k, xs)
        over = np.bincount(k, weights=None if tr is None else tr[n][ys, xs], minlength=cnt)
        row = (np.full(cnt, n), np.arange(1, cnt + 1), np.bincount(k, minlength=cnt), lo_y, lo_x, hi_y, hi_x, over)
        for key, v in zip(names, row):
            cols[key].append(np.asarray(v).astype(np.int64))
    out = {k: np.concatenate(v) if v else np.zeros(0, np.int64) for k, v in cols.items()}
    if truth is None:
        del out["overlap"]
    return out


def clean_reference(binary, min_area: int = 0, max_hole: int = 0, connectivity: int = 8) -> Tuple[np.ndarray, Dict[str, int]]:
    """``clean_mask`` in numpy: returns ``(mask, stats)``, uint8 of the input's shape.  Foreground components (``connectivity``) of
    fewer than ``min_area`` pixels go; background components (the dual connectivity) of at most ``max_hole`` pixels whose bounding
    box touches no image edge are filled; both are found in the input."""
    min_area, max_hole, connectivity = _check_clean_args(min_area, max_hole, connectivity)
    a, single = _as_images(binary)
    out = a.copy()
    stats = dict.fromkeys(STAT_NAMES, 0)
    N, h, w = a.shape
    for n in range(N):
        lab, cnt = _label_image(a[n], connectivity)
        area = np.bincount(lab.reshape(-1), minlength=cnt + 1)
        small = area < min_area
        small[0] = False
        gone = small[lab]
        out[n][gone] = False
        stats["components_removed"] += int(small.sum())
        stats["pixels_removed"] += int(gone.sum())
        lab, cnt = _label_image(~a[n], 4 if connectivity == 8 else 8)
        area = np.bincount(lab.reshape(-1), minlength=cnt + 1)
        on_edge = np.zeros(cnt + 1, dtype=bool)
        for strip in (lab[0, :], lab[-1, :], lab[:, 0], lab[:, -1]):
            on_edge[strip] = True
        hole = ~on_edge & (area <= max_hole)
        hole[0] = False
        fill = hole[lab]
        out[n][fill] = True
        stats["holes_filled"] += int(hole.sum())
        stats["pixels_filled"] += int(fill.sum())
    res = out.astype(np.uint8)
    return (res[0] if single else res), stats
