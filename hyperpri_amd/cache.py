"""Device-resident cube cache with a fused crop / flip batch gather -- opt-in, ``src/dataset.py`` stays untouched.

A HyperPRI fold has 43-45 training cubes; band-sliced and padded they are 25 GB of the card's 288 GB
as fp32.  ``CubeStager`` (ingest.py) still sends every batch over PCIe on every step of every epoch; ``CubeCache`` loads
the split ONCE and assembles each batch from HBM with one gather pass (csrc/cache.hip) that also applies the reference's
only augmentation -- ``RandomCrop(patch_size)`` with one RNG state for image and mask (params_HyperPRI.py:201-203,
dataset.py:283-293) -- and, for the same price, flips:

    cache = CubeCache(capacity=45, height=608, width=968, bands=299, hsi_lo=25, hsi_hi=263, device="cuda:0")
    cache.fill((cube_hwb, mask, name) for ... in training_split)      # (H, W, B) arrays as ENVI delivers them
    for epoch in range(num_epochs):
        for batch in cache.epoch(batch_size=2, generator=g, patch=(512, 512), random_crop=True, flips=True):
            loss = model.training_step(batch, 0)                       # batch = {'image', 'mask', 'index'}
            loss.backward(); optimizer.step(); optimizer.zero_grad()

* a slot holds bands ``[hsi_lo, hsi_hi)`` of one (H, W, B) cube at channel stride ``cs = roundup(C, 8)`` with zero pad
  channels, as fp32 (default) or fp16.  ``store_dtype=torch.float16`` halves the memory and the bytes every gather reads;
  it quantises reflectance to 11 bits -- NOT the reference's numerics, opt-in (the same trade as ``CubeStager``'s fp16
  source).  Masks are stored as uint8;
* ``batch()`` / ``epoch()`` hand back the reference's logical shapes -- ``image`` (N,1,C,h,w) for CubeNET
  (``unsqueeze_hsi``, dataset.py:269-270) or (N,C,h,w) for SpectralUNET, ``mask`` (N,1,h,w) fp32 -- as ordinary strided
  views of a zero-padded channels-last buffer, marked ``_hpri_zero_padded`` like ``CubeStager.submit()``'s: the
  hyperpri_amd networks consume them in place, no layout kernel runs;
* image and mask of a sample are cut by the same table entry ``{slot, top, left, flags}``: they always receive the same
  window and the same flips.

Epoch plan and draw order (``plan_epoch``, a pure host function).  With n cubes and one ``torch.Generator``:
  1. ``order = torch.randperm(n, generator=g)`` when shuffling, else ``range(n)``;
  2. with ``random_crop``: ``top = torch.randint(0, H - h + 1, (n,), generator=g)``, then
     ``left = torch.randint(0, W - w + 1, (n,), generator=g)`` (without it a smaller ``patch`` is centred);
  3. with ``flips``: ``flip_h = torch.randint(0, 2, (n,), generator=g)``, then ``flip_w`` likewise.
Entry j of every draw belongs to the j-th sample SERVED (position j of ``order``).  All draws happen before the first
step, the whole epoch's table is uploaded once, and a step is two kernel launches on the caller's stream: no
host-to-device copy, no host synchronisation.

Output slots.  Batches rotate over ``out_slots`` buffers; a batch stays valid until ``out_slots`` further batches have
been requested.  What orders the gather that overwrites a buffer behind the step that read it:
  * the gather runs on the CALLER's current stream, so everything that step enqueued on that stream -- forward,
    backward, optimizer -- precedes it;
  * the engine runs weight gradients on a second stream (``engine._side``), and the first layer's reads the input buffer
    itself.  Every backward ends by joining that stream into the stream it runs on: ``_HipFn._backward_impl`` calls
    ``join_side`` after ``Tape.backward`` (the segmented chain joins with the node that holds slice 0, which is the one
    that owns the first layer), and ``Tape.backward``'s tail makes the current stream wait for its hand-over stream.
    Once ``loss.backward()`` has returned, the current stream is therefore already ordered behind every reader of the
    batch: on one stream no extra wait is needed, with ``out_slots=1`` as well;
  * the ordering IS missing when a buffer comes round on a different stream than the one its previous batch was handed
    out on.  There the cache waits as ``CubeStager.submit()`` does: for the event ``release()`` recorded (``_consumed``)
    or, without one, for everything enqueued so far on that earlier stream.
Requesting batch k + out_slots BEFORE the backward of batch k has been enqueued is outside this contract.

Augmentation (``CubeAugment``, ``plan_epoch_augmented``, csrc/cache_warp.hip) -- opt-in; without it nothing above changes.
A sample that asks for more than a crop and flips is served by the warp kernel pair: the window is resampled through one
affine map (bilinear for the cube, nearest neighbour for the mask), scaled by ``gain``, shifted by ``offset`` and a run of
bands is zeroed.  Per sample one 64-byte entry of 16 32-bit words:
    ``[slot, drop_lo, drop_n, 0, a00, a01, cx, a10, a11, cy, gain, offset, 0, 0, 0, 0]``  (words 4..11 hold fp32 bits)
    output pixel (y, x):  u = x - (w-1)/2, v = y - (h-1)/2;  source column sx = a00 u + a01 v + cx, row sy = a10 u + a11 v + cy
    A = (1/zoom) [[cos t, -sin t], [sin t, cos t]], column 0 negated by a column flip, column 1 by a row flip (fp64, rounded
    once to fp32; multiples of 90 degrees use exact 0 / +-1); cx = left + (w-1)/2 + shift_x, cy = top + (h-1)/2 + shift_y.
Draw order of ``plan_epoch_augmented``: first ``plan_epoch``'s draws, unchanged; then ten vectors
``torch.rand(n, dtype=torch.float64, generator=g)``, ALL of them whatever the settings are (a knob never shifts another
quantity's stream), entry j again for the j-th sample served:
  1. ``apply``: the sample is warped geometrically when ``apply < p``  (else angle 0, zoom 1, no shift);
  2. ``angle = (2 r - 1) * rotate`` degrees;
  3. ``zoom = exp(log(lo) + r * (log(hi) - log(lo)))``  (above 1 magnifies: the source step is 1 / zoom);
  4. ``shift_x = (2 r - 1) * shift``;   5. ``shift_y`` likewise;
  6. ``gain = lo + r * (hi - lo)``;     7. ``offset`` likewise  (both for every sample, warped or not);
  8. ``drop``: a run of bands is dropped when ``drop < probability``;
  9. ``run = min(1 + floor(r * max_run), max_run, C)``;   10. ``drop_lo = min(floor(r * (C - run + 1)), C - run)``.
A batch in which no sample needs the warp (identity geometry, gain 1, offset 0, no drop) goes through the plain gather.

Deformation (``CubeDeform``, ``plan_epoch_deformed``, csrc/cache_warp.hip, csrc/cache_deform.hip) -- opt-in again; without it nothing above changes.
Elastic deformation, additive Gaussian noise and CutMix in the same pass.  Beside the warp entry a second 64-byte record per sample:
    ``[mix_from, ry0, ry1, rx0, rx1, nodes_off, gy, gx, inv_pitch, noise_sigma, k0, k1, 0, 0, 0, 0]``  (words 8, 9 hold fp32 bits)
  * elastic: a coarse lattice of random displacements (``(gy, gx, 2)`` fp32 = (dx, dy) in output pixels, nodes ``pitch`` pixels apart,
    ``elastic_lattice``), interpolated by the uniform cubic B-spline into a per-pixel field that is added to the output coordinate
    before the affine map -- the U-Net paper's form.  Cube and mask read the same field;
  * noise: ``out = sigma * z + base`` with z from Philox4x32-10 under the sample's key ``(k0, k1)`` at the counter
    ``(y * w + x) * (cs / 4) + c / 4`` (one call per channel quad) through Box-Muller.  Dropped and pad channels stay 0, the mask is
    not touched;
  * CutMix: the pixels of the rectangle ``[ry0, ry1) x [rx0, rx1)`` of sample s come from batch sample ``mix_from`` -- its slot, warp
    entry and elastic field, image and mask alike (hard labels) --, the noise stays s's own.
Draw order of ``plan_epoch_deformed``: first ``plan_epoch_augmented``'s draws, unchanged; then, ALL of them whatever the settings
are, seven vectors ``torch.rand(n, dtype=torch.float64, generator=g)``:
  1. ``elastic``: the sample is deformed when ``elastic < probability``;
  2. ``noise_sigma = lo + r * (hi - lo)``;
  3. ``cut``: the sample receives a rectangle when ``cut < probability``;
  4. ``cut_h``: ``rh = clamp(round((min + r * (max - min)) * h), 1, h)``;   5. ``cut_w`` likewise with w;
  6. ``cut_y``: ``ry0 = min(floor(r * (h - rh + 1)), h - rh)``;             7. ``cut_x`` likewise;
  8. ``torch.randint(0, 2**32, (n, 2), dtype=torch.int64, generator=g)``: the noise keys;
  9. last, and only when the elastic probability and sigma are both above 0:
     ``torch.randn(n, gy, gx, 2, dtype=torch.float64, generator=g) * sigma``, rounded once to fp32 (last, so that its size shifts
     no other quantity's stream).
The CutMix partner of the j-th sample of a batch is the sample before it in that batch, cyclically (no draw); a batch of one has no
CutMix.  A batch in which no sample needs any of the three goes through the warp pair or the plain gather as before.

Views for test-time augmentation (``view``, ``epoch_views``, ``view_warp_entries``; hyperpri_amd/tta.py) -- opt-in as well.  The
eight dihedral views of a whole frame, bit for bit: the four that keep the axes through the plain gather's flip flags, the four
that swap them through the warp kernels with a (W, H) window and entries of exact 0 / +-1 (``view_warp_entries`` says why every
source coordinate is then an integer in fp32), written into the same output slots.
"""
from __future__ import annotations

import ctypes
import logging
import math
from dataclasses import dataclass
from typing import Iterable, Iterator, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._args import _p, _rup

_log = logging.getLogger("hyperpri_amd")
_DT = {torch.float32: 0, torch.float16: 1}


def _hw(patch, H: int, W: int) -> Tuple[int, int]:
    if patch is None:
        return H, W
    h, w = (patch, patch) if isinstance(patch, int) else (int(patch[0]), int(patch[1]))
    if not (0 < h <= H and 0 < w <= W):
        raise ValueError(f"CubeCache: a {h}x{w} window does not fit a {H}x{W} frame")
    return h, w


class EpochPlan(NamedTuple):
    order: torch.Tensor                 # (m,) int64: the cache slot of every sample served, in order
    table: torch.Tensor                 # (m, 4) int32: {slot, top, left, flags} (flags bit 0: flip rows, bit 1: flip columns)
    batches: List[Tuple[int, int]]      # [start, stop) rows of ``table`` per step
    window: Tuple[int, int]             # (h, w)


def plan_epoch(n: int, batch_size: int, frame: Tuple[int, int], patch=None, shuffle: bool = True, random_crop: bool = False,
               flips: bool = False, drop_last: bool = False, generator: Optional[torch.Generator] = None) -> EpochPlan:
    """One epoch over ``n`` cached cubes as a host-side table (no device, no library): the draw order is the module
    docstring's.  ``drop_last`` drops the trailing incomplete batch AFTER all n draws."""
    if n <= 0 or batch_size <= 0:
        raise ValueError("plan_epoch: n and batch_size must be positive")
    H, W = frame
    h, w = _hw(patch, H, W)
    order = torch.randperm(n, generator=generator) if shuffle else torch.arange(n)
    if random_crop:
        top = torch.randint(0, H - h + 1, (n,), generator=generator)
        left = torch.randint(0, W - w + 1, (n,), generator=generator)
    else:
        top = torch.full((n,), (H - h) // 2, dtype=torch.int64)
        left = torch.full((n,), (W - w) // 2, dtype=torch.int64)
    if flips:
        fh = torch.randint(0, 2, (n,), generator=generator)
        fw = torch.randint(0, 2, (n,), generator=generator)
    else:
        fh = fw = torch.zeros(n, dtype=torch.int64)
    m = n - n % batch_size if drop_last else n
    table = torch.stack([order, top, left, fh + 2 * fw], dim=1)[:m].to(torch.int32).contiguous()
    batches = [(s, min(s + batch_size, m)) for s in range(0, m, batch_size)]
    return EpochPlan(order[:m].clone(), table, batches, (h, w))


def _pair(v, what: str) -> Tuple[float, float]:
    lo, hi = (v, v) if isinstance(v, (int, float)) else v
    lo, hi = float(lo), float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
        raise ValueError(f"CubeAugment: {what} must be a finite (lo, hi) range with lo <= hi, got {v!r}")
    return lo, hi


@dataclass(frozen=True)
class CubeAugment:
    """What ``plan_epoch_augmented`` draws per sample (module docstring); the defaults are neutral.  Needs no device."""
    p: float = 0.0                                  # probability that a sample is warped geometrically at all
    rotate: float = 0.0                             # degrees: the angle is uniform in [-rotate, rotate]
    zoom: Tuple[float, float] = (1.0, 1.0)          # (lo, hi), log-uniform; above 1 magnifies
    shift: float = 0.0                              # pixels: the window centre moves uniformly in [-shift, shift] per axis
    gain: Tuple[float, float] = (1.0, 1.0)          # (lo, hi), uniform
    offset: Tuple[float, float] = (0.0, 0.0)        # (lo, hi), uniform
    band_drop: Tuple[float, int] = (0.0, 1)         # (probability, longest run of bands set to zero)

    def __post_init__(self):
        for name in ("p", "rotate", "shift"):
            v = float(getattr(self, name))
            if not math.isfinite(v):
                raise ValueError(f"CubeAugment: {name} must be finite, got {v!r}")
            object.__setattr__(self, name, v)
        if not 0.0 <= self.p <= 1.0:
            raise ValueError(f"CubeAugment: p must lie in [0, 1], got {self.p!r}")
        if self.rotate < 0 or self.shift < 0:
            raise ValueError("CubeAugment: rotate and shift are half-widths and must not be negative")
        z = _pair(self.zoom, "zoom")
        if z[0] <= 0 or z[0] < 1 / 16 or z[1] > 16:
            raise ValueError(f"CubeAugment: zoom must lie in [1/16, 16], got {self.zoom!r}")
        object.__setattr__(self, "zoom", z)
        object.__setattr__(self, "gain", _pair(self.gain, "gain"))
        object.__setattr__(self, "offset", _pair(self.offset, "offset"))
        prob, run = self.band_drop
        prob = float(prob)
        if not (math.isfinite(prob) and 0.0 <= prob <= 1.0):
            raise ValueError(f"CubeAugment: the band_drop probability must lie in [0, 1], got {prob!r}")
        if isinstance(run, float) and not run.is_integer() or int(run) < 1:
            raise ValueError(f"CubeAugment: the band_drop run must be a whole number of at least 1, got {run!r}")
        object.__setattr__(self, "band_drop", (prob, int(run)))


def warp_matrix(angle: float, zoom: float, flip_h: bool, flip_w: bool) -> Tuple[float, float, float, float]:
    """``(a00, a01, a10, a11)`` in fp64: (1/zoom) * rotation by ``angle`` degrees, column 0 negated by a column flip and
    column 1 by a row flip.  Multiples of 90 degrees use exact 0 and +-1."""
    k = angle / 90.0
    if k == math.floor(k):
        c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(k) % 4]
    else:
        c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    r = 1.0 / zoom
    a00, a01, a10, a11 = r * c, -(r * s), r * s, r * c
    if flip_w:
        a00, a10 = -a00, -a10
    if flip_h:
        a01, a11 = -a01, -a11
    return a00 + 0.0, a01 + 0.0, a10 + 0.0, a11 + 0.0          # (+ 0.0: no negative zeros in the table)


def warp_entries(slots, tops, lefts, flip_h, flip_w, window, angle, zoom, shift_x, shift_y, gain, offset, drop_lo, drop_n) -> torch.Tensor:
    """The (n, 16) int32 entry array of the warp kernels (module docstring) from per-sample sequences: fp64 arithmetic,
    rounded once to fp32."""
    h, w = window
    n = len(slots)
    f = np.zeros((n, 8), dtype=np.float64)
    for j in range(n):
        a00, a01, a10, a11 = warp_matrix(float(angle[j]), float(zoom[j]), bool(flip_h[j]), bool(flip_w[j]))
        f[j] = (a00, a01, float(lefts[j]) + (w - 1) / 2 + float(shift_x[j]), a10, a11, float(tops[j]) + (h - 1) / 2 + float(shift_y[j]),
                float(gain[j]), float(offset[j]))
    e = np.zeros((n, 16), dtype=np.int32)
    e[:, 0] = np.asarray(slots, dtype=np.int64)
    e[:, 1] = np.asarray(drop_lo, dtype=np.int64)
    e[:, 2] = np.asarray(drop_n, dtype=np.int64)
    e[:, 4:12] = f.astype(np.float32).view(np.int32)
    return torch.from_numpy(e)


# the matrices (a00, a01, a10, a11) of the four views that swap the axes (hyperpri_amd/tta.py): exact 0 / +-1
_VIEW_MATRIX = {"rot90": (0.0, -1.0, 1.0, 0.0), "rot270": (0.0, 1.0, -1.0, 0.0), "transpose": (0.0, 1.0, 1.0, 0.0),
                "antitranspose": (0.0, -1.0, -1.0, 0.0)}


def view_warp_entries(slots, view: str, frame: Tuple[int, int]) -> torch.Tensor:
    """The (n, 16) int32 warp entries with which ``CubeCache.view`` makes ``view`` -- ``rot90``, ``rot270``, ``transpose`` or
    ``antitranspose`` -- of whole ``frame`` = (H, W) cubes: the output window is (W, H), the matrix holds exact 0 / +-1, the centre
    is the frame's, ``((W - 1) / 2, (H - 1) / 2)``, gain 1, offset 0, nothing dropped (a pure host function).

    Every source coordinate is an integer in fp32, for even and odd H, W alike.  The kernels form ``u = x - (H - 1) / 2`` and
    ``v = y - (W - 1) / 2`` for output pixel (y, x) of the (W, H) window, ``sx = fma(a00, u, fma(a01, v, cx))`` and
    ``sy = fma(a10, u, fma(a11, v, cy))``.  With a00 = a11 = 0 these are ``sx = +-v + (W - 1) / 2`` and ``sy = +-u + (H - 1) / 2``
    (the product with 0 adds a signed zero).  ``v`` and ``cx`` are both integers (odd W) or both half-integers (even W), and so
    are ``u`` and ``cy`` with H: each sum or difference is an integer below 2^12, exact in fp32.  The bilinear weights are then 1
    for one neighbour and 0 for the other three, which are not loaded: the stored bits come out."""
    if view not in _VIEW_MATRIX:
        raise ValueError(f"view_warp_entries: {view!r} does not swap the axes (the plain gather makes it)")
    H, W = frame
    n = len(slots)
    a00, a01, a10, a11 = _VIEW_MATRIX[view]
    f = np.empty((n, 8), dtype=np.float64)
    f[:] = (a00, a01, (W - 1) / 2, a10, a11, (H - 1) / 2, 1.0, 0.0)
    e = np.zeros((n, 16), dtype=np.int32)
    e[:, 0] = np.asarray(slots, dtype=np.int64)
    e[:, 4:12] = f.astype(np.float32).view(np.int32)
    return torch.from_numpy(e)


class AugmentedPlan(NamedTuple):
    order: torch.Tensor                 # as EpochPlan
    table: torch.Tensor                 # (m, 4) int32: the plain table, exactly plan_epoch's
    entries: torch.Tensor               # (m, 16) int32: the warp entries (words 4..11 hold fp32 bits)
    batches: List[Tuple[int, int]]
    window: Tuple[int, int]
    warped: List[bool]                  # per batch: some sample needs the warp kernels


def plan_epoch_augmented(n: int, batch_size: int, frame: Tuple[int, int], channels: int, augment: Optional[CubeAugment] = None,
                         patch=None, shuffle: bool = True, random_crop: bool = False, flips: bool = False, drop_last: bool = False,
                         generator: Optional[torch.Generator] = None) -> AugmentedPlan:
    """``plan_epoch`` plus the augmentation draws of the module docstring (a pure host function; ``channels`` is the band
    count C the dropped runs lie in).  Order, windows and flips are ``plan_epoch``'s for the same generator state."""
    if channels <= 0:
        raise ValueError("plan_epoch_augmented: channels must be positive")
    aug = CubeAugment() if augment is None else augment
    plan = plan_epoch(n, batch_size, frame, patch, shuffle, random_crop, flips, drop_last, generator)
    r = [torch.rand(n, dtype=torch.float64, generator=generator).numpy() for _ in range(10)]
    m = plan.table.shape[0]
    apply = r[0] < aug.p
    angle = np.where(apply, (2 * r[1] - 1) * aug.rotate, 0.0)
    llo, lhi = math.log(aug.zoom[0]), math.log(aug.zoom[1])
    zoom = np.where(apply, np.exp(llo + r[2] * (lhi - llo)), 1.0)
    sx = np.where(apply, (2 * r[3] - 1) * aug.shift, 0.0)
    sy = np.where(apply, (2 * r[4] - 1) * aug.shift, 0.0)
    gain = aug.gain[0] + r[5] * (aug.gain[1] - aug.gain[0])
    offset = aug.offset[0] + r[6] * (aug.offset[1] - aug.offset[0])
    prob, max_run = aug.band_drop
    run = np.minimum(1 + np.floor(r[8] * max_run).astype(np.int64), min(max_run, channels))
    drop_n = np.where(r[7] < prob, run, 0)
    drop_lo = np.where(drop_n > 0, np.minimum(np.floor(r[9] * (channels - run + 1)).astype(np.int64), channels - run), 0)
    t = plan.table.numpy()
    entries = warp_entries(t[:, 0], t[:, 1], t[:, 2], t[:, 3] & 1, t[:, 3] & 2, plan.window, angle[:m], zoom[:m], sx[:m], sy[:m],
                           gain[:m], offset[:m], drop_lo[:m], drop_n[:m])
    needs = (angle != 0) | (zoom != 1) | (sx != 0) | (sy != 0) | (gain != 1) | (offset != 0) | (drop_n > 0)
    warped = [bool(needs[s:e].any()) for s, e in plan.batches]
    return AugmentedPlan(plan.order, plan.table, entries, plan.batches, plan.window, warped)


def _finite(v, what: str, n: int) -> Tuple[float, ...]:
    try:
        t = tuple(float(e) for e in v)
    except TypeError:
        t = ()
    if len(t) != n or not all(math.isfinite(e) for e in t):
        raise ValueError(f"CubeDeform: {what} must be {n} finite numbers, got {v!r}")
    return t


@dataclass(frozen=True)
class CubeDeform:
    """What ``plan_epoch_deformed`` draws per sample beyond ``CubeAugment`` (module docstring); the defaults are neutral.
    Needs no device."""
    elastic: Tuple[float, float, float] = (0.0, 0.0, 32.0)    # (probability, sigma of the node displacements in pixels, node pitch in pixels)
    noise: Tuple[float, float] = (0.0, 0.0)                   # (lo, hi): the per-sample sigma is uniform in this range
    cutmix: Tuple[float, float, float] = (0.0, 0.1, 0.5)      # (probability, smallest, largest side as a fraction of h and w)

    def __post_init__(self):
        p, sigma, pitch = _finite(self.elastic, "elastic = (probability, sigma, pitch)", 3)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"CubeDeform: the elastic probability must lie in [0, 1], got {p!r}")
        if sigma < 0 or pitch < 4:
            raise ValueError(f"CubeDeform: elastic needs sigma >= 0 and pitch >= 4, got {self.elastic!r}")
        lo, hi = _finite(self.noise, "noise = (lo, hi)", 2)
        if lo < 0 or lo > hi:
            raise ValueError(f"CubeDeform: noise must be a range 0 <= lo <= hi, got {self.noise!r}")
        cp, fmin, fmax = _finite(self.cutmix, "cutmix = (probability, min_frac, max_frac)", 3)
        if not 0.0 <= cp <= 1.0:
            raise ValueError(f"CubeDeform: the cutmix probability must lie in [0, 1], got {cp!r}")
        if not 0.0 < fmin <= fmax <= 1.0:
            raise ValueError(f"CubeDeform: cutmix needs 0 < min_frac <= max_frac <= 1, got {self.cutmix!r}")
        object.__setattr__(self, "elastic", (p, sigma, pitch))
        object.__setattr__(self, "noise", (lo, hi))
        object.__setattr__(self, "cutmix", (cp, fmin, fmax))


def elastic_lattice(h: int, w: int, pitch: float) -> Tuple[int, int]:
    """``(gy, gx)``: rows and columns of the node lattice an h x w window needs at ``pitch`` pixels between nodes -- the cell of the
    last pixel, ``floor((h - 1) / pitch)``, plus the four nodes the cubic B-spline reads from there."""
    if h <= 0 or w <= 0 or not pitch >= 4:
        raise ValueError("elastic_lattice: h, w must be positive and pitch at least 4")
    return int(math.floor((h - 1) / pitch)) + 4, int(math.floor((w - 1) / pitch)) + 4


def deform_entries(mix_from, ry0, ry1, rx0, rx1, nodes_off, gy, gx, inv_pitch, sigma, k0, k1) -> torch.Tensor:
    """The (n, 16) int32 deform entry array of the deforming kernels (module docstring) from per-sample sequences; ``inv_pitch`` and
    ``sigma`` are rounded once to fp32, the keys ``k0``, ``k1`` in [0, 2^32) stored by their bits."""
    n = len(mix_from)
    e = np.zeros((n, 16), dtype=np.int32)
    for col, v in enumerate((mix_from, ry0, ry1, rx0, rx1, nodes_off, gy, gx)):
        e[:, col] = np.asarray(v, dtype=np.int64)
    e[:, 8] = np.asarray(inv_pitch, dtype=np.float64).astype(np.float32).view(np.int32)
    e[:, 9] = np.asarray(sigma, dtype=np.float64).astype(np.float32).view(np.int32)
    e[:, 10] = np.asarray(k0, dtype=np.int64).astype(np.uint32).view(np.int32)
    e[:, 11] = np.asarray(k1, dtype=np.int64).astype(np.uint32).view(np.int32)
    return torch.from_numpy(e)


class DeformedPlan(NamedTuple):
    order: torch.Tensor                 # as AugmentedPlan
    table: torch.Tensor
    entries: torch.Tensor
    batches: List[Tuple[int, int]]
    window: Tuple[int, int]
    warped: List[bool]
    deform: torch.Tensor                # (m, 16) int32: the deform entries (mix_from is an index INSIDE the sample's batch)
    nodes: Optional[torch.Tensor]       # flat fp32 node table (nodes_off counts from its start), or None
    deformed: List[bool]                # per batch: some sample needs the deforming kernels


def plan_epoch_deformed(n: int, batch_size: int, frame: Tuple[int, int], channels: int, augment: Optional[CubeAugment] = None,
                        deform: Optional[CubeDeform] = None, patch=None, shuffle: bool = True, random_crop: bool = False,
                        flips: bool = False, drop_last: bool = False, generator: Optional[torch.Generator] = None) -> DeformedPlan:
    """``plan_epoch_augmented`` plus the deformation draws of the module docstring (a pure host function).  Order, table, entries
    and ``warped`` are ``plan_epoch_augmented``'s for the same generator state."""
    dfm = CubeDeform() if deform is None else deform
    plan = plan_epoch_augmented(n, batch_size, frame, channels, augment, patch, shuffle, random_crop, flips, drop_last, generator)
    h, w = plan.window
    r = [torch.rand(n, dtype=torch.float64, generator=generator).numpy() for _ in range(7)]
    keys = torch.randint(0, 2 ** 32, (n, 2), dtype=torch.int64, generator=generator).numpy()
    ep, esigma, pitch = dfm.elastic
    m = plan.table.shape[0]
    nodes, gy, gx = None, 0, 0
    if ep > 0 and esigma > 0:
        gy, gx = elastic_lattice(h, w, pitch)
        nodes = (torch.randn(n, gy, gx, 2, dtype=torch.float64, generator=generator) * esigma).to(torch.float32)[:m].reshape(-1).contiguous()
    elastic = (r[0] < ep) & (nodes is not None)
    sigma = dfm.noise[0] + r[1] * (dfm.noise[1] - dfm.noise[0])
    cp, fmin, fmax = dfm.cutmix
    cut = r[2] < cp
    rh = np.clip(np.round((fmin + r[3] * (fmax - fmin)) * h), 1, h).astype(np.int64)
    rw = np.clip(np.round((fmin + r[4] * (fmax - fmin)) * w), 1, w).astype(np.int64)
    ry0 = np.minimum(np.floor(r[5] * (h - rh + 1)).astype(np.int64), h - rh)
    rx0 = np.minimum(np.floor(r[6] * (w - rw + 1)).astype(np.int64), w - rw)
    mix_from = np.full(n, -1, dtype=np.int64)
    for s, e in plan.batches:
        if e - s > 1:
            j = np.arange(e - s)
            mix_from[s:e] = np.where(cut[s:e], (j - 1) % (e - s), -1)
    on = mix_from >= 0
    off = np.where(elastic, np.arange(n, dtype=np.int64) * (2 * gy * gx), -1)
    d = deform_entries(mix_from[:m], np.where(on, ry0, 0)[:m], np.where(on, ry0 + rh, 0)[:m], np.where(on, rx0, 0)[:m],
                       np.where(on, rx0 + rw, 0)[:m], off[:m], np.where(elastic, gy, 0)[:m], np.where(elastic, gx, 0)[:m],
                       np.where(elastic, 1.0 / pitch, 0.0)[:m], sigma[:m], keys[:m, 0], keys[:m, 1])
    needs = elastic | (sigma > 0) | on
    deformed = [bool(needs[s:e].any()) for s, e in plan.batches]
    return DeformedPlan(plan.order, plan.table, plan.entries, plan.batches, plan.window, plan.warped, d, nodes, deformed)


class BatchPlan(NamedTuple):
    path: str                           # "gather", "warp" or "deform": the kernels that serve the batch
    window: Tuple[int, int]             # (h, w)
    table: Optional[torch.Tensor]       # gather: (n, 4) int32 {slot, top, left, flags}
    entries: Optional[torch.Tensor]     # warp, deform: (n, 16) int32 warp entries
    deform: Optional[torch.Tensor]      # deform: (n, 16) int32 deform entries (nodes_off = j * 2 gy gx with a lattice, else -1)
    nodes: Optional[torch.Tensor]       # deform with ``elastic``: the flat fp32 node table


def plan_batch(indices: Sequence[int], frame: Tuple[int, int], channels: int, top=None, left=None, flip_h=None, flip_w=None, patch=None,
               angle=None, zoom=None, shift=None, gain=None, offset=None, band_drop=None, elastic=None, noise=None, cutmix=None,
               force_warp: bool = False, force_deform: bool = False) -> BatchPlan:
    """The host half of ``CubeCache.batch`` (whose arguments these are; ``frame`` = (H, W) and ``channels`` = C of the cache; a pure
    host function): one value per sample of everything, validated; which kernels serve the batch -- the deforming ones with a
    lattice, a sigma above 0 or a CutMix partner inside the batch, else the warp pair when any sample is not neutral, else the
    plain gather --; and the host tensors that path uploads."""
    idx = [int(i) for i in indices]
    n = len(idx)
    if n == 0:
        raise ValueError("CubeCache.batch: no indices")
    H, W = frame
    h, w = _hw(patch, H, W)

    def per_sample(v, default):
        if v is None:
            return [default] * n
        v = [int(e) for e in (v.tolist() if hasattr(v, "tolist") else v)] if hasattr(v, "__len__") else [int(v)] * n
        if len(v) != n:
            raise ValueError("CubeCache.batch: one value per sample")
        return v
    tops, lefts = per_sample(top, (H - h) // 2), per_sample(left, (W - w) // 2)
    fhs, fws = per_sample(flip_h, 0), per_sample(flip_w, 0)
    for t_, l_ in zip(tops, lefts):
        if not (0 <= t_ <= H - h and 0 <= l_ <= W - w):
            raise ValueError(f"CubeCache.batch: window {h}x{w} at ({t_}, {l_}) leaves the {H}x{W} frame")

    def per_sample_f(v, default, width=1):
        if v is None:
            return [default] * n
        a = np.asarray(v.tolist() if hasattr(v, "tolist") else v, dtype=np.float64)
        if a.ndim == (width > 1):
            a = np.broadcast_to(a, (n,) + a.shape)
        if a.shape != ((n,) if width == 1 else (n, width)) or not np.isfinite(a).all():
            raise ValueError("CubeCache.batch: one finite value per sample" if width == 1 else
                             f"CubeCache.batch: one finite {width}-tuple per sample")
        return a.tolist()
    angles, zooms, shifts = per_sample_f(angle, 0.0), per_sample_f(zoom, 1.0), per_sample_f(shift, [0.0, 0.0], 2)
    gains, offsets, drops = per_sample_f(gain, 1.0), per_sample_f(offset, 0.0), per_sample_f(band_drop, [0.0, 0.0], 2)
    if any(not 1 / 16 <= z <= 16 for z in zooms):
        raise ValueError("CubeCache.batch: zoom must lie in [1/16, 16]")
    for lo_, n_ in drops:
        if lo_ != int(lo_) or n_ != int(n_) or lo_ < 0 or n_ < 0 or lo_ + n_ > channels:
            raise ValueError(f"CubeCache.batch: band_drop {(lo_, n_)} leaves the {channels} bands")
    neutral = all(a == 0 and z == 1 and s_ == [0.0, 0.0] and g_ == 1 and o_ == 0 and d_[1] == 0
                  for a, z, s_, g_, o_, d_ in zip(angles, zooms, shifts, gains, offsets, drops))
    nz = per_sample_f(noise, [0.0, 0.0, 0.0], 3)
    cm = per_sample_f(cutmix, [-1.0, 0.0, 0.0, 0.0, 0.0], 5)
    if any(k_ != int(k_) or not 0 <= k_ < 2 ** 32 for z_ in nz for k_ in z_[1:]):
        raise ValueError("CubeCache.batch: noise keys must be whole numbers in [0, 2^32)")
    if any(v_ != int(v_) or abs(v_) >= 2 ** 31 for c_ in cm for v_ in c_):
        raise ValueError("CubeCache.batch: cutmix takes whole numbers (from, ry0, ry1, rx0, rx1)")
    mixes = [0 <= c_[0] < n and c_[0] != j and max(c_[1], 0) < min(c_[2], h) and max(c_[3], 0) < min(c_[4], w) for j, c_ in enumerate(cm)]
    deformed = force_deform or elastic is not None or any(z_[0] > 0 for z_ in nz) or any(mixes)
    if not (deformed or force_warp or not neutral):
        rows = [[i, t_, l_, (1 if a else 0) | (2 if b else 0)] for i, t_, l_, a, b in zip(idx, tops, lefts, fhs, fws)]
        return BatchPlan("gather", (h, w), torch.tensor(rows, dtype=torch.int32), None, None, None)
    entries = warp_entries(idx, tops, lefts, fhs, fws, (h, w), angles, zooms, [s_[0] for s_ in shifts], [s_[1] for s_ in shifts],
                           gains, offsets, [int(d_[0]) for d_ in drops], [int(d_[1]) for d_ in drops])
    if not deformed:
        return BatchPlan("warp", (h, w), None, entries, None, None)
    nodes, gy, gx, inv_pitch = None, 0, 0, 0.0
    if elastic is not None:
        nd, pitch = elastic
        nodes = torch.as_tensor(np.asarray(nd.tolist() if hasattr(nd, "tolist") else nd, dtype=np.float64), dtype=torch.float32)
        if nodes.dim() != 4 or nodes.shape[0] != n or nodes.shape[3] != 2 or not bool(torch.isfinite(nodes).all()) or not float(pitch) >= 4:
            raise ValueError("CubeCache.batch: elastic takes ((n, gy, gx, 2) finite node displacements, pitch >= 4)")
        if tuple(nodes.shape[1:3]) != elastic_lattice(h, w, float(pitch)):
            raise ValueError(f"CubeCache.batch: a {h}x{w} window at pitch {pitch} needs a lattice of {elastic_lattice(h, w, float(pitch))}, "
                             f"got {tuple(nodes.shape[1:3])}")
        gy, gx, inv_pitch = int(nodes.shape[1]), int(nodes.shape[2]), 1.0 / float(pitch)
        nodes = nodes.reshape(-1).contiguous()
    cell = 2 * gy * gx
    deform = deform_entries([int(c_[0]) for c_ in cm], [int(c_[1]) for c_ in cm], [int(c_[2]) for c_ in cm], [int(c_[3]) for c_ in cm],
                            [int(c_[4]) for c_ in cm], [j * cell if nodes is not None else -1 for j in range(n)], [gy] * n, [gx] * n,
                            [inv_pitch] * n, [z_[0] for z_ in nz], [int(z_[1]) for z_ in nz], [int(z_[2]) for z_ in nz])
    return BatchPlan("deform", (h, w), None, entries, deform, nodes)


class CubeCache:
    def __init__(self, capacity: int, height: int, width: int, bands: int, hsi_lo: int = 0, hsi_hi: Optional[int] = None,
                 device="cuda:0", store_dtype=torch.float32, unsqueeze_hsi: bool = True, out_slots: int = 2):
        hsi_hi = bands if hsi_hi is None else hsi_hi
        if not (0 <= hsi_lo < hsi_hi <= bands):
            raise ValueError(f"CubeCache: bad band range [{hsi_lo}:{hsi_hi}] of {bands}")
        if capacity <= 0 or height <= 0 or width <= 0 or out_slots <= 0:
            raise ValueError("CubeCache: capacity, height, width and out_slots must be positive")
        if store_dtype not in _DT:
            raise ValueError("CubeCache: store_dtype must be torch.float32 or torch.float16")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("hyperpri_amd: CubeCache needs a ROCm device; there is no CPU fallback")
        self.capacity, self.H, self.W, self.B = capacity, height, width, bands
        self.lo, self.C = hsi_lo, hsi_hi - hsi_lo
        self.cs = _rup(self.C, 8)
        self.store_dtype, self.unsqueeze, self.out_slots = store_dtype, unsqueeze_hsi, out_slots
        # said before it is taken: a split that does not fit should fail here, with the figure, not inside the allocator
        self.cache_bytes = self.planned_bytes(capacity, height, width, self.C, store_dtype)
        free, total = torch.cuda.mem_get_info(self.device)
        _log.info("CubeCache: allocating %.2f GB on %s (%d slots of %dx%dx%d %s + uint8 masks; %.1f of %.1f GB free)",
                  self.cache_bytes / 1e9, self.device, capacity, height, width, self.cs,
                  "fp16" if store_dtype == torch.float16 else "fp32", free / 1e9, total / 1e9)
        if self.cache_bytes > free:
            raise RuntimeError(f"hyperpri_amd: CubeCache needs {self.cache_bytes / 1e9:.2f} GB on {self.device}, "
                               f"{free / 1e9:.2f} GB are free")
        # (the store pass writes every channel of a slot, pad zeros included: no fill here)
        self._cubes = torch.empty((capacity, height, width, self.cs), dtype=store_dtype, device=self.device)
        self._masks = torch.zeros((capacity, height, width), dtype=torch.uint8, device=self.device)
        self._names: List[object] = [None] * capacity
        self._filled = [False] * capacity
        self._pinned = {}               # source dtype -> pinned (H, W, B) staging tensor
        self._raw = {}                  # source dtype -> device (H, W, B) staging tensor
        self._staged: Optional[torch.cuda.Event] = None
        self._out: List[torch.Tensor] = []
        self._mout: List[torch.Tensor] = []
        self._fout: List[Optional[torch.Tensor]] = []        # the elastic field of every output slot: (N, h, w, 2), allocated on first use
        self._out_shape = (0, 0, 0)     # (N allocated, h, w)
        self._out_stream: List[Optional[torch.cuda.Stream]] = []
        self._consumed: List[Optional[torch.cuda.Event]] = []
        self._next = 0

    @staticmethod
    def planned_bytes(capacity: int, height: int, width: int, channels: int, store_dtype=torch.float32) -> int:
        """Device bytes a cache of this geometry holds for its lifetime (cubes + masks; the ``out_slots`` output buffers are
        sized by the first batch and reported then)."""
        esz = 2 if store_dtype == torch.float16 else 4
        return capacity * height * width * (_rup(channels, 8) * esz + 1)

    def __len__(self) -> int:
        return sum(self._filled)

    # ---- loading -----------------------------------------------------------------------------------------------------
    def put(self, i: int, cube_hwb, mask, name=None) -> None:
        """Store one (H, W, B) fp32 / fp16 cube (numpy array or torch tensor, host or device) and its (H, W) or (1, H, W)
        mask in slot ``i``.  Host sources go through a pinned buffer; the band slice / convert / pad pass runs on the
        current stream."""
        if not 0 <= i < self.capacity:
            raise IndexError(f"CubeCache.put: slot {i} of {self.capacity}")
        t = torch.from_numpy(cube_hwb) if isinstance(cube_hwb, np.ndarray) else cube_hwb
        if t.dtype not in _DT or tuple(t.shape) != (self.H, self.W, self.B):
            raise ValueError(f"CubeCache.put: need a ({self.H}, {self.W}, {self.B}) float32 / float16 cube, got "
                             f"{tuple(t.shape)} {t.dtype}")
        m = torch.from_numpy(np.ascontiguousarray(mask)) if isinstance(mask, np.ndarray) else mask
        if m.numel() != self.H * self.W:
            raise ValueError(f"CubeCache.put: need a ({self.H}, {self.W}) mask, got {tuple(m.shape)}")
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if t.is_cuda:
                if t.device != self.device:
                    raise ValueError(f"CubeCache.put: the cube is on {t.device}, the cache on {self.device}")
                src = t.contiguous()
            else:
                pin = self._pinned.get(t.dtype)
                if pin is None:
                    pin = self._pinned[t.dtype] = torch.empty((self.H, self.W, self.B), dtype=t.dtype).pin_memory()
                    self._raw[t.dtype] = torch.empty((self.H, self.W, self.B), dtype=t.dtype, device=self.device)
                if self._staged is not None:
                    self._staged.synchronize()          # the previous cube's copy has finished reading the pinned buffer
                pin.copy_(t)
                src = self._raw[t.dtype]
                src.copy_(pin, non_blocking=True)
                self._staged = torch.cuda.Event()
                self._staged.record(cur)
            _lib.call("hpri_hwb_store", _p(src), _DT[src.dtype], _p(self._cubes[i]), _DT[self.store_dtype], self.H * self.W,
                      self.B, self.lo, self.C, self.cs, ctypes.c_void_p(cur.cuda_stream))
            self._masks[i].copy_(m.reshape(self.H, self.W).to(torch.uint8), non_blocking=True)
        self._names[i] = i if name is None else name
        self._filled[i] = True

    def fill(self, items: Iterable) -> int:
        """``put`` every ``(cube, mask, name)`` of an iterable into slots 0, 1, ...; frees the staging buffers; returns the count."""
        k = 0
        for k, (cube, mask, name) in enumerate(items, 1):
            self.put(k - 1, cube, mask, name)
        self.release_staging()
        return k

    def release_staging(self) -> None:
        """Drop the pinned and device staging buffers ``put`` keeps for host sources (a raw 299-band cube is 0.7 GB)."""
        if self._staged is not None:
            self._staged.synchronize()
            self._staged = None
        self._pinned.clear()
        self._raw.clear()

    # ---- serving -----------------------------------------------------------------------------------------------------
    def _take_slot(self, n: int, h: int, w: int, cur) -> int:
        N0, h0, w0 = self._out_shape
        if (h, w) != (h0, w0) or n > N0:
            nbytes = self.out_slots * n * h * w * (self.cs + 1) * 4
            _log.info("CubeCache: allocating %.2f GB of output buffers (%d x %dx%dx%dx%d fp32 + masks)", nbytes / 1e9,
                      self.out_slots, n, h, w, self.cs)
            # pad channels are rewritten (as zeros, from the slots) by every gather: no fill here either
            self._out = [torch.empty((n, h, w, self.cs), dtype=torch.float32, device=self.device) for _ in range(self.out_slots)]
            self._mout = [torch.empty((n, 1, h, w), dtype=torch.float32, device=self.device) for _ in range(self.out_slots)]
            self._fout = [None] * self.out_slots
            self._out_shape = (n, h, w)
            self._out_stream = [None] * self.out_slots
            self._consumed = [None] * self.out_slots
            self._next = 0
        k = self._next
        self._next = (k + 1) % self.out_slots
        done, last = self._consumed[k], self._out_stream[k]
        if done is None and last is not None and last != cur:
            done = torch.cuda.Event()                    # release() was not called: wait for everything enqueued there so far
            done.record(last)
        if done is not None:
            cur.wait_event(done)                         # work that read this buffer's previous contents has finished
        self._consumed[k] = None
        self._out_stream[k] = cur
        return k

    def _launch(self, slots: Sequence[int], window: Tuple[int, int], table: int = 0, entries: int = 0, deform: int = 0,
                nodes: Optional[torch.Tensor] = None, lattice: bool = False, transposed: bool = False) -> dict:
        """Fill the next output slot with the ``window`` = (h, w) of the cubes ``slots`` on the current stream and hand it out.  The
        arguments are device addresses of ``len(slots)`` rows: with ``deform`` (64-byte deform entries beside the warp entries at
        ``entries``; ``nodes`` is the device node table their ``nodes_off`` count into) the deforming kernels run, else with
        ``entries`` the warp kernel pair, else the plain gather with the 16-byte rows at ``table``.  With ``lattice`` (some sample of
        the batch has one) the field of the output slot is built first; otherwise that launch is skipped and the deforming kernels
        get a null field.  ``transposed``: the window is (W, H) of whole frames.  It has as many pixels as the frame, so it is
        written into the (H, W) output buffers themselves, read as (n, W, H, cs): ``_take_slot`` sees the frame's shape, and
        alternating between the two orientations allocates nothing."""
        n = len(slots)
        h, w = window
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            k = self._take_slot(n, *((w, h) if transposed else (h, w)), cur)
            s = ctypes.c_void_p(cur.cuda_stream)
            tp, ep, dp = ctypes.c_void_p(table), ctypes.c_void_p(entries), ctypes.c_void_p(deform)
            cube = (_p(self._cubes), _DT[self.store_dtype], self.capacity, self.H, self.W, self.cs)
            mask = (_p(self._masks), self.capacity, self.H, self.W)
            out = (n, h, w, _p(self._out[k]), s)
            mout = (n, h, w, _p(self._mout[k]), s)
            if deform:
                fp = ctypes.c_void_p(0)
                if lattice:
                    if self._fout[k] is None:
                        self._fout[k] = torch.empty((self._out_shape[0], h, w, 2), dtype=torch.float32, device=self.device)
                    fp = _p(self._fout[k])
                    _lib.call("hpri_elastic_field", _p(nodes) if nodes is not None else ctypes.c_void_p(0),
                              nodes.numel() if nodes is not None else 0, dp, n, h, w, fp, s)
                _lib.call("hpri_cube_deform", *cube, self.C, ep, dp, fp, *out)
                _lib.call("hpri_mask_deform", *mask, ep, dp, fp, *mout)
            elif entries:
                _lib.call("hpri_cube_warp", *cube, self.C, ep, *out)
                _lib.call("hpri_mask_warp", *mask, ep, *mout)
            else:
                _lib.call("hpri_cube_gather", *cube, tp, *out)
                _lib.call("hpri_mask_gather", *mask, tp, *mout)
        return self._hand_out(k, slots, window)

    def _hand_out(self, k: int, slots: Sequence[int], window: Tuple[int, int]) -> dict:
        n = len(slots)
        h, w = window
        x = self._out[k][:n].view(n, h, w, self.cs)[:, :, :, :self.C].permute(0, 3, 1, 2)       # logical (N,C,h,w), channels-last strides
        if self.unsqueeze:
            x = x.unsqueeze(1)                                          # (N,1,C,h,w) as dataset.py:269-270
        x._hpri_zero_padded = True
        x._hpri_slot = k
        return {'image': x, 'mask': self._mout[k][:n].view(n, 1, h, w), 'index': [self._names[i] for i in slots]}

    def _check_filled(self, slots: Sequence[int]) -> None:
        for i in slots:
            if not (0 <= i < self.capacity and self._filled[i]):
                raise IndexError(f"CubeCache: slot {i} is empty or out of range")

    def batch(self, indices: Sequence[int], top=None, left=None, flip_h=None, flip_w=None, patch=None, angle=None, zoom=None,
              shift=None, gain=None, offset=None, band_drop=None, _force_warp: bool = False, elastic=None, noise=None, cutmix=None,
              _force_deform: bool = False) -> dict:
        """``{'image', 'mask', 'index'}`` for the cached cubes ``indices``: a window of ``patch`` (the whole frame by
        default) at ``top`` / ``left`` (per sample or one value; default: centred), flipped along rows (``flip_h``) and
        columns (``flip_w``).  Uploads a table of 16 bytes per sample; ``epoch()`` is the path without any copy.

        Augmentation, each per sample or one value for all (module docstring): ``angle`` in degrees, ``zoom`` (above 1
        magnifies), ``shift`` = ``(dx, dy)`` pixels added to the window centre, ``gain``, ``offset``, ``band_drop`` =
        ``(first, count)`` bands written as zeros.  A batch in which every sample is neutral takes the plain gather (the
        same bits as without these arguments); any other one the warp kernels, with 64 bytes per sample uploaded.

        Deformation (module docstring): ``elastic`` = ``(nodes, pitch)`` with ``nodes`` an (n, gy, gx, 2) array of (dx, dy) node
        displacements in output pixels (``elastic_lattice`` gives gy, gx) -- one lattice per sample --, ``noise`` = ``(sigma, k0, k1)``
        and ``cutmix`` = ``(from, ry0, ry1, rx0, rx1)``, each per sample or one tuple for all; ``from`` is an index into ``indices``
        (-1: none), and the kernels clamp the rectangle into the window.  With neutral values (no lattice, no sigma above 0, no
        ``from`` inside the batch) the path and the bits are those without these arguments; otherwise the deforming kernels run,
        with 128 bytes per sample and the lattices uploaded."""
        idx = [int(i) for i in indices]
        self._check_filled(idx)
        plan = plan_batch(idx, (self.H, self.W), self.C, top, left, flip_h, flip_w, patch, angle, zoom, shift, gain, offset, band_drop,
                          elastic, noise, cutmix, force_warp=_force_warp, force_deform=_force_deform)
        nodes = plan.nodes.to(self.device) if plan.nodes is not None else None
        if plan.path == "deform":
            rows = torch.cat([plan.entries, plan.deform]).to(self.device)
            out = self._launch(idx, plan.window, entries=rows.data_ptr(), deform=rows.data_ptr() + 64 * len(idx), nodes=nodes,
                               lattice=nodes is not None)
        elif plan.path == "warp":
            rows = plan.entries.to(self.device)
            out = self._launch(idx, plan.window, entries=rows.data_ptr())
        else:
            rows = plan.table.to(self.device)
            out = self._launch(idx, plan.window, table=rows.data_ptr())
        rows.record_stream(torch.cuda.current_stream(self.device))
        if nodes is not None:
            nodes.record_stream(torch.cuda.current_stream(self.device))
        return out

    def epoch(self, batch_size: int, shuffle: bool = True, generator: Optional[torch.Generator] = None, patch=None,
              random_crop: bool = False, flips: bool = False, drop_last: bool = False,
              augment: Optional[CubeAugment] = None, deform: Optional[CubeDeform] = None) -> Iterator[dict]:
        """Iterate one epoch (``plan_epoch`` over the filled slots, which must be slots 0 .. len-1).  The plan is drawn and
        its table uploaded before the first batch; ``plan`` of the most recent call is kept as ``last_plan``.  With
        ``augment`` the plan is ``plan_epoch_augmented``'s (an ``AugmentedPlan``): its entries are uploaded beside the table,
        and every batch it flags goes through the warp kernels, the others through the plain gather.  With ``deform`` the plan
        is ``plan_epoch_deformed``'s (a ``DeformedPlan``; ``augment`` may be None): its deform entries and node table are uploaded
        once as well, a batch it flags as ``deformed`` goes through the deforming kernels -- the field launch skipped, and a null
        field passed, when no sample of the batch has a lattice --, the others as before."""
        n = len(self)
        if n == 0 or not all(self._filled[:n]):
            raise RuntimeError("CubeCache.epoch: fill slots 0 .. len-1 first")
        if deform is not None:
            plan = plan_epoch_deformed(n, batch_size, (self.H, self.W), self.C, augment, deform, patch, shuffle, random_crop, flips,
                                       drop_last, generator)
        elif augment is None:
            plan = plan_epoch(n, batch_size, (self.H, self.W), patch, shuffle, random_crop, flips, drop_last, generator)
        else:
            plan = plan_epoch_augmented(n, batch_size, (self.H, self.W), self.C, augment, patch, shuffle, random_crop, flips,
                                        drop_last, generator)
        self.last_plan = plan
        return self._serve(plan)

    def _serve(self, plan) -> Iterator[dict]:
        if not plan.batches:
            return
        with torch.cuda.device(self.device):
            table = plan.table.pin_memory().to(self.device, non_blocking=True)     # once per epoch, asynchronous
            warped = getattr(plan, "warped", None)
            deformed = getattr(plan, "deformed", None)
            entries = plan.entries.pin_memory().to(self.device, non_blocking=True) if warped and (any(warped) or any(deformed or ())) else None
            dtable = nodes = lattice = None
            if deformed and any(deformed):
                dtable = plan.deform.pin_memory().to(self.device, non_blocking=True)
                nodes = plan.nodes.pin_memory().to(self.device, non_blocking=True) if plan.nodes is not None else None
                lattice = (plan.deform[:, 5] >= 0).tolist()
        self._deform_tables = (dtable, nodes)
        self._table = table             # (alive until the next epoch's table replaces it, also when this iterator is dropped early)
        self._entries = entries
        order = plan.order.tolist()
        base = table.data_ptr()
        for b, (start, stop) in enumerate(plan.batches):
            slots = order[start:stop]
            if dtable is not None and deformed[b]:
                yield self._launch(slots, plan.window, entries=entries.data_ptr() + 64 * start, deform=dtable.data_ptr() + 64 * start,
                                   nodes=nodes, lattice=any(lattice[start:stop]))
            elif entries is not None and warped[b]:
                yield self._launch(slots, plan.window, entries=entries.data_ptr() + 64 * start)
            else:
                yield self._launch(slots, plan.window, table=base + 16 * start)

    # ---- views for test-time augmentation (hyperpri_amd/tta.py) -----------------------------------------------------
    def view(self, indices: Sequence[int], view: str) -> dict:
        """``{'image', 'mask', 'index'}`` of the WHOLE frame of the cached cubes ``indices`` in one of the eight dihedral views of
        ``hyperpri_amd.tta`` -- image and mask alike, bit for bit ``apply_view`` of ``batch(indices)``.  ``id``, ``flip_h``,
        ``flip_w`` and ``rot180`` are the plain gather with the table's flip flags; ``rot90``, ``rot270``, ``transpose`` and
        ``antitranspose`` come out as (W, H) frames from the warp kernels with the entries of ``view_warp_entries`` (exact
        0 / +-1, every source coordinate an integer in fp32: see there).  Uploads 16 or 64 bytes per sample; the output slots
        rotate, and the streams are ordered, as for ``batch()``."""
        from .tta import view_code
        code = view_code(view)
        idx = [int(i) for i in indices]
        if not idx:
            raise ValueError("CubeCache.view: no indices")
        self._check_filled(idx)
        if code >= 4:
            rows = view_warp_entries(idx, view, (self.H, self.W)).to(self.device)
            out = self._launch(idx, (self.W, self.H), entries=rows.data_ptr(), transposed=True)
        else:
            flags = {"id": 0, "flip_h": 1, "flip_w": 2, "rot180": 3}[view]
            rows = torch.tensor([[i, 0, 0, flags] for i in idx], dtype=torch.int32).to(self.device)
            out = self._launch(idx, (self.H, self.W), table=rows.data_ptr())
        rows.record_stream(torch.cuda.current_stream(self.device))
        return out

    def epoch_views(self, batch_size: int, views: Sequence[str]) -> Iterator[dict]:
        """One unshuffled pass over the filled slots (which must be slots 0 .. len-1) for test-time augmentation: yields
        ``{'mask', 'index', 'views', 'image_of'}`` -- ``mask`` and ``index`` of the identity orientation, ``views`` the names
        asked for, and ``image_of(name)``, which gathers that view of the batch's images when it is called.

        Every ``image_of`` call is a gather into the next output slot (the first ``image_of('id')`` of a batch hands out the
        gather that made ``mask``): a view tensor -- and ``mask`` -- is valid until ``out_slots`` further gathers.  The consumer
        must be done with one view (and have copied the mask) before it asks for the next; ``predict_split`` is."""
        from .tta import view_code
        names = [views] if isinstance(views, str) else list(views)
        for v in names:
            view_code(v)
        if batch_size <= 0:
            raise ValueError("CubeCache.epoch_views: batch_size must be positive")
        n = len(self)
        if n == 0 or not all(self._filled[:n]):
            raise RuntimeError("CubeCache.epoch_views: fill slots 0 .. len-1 first")
        return self._serve_views(n, batch_size, tuple(names))

    def _serve_views(self, n: int, batch_size: int, names: Tuple[str, ...]) -> Iterator[dict]:
        for start in range(0, n, batch_size):
            slots = list(range(start, min(start + batch_size, n)))
            first = self.view(slots, "id")
            fresh = [first['image']]

            def image_of(name: str, slots=slots, fresh=fresh) -> torch.Tensor:
                image = fresh.pop() if fresh and name == "id" else self.view(slots, name)['image']
                fresh.clear()
                return image
            yield {'mask': first['mask'], 'index': first['index'], 'views': names, 'image_of': image_of}

    def release(self, slot_tensor=None) -> None:
        """Mark an output buffer as consumed up to this point of the current stream.  Only needed when the next batch that
        reuses the buffer is requested on ANOTHER stream (module docstring); ``slot_tensor`` is a batch's ``image`` (or
        its slot index), by default the most recent batch."""
        if not self._out:
            return
        if slot_tensor is None:
            k = (self._next - 1) % self.out_slots
        elif isinstance(slot_tensor, int):
            k = slot_tensor
        else:
            k = getattr(slot_tensor, "_hpri_slot", None)
            if k is None:
                raise ValueError("CubeCache.release: not an image returned by batch() / epoch()")
        if not 0 <= k < self.out_slots:
            raise ValueError(f"CubeCache.release: slot {k} out of range")
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._consumed[k] = ev
