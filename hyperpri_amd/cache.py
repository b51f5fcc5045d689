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
"""
from __future__ import annotations

import ctypes
import logging
from typing import Iterable, Iterator, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .engine import _p, _rup

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

    def _gather(self, table_ptr: int, slots: Sequence[int], h: int, w: int) -> dict:
        n = len(slots)
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            k = self._take_slot(n, h, w, cur)
            s = ctypes.c_void_p(cur.cuda_stream)
            tp = ctypes.c_void_p(table_ptr)
            _lib.call("hpri_cube_gather", _p(self._cubes), _DT[self.store_dtype], self.capacity, self.H, self.W, self.cs, tp, n,
                      h, w, _p(self._out[k]), s)
            _lib.call("hpri_mask_gather", _p(self._masks), self.capacity, self.H, self.W, tp, n, h, w, _p(self._mout[k]), s)
        x = self._out[k][:n, :, :, :self.C].permute(0, 3, 1, 2)        # logical (N,C,h,w), channels-last strides
        if self.unsqueeze:
            x = x.unsqueeze(1)                                          # (N,1,C,h,w) as dataset.py:269-270
        x._hpri_zero_padded = True
        x._hpri_slot = k
        return {'image': x, 'mask': self._mout[k][:n], 'index': [self._names[i] for i in slots]}

    def _check_filled(self, slots: Sequence[int]) -> None:
        for i in slots:
            if not (0 <= i < self.capacity and self._filled[i]):
                raise IndexError(f"CubeCache: slot {i} is empty or out of range")

    def batch(self, indices: Sequence[int], top=None, left=None, flip_h=None, flip_w=None, patch=None) -> dict:
        """``{'image', 'mask', 'index'}`` for the cached cubes ``indices``: a window of ``patch`` (the whole frame by
        default) at ``top`` / ``left`` (per sample or one value; default: centred), flipped along rows (``flip_h``) and
        columns (``flip_w``).  Uploads a table of 16 bytes per sample; ``epoch()`` is the path without any copy."""
        idx = [int(i) for i in indices]
        n = len(idx)
        if n == 0:
            raise ValueError("CubeCache.batch: no indices")
        self._check_filled(idx)
        h, w = _hw(patch, self.H, self.W)

        def per_sample(v, default):
            if v is None:
                return [default] * n
            v = [int(e) for e in (v.tolist() if hasattr(v, "tolist") else v)] if hasattr(v, "__len__") else [int(v)] * n
            if len(v) != n:
                raise ValueError("CubeCache.batch: one value per sample")
            return v
        tops, lefts = per_sample(top, (self.H - h) // 2), per_sample(left, (self.W - w) // 2)
        fhs, fws = per_sample(flip_h, 0), per_sample(flip_w, 0)
        for t_, l_ in zip(tops, lefts):
            if not (0 <= t_ <= self.H - h and 0 <= l_ <= self.W - w):
                raise ValueError(f"CubeCache.batch: window {h}x{w} at ({t_}, {l_}) leaves the {self.H}x{self.W} frame")
        rows = [[i, t_, l_, (1 if a else 0) | (2 if b else 0)] for i, t_, l_, a, b in zip(idx, tops, lefts, fhs, fws)]
        table = torch.tensor(rows, dtype=torch.int32).to(self.device)
        out = self._gather(table.data_ptr(), idx, h, w)
        table.record_stream(torch.cuda.current_stream(self.device))
        return out

    def epoch(self, batch_size: int, shuffle: bool = True, generator: Optional[torch.Generator] = None, patch=None,
              random_crop: bool = False, flips: bool = False, drop_last: bool = False) -> Iterator[dict]:
        """Iterate one epoch (``plan_epoch`` over the filled slots, which must be slots 0 .. len-1).  The plan is drawn and
        its table uploaded before the first batch; ``plan`` of the most recent call is kept as ``last_plan``."""
        n = len(self)
        if n == 0 or not all(self._filled[:n]):
            raise RuntimeError("CubeCache.epoch: fill slots 0 .. len-1 first")
        plan = plan_epoch(n, batch_size, (self.H, self.W), patch, shuffle, random_crop, flips, drop_last, generator)
        self.last_plan = plan
        return self._serve(plan)

    def _serve(self, plan: EpochPlan) -> Iterator[dict]:
        if not plan.batches:
            return
        h, w = plan.window
        with torch.cuda.device(self.device):
            table = plan.table.pin_memory().to(self.device, non_blocking=True)     # once per epoch, asynchronous
        self._table = table             # (alive until the next epoch's table replaces it, also when this iterator is dropped early)
        order = plan.order.tolist()
        base = table.data_ptr()
        for start, stop in plan.batches:
            yield self._gather(base + 16 * start, order[start:stop], h, w)

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
