#!/usr/bin/env python3
"""Augmenting gather of the cube cache (csrc/cache_warp.hip): what the four-neighbour read costs beside the plain gather.

    python tools/cube_warp_bench.py                  # one MI355X; writes profiles/cube_warp.json
    python tools/cube_warp_bench.py --out FILE --rounds 15 --calls 20
    python tools/cube_warp_bench.py --only rot10_zoom1.1 --store fp32 --rounds 1 --calls 3 --out FILE     # one arm alone, e.g. under
                                                                                                         # rocprofv3 --pmc

The benched batch of tools/cube_cache_bench.py -- 2 x 238 of 299 bands x 608 x 968, the whole frame as the window -- from fp32 and
fp16 slots, four arms interleaved round by round in one process: the plain gather (``hpri_cube_gather``: unchanged code, the
yardstick), the identity forced through the warp kernel, a 10 degree rotation at zoom 1.1 and a 45 degree rotation at zoom 0.8
(about the frame's centre; gain 1, offset 0, no drop).  The method is cube_cache_bench's: device events around runs of ``--calls``
back-to-back launches after a warm-up, the median over ``--rounds`` with the spread.  Per arm: ms, TB/s of bytes WRITTEN (the
destination is the same 1.13 GB in every arm; what is read differs: one record per output for the identity, up to four, shared
through the caches, for a rotation, none for outputs outside the frame), the ratio to the plain gather and the share of the
cache-fed training steps DESIGN.md reports (31.3 ms fp32, 9.5 ms bf16).  The mask kernels are timed and listed separately.
Nothing is gated."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from cube_cache_bench import BANDS, BATCH, H, SRC_BANDS, W, _events_ms, _fill_cache  # noqa: E402

STEP_MS = {"fp32": 31.3, "bf16": 9.5}       # the cache-fed steps of DESIGN.md (profiles/cube_cache.json)
ARMS = [("plain_gather", None), ("identity_warp", (0.0, 1.0)), ("rot10_zoom1.1", (10.0, 1.1)), ("rot45_zoom0.8", (45.0, 0.8))]


def _outside(entries, h, w, Hs, Ws):
    """Share of the output pixels whose source point lies outside the frame (nothing is read for those beyond one pixel out)."""
    f = entries.numpy()[:, 4:12].copy().view(np.float32).astype(np.float64)
    u = (np.arange(w) - (w - 1) / 2)[None, :]
    v = (np.arange(h) - (h - 1) / 2)[:, None]
    out = []
    for r in f:
        sx, sy = r[0] * u + r[1] * v + r[2], r[3] * u + r[4] * v + r[5]
        out.append(float(((sx < 0) | (sx > Ws - 1) | (sy < 0) | (sy > Hs - 1)).mean()))
    return sum(out) / len(out)


def measure(dev, rounds, calls, stores, only):
    from hyperpri_amd import _lib
    from hyperpri_amd.cache import CubeCache, warp_entries
    from hyperpri_amd.engine import _p
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    for store in stores:
        sname = "fp32" if store == torch.float32 else "fp16"
        dt = 0 if store == torch.float32 else 1
        c = CubeCache(BATCH, H, W, SRC_BANDS, hsi_lo=0, hsi_hi=BANDS, device=dev, store_dtype=store, out_slots=1)
        _fill_cache(c, BATCH, dev, (H, W))
        cs = c.cs
        elems = BATCH * H * W * cs
        dst = torch.empty((BATCH, H, W, cs), dtype=torch.float32, device=dev)
        mdst = torch.empty((BATCH, 1, H, W), dtype=torch.float32, device=dev)
        table = torch.tensor([[i, 0, 0, 0] for i in range(BATCH)], dtype=torch.int32).to(dev)
        fns, mfns, outside, keep = {}, {}, {}, []
        for name, geo in ARMS:
            if only and name not in only:
                continue
            if geo is None:
                fns[name] = lambda: _lib.call("hpri_cube_gather", _p(c._cubes), dt, c.capacity, H, W, cs, _p(table), BATCH, H, W, _p(dst), stream)
                mfns[name] = lambda: _lib.call("hpri_mask_gather", _p(c._masks), c.capacity, H, W, _p(table), BATCH, H, W, _p(mdst), stream)
                outside[name] = 0.0
                continue
            host = warp_entries(list(range(BATCH)), [0] * BATCH, [0] * BATCH, [0] * BATCH, [0] * BATCH, (H, W), [geo[0]] * BATCH,
                                [geo[1]] * BATCH, [0.0] * BATCH, [0.0] * BATCH, [1.0] * BATCH, [0.0] * BATCH, [0] * BATCH, [0] * BATCH)
            e = host.to(dev)
            keep.append(e)
            outside[name] = _outside(host, H, W, H, W)
            fns[name] = lambda e=e: _lib.call("hpri_cube_warp", _p(c._cubes), dt, c.capacity, H, W, cs, c.C, _p(e), BATCH, H, W, _p(dst), stream)
            mfns[name] = lambda e=e: _lib.call("hpri_mask_warp", _p(c._masks), c.capacity, H, W, _p(e), BATCH, H, W, _p(mdst), stream)
        for fn in list(fns.values()) + list(mfns.values()):            # warm-up: code objects, clocks
            _events_ms(fn, calls)
        t = {name: [] for name in fns}
        for _ in range(rounds):                                         # interleaved: the same seconds of the same box
            for name, fn in fns.items():
                t[name].append(_events_ms(fn, calls))
        tm = {name: statistics.median(_events_ms(fn, calls) for _ in range(3)) for name, fn in mfns.items()}
        base = statistics.median(t["plain_gather"]) if "plain_gather" in t else None
        for name in fns:
            med = statistics.median(t[name])
            row = {"arm": name, "store": sname, "window": [H, W], "bytes_written": elems * 4,
                   "slot_bytes_per_record_read": cs * (4 if store == torch.float32 else 2),
                   "outputs_outside_frame": outside[name], "ms": {"median": med, "min": min(t[name]), "max": max(t[name])},
                   "written_TBps": elems * 4 / med / 1e9, "ratio_to_plain_gather": med / base if base else None,
                   "extra_ms_over_plain_gather": med - base if base else None,
                   "share_of_step": {k: med / v for k, v in STEP_MS.items()}, "mask_ms": tm[name], "rounds": rounds,
                   "calls_per_round": calls}
            print(f"{sname} {name:14s} {med:.4f} ms  {row['written_TBps']:.2f} TB/s written  ratio "
                  f"{row['ratio_to_plain_gather'] if base else float('nan'):.3f}  outside {outside[name]:.3f}  mask {tm[name]:.4f} ms", file=sys.stderr)
            rows.append(row)
        del c, dst, mdst, keep, fns, mfns
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cube_warp.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back launches per timed run")
    ap.add_argument("--store", choices=["fp32", "fp16", "both"], default="both")
    ap.add_argument("--only", action="append", help="run only this arm (repeatable); ratios need plain_gather among them")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cube_warp_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stores = {"fp32": [torch.float32], "fp16": [torch.float16], "both": [torch.float32, torch.float16]}[args.store]
    rep = {"device": torch.cuda.get_device_name(dev), "batch": [BATCH, BANDS, H, W], "source_bands": SRC_BANDS,
           "step_ms": STEP_MS, "arms": measure(dev, args.rounds, args.calls, stores, args.only)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({"out": args.out, "worst_ratio": max((r["ratio_to_plain_gather"] or 0) for r in rep["arms"])}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
