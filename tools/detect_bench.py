#!/usr/bin/env python3
"""Spectral detectors (hyperpri_amd/detect.py): what a score map costs on the card, and what the torch composite of the same
arithmetic costs.

    python tools/detect_bench.py                   # one MI355X; writes profiles/detect.json
    python tools/detect_bench.py --rounds 5 --out FILE

On a gathered batch of two 608 x 968 x 238 cubes (the layout ``CubeCache`` hands out), by device events over runs of ``--calls``
back-to-back calls, the legs interleaved round by round, median with min and max:

* the ``cholesky`` detector, ``score="ace"`` (a lower-triangular whitener: the column extents skip about half the MFMAs);
* the ``pca`` detector at rank 32;
* the SAM path (identity metric, no matrix unit);
* the torch composite of the cholesky detector's arithmetic: ``z = (x - mu) @ W^T``, ``q = (z * z).sum(1)``, ``t = (x - mu) @ f``,
  ``t / sqrt(q)`` -- hipBLASLt's fp32 GEMM plus elementwise passes that move the whitened copy through HBM;
* the plain gather of that batch (``hpri_cube_gather``), the project's measure of "gather speed".

TFLOP/s are those of the MFMA work the kernel executes (``2 * 16 * cend`` per pixel and 16-row block, pad rows included); bytes
are the batch read once plus the maps written once.  Nothing is gated: the numbers and the ratios are recorded.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, BANDS, BATCH, RANK, CUBES = 608, 968, 238, 2, 32, 4
FP32_MFMA_PEAK_TFLOPS = 157.3


def _events_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _fill(cache, n, dev):
    from hyperpri_amd.engine import synth_fill_
    raw = torch.empty((H, W, BANDS), dtype=torch.float32, device=dev)
    m = torch.empty((H, W), dtype=torch.float32, device=dev)
    for k in range(n):
        synth_fill_(raw, 1234 + k, mode=0)
        synth_fill_(m, 4321 + k, mode=1, thr=0.9)
        cache.put(k, raw, m, name=f"cube{k}")
    torch.cuda.synchronize()


def _executed_flop(det, kind, cs, pixels):
    _, _, cend = det.host_weights(kind, cs)
    return 2 * 16 * int(np.asarray(cend, dtype=np.int64).sum()) * pixels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=4, help="back-to-back calls per timed run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("detect_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
    from hyperpri_amd import _lib
    from hyperpri_amd import detect as D
    from hyperpri_amd import spectral as S
    from hyperpri_amd.cache import CubeCache
    from hyperpri_amd.engine import _p
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cache = CubeCache(CUBES, H, W, BANDS, device=dev)
    _fill(cache, CUBES, dev)
    cs = cache.cs
    stats = S.band_statistics(cache, select="background")
    target = S.class_spectra(cache)["foreground"]["mean"]
    chol = D.SpectralDetector.from_statistics(stats, target, whitener="cholesky").to(dev)
    pca = D.SpectralDetector.from_statistics(stats, target, whitener="pca", rank=RANK).to(dev)
    x = cache.batch(list(range(BATCH)))["image"]
    pixels = BATCH * H * W
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = torch.tensor([[i, 0, 0, 0] for i in range(BATCH)], dtype=torch.int32).to(dev)
    dst = torch.empty((BATCH, H, W, cs), dtype=torch.float32, device=dev)
    # the composite's operands: the padded batch as a (P, cs) matrix, mu, W^T and the ACE filter on the device
    xf = torch.as_strided(x, (pixels, cs), (cs, 1))
    w, b, cend = chol.host_weights("ace", cs)
    Kq = chol.rank
    mu = torch.zeros(cs, dtype=torch.float32, device=dev)
    mu[:BANDS] = torch.from_numpy(stats.mean.astype(np.float32)).to(dev)
    Wt = torch.from_numpy(np.ascontiguousarray(w[:Kq].T)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(w[Kq])).to(dev)

    def leg_chol():
        return chol(x, score="ace")

    def leg_pca():
        return pca(x, score="ace")

    def leg_sam():
        return chol(x, score="sam")

    def leg_composite():
        d = xf - mu
        z = d @ Wt
        q = (z * z).sum(dim=1)
        return (d @ f) / q.sqrt()

    def leg_gather():
        _lib.call("hpri_cube_gather", _p(cache._cubes), 0, cache.capacity, H, W, cs, _p(table), BATCH, H, W, _p(dst), stream)
    legs = {"cholesky_ace": leg_chol, "pca32_ace": leg_pca, "sam": leg_sam, "torch_composite": leg_composite, "gather": leg_gather}
    for fn in legs.values():
        _events_ms(fn, 1)
    # the composite computes what the kernel computes (the bias is -W mu rounded once; the composite subtracts mu first)
    diff = float((leg_chol().reshape(-1) - leg_composite()).abs().max())
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(_events_ms(fn, args.calls))
    med = {k: statistics.median(v) for k, v in times.items()}
    flop = {"cholesky_ace": _executed_flop(chol, "ace", cs, pixels), "pca32_ace": _executed_flop(pca, "ace", cs, pixels)}
    bytes_moved = pixels * (cs + 1) * 4
    rep = {"device": torch.cuda.get_device_name(dev), "batch": [BATCH, BANDS, H, W], "channel_stride": cs, "pixels": pixels,
           "rounds": args.rounds, "calls_per_round": args.calls, "ms": {k: _spread(v) for k, v in times.items()},
           "executed_mfma_flop": flop, "dense_flop_cholesky": 2 * pixels * cs * (Kq + 1), "column_extents_cholesky": [int(c) for c in cend],
           "TFLOPs_executed": {k: flop[k] / med[k] / 1e9 for k in flop},
           "fraction_of_fp32_mfma_peak": {k: flop[k] / med[k] / 1e9 / FP32_MFMA_PEAK_TFLOPS for k in flop},
           "bytes": bytes_moved, "TBps": {k: bytes_moved / med[k] / 1e9 for k in ("cholesky_ace", "pca32_ace", "sam")},
           "gather_bytes": pixels * cs * 8, "gather_TBps": pixels * cs * 8 / med["gather"] / 1e9,
           "composite_over_cholesky": med["torch_composite"] / med["cholesky_ace"], "max_abs_diff_kernel_composite": diff}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({"out": args.out, "ms": med, "TFLOPs_executed": rep["TFLOPs_executed"],
                      "composite_over_cholesky": rep["composite_over_cholesky"], "max_abs_diff": diff}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
