#!/usr/bin/env python3
"""Spectral statistics and projection (hyperpri_amd/spectral.py): what they cost on the card, and what the route without them costs.

    python tools/spectral_bench.py                 # one MI355X; writes profiles/spectral.json
    python tools/spectral_bench.py --cubes 8 --out FILE

(a) ``band_statistics`` over a filled fp32 cache of 238-band 608 x 968 cubes -- as many as ``--cubes`` (default 44, a HyperPRI
    training fold) and the free device memory allow; the count is recorded.  Host clock around the call, which ends in the
    device-to-host copy of its result; the moments and the Gram pass also on their own, by device events.  The Gram pass'
    operations are the ones its contract needs, ``2 P cs (cs + 1) / 2`` for the upper triangle it computes, over its time.
    Against it, in the same run: the route the package offered before -- ``.cpu()`` of the same slots, one at a time, and fp64
    numpy (sum, ``X^T X``) on the host's threads -- and the two results compared.
(b) ``SpectralProjection.pca(k=32)`` on a batch of two of those cubes (the layout ``CubeCache`` hands out): the kernel by itself into
    a preallocated buffer and the module call (which adds ``torch.empty`` and the Python around it), by device events over runs of
    ``--calls`` back-to-back calls; bytes = the batch read once + the output written once.  Against it, interleaved round by
    round: the plain gather of that same batch (``hpri_cube_gather``), the project's measure of "gather speed".
Nothing is gated: the numbers and the ratios are recorded.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, BANDS, BATCH, K = 608, 968, 238, 2, 32


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


def host_route(cache, n):
    """Count, mean and covariance of slots 0 .. n-1 the way the parent commit allows: every slot to the host, fp64 numpy there."""
    C = cache.C
    sums, gram, count = np.zeros(C), np.zeros((C, C)), 0
    for i in range(n):
        x = cache._cubes[i].cpu().numpy().reshape(-1, cache.cs)[:, :C].astype(np.float64)
        sums += x.sum(axis=0)
        gram += x.T @ x
        count += x.shape[0]
    mean = sums / count
    return count, mean, (gram - count * np.outer(mean, mean)) / (count - 1)


def statistics_leg(cache, n, rounds):
    from hyperpri_amd import spectral as S
    S.band_statistics(cache, slots=[0])                     # warm-up: code objects, the workspace in the allocator
    dev_s = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = S.band_statistics(cache)
        dev_s.append(time.perf_counter() - t0)
    ps = S._Pass(cache, list(range(n)))
    pivot = ps.pivot(st.mean)
    work, nbytes = ps.work, ps.nbytes
    from hyperpri_amd import _lib
    from hyperpri_amd.engine import _p, _stream
    count = torch.empty(1, dtype=torch.int64, device=cache.device)
    sums = torch.empty(cache.cs, dtype=torch.float64, device=cache.device)
    g = torch.empty((cache.cs, cache.cs), dtype=torch.float64, device=cache.device)

    def moments():
        _lib.call("hpri_band_moments", *ps.head, 0, None, _p(work), nbytes, _p(count), _p(sums), None, _stream())

    def gram():
        _lib.call("hpri_band_gram", *ps.head, 0, _p(pivot), _p(work), nbytes, _p(g), _stream())
    mo = [_events_ms(moments, 1) for _ in range(rounds + 1)][1:]
    gr = [_events_ms(gram, 1) for _ in range(rounds + 1)][1:]
    t0 = time.perf_counter()
    hc, hmean, hcov = host_route(cache, n)
    host_s = time.perf_counter() - t0
    pixels = n * H * W
    cs = cache.cs
    slot_bytes = pixels * cs * 4
    gram_flop = pixels * cs * (cs + 1)                      # 2 * pixels * cs (cs + 1) / 2: the triangle the contract needs
    mo_ms, gr_ms, dev_med = statistics.median(mo), statistics.median(gr), statistics.median(dev_s)
    row = {"cubes": n, "frame": [H, W], "bands": BANDS, "channel_stride": cs, "store": "fp32", "pixels": pixels, "slot_bytes": slot_bytes,
           "band_statistics_s": _spread(dev_s), "moments_ms": _spread(mo), "gram_ms": _spread(gr),
           "moments_TBps": slot_bytes / mo_ms / 1e9, "gram_TBps": slot_bytes / gr_ms / 1e9, "gram_TFLOPs": gram_flop / gr_ms / 1e9,
           "gram_flop": gram_flop, "host_route_s": host_s, "host_threads": torch.get_num_threads(), "speedup": host_s / dev_med,
           "rounds": rounds, "count_equal": int(hc) == int(st.count),
           "max_rel_mean_diff": float(np.abs(st.mean - hmean).max() / np.abs(hmean).max()),
           "max_cov_diff_over_max_cov": float(np.abs(st.cov - hcov).max() / np.abs(hcov).max()),
           "note": "host route: one slot at a time, .cpu() then fp64 numpy (sum and X^T X), timed once; band_statistics: host clock "
                   "around the whole call (two passes, two device-to-host copies, the fp64 algebra)"}
    print(f"statistics: {n} cubes  band_statistics {dev_med:.3f} s (moments {mo_ms:.2f} ms, gram {gr_ms:.2f} ms = "
          f"{row['gram_TFLOPs']:.1f} TFLOP/s)  host route {host_s:.1f} s  x{row['speedup']:.0f}", file=sys.stderr)
    return row, st


def projection_leg(cache, st, rounds, calls):
    from hyperpri_amd import _lib
    from hyperpri_amd import spectral as S
    from hyperpri_amd.engine import _p
    dev = cache.device
    cs = cache.cs
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    proj = S.SpectralProjection.pca(st, K).to(dev)
    x = cache.batch(list(range(BATCH)))["image"]
    wd, bd = proj._device_weights(dev, cs)
    ks = (K + 7) // 8 * 8
    y = torch.empty((BATCH, H, W, ks), dtype=torch.float32, device=dev)
    src = x[:, 0]
    table = torch.tensor([[i, 0, 0, 0] for i in range(BATCH)], dtype=torch.int32).to(dev)
    dst = torch.empty((BATCH, H, W, cs), dtype=torch.float32, device=dev)
    pixels = BATCH * H * W

    def kernel():
        _lib.call("hpri_band_project", _p(src), pixels, cs, _p(wd), _p(bd), K, _p(y), stream)

    def module():
        proj(x)

    def gather():
        _lib.call("hpri_cube_gather", _p(cache._cubes), 0, cache.capacity, H, W, cs, _p(table), BATCH, H, W, _p(dst), stream)
    for fn in (kernel, module, gather):
        _events_ms(fn, calls)
    assert torch.equal(torch.as_strided(proj(x)[:, 0], (BATCH, H, W, ks), (H * W * ks, W * ks, ks, 1)), y)
    kt, mt, gt = [], [], []
    for _ in range(rounds):
        kt.append(_events_ms(kernel, calls))
        gt.append(_events_ms(gather, calls))
        mt.append(_events_ms(module, calls))
    km, mm, gm = statistics.median(kt), statistics.median(mt), statistics.median(gt)
    pbytes = pixels * (cs + ks) * 4
    gbytes = pixels * cs * 8
    row = {"batch": [BATCH, BANDS, H, W], "k": K, "channel_stride": cs, "out_stride": ks, "bytes": pbytes, "flop": 2 * pixels * cs * ks,
           "project_kernel_ms": _spread(kt), "project_module_ms": _spread(mt), "gather_ms": _spread(gt), "gather_bytes": gbytes,
           "project_TBps": pbytes / km / 1e9, "project_TFLOPs": 2 * pixels * cs * ks / km / 1e9, "gather_TBps": gbytes / gm / 1e9,
           "ratio_kernel_to_gather": km / gm, "ratio_module_to_gather": mm / gm, "rounds": rounds, "calls_per_round": calls}
    print(f"projection: kernel {km:.4f} ms ({row['project_TBps']:.2f} TB/s, {row['project_TFLOPs']:.1f} TFLOP/s)  module {mm:.4f} ms  "
          f"gather {gm:.4f} ms ({row['gather_TBps']:.2f} TB/s)  kernel / gather {row['ratio_kernel_to_gather']:.2f}", file=sys.stderr)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral.json"))
    ap.add_argument("--cubes", type=int, default=44)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--proj-rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed run of the projection leg")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spectral_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
    from hyperpri_amd.cache import CubeCache
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    free, _ = torch.cuda.mem_get_info(dev)
    slot = CubeCache.planned_bytes(1, H, W, BANDS)
    n = int(max(BATCH, min(args.cubes, (free - 8 * 2 ** 30) // slot)))      # (8 GB stay free: output buffers, workspace, the allocator)
    cache = CubeCache(n, H, W, BANDS, device=dev)
    _fill(cache, n, dev)
    rep = {"device": torch.cuda.get_device_name(dev), "cubes_asked": args.cubes, "cubes": n}
    rep["statistics"], st = statistics_leg(cache, n, args.rounds)
    rep["projection"] = projection_leg(cache, st, args.proj_rounds, args.calls)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({"out": args.out, "cubes": n, "statistics_speedup": rep["statistics"]["speedup"],
                      "project_over_gather": rep["projection"]["ratio_kernel_to_gather"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
