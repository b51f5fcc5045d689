#!/usr/bin/env python3
"""Spectral k-means (hyperpri_amd/cluster.py): what a fitting pass and a label map cost on the card, against two yardsticks of the
same session.

    python tools/cluster_probe.py                  # one MI355X; writes profiles/cluster.json
    python tools/cluster_probe.py --rounds 5 --out FILE

On slots of 608 x 968 x 238 (channel stride 240, fp32), by device events over runs of ``--calls`` back-to-back calls, the legs
interleaved round by round, median with min and max:

* ``fit``: one ``hpri_band_cluster_sums`` pass over four slots at K in {2, 8, 32, 64};
* ``assign``: ``hpri_band_assign`` (labels) on a gathered batch of two cubes at the same K, and the squared-distance map at K = 8;
* the floor: ``hpri_band_moments`` over the same slots -- one memory-bound read of the same bytes;
* the torch composite of the same work on the card: ``z = x @ W^T + b``, ``argmin``, and for the fit ``index_add_`` of the pixels
  into (K, cs) sums plus a ``bincount``.

Each of the two steps runs in a child process of its own under a time limit; the second is not started when the first fails.
Nothing is gated: the numbers and the ratios are recorded.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, BANDS, FIT_SLOTS, BATCH = 608, 968, 238, 4, 2
KS = (2, 8, 32, 64)
STEP_SECONDS = 240


def _events_ms(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _measure(legs, rounds, calls):
    for fn in legs.values():
        _events_ms(fn, 1)
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(_events_ms(fn, calls))
    return {k: _spread(v) for k, v in times.items()}


def _setup(n):
    import numpy as np
    import torch
    from hyperpri_amd import cluster as K
    from hyperpri_amd import spectral as S
    from hyperpri_amd.cache import CubeCache
    from hyperpri_amd.engine import synth_fill_
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cache = CubeCache(n, H, W, BANDS, device=dev)
    raw = torch.empty((H, W, BANDS), dtype=torch.float32, device=dev)
    m = torch.empty((H, W), dtype=torch.float32, device=dev)
    for k in range(n):
        synth_fill_(raw, 1234 + k, mode=0)
        synth_fill_(m, 4321 + k, mode=1, thr=0.9)
        cache.put(k, raw, m, name=f"cube{k}")
    torch.cuda.synchronize()
    cnt, sums = S.band_moments(cache)
    pivot = (sums[:BANDS] / cnt).astype(np.float32)
    sample = K._sample_pixels(cache, list(range(n)), 0, 0) - pivot.astype(np.float64)
    centers = {k: K.init_centers(sample, k, "sample", 0).astype(np.float32) for k in KS}
    return dev, cache, pivot, centers


def _rows(centers, cs, dev):
    import torch
    from hyperpri_amd import cluster as K
    w, b = K._padded_rows(centers, cs)
    return torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)


def step_fit(rounds, calls):
    import numpy as np
    import torch
    from hyperpri_amd import _lib
    from hyperpri_amd import cluster as K
    from hyperpri_amd import spectral as S
    from hyperpri_amd.engine import _p
    dev, cache, pivot, centers = _setup(FIT_SLOTS)
    cs = cache.cs
    idx = list(range(FIT_SLOTS))
    pixels = FIT_SLOTS * H * W
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    mom = S._Pass(cache, idx)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    msum = torch.empty(cs, dtype=torch.float64, device=dev)
    xf = cache._cubes[:FIT_SLOTS].reshape(pixels, cs)
    legs = {"moments": lambda: _lib.call("hpri_band_moments", *mom.head, 0, None, _p(mom.work), mom.nbytes, _p(count), _p(msum), None, stream)}
    passes, rows, disagree = {}, {}, {}
    for k in KS:
        ps = K._FitPass(cache, idx, pivot, k)
        wd, bd = _rows(centers[k], cs, dev)
        # the composite scores the uncentred pixel: W x + (b - W pivot) is the same affine map
        shift = (bd - wd @ ps.pivot)[:k]
        passes[k], rows[k] = ps, (wd, bd, wd[:k].t().contiguous(), shift)             # (the composite takes the K real rows only)

        def fit(k=k):
            ps, (wd, bd, _, _) = passes[k], rows[k]
            base = ps.out.data_ptr()
            _lib.call("hpri_band_cluster_sums", *ps.head, 0, _p(ps.pivot), _p(wd), _p(bd), k, _p(ps.work), ps.nbytes, base, base + 8 * k,
                      base + 8 * (k + k * cs), stream)

        def composite(k=k):
            _, _, wt, shift = rows[k]
            lab = torch.addmm(shift, xf, wt).argmin(dim=1)
            sums = torch.zeros((wt.shape[1], cs), dtype=torch.float32, device=dev).index_add_(0, lab, xf)
            return torch.bincount(lab, minlength=wt.shape[1]), sums
        legs[f"fit_k{k}"], legs[f"composite_k{k}"] = fit, composite
        fit()
        got = ps.out[:k].cpu().numpy().view(np.int64)
        disagree[k] = int(np.abs(got - composite()[0].cpu().numpy()).sum())
    ms = _measure(legs, rounds, calls)
    med = {k: v["median"] for k, v in ms.items()}
    nbytes = pixels * cs * 4
    return {"slots": FIT_SLOTS, "pixels": pixels, "bytes_read": nbytes, "ms": ms,
            "TBps": {k: nbytes / med[k] / 1e9 for k in med if not k.startswith("composite")},
            "fit_over_moments": {str(k): med[f"fit_k{k}"] / med["moments"] for k in KS},
            "composite_over_fit": {str(k): med[f"composite_k{k}"] / med[f"fit_k{k}"] for k in KS},
            "count_differences_kernel_vs_composite": {str(k): disagree[k] for k in KS}}


def step_assign(rounds, calls):
    import torch
    from hyperpri_amd import _lib
    from hyperpri_amd import cluster as K
    from hyperpri_amd import spectral as S
    from hyperpri_amd.engine import _p
    dev, cache, pivot, centers = _setup(BATCH)
    cs = cache.cs
    pixels = BATCH * H * W
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = cache.batch(list(range(BATCH)))["image"]
    xf = torch.as_strided(x, (pixels, cs), (cs, 1))
    mom = S._Pass(cache, list(range(BATCH)))
    count = torch.empty(1, dtype=torch.int64, device=dev)
    msum = torch.empty(cs, dtype=torch.float64, device=dev)
    legs = {"moments": lambda: _lib.call("hpri_band_moments", *mom.head, 0, None, _p(mom.work), mom.nbytes, _p(count), _p(msum), None, stream)}
    models = {k: K.SpectralKMeans(pivot, centers[k]).to(dev) for k in KS}
    disagree = {}
    for k in KS:
        pv, wd, bd = models[k]._device_rows(dev, cs)
        shift = (bd - wd @ pv)[:k]
        wt = wd[:k].t().contiguous()                           # (the composite takes the K real rows only)
        legs[f"assign_k{k}"] = lambda k=k: models[k](x, output="labels")
        legs[f"composite_k{k}"] = lambda wt=wt, shift=shift: torch.addmm(shift, xf, wt).argmin(dim=1)
        disagree[k] = int((legs[f"assign_k{k}"]().reshape(-1).to(torch.int64) != legs[f"composite_k{k}"]()).sum())
    legs["distance_k8"] = lambda: models[8](x, output="distance")
    ms = _measure(legs, rounds, calls)
    med = {k: v["median"] for k, v in ms.items()}
    nbytes = pixels * cs * 4
    return {"batch": [BATCH, BANDS, H, W], "pixels": pixels, "bytes_read": nbytes, "ms": ms,
            "TBps": {k: nbytes / med[k] / 1e9 for k in med if not k.startswith("composite")},
            "assign_over_moments": {str(k): med[f"assign_k{k}"] / med["moments"] for k in KS},
            "composite_over_assign": {str(k): med[f"composite_k{k}"] / med[f"assign_k{k}"] for k in KS},
            "label_differences_kernel_vs_composite": {str(k): disagree[k] for k in KS}}


STEPS = {"fit": step_fit, "assign": step_assign}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2, help="back-to-back calls per timed run")
    ap.add_argument("--step", choices=sorted(STEPS), help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            sys.exit("cluster_probe: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
        rep = STEPS[args.step](args.rounds, args.calls)
        rep["device"] = torch.cuda.get_device_name(0)
        print("CLUSTER_PROBE " + json.dumps(rep))
        return 0
    rep = {"channel_stride": (BANDS + 7) // 8 * 8, "rounds": args.rounds, "calls_per_round": args.calls}
    for name in ("fit", "assign"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--rounds", str(args.rounds), "--calls", str(args.calls)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired:
            sys.exit(f"cluster_probe: step {name} ran into its limit of {STEP_SECONDS} s; nothing more is started")
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("CLUSTER_PROBE ")), None)
        if r.returncode != 0 or line is None:
            sys.exit(f"cluster_probe: step {name} failed (exit {r.returncode}); nothing more is started\n{r.stdout[-3000:]}")
        rep[name] = json.loads(line[len("CLUSTER_PROBE "):])
        rep["device"] = rep[name].pop("device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({"out": args.out, "fit_ms": {k: v["median"] for k, v in rep["fit"]["ms"].items()},
                      "fit_over_moments": rep["fit"]["fit_over_moments"], "composite_over_fit": rep["fit"]["composite_over_fit"],
                      "assign_ms": {k: v["median"] for k, v in rep["assign"]["ms"].items()},
                      "assign_over_moments": rep["assign"]["assign_over_moments"],
                      "composite_over_assign": rep["assign"]["composite_over_assign"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
