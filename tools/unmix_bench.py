#!/usr/bin/env python3
"""Spectral unmixing (hyperpri_amd/unmix.py): what an abundance map costs on the card, what the active-set solver adds to the
projection, and what the host route costs.

    python tools/unmix_bench.py                    # one MI355X; writes profiles/unmix.json
    python tools/unmix_bench.py --rounds 5 --out FILE

Four cached 608 x 968 x 238 cubes of sparse mixtures of eight smooth endmembers (normalised 1 / 0.3 powers of uniforms, close to
Dirichlet(0.3)) plus N(0, 0.03^2) noise, every fifth pixel noise only, made on the device from a seed.  On a gathered batch of two of them (the layout ``CubeCache`` hands out), by device events over runs
of ``--calls`` back-to-back calls, the legs interleaved round by round, median with min and max:

* ``ucls`` and ``fcls`` abundance maps at M = 2, 4, 8 (the first M endmembers); ``fcls - ucls`` is the price of the solver;
* ``fcls`` at M = 8 with the ``rmse`` and with the ``logit`` output added;
* one ATGP step (``hpri_band_extreme``, four rows) over the four cached cubes;
* the plain gather of the batch (``hpri_cube_gather``), the project's measure of "gather speed";
* the ``cholesky`` ACE detector on the same batch, the family's closest kernel.

The host route -- ``unmix_reference`` (vectorised fp64 numpy) on 10 000 pixels of the batch, scaled to the batch -- is recorded as
what it is, an extrapolation.  Bytes are the batch read once plus the maps written once.  Nothing is gated: the numbers are
recorded.
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

H, W, BANDS, BATCH, CUBES, MEMBERS, HOST_PIXELS = 608, 968, 238, 2, 4, (2, 4, 8), 10000


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


def _endmembers(M):
    t = np.linspace(0.0, 1.0, BANDS)
    m = np.arange(M)[:, None]
    return (0.3 + 0.25 * np.sin(2 * np.pi * (0.5 + 0.3 * m) * t[None, :] + m) + 0.1 * m * t[None, :]).astype(np.float32)


def _fill(cache, E, dev):
    g = torch.Generator(device=dev)
    Ed = torch.from_numpy(E).to(dev)
    for k in range(CUBES):
        g.manual_seed(1234 + k)
        u = torch.rand((H * W, E.shape[0]), generator=g, device=dev).clamp_min(1e-12)
        a = u ** (1.0 / 0.3)                                 # (normalised powers of uniforms: sparse mixtures like Dirichlet(0.3)'s)
        a = a / a.sum(dim=1, keepdim=True)
        noise = 0.03 * torch.randn((H * W, BANDS), generator=g, device=dev)
        x = a @ Ed + noise
        x[::5] = noise[::5]
        cache.put(k, x.reshape(H, W, BANDS), (a[:, 0] > 0.5).to(torch.float32).reshape(H, W), name=f"cube{k}")
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unmix.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2, help="back-to-back calls per timed run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("unmix_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
    from hyperpri_amd import _lib
    from hyperpri_amd import detect as D
    from hyperpri_amd import spectral as S
    from hyperpri_amd import unmix as Um
    from hyperpri_amd.cache import _DT, CubeCache
    from hyperpri_amd.engine import _p
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    E = _endmembers(max(MEMBERS))
    cache = CubeCache(CUBES, H, W, BANDS, device=dev)
    _fill(cache, E, dev)
    cs = cache.cs
    models = {M: Um.SpectralUnmixer(E[:M], foreground=[True] + [False] * (M - 1)).to(dev) for M in MEMBERS}
    chol = D.SpectralDetector.from_statistics(S.band_statistics(cache, select="background"), S.class_spectra(cache)["foreground"]["mean"],
                                              whitener="cholesky").to(dev)
    x = cache.batch(list(range(BATCH)))["image"]
    pixels = BATCH * H * W
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = torch.tensor([[i, 0, 0, 0] for i in range(BATCH)], dtype=torch.int32).to(dev)
    dst = torch.empty((BATCH, H, W, cs), dtype=torch.float32, device=dev)
    # one ATGP step with four rows: the rows of the first four picks
    spectra, picks = Um.extract_endmembers(cache, 4)
    rows = []
    for s in spectra:
        rows.append(Um._atgp_row(s, rows))
    basis = torch.zeros((16, cs), dtype=torch.float32, device=dev)
    basis[:4, :BANDS] = torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev)
    slots = torch.arange(CUBES, dtype=torch.int32).to(dev)
    nbytes = int(_lib.load().hpri_band_extreme_workspace_bytes())
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(2, dtype=torch.int64, device=dev)

    def leg_atgp():
        _lib.call("hpri_band_extreme", _p(cache._cubes), _DT[cache.store_dtype], cache.capacity, H, W, cs, _p(cache._masks), _p(slots), CUBES, 0,
                  _p(basis), 4, _p(work), nbytes, out.data_ptr() + 8, out.data_ptr(), stream)

    def leg_gather():
        _lib.call("hpri_cube_gather", _p(cache._cubes), 0, cache.capacity, H, W, cs, _p(table), BATCH, H, W, _p(dst), stream)
    legs = {}
    for M in MEMBERS:
        for mode in ("ucls", "fcls"):
            legs[f"{mode}_M{M}"] = (lambda M=M, mode=mode: models[M](x, mode=mode))
    legs["fcls_M8_rmse"] = lambda: models[8](x, output="rmse")
    legs["fcls_M8_logit"] = lambda: models[8](x, output="logit")
    legs["atgp_step_4_cubes"] = leg_atgp
    legs["gather"] = leg_gather
    legs["cholesky_ace"] = lambda: chol(x, score="ace")
    for fn in legs.values():
        _events_ms(fn, 1)
    capped = {}
    for M in MEMBERS:
        models[M](x, mode="fcls")
        capped[f"fcls_M{M}"] = models[M].capped
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(_events_ms(fn, args.calls))
    med = {k: statistics.median(v) for k, v in times.items()}
    # the host route: the vectorised fp64 restatement on a sample of the batch, scaled
    sample = torch.as_strided(x, (pixels, cs), (cs, 1))[:HOST_PIXELS, :BANDS].cpu().numpy()
    host = {}
    for M in MEMBERS:
        Q32, R = models[M].basis.cpu().numpy(), models[M].tri.cpu().numpy()
        t0 = time.perf_counter()
        _, its, _, _ = Um.unmix_reference(sample, Q32, R, "fcls")
        dt = time.perf_counter() - t0
        host[f"fcls_M{M}"] = {"seconds_on_sample": dt, "sample_pixels": HOST_PIXELS, "extrapolated_seconds_for_the_batch": dt * pixels / HOST_PIXELS,
                              "max_sub_solves": int(its.max()), "mean_sub_solves": float(its.mean())}
    rep = {"device": torch.cuda.get_device_name(dev), "batch": [BATCH, BANDS, H, W], "channel_stride": cs, "pixels": pixels,
           "rounds": args.rounds, "calls_per_round": args.calls, "ms": {k: _spread(v) for k, v in times.items()},
           "solver_ms_fcls_minus_ucls": {f"M{M}": med[f"fcls_M{M}"] - med[f"ucls_M{M}"] for M in MEMBERS},
           "bytes": {f"M{M}": pixels * (cs + M) * 4 for M in MEMBERS},
           "TBps": {f"{mode}_M{M}": pixels * (cs + M) * 4 / med[f"{mode}_M{M}"] / 1e9 for M in MEMBERS for mode in ("ucls", "fcls")},
           "atgp_bytes": CUBES * H * W * cs * 4, "atgp_TBps": CUBES * H * W * cs * 4 / med["atgp_step_4_cubes"] / 1e9,
           "gather_bytes": pixels * cs * 8, "gather_TBps": pixels * cs * 8 / med["gather"] / 1e9,
           "capped_pixels": capped, "atgp_picks": [[int(e), int(p)] for e, p in picks],
           "host_route_extrapolated": host}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({"out": args.out, "ms": med, "solver_ms": rep["solver_ms_fcls_minus_ucls"],
                      "host_s": {k: v["extrapolated_seconds_for_the_batch"] for k, v in host.items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
