#!/usr/bin/env python3
"""Ridge filter (hyperpri_amd/ridge.py): what a multi-scale Hessian ridge measure of a batch of planes costs on the card, against the
usual torch route.

    python tools/ridge_bench.py                    # one MI355X; writes profiles/ridge.json
    python tools/ridge_bench.py --rounds 5 --out FILE

Two cached 608 x 968 x 238 cubes (a smooth low-rank scene plus noise, made on the device from a seed), gathered as one batch (the
layout ``CubeCache`` hands out).  The planes are the first T = 1 and T = 8 principal components of the batch (``SpectralProjection.pca``,
read zero-copy with a pixel stride of 8), filtered with frangi, bright, at S = 1, 3, 5 scales.  By device events over runs of
``--calls`` back-to-back calls, the legs interleaved round by round, median with min and max:

* ``RidgeFilter`` (one launch);
* a torch composite of the usual route on the same device: a symmetric pad, six 1-d ``conv2d`` per scale with the full kernels (centre
  taps included) on the values themselves, the eigen-analysis and the measure elementwise, the maximum over the scales;
* the plain gather of the batch (``hpri_cube_gather``), the project's measure of "gather speed".

Accuracy, on a 96 x 128 crop against ``ridge_reference`` (fp64 numpy on the same fp32 inputs): the largest error of the Hessian planes
and of the response, for the filter (also as the largest fraction of ``ridge_bound``) and for the composite, on the first component as it
is and on that plane shifted to a mean of 1000 with a variation of 0.01 -- the mean far larger than the local variation that makes
zero-sum taps cancel.  Nothing is gated: the numbers are recorded."""
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
import torch.nn.functional as F  # noqa: E402

from guided_bench import BANDS, BATCH, H, W, _events_ms, _fill, _spread  # noqa: E402

SCALES = {1: (1.5,), 3: (1.0, 2.0, 3.0), 5: (0.75, 1.0, 1.5, 2.0, 3.0)}
MAPS, CROP, BETA = (1, 8), (96, 128), 0.5


def _kernels(sigma, dev):
    from hyperpri_amd.ridge import ridge_taps
    R, g0, g1, g2 = ridge_taps(sigma)
    k0 = np.concatenate([g0[::-1], [np.float32(1.0 - 2.0 * g0.astype(np.float64).sum())], g0])
    k1 = np.concatenate([-g1[::-1], [np.float32(0.0)], g1])
    k2 = np.concatenate([g2[::-1], [np.float32(-2.0 * g2.astype(np.float64).sum())], g2])
    return R, [torch.from_numpy(k.astype(np.float32)).to(dev) for k in (k0, k1, k2)]


def _rho(i, n):
    m = i % (2 * n)
    return torch.where(m < n, m, 2 * n - 1 - m)


def composite(planes, sigmas, beta, c, kernels, return_hessian=False):
    """The usual route out of torch operators, frangi, bright: planes (N, T, h, w) -> the response (N, T, h, w)."""
    N, T, h, w = planes.shape
    x = planes.reshape(N * T, 1, h, w)
    best, hess = None, []
    for s in sigmas:
        R, (k0, k1, k2) = kernels[s]
        iy, ix = _rho(torch.arange(-R, h + R, device=x.device), h), _rho(torch.arange(-R, w + R, device=x.device), w)
        pad = x[:, :, iy][:, :, :, ix]
        rows = [F.conv2d(pad, k.view(1, 1, 1, -1)) for k in (k2, k1, k0)]
        s2 = float(np.float32(s * s))
        hxx, hxy, hyy = (F.conv2d(r, k.view(1, 1, -1, 1)) * s2 for r, k in zip(rows, (k0, k1, k2)))
        mu, hd = (hxx + hyy) / 2, (hxx - hyy) / 2
        d = torch.sqrt(hd * hd + hxy * hxy)
        l2, l1 = mu - d, mu + d
        ok = (mu < 0) & (l2 != 0)
        rb = l1 / torch.where(ok, l2, torch.ones_like(l2))
        v = torch.where(ok, torch.exp(-(rb * rb) / (2 * beta * beta)) * (-torch.expm1(-(l1 * l1 + l2 * l2) / (2 * c * c))), torch.zeros_like(mu))
        best = v if best is None else torch.maximum(best, v)
        if return_hessian:
            hess.append(torch.stack([hxx, hxy, hyy], dim=1).reshape(N, T, 3, h, w))
    best = best.reshape(N, T, h, w)
    return (best, torch.stack(hess, dim=2)) if return_hessian else best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ridge.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="back-to-back calls per timed run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ridge_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
    from hyperpri_amd import _lib
    from hyperpri_amd import ridge as R
    from hyperpri_amd import spectral as S
    from hyperpri_amd.cache import CubeCache
    from hyperpri_amd.engine import _p
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cache = CubeCache(BATCH, H, W, BANDS, device=dev)
    _fill(cache, dev)
    cs = cache.cs
    x = cache.batch(list(range(BATCH)))["image"]
    proj = S.SpectralProjection.pca(S.band_statistics(cache), 8).to(dev)
    pcs = proj(x)
    pcs = pcs[:, 0] if pcs.dim() == 5 else pcs                                          # (N, 8, h, w), pixel stride 8
    planes = {T: pcs[:, :T] for T in MAPS}
    assert all(R._plane_input(planes[T])[0].data_ptr() == pcs.data_ptr() and R._plane_input(planes[T])[3] == 8 for T in MAPS)
    plain = {T: planes[T].contiguous() for T in MAPS}                                   # the composite reads NCHW
    c = float(np.float32(pcs[:, 0].std().item()))                                       # the structure scale: the plane's own spread
    kernels = {s: _kernels(s, dev) for sig in SCALES.values() for s in sig}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = torch.tensor([[i, 0, 0, 0] for i in range(BATCH)], dtype=torch.int32).to(dev)
    dst = torch.empty((BATCH, H, W, cs), dtype=torch.float32, device=dev)
    legs = {"gather": lambda: _lib.call("hpri_cube_gather", _p(cache._cubes), 0, cache.capacity, H, W, cs, _p(table), BATCH, H, W, _p(dst), stream)}
    for nS, sig in SCALES.items():
        mod = R.RidgeFilter(sig, "frangi", "bright", BETA, c)
        for T in MAPS:
            legs[f"filter_S{nS}_T{T}"] = (lambda mod=mod, T=T: mod(planes[T]))
            legs[f"composite_S{nS}_T{T}"] = (lambda sig=sig, T=T: composite(plain[T], sig, BETA, c, kernels))
    for fn in legs.values():
        _events_ms(fn, 1)
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(_events_ms(fn, args.calls))
    med = {k: statistics.median(v) for k, v in times.items()}
    # accuracy on a crop: the filter and the composite against the fp64 restatement
    ch, cw = CROP
    sig = SCALES[5]
    base = plain[1][:1, :, :ch, :cw].contiguous()
    local = base - base.mean(dim=(2, 3), keepdim=True)
    shifted = 1000.0 + 0.01 * local / local.abs().max()
    errors = {}
    for name, g, cc in (("pca", base, c), ("pca_shifted_1000_scaled_0.01", shifted, float(np.float32(shifted.std().item())))):
        ref, bound = R.ridge_reference(g.cpu().numpy(), sig, "frangi", "bright", BETA, cc), R.ridge_bound(g.cpu().numpy(), sig, "frangi", "bright", BETA, cc)
        v, hess = R.ridge_filter(g, sig, "frangi", "bright", BETA, cc, return_hessian=True)
        tv, thess = composite(g, sig, BETA, cc, kernels, return_hessian=True)
        v, hess, tv, thess = (a.cpu().numpy().astype(np.float64) for a in (v, hess, tv, thess))
        keep = ~bound["undecided"]
        with np.errstate(divide="ignore", invalid="ignore"):
            fh = np.where(bound["hessian"] > 0, np.abs(hess - ref["hessian"]) / bound["hessian"], 0.0).max()
            fv = np.where(keep, np.abs(v - ref["response"]) / bound["value"], 0.0).max()
        errors[name] = {"filter_hessian_max_abs_error": float(np.abs(hess - ref["hessian"]).max()),
                        "composite_hessian_max_abs_error": float(np.abs(thess - ref["hessian"]).max()),
                        "filter_response_max_abs_error": float(np.abs(v - ref["response"])[keep].max()),
                        "composite_response_max_abs_error": float(np.abs(tv - ref["response"])[keep].max()),
                        "filter_hessian_fraction_of_bound": float(fh), "filter_response_fraction_of_bound": float(fv),
                        "undecided_share": float(1 - keep.mean()), "hessian_max_abs": float(np.abs(ref["hessian"]).max()),
                        "response_max": float(ref["response"].max()), "plane_mean": float(g.mean()), "plane_std": float(g.std()), "c": cc,
                        "sigmas": list(sig)}
    pixels = BATCH * H * W
    rep = {"device": torch.cuda.get_device_name(dev), "batch": [BATCH, BANDS, H, W], "plane_pixel_stride": 8, "pixels": pixels,
           "measure": "frangi", "polarity": "bright", "beta": BETA, "c": c, "scales": {str(k): list(v) for k, v in SCALES.items()},
           "rounds": args.rounds, "calls_per_round": args.calls, "ms": {k: _spread(v) for k, v in times.items()},
           "speedup_over_composite": {k[len("filter_"):]: med["composite_" + k[len("filter_"):]] / v for k, v in med.items() if k.startswith("filter_")},
           "gather_bytes": pixels * cs * 8, "gather_TBps": pixels * cs * 8 / med["gather"] / 1e9, "error_on_a_crop": errors}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({"out": args.out, "ms": med, "errors": errors}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
