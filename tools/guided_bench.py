#!/usr/bin/env python3
"""Guided filter (hyperpri_amd/guided.py): what refining a batch of score maps costs on the card, against the usual torch route.

    python tools/guided_bench.py                    # one MI355X; writes profiles/guided.json
    python tools/guided_bench.py --rounds 5 --out FILE

Two cached 608 x 968 x 238 cubes (a smooth low-rank scene plus noise, made on the device from a seed), gathered as one batch (the
layout ``CubeCache`` hands out).  The guide is the first 1 and the first 3 principal components of the batch (``SpectralProjection.pca``,
read zero-copy with a channel stride of 8); the maps are T = 1 and T = 8 planes of logits, filtered in the ``prob`` domain at r = 2, 4,
8.  By device events over runs of ``--calls`` back-to-back calls, the legs interleaved round by round, median with min and max:

* ``GuidedFilter`` (two launches);
* a torch composite of the published algorithm on the same device: ``avg_pool2d(count_include_pad=False)`` box means, the moment form
  ``E[I I^T] - E[I] E[I]^T``, the 3 x 3 inverse by cofactors, ``mean(a) . I + mean(b)``, with the sigmoid in front and the logit behind;
* the plain gather of the batch (``hpri_cube_gather``), the project's measure of "gather speed".

Accuracy, on a 96 x 128 crop against ``guided_reference`` (fp64 numpy on the same fp32 inputs, before the logit): the largest error of
the filter and of the composite under the principal-component guide, and under that guide shifted by 1000 and scaled to 0.01 -- the
mean far larger than the local variation that breaks the moment form.  Nothing is gated: the numbers are recorded."""
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
import torch.nn.functional as F  # noqa: E402

H, W, BANDS, BATCH, RADII, MAPS, GUIDES, EPS, CROP = 608, 968, 238, 2, (2, 4, 8), (1, 8), (1, 3), 1e-2, (96, 128)


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


def _fill(cache, dev):
    g = torch.Generator(device=dev)
    band = torch.linspace(0.0, 1.0, BANDS, device=dev)
    comps = torch.stack([torch.cos(np.pi * (k + 1) * band) for k in range(5)])
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    for k in range(BATCH):
        g.manual_seed(4321 + k)
        smooth = torch.stack([torch.sin(0.01 * (j + 1) * yy + 0.013 * (j + 2) * xx + k + j) for j in range(5)], dim=-1)
        amp = 0.08 * 0.6 ** torch.arange(5, device=dev)
        x = 0.3 + (smooth * amp) @ comps + 0.004 * torch.randn((H, W, BANDS), generator=g, device=dev)
        cache.put(k, x, (smooth[..., 0] > 0.5).to(torch.float32), name=f"cube{k}")
    torch.cuda.synchronize()


def _box(x, r):
    return F.avg_pool2d(x, 2 * r + 1, stride=1, padding=r, count_include_pad=False)


def composite(guide, maps, r, eps, prob=True):
    """The published algorithm out of torch operators: guide (N, K, h, w), maps (N, T, h, w)."""
    p = torch.sigmoid(maps) if prob else maps
    K = guide.shape[1]
    mI, mp = _box(guide, r), _box(p, r)
    cov = [_box(guide[:, a:a + 1] * p, r) - mI[:, a:a + 1] * mp for a in range(K)]                     # K x (N, T, h, w)
    var = {(a, b): _box(guide[:, a:a + 1] * guide[:, b:b + 1], r) - mI[:, a:a + 1] * mI[:, b:b + 1] for a in range(K) for b in range(a, K)}
    if K == 1:
        a = [cov[0] / (var[0, 0] + eps)]
    else:
        s00, s01, s02, s11, s12, s22 = var[0, 0] + eps, var[0, 1], var[0, 2], var[1, 1] + eps, var[1, 2], var[2, 2] + eps
        c00, c01, c02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
        c11, c12, c22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
        det = s00 * c00 + s01 * c01 + s02 * c02
        a = [(c00 * cov[0] + c01 * cov[1] + c02 * cov[2]) / det, (c01 * cov[0] + c11 * cov[1] + c12 * cov[2]) / det,
             (c02 * cov[0] + c12 * cov[1] + c22 * cov[2]) / det]
    b = mp - sum(a[k] * mI[:, k:k + 1] for k in range(K))
    q = sum(_box(a[k], r) * guide[:, k:k + 1] for k in range(K)) + _box(b, r)
    if not prob:
        return q
    q = q.clamp(2.0 ** -24, 1 - 2.0 ** -24)
    return torch.log(q) - torch.log1p(-q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="back-to-back calls per timed run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("guided_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
    from hyperpri_amd import _lib
    from hyperpri_amd import guided as G
    from hyperpri_amd import spectral as S
    from hyperpri_amd.cache import CubeCache
    from hyperpri_amd.engine import _p
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cache = CubeCache(BATCH, H, W, BANDS, device=dev)
    _fill(cache, dev)
    cs = cache.cs
    x = cache.batch(list(range(BATCH)))["image"]
    proj = S.SpectralProjection.pca(S.band_statistics(cache), 3).to(dev)
    pcs = proj(x)
    pcs = pcs[:, 0] if pcs.dim() == 5 else pcs                                          # (N, 3, h, w), channel stride 8
    guides = {K: pcs[:, :K] for K in GUIDES}
    plain = {K: guides[K].contiguous() for K in GUIDES}                                 # the composite reads NCHW
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    maps = {T: 2.0 * torch.randn((BATCH, T, H, W), generator=gen, device=dev) for T in MAPS}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = torch.tensor([[i, 0, 0, 0] for i in range(BATCH)], dtype=torch.int32).to(dev)
    dst = torch.empty((BATCH, H, W, cs), dtype=torch.float32, device=dev)
    legs = {"gather": lambda: _lib.call("hpri_cube_gather", _p(cache._cubes), 0, cache.capacity, H, W, cs, _p(table), BATCH, H, W, _p(dst), stream)}
    for K in GUIDES:
        for r in RADII:
            mod = G.GuidedFilter(r, EPS, "prob")
            for T in MAPS:
                legs[f"filter_K{K}_r{r}_T{T}"] = (lambda mod=mod, K=K, T=T: mod(guides[K], maps[T]))
                legs[f"composite_K{K}_r{r}_T{T}"] = (lambda K=K, r=r, T=T: composite(plain[K], maps[T], r, EPS))
    for fn in legs.values():
        _events_ms(fn, 1)
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(_events_ms(fn, args.calls))
    med = {k: statistics.median(v) for k, v in times.items()}
    # accuracy on a crop, before the logit: the filter and the composite against the fp64 restatement
    ch, cw = CROP
    errors = {}
    for K in GUIDES:
        base = plain[K][:1, :, :ch, :cw].contiguous()
        local = base - base.mean(dim=(2, 3), keepdim=True)
        shifted = 1000.0 + 0.01 * local / local.abs().max()
        pm = torch.sigmoid(maps[1][:1, :, :ch, :cw]).contiguous()
        for name, g in (("pca", base), ("pca_shifted_1000_scaled_0.01", shifted)):
            eps = EPS if name == "pca" else 1e-6
            ref = G.guided_reference(g.cpu().numpy(), pm.cpu().numpy(), 4, eps)["q"]
            ours = G.guided_filter(g, pm, 4, eps).cpu().numpy().astype(np.float64)
            theirs = composite(g, pm, 4, eps, prob=False).cpu().numpy().astype(np.float64)
            errors[f"{name}_K{K}"] = {"filter_max_abs_error": float(np.abs(ours - ref).max()), "composite_max_abs_error": float(np.abs(theirs - ref).max()),
                                      "guide_mean": float(g.mean()), "guide_std": float(g.std()), "radius": 4, "eps": eps}
    pixels = BATCH * H * W
    rep = {"device": torch.cuda.get_device_name(dev), "batch": [BATCH, BANDS, H, W], "guide_channel_stride": 8, "pixels": pixels, "eps": EPS,
           "domain": "prob", "rounds": args.rounds, "calls_per_round": args.calls, "ms": {k: _spread(v) for k, v in times.items()},
           "speedup_over_composite": {k[len("filter_"):]: med["composite_" + k[len("filter_"):]] / v for k, v in med.items() if k.startswith("filter_")},
           "gather_bytes": pixels * cs * 8, "gather_TBps": pixels * cs * 8 / med["gather"] / 1e9,
           "error_on_a_crop_before_the_logit": errors}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({"out": args.out, "ms": med, "errors": errors}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
