#!/usr/bin/env python3
"""Dense CRF (hyperpri_amd/crf.py): what refining a batch of score maps costs on the card, against an ``unfold`` composite in torch.

    python tools/crf_bench.py                    # one MI355X; writes profiles/crf.json
    python tools/crf_bench.py --rounds 5 --out FILE

Two 608 x 968 maps: binary logits and C = 4 unaries, a guide of K = 1 and K = 3 channels (channels-last with a stride of 8, the layout
``SpectralProjection`` hands out), r = 2, 4, 8, T = 5 iterations.  By device events over runs of ``--calls`` back-to-back calls after a
warm-up of every leg, the legs interleaved round by round, median with min and max:

* ``DenseCRF`` (T launches);
* a torch composite of the same contract on the same card: ``F.unfold`` of the guide and of Q, the kernel weights once, then per
  iteration a weighted sum over the (2r+1)^2 copies -- it materialises every copy and is run in row chunks so that it fits;
* per iteration: the T = 5 time minus the T = 1 time, over 4.

The instruction floor of an iteration counts, per pixel and neighbour, K subtractions, K fmaf, one product, the exponential as two
instructions (its scaling product and ``v_exp_f32``), one fmaf for k and C fmaf for M, every one at the plain vector issue rate of
256 CUs x 4 SIMDs x 32 lanes per cycle at the nominal 2.4 GHz; the achieved fraction is that floor over the measured time per
iteration.  The clock the card held is not read (no tool is asked for it): the floor names its nominal clock.  Accuracy: the largest
error of both routes against ``crf_reference`` on a 64 x 96 crop.  Nothing is gated: the numbers are recorded."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

H, W, BATCH, RADII, GUIDES, CLASSES, T, CROP = 608, 968, 2, (2, 4, 8), (1, 3), (2, 4), 5, (64, 96)
PARAMS = dict(theta_alpha=3.0, theta_beta=1.0, theta_gamma=1.5, w_appearance=4.0, w_smooth=1.0)
NOMINAL_HZ, LANES_PER_CYCLE = 2.4e9, 256 * 4 * 32


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


def composite(unary, guide, radius, iterations, theta_alpha, theta_beta, theta_gamma, w_appearance, w_smooth, rows=64):
    """The contract out of torch operators (Potts): unary (N, C, h, w), guide (N, K, h, w) -> the last L.  Row chunks of ``rows``."""
    from hyperpri_amd import crf
    N, C, h, w = unary.shape
    r, win = radius, 2 * radius + 1
    ta, tg, b = crf.crf_tables(r, theta_alpha, theta_beta, theta_gamma)
    d = torch.arange(-r, r + 1, device=unary.device).abs()
    ta, tg = torch.from_numpy(ta).to(unary.device), torch.from_numpy(tg).to(unary.device)
    ga = ((w_appearance * ta[d])[:, None] * ta[d][None, :]).reshape(1, 1, win * win, 1)
    gs_ = ((w_smooth * tg[d])[:, None] * tg[d][None, :]).reshape(1, 1, win * win, 1)
    centre = torch.ones(win * win, device=unary.device)
    centre[win * win // 2] = 0.0
    ones = torch.ones((1, 1, h, w), device=unary.device)
    cnt = (F.unfold(ones, win, padding=r).sum(dim=1) - 1.0).reshape(1, 1, h, w)
    q = torch.softmax(unary, dim=1)
    L = unary
    for _ in range(iterations):
        m = torch.empty_like(unary)
        for y0 in range(0, h, rows):
            y1 = min(h, y0 + rows)
            a0, a1 = max(0, y0 - r), min(h, y1 + r)
            pad = (r, r, r - (y0 - a0), r - (a1 - y1))
            gp, qp = F.pad(guide[:, :, a0:a1], pad), F.pad(q[:, :, a0:a1], pad)
            K = guide.shape[1]
            gu = F.unfold(gp, win).reshape(N, K, win * win, -1)
            s = ((gu - guide[:, :, y0:y1].reshape(N, K, 1, -1)) ** 2).sum(dim=1, keepdim=True)
            k = (ga * torch.exp(-(s * b)) + gs_) * centre.reshape(1, 1, -1, 1)
            qu = F.unfold(qp, win).reshape(N, C, win * win, -1)
            m[:, :, y0:y1] = (k * qu).sum(dim=2).reshape(N, C, y1 - y0, w)
        L = unary + torch.where(cnt > 0, m / cnt.clamp(min=1.0), torch.zeros_like(m))
        q = torch.softmax(L, dim=1)
    return L


def floor_ms(pixels, r, K, C):
    """The least time of one iteration if every vector instruction of the window loop issued at the plain rate (see the module's text)."""
    per_neighbour = 2 * K + 1 + 2 + 1 + C
    return pixels * ((2 * r + 1) ** 2 - 1) * per_neighbour / (LANES_PER_CYCLE * NOMINAL_HZ) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crf.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="back-to-back calls per timed run")
    ap.add_argument("--composite-radius", type=int, default=8, help="largest radius the composite is timed at")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("crf_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
    from hyperpri_amd import crf
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(77)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    wide = torch.full((BATCH, H, W, 8), float("nan"), device=dev)
    for k in range(3):
        wide[..., k] = torch.sin(0.02 * (k + 1) * yy + 0.015 * (k + 2) * xx + k)[None] + 0.3 * torch.randn((BATCH, H, W), generator=gen, device=dev)
    guides = {K: wide.permute(0, 3, 1, 2)[:, :K] for K in GUIDES}                       # zero-copy, channel stride 8
    plain = {K: guides[K].contiguous() for K in GUIDES}                                 # the composite reads NCHW
    unaries = {2: 2.0 * torch.randn((BATCH, H, W), generator=gen, device=dev), 4: 2.0 * torch.randn((BATCH, 4, H, W), generator=gen, device=dev)}
    two = torch.stack([torch.zeros_like(unaries[2]), unaries[2]], dim=1)
    legs = {}
    for C in CLASSES:
        for K in GUIDES:
            for r in RADII:
                key = f"C{C}_K{K}_r{r}"
                for it in (1, T):
                    mod = crf.DenseCRF(r, it, **PARAMS)
                    legs[f"crf_{key}_T{it}"] = (lambda mod=mod, C=C, K=K: mod(unaries[C], guides[K]))
                if r <= args.composite_radius:
                    u = two if C == 2 else unaries[4]
                    legs[f"composite_{key}_T{T}"] = (lambda u=u, K=K, r=r: composite(u, plain[K], r, T, **PARAMS))
    for fn in legs.values():
        _events_ms(fn, 1)
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(_events_ms(fn, args.calls if k.startswith("crf_") else 1))
    med = {k: statistics.median(v) for k, v in times.items()}
    pixels = BATCH * H * W
    per_iter, fraction, speedup = {}, {}, {}
    for C in CLASSES:
        for K in GUIDES:
            for r in RADII:
                key = f"C{C}_K{K}_r{r}"
                per_iter[key] = (med[f"crf_{key}_T{T}"] - med[f"crf_{key}_T1"]) / (T - 1)
                fraction[key] = floor_ms(pixels, r, K, C) / per_iter[key]
                if f"composite_{key}_T{T}" in med:
                    speedup[key] = med[f"composite_{key}_T{T}"] / med[f"crf_{key}_T{T}"]
    # accuracy on a crop: both routes against the fp64 restatement
    ch, cw = CROP
    errors = {}
    for K in GUIDES:
        g = plain[K][:1, :, :ch, :cw].contiguous()
        u = unaries[4][:1, :, :ch, :cw].contiguous()
        ref = crf.crf_reference(u.cpu().numpy(), g.cpu().numpy(), 4, T, **PARAMS)["L"]
        ours = crf.dense_crf(u, g, 4, T, **PARAMS).cpu().numpy().astype(np.float64)
        theirs = composite(u, g, 4, T, **PARAMS).cpu().numpy().astype(np.float64)
        errors[f"C4_K{K}_r4"] = {"crf_max_abs_error": float(np.abs(ours - ref).max()), "composite_max_abs_error": float(np.abs(theirs - ref).max())}
    rep = {"device": torch.cuda.get_device_name(dev), "maps": [BATCH, H, W], "guide_channel_stride": 8, "pixels": pixels, "iterations": T,
           "parameters": PARAMS, "rounds": args.rounds, "calls_per_round": args.calls, "warm_up": "every leg once before the timed rounds",
           "timer": "device events", "clock_state": "not read; the floor assumes the nominal 2.4 GHz", "tile": list(crf.tile_shape()),
           "workgroups_offered_per_cu": 2, "ms": {k: _spread(v) for k, v in times.items()}, "ms_per_iteration": per_iter,
           "instruction_floor_ms_per_iteration": {f"C{C}_K{K}_r{r}": floor_ms(pixels, r, K, C) for C in CLASSES for K in GUIDES for r in RADII},
           "fraction_of_instruction_floor": fraction, "speedup_over_composite": speedup, "error_on_a_crop": errors}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({"out": args.out, "ms": med, "fraction": fraction, "speedup": speedup, "errors": errors}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
