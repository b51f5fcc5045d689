#!/usr/bin/env python3
"""Trainable dense CRF (hyperpri_amd/crf.py: crf_layer): what a forward plus a backward through the mean-field iterations costs on the card.

    python tools/crf_train_bench.py                    # one MI355X; writes profiles/crf_train.json
    python tools/crf_train_bench.py --rounds 5 --out FILE

tools/crf_bench.py's method and data (two 608 x 968 maps, a guide with a channel stride of 8, T = 5, r = 2, 4, 8), (C, K) = (2, 1)
(binary logits), (2, 3), (4, 3); device events, every leg warmed up, the legs interleaved round by round, medians with min and max:
``dense`` -- ``DenseCRF``; ``train_forward`` -- ``crf_layer``'s forward keeping its stack; ``step`` -- that forward plus the backward to
the unaries, w_a and w_s; ``composite_step`` -- crf_bench's ``unfold`` composite under ``torch.autograd``, up to ``--composite-radius``.
Reported: the backward (``step`` minus ``train_forward``) over ``dense``, in the same run and against the ``DenseCRF`` time
profiles/crf.json records for the commit before; ``train_forward`` over ``dense``; ``composite_step`` over ``step``; dU, dw_a and dw_s
against ``crf_backward_reference`` on a 64 x 96 crop.  Nothing is gated: the numbers are recorded."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from crf_bench import BATCH, CROP, H, PARAMS, RADII, T, W, _events_ms, _spread, composite  # noqa: E402

CASES = ((2, 1), (2, 3), (4, 3))                   # (C, K)
TH = {k: v for k, v in PARAMS.items() if k.startswith("theta")}


def _rounded(o):
    """The report with its floats at five significant digits (a timing has no more)."""
    if isinstance(o, float):
        return float(f"{o:.5g}")
    if isinstance(o, dict):
        return {k: _rounded(v) for k, v in o.items()}
    return [_rounded(v) for v in o] if isinstance(o, (list, tuple)) else o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crf_train.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="back-to-back calls per timed run")
    ap.add_argument("--composite-radius", type=int, default=4, help="largest radius the composite is timed at (it keeps every unfolded copy)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("crf_train_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
    from hyperpri_amd import crf
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(77)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    wide = torch.full((BATCH, H, W, 8), float("nan"), device=dev)
    for k in range(3):
        wide[..., k] = torch.sin(0.02 * (k + 1) * yy + 0.015 * (k + 2) * xx + k)[None] + 0.3 * torch.randn((BATCH, H, W), generator=gen, device=dev)
    guides = {K: wide.permute(0, 3, 1, 2)[:, :K] for K in (1, 3)}
    plain = {K: guides[K].contiguous() for K in (1, 3)}
    unaries = {2: 2.0 * torch.randn((BATCH, H, W), generator=gen, device=dev), 4: 2.0 * torch.randn((BATCH, 4, H, W), generator=gen, device=dev)}
    grads = {C: torch.randn(tuple(u.shape), generator=gen, device=dev) for C, u in unaries.items()}
    two = torch.stack([torch.zeros_like(unaries[2]), unaries[2]], dim=1)
    two_grad = torch.stack([-grads[2], grads[2]], dim=1)

    w_dev = (torch.tensor(PARAMS["w_appearance"], device=dev, requires_grad=True), torch.tensor(PARAMS["w_smooth"], device=dev, requires_grad=True))

    def weights():                                  # made once: a step uploads nothing
        for t in w_dev:
            t.grad = None
        return w_dev

    def step(C, K, r):
        u = unaries[C].detach().requires_grad_()
        wa, ws = weights()
        crf.crf_layer(u, guides[K], wa, ws, None, r, T, **TH).backward(grads[C])

    def composite_step(C, K, r):
        u = (two if C == 2 else unaries[4]).detach().requires_grad_()
        wa, ws = weights()
        composite(u, plain[K], r, T, w_appearance=wa, w_smooth=ws, **TH).backward(two_grad if C == 2 else grads[4])

    legs = {}
    for C, K in CASES:
        for r in RADII:
            key = f"C{C}_K{K}_r{r}"
            mod = crf.DenseCRF(r, T, **PARAMS)
            legs[f"dense_{key}"] = (lambda mod=mod, C=C, K=K: mod(unaries[C], guides[K]))
            legs[f"train_forward_{key}"] = (lambda C=C, K=K, r=r: crf.crf_layer(unaries[C], guides[K], *weights(), None, r, T, **TH))
            legs[f"step_{key}"] = (lambda C=C, K=K, r=r: step(C, K, r))
            if r <= args.composite_radius:
                legs[f"composite_step_{key}"] = (lambda C=C, K=K, r=r: composite_step(C, K, r))
    for fn in legs.values():
        _events_ms(fn, 1)
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(_events_ms(fn, 1 if k.startswith("composite") else args.calls))
    med = {k: statistics.median(v) for k, v in times.items()}
    parent = {}
    try:
        with open(os.path.join(ROOT, "profiles", "crf.json")) as fh:
            parent = {k[4:-3]: v["median"] for k, v in json.load(fh)["ms"].items() if k.startswith("crf_") and k.endswith(f"_T{T}")}
    except (OSError, KeyError, ValueError):
        pass
    ratios = {}
    for C, K in CASES:
        for r in RADII:
            key = f"C{C}_K{K}_r{r}"
            back = med[f"step_{key}"] - med[f"train_forward_{key}"]
            ratios[key] = {"backward_ms": back, "backward_over_forward": back / med[f"dense_{key}"],
                           "backward_over_recorded_parent_forward": back / parent[key] if key in parent else None,
                           "train_forward_over_dense": med[f"train_forward_{key}"] / med[f"dense_{key}"],
                           "composite_step_over_step": med[f"composite_step_{key}"] / med[f"step_{key}"] if f"composite_step_{key}" in med else None}
    # accuracy on a crop: against the fp64 restatement of the backward
    ch, cw = CROP
    g3 = plain[3][:1, :, :ch, :cw].contiguous()
    u0, go = unaries[4][:1, :, :ch, :cw].contiguous(), grads[4][:1, :, :ch, :cw].contiguous()
    ref = crf.crf_backward_reference(u0.cpu().numpy(), g3.cpu().numpy(), go.cpu().numpy(), 4, T, **PARAMS)
    u = u0.detach().requires_grad_()
    wa, ws = weights()
    crf.crf_layer(u, g3, wa, ws, None, 4, T, **TH).backward(go)
    errors = {"crf_layer": {"dU_max_abs_error": float(np.abs(u.grad.cpu().numpy().astype(np.float64) - ref["unary"]).max()),
                            "dw_s_abs_error": abs(float(ws.grad) - ref["w_smooth"]), "dw_a_abs_error": abs(float(wa.grad) - ref["w_appearance"])}}
    errors["reference"] = {"dU_max_abs": float(np.abs(ref["unary"]).max()), "dw_s": ref["w_smooth"], "dw_a": ref["w_appearance"]}
    rep = {"device": torch.cuda.get_device_name(dev), "maps": [BATCH, H, W], "guide_channel_stride": 8, "iterations": T, "parameters": PARAMS,
           "rounds": args.rounds, "calls_per_round": args.calls, "warm_up": "every leg once before the timed rounds", "timer": "device events",
           "clock_state": "not read", "ms": {k: _spread(v) for k, v in times.items()}, "recorded_parent_dense_ms": parent, "ratios": ratios,
           "error_on_a_crop": errors}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(_rounded(rep), fh)
    print(json.dumps({"out": args.out, "ms": med, "ratios": ratios, "errors": errors}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
