#!/usr/bin/env python3
"""BASELINE config C2 (CubeNET-64, 238 bands, 608x968, batch 2) training step in the f16 mode, nn.BCEWithLogitsLoss + FusedAdam:
    explicit_static    set_precision(net, "f16"), engine.F16_LOSS_SCALE = "static" (the host-picked scale of earlier versions)
    explicit           set_precision(net, "f16") (the loss scale picked on the device: two small launches per step)
    torch_amp          set_precision(net, "torch") under torch.autocast("cuda", torch.float16) with torch.amp.GradScaler("cuda")
ms per step from CUDA events around --steps steps after --warmup.   usage: amp_step_bench.py [--steps K] [--warmup W] [--out f.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def leg(name, steps, warmup):
    import hyperpri_amd as H
    from hyperpri_amd import engine as E
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = H.CubeNET(238, 1, first_depth=64, bilinear=False).to(dev).train()
    H.set_precision(net, "torch" if name == "torch_amp" else "f16")
    x = E.synth_fill_(torch.empty(2, 1, 238, 608, 968, device=dev), 1235)
    m = (E.synth_fill_(torch.empty(2, 1, 608, 968, device=dev), 4321) > 0.9).float()
    opt = H.FusedAdam(net.parameters(), lr=1e-4)
    crit = torch.nn.BCEWithLogitsLoss()
    scaler = torch.amp.GradScaler("cuda") if name == "torch_amp" else None
    old = E.F16_LOSS_SCALE
    E.F16_LOSS_SCALE = "static" if name == "explicit_static" else "adaptive"

    def step():
        for p in net.parameters():
            p.grad = None
        if scaler is None:
            crit(net(x), m).backward()
            opt.step()
            return
        with torch.autocast("cuda", torch.float16):
            loss = crit(net(x), m)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()

    try:
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            step()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / steps
    finally:
        E.F16_LOSS_SCALE = old
    res = {"ms_per_step": round(ms, 2), "cubes_per_s": round(2 * 1000 / ms, 1)}
    if scaler is not None:
        res["grad_scaler_scale_after"] = scaler.get_scale()
    del net, x, m, opt
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    for name in ("explicit_static", "explicit", "torch_amp"):
        res[name] = leg(name, a.steps, a.warmup)
        print(name, res[name], flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
