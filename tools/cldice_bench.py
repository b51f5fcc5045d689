#!/usr/bin/env python3
"""The centerline loss (trainer.clDiceLoss, csrc/skeleton.hip) on the card, against the torch composite of the published code.

    python tools/cldice_bench.py                   # one MI355X; writes profiles/cldice.json
    python tools/cldice_bench.py --iters 3 10 32 --out FILE

At (2, 1, 608, 968) -- a HyperPRI batch -- and for each ``iters``: forward plus backward of ``clDiceLoss(iters, alpha=1)`` (the
centerline term alone, so both arms compute the same thing) and of the composite below (``soft_skel`` of the paper's repository
with max_pool2d, the same ratios, torch autograd), by device events over runs of ``--calls`` back-to-back steps, the two arms
interleaved round by round, median and min .. max of ``--rounds`` rounds after a warm-up round of each.  The kernel launches of
one step of each arm are counted by the torch profiler in a run of its own (tracing slows the host); the bytes the forward keeps
for the backward come from the library's own size functions.  The two losses and the two gradients are compared at that size (the
arms differ by rounding, and where the prediction has exact ties by the subgradient taken).  Nothing is gated: the figures are
recorded.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

N, H, W = 2, 608, 968


def soft_erode(img):
    return torch.min(-F.max_pool2d(-img, (3, 1), (1, 1), (1, 0)), -F.max_pool2d(-img, (1, 3), (1, 1), (0, 1)))


def soft_open(img):
    return F.max_pool2d(soft_erode(img), (3, 3), (1, 1), (1, 1))


def soft_skel(img, iters):
    skel = F.relu(img - soft_open(img))
    for _ in range(iters):
        img = soft_erode(img)
        delta = F.relu(img - soft_open(img))
        skel = skel + F.relu(delta - skel * delta)
    return skel


def composite(x, y, iters, smooth=1.0):
    p = torch.sigmoid(x)
    sp, sy = soft_skel(p, iters), soft_skel(y, iters)
    tprec = ((sp * y).sum() + smooth) / (sp.sum() + smooth)
    tsens = ((sy * p).sum() + smooth) / (sy.sum() + smooth)
    return 1.0 - 2.0 * tprec * tsens / (tprec + tsens)


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


def _launches(fn):
    """Device kernels of one call, by the torch profiler; None where the profiler reports no device activity."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    except Exception as exc:                                 # (a profiler without device tracing: recorded as not measured)
        return None, f"{type(exc).__name__}: {exc}"
    kernels = [n for n in names if not n.lower().startswith(("memcpy", "memset"))]
    return (len(kernels) if kernels else None), sorted(set(kernels))[:40]


def inputs(dev):
    """A drawn root mask (curved bands one to seven pixels thick) and logits that mostly agree with it."""
    g = torch.Generator().manual_seed(7)
    x = torch.rand((N, 1, H, W), generator=g) * 2 - 1
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    y = torch.zeros((N, 1, H, W))
    for n in range(N):
        for k in range(9):
            centre = 60.0 * k + 40 * torch.sin(xx / (50.0 + 10 * k) + n) + 30
            y[n, 0] = torch.maximum(y[n, 0], ((yy - centre).abs() < 1 + (k % 4)).float())
    x = x + (2 * y - 1) * (1 + 5 * torch.rand((N, 1, H, W), generator=g))
    return x.to(dev), y.to(dev)


def one(iters, x, y, rounds, calls):
    import hyperpri_amd as Hp
    from hyperpri_amd import _lib
    crit = Hp.clDiceLoss(iters=iters, alpha=1.0)

    def ours():
        xg = x.detach().requires_grad_(True)
        crit(xg, y).backward()
        return xg

    def torch_arm():
        xg = x.detach().requires_grad_(True)
        composite(xg, y, iters).backward()
        return xg
    for fn in (ours, torch_arm):
        _events_ms(fn, 2)
    a, b = [], []
    for _ in range(rounds):
        a.append(_events_ms(ours, calls))
        b.append(_events_ms(torch_arm, calls))
    xo, xt = ours(), torch_arm()
    lo, lt = float(crit(x, y)), float(composite(x, y, iters))
    gdiff = float((xo.grad - xt.grad).abs().max())
    differing = int(((xo.grad - xt.grad).abs() > 1e-6 * xt.grad.abs().max()).sum())
    lib = _lib.load()
    kept = 4 * (lib.hpri_soft_skeleton_saved_floats(N, H, W, iters) + 2 * N * H * W)         # the saved planes, p and Sy
    lo_n, lo_names = _launches(ours)
    lt_n, _ = _launches(torch_arm)
    row = {"iters": iters, "shape": [N, 1, H, W], "hip_ms": _spread(a), "torch_composite_ms": _spread(b),
           "speedup_median": statistics.median(b) / statistics.median(a), "hip_launches": lo_n, "torch_composite_launches": lt_n,
           "hip_kernels": lo_names, "bytes_kept_for_backward": kept, "lds_bytes_forward": lib.hpri_soft_skeleton_lds_bytes(iters),
           "loss_hip": lo, "loss_torch": lt, "max_abs_gradient_difference": gdiff, "max_abs_gradient": float(xt.grad.abs().max()),
           "pixels_differing_beyond_1e-6_of_max": differing, "rounds": rounds, "calls_per_round": calls}
    print(f"iters {iters}: hip {row['hip_ms']['median']:.3f} ms ({lo_n} launches)  torch composite {row['torch_composite_ms']['median']:.3f} ms "
          f"({lt_n} launches)  x{row['speedup_median']:.1f}  kept {kept / 2 ** 20:.0f} MiB  loss {lo:.7f} / {lt:.7f}", file=sys.stderr)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cldice.json"))
    ap.add_argument("--iters", type=int, nargs="+", default=[3, 10])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cldice_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    x, y = inputs(dev)
    rep = {"device": torch.cuda.get_device_name(dev), "cases": [one(i, x, y, args.rounds, args.calls) for i in args.iters]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({"out": args.out, "speedup": {str(c["iters"]): c["speedup_median"] for c in rep["cases"]}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
