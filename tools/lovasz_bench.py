#!/usr/bin/env python3
"""The Lovasz hinge (losses.LovaszHingeLoss, csrc/sort.hip) and the ranking metrics on the card, against torch.

    python tools/lovasz_bench.py                   # one MI355X; writes profiles/lovasz_hinge.json
    python tools/lovasz_bench.py --rounds 21 --calls 50 --out FILE

At (2, 1, 608, 968) -- a HyperPRI batch -- forward plus backward of ``LovaszHingeLoss()`` and of the torch composite of the published
code (``torch.sort``, gathers, cumulative sums, dot; autograd), on two sets of logits that bracket the share of pixels with a
positive hinge error: those of a UNet(3, 1) trained for a few steps on the batch, and random ones.  Device events over runs of
``--calls`` back-to-back steps, the two arms interleaved round by round, median and min .. max of ``--rounds`` rounds (at least 20)
after a warm-up round of each.  The kernel launches of one step of each arm, and the device time of the HIP arm's kernels by name,
are taken by the torch profiler in a run of its own (tracing slows the host).  The step-level cost is the HIP arm's median beside
the 29.8 ms fp32 step of CubeNET-64 on a batch of the same size (profiles/r05_bench.json).  The ranking metrics:
``ranking_metrics`` beside ``average_precision`` on a 15-image split (about 8.8 M scores), by a host clock around calls that end in
the read of their result.  Nothing is gated: the figures are recorded.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

N, H, W = 2, 608, 968
SPLIT_IMAGES = 15


def composite(x, y, per_image=True):
    """lovasz_hinge / lovasz_hinge_flat / lovasz_grad of the published code."""
    total = 0.0
    rows = x.shape[0] if per_image else 1
    for lg, lb in zip(x.reshape(rows, -1), y.reshape(rows, -1)):
        signs = 2.0 * lb - 1.0
        errors = 1.0 - lg * signs
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True)
        gt_sorted = lb[perm]
        gts = gt_sorted.sum()
        intersection = gts - gt_sorted.cumsum(0)
        union = gts + (1.0 - gt_sorted).cumsum(0)
        jaccard = 1.0 - intersection / union
        jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
        total = total + torch.dot(torch.relu(errors_sorted), jaccard.detach())
    return total / rows


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
    """(device kernels of one call, {kernel name: [calls, device microseconds]}) by the torch profiler; None where it reports no
    device activity."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    except Exception as exc:                                 # (a profiler without device tracing: recorded as not measured)
        return None, f"{type(exc).__name__}: {exc}"
    rows = [e for e in rows if not e.name.lower().startswith(("memcpy", "memset"))]
    by_name = {}
    for e in rows:
        name = e.name.split("(")[0]
        cur = by_name.setdefault(name, [0, 0.0])
        cur[0] += 1
        cur[1] += float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0) or 0.0)
    return (len(rows) if rows else None), by_name


def inputs(dev):
    """A drawn root mask (curved bands one to seven pixels thick) and an image that shows it under noise."""
    g = torch.Generator().manual_seed(7)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    y = torch.zeros((N, 1, H, W))
    for n in range(N):
        for k in range(9):
            centre = 60.0 * k + 40 * torch.sin(xx / (50.0 + 10 * k) + n) + 30
            y[n, 0] = torch.maximum(y[n, 0], ((yy - centre).abs() < 1 + (k % 4)).float())
    image = 0.5 * y.expand(N, 3, H, W) + 0.5 * torch.rand((N, 3, H, W), generator=g)
    random_logits = torch.randn((N, 1, H, W), generator=g)
    return image.to(dev), y.to(dev), random_logits.to(dev)


def trained_logits(image, y, steps):
    import hyperpri_amd as Hp
    torch.manual_seed(7)
    net = Hp.UNet(3, 1, bilinear=False).to(image.device).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    crit = Hp.BCEWithLogitsLoss()
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        crit(net(image), y).backward()
        opt.step()
    with torch.no_grad():
        return net(image).detach().contiguous()


def one(tag, x, y, rounds, calls):
    import hyperpri_amd as Hp
    crit = Hp.LovaszHingeLoss()

    def ours():
        xg = x.detach().requires_grad_(True)
        crit(xg, y).backward()
        return xg

    def torch_arm():
        xg = x.detach().requires_grad_(True)
        composite(xg, y).backward()
        return xg
    for fn in (ours, torch_arm):
        _events_ms(fn, 2)
    a, b = [], []
    for _ in range(rounds):
        a.append(_events_ms(ours, calls))
        b.append(_events_ms(torch_arm, calls))
    xo, xt = ours(), torch_arm()
    lo, lt = float(crit(x, y)), float(composite(x, y))
    share = float(((1.0 - x * (2.0 * y - 1.0)) > 0).float().mean())
    lo_n, lo_kernels = _launches(ours)
    lt_n, _ = _launches(torch_arm)
    row = {"logits": tag, "shape": [N, 1, H, W], "share_of_pixels_with_positive_error": share, "hip_ms": _spread(a),
           "torch_composite_ms": _spread(b), "speedup_median": statistics.median(b) / statistics.median(a), "hip_launches": lo_n,
           "torch_composite_launches": lt_n, "hip_kernels_calls_and_device_us": lo_kernels, "loss_hip": lo, "loss_torch": lt,
           "max_abs_gradient_difference": float((xo.grad - xt.grad).abs().max()), "max_abs_gradient": float(xt.grad.abs().max()),
           "rounds": rounds, "calls_per_round": calls}
    print(f"{tag}: e > 0 on {100 * share:.1f} %  hip {row['hip_ms']['median']:.3f} ms ({lo_n} launches)  torch composite "
          f"{row['torch_composite_ms']['median']:.3f} ms ({lt_n} launches)  x{row['speedup_median']:.2f}  loss {lo:.7f} / {lt:.7f}",
          file=sys.stderr)
    return row


def _host_ms(fn, rounds):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                                  # (ends in the read of its result: a device synchronise)
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def ranking(dev, rounds):
    import hyperpri_amd as Hp
    n = SPLIT_IMAGES * H * W
    g = torch.Generator().manual_seed(11)
    t = (torch.rand(n, generator=g) < 0.08).float()
    s = torch.sigmoid(torch.randn(n, generator=g) * 2 + (2 * t - 1) * 2).to(dev)
    t = t.to(dev)
    a = _host_ms(lambda: Hp.ranking_metrics(s, t), rounds)
    b = _host_ms(lambda: Hp.average_precision(s, t), rounds)
    got, ap = Hp.ranking_metrics(s, t), Hp.average_precision(s, t)
    row = {"scores": n, "distinct_scores": int(torch.unique(s).numel()), "ranking_metrics_ms": _spread(a), "average_precision_ms": _spread(b),
           "avg_prec": got["avg_prec"], "roc_auc": got["roc_auc"], "average_precision": ap, "rounds": rounds}
    print(f"ranking on {n} scores: ranking_metrics {row['ranking_metrics_ms']['median']:.2f} ms (AP and AUC)  average_precision "
          f"{row['average_precision_ms']['median']:.2f} ms (AP)  {got} / {ap}", file=sys.stderr)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lovasz_hinge.json"))
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--train-steps", type=int, default=30)
    ap.add_argument("--ranking-rounds", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lovasz_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
    if args.rounds < 20:
        sys.exit("lovasz_bench: at least 20 rounds")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    image, y, random_logits = inputs(dev)
    cases = [one("trained", trained_logits(image, y, args.train_steps), y, args.rounds, args.calls),
             one("random", random_logits, y, args.rounds, args.calls)]
    rep = {"device": torch.cuda.get_device_name(dev), "train_steps": args.train_steps, "cases": cases,
           "fp32_step_ms_r05_bench": 29.8, "ranking": ranking(dev, args.ranking_rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({"out": args.out, "speedup": {c["logits"]: c["speedup_median"] for c in cases}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
