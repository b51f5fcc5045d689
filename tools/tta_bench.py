#!/usr/bin/env python3
"""Test-time augmentation: what the merge kernel costs, against the torch composite a user would write without it, and its share
of a whole TTA prediction of one batch.  Needs an MI355X; writes profiles/tta_merge.json.

    python tools/tta_bench.py                       # both steps, each a child process under its own time limit
    python tools/tta_bench.py --step merge          # one step in this process (what the children run)

Step ``merge``: the benched frame, N = 2 at 608 x 968, K = 1 and K = 3, V = 4 (the default views) and V = 8, mean probability with
the spread map.  Two arms, interleaved round by round in one process: ``hpri_tta_merge`` (one launch) and the composite --
``rot90`` / ``flip`` back, ``sigmoid`` or ``softmax``, ``stack``, ``mean``, ``std`` (K = 1) or the argmax vote (K > 1), ``log``.
Device events around 20 launches, median and min .. max of 15 rounds, after a warm-up round of each arm.  The bytes a merge must
move ((V + 1) K + 1 planes of N h w floats) over the kernel's time is reported as an achieved rate, not as a share of peak.

Step ``share``: CubeNET-64 on two 238-band cubes served by ``CubeCache.epoch_views``: per view the gather and the forward, then the
merge, each between device events, in the same run (fp32, the default precision).  The share is merge / (gathers + forwards + merge).

The parent stops at the first step that fails or runs into its limit."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, H, W = 2, 608, 968
DEFAULT = ("id", "flip_w", "flip_h", "rot180")
ALL = ("id", "flip_h", "flip_w", "rot180", "rot90", "rot270", "transpose", "antitranspose")
LIMITS = {"merge": 420, "share": 420}          # seconds per child


def _stats(ms):
    return {"median_us": 1e3 * statistics.median(ms), "min_us": 1e3 * min(ms), "max_us": 1e3 * max(ms)}


def _composite(views_logits, views, K):
    import torch
    from hyperpri_amd.tta import FLT_MIN, invert_view
    back = [invert_view(x, v) for x, v in zip(views_logits, views)]
    if K == 1:
        p = torch.stack([torch.sigmoid(b) for b in back])
        pm = p.mean(0)
        out = torch.log(pm.clamp_min(FLT_MIN)) - torch.log((1 - pm).clamp_min(FLT_MIN))
        return out, p.std(0, unbiased=False)[:, 0]
    p = torch.stack([torch.softmax(b, 1) for b in back])
    out = torch.log(p.mean(0).clamp_min(FLT_MIN))
    votes = torch.stack([b.argmax(1) for b in back])
    return out, (votes != out.argmax(1)).float().mean(0)


def step_merge(rounds, launches):
    import torch
    import hyperpri_amd as Hp
    from hyperpri_amd.tta import view_shape
    dev = "cuda:0"
    results = []
    for K in (1, 3):
        for views in (DEFAULT, ALL):
            g = torch.Generator(device=dev)
            g.manual_seed(17 * K + len(views))
            xs = [4 * torch.randn((N, K, *view_shape(v, H, W)), device=dev, generator=g) for v in views]
            arms = {"kernel": lambda: Hp.tta_merge(xs, views, "prob", True), "composite": lambda: _composite(xs, views, K)}
            a, b = arms["kernel"](), arms["composite"]()
            agree = {"out_max_abs_diff": float((a[0] - b[0]).abs().max()), "spread_max_abs_diff": float((a[1] - b[1]).abs().max())}
            times = {k: [] for k in arms}
            for r in range(rounds + 1):                            # round 0 warms both arms up
                for name, fn in arms.items():
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    for _ in range(launches):
                        fn()
                    stop.record()
                    stop.synchronize()
                    if r:
                        times[name].append(start.elapsed_time(stop) / launches)
            row = {"N": N, "K": K, "h": H, "w": W, "V": len(views), "views": list(views), "mode": "prob", "spread": True,
                   "kernel": _stats(times["kernel"]), "composite": _stats(times["composite"]), **agree}
            nbytes = 4 * N * H * W * ((len(views) + 1) * K + 1)
            row["kernel_algorithmic_GBps"] = nbytes / (row["kernel"]["median_us"] * 1e-6) / 1e9
            spread = row["composite"]["max_us"] - row["composite"]["min_us"]
            row["kernel_not_slower"] = row["kernel"]["median_us"] <= row["composite"]["median_us"] + spread
            print(json.dumps(row), flush=True)
            results.append(row)
    return {"rounds": rounds, "launches_per_round": launches, "cases": results}


def step_share(rounds, launches):
    import torch
    import hyperpri_amd as Hp
    from hyperpri_amd.cache import CubeCache
    dev = "cuda:0"
    torch.manual_seed(3)
    net = Hp.CubeNET(238, 1, 64, bilinear=False).to(dev).eval()
    cache = CubeCache(N, H, W, 299, hsi_lo=25, hsi_hi=263, device=dev, out_slots=2)
    for i in range(N):
        cache.put(i, torch.rand((H, W, 299), device=dev), (torch.rand((H, W), device=dev) > 0.9).to(torch.uint8), f"cube{i}")
    out = []
    with torch.inference_mode():
        for views in (DEFAULT, ALL):
            per_round = []
            for r in range(rounds + 1):
                ev = lambda: torch.cuda.Event(enable_timing=True)    # noqa: E731
                marks = [ev()]
                marks[0].record()
                batch = next(iter(cache.epoch_views(N, views)))
                mask = batch["mask"].clone()
                logits = []
                for v in views:
                    image = batch["image_of"](v)
                    marks.append(ev()); marks[-1].record()
                    logits.append(net(image).float().contiguous())
                    marks.append(ev()); marks[-1].record()
                Hp.tta_merge(logits, views, "prob", True)
                marks.append(ev()); marks[-1].record()
                marks[-1].synchronize()
                del mask
                if r:
                    gaps = [marks[i].elapsed_time(marks[i + 1]) for i in range(len(marks) - 1)]
                    per_round.append({"gather_ms": sum(gaps[0:-1:2]), "forward_ms": sum(gaps[1:-1:2]), "merge_ms": gaps[-1]})
            med = {k: statistics.median(p[k] for p in per_round) for k in per_round[0]}
            total = sum(med.values())
            row = {"network": "CubeNET(238, 1, 64)", "precision": "fp32", "N": N, "h": H, "w": W, "V": len(views), "views": list(views),
                   "rounds": len(per_round), **med, "total_ms": total, "merge_share": med["merge_ms"] / total}
            print(json.dumps(row), flush=True)
            out.append(row)
    return {"cases": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("merge", "share"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_merge.json"))
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            sys.exit("tta_bench: no GPU; this tool measures on an MI355X only")
        res = step_merge(args.rounds, args.launches) if args.step == "merge" else step_share(min(args.rounds, 5), args.launches)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f)
        return 0
    result = {"tool": "tools/tta_bench.py", "device": "MI355X"}
    with tempfile.TemporaryDirectory() as tmp:
        for step in ("merge", "share"):
            part = os.path.join(tmp, step + ".json")
            cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--rounds", str(args.rounds),
                   "--launches", str(args.launches), "--json", part]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(f"tta_bench: step {step} ended with status {rc}; nothing further is started", file=sys.stderr)
                return rc
            result[step] = json.load(open(part))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
