#!/usr/bin/env python3
"""Device-resident cube cache (hyperpri_amd/cache.py): what the batch gather costs, and what a training step costs fed from it.

    python tools/cube_cache_bench.py                 # one MI355X; writes profiles/cube_cache.json
    python tools/cube_cache_bench.py --out FILE --rounds 15 --no-steps

(a) the gather of the benched batch -- 2 x 238 of 299 bands x 608 x 968 -- from fp32 and fp16 slots: plain, each flip, both
    flips, cropped from a larger frame (with and without flips).  Its yardstick is a ``torch.Tensor.copy_`` that reads and
    writes the same number of bytes (fp32 slots: fp32 -> fp32; fp16 slots: a converting fp16 -> fp32 copy), measured in the
    same process, interleaved round by round.  Times are device events around runs of ``--calls`` back-to-back launches
    after a warm-up; the median over the rounds is reported with the spread, the bytes (computed from the shapes: slot
    bytes read + destination bytes written; the 0.4 % of the mask gather is timed and listed separately) and the rate.
    The gate: median gather <= 1.3 x median copy (6.29 TB/s float4 sweep against 5.5-5.8 TB/s whole-row gathers in
    MI355X_MICROARCH.md is 1.14; the rest covers index arithmetic and reversed pixel order).  Exit code 1 when a case misses.
(b) 22 training steps of BASELINE config C2 (CubeNET(238, 1, 64), batch 2, forward + loss + backward as bench.py) fed three
    ways -- one epoch over 44 cached cubes; ``CubeStager`` out of pinned host memory (the best path without the cache); one
    resident tensor as bench.py -- in fp32 and bf16, legs alternating, host clock around the 22 steps ending in a
    synchronise.  Reported, not gated.
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

import torch  # noqa: E402

H, W, BANDS, SRC_BANDS, BATCH = 608, 968, 238, 299, 2
BIG_H, BIG_W = 704, 1064                  # the larger frame the cropped cases cut their 608 x 968 window from
GATE = 1.3


def _events_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def _fill_cache(cache, n, dev, frame):
    from hyperpri_amd.engine import synth_fill_
    raw = torch.empty((*frame, SRC_BANDS), dtype=torch.float32, device=dev)
    m = torch.empty(frame, dtype=torch.float32, device=dev)
    for k in range(n):
        synth_fill_(raw, 1234 + k, mode=0)
        synth_fill_(m, 4321 + k, mode=1, thr=0.9)
        cache.put(k, raw, m, name=f"cube{k}")


def gather_matrix(dev, rounds, calls):
    from hyperpri_amd import _lib
    from hyperpri_amd.cache import CubeCache
    from hyperpri_amd.engine import _p
    cases = [("plain", (H, W), [(0, 0, 0, 0), (1, 0, 0, 0)]),
             ("flip_h", (H, W), [(0, 0, 0, 1), (1, 0, 0, 1)]),
             ("flip_w", (H, W), [(0, 0, 0, 2), (1, 0, 0, 2)]),
             ("flip_hw", (H, W), [(0, 0, 0, 3), (1, 0, 0, 3)]),
             ("crop", (BIG_H, BIG_W), [(0, 37, 51, 0), (1, 96, 0, 0)]),
             ("crop_flip_hw", (BIG_H, BIG_W), [(1, 0, 96, 3), (0, 59, 13, 3)])]
    out = []
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for store in (torch.float32, torch.float16):
        esz = 4 if store == torch.float32 else 2
        caches = {}
        for frame in ((H, W), (BIG_H, BIG_W)):
            c = CubeCache(BATCH, *frame, SRC_BANDS, hsi_lo=0, hsi_hi=BANDS, device=dev, store_dtype=store, out_slots=1)
            _fill_cache(c, BATCH, dev, frame)
            caches[frame] = c
        cs = caches[(H, W)].cs
        elems = BATCH * H * W * cs
        dst = torch.empty((BATCH, H, W, cs), dtype=torch.float32, device=dev)
        mdst = torch.empty((BATCH, 1, H, W), dtype=torch.float32, device=dev)
        copy_src = torch.empty(elems, dtype=store, device=dev).normal_()
        copy_dst = torch.empty(elems, dtype=torch.float32, device=dev)
        nbytes = elems * (esz + 4)
        for name, frame, rows in cases:
            c = caches[frame]
            table = torch.tensor(rows, dtype=torch.int32).to(dev)

            def gather():
                _lib.call("hpri_cube_gather", _p(c._cubes), 0 if store == torch.float32 else 1, c.capacity, c.H, c.W, cs,
                          _p(table), BATCH, H, W, _p(dst), stream)

            def mgather():
                _lib.call("hpri_mask_gather", _p(c._masks), c.capacity, c.H, c.W, _p(table), BATCH, H, W, _p(mdst), stream)

            def copy():
                copy_dst.copy_(copy_src)
            for fn in (gather, copy, mgather):                      # warm-up: code objects, clocks
                _events_ms(fn, calls)
            g, k, m = [], [], []
            for _ in range(rounds):                                 # interleaved: the same seconds of the same box
                g.append(_events_ms(gather, calls))
                k.append(_events_ms(copy, calls))
            for _ in range(3):
                m.append(_events_ms(mgather, calls))
            gm, km = statistics.median(g), statistics.median(k)
            row = {"case": name, "store": "fp32" if store == torch.float32 else "fp16", "frame": list(frame), "window": [H, W],
                   "bytes_read": elems * esz, "bytes_written": elems * 4,
                   "gather_ms": {"median": gm, "min": min(g), "max": max(g)}, "copy_ms": {"median": km, "min": min(k), "max": max(k)},
                   "gather_TBps": nbytes / gm / 1e9, "copy_TBps": nbytes / km / 1e9, "ratio": gm / km, "bound": GATE,
                   "within_bound": gm <= GATE * km, "mask_gather_ms": statistics.median(m), "rounds": rounds, "calls_per_round": calls}
            print(f"{row['store']} {name:13s} gather {gm:.4f} ms ({row['gather_TBps']:.2f} TB/s)  copy_ {km:.4f} ms "
                  f"({row['copy_TBps']:.2f} TB/s)  ratio {row['ratio']:.3f}  mask {row['mask_gather_ms']:.4f} ms", file=sys.stderr)
            out.append(row)
        del caches, dst, copy_src, copy_dst
        torch.cuda.empty_cache()
    return out


def step_legs(dev, rounds, steps=22):
    import hyperpri_amd as HP
    from bench import synth_init_
    from hyperpri_amd.cache import CubeCache
    from hyperpri_amd.engine import synth_fill_
    from hyperpri_amd.ingest import CubeStager
    n = steps * BATCH
    cache = CubeCache(n, H, W, SRC_BANDS, hsi_lo=0, hsi_hi=BANDS, device=dev)
    _fill_cache(cache, n, dev, (H, W))
    st = CubeStager(BATCH, H, W, SRC_BANDS, hsi_lo=0, hsi_hi=BANDS, device=dev)
    raw = torch.empty((BATCH, H, W, SRC_BANDS), dtype=torch.float32, device=dev)
    for i in range(BATCH):
        synth_fill_(raw[i], 1234 + i, mode=0)
    for k in range(st.slots):
        st.host_slot(k)[...] = raw.cpu().numpy()
    x_res = raw[..., :BANDS].permute(0, 3, 1, 2).unsqueeze(1).contiguous()          # (N,1,C,H,W) contiguous, as bench.py's input
    del raw
    mask = torch.empty((BATCH, 1, H, W), dtype=torch.float32, device=dev)
    for i in range(BATCH):
        synth_fill_(mask[i], 4321 + i, mode=1, thr=0.9)
    gen = torch.Generator()
    gen.manual_seed(0)
    result = {}
    for prec in ("fp32", "bf16"):
        net = HP.CubeNET(BANDS, 1, first_depth=64, bilinear=False).to(dev).train()
        synth_init_(net)
        HP.set_precision(net, prec)

        def one(x, m):
            for p in net.parameters():
                p.grad = None
            _, loss = HP.forward_loss(net, x, m)
            loss.backward()

        def leg_cache(k):
            for i, b in enumerate(cache.epoch(BATCH, shuffle=True, generator=gen)):
                if i >= k:
                    break
                one(b["image"], b["mask"])

        def leg_stager(k):
            for _ in range(k):
                one(st.submit(), mask)
                st.release()

        def leg_resident(k):
            for _ in range(k):
                one(x_res, mask)
        legs = {"cache": leg_cache, "stager_pinned": leg_stager, "resident": leg_resident}
        times = {name: [] for name in legs}
        for fn in legs.values():
            fn(3)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(steps)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / steps)
        result[prec] = {name: {"ms_per_step_median": statistics.median(v), "min": min(v), "max": max(v)} for name, v in times.items()}
        print(prec, json.dumps(result[prec]), file=sys.stderr)
        del net
    return {"steps": steps, "rounds": rounds, "batch": BATCH, "ms_per_step": result,
            "note": "forward + loss + backward of BASELINE C2, no optimizer; the stager leg resends a filled pinned slot every step "
                    "(no host-side cube loading in any leg)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cube_cache.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back launches per timed run")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--no-steps", action="store_true", help="skip (b), the three-way step timing")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cube_cache_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rep = {"device": torch.cuda.get_device_name(dev), "batch": [BATCH, BANDS, H, W], "source_bands": SRC_BANDS,
           "gather": gather_matrix(dev, args.rounds, args.calls)}
    rep["gather_ok"] = all(r["within_bound"] for r in rep["gather"])
    if not args.no_steps:
        rep["steps"] = step_legs(dev, args.step_rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({"out": args.out, "gather_ok": rep["gather_ok"],
                      "worst_ratio": max(r["ratio"] for r in rep["gather"])}))
    return 0 if rep["gather_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
