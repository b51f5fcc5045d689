#!/usr/bin/env python3
"""Deforming gather of the cube cache (csrc/cache_warp.hip, csrc/cache_deform.hip): what the elastic field, the noise and CutMix cost beside the warp kernel.

    python tools/cube_deform_bench.py                  # one MI355X; writes profiles/cube_deform.json
    python tools/cube_deform_bench.py --out FILE --rounds 15 --calls 20
    python tools/cube_deform_bench.py --only noise --store fp32 --rounds 1 --calls 3 --out FILE      # one arm alone, e.g. under
                                                                                                     # rocprofv3 --pmc

The benched batch of tools/cube_cache_bench.py -- 2 x 238 of 299 bands x 608 x 968, the whole frame as the window -- from fp32 and
fp16 slots.  Every arm resamples through the same map, a 10 degree rotation at zoom 1.1 about the frame's centre, and the arms are
interleaved round by round in one process:
    warp_rot10         the unchanged ``hpri_cube_warp`` (the yardstick)
    deform_neutral     ``hpri_cube_deform`` with neutral deform entries and a null field
    elastic            a lattice at pitch 64 with sigma 8 pixels per sample, the field built beforehand (launch not counted)
    elastic+field      the same with the ``hpri_elastic_field`` launch inside the timed run
    noise              sigma 0.05 per sample, no field
    cutmix             each sample takes a half-height, half-width rectangle from the other one, no field
    all                field launch, elastic, noise and CutMix together
The method is cube_cache_bench's: device events around runs of ``--calls`` back-to-back launches after a warm-up, the median over
``--rounds`` with the spread.  Per arm: ms, TB/s of bytes WRITTEN (the same 1.13 GB in every arm), the ratio to the warp arm and
the share of the cache-fed training steps DESIGN.md reports (31.3 ms fp32, 9.5 ms bf16).  The mask kernels of the first and the
last arm are timed and listed separately.  Nothing is gated."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
from cube_cache_bench import BANDS, BATCH, H, SRC_BANDS, W, _events_ms, _fill_cache  # noqa: E402

STEP_MS = {"fp32": 31.3, "bf16": 9.5}       # the cache-fed steps of DESIGN.md (profiles/cube_cache.json)
ARMS = ["warp_rot10", "deform_neutral", "elastic", "elastic+field", "noise", "cutmix", "all"]
PITCH, SIGMA_PX, NOISE = 64.0, 8.0, 0.05


def measure(dev, rounds, calls, stores, only):
    from hyperpri_amd import _lib
    from hyperpri_amd.cache import CubeCache, deform_entries, elastic_lattice, warp_entries
    from hyperpri_amd.engine import _p
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    n = BATCH
    gy, gx = elastic_lattice(H, W, PITCH)
    cell = 2 * gy * gx
    g = torch.Generator()
    g.manual_seed(5)
    nodes = (torch.randn(n, gy, gx, 2, dtype=torch.float64, generator=g) * SIGMA_PX).to(torch.float32).reshape(-1).to(dev)
    entries = warp_entries(list(range(n)), [0] * n, [0] * n, [0] * n, [0] * n, (H, W), [10.0] * n, [1.1] * n, [0.0] * n, [0.0] * n,
                           [1.0] * n, [0.0] * n, [0] * n, [0] * n).to(dev)

    def rows(elastic=False, noise=False, cutmix=False):
        partner = [(j - 1) % n if cutmix else -1 for j in range(n)]
        rect = (H // 4, H // 4 + H // 2, W // 4, W // 4 + W // 2) if cutmix else (0, 0, 0, 0)
        return deform_entries(partner, [rect[0]] * n, [rect[1]] * n, [rect[2]] * n, [rect[3]] * n,
                              [j * cell if elastic else -1 for j in range(n)], [gy if elastic else 0] * n, [gx if elastic else 0] * n,
                              [1 / PITCH if elastic else 0.0] * n, [NOISE if noise else 0.0] * n, [1234 + j for j in range(n)],
                              [99 + j for j in range(n)]).to(dev)
    tables = {"deform_neutral": rows(), "elastic": rows(elastic=True), "noise": rows(noise=True), "cutmix": rows(cutmix=True),
              "all": rows(True, True, True)}
    tables["elastic+field"] = tables["elastic"]
    out = []
    for store in stores:
        sname = "fp32" if store == torch.float32 else "fp16"
        dt = 0 if store == torch.float32 else 1
        c = CubeCache(n, H, W, SRC_BANDS, hsi_lo=0, hsi_hi=BANDS, device=dev, store_dtype=store, out_slots=1)
        _fill_cache(c, n, dev, (H, W))
        cs = c.cs
        elems = n * H * W * cs
        dst = torch.empty((n, H, W, cs), dtype=torch.float32, device=dev)
        mdst = torch.empty((n, 1, H, W), dtype=torch.float32, device=dev)
        field = torch.empty((n, H, W, 2), dtype=torch.float32, device=dev)

        def build_field(t):
            _lib.call("hpri_elastic_field", _p(nodes), nodes.numel(), _p(t), n, H, W, _p(field), stream)

        def cube(t, f):
            _lib.call("hpri_cube_deform", _p(c._cubes), dt, c.capacity, H, W, cs, c.C, _p(entries), _p(t), f, n, H, W, _p(dst), stream)
        build_field(tables["elastic"])                     # (both lattice tables describe the same field)
        fns = {"warp_rot10": lambda: _lib.call("hpri_cube_warp", _p(c._cubes), dt, c.capacity, H, W, cs, c.C, _p(entries), n, H, W, _p(dst), stream)}
        for name in ("deform_neutral", "noise", "cutmix"):
            fns[name] = lambda t=tables[name]: cube(t, null)
        fns["elastic"] = lambda t=tables["elastic"]: cube(t, _p(field))
        fns["elastic+field"] = lambda t=tables["elastic"]: (build_field(t), cube(t, _p(field)))
        fns["all"] = lambda t=tables["all"]: (build_field(t), cube(t, _p(field)))
        fns = {k: v for k, v in fns.items() if not only or k in only}
        mfns = {"warp_rot10": lambda: _lib.call("hpri_mask_warp", _p(c._masks), c.capacity, H, W, _p(entries), n, H, W, _p(mdst), stream),
                "all": lambda t=tables["all"]: _lib.call("hpri_mask_deform", _p(c._masks), c.capacity, H, W, _p(entries), _p(t), _p(field), n, H, W,
                                                         _p(mdst), stream),
                "field_alone": lambda t=tables["elastic"]: build_field(t)}
        for fn in list(fns.values()) + list(mfns.values()):            # warm-up: code objects, clocks
            _events_ms(fn, calls)
        t = {name: [] for name in fns}
        for _ in range(rounds):                                         # interleaved: the same seconds of the same box
            for name, fn in fns.items():
                t[name].append(_events_ms(fn, calls))
        tm = {name: statistics.median(_events_ms(fn, calls) for _ in range(3)) for name, fn in mfns.items()}
        base = statistics.median(t["warp_rot10"]) if "warp_rot10" in t else None
        for name in fns:
            med = statistics.median(t[name])
            row = {"arm": name, "store": sname, "window": [H, W], "bytes_written": elems * 4,
                   "ms": {"median": med, "min": min(t[name]), "max": max(t[name])}, "written_TBps": elems * 4 / med / 1e9,
                   "ratio_to_warp": med / base if base else None, "extra_ms_over_warp": med - base if base else None,
                   "share_of_step": {k: med / v for k, v in STEP_MS.items()}, "rounds": rounds, "calls_per_round": calls}
            print(f"{sname} {name:15s} {med:.4f} ms  {row['written_TBps']:.2f} TB/s written  ratio "
                  f"{row['ratio_to_warp'] if base else float('nan'):.3f}", file=sys.stderr)
            out.append(row)
        out.append({"arm": "masks_and_field", "store": sname, "ms": tm})
        print(f"{sname} mask warp {tm['warp_rot10']:.4f} ms, mask deform {tm['all']:.4f} ms, field alone {tm['field_alone']:.4f} ms", file=sys.stderr)
        del c, dst, mdst, field, fns, mfns
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cube_deform.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back launches per timed run")
    ap.add_argument("--store", choices=["fp32", "fp16", "both"], default="both")
    ap.add_argument("--only", action="append", choices=ARMS, help="run only this arm (repeatable); ratios need warp_rot10 among them")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cube_deform_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stores = {"fp32": [torch.float32], "fp16": [torch.float16], "both": [torch.float32, torch.float16]}[args.store]
    rep = {"device": torch.cuda.get_device_name(dev), "batch": [BATCH, BANDS, H, W], "source_bands": SRC_BANDS, "step_ms": STEP_MS,
           "elastic": {"pitch": PITCH, "sigma_px": SIGMA_PX}, "noise_sigma": NOISE,
           "arms": measure(dev, args.rounds, args.calls, stores, args.only)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({"out": args.out, "worst_ratio": max((r.get("ratio_to_warp") or 0) for r in rep["arms"])}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
