#!/usr/bin/env python3
"""The bf16-PLANE 3x3 convolution (conv_bf16v3.hip: two 4-wave workgroups per CU, 16x16x32 MFMA, stores from the accumulators) on the
CubeNET layer shapes: interleaved rounds in one process on the same random data (rule 24), with and (NOSTATS=1) without the BatchNorm
partial statistics; the statistics records are checked against the fp32 output they describe.
    usage: v3_bench.py [out.json]      env: SHAPES='[[N,H,W,Cin,Cout],...]'  DATA=randn|relu|uniform01|zeros  NOSTATS=1"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hyperpri_amd import _lib  # noqa: E402

SHAPES = json.loads(os.environ["SHAPES"]) if "SHAPES" in os.environ else [  # N, H, W, Cin, Cout
    (2, 608, 968, 238, 64), (2, 608, 968, 64, 64), (2, 608, 968, 128, 64), (2, 304, 484, 64, 128),
    (2, 304, 484, 128, 128), (2, 304, 484, 256, 128), (2, 152, 242, 256, 256), (2, 152, 242, 512, 256),
    (2, 76, 121, 512, 512), (2, 76, 121, 1024, 512), (2, 38, 60, 1024, 1024),
]


def rup(x, m):
    return (x + m - 1) // m * m


def chan_stats(stats, tiles, cout_pad, cout):
    s = stats.view(tiles, cout_pad, 4).double()
    n = s[:, :, 2]
    mean = (s[:, :, 0] * n).sum(0) / n.sum(0)
    m2 = (s[:, :, 1] + n * (s[:, :, 0] - mean) ** 2).sum(0)
    return mean[:cout], (m2 / n.sum(0))[:cout]


def main():
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    rows = []
    for (N, H, W, Cin, Cout) in SHAPES:
        cs16, cout_pad = rup(Cin, 32), rup(Cout, 64)
        planes = torch.zeros(N * H * W, cs16, dtype=torch.bfloat16, device=dev)
        data = os.environ.get("DATA", "randn")        # operand statistics move the clock the chip holds (DVFS): say which
        src = torch.randn(N * H * W, Cin, device=dev)
        if data == "relu":
            src = torch.relu(src)                      # what a 3x3 layer inside the networks reads: the output of BN + ReLU
        elif data == "uniform01":
            src = torch.rand(N * H * W, Cin, device=dev)   # the synthetic cube of the first layer: u in [0, 1)
        elif data == "zeros":
            src = torch.zeros(N * H * W, Cin, device=dev)
        planes[:, :Cin] = src.to(torch.bfloat16)
        del src
        w = torch.randn(Cout * Cin * 9, device=dev) * 0.05
        b = torch.randn(Cout, device=dev)
        flops = 2.0 * N * H * W * Cin * Cout * 9
        wpb = torch.empty(((Cin + 31) // 32) * 9 * cout_pad * 32, dtype=torch.bfloat16, device=dev)
        assert lib.hpri_pack_weight_bf16(P(w), P(wpb), 0, Cin, Cout, cout_pad, 9, Cin, 0, 0, st) == 0
        arms = {}
        k, tl, wsf = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        lib.hpri_conv_bf16v3_plan(N, H, W, cs16, cout_pad, ctypes.byref(k), ctypes.byref(tl), ctypes.byref(wsf))
        for kind in ["v3"] + (["v3nostats"] if os.environ.get("NOSTATS") else []):
            ws = torch.empty(max(wsf.value, 4), device=dev)
            stats = torch.zeros(tl.value * cout_pad * 4, device=dev)
            y = torch.zeros(N * H * W * Cout, device=dev)

            def call(y=y, stats=stats if kind == "v3" else None, ws=ws):
                return lib.hpri_conv_bf16v3(P(planes), 0, cs16, 0, P(wpb), P(b), P(y), Cout, 0, P(stats), N, H, W, cs16, Cout,
                                            cout_pad, Cout, 0, 0, P(ws), ws.numel(), st)
            arms[kind] = (call, y, stats)
        res = {k: [] for k in arms}
        for rnd in range(6):
            for kind, (fn, *_r) in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                reps = 5
                e0.record()
                for _ in range(reps):
                    rc = fn()
                    assert rc == 0, lib.hpri_last_error()
                e1.record()
                torch.cuda.synchronize()
                if rnd > 0:
                    res[kind].append(e0.elapsed_time(e1) / reps)
        y3 = arms["v3"][1].view(N * H * W, Cout).double()
        m3, v3 = chan_stats(arms["v3"][2], tl.value, cout_pad, Cout)
        med = {kd: sorted(v)[len(v) // 2] for kd, v in res.items()}
        row = {"shape": [N, H, W, Cin, Cout], "ms": med, "tf": {kd: flops / v / 1e9 for kd, v in med.items()}, "ksplit": k.value,
               "max_abs_y": float(y3.abs().max()), "max_dmean": float((m3 - y3.mean(0)).abs().max()),
               "max_dvar_rel": float(((v3 - y3.var(0, unbiased=False)).abs() / y3.var(0, unbiased=False)).max())}
        rows.append(row)
        print(f"N{N} {H}x{W} {Cin}->{Cout} (k{k.value}): " + "  ".join(f"{kd} {row['tf'][kd]:7.1f} TF ({med[kd]:.3f} ms)" for kd in med)
              + f"  max|y| {row['max_abs_y']:.1f}  statistics vs output: dmean {row['max_dmean']:.1e} dvar {row['max_dvar_rel']:.1e}", flush=True)
        del planes, arms, y3
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
