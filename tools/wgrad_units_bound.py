#!/usr/bin/env python3
"""conv_wino_wgrad_kernel alone, on two launches of the fp32 step, in up to three builds of csrc/conv_wino.hip
(tools/build_wgrad_diag.sh): plain (what the product library runs), diag (-DWGRAD_DIAG_NO_UNIT_LOAD: no loads inside the unit loop --
results meaningless, the time is what is left when the unit boundary costs nothing: the MOST any change to the boundary can give)
and, if present, plain_src (the same file of another tree).  Each launch alone, HIP events over back-to-back launches after
``SETTLE`` seconds of the same launches (as tools/first_conv.py times its layer).  Prints one JSON object.

usage: wgrad_units_bound.py [reps]"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

LIBDIR = os.path.join(ROOT, "hyperpri_amd", "lib")
SHAPES = [(2, 608, 968, 64, 64), (2, 76, 121, 512, 512)]          # (N, H, W, Cin, Cout)


def _open(name):
    path = os.path.join(LIBDIR, name)
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    V, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.hpri_conv_wino_wgrad.argtypes = [V, I, I, I, V, I, I, I, V, Z, I, I, I, I, I, V]
    lib.hpri_conv_wino_wgrad.restype = I
    lib.hpri_wino_wgrad_plan.argtypes = [I, I, I, I, I, ctypes.POINTER(I), ctypes.POINTER(I), ctypes.POINTER(I)]
    return lib


def _time(call, reps, settle_s):
    for _ in range(3):
        assert call() == 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < settle_s:
        for _ in range(50):
            call()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(3):                                  # three timed bursts: their spread is the noise of the figure
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    settle = float(os.environ.get("SETTLE", "1.0"))
    libs = {k: _open(f) for k, f in (("plain", "libwgradplain.so"), ("diag_no_unit_load", "libwgraddiag.so"),
                                     ("plain_src", "libwgradplain_src.so"))}
    libs = {k: v for k, v in libs.items() if v is not None}
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"reps": reps, "settle_s": settle, "launches": []}
    for N, H, W, cin, cout in SHAPES:
        torch.manual_seed(W)
        x = torch.rand(N * H * W, cin, device=dev)              # post-ReLU-like activations, gradient-like dY
        dy = torch.randn(N * H * W, cout, device=dev) * 1e-3
        row = {"shape": {"N": N, "H": H, "W": W, "Cin": cin, "Cout": cout}, "ms": {}}
        for _round in range(2):                                 # plain, diag, plain, diag: a drift of the box would show
            for kind, lib in libs.items():
                sp, cr, nr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
                lib.hpri_wino_wgrad_plan(N, H, W, cin, cout, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr))
                ws = torch.empty(sp.value * 16 * cr.value * nr.value, device=dev)
                call = lambda: lib.hpri_conv_wino_wgrad(x.data_ptr(), cin, 0, cin, dy.data_ptr(), cout, 0, cout, ws.data_ptr(),
                                                        ws.numel(), N, H, W, cin, cout, st)
                row["ms"].setdefault(kind, []).extend(round(t, 4) for t in _time(call, reps, settle))
                row["splits"] = sp.value
                del ws
        mean = {k: sum(v) / len(v) for k, v in row["ms"].items()}
        row["mean_ms"] = {k: round(v, 4) for k, v in mean.items()}
        if "diag_no_unit_load" in mean:
            row["upper_bound_ms"] = round(mean["plain"] - mean["diag_no_unit_load"], 4)
            row["upper_bound_fraction"] = round(1.0 - mean["diag_no_unit_load"] / mean["plain"], 4)
        res["launches"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
