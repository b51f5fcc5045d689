#!/usr/bin/env python3
"""Per-launch durations of conv_wino_wgrad_kernel from a rocprofv3 --kernel-trace run of bench.py, by position in the step.
The launches of a step come in a fixed order (the backward walks the layers from the head down), so position p of every step
is the same layer; the first `skip` steps (warm-up) are left out.  usage: wgrad_launch_trace.py <dir> <steps in trace> [skip]"""
import csv, glob, sys

d, steps = sys.argv[1], int(sys.argv[2])
skip = int(sys.argv[3]) if len(sys.argv) > 3 else 3
rows = []
for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
    rows += [r for r in csv.DictReader(open(f)) if r["Kernel_Name"].startswith("conv_wino_wgrad_kernel")]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
if not rows or len(rows) % steps:
    sys.exit(f"{len(rows)} launches do not divide into {steps} steps")
per = len(rows) // steps
print(f"conv_wino_wgrad_kernel: {len(rows)} launches, {per} per step, steps {skip + 1}..{steps} averaged")
print("pos  workgroups   avg us   min us   max us")
tot = 0.0
for p in range(per):
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows[p::per][skip:]]
    wgs = int(rows[p]["Grid_Size_X"]) // max(1, int(rows[p]["Workgroup_Size_X"]))
    tot += sum(us) / len(us)
    print(f"{p:3d}  {wgs:10d}  {sum(us) / len(us):7.1f}  {min(us):7.1f}  {max(us):7.1f}")
print(f"sum of the averages: {tot / 1e3:.3f} ms per step")
