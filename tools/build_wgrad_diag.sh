#!/bin/bash
# timing-only build of conv_wino.hip whose weight-gradient kernel issues no loads inside its unit loop
# (-DWGRAD_DIAG_NO_UNIT_LOAD: every unit multiplies the first unit's data): lib/libwgraddiag.so beside a plain build of the same
# file, lib/libwgradplain.so.  Outputs of the first are wrong by construction; only time matters (tools/wgrad_units_bound.py).
# SRC=<file> builds the plain library from another copy of conv_wino.hip (the parent's, say) as lib/libwgradplain_src.so.
set -e
cd "$(dirname "$0")/../hyperpri_amd/csrc"
F="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -I."
T=$(mktemp -d)
/opt/rocm/bin/hipcc $F -x hip -c api.cpp -o $T/api.o &
/opt/rocm/bin/hipcc $F -x hip -c conv_wino.hip -o $T/plain.o &
/opt/rocm/bin/hipcc $F -DWGRAD_DIAG_NO_UNIT_LOAD -x hip -c conv_wino.hip -o $T/diag.o &
if [ -n "$SRC" ]; then /opt/rocm/bin/hipcc $F -x hip -c "$SRC" -o $T/src.o & fi
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/libwgradplain.so $T/api.o $T/plain.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/libwgraddiag.so $T/api.o $T/diag.o
if [ -n "$SRC" ]; then /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/libwgradplain_src.so $T/api.o $T/src.o; fi
rm -r $T
echo built
