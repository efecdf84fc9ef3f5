#!/bin/bash
# Host side of the full BA under AddressSanitizer + UndefinedBehaviorSanitizer, as two stand-alone programs run on the CPU:
#   tests/cpp/full_ba_host_check.cpp  with sanitized host code of csrc/full_ba.hip and misc.cpp: what ba_solve does before and
#                                     without a launch (refusals, conversions, the solves that run no iteration)
#   tests/cpp/full_ba_glue.cpp        the reference-signature glue over mock objects with a recording solver
# The kernels are compiled as always; nothing here is loaded into Python.  Meant for a box without a GPU: no device is needed or used.
# Usage: tools/full_ba_sanitize.sh [output directory]
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function -Wno-unused-variable"
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -Xarch_host -fno-omit-frame-pointer"
$HIPCC $FLAGS $SAN -c "$ROOT/multi_orbslam3_amd/csrc/full_ba.hip" -o "$OUT/full_ba.o"
$HIPCC $FLAGS $SAN -x hip -c "$ROOT/multi_orbslam3_amd/csrc/misc.cpp" -o "$OUT/misc.o"
$HIPCC $FLAGS $SAN -x hip -I "$ROOT/include" -c "$ROOT/tests/cpp/full_ba_host_check.cpp" -o "$OUT/check.o"
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined "$OUT/full_ba.o" "$OUT/misc.o" "$OUT/check.o" -o "$OUT/full_ba_host_check"
"$OUT/full_ba_host_check"
$HIPCC $FLAGS $SAN -x hip -I "$ROOT/include" -I "$ROOT/tests/cpp" -c "$ROOT/tests/cpp/full_ba_glue.cpp" -o "$OUT/glue.o"
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined "$OUT/glue.o" "$OUT/misc.o" -o "$OUT/full_ba_glue"
"$OUT/full_ba_glue"
