#!/bin/bash
# The reference-signature glue of the welding BA (orbgpu::dropin::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag))
# under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program run on the CPU: tests/cpp/weld_ba_glue.cpp over mock
# objects with a recording solver.  Nothing here is loaded into Python, and no device is needed or used.
# Usage: tools/weld_ba_sanitize.sh [output directory]
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function -Wno-unused-variable"
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -Xarch_host -fno-omit-frame-pointer"
$HIPCC $FLAGS $SAN -x hip -c "$ROOT/multi_orbslam3_amd/csrc/misc.cpp" -o "$OUT/misc.o"
$HIPCC $FLAGS $SAN -x hip -I "$ROOT/include" -I "$ROOT/tests/cpp" -c "$ROOT/tests/cpp/weld_ba_glue.cpp" -o "$OUT/glue.o"
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined "$OUT/glue.o" "$OUT/misc.o" -o "$OUT/weld_ba_glue"
"$OUT/weld_ba_glue"
