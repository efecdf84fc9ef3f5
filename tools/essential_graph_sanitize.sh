#!/bin/bash
# Host side of the essential graph under AddressSanitizer + UndefinedBehaviorSanitizer, as two stand-alone programs run on the CPU:
#   tests/cpp/essential_graph_host_check.cpp  with sanitized host code of csrc/essential_graph.hip and misc.cpp: what eg_solve does
#                                             before and without a launch (refusals, the cap, the problems answered on the host)
#   tests/cpp/essential_graph_glue.cpp        the reference-signature glue over mock objects with a recording solver, on a scene of
#                                             tests/essential_graph_model.py with a bad keyframe
# The kernels are compiled as always; nothing here is loaded into Python.  Meant for a box without a GPU: no device is needed or used.
# Usage: tools/essential_graph_sanitize.sh [output directory]
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function -Wno-unused-variable"
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -Xarch_host -fno-omit-frame-pointer"
$HIPCC $FLAGS $SAN -c "$ROOT/multi_orbslam3_amd/csrc/essential_graph.hip" -o "$OUT/essential_graph.o"
$HIPCC $FLAGS $SAN -x hip -c "$ROOT/multi_orbslam3_amd/csrc/misc.cpp" -o "$OUT/misc.o"
$HIPCC $FLAGS $SAN -x hip -I "$ROOT/include" -c "$ROOT/tests/cpp/essential_graph_host_check.cpp" -o "$OUT/check.o"
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined "$OUT/essential_graph.o" "$OUT/misc.o" "$OUT/check.o" -o "$OUT/essential_graph_host_check"
"$OUT/essential_graph_host_check"
g++ -std=c++17 -O1 -g -Wall -Wno-unused-function -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
    -I "$ROOT/include" -I "$ROOT/tests/cpp" "$ROOT/tests/cpp/essential_graph_glue.cpp" -o "$OUT/essential_graph_glue"
(cd "$ROOT/tests" && python3 -c "
import sys
sys.path.insert(0, '.')
import essential_graph_model as em
from test_essential_graph_glue import write_scene
write_scene(em.make_scene(14, False, 7, bad=(5,)), sys.argv[1])" "$OUT/scene.txt")
"$OUT/essential_graph_glue" "$OUT/scene.txt" | tail -n 2
