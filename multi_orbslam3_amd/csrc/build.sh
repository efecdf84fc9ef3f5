#!/bin/bash
# Builds multi_orbslam3_amd/liborbgpu.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="$HERE/../liborbgpu.so"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function"
mkdir -p "$HERE/obj"
pids=()
# an object is rebuilt when its source, any header / include file here, the public header or this script is newer than it
DEPS=("$HERE"/*.hpp "$HERE"/*.inc "$HERE/../../include/orbgpu.h" "$HERE/build.sh")
for f in extractor matcher lba full_ba essential_graph pose_opt pose_inertial inertial_ba inertial_init bow sim3 sim3_opt newpoints fuse two_view search_init mlpnp; do
  stale=0
  for d in "$HERE/$f.hip" "${DEPS[@]}"; do
    if [ "$d" -nt "$HERE/obj/$f.o" ]; then stale=1; break; fi
  done
  if [ ! -f "$HERE/obj/$f.o" ] || [ $stale = 1 ]; then
    $HIPCC $FLAGS -c "$HERE/$f.hip" -o "$HERE/obj/$f.o" &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
$HIPCC $FLAGS -x hip -c "$HERE/misc.cpp" -o "$HERE/obj/misc.o"
g++ -O2 -std=c++17 -fPIC -Wall -c "$HERE/vocab_text.cpp" -o "$HERE/obj/vocab_text.o"      # host C++ only: the ORBvoc.txt parser
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT" "$HERE/obj/extractor.o" "$HERE/obj/matcher.o" "$HERE/obj/lba.o" "$HERE/obj/full_ba.o" "$HERE/obj/essential_graph.o" "$HERE/obj/pose_opt.o" "$HERE/obj/pose_inertial.o" "$HERE/obj/inertial_ba.o" "$HERE/obj/inertial_init.o" "$HERE/obj/bow.o" "$HERE/obj/sim3.o" "$HERE/obj/sim3_opt.o" "$HERE/obj/newpoints.o" "$HERE/obj/fuse.o" "$HERE/obj/two_view.o" "$HERE/obj/search_init.o" "$HERE/obj/mlpnp.o" "$HERE/obj/misc.o" "$HERE/obj/vocab_text.o"
# the Tracking-thread loop above the C-ABI (host C++ only: plain g++ against liborbgpu.so)
g++ -O2 -std=c++17 -fPIC -shared -Wall "$HERE/agent_loop.cpp" -o "$HERE/../libagentloop.so" -L"$HERE/.." -lorbgpu -Wl,-rpath,'$ORIGIN' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib
echo "built $OUT"
