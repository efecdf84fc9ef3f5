"""Times the welding BA of LoopClosing::MergeLocal on the GPU (ba_weld_solve_h, warm handle, the Python call included) on MergeLocal's
shape: 15 adjusted + 15 fixed keyframes (numTemporalKFs, S/LoopClosing.cc:1324), about 3000 points, about 5 % gross outliers, 5 + 10
iterations -- once in the form the reference's own glue hands over (the adjusted keyframes carry no stamp: free poses without edges, a
points-only solve) and once with every keyframe stamped.  Beside each, on the same problem and handle, two ba_solve_h calls -- 5
robust iterations and 10 plain ones over ALL edges -- which is what the two solves cost without the level, the compaction and the
second structure build (and with the outliers still in the second one).  Prints per row the wall time (median of --reps), the device
time by phase from the handle's HIP events (ba_set_profiling) and the sizes.

    python tools/weld_ba_time.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_orbslam3_amd import api, synth, views  # noqa: E402

SHAPE = dict(n_free=15, n_fixed=15, n_points=3000, n_cameras=2, mono_frac=0.3, outlier_frac=0.05, seed=0xDE71, min_obs=3, max_obs=8)
PHASES = ("structure", "linearisation", "schur", "ldlt", "update_and_evaluation")


def _median_wall(fn, reps):
    fn()                                                      # cold: allocations
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        walls.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(walls)), 1e3 * min(walls), 1e3 * max(walls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    base = synth.make_ba_problem(**SHAPE)
    fixed_edges = base["pose_fixed"][base["edges"]["pose"]] != 0
    forms = (("reference_form_free_keyframes_without_edges", dict(base, edges=base["edges"][fixed_edges])), ("every_keyframe_stamped", base))
    h = api.FullBA()
    for name, pr in forms:
        arrays = (pr["poses"], pr["pose_fixed"], pr["pose_camera"], pr["points"], pr["edges"], pr["cameras"])
        row = dict(form=name, keyframes=len(pr["poses"]), free_keyframes_with_edges=int(len(set(pr["edges"]["pose"][~(pr["pose_fixed"][pr["edges"]["pose"]] != 0)].tolist()))),
                   points=len(pr["points"]), edges=len(pr["edges"]))
        pw, keepw = views.ba_weld_problem(*arrays, iterations=5, iterations_second=10)
        outw = views.BaWeldOutput(pw.ba.n_poses, pw.ba.n_points, pw.ba.n_edges)
        med, lo, hi = _median_wall(lambda: h.weld(pw, out=outw), args.reps)
        h.set_profiling(True)
        h.weld(pw, out=outw)
        ph = h.phase_ms()
        h.set_profiling(False)
        row["weld"] = dict(wall_ms_median=med, wall_ms_min=lo, wall_ms_max=hi, iterations=[outw.iters, outw.iters_second], rounds_run=outw.rounds_run,
                           level1=outw.n_level1, to_erase=int(len(outw.to_erase)), trials=[int(outw.trace_rows()[:, 2].sum()), int(outw.trace_second_rows()[:, 2].sum())],
                           device_ms=dict(zip(PHASES, ph)))
        p1, keep1 = views.ba_problem(*arrays, iterations=5, robust=True)
        p2, keep2 = views.ba_problem(*arrays, iterations=10, robust=False)
        o1, o2 = views.BaOutput(p1.n_poses, p1.n_points, p1.n_edges), views.BaOutput(p2.n_poses, p2.n_points, p2.n_edges)

        def two():
            h.solve(p1, out=o1)
            h.solve(p2, out=o2)

        med, lo, hi = _median_wall(two, args.reps)
        h.set_profiling(True)
        h.solve(p1, out=o1)
        pa = h.phase_ms()
        h.solve(p2, out=o2)
        pb = h.phase_ms()
        h.set_profiling(False)
        row["two_full_ba_solves"] = dict(wall_ms_median=med, wall_ms_min=lo, wall_ms_max=hi, iterations=[o1.iters, o2.iters],
                                         device_ms=dict(zip(PHASES, [a + b for a, b in zip(pa, pb)])))
        print(json.dumps(row), flush=True)
    h.close()


if __name__ == "__main__":
    main()
