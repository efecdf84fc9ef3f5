"""Times Optimizer::BundleAdjustment on the GPU (ba_solve_h, warm handle, the Python call included) on three synthetic maps:
2 keyframes / 100 points / 20 iterations, 100 / 10 000 / 10 and 500 / 50 000 / 10, each with two cameras (one for the first), and
prints per problem the wall time (median of --reps), the device time by phase from the handle's HIP events (structure build,
linearisation, Schur complement, LDL^T, update + evaluation) and the sizes.  --model also times tests/full_ba_model.py, the only CPU
figure there is, on the first two problems (no GPU needed for that part: --model-only).

    python tools/full_ba_time.py [--reps 5] [--model | --model-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multi_orbslam3_amd import synth, views  # noqa: E402

PROBLEMS = [
    ("2kf_100pt", dict(n_free=1, n_fixed=1, n_points=100, n_cameras=1, mono_frac=1.0, outlier_frac=0.0, seed=0xBA71, min_obs=2, max_obs=2), 20, True),
    ("100kf_10000pt", dict(n_free=99, n_fixed=1, n_points=10000, n_cameras=2, mono_frac=0.3, outlier_frac=0.02, seed=0xBA72, min_obs=3, max_obs=8), 10, False),
    ("500kf_50000pt", dict(n_free=499, n_fixed=1, n_points=50000, n_cameras=2, mono_frac=0.3, outlier_frac=0.02, seed=0xBA73, min_obs=3, max_obs=8), 10, False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--model-only", action="store_true")
    args = ap.parse_args()
    for name, kw, its, robust in PROBLEMS:
        pr = synth.make_ba_problem(**kw)
        row = dict(problem=name, keyframes=len(pr["poses"]), points=len(pr["points"]), edges=len(pr["edges"]), iterations=its, robust=robust)
        if not args.model_only:
            from multi_orbslam3_amd import api
            h = api.FullBA()
            p, keep = views.ba_problem(pr["poses"], pr["pose_fixed"], pr["pose_camera"], pr["points"], pr["edges"], pr["cameras"],
                                       iterations=its, robust=robust)
            out = views.BaOutput(p.n_poses, p.n_points, p.n_edges)
            h.solve(p, out=out)                                   # cold: allocations
            walls = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                h.solve(p, out=out)
                walls.append(time.perf_counter() - t0)
            h.set_profiling(True)
            h.solve(p, out=out)
            ph = h.phase_ms()
            h.close()
            row.update(wall_ms_median=1e3 * float(np.median(walls)), wall_ms_min=1e3 * min(walls), wall_ms_max=1e3 * max(walls), lm_iterations=out.iters,
                       trials=int(out.trace_rows()[:, 2].sum()), chi2=list(out.chi2),
                       device_ms=dict(structure=ph[0], linearisation=ph[1], schur=ph[2], ldlt=ph[3], update_and_evaluation=ph[4]))
        if (args.model or args.model_only) and len(pr["poses"]) <= 100:
            import full_ba_model as fm
            t0 = time.perf_counter()
            m = fm.solve(pr, its, robust)
            row.update(model_wall_s=time.perf_counter() - t0, model_iterations=m.iters)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
