"""Times Optimizer::LocalInertialBA on the GPU (inertial_ba_solve_h, warm handle, the Python call included) on two synthetic windows of
tests/inertial_ba_model.py -- 10 free + 20 fixed keyframes with 1500 points, and 25 + 50 with bLarge -- and prints per problem the wall
time (median of --reps), the device time by phase from the handle's HIP events (structure and upload, linearisation, Schur complement,
LDL^T, update + evaluation) and the sizes.  The yardstick of the same run: lba_solve_h, the visual local BA, over the same visual
edges with the same keyframes free (camera poses from the body poses, no inertial edges).

    python tools/inertial_ba_time.py [--reps 5]
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

import inertial_ba_model as m  # noqa: E402
from multi_orbslam3_amd import api, views  # noqa: E402

PROBLEMS = [
    ("10kf_20fixed_1500pt", dict(n_free=10, n_points=1500, seed=0x1BA1, n_other_fixed=19, outlier_frac=0.02, steps=20)),
    ("25kf_50fixed_large", dict(n_free=25, n_points=1500, seed=0x1BA2, n_other_fixed=49, outlier_frac=0.02, steps=10, large=True)),
]


def visual_lba_problem(P):
    """the views.lba_problem over the visual edges of a model problem: Tcw of every keyframe from its body pose"""
    Tcb = np.asarray(P["Tcb"], np.float64).reshape(3, 4)
    poses = []
    for kf in P["kfs"]:
        s = m.pim.make_state(**{k: np.asarray(v, np.float64) for k, v in kf["state"].items()})
        Rcw, tcw = m.pim.camera_pose(s, Tcb)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rcw, tcw
        poses.append(T)
    fixed = np.array([kf["fixed"] for kf in P["kfs"]], np.uint8)
    return views.lba_problem(np.array(poses, np.float32), fixed, P["points"], P["edges"], P["cam"])


def timed(call, reps):
    call()                                                    # cold: allocations
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    return dict(wall_ms_median=1e3 * float(np.median(walls)), wall_ms_min=1e3 * min(walls), wall_ms_max=1e3 * max(walls))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    opt = api.Optimizer()
    for name, kw in PROBLEMS:
        P = m.make_scene(**kw)
        S = m.Structure(P)
        row = dict(problem=name, free_keyframes=int(S.nF), fixed_keyframes=int(S.NK - S.nF), points=int(S.NX), edges=int(S.NE), unknowns=int(S.n),
                   inertial_edges=len(S.inertial), large=bool(P["large"]))
        p, keep = m.to_c_problem(P)
        h = api.InertialBA()
        res = {}

        def solve():
            res["out"] = opt.LocalInertialBA(p, handle=h)
        row["inertial_ba"] = timed(solve, args.reps)
        h.set_profiling(True)
        solve()
        ph = h.phase_ms()
        h.close()
        out = res["out"].as_dict()
        row["inertial_ba"].update(lm_iterations=int(out["iters"]), trials=int(out["trace"][:, 2].sum()), chi2=[out["chi2_initial"], out["chi2_final"]],
                                  outliers=int(out["n_outliers"]), failed=int(out["failed"]),
                                  device_ms=dict(structure_and_upload=ph[0], linearisation=ph[1], schur=ph[2], ldlt=ph[3], update_and_evaluation=ph[4]))
        lp, lkeep = visual_lba_problem(P)
        lout = views.LbaOutput(lp.n_poses, lp.n_points, lp.n_edges)
        row["lba_solve_h"] = timed(lambda: opt.LocalBundleAdjustment(lp, out=lout), args.reps)
        row["lba_solve_h"].update(iterations=[int(lout.c.iters_round1), int(lout.c.iters_round2)])
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
