"""Times Optimizer::OptimizeEssentialGraph on the GPU (eg_solve on the calling thread's warm work area, the Python call included) on
keyframe rings of about 50 / 300 / 1000 keyframes (tests/essential_graph_model.py's scene family), each with the scale fixed and
free, and prints per problem the wall time (median of --reps), the device time by phase from HIP events (linearise / assemble /
LDL^T / update) and the sizes.  --model also times tests/essential_graph_model.py in float64 on one core, the only CPU figure there
is, up to --model-max keyframes (no GPU needed for that part: --model-only).

    python tools/essential_graph_time.py [--reps 5] [--model | --model-only] [--model-max 300]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    if "--model" in " ".join(sys.argv):
        os.environ[_v] = "1"                      # the model on one core

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import essential_graph_model as em  # noqa: E402

SIZES = [(50, 0xE650), (300, 0xE651), (1000, 0xE652)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--model-only", action="store_true")
    ap.add_argument("--model-max", type=int, default=300)
    args = ap.parse_args()
    for n_kf, seed in SIZES:
        for fix_scale in (True, False):
            p = em.flat_problem(em.collect_loop_form(em.make_scene(n_kf, fix_scale, seed, drift=em.FAMILY_DRIFT * 50.0 / n_kf, n_points=20 * n_kf)))
            row = dict(keyframes=n_kf, free=p.n_free, unknowns=7 * p.n_free, edges=len(p.vi), points=len(p.ref), fix_scale=fix_scale)
            if not args.model_only:
                from multi_orbslam3_amd import _capi as capi, api
                from test_essential_graph_cpu import api_arrays
                V, E, P = api_arrays(p)
                lib = capi.load()
                out = api.OptimizeEssentialGraph(V, E, P)          # cold: allocations
                walls = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    out = api.OptimizeEssentialGraph(V, E, P)
                    walls.append(time.perf_counter() - t0)
                lib.eg_set_profiling(1)
                api.OptimizeEssentialGraph(V, E, P)
                ms = (C.c_double * 4)()
                lib.eg_get_phase_ms(ms)
                lib.eg_set_profiling(0)
                row.update(wall_ms_median=1e3 * float(np.median(walls)), wall_ms_min=1e3 * min(walls), wall_ms_max=1e3 * max(walls),
                           lm_iterations=out.iters, trials=int(out.trace[:, 0].sum()), chi2=[out.err0, out.errEnd],
                           device_ms=dict(linearise=ms[0], assemble=ms[1], ldlt=ms[2], update=ms[3]))
            if (args.model or args.model_only) and n_kf <= args.model_max:
                t0 = time.perf_counter()
                ref = em.run(p, np.float64)
                row.update(model_f64_one_core_ms=1e3 * (time.perf_counter() - t0), model_iterations=ref["iters"],
                           model_trials=int(sum(t[0] for t in ref["trace"])), model_chi2=[float(ref["err0"]), float(ref["errEnd"])])
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
