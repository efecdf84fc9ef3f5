"""Wall time of inertial_init_solve at 10, 100 and 1000 keyframes in the first overload's form (monocular: velocities, biases, gravity
direction and scale free, LM, up to 200 iterations) and the third's (velocities and biases, LM): synchronous calls, each ending in the wait
on its completion word, the calling thread's work area warm, median and spread over the repetitions.  Beside each timing: the iterations
and LM trials the call ran, and the time the numpy model (tests/inertial_init_model.py, formulation (b)) takes for the same problem on one
core.  No threshold is attached; README and DESIGN section 4 hold the figures."""
import ctypes as C
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("MKL_NUM_THREADS", "1")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inertial_init_model as m                       # the scene generator and the model
from multi_orbslam3_amd import _capi as capi, views


def main(sizes=(10, 100, 1000), reps=7):
    lib = capi.load()
    for n in sizes:
        for name, form in (("first (mono)", 1), ("third (list)", 3)):
            P = m.make_scene(n=n, seed=700 + n + form, **m.form_problem(form, bMono=True))
            p, keep = m.to_c_problem(P)
            out = views.InertialInitOutput(p)
            call = lambda: capi.check(lib.inertial_init_solve(C.byref(p), C.byref(out.c)), "inertial_init_solve")
            for _ in range(3):
                call()
            calls = max(1, min(50, 2000 // n))
            us = []
            for _ in range(reps):
                t0 = time.perf_counter()
                for _ in range(calls):
                    call()
                us.append(1e6 * (time.perf_counter() - t0) / calls)
            g = out.as_dict()
            t0 = time.perf_counter()
            r = m.solve(P)
            t_model = time.perf_counter() - t0
            trials = int(g["trace"][:, 2].sum())
            print("n=%d %s: %d unknowns, %d iterations / %d trials (model %d / %d): %.1f us (min %.1f, max %.1f), %.1f us per trial; numpy model "
                  "on one core %.1f ms" % (n, name, g["n_unknowns"], g["iters"], trials, r["iters"], int(r["trace"][:, 2].sum()), float(np.median(us)),
                                           min(us), max(us), float(np.median(us)) / max(trials, 1), 1e3 * t_model), flush=True)


if __name__ == "__main__":
    main()
