"""Wall time of pose_inertial_optimize (both forms) next to pose_optimize at the same number of correspondences, in one process:
synchronous calls (each ends in the wait on its completion word), warmed up, the three entry points alternating within every
repetition, median and spread over the repetitions.  Prints one line per n; DESIGN section 6 holds the figures."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_inertial_model as pm                      # the scene generator
from multi_orbslam3_amd import _capi as capi, synth, views


def main(sizes=(300, 1000), reps=15, calls=200):
    lib = capi.load()
    for n in sizes:
        fns = {}
        for name, form in (("last_keyframe", pm.FORM_KF), ("last_frame", pm.FORM_FRAME)):
            p, keep = pm.to_c_problem(pm.make_scene(form, n, 900 + n + form, kind="mixed", outlier_frac=0.1))
            out = views.PoseInertialOutput(n)
            fns[name] = (lambda p=p, out=out, keep=keep: capi.check(lib.pose_inertial_optimize(C.byref(p), C.byref(out.c)), "pose_inertial_optimize"))
        pr = synth.make_pose_opt_problem(n=n, seed=77)
        pp, keep2 = views.pose_opt_problem(pr["Xw"], pr["u"], pr["v"], pr["ur"], pr["inv_sigma2"], pr["cam"], pr["Tcw"])
        po = views.PoseOptOutput(n)
        fns["pose_optimize"] = lambda: capi.check(lib.pose_optimize(C.byref(pp), C.byref(po.c)), "pose_optimize")
        for f in fns.values():
            for _ in range(20):
                f()
        us = {k: [] for k in fns}
        for _ in range(reps):
            for k, f in fns.items():
                t0 = time.perf_counter()
                for _ in range(calls):
                    f()
                us[k].append(1e6 * (time.perf_counter() - t0) / calls)
        med = {k: float(np.median(v)) for k, v in us.items()}
        print("n=%d: " % n + "; ".join("%s %.1f us (min %.1f, max %.1f)" % (k, med[k], min(us[k]), max(us[k])) for k in fns) +
              "; ratio to pose_optimize: last_keyframe %.2f, last_frame %.2f" % (med["last_keyframe"] / med["pose_optimize"],
                                                                                 med["last_frame"] / med["pose_optimize"]), flush=True)


if __name__ == "__main__":
    main()
