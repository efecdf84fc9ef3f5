"""Times TwoViewReconstruction::Reconstruct at 200 iterations for 100, 500 and 2000 matches: the GPU call (api.TwoViewReconstruction,
median of 30 synchronised calls after 3 warm-up calls, ctypes marshalling included) and, on the same box, the serial restatement
(tests/two_view_model.py in float32: numpy, batched over the hypotheses, so a LOWER bound on what a scalar serial loop costs in
Python and no stand-in for the reference's C++).  Prints one line per size.  Needs a GPU."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import two_view_model as tm  # noqa: E402
from multi_orbslam3_amd import api  # noqa: E402


def main():
    for n in (100, 500, 2000):
        sc = tm.scene("3d", n, 11, n_extra1=n // 4, n_extra2=n // 3)
        d = api.two_view_draws(n, 200, 12)
        tv = api.TwoViewReconstruction(sc.cam, 1.0, 200)
        for _ in range(3):
            r = tv.Reconstruct(sc.keys1, sc.keys2, sc.matches12, draws=d)
        ts = []
        for _ in range(30):
            t0 = time.perf_counter()
            r = tv.Reconstruct(sc.keys1, sc.keys2, sc.matches12, draws=d)
            ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        o = tm.reconstruct(sc.keys1, sc.keys2, sc.matches12, sc.cam, 1.0, 200, d, np.float32)
        t_model = time.perf_counter() - t0
        print("matches %4d: GPU call median %.3f ms (min %.3f), numpy model %.1f ms; ok %s / %s, model %d / %d" %
              (n, 1e3 * float(np.median(ts)), 1e3 * min(ts), 1e3 * t_model, r.ok, o.ok, r.model, o.model))


if __name__ == "__main__":
    main()
