"""Wall time of OptimizeSim3 on the device: median of >= 200 synchronised calls after warm-up, for one problem at n = 100 / 300 / 1000
and for batches of 6 and 24 problems at n = 300; 24 single calls against one batch of 24 in the same run.

    python tools/sim3_opt_time.py [--reps 200] [--one N]      (--one N: a single call at n = N and exit: for a kernel trace, e.g.
    rocprofv3 --kernel-trace --stats -d prof -- python tools/sim3_opt_time.py --one 300)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3_opt_model as om                     # noqa: E402  (the seeded scenes; nothing of the model runs here)
from multi_orbslam3_amd import api              # noqa: E402


def problem(n, seed):
    p = om.make_problem(seed, n, bool(seed & 1), 0.3)
    return api.Sim3OptProblem(p.X1, p.X2, p.obs1, p.obs2, p.w1, p.w2, p.K1, p.K2, p.fix_scale, p.th2, p.q, p.t, p.s)


def median_us(fn, reps, warm=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--one-batch", type=int, default=0)
    a = ap.parse_args()
    if a.one:
        r = api.OptimizeSim3(problem(a.one, 300031))
        print("one call, n = %d: nIn %d, LM iterations %s" % (a.one, r.nIn, r.iters))
        return
    if a.one_batch:
        rs = api.OptimizeSim3.batch([problem(300, 300030 + k) for k in range(a.one_batch)])
        print("one batch of %d, n = 300: nIn %s" % (a.one_batch, [r.nIn for r in rs]))
        return
    for n in (100, 300, 1000):
        p = problem(n, 1000 * n + 31)
        r = api.OptimizeSim3(p)
        print("single n = %4d: %8.1f us   (nIn %d, LM iterations %s, trials %d)" % (
            n, median_us(lambda: api.OptimizeSim3(p), a.reps), r.nIn, r.iters, int(r.trace[:, 3].sum())))
    probs = [problem(300, 300030 + k) for k in range(24)]
    for B in (6, 24):
        print("batch of %2d at n = 300: %8.1f us" % (B, median_us(lambda: api.OptimizeSim3.batch(probs[:B]), a.reps)))
    t_single = median_us(lambda: [api.OptimizeSim3(p) for p in probs], max(a.reps // 4, 20), warm=5)
    t_batch = median_us(lambda: api.OptimizeSim3.batch(probs), max(a.reps // 4, 20), warm=5)
    print("24 single calls %.1f us, one batch of 24 %.1f us: %s" % (t_single, t_batch, "batch faster" if t_batch < t_single else "BATCH NOT FASTER"))


if __name__ == "__main__":
    main()
