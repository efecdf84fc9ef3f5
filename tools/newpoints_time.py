"""Wall time of CreateNewMapPoints on the device: median of 200 synchronised calls after warm-up at n = 1000 features per keyframe,
B = 10 neighbours (stereo) and B = 20 neighbours (monocular); B single-neighbour calls against one call of B in the same run; and,
beside it, the serial C++ restatement (tests/cpp/new_points_ref.hpp through tests/cpp/new_points_glue --time) on a scene of the same
size as the CPU figure.  The device keyframes are resident (uploaded once, as the glue's cache keeps them); a call covers the host
merge-join, staging, the launch, the copy back and the replay.

    python tools/newpoints_time.py [--reps 200] [--one B]      (--one B: a single call at n = 1000 with B neighbours and exit: for a
    kernel trace, e.g. rocprofv3 --kernel-trace --stats -d prof -- python tools/newpoints_time.py --one 10)
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import newpoints_model as nm                    # noqa: E402  (the seeded scenes; nothing of the model runs here)
from multi_orbslam3_amd import api              # noqa: E402


def median_us(fn, reps, warm=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts))


def scene(B, mono, n=1000):
    k1, nbs = nm.make_scene(500 + B, n=n, B=B, n_nodes=n // 8, stereo_fraction=0.0 if mono else 0.5)
    return nm.device_keyframe(k1), [nm.device_keyframe(k) for k in nbs]


def restatement_us(n, B, mono, reps):
    exe = os.path.join(ROOT, "tests", "cpp", "new_points_glue")
    if not os.path.exists(exe):
        return None
    out = subprocess.check_output([exe, "--time", str(n), str(B), str(int(mono)), str(reps)], text=True)
    return float(out.split("restatement_us:")[1].split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--one", type=int, default=0)
    a = ap.parse_args()
    if a.one:
        d1, dn = scene(a.one, False)
        r = api.CreateNewMapPoints(d1, dn)
        print("one call, n = 1000, B = %d: %d points created" % (a.one, len(r.out)))
        return
    for B, mono in ((10, False), (20, True)):
        d1, dn = scene(B, mono)
        r = api.CreateNewMapPoints(d1, dn)
        whole, singles = api.NewPointsCall(d1, dn), [api.NewPointsCall(d1, [k]) for k in dn]      # (arguments flattened once: the call alone is timed)
        t_one = median_us(whole.run, a.reps)
        t_single = median_us(lambda: [c.run() for c in singles], max(a.reps // 4, 20), warm=5)
        cpu = restatement_us(1000, B, mono, max(a.reps // 10, 5))
        print("n = 1000, B = %2d %-6s: one call %8.1f us (%d matches, %d points); %d single calls %8.1f us: %s; serial C++ restatement %s us" % (
            B, "mono" if mono else "stereo", t_one, int((r.records["idx2"] >= 0).sum()), len(r.out), B, t_single,
            "one call faster" if t_one < t_single else "ONE CALL NOT FASTER", "%.1f" % cpu if cpu is not None else "(not built)"))


if __name__ == "__main__":
    main()
