"""Wall time of SearchInNeighbors through the glue (include/orbgpu_localmapping.hpp: two orbm_fuse launches and their replays) and of
the serial C++ restatement (tests/cpp/fuse_ref.hpp) on the same box and the same mock map, through tests/cpp/fuse_glue --time: 1000
features per keyframe, 30 stereo targets and 60 monocular targets; median of `reps` calls after two warm-up calls, every call on a
fresh copy of the map with its keyframes resident before the clock starts.  Also: how many replayed records needed the host rescoring
and how many the single-pair relaunch; and the orbm_fuse call alone (staging, launch, the dense K x P download) on a seeded scene of the
same size.

    python tools/fuse_time.py [--reps 30] [--one K]      (--one K: a single orbm_fuse call at n = P = 1000 with K keyframes and exit:
    for a kernel trace, e.g. rocprofv3 --kernel-trace --stats -d prof -- python tools/fuse_time.py --one 30)
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
import fuse_model as fm                         # noqa: E402  (the seeded scenes; nothing of the model runs here)
from multi_orbslam3_amd import api              # noqa: E402


def median_us(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts))


def launch_scene(K, mono, n=1000):
    kfs, pts, _ = fm.make_scene(900 + K, K=K, n=n, P=n, stereo_fraction=0.0 if mono else 0.5)
    return [fm.device_keyframe(k) for k in kfs], fm.device_points(pts)


def glue_times(n, targets, mono, reps):
    exe = os.path.join(ROOT, "tests", "cpp", "fuse_glue")
    if not os.path.exists(exe):
        return None
    out = subprocess.check_output([exe, "--time", str(n), str(targets), str(int(mono)), str(reps)], text=True)
    return {ln.split(":")[0]: ln.split(":")[1].split() for ln in out.splitlines() if ":" in ln}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--one", type=int, default=0)
    a = ap.parse_args()
    if a.one:
        dk, dp = launch_scene(a.one, False)
        rec, _ = api.Fuse(dk, dp)
        print("one call, n = P = 1000, K = %d: %d pairs with candidates" % (a.one, int((rec["status"] == 0).sum())))
        return
    for targets, mono in ((30, False), (60, True)):
        dk, dp = launch_scene(targets, mono)
        rec, _ = api.Fuse(dk, dp)
        t_call = median_us(lambda: api.Fuse(dk, dp), a.reps)
        g = glue_times(1000, targets + 1, mono, a.reps)                     # (+ 1: one keyframe of the mock map is bad)
        line = "n = 1000, %2d %-6s targets: orbm_fuse alone %8.1f us (%d of %d pairs reach the window, %d with candidates)" % (
            targets, "mono" if mono else "stereo", t_call, int((rec["status"] >= 5).sum() + (rec["status"] == 0).sum()), rec.size, int((rec["status"] == 0).sum()))
        if g is None:
            print(line + "; glue (not built)")
            continue
        print(line + "; SearchInNeighbors through the glue %s us, serial C++ restatement %s us (%s targets; %s records replayed, %s rescored on the host, "
              "%s re-evaluated singly)" % (g["glue_us"][0], g["restatement_us"][0], g["targets"][0], g["pairs"][0], g["rescored"][0], g["relaunched"][0]))


if __name__ == "__main__":
    main()
