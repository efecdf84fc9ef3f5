"""Times ORBmatcher::SearchForInitialization at window 100 on two shapes with extractor-shaped level populations: n1 = n2 = 5000 at
640 x 480 and 10 000 at 1280 x 720.  Per shape, medians of 30 synchronised calls of the whole C-ABI call after 3 warm-up calls:
  fresh   F2 has a new content before every call, as mCurrentFrame has at S/Tracking.cc:2217, so the call builds the level-0 view
          (the upload of F2 is outside the timed region and complete before it);
  cached  F2 keeps its content, so the view is reused.
The parts: view = fresh - cached; replay = the library's replay header (csrc/init_replay.hpp) alone over the call's own lists, built
-O2 as tests/cpp/init_replay_check and run on one core; search kernel, the record and list copies and the waits = cached - replay.
The library itself carries no clock.  Beside them the serial C++ restatement (tests/cpp/search_init_glue --time) on one core of the
same box.  Needs a GPU, g++ and the built glue program."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import search_init_model as sm  # noqa: E402
from multi_orbslam3_amd import api, views  # noqa: E402

CAM = (458.0, 457.0, 320.0, 240.0, 40.0, 0.08)


def device_frame(F):
    fv, keep = views.frame_view(F.kps, F.desc, None, None, [float(b) for b in F.bounds], CAM, 8, 1.2)
    return api.Frame(cap_features=F.n).upload(fv, keep)


def main():
    for n, (w, h) in ((5000, (640, 480)), (10000, (1280, 720))):
        F1, F2 = sm.make_pair(71, n, n, width=w, height=h)
        prev = F1.pts
        d1, d2 = device_frame(F1), device_frame(F2)
        m = api.ORBmatcher(0.9, True)
        nm, m12, pv, lists = m.SearchForInitialization(d1, d2, prev, 100, debug=True)
        fv2, keep2 = views.frame_view(F2.kps, F2.desc, None, None, [float(b) for b in F2.bounds], CAM, 8, 1.2)
        times = {}
        for mode in ("cached", "fresh"):
            ts = []
            for k in range(33):
                if mode == "fresh":
                    d2.upload(fv2, keep2)                                # a new content: the view is built inside the call
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.SearchForInitialization(d1, d2, prev, 100)
                ts.append(time.perf_counter() - t0)
            times[mode] = 1e3 * np.array(ts[3:])
        fresh, cached = float(np.median(times["fresh"])), float(np.median(times["cached"]))
        with tempfile.TemporaryDirectory() as td:
            p = os.path.join(td, "scene.bin")
            sm.write_scene(p, F1, F2, prev, 100)
            lp, exe = os.path.join(td, "lists.bin"), os.path.join(td, "init_replay_check")
            sm.write_lists(lp, lists, F1, F2, prev)
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "multi_orbslam3_amd", "csrc"),
                                   os.path.join(ROOT, "tests", "cpp", "init_replay_check.cpp"), "-o", exe])
            replay = float(subprocess.run([exe, lp, "30"], capture_output=True, text=True, check=True).stdout.split()[1]) / 1e3
            out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "search_init_glue"), "--time", p, "30"], capture_output=True, text=True)
        ref_us = float(out.stdout.split()[1]) if out.returncode == 0 else float("nan")
        ll = np.diff(lists["list_start"])
        print("n %5d at %dx%d: %d queries, %d candidates (longest list %d), %d matches | call median (min): fresh F2 %.3f (%.3f) ms, "
              "cached view %.3f (%.3f) ms | parts: view %.3f, search + copies + waits %.3f, replay %.3f ms | serial C++ on one core %.3f ms" %
              (n, w, h, lists["n_queries"], lists["n_candidates"], int(ll.max()), nm, fresh, times["fresh"].min(), cached,
               times["cached"].min(), fresh - cached, cached - replay, replay, ref_us / 1e3))


if __name__ == "__main__":
    main()
