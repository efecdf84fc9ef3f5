"""Times the RGB-D Frame constructor (orbx_frame_rgbd: host images in, device frame with its grid out, one synchronisation) at
640 x 480 and 1000 features for three inputs -- 16-bit depth with a gray image, 16-bit depth with a BGR image, float32 depth with a gray
image -- and, beside them, the monocular constructor (orbx_frame_mono) on the same gray image.  Per input: median, 10th and 90th
percentile of 200 synchronous calls after 20 warm-up calls, wall clock around the whole C-ABI call, no host copies of the features.
What the RGB-D constructor does on top of the monocular one: the depth image through its staging slot and one copy kernel
(614 400 / 1 228 800 bytes for u16 / f32), for a colour image three times the bytes through the image's slot and the conversion kernel
instead of the plain copy, and the depth lookup inside the chain's last launch.
--mono-only times the monocular constructor alone (it runs on a tree without the RGB-D entry points: the parent's figure).
Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_orbslam3_amd import _capi as capi  # noqa: E402
from multi_orbslam3_amd import api, synth, views  # noqa: E402

REPS, WARM = 200, 20


def _time(fn):
    ts = []
    for k in range(REPS + WARM):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    us = 1e6 * np.array(ts[WARM:])
    return dict(median_us=round(float(np.median(us)), 1), p10_us=round(float(np.percentile(us, 10)), 1),
                p90_us=round(float(np.percentile(us, 90)), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mono-only", action="store_true")
    args = ap.parse_args()
    sc = synth.Scene(640, 480)
    L, R, Tcw = sc.stereo_pair(4)
    L = np.ascontiguousarray(L)
    p = sc.frame_view_params()
    fv0, keep0 = views.frame_view(np.zeros(1, capi.KEYPOINT_DTYPE), np.zeros((1, 32), np.uint8), None, None, p["bounds"], p["cam"], 8, 1.2)
    ex = api.ORBextractor(1000, 1.2, 8, 20, 7, 640, 480, n_cams=1)
    F = api.Frame()
    out = {"shape": "640x480, 1000 features", "reps": REPS}
    n = ex.frame_mono(F, fv0, L, None, download=False)
    out["n_features"] = n
    out["mono_gray"] = _time(lambda: ex.frame_mono(F, fv0, L, None, download=False))
    if not args.mono_only:
        bf = float(sc.cam["bf"])
        fac = api.depth_map_factor(5000.0)
        d16 = sc.depth_image(Tcw, np.uint16, 5000.0)
        d32 = sc.depth_image(Tcw, np.float32)
        bgr = sc.color_image(L, 3, rgb_order=False)
        cases = (("rgbd_u16_gray", L, d16, fac), ("rgbd_u16_bgr", bgr, d16, fac), ("rgbd_f32_gray", L, d32, 1.0))
        for name, img, dep, f in cases:
            ex.frame_rgbd(F, fv0, img, dep, bf, f, download=False)
            out[name] = _time(lambda: ex.frame_rgbd(F, fv0, img, dep, bf, f, download=False))
        out["mono_gray_again"] = _time(lambda: ex.frame_mono(F, fv0, L, None, download=False))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
