"""The problems of the full-BA tests, shared by tests/test_full_ba_cpu.py (which checks that each of them is well enough conditioned
to compare two implementations on) and tests/test_gpu_full_ba.py (which holds the product against tests/full_ba_model.py on them).
A model solve is computed once per process and shared; nobody changes it."""
import functools

import numpy as np

from multi_orbslam3_amd import synth

import full_ba_model as fm

# name -> (make_ba_problem arguments, iterations, robust)
CASES = {
    # Tracking::CreateInitialMapMonocular: two keyframes, the first one fixed, monocular points, GlobalBundleAdjustemnt(map, 20)
    "initial_map": (dict(n_free=1, n_fixed=1, n_points=80, n_cameras=1, mono_frac=1.0, outlier_frac=0.0, seed=0xBA01, min_obs=2, max_obs=2), 20, True),
    # LoopClosing::RunGlobalBundleAdjustment after a merge: keyframes of two agents, bRobust = false, 10 iterations
    "loop_closing": (dict(n_free=5, n_fixed=1, n_points=90, n_cameras=2, mono_frac=0.4, outlier_frac=0.03, seed=0xBA02), 10, False),
    "kb8_pinhole": (dict(n_free=5, n_fixed=1, n_points=90, n_cameras=2, mono_frac=1.0, outlier_frac=0.0, seed=0xBA03, kb8_camera=1), 5, True),
    # one camera, stereo edges: comparable with the first round of the oracle's local BA (whose monocular Huber threshold is
    # sqrt(5.991) where BundleAdjustment has sqrt(5.99); the stereo one is the same)
    "one_camera": (dict(n_free=4, n_fixed=2, n_points=80, n_cameras=1, mono_frac=0.0, outlier_frac=0.03, seed=0xBA04), 5, True),
    # a chain: each point is seen by 2-3 neighbouring keyframes, most pose pairs share nothing
    "chain40": (dict(n_free=40, n_fixed=1, n_points=600, n_cameras=2, mono_frac=0.3, outlier_frac=0.0, seed=0xBA05, min_obs=2, max_obs=3), 3, True),
}
# the sizes at which the reduced camera system changes solver (one workgroup <= 20 free poses, eight <= 50, many beyond) and
# 64 / 65 / 130: the first sizes past one and two words of a pair-bitmap row
BOUNDARY_POSES = (20, 21, 50, 51, 64, 65, 130)
for _n in BOUNDARY_POSES:
    CASES["boundary_%d" % _n] = (dict(n_free=_n, n_fixed=2, n_points=15 * _n, n_cameras=2, mono_frac=0.3, outlier_frac=0.01, seed=0xBB00 + _n,
                                      min_obs=2, max_obs=4), 3, True)


# Bounds of the one problem with a KannalaBrandt8 keyframe.  theta and psi of KannalaBrandt8::project are float32 VALUES of atan2f in
# the reference (S/CameraModels/KannalaBrandt8.cpp:52-56); the oracle calls the host's atan2f, the device rounds the double atan2 to
# float, and the two differ in the last bit for some arguments.  Measured ON THE CPU (tests/test_full_ba_cpu.py,
# test_float_angles_of_the_fisheye_projection_bound_the_kb8_case: the model solved again with the double atan2 rounded to float, and
# with theta and psi of every edge one float32 ulp up / down), largest over the three: chi2 of the trace 5.82e-7 relative, chi2 of one
# edge 4.86e-5 absolute, lambda 0, trial counts equal.  The bounds are ten times the measured values; lambda, trial counts and the
# state keep the bounds of every other case.
KB8_CHI2_RTOL = 5.82e-6
KB8_EDGE_CHI2_ATOL = 4.86e-4
KB8_ANGLE_FORMS = ("rounded_double", "ulp_up", "ulp_down")


@functools.lru_cache(maxsize=None)
def problem(name):
    return synth.make_ba_problem(**CASES[name][0])


@functools.lru_cache(maxsize=None)
def model(name, reverse=False, stop_after_trials=None, kb8_angles="oracle"):
    _, its, robust = CASES[name]
    return fm.solve(problem(name), its, robust, reverse_sums=reverse, stop_after_trials=stop_after_trials, kb8_angles=kb8_angles)


def with_degenerate_vertices(pr):
    """pr plus a point nobody observes (appended) and a free keyframe without an observation (appended)."""
    out = dict(pr)
    out["points"] = np.concatenate([pr["points"], np.array([[0.5, -0.25, 4.0]], np.float32)])
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (0.3, 0.1, -0.2)
    out["poses"] = np.concatenate([pr["poses"], T.reshape(1, 16)])
    out["pose_fixed"] = np.concatenate([pr["pose_fixed"], np.zeros(1, np.uint8)])
    out["pose_camera"] = np.concatenate([pr["pose_camera"], np.zeros(1, np.int32)])
    return out
