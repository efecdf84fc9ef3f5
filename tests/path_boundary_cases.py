"""Inputs of the path-boundary tests (tests/test_gpu_path_boundaries.py on the device, tests/test_path_boundaries_cpu.py for the
conditions those rest on): every size at which a kernel of the library changes its code path, and the seeds chosen for them.  Nothing
here touches the GPU; the oracle and the numpy models are the only things that run."""
import numpy as np

import helpers
import sim3_model as sm
import sim3_opt_model as om
from multi_orbslam3_amd import synth, views
from oracle import binding as ob

# ------------------------------------------------------------------ 1. PoseOptimization (csrc/pose_opt.hip)
# n < 3 returns; n <= 512 pose_opt_wide_kernel<1>; n <= 1024 <2> (inputs read from the pinned block up to there); beyond, the
# four-wavefront pose_opt_kernel; 4096 is the cap.  The rig form: <1> / <2> / <4> / <8> at 512 / 1024 / 2048, cap 4096.
POSE_N = (3, 4, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4095, 4096)
POSE_RIG_N = (512, 513, 1024, 1025, 2048, 2049, 4096)
POSE_PAD = ((512, 1), (512, 37), (1024, 1), (1024, 37))          # (n, k): n + k runs on the next kernel


def pose_seed(n):
    return 7000 + n


def pose_problem(n, mono_frac=0.2, outlier_frac=0.1):
    return synth.make_pose_opt_problem(n=n, outlier_frac=outlier_frac, mono_frac=mono_frac, seed=pose_seed(n))


def pose_rig_split(n):
    """(n_left, n_right) with n_left + n_right = n, the right camera holding two fifths."""
    return n - 2 * n // 5, 2 * n // 5


def pose_rig_problem(n):
    nl, nr = pose_rig_split(n)
    return synth.make_pose_opt_rig_problem(n_left=nl, n_right=nr, outlier_frac=0.1, seed=0xB0DE + n)


def pose_view(pr):
    rig = views.camera_rig(*pr["rig"]) if "rig" in pr else None
    return views.pose_opt_problem(pr["Xw"], pr["u"], pr["v"], pr["ur"], pr["inv_sigma2"], pr["cam"], pr["Tcw"], rig=rig)


def pose_pad_inert(pr, k):
    """pr with k inert correspondences appended: a point in front of the true camera, its projection (rounded to float32) as the
    observation, inv_sigma2 = 0.  Whatever the pose, its weighted error, its chi2 and its terms of H and b are exact zeros (0 times a
    finite number), it is an inlier of every round, and a sum it joins is the sum without it."""
    rng = np.random.RandomState(977 + k)
    fx, fy, cx, cy, bf = pr["cam"]
    T = pr["T_true"]
    z = rng.uniform(2.0, 8.0, k)
    uu, vv = rng.uniform(40, 600, k), rng.uniform(40, 440, k)
    Pc = np.stack([(uu - cx) * z / fx, (vv - cy) * z / fy, z], 1)
    Xw = (Pc - T[:3, 3]) @ T[:3, :3]
    ur = uu - bf / z
    ur[::2] = -1.0                                                      # monocular and stereo ones alike
    f = np.float32
    out = dict(pr)
    out["Xw"] = np.concatenate([pr["Xw"], Xw.astype(f)])
    out["u"] = np.concatenate([pr["u"], uu.astype(f)])
    out["v"] = np.concatenate([pr["v"], vv.astype(f)])
    out["ur"] = np.concatenate([pr["ur"], ur.astype(f)])
    out["inv_sigma2"] = np.concatenate([pr["inv_sigma2"], np.zeros(k, f)])
    return out


# ------------------------------------------------------------------ 2. Sim3Solver (csrc/sim3.hip)
# correspondences through LDS in tiles of kTile = 1024; masks in 64-bit words, row stride ceil(n / 64); kGroup = 16 hypotheses per
# workgroup.  (n, fix_scale, outlier fraction, seed, H) as tests/test_gpu_sim3.py's HYP_CASES.
SIM3_HYP_CASES = [(n, k % 2 == 0, (0.3, 0.5)[k % 3 == 0], 900 + k, 65)
                  for k, n in enumerate((63, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049))] + \
                 [(1025, True, 0.3, 921, 15), (1025, False, 0.3, 922, 16), (1025, True, 0.5, 923, 17)]
SIM3_BATCH = ((3, 17, 931), (1024, 300, 932), (1025, 16, 933), (2049, 65, 934))      # (n, H, seed) of the one-launch batch


def sim3_left_out(cases):
    """(decisions, decisions whose float64-model error lies within a relative 1e-3 of its threshold) over the cases, with the draws
    the device test uses."""
    from multi_orbslam3_amd import api
    decisions = near = 0
    for n, fs, of, seed, H in cases:
        sc = sm.make_scene(seed, n, fs, of)
        draws = api.sim3_draws(n, H, seed + 1)
        b = sm.hypotheses(sc["X1"], sc["X2"], sc["e1"], sc["e2"], sc["K1"], sc["K2"], sc["fix_scale"], draws, np.float64)
        nt = sm.near_threshold(b, sc["e1"], sc["e2"])
        decisions += nt.size
        near += int(nt.sum())
    return decisions, near


# ------------------------------------------------------------------ 3. OptimizeSim3 (csrc/sim3_opt.hip)
# n <= kS3oTile = 1024: the LDS_IN = true instantiation; beyond, global memory on every pass.  Thread t owns pairs t, t + 256, ...
def sim3_opt_family():
    """(seed, n, fix_scale, outlier fraction, special) as sim3_opt_model.family(): both scale modes, 30 % wrong matches."""
    return [(3000000 + 10 * n + int(fs), n, fs, 0.3, None) for n in (255, 256, 257, 1023, 1024, 1025) for fs in (True, False)]


def sim3_opt_pad_inert(p):
    """p with one inert pair appended: finite geometry in front of both cameras, w1 = w2 = 0, n_correspondences raised by one.  Both
    of its weighted errors are exact zeros at every estimate, so it adds zeros to H, b and chi2 and is never removed."""
    f = np.float32
    return om.Problem(np.concatenate([p.X1, np.array([[0.25, -0.5, 4.0]], f)]), np.concatenate([p.X2, np.array([[-0.5, 0.25, 5.0]], f)]),
                      np.concatenate([p.obs1, np.array([[300.0, 200.0]], f)]), np.concatenate([p.obs2, np.array([[280.0, 260.0]], f)]),
                      np.concatenate([p.w1, np.zeros(1, f)]), np.concatenate([p.w2, np.zeros(1, f)]), p.K1, p.K2, p.fix_scale, p.th2,
                      p.q, p.t, p.s, n_corr=p.n_corr + 1)


SIM3_OPT_PAD = ((3010241, 1024, True), (3002560, 256, False))          # (seed, n, fix_scale): 1024 -> 1025 changes the path, 256 -> 257 does not


def sim3_opt_pad_problem(entry):
    seed, n, fs = entry
    return om.make_problem(seed, n, fs, 0.3)
