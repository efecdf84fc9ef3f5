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


# ---------------------------------------------------------------- where the kernels of csrc/full_ba.hip take a second lap
# The cases above never leave the first lap of a per-pose, per-pair or per-point loop and never reject an LM trial (at most 80 edges
# per free pose, 53 items per pair, 513 pairs, 4 observations per point, 130 free poses, one trial per iteration).  The cases below do;
# tests/test_full_ba_cpu.py checks for each of them, from the problem itself, that it has the property it exists for.  A case may name
# a derivation step in DERIVED: problem() applies it to what the generator returns.
LAPS_DEGREES = (255, 256, 257, 512, 513)
SCRAMBLE = (3, 5, 0, 1, 4, 2)           # new index of old pose k of loop_closing: the fixed keyframe lands at index 3
CASES.update({
    # every pose sees every point (600 edges each); the edges of the free poses are trimmed to LAPS_DEGREES, around the 256 edges a
    # workgroup of k_ba_poses / k_ba_schur / k_ba_items_count / k_ba_items_fill takes per lap.  The two long poses share 425 points:
    # an off-diagonal pair of two laps
    "laps": (dict(n_free=5, n_fixed=1, n_points=600, n_cameras=2, mono_frac=0.3, outlier_frac=0.01, seed=0xBC20, min_obs=6, max_obs=6), 3, True),
    # every point seen by every pose: nP (nP + 1) / 2 > 1024 non-empty pairs (two elements per thread of k_ba_scan), runs of 47 / 53
    # observations, a fully dense reduced system through the eight-workgroup LDL^T (46 free poses) and through k_wide_* (52)
    "dense46": (dict(n_free=46, n_fixed=1, n_points=30, n_cameras=2, mono_frac=0.3, outlier_frac=0.0, seed=0xBC12, min_obs=47, max_obs=47), 2, True),
    "dense52": (dict(n_free=52, n_fixed=1, n_points=30, n_cameras=2, mono_frac=0.3, outlier_frac=0.0, seed=0xBC14, min_obs=53, max_obs=53), 2, True),
    # the first size past 256 free poses: second lap over hist[] / run[] of the counting sort, second workgroup of the thread-per-pose
    # kernels, 9 bitmap words per row, 1542 unknowns on k_wide_*
    "chain257": (dict(n_free=257, n_fixed=1, n_points=1542, n_cameras=2, mono_frac=0.2, outlier_frac=0.0, seed=0xBC13, min_obs=2, max_obs=3), 2, True),
    # loop_closing with its poses relabelled by SCRAMBLE and every point's run shuffled: the reference walks a
    # std::map<KeyFrame*, ...> per point, in any order, and its fixed keyframe has no place of its own
    "scrambled": (CASES["loop_closing"][0], 10, False),
    # ... plus an unobserved point at index 0, one in the middle of the point list, and a free keyframe without observations at index 2
    "scrambled_gaps": (CASES["loop_closing"][0], 10, False),
    # the fifth iteration rejects its first trial (trials 1 1 1 1 2 1 1 1): lambda * ni, the trial buffer dropped
    "rejected": (dict(n_free=5, n_fixed=1, n_points=90, n_cameras=2, mono_frac=0.4, outlier_frac=0.1, seed=0xBD02, sigma_rot_deg=2.0, sigma_t=0.1,
                      sigma_point=0.6), 8, False),
})
NEW_CASES = ("laps", "dense46", "dense52", "chain257", "scrambled", "scrambled_gaps", "rejected")
# Forward against reversed sums, measured on the CPU (tests/test_full_ba_cpu.py::test_reordered_sums_bound_the_trace prints them):
# largest relative difference of lambda / of chi2 over the trace.  A reordering of float64 sums is what legitimately separates two
# implementations, so the GPU bound of a case is max(1e-9, 10 x that figure), the margin of the KannalaBrandt8 case.
# name -> (lambda, chi2).  lambda does not move at all: its first value comes from the pose blocks, which the reversal leaves alone, and
# every accepted step of these solves scales it by the clamped 1/3.  chi2 of the ten-iteration non-robust problems moves most
# (loop_closing itself: 2.33e-10), so scrambled_gaps alone gets a bound above the project's 1e-9: 2.771e-9.  For the record, poses
# forward against reversed: laps 2.4e-16, dense46 1.8e-15, dense52 5.3e-15, chain257 7.8e-13, scrambled 7.8e-12, scrambled_gaps
# 2.4e-11, rejected 1.1e-11; smallest |gain ratio| 1.01, 1.04, 1.04, 1.00, 0.95, 0.95, 0.84; model solve 0.2 .. 1.7 s.
REORDER_MEASURED = {
    "laps": (0.0, 2.73e-16),
    "dense46": (0.0, 1.15e-15),
    "dense52": (0.0, 8.35e-16),
    "chain257": (0.0, 6.81e-15),
    "scrambled": (0.0, 9.83e-11),
    "scrambled_gaps": (0.0, 2.771e-10),
    "rejected": (0.0, 1.97e-11),
}


def trace_rtol(name):
    """The bound on lambda and chi2 of the trace, product against model, of one of NEW_CASES."""
    return max(1e-9, 10.0 * max(REORDER_MEASURED[name]))


def _select_edges(pr, keep):
    out = dict(pr)
    out["edges"] = pr["edges"][keep]
    return out


def trim_to_degrees(pr, degrees=LAPS_DEGREES):
    """Drops edges of the free poses 1 .. 5 until pose k has degrees[k - 1] of them.  Pose k loses the points j with
    (j + 97 k) mod n_points < n_points - degree: five windows of consecutive points.  The windows of the two long poses (points
    212 .. 299 and 115 .. 201) do not meet and the fixed pose keeps every edge, so every point keeps at least 2 observations."""
    e = pr["edges"]
    n = len(pr["points"])
    keep = np.ones(len(e), bool)
    for k, d in enumerate(degrees, start=1):
        keep &= ~((e["pose"] == k) & ((e["point"].astype(np.int64) + 97 * k) % n < n - d))
    return _select_edges(pr, keep)


def scramble(pr, perm=SCRAMBLE, seed=5):
    """pr with pose k relabelled perm[k] (poses, pose_fixed, pose_camera and the edges follow) and every point's run of edges
    shuffled.  out['edge_source'][k] is the index in pr['edges'] of edge k."""
    perm = np.asarray(perm, np.int64)
    inv = np.argsort(perm)                       # old index of new pose
    out = dict(pr)
    for f in ("poses", "pose_fixed", "pose_camera", "poses_true"):
        out[f] = pr[f][inv]
    e = pr["edges"]
    rng = np.random.RandomState(seed)
    src = np.arange(len(e))
    starts = np.flatnonzero(np.r_[True, e["point"][1:] != e["point"][:-1], True])
    for b, t in zip(starts[:-1], starts[1:]):
        rng.shuffle(src[b:t])
    e2 = e[src].copy()
    e2["pose"] = perm[e2["pose"]]
    out["edges"] = e2
    out["edge_source"] = src
    return out


def with_degenerate_vertices(pr, points_at=None, poses_at=None):
    """pr plus points nobody observes and free keyframes without an observation, at the given indices of the RESULT's point and pose
    lists (ascending); the ids of the later points and poses in the edges move up, so the order rule still holds.  Default: one of
    each, appended."""
    out = dict(pr)
    e = pr["edges"].copy()
    points, poses, fixed, cam = pr["points"], pr["poses"], pr["pose_fixed"], pr["pose_camera"]
    for n, at in enumerate([len(points)] if points_at is None else points_at):
        e["point"][e["point"] >= at] += 1
        points = np.insert(points, at, np.array([0.5 + n, -0.25, 4.0], np.float32), axis=0)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (0.3, 0.1, -0.2)
    for at in [len(poses)] if poses_at is None else poses_at:
        e["pose"][e["pose"] >= at] += 1
        poses = np.insert(poses, at, T.reshape(16), axis=0)
        fixed = np.insert(fixed, at, 0)
        cam = np.insert(cam, at, 0)
    out.update(points=points, poses=poses, pose_fixed=fixed.astype(np.uint8), pose_camera=cam.astype(np.int32), edges=e)
    out.pop("poses_true", None); out.pop("points_true", None)        # (they no longer line up with the vertices)
    return out


GAP_POINTS = (0, 46)                    # indices of the unobserved points of scrambled_gaps (46: the middle of 92 points)
GAP_POSE = 2                            # index of its keyframe without observations
DERIVED = {
    "laps": trim_to_degrees,
    "scrambled": scramble,
    "scrambled_gaps": lambda pr: with_degenerate_vertices(scramble(pr), points_at=GAP_POINTS, poses_at=(GAP_POSE,)),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    pr = synth.make_ba_problem(**CASES[name][0])
    return DERIVED[name](pr) if name in DERIVED else pr


# ---------------------------------------------------------------- the caps, against a model that stays cheap
# K disjoint copies of one component: chi2 is K times the component's, the largest diagonal entry (lambda's first value) is the
# component's, and the gain ratio of a trial is K dchi2 / (K scale + 1e-3) where the component's is dchi2 / (scale + 1e-3): the same
# sign, and the same factor on lambda as long as both sit above the 0.937 from which the factor is the clamped 1/3.  The LM
# trajectory of every copy is then the component's, which the model solves in half a second.  The component: 13 free poses and a
# fixed one, robust with 3 % outliers, four iterations (gain ratios 1.07 .. 1.4, computeScale 50 and more; tests/test_full_ba_cpu.py
# checks both for K = REPLICATED_MAX_K).  It is a case like the others (CASES), the replicated problems are not: nobody runs the model on them.
CASES["component13"] = (dict(n_free=13, n_fixed=1, n_points=195, n_cameras=2, mono_frac=0.3, outlier_frac=0.03, seed=0xBE01, min_obs=2, max_obs=4), 4, True)
# name -> (component, copies).  105 x 13 = 1365 = BA_MAX_FREE_POSES (8190 unknowns); 80 x 13 = 1040: past the 1024 threads of
# one workgroup of the thread-per-pose kernels and below the cap, so that a failure at the cap can be told from one at the second workgroup
REPLICATED = {"cap1365": ("component13", 105), "kilo1040": ("component13", 80)}
REPLICATED_MAX_K = 105


def replicate(pr, K, seed=11):
    """K disjoint copies of pr, interleaved: pose (point) k of copy c is pose (point) k * K + c of the result, every copy with its own
    fixed keyframes and points.  The edges keep the order rule (edge.point never decreases) and nothing else: inside a point's run
    they are shuffled by a seeded permutation.  out['edge_source'][e] / out['edge_copy'][e]: the component's edge and the copy."""
    out = {f: np.repeat(pr[f], K, axis=0) for f in ("poses", "pose_fixed", "pose_camera", "points")}
    out["cameras"] = pr["cameras"]
    e = np.repeat(pr["edges"], K)
    src = np.repeat(np.arange(len(pr["edges"])), K)
    copy = np.tile(np.arange(K), len(pr["edges"]))
    e["pose"] = e["pose"].astype(np.int64) * K + copy
    e["point"] = e["point"].astype(np.int64) * K + copy
    rng = np.random.RandomState(seed)
    o = np.lexsort((rng.permutation(len(e)), e["point"]))
    out.update(edges=e[o], edge_source=src[o], edge_copy=copy[o], copies=K)
    return out


@functools.lru_cache(maxsize=None)
def replicated_problem(name):
    comp, K = REPLICATED[name]
    return replicate(problem(comp), K)


def replicated_model(m, rp):
    """What the model would return on the replicated problem rp, from its result m on the component."""
    K = rp["copies"]
    r = fm.BaModelResult()
    r.iters, r.trace = m.iters, m.trace * np.array([1.0, K, 1.0])
    r.chi2_initial, r.chi2_final = K * m.chi2_initial, K * m.chi2_final
    r.poses, r.poses64, r.points = np.repeat(m.poses, K, axis=0), np.repeat(m.poses64, K, axis=0), np.repeat(m.points, K, axis=0)
    r.point_included = np.repeat(m.point_included, K)
    r.edge_chi2, r.edge_depth_pos = m.edge_chi2[rp["edge_source"]], m.edge_depth_pos[rp["edge_source"]]
    return r


def replicated_sum_figure(m, pr, robust, K):
    """Forward against reversed for the chi2 sum of K interleaved copies (rho of every edge of the model's last evaluation on the
    component pr, one term per edge of the replicated problem), relative."""
    chi = np.asarray(m.edge_chi2, np.float64)
    delta = np.where(pr["edges"]["ur"] < 0, fm.D_MONO, fm.D_STEREO)
    rho = np.where(robust & (chi > delta * delta), 2 * np.sqrt(chi) * delta - delta * delta, chi)
    terms = np.repeat(rho, K)
    fwd, rev = 0.0, 0.0
    for v in terms.tolist():
        fwd += v
    for v in terms[::-1].tolist():
        rev += v
    return abs(fwd - rev) / fwd


def replicated_trace_rtol(name):
    """max(1e-9, 10 x the larger of: the component's trace forward against reversed, the replicated chi2 sum forward against
    reversed) -- measured on the CPU, tests/test_full_ba_cpu.py::test_copies_of_a_component_follow_its_trajectory prints both."""
    return max(1e-9, 10.0 * max(REPLICATED_MEASURED[name]))


# name -> (component's trace forward against reversed, chi2 sum of the K copies forward against reversed).  Three copies against
# three times the component, for the record: lambda 0, chi2 1.1e-14, poses 1.3e-13, points 0.
REPLICATED_MEASURED = {"cap1365": (9.79e-15, 9.07e-14), "kilo1040": (9.79e-15, 6.58e-15)}


@functools.lru_cache(maxsize=None)
def model(name, reverse=False, stop_after_trials=None, kb8_angles="oracle"):
    _, its, robust = CASES[name]
    return fm.solve(problem(name), its, robust, reverse_sums=reverse, stop_after_trials=stop_after_trials, kb8_angles=kb8_angles)
