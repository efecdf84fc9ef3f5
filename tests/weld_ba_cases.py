"""The problems of the welding-BA tests, shared by tests/test_weld_ba_cpu.py (which checks the model on them and that each has the
property it exists for) and tests/test_gpu_weld_ba.py (which holds ba_weld_solve against tests/weld_ba_model.py on them).  Conventions
of tests/full_ba_cases.py: a case is (make_ba_problem arguments, round 1's iterations, round 2's), DERIVED names the steps applied to
what the generator returns, a model solve is computed once per process and nobody changes it.

The gross outliers are PLANTED here instead of drawn by the generator (pr['outlier'], one flag per edge), because two
implementations can only be compared on a round 2 that is well posed: a point whose level-0 edges are one monocular observation is a
ray -- its 3 x 3 block is singular up to lambda and its depth is whatever rounding makes of it (the reference does the same; it is not
something to hold two float64 implementations against each other on).  So an edge is corrupted only where its point keeps a stereo
observation or two observations without it, and the pixel noise is half a pixel, which keeps every clean edge far below the
thresholds.  tests/test_weld_ba_cpu.py checks that no point of round 2 is left as such a ray."""
import functools

import numpy as np

from multi_orbslam3_amd import synth

import weld_ba_model as wm

# 4 to 6 observations per point, one in five monocular.  The seeds are chosen per case: see test_weld_ba_cpu.py,
# test_every_case_is_comparable -- the stereo projection of the reference rounds the inverse depth to float32, so an edge's residual is
# a step function of the state (steps of about 3e-5 px), and two float64 implementations agree to 1e-6 in an edge's chi2 only on a run
# during which no such rounding falls differently.  Over 15 iterations that holds for some inputs and not for others (DESIGN.md,
# "Welding BA": of 40 seeds each of weld_points_only and weld_dropped, 1 and 2 stay within 1e-7 both model against reversed model and
# product against model; those are the ones used).
_SMALL = dict(n_free=5, n_fixed=3, n_points=90, n_cameras=2, mono_frac=0.2, min_obs=4, max_obs=6, outlier_frac=0.0, pixel_sigma=0.5, seed=0xDE19)
CASES = {
    # 5 adjusted + 3 fixed keyframes of two agents, monocular and stereo edges, about 8 % gross outliers
    "weld_small": (_SMALL, 5, 10),
    # ... with every edge of a free keyframe removed: what the reference's glue normally hands over (the edge filter tests a stamp the
    # adjusted keyframes do not carry): no free pose has an edge, nP = 0 in both rounds, points against the fixed keyframes
    "weld_points_only": (dict(_SMALL, seed=0xDE6B), 5, 10),
    # every observation of some points and of the free keyframe DROPPED_POSE corrupted: they leave round 2 entirely; one point is
    # also seen from an added fixed keyframe that faces away, the observation at its projection
    "weld_dropped": (dict(_SMALL, seed=0xDE69), 5, 10),
    # no outliers: every edge stays at level 0, the compaction is the identity
    "weld_clean": (dict(_SMALL, seed=0xDE7A), 5, 10),
    # more than 1024 edges: the second element per thread of the one-workgroup scan, five workgroups and more of the per-edge kernels
    # with a partial last one.  2 + 2 iterations keep the model within seconds
    "weld_1100": (dict(_SMALL, n_points=300, seed=0xDE43), 2, 2),
}
OUTLIER_FRAC = {"weld_small": 0.08, "weld_points_only": 0.08, "weld_dropped": 0.08, "weld_clean": 0.0, "weld_1100": 0.05}
DROPPED_POINTS = (10, 47)               # weld_dropped: the points asked for (pr['dropped_points'] has them and those that follow DROPPED_POSE)
DROPPED_POSE = 5
FACING_AWAY = 1.9                       # rad: the trace of the rotation stays positive (the model's quaternion-from-rotation has that branch alone)


def _placed(e, clean, n_points):
    """Per point: its clean edges hold a stereo observation or at least two observations."""
    n = np.bincount(e["point"][clean], minlength=n_points)
    st = np.bincount(e["point"][clean & (e["ur"] >= 0)], minlength=n_points)
    return (st > 0) | (n >= 2)


def _corrupt(e, k, n):
    """+-30 px on u, -+30 px on v (and u_R with u) of edge k, the sign alternating with n."""
    s = np.float32(30.0 if n % 2 == 0 else -30.0)
    e["u"][k] += s; e["v"][k] -= s
    if e["ur"][k] >= 0:
        e["ur"][k] += s


def plant_outliers(pr, frac, seed):
    """Corrupts about frac of the edges, in a seeded random order, each only if its point stays placed by its clean edges FROM THE
    FIXED KEYFRAMES alone or -- for a point they do not place anyway -- by all its clean edges.  out['outlier']: the flags."""
    out = dict(pr)
    e = pr["edges"].copy()
    L = len(pr["points"])
    fixed_edge = pr["pose_fixed"][e["pose"]] != 0
    bad = np.zeros(len(e), bool)
    rng = np.random.RandomState(seed)
    n = 0
    for k in rng.permutation(len(e)):
        if rng.rand() >= frac:
            continue
        l = int(e["point"][k])
        before = _placed(e, ~bad & fixed_edge, L)[l]
        bad[k] = True
        ok = _placed(e, ~bad & fixed_edge, L)[l] if before else _placed(e, ~bad, L)[l]
        if not ok:
            bad[k] = False
            continue
        _corrupt(e, k, n)
        n += 1
    out["edges"], out["outlier"] = e, bad
    return out


def points_only(pr):
    """Every edge of a free keyframe removed, and with them the edges of the points that the clean edges of the fixed keyframes do
    not place: those become unobserved points of the problem."""
    out = dict(pr)
    e, bad = pr["edges"], pr["outlier"]
    keep = pr["pose_fixed"][e["pose"]] != 0
    keep &= _placed(e, keep & ~bad, len(pr["points"]))[e["point"]]
    out["edges"], out["outlier"] = e[keep], bad[keep]
    return out


def dropped(pr):
    """Corrupts every clean edge of DROPPED_POINTS and of DROPPED_POSE, then every edge of the points which that leaves unplaced
    (out['dropped_points']: all the points without a clean edge).  out['behind_edge']: index of the added edge (monocular, coarsest
    level) from the added fixed keyframe len(poses) - 1, which is keyframe 0 turned by FACING_AWAY about its y axis: the point
    out['behind_point'] lies behind it; the observation is what the projection formula gives there."""
    out = dict(pr)
    e, bad = pr["edges"].copy(), pr["outlier"].copy()
    L = len(pr["points"])
    rng = np.random.RandomState(len(e))
    want = np.isin(e["point"], DROPPED_POINTS) | (e["pose"] == DROPPED_POSE)
    for _ in range(2):
        for k in np.flatnonzero(want & ~bad):
            # 30 px in a direction of its own: a keyframe ALL of whose observations move could follow any common part of the moves
            a = rng.uniform(0.0, 2.0 * np.pi)
            du, dv = np.float32(30.0 * np.cos(a)), np.float32(30.0 * np.sin(a))
            e["u"][k] += du; e["v"][k] += dv
            if e["ur"][k] >= 0:
                e["ur"][k] -= du
            bad[k] = True
        want = ~_placed(e, ~bad, L)[e["point"]]
    assert _placed(e, ~bad, L)[e["point"][~bad]].all()
    has_clean = np.bincount(e["point"][~bad], minlength=L) > 0
    has_edge = np.bincount(e["point"], minlength=L) > 0
    out["dropped_points"] = np.flatnonzero(has_edge & ~has_clean)
    T0 = np.asarray(pr["poses"][0], np.float32).reshape(4, 4).astype(np.float64)
    c, sn = np.cos(FACING_AWAY), np.sin(FACING_AWAY)
    Ry = np.array([[c, 0.0, sn], [0.0, 1.0, 0.0], [-sn, 0.0, c]])
    T = np.eye(4)
    T[:3, :3] = Ry @ T0[:3, :3]; T[:3, 3] = Ry @ T0[:3, 3]
    T32 = T.astype(np.float32)
    assert np.trace(T32[:3, :3]) > 0.2

    def behind(j):
        return T32[:3, :3].astype(np.float64) @ pr["points"][j].astype(np.float64) + T32[:3, 3].astype(np.float64)

    # the point seen from behind: the first one with three clean observations or more, none by DROPPED_POSE, well behind that keyframe
    j = next(j for j in range(L) if (~bad & (e["point"] == j)).sum() >= 3 and not (e["pose"][e["point"] == j] == DROPPED_POSE).any() and
             behind(j)[2] < -1.5)
    Xc = behind(j)
    fx, fy, cx, cy = pr["cameras"][0][:4]
    new = np.zeros(1, e.dtype)
    new[0] = (len(pr["poses"]), j, np.float32(fx * Xc[0] / Xc[2] + cx), np.float32(fy * Xc[1] / Xc[2] + cy), np.float32(-1.0),
              e["inv_sigma2"].min())
    at = int(np.flatnonzero(e["point"] == j)[-1]) + 1
    out["edges"] = np.concatenate([e[:at], new, e[at:]])
    out["outlier"] = np.concatenate([bad[:at], [False], bad[at:]])          # (not an outlier by its chi2: level 1 by its depth)
    out["poses"] = np.concatenate([pr["poses"], T32.reshape(1, 16)])
    out["pose_fixed"] = np.concatenate([pr["pose_fixed"], np.ones(1, np.uint8)])
    out["pose_camera"] = np.concatenate([pr["pose_camera"], np.zeros(1, np.int32)])
    out["behind_edge"], out["behind_point"] = at, j
    out.pop("poses_true", None)
    return out


DERIVED = {"weld_points_only": (points_only,), "weld_dropped": (dropped,)}

# Forward against reversed sums of the model (tests/test_weld_ba_cpu.py::test_reordered_sums_bound_the_traces prints them): largest
# relative difference of lambda / of chi2 over BOTH traces.  name -> (lambda, chi2); the GPU bound of a case is
# max(1e-9, 10 x the larger figure), as in tests/full_ba_cases.py.
REORDER_MEASURED = {
    "weld_small": (0.0, 8.27e-13),
    "weld_points_only": (0.0, 3.58e-11),
    "weld_dropped": (0.0, 3.08e-10),
    "weld_clean": (0.0, 2.22e-14),
    "weld_1100": (1.49e-16, 1.16e-15),
}


def trace_rtol(name):
    return max(1e-9, 10.0 * max(REORDER_MEASURED[name]))


@functools.lru_cache(maxsize=None)
def problem(name):
    args = CASES[name][0]
    pr = plant_outliers(synth.make_ba_problem(**args), OUTLIER_FRAC[name], args["seed"] + 1)
    for step in DERIVED.get(name, ()):
        pr = step(pr)
    return pr


@functools.lru_cache(maxsize=None)
def model(name, reverse=False, stop_after_trials=None, stop_before=False, iterations_second=None):
    _, its, its2 = CASES[name]
    return wm.solve(problem(name), its, its2 if iterations_second is None else iterations_second, reverse_sums=reverse,
                    stop_after_trials=stop_after_trials, stop_before=stop_before)
