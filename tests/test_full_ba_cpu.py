"""tests/full_ba_model.py, the float64 restatement of Optimizer::BundleAdjustment that the GPU tests hold the product against, pinned
on the CPU: against the oracle's local BA, robust against non-robust, the conditioning of every problem the GPU tests use, the
effect of per-keyframe cameras.  Also what ba_solve answers without a device: its refusals and the solves that run no iteration."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import full_ba_cases as fc
import full_ba_model as fm
from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import synth, views
from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# chi2 and lambda of the trace, model against oracle and product against model: the project's GPU-versus-oracle bound.  The model
# meets it against the oracle (largest relative difference measured over the one-camera problems below: 2.6e-14, printed by the test).
TRACE_RTOL = 1e-9


def _ba_view(pr, iterations, robust, pose_camera=None):
    return views.ba_problem(pr["poses"], pr["pose_fixed"], pr["pose_camera"] if pose_camera is None else pose_camera, pr["points"],
                            pr["edges"], pr["cameras"], iterations=iterations, robust=robust)


def test_header_declares_the_full_ba_symbols():
    hdr = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    declared = set(re.findall(r"^int\s+(ba_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(capi.FULL_BA_SYMBOLS), declared ^ set(capi.FULL_BA_SYMBOLS)
    lib = capi.load()
    for s in declared:
        assert hasattr(lib, s), s
    assert C.sizeof(capi.BaCamera) == 20 + C.sizeof(capi.Camera)


@pytest.mark.parametrize("seed", [0xBA04, 0xBA14])
def test_trace_equals_the_oracles_first_round(seed):
    args = dict(fc.CASES["one_camera"][0], seed=seed)
    pr = synth.make_ba_problem(**args)
    m = fm.solve(pr, 5, True)
    p, keep = views.lba_problem(pr["poses"], pr["pose_fixed"], pr["points"], pr["edges"], pr["cameras"][0][:5], its=(5, 10))
    o = ob.lba_solve(p)
    rows = o.trace_rows()[: o.iters[0]]
    assert m.iters == o.iters[0] == len(m.trace)
    assert np.array_equal(m.trace[:, 2], rows[:, 2])
    rel = np.abs(m.trace[:, :2] - rows[:, :2]) / np.abs(rows[:, :2])
    print("model against oracle, largest relative difference of lambda / chi2: %.3g" % rel.max())
    assert rel.max() <= TRACE_RTOL
    assert abs(m.chi2_initial - o.chi2[0]) <= TRACE_RTOL * o.chi2[0]


def test_robust_equals_non_robust_below_the_huber_threshold_and_differs_above():
    args = dict(fc.CASES["one_camera"][0], mono_frac=0.3, outlier_frac=0.0, pixel_sigma=0.3, sigma_rot_deg=0.01, sigma_t=0.0005, sigma_point=0.002)
    pr = synth.make_ba_problem(**args)
    a, b = fm.solve(pr, 4, True), fm.solve(pr, 4, False)
    # noise only, and little of it: no edge's chi2 reaches the lower (monocular) Huber threshold in any evaluation of either solve
    assert 0 < a.max_edge_chi2 < 5.99 and 0 < b.max_edge_chi2 < 5.99
    assert np.array_equal(a.trace, b.trace) and np.array_equal(a.poses, b.poses) and np.array_equal(a.points, b.points)
    pr = synth.make_ba_problem(**dict(fc.CASES["one_camera"][0], mono_frac=0.3, outlier_frac=0.1))
    a, b = fm.solve(pr, 4, True), fm.solve(pr, 4, False)
    assert not np.array_equal(a.trace, b.trace)
    assert np.abs(a.poses - b.poses).max() > 1e-4


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_every_problem_of_the_gpu_tests_is_well_conditioned(name):
    a, b = fc.model(name), fc.model(name, True)
    assert a.iters == b.iters and np.array_equal(a.trace[:, 2], b.trace[:, 2])
    assert np.abs(a.poses64 - b.poses64).max() <= 1e-6
    assert np.abs(a.points.astype(np.float64) - b.points).max() <= 1e-6
    assert min(a.min_abs_rho, b.min_abs_rho) > 1e-6, (a.min_abs_rho, b.min_abs_rho)


# ---------------------------------------------------------------- the cases past the first lap of the kernels' loops

def _shape(pr):
    """Free pose columns, degree per pose, observations per point, the set of non-empty pairs of free columns (diagonal included),
    the largest number of points an off-diagonal pair shares."""
    e = pr["edges"]
    fixed = np.asarray(pr["pose_fixed"]).astype(bool)
    col = np.where(fixed, -1, np.cumsum(~fixed) - 1)
    nP = int((~fixed).sum())
    deg = np.bincount(e["pose"], minlength=len(fixed))
    obs = np.bincount(e["point"], minlength=len(pr["points"]))
    seen = np.zeros((len(pr["points"]), nP), np.int64)
    c = col[e["pose"]]
    seen[e["point"][c >= 0], c[c >= 0]] = 1
    shared = seen.T @ seen
    pairs = int((np.triu(shared, 1) > 0).sum()) + nP
    return nP, deg, obs, pairs, int(np.triu(shared, 1).max()) if nP > 1 else 0


def _validates(pr, robust):
    p, keep = _ba_view(pr, 0, robust)
    rc, out = _solve(p)
    return rc == capi.ORBG_OK and out.iters == 0


def _has_descending_run(pr):
    e = pr["edges"]
    same = e["point"][1:] == e["point"][:-1]
    return bool((same & (e["pose"][1:] < e["pose"][:-1])).any())


def test_laps_has_degrees_around_one_and_two_laps():
    pr = fc.problem("laps")
    nP, deg, obs, pairs, shared = _shape(pr)
    free = np.flatnonzero(pr["pose_fixed"] == 0)
    assert tuple(deg[free]) == fc.LAPS_DEGREES == (255, 256, 257, 512, 513)
    assert deg[pr["pose_fixed"] != 0].tolist() == [600] and len(pr["edges"]) == 600 + sum(fc.LAPS_DEGREES)
    assert shared > 256                                        # an off-diagonal pair past one lap of k_ba_schur / k_ba_items_fill
    assert obs.min() >= 2
    assert _validates(pr, True)


@pytest.mark.parametrize("name", ["dense46", "dense52"])
def test_dense_cases_fill_every_pair(name):
    pr = fc.problem(name)
    nP, deg, obs, pairs, shared = _shape(pr)
    assert pairs == nP * (nP + 1) // 2 and pairs > 1024        # k_ba_scan: two elements per thread
    assert (nP <= 50) if name == "dense46" else (nP > 50)      # the eight-workgroup LDL^T / k_wide_*
    assert nP == (46 if name == "dense46" else 52)
    assert obs.max() >= 47
    assert _validates(pr, True)


def test_chain257_is_past_256_free_poses():
    pr = fc.problem("chain257")
    nP, deg, obs, pairs, shared = _shape(pr)
    assert nP == 257 and (nP + 31) // 32 == 9
    assert deg[pr["pose_fixed"] == 0].min() >= 1 and obs.min() >= 2
    assert _validates(pr, True)


@pytest.mark.parametrize("name", ["scrambled", "scrambled_gaps"])
def test_scrambled_cases_have_no_pose_order(name):
    pr = fc.problem(name)
    fixed = np.flatnonzero(pr["pose_fixed"])
    assert len(fixed) == 1 and 0 < fixed[0] < len(pr["poses"]) - 1
    assert _has_descending_run(pr) and not _has_descending_run(fc.problem("loop_closing"))
    assert _validates(pr, False)
    nP, deg, obs, pairs, shared = _shape(pr)
    if name == "scrambled":
        assert fixed[0] == 3 and obs.min() >= 2 and deg.min() >= 1
        return
    assert np.flatnonzero(obs == 0).tolist() == list(fc.GAP_POINTS) and 0 < fc.GAP_POINTS[1] < len(obs) - 1
    assert np.flatnonzero(deg == 0).tolist() == [fc.GAP_POSE] and not pr["pose_fixed"][fc.GAP_POSE]
    # nothing else moved: without its gaps the problem is `scrambled`
    s = fc.problem("scrambled")
    kp, kx = deg > 0, obs > 0
    assert np.array_equal(pr["poses"][kp], s["poses"]) and np.array_equal(pr["points"][kx], s["points"])
    assert np.array_equal(pr["pose_fixed"][kp], s["pose_fixed"]) and np.array_equal(pr["pose_camera"][kp], s["pose_camera"])
    assert np.array_equal((np.cumsum(kp) - 1)[pr["edges"]["pose"]], s["edges"]["pose"])
    assert np.array_equal((np.cumsum(kx) - 1)[pr["edges"]["point"]], s["edges"]["point"])


def test_the_model_does_not_depend_on_the_labelling():
    """The model on `scrambled` is the model on loop_closing mapped through the permutation: pinned here before the device is held
    to it."""
    a, b = fc.model("loop_closing"), fc.model("scrambled")
    pa, pb = fc.problem("loop_closing"), fc.problem("scrambled")
    perm = np.asarray(fc.SCRAMBLE)
    assert sorted(perm.tolist()) == list(range(len(pa["poses"])))
    assert np.array_equal(pb["poses"][perm], pa["poses"]) and np.array_equal(pb["pose_fixed"][perm], pa["pose_fixed"])
    assert np.array_equal(pb["pose_camera"][perm], pa["pose_camera"])
    src = pb["edge_source"]
    assert np.array_equal(np.sort(src), np.arange(len(src))) and not np.array_equal(src, np.arange(len(src)))
    for f in ("point", "u", "v", "ur", "inv_sigma2"):
        assert np.array_equal(pb["edges"][f], pa["edges"][f][src]), f
    assert np.array_equal(pb["edges"]["pose"], perm[pa["edges"]["pose"][src]])
    assert a.iters == b.iters and np.array_equal(a.trace[:, 2], b.trace[:, 2])
    rel = np.abs(a.trace[:, :2] - b.trace[:, :2]) / np.abs(a.trace[:, :2])
    dp, dx = np.abs(b.poses64[perm] - a.poses64).max(), np.abs(a.points.astype(np.float64) - b.points).max()
    print("relabelled against original: lambda %.3g chi2 %.3g poses %.3g points %.3g edge chi2 %.3g" %
          (rel[:, 0].max(), rel[:, 1].max(), dp, dx, np.abs(b.edge_chi2 - a.edge_chi2[src]).max()))
    assert rel.max() <= TRACE_RTOL
    assert abs(a.chi2_initial - b.chi2_initial) <= TRACE_RTOL * a.chi2_initial
    assert dp <= 1e-6 and dx <= 1e-6
    assert np.allclose(b.edge_chi2, a.edge_chi2[src], rtol=1e-6, atol=1e-6)
    assert np.array_equal(b.edge_depth_pos, a.edge_depth_pos[src]) and np.array_equal(a.point_included, b.point_included)


def test_a_stop_right_after_a_rejected_trial_returns_the_accepted_state():
    """optimization_algorithm_levenberg.cpp:143-147: a rejected trial multiplies lambda by ni and pop()s the vertices, but no
    computeActiveErrors follows: e->chi2() stays the rejected trial's."""
    full = fc.model("rejected")
    trials = full.trace[:, 2].astype(int).tolist()
    assert max(trials) > 1
    it = next(i for i, q in enumerate(trials) if q > 1)        # the first iteration with a rejection
    k = sum(trials[:it]) + 1                                   # its first trial, counted over the solve
    assert (it, k) == (4, 5)
    before, after = fc.model("rejected", False, k - 1), fc.model("rejected", False, k)
    assert before.iters == it and after.iters == it + 1 and after.trace[it, 2] == 1
    assert np.array_equal(after.trace[:it], before.trace) and np.array_equal(after.trace[:it], full.trace[:it])
    # the state: of the k - 1 accepted trials, to the bit
    assert np.array_equal(after.poses64, before.poses64) and np.array_equal(after.points, before.points)
    assert np.array_equal(after.edge_depth_pos, before.edge_depth_pos)
    assert after.chi2_final == before.chi2_final == after.trace[it, 1]
    # lambda: the raised one (ni = 2 after an accepted step), and the one the second trial of the full solve started from
    assert after.trace[it, 0] == 2.0 * before.trace[it - 1, 0]
    assert full.trace[it, 0] < after.trace[it, 0] and full.trace[it, 1] < after.trace[it, 1]
    # e->chi2(): of the rejected trial's state.  Without Huber kernels the chi2 of an evaluation is the sum over its edges: the
    # accepted state's is the trace's, the rejected trial's is larger (that is why it was rejected)
    assert abs(before.edge_chi2.sum() - before.chi2_final) <= 1e-12 * before.chi2_final
    assert after.edge_chi2.sum() > after.chi2_final * (1 + 1e-6)
    assert not np.allclose(after.edge_chi2, before.edge_chi2, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("name", fc.NEW_CASES)
def test_reordered_sums_bound_the_trace(name):
    """Where the GPU bound on lambda and chi2 of the cases above comes from (tests/full_ba_cases.py): forward against reversed sums,
    times ten, and never below the project's 1e-9.  Prints the figures; fails if one outgrows a tenth of its bound."""
    a, b = fc.model(name), fc.model(name, True)
    assert np.array_equal(a.trace[:, 2], b.trace[:, 2])
    rel = np.abs(a.trace[:, :2] - b.trace[:, :2]) / np.abs(a.trace[:, :2])
    chi2 = max(rel[:, 1].max(), abs(a.chi2_initial - b.chi2_initial) / a.chi2_initial)
    print("%s: forward against reversed sums: lambda %.3g chi2 %.3g poses %.3g points %.3g; bound %.3g" %
          (name, rel[:, 0].max(), chi2, np.abs(a.poses64 - b.poses64).max(), np.abs(a.points.astype(np.float64) - b.points).max(),
           fc.trace_rtol(name)))
    assert set(fc.REORDER_MEASURED) == set(fc.NEW_CASES)
    assert fc.trace_rtol(name) == max(1e-9, 10 * max(fc.REORDER_MEASURED[name]))
    assert max(rel[:, 0].max(), chi2) <= fc.trace_rtol(name) / 10 * 1.0001


def test_float_angles_of_the_fisheye_projection_bound_the_kb8_case():
    """Where the bounds of the KannalaBrandt8 case come from (tests/full_ba_cases.py): the model solved with theta and psi of
    KannalaBrandt8::project taken as the double atan2 rounded to float -- what the device computes -- and moved by one float32 ulp,
    against the model over the oracle's atan2f.  The GPU test's bounds are ten times the largest change measured here; this test
    prints the figures and fails if a change outgrows a tenth of its bound."""
    base = fc.model("kb8_pinhole")
    worst_chi2 = worst_edge = worst_lambda = 0.0
    for form in fc.KB8_ANGLE_FORMS:
        m = fc.model("kb8_pinhole", False, None, form)
        assert m.iters == base.iters and np.array_equal(m.trace[:, 2], base.trace[:, 2])
        assert 0 < m.max_kb8_residual_shift < 1e-4                                   # px: the angles did move, by last bits
        rel = np.abs(m.trace[:, :2] - base.trace[:, :2]) / np.abs(base.trace[:, :2])
        chi2 = max(rel[:, 1].max(), abs(m.chi2_initial - base.chi2_initial) / base.chi2_initial)
        edge = np.abs(m.edge_chi2 - base.edge_chi2).max()
        print("%s: chi2 %.3g lambda %.3g edge chi2 %.3g poses %.3g points %.3g" % (form, chi2, rel[:, 0].max(), edge,
              np.abs(m.poses64 - base.poses64).max(), np.abs(m.points.astype(np.float64) - base.points).max()))
        worst_chi2, worst_edge, worst_lambda = max(worst_chi2, chi2), max(worst_edge, edge), max(worst_lambda, rel[:, 0].max())
        assert np.abs(m.poses64 - base.poses64).max() <= 1e-5 and np.abs(m.points.astype(np.float64) - base.points).max() <= 1e-5
    assert worst_lambda <= TRACE_RTOL / 10
    assert worst_chi2 <= fc.KB8_CHI2_RTOL / 10 * 1.0001 and worst_edge <= fc.KB8_EDGE_CHI2_ATOL / 10 * 1.0001


def test_copies_of_a_component_follow_its_trajectory():
    """The argument the cap cases of tests/test_gpu_full_ba.py rest on (fc.REPLICATED), on three interleaved copies where the model
    can still solve the whole problem: trial counts equal the component's, lambda equal and chi2 three times the component's within
    the rule of the cases past the first lap, states equal.  For the K of the GPU cases the one term that does not scale -- the
    1e-3 next to computeScale in the gain ratio -- is shown not to matter from the component's own trials: every ratio has the
    component's sign and stays above the 0.937 from which the factor on lambda is the clamped 1/3.  Prints the forward-against-
    reversed figures the GPU bound is made of."""
    name = "component13"
    _, its, robust = fc.CASES[name]
    pr, one = fc.problem(name), fc.model(name)
    assert robust and one.iters == its and (one.edge_chi2 > fm.D_MONO ** 2 * 4).sum() >= 5          # robust, with outliers that stay
    rp = fc.replicate(pr, 3)
    K = rp["copies"]
    nP, deg, obs, pairs, shared = _shape(rp)
    assert nP == 3 * 13 and rp["pose_fixed"][:K].all() and not rp["pose_fixed"][K:].any()           # every copy its own fixed keyframe
    assert np.array_equal(rp["edges"]["pose"] % K, rp["edge_copy"]) and np.array_equal(rp["edges"]["point"] % K, rp["edge_copy"])
    assert (np.diff(rp["edges"]["point"].astype(np.int64)) >= 0).all() and _has_descending_run(rp) and _validates(rp, robust)
    three, want = fm.solve(rp, its, robust), fc.replicated_model(one, rp)
    assert three.iters == one.iters and np.array_equal(three.trace[:, 2], one.trace[:, 2])
    rel = np.abs(three.trace[:, :2] - want.trace[:, :2]) / np.abs(want.trace[:, :2])
    chi2 = max(rel[:, 1].max(), abs(three.chi2_initial - want.chi2_initial) / want.chi2_initial)
    dp, dx = np.abs(three.poses64 - want.poses64).max(), np.abs(three.points.astype(np.float64) - want.points).max()
    print("three copies against 3 x one: lambda %.3g chi2 %.3g poses %.3g points %.3g" % (rel[:, 0].max(), chi2, dp, dx))
    assert max(rel[:, 0].max(), chi2) <= 1e-9 and dp <= 1e-9 and dx <= 1e-6                       # (points: float32 values)
    assert np.array_equal(three.edge_depth_pos, want.edge_depth_pos) and np.array_equal(three.point_included, want.point_included)
    assert np.allclose(three.edge_chi2, want.edge_chi2, rtol=1e-9, atol=1e-9)
    # the gain ratios at the K of the GPU cases
    assert len(one.trial_gain) == int(one.trace[:, 2].sum())
    for d, s in one.trial_gain:
        assert s > 1.0
        for k in (1, 3) + tuple(c for _, c in fc.REPLICATED.values()):
            assert k * d / (k * s + 1e-3) > 0.95
    # the bounds of the replicated cases
    rev = fc.model(name, True)
    assert np.array_equal(rev.trace[:, 2], one.trace[:, 2])
    r2 = np.abs(one.trace[:, :2] - rev.trace[:, :2]) / np.abs(one.trace[:, :2])
    f_comp = max(r2.max(), abs(one.chi2_initial - rev.chi2_initial) / one.chi2_initial)
    assert max(c for _, c in fc.REPLICATED.values()) == fc.REPLICATED_MAX_K and set(fc.REPLICATED_MEASURED) == set(fc.REPLICATED)
    for rname, (comp, copies) in sorted(fc.REPLICATED.items()):
        f_sum = fc.replicated_sum_figure(one, pr, robust, copies)
        print("%s: component forward against reversed %.3g, chi2 sum of %d copies forward against reversed %.3g; bound %.3g" %
              (rname, f_comp, copies, f_sum, fc.replicated_trace_rtol(rname)))
        assert comp == name and max(f_comp, f_sum) <= fc.replicated_trace_rtol(rname) / 10 * 1.0001


def test_the_cap_case_is_at_the_cap_and_spans_every_index_range():
    rp = fc.replicated_problem("cap1365")
    K = rp["copies"]
    nP = int((rp["pose_fixed"] == 0).sum())
    deg, obs = np.bincount(rp["edges"]["pose"], minlength=len(rp["poses"])), np.bincount(rp["edges"]["point"], minlength=len(rp["points"]))
    assert nP == capi.BA_MAX_FREE_POSES == 1365 and 6 * nP == 8190 and (nP + 31) // 32 == 43        # 43 bitmap words per row
    free = np.flatnonzero(rp["pose_fixed"] == 0)
    assert deg[free].min() >= 1 and obs.min() >= 2
    e = rp["edges"]
    assert np.array_equal(e["pose"] % K, e["point"] % K)                       # disjoint copies ...
    first = e["pose"][np.r_[True, e["point"][1:] != e["point"][:-1]]]
    assert len(set((first // K).tolist())) > 1 and _has_descending_run(rp)       # ... interleaved, the runs in no pose order
    assert _validates(rp, True)
    nP2 = int((fc.replicated_problem("kilo1040")["pose_fixed"] == 0).sum())
    assert 1024 < nP2 == 1040 < capi.BA_MAX_FREE_POSES


def test_per_keyframe_cameras_matter():
    pr = fc.problem("loop_closing")
    a = fc.model("loop_closing")
    b = fm.solve(pr, 10, False, pose_camera=np.zeros(len(pr["poses"]), np.int32))
    assert np.abs(a.poses64 - b.poses64).max() > 1e-2


# ---------------------------------------------------------------- the C ABI without a device

def _solve(p, stop=None, boolean=False):
    out = views.BaOutput(p.n_poses, p.n_points, p.n_edges)
    lib = capi.load()
    fn = lib.ba_solve_b if boolean else lib.ba_solve
    rc = fn(C.byref(p), None if stop is None else C.c_void_p(stop.ctypes.data), C.byref(out.c))
    return rc, out


def test_refusals_come_before_any_device_work():
    pr = fc.problem("loop_closing")
    e = pr["edges"].copy()
    e["ur"][3] = capi.UR_RIGHT_CAMERA
    p, keep = _ba_view(dict(pr, edges=e), 10, True)
    assert _solve(p)[0] == capi.ORBG_BAD_ARG
    n = capi.BA_MAX_FREE_POSES + 1
    poses = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (n, 1))
    p, keep = views.ba_problem(poses, np.zeros(n, np.uint8), np.zeros(n, np.int32), pr["points"], pr["edges"][:0], pr["cameras"])
    assert _solve(p)[0] == capi.ORBG_CAP_EXCEEDED
    e = pr["edges"].copy()
    e[[0, len(e) - 1]] = e[[len(e) - 1, 0]]                      # a point's observations are no longer consecutive
    p, keep = _ba_view(dict(pr, edges=e), 10, True)
    assert _solve(p)[0] == capi.ORBG_BAD_ARG
    p, keep = _ba_view(pr, 10, True, pose_camera=np.full(len(pr["poses"]), 2, np.int32))
    assert _solve(p)[0] == capi.ORBG_BAD_ARG


@pytest.mark.parametrize("form", ["iterations0", "raised", "no_points"])
def test_a_solve_without_an_iteration_returns_the_estimate_it_was_given(form):
    pr = fc.problem("loop_closing")
    stop = None
    if form == "no_points":
        pr = dict(pr, points=pr["points"][:0], edges=pr["edges"][:0])
    p, keep = _ba_view(pr, 0 if form == "iterations0" else 10, True)
    if form == "raised":
        stop = np.array([np.iinfo(np.int32).min], np.int32)
    rc, out = _solve(p, stop)
    assert rc == capi.ORBG_OK and out.iters == 0 and out.c.trace_len == 0
    m = fm.solve(pr, 0, True)
    assert np.abs(out.poses - m.poses).max() <= 1e-6 and np.array_equal(out.points, pr["points"])
    assert np.array_equal(out.edge_depth_pos, m.edge_depth_pos) and not out.edge_chi2.any()
    assert np.array_equal(out.point_included, m.point_included)
