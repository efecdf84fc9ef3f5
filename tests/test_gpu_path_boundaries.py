"""Every kernel at the sizes where it switches code path (inputs and seeds: tests/path_boundary_cases.py; the conditions they rest on,
without a device: tests/test_path_boundaries_cpu.py).  PoseOptimization at 3 / 512 / 1024 / 4096 and its rig form at 512 / 1024 / 2048 /
4096; Sim3Solver around its LDS tile of 1024 pairs, its 64-bit mask words and its groups of 16 hypotheses; OptimizeSim3 around its LDS
tile of 1024 pairs and its 256 threads; the frame searches above 4096 features (occupancy in device arrays) up to the cap of 65534."""
import ctypes as C

import numpy as np
import pytest

import frame_boundary_cases as fb
import path_boundary_cases as pb
import sim3_model as sm
import sim3_opt_model as om
import test_gpu_sim3 as ts
import test_gpu_sim3_opt as tso
from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import api, views
from oracle import binding as ob

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. PoseOptimization

def _assert_pose_parity(g, o):
    """The assertions of test_gpu_parity.test_pose_optimization_parity."""
    assert g.n_inliers == o.n_inliers
    assert np.array_equal(g.outliers, o.outliers)
    assert np.abs(g.Tcw.astype(np.float64) - o.Tcw.astype(np.float64)).max() <= 1e-6
    assert all(abs(a - b) <= 1 for a, b in zip(g.iters, o.iters)), (g.iters, o.iters)
    if g.iters == o.iters:
        assert np.allclose(g.chi2, o.chi2, rtol=1e-8, atol=1e-9)
    else:
        assert np.allclose(g.chi2, o.chi2, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("n", pb.POSE_N)
def test_pose_optimization_at_every_kernel_boundary(n):
    """3 is the smallest problem that launches; 512 | 513: one | two correspondences per thread; 1024 | 1025: the wide kernel reading
    the pinned block | the four-wavefront kernel reading a device copy; 4096: sixteen per thread, the cap."""
    pr = pb.pose_problem(n)
    p, keep = pb.pose_view(pr)
    g = api.Optimizer().PoseOptimization(p)
    o = ob.pose_optimize(p)
    print("n=%d iters %s / %s inliers %d" % (n, g.iters, o.iters, g.n_inliers))
    _assert_pose_parity(g, o)
    g2 = api.Optimizer().PoseOptimization(p)
    assert np.array_equal(g.Tcw, g2.Tcw) and g.iters == g2.iters and g.chi2 == g2.chi2 and np.array_equal(g.outliers, g2.outliers)
    if n >= 63:
        assert 0 < (g.outliers != 0).sum() < n // 4                     # the problem has outliers, and they were told apart


def test_pose_optimization_of_three_monocular_correspondences():
    """n = 3, all monocular: six equations for six unknowns, one round (fewer than 10 edges).  The oracle runs its LM iterations down
    to a chi2 of rounding size; the launch must end where the oracle ends."""
    pr = pb.pose_problem(3, mono_frac=1.0, outlier_frac=0.0)
    assert (pr["ur"] < 0).all()
    p, keep = pb.pose_view(pr)
    g = api.Optimizer().PoseOptimization(p)
    o = ob.pose_optimize(p)
    print("iters %s / %s chi2 %s / %s" % (g.iters, o.iters, g.chi2, o.chi2))
    assert o.iters[0] > 0 and o.iters[1:] == (0, 0, 0)
    _assert_pose_parity(g, o)


def _raw_pose_optimize(p):
    out = views.PoseOptOutput(p.n)
    out.c.n_inliers = -7
    return capi.load().pose_optimize(C.byref(p), C.byref(out.c)), out


def test_pose_optimization_refuses_4097_correspondences():
    pr = pb.pose_problem(4097)
    rc, out = _raw_pose_optimize(pb.pose_view(pr)[0])
    assert rc == capi.ORBG_CAP_EXCEEDED and out.c.n_inliers == -7
    rg = pb.pose_rig_problem(4097)
    p, keep = pb.pose_view(rg)
    rc, out = _raw_pose_optimize(p)
    assert rc == capi.ORBG_CAP_EXCEEDED and out.c.n_inliers == -7


@pytest.mark.parametrize("n", pb.POSE_RIG_N)
def test_pose_optimization_rig_form_at_every_kernel_boundary(n):
    """The rig form's one / two / four / eight correspondences per thread, with the assertions of
    test_gpu_parity.test_pose_optimization_with_the_two_fisheye_rig as they stand."""
    pr = pb.pose_rig_problem(n)
    p, keep = pb.pose_view(pr)
    g = api.Optimizer().PoseOptimization(p)
    o = ob.pose_optimize(p)
    print("n=%d iters %s / %s inliers %d / %d" % (n, g.iters, o.iters, g.n_inliers, o.n_inliers))
    assert abs(g.n_inliers - o.n_inliers) <= 1 and (g.outliers != o.outliers).sum() <= 1
    assert np.abs(g.Tcw.astype(np.float64) - o.Tcw.astype(np.float64)).max() <= 1e-5
    assert all(abs(a - b) <= 2 for a, b in zip(g.iters, o.iters)), (g.iters, o.iters)
    assert np.allclose(g.chi2, o.chi2, rtol=5e-3, atol=1e-6)
    assert np.abs(g.Tcw - pr["T_true"]).max() < np.abs(pr["Tcw"] - pr["T_true"]).max()
    g2 = api.Optimizer().PoseOptimization(p)
    assert np.array_equal(g.Tcw, g2.Tcw) and g.iters == g2.iters


@pytest.mark.parametrize("n,k", pb.POSE_PAD)
def test_pose_optimization_across_a_boundary_with_inert_correspondences(n, k):
    """The same problem on two kernels: n correspondences, and those followed by k inert ones (exact zeros in H, b and chi2, never
    outliers), which puts it on the next kernel.  512 + 1 lands in thread 0 behind that thread's own correspondence: whether the bits
    agree is printed, not asserted (the order of the sums is not documented).  Measured on an MI355X: 512 -> 513 and 512 -> 549 agree in
    every bit of Tcw, iters and chi2; 1024 -> 1025 and 1024 -> 1061 (the four-wavefront kernel, another order of summation) give the same
    iterations and the same float32 pose, with chi2 differing in its last bits."""
    pr = pb.pose_problem(n)
    a = api.Optimizer().PoseOptimization(pb.pose_view(pr)[0])
    p2, keep = pb.pose_view(pb.pose_pad_inert(pr, k))
    assert p2.n == n + k
    b = api.Optimizer().PoseOptimization(p2)
    same = np.array_equal(a.Tcw, b.Tcw) and a.iters == b.iters and a.chi2 == b.chi2
    print("%d -> %d: bits of Tcw / iters / chi2 %s; iters %s / %s; max |d Tcw| %.3g" % (
        n, n + k, "agree" if same else "differ", a.iters, b.iters, np.abs(a.Tcw.astype(np.float64) - b.Tcw).max()))
    assert np.array_equal(b.outliers[:n], a.outliers) and not b.outliers[n:].any()
    assert b.n_inliers == a.n_inliers + k
    assert np.abs(a.Tcw.astype(np.float64) - b.Tcw.astype(np.float64)).max() <= 1e-6
    assert all(abs(x - y) <= 1 for x, y in zip(a.iters, b.iters)), (a.iters, b.iters)


# ------------------------------------------------------------------ 2. Sim3Solver

def test_sim3_hypotheses_around_the_lds_tile_the_mask_words_and_the_groups():
    """tests/test_gpu_sim3.py's comparison (masks equal outside the model's threshold band, counts equal to the masks' sums -- no bit
    beyond n in a partial last word --, T12 within 4 x the model's band) at n = 63 ... 2049 and H = 15 / 16 / 17."""
    decisions, left_out, hyps, low_gap, nan_hyps = ts._compare_hypotheses(pb.SIM3_HYP_CASES)
    print("decisions %d, left out %d (%.4f %%); hypotheses %d, gap < 0.01: %d, NaN: %d" % (
        decisions, left_out, 100.0 * left_out / decisions, hyps, low_gap, nan_hyps))
    assert left_out <= 1e-3 * decisions
    assert low_gap <= 0.05 * hyps


def test_sim3_batch_of_problems_on_both_sides_of_the_tile():
    """One orbm_sim3_solve_batch launch over n = 3 / 1024 / 1025 / 2049 with H = 17 / 300 / 16 / 65: every problem's per-hypothesis
    counts, masks and T12 and its outcome equal its single call's, bit for bit (groups beyond a problem's own n_groups return early;
    the problems' mask rows have 1 / 16 / 17 / 33 words)."""
    probs, params, draws = [], [], []
    for n, H, seed in pb.SIM3_BATCH:
        sc = sm.make_scene(seed, n, n % 2 == 0, 0.3)
        probs.append(ts._problem(sc)); params.append(ts._all_params(n, H)); draws.append(api.sim3_draws(n, H, seed + 1))
    batch = api.Sim3Solver.solve_batch(probs, params, draws, per_hypothesis=True)
    for b, (n, H, seed) in enumerate(pb.SIM3_BATCH):
        s = api.Sim3Solver(probs[b])
        s.SetRansacParameters(*params[b])
        assert s.mRansacMaxIts == H
        one = s.iterate(H, draws[b], per_hypothesis=True)
        s.close()
        r = batch[b]
        ts._same(r, one)
        assert r.hyp_masks.shape == (H, n) and r.hyp_T12.shape == (H, 4, 4)
        assert np.array_equal(r.hyp_n_inliers, one.hyp_n_inliers) and np.array_equal(r.hyp_masks, one.hyp_masks), n
        assert r.hyp_T12.tobytes() == one.hyp_T12.tobytes(), n
        assert np.array_equal(r.hyp_n_inliers, r.hyp_masks.sum(axis=1))
        if n > 3:
            assert r.hyp_n_inliers.max() > n // 2


# ------------------------------------------------------------------ 3. OptimizeSim3

@tso.needs_long_double
def test_optimize_sim3_on_the_boundary_family(capsys):
    """255 / 256 / 257 pairs (one pair per thread | a second one in thread 0) and 1023 / 1024 / 1025 (LDS | global memory), both scale
    modes, 30 % wrong matches, judged as tests/test_gpu_sim3_opt.py judges its family; the bands are the float64-vs-long-double
    differences of THESE scenes (sim3_opt_model.measure_entries)."""
    fam = om.measure_entries(pb.sim3_opt_family())
    got, decisions, left_out, worst, lines, failures = tso._judge_family(fam)
    with capsys.disabled():
        print("\nOptimizeSim3 boundary family: %d scenes, %d decisions, %d left out" % (len(got), decisions, left_out))
        for ln in lines:
            print("  " + ln)
        for b in sorted(fam["band_max"]):
            print("  band n_in >= %d, fix_scale %d: device vs model max %.3g, model f64 vs long double max %.3g (tolerance 4 x)" % (
                b[0], b[1], worst.get(b, float("nan")), fam["band_max"][b]))
    assert left_out <= 1e-3 * decisions
    assert not failures, failures
    assert sum(1 for g in got if not g.returned_early and g.nIn >= 10) >= 10


@pytest.mark.parametrize("entry", pb.SIM3_OPT_PAD)
def test_optimize_sim3_lds_path_against_global_path_bit_for_bit(entry):
    """n pairs, and those followed by one inert pair (exact zeros, never removed), which lands in thread 0 behind that thread's own
    pairs: q, t, s, the trace, iters and chi2 bit-equal, removed[:n] equal, nIn larger by one.  1024 -> 1025 moves the problem from the
    LDS_IN = true instantiation to the one that re-reads global memory; 256 -> 257 stays on one path and is the control."""
    p = pb.sim3_opt_pad_problem(entry)
    a = api.OptimizeSim3(tso._api_problem(p))
    b = api.OptimizeSim3(tso._api_problem(pb.sim3_opt_pad_inert(p)))
    n = p.n
    assert not a.returned_early and a.nIn >= 100
    assert np.array_equal(b.removed[:n], a.removed) and b.removed[n] == 0
    assert b.nIn == a.nIn + 1 and b.n_bad_round1 == a.n_bad_round1
    assert a.q.tobytes() == b.q.tobytes() and a.t.tobytes() == b.t.tobytes() and np.float64(a.s).tobytes() == np.float64(b.s).tobytes()
    assert a.trace.tobytes() == b.trace.tobytes() and a.iters == b.iters
    assert np.float64(a.chi2).tobytes() == np.float64(b.chi2).tobytes()


# ------------------------------------------------------------------ 4. frames above 4096 features

def _same_search(g, o, what):
    assert g[-1] == o[-1], (what, g[-1], o[-1])
    for a, b in zip(g[:-1], o[:-1]):
        if b is not None:
            assert np.array_equal(a, b), what


def _device_runs(c, F, amp, aob, res):
    """Every device form of the case's entry point on the occupancy (amp, aob): [(name, (assigned_mp, assigned_obs or None, count))]."""
    e = c.entry
    if e == "mps":
        return [("orbm_search_by_projection_mps", api.ORBmatcher(0.8).SearchByProjection(F, c.mv, 3.0, True, 4.0, amp, aob))]
    if e == "local":
        m = api.ORBmatcher(0.8)
        vis = np.zeros(len(c.skip), np.uint8)
        out = [("orbm_search_local_points_vis", m.SearchLocalPoints(F, res["LM"], c.T, 3.0, False, 0.0, amp, aob, c.skip, in_frustum=vis))]
        assert np.array_equal(vis, c.want_vis) and vis.sum() > 100
        a, b, cnt = amp.copy(), aob.copy(), C.c_int(0)
        T = np.ascontiguousarray(c.T, np.float32).reshape(16)
        vp = lambda x: C.c_void_p(x.ctypes.data)                          # (the symbol has no argtypes: a bare int would be cut to 32 bits)
        capi.check(capi.load().orbm_search_local_points(F.h, res["LM"].h, vp(T), vp(c.skip), C.c_float(3.0), 0, C.c_float(0.0), C.c_float(0.8),
                                                        vp(a), vp(b), C.byref(cnt)), "orbm_search_local_points")
        return out + [("orbm_search_local_points", (a, b, cnt.value))]
    if e == "frame":
        m = api.ORBmatcher(0.9, True)
        return [("orbm_search_by_projection_frame", m.SearchByProjectionFrame(F, c.T, c.lv, 7.0, False, amp, aob)),
                ("orbm_search_by_projection_frame_resident", m.SearchByProjectionFrameResident(F, c.T, res["LV"], 7.0, False, amp, aob))]
    if e == "reloc":
        a, cnt = api.ORBmatcher(0.75, True).SearchByProjectionReloc(F, c.T, res["KP"], c.kf_angle, amp, 10.0, 100, c.found)
        return [("orbm_search_by_projection_reloc", (a, None, cnt))]
    a, cnt = api.ORBmatcher(0.75, True).SearchByProjectionSim3(F, c.S, res["LM"], amp, 8, 1.5, c.found, False)
    return [("orbm_search_by_projection_sim3", (a, None, cnt))]


@pytest.mark.parametrize("n", fb.FRAME_SIZES)
@pytest.mark.parametrize("entry", fb.ENTRIES)
def test_frame_searches_on_frames_of_more_than_4096_features(scene, entry, n):
    """stage_occupancy's device arrays (n > kOccBits = 4096; 4096 itself is the last frame on the bitmask) under every search that
    stages occupancy, bit-equal to the oracle: nothing assigned; 30 % of the features holding a point (for the entry points that take
    assigned_obs, every such point observed -- what the relocalisation and Sim3 searches mean by passing no assigned_obs at all); and a
    third of those points with 0 observations, which leaves their features free.  The case's own conditions (matches on features beyond
    4096 and 32768, occupancy deciding at least 20 results, the two variants differing) are asserted on the oracle's answers."""
    c = fb.FrameCase(scene, entry, n)
    assert c.check_not_vacuous()
    F = api.Frame().upload(c.fv, c._keep_fv)
    res = {}
    if entry in ("local", "sim3"):
        res["LM"] = api.LocalMap().upload(c.wv)
    if entry == "reloc":
        res["KP"] = api.LocalMap().upload(c.wv)
    if entry == "frame":
        res["LV"] = api.LastFrameOnDevice(1024)
        res["LV"].upload(c.lv)
    variants = [("none", c.none, np.zeros(n, np.int32), c.o_none), ("observed", c.amp0, c.aob_all, c.o_all)]
    if c.has_obs:
        variants.append(("a third unobserved", c.amp0, c.aob_third, c.o_third))
    for name, amp, aob, want in variants:
        for fn, g in _device_runs(c, F, amp, aob, res):
            _same_search(g, want, (fn, n, name))


@pytest.mark.parametrize("size", sorted(fb.RIG_SIZES))
@pytest.mark.parametrize("form", fb.RIG_FORMS)
def test_rig_searches_across_feature_4096(form, size):
    """The two rig forms: left + right = 4097 (global indices cross 4096 inside the right camera; each camera on its bitmask), and a left
    camera of 5000 features (that camera's occupancy in device arrays)."""
    c = fb.RigCase(form, size)
    assert c.check_not_vacuous()
    sc = c.sc
    FL, FR = api.Frame().upload(c.fl, c._keep[0]), api.Frame().upload(c.fr, c._keep[1])
    for name, amp, aob, want in (("none", c.none, np.zeros(c.n, np.int32), c.o_none), ("observed", c.amp0, c.aob_all, c.o_all),
                                 ("a third unobserved", c.amp0, c.aob_third, c.o_third)):
        if form == "mps_rig":
            g = api.ORBmatcher(0.8).SearchByProjectionRig(FL, FR, c.mv, c.mvr, sc["left_to_right"], sc["right_to_left"], 3.0, True, 6.0, amp, aob)
        else:
            g = api.ORBmatcher(0.9, True).SearchByProjectionFrameRig(FL, FR, sc["Tcw"], c.rig, c.lv, 7.0, False, amp, aob)
        _same_search(g, want, (form, size, name))


def test_a_frame_of_65534_features_and_the_refusal_of_65535(scene):
    """ORBG_MAX_FRAME_FEATURES - 1 features upload and answer a search as the oracle does (feature indices up to 65533 in 16 bits next to
    0xFFFF = none); one more is ORBG_CAP_EXCEEDED."""
    c = fb.FrameCase(scene, "mps", 65534)
    assert c.check_not_vacuous()
    new = np.nonzero(c._newly(c.o_all, c.aob_all))[0]
    assert new.max() > 60000
    F = api.Frame().upload(c.fv, c._keep_fv)
    for name, amp, aob, want in (("none", c.none, np.zeros(c.n, np.int32), c.o_none), ("observed", c.amp0, c.aob_all, c.o_all),
                                 ("a third unobserved", c.amp0, c.aob_third, c.o_third)):
        _same_search(api.ORBmatcher(0.8).SearchByProjection(F, c.mv, 3.0, True, 4.0, amp, aob), want, name)
    fr = fb.big_frame(scene, 5, 65535, 5)
    p = scene.frame_view_params()
    fv, keep = views.frame_view(fr["kps"], fr["desc"], fr["uright"], fr["depth"], p["bounds"], p["cam"], 8, 1.2)
    assert capi.load().orbm_frame_upload(F.h, C.byref(fv)) == capi.ORBG_CAP_EXCEEDED
    # the refused upload left the frame as it was
    _same_search(api.ORBmatcher(0.8).SearchByProjection(F, c.mv, 3.0, True, 4.0, c.amp0, c.aob_all), c.o_all, "after the refusal")
