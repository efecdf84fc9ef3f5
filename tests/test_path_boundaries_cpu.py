"""What tests/test_gpu_path_boundaries.py rests on, checked without a device: the oracle and the numpy models alone on the inputs of
tests/path_boundary_cases.py."""
import time

import numpy as np
import pytest

import frame_boundary_cases as fb
import path_boundary_cases as pb
import sim3_opt_model as om
from oracle import binding as ob


# ------------------------------------------------------------------ 1. PoseOptimization

@pytest.mark.parametrize("n,k", pb.POSE_PAD)
def test_oracle_pose_optimization_ignores_inert_correspondences(n, k):
    """Seeds pose_seed(512) = 7512 and pose_seed(1024) = 8024, pad seeds 977 + k: the oracle's answer with k inert correspondences
    appended is its answer without them -- flags, iterations, chi2 (appended zeros leave a serial sum as it was) and pose."""
    pr = pb.pose_problem(n)
    a = ob.pose_optimize(pb.pose_view(pr)[0])
    padded = pb.pose_pad_inert(pr, k)
    assert len(padded["u"]) == n + k and (padded["inv_sigma2"][n:] == 0).all() and (padded["ur"][n:] < 0).any() and (padded["ur"][n:] >= 0).any() == (k > 1)
    b = ob.pose_optimize(pb.pose_view(padded)[0])
    assert np.array_equal(b.outliers[:n], a.outliers) and not b.outliers[n:].any() and b.n_inliers == a.n_inliers + k
    assert a.iters == b.iters and a.chi2 == b.chi2
    assert np.abs(a.Tcw.astype(np.float64) - b.Tcw.astype(np.float64)).max() <= 1e-12
    assert 0.05 * n < a.outliers.sum() < 0.2 * n and min(a.iters) >= 3              # a real problem: four rounds, outliers told apart


def test_pose_boundary_problems_are_what_the_device_tests_need():
    """Every size has its outliers and its monocular part (from 63 on), every round of the oracle runs, and the three-point problem is
    monocular throughout and ends after one round."""
    for n in pb.POSE_N:
        pr = pb.pose_problem(n)
        o = ob.pose_optimize(pb.pose_view(pr)[0])
        assert len(pr["u"]) == n
        if n >= 63:
            assert 0 < o.outliers.sum() < n // 4 and (pr["ur"] < 0).any() and (pr["ur"] >= 0).any() and min(o.iters) >= 3
    for n in pb.POSE_RIG_N:
        nl, nr = pb.pose_rig_split(n)
        assert nl + nr == n and nr > 0
        pr = pb.pose_rig_problem(n)
        assert len(pr["u"]) == n and int((pr["ur"] < -1.5).sum()) == nr
    pr = pb.pose_problem(3, mono_frac=1.0, outlier_frac=0.0)
    o = ob.pose_optimize(pb.pose_view(pr)[0])
    assert (pr["ur"] < 0).all() and o.iters[0] > 0 and o.iters[1:] == (0, 0, 0) and o.n_inliers == 3


# ------------------------------------------------------------------ 2. Sim3Solver

def test_sim3_boundary_cases_leave_out_at_most_a_thousandth_of_the_decisions(capsys):
    """The float64 model alone on the chosen seeds (900 ... 909 at H = 65, 921 ... 923 at n = 1025): decisions within a relative 1e-3
    of their threshold.  Recorded: 51 of 677 295 (0.0075 %)."""
    ns = sorted(set(c[0] for c in pb.SIM3_HYP_CASES))
    assert ns == [63, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049]
    assert sorted(c[4] for c in pb.SIM3_HYP_CASES if c[4] != 65) == [15, 16, 17]
    assert {c[1] for c in pb.SIM3_HYP_CASES if c[0] >= 1023 and c[4] == 65} == {True, False}     # both scale modes around the tile
    decisions, near = pb.sim3_left_out(pb.SIM3_HYP_CASES)
    with capsys.disabled():
        print("\nsim3 boundary cases: %d decisions, %d within 1e-3 of a threshold (%.4f %%)" % (decisions, near, 100.0 * near / decisions))
    assert decisions == sum(c[0] * c[4] for c in pb.SIM3_HYP_CASES)
    assert near <= 1e-3 * decisions


# ------------------------------------------------------------------ 3. OptimizeSim3

@pytest.mark.skipif(not om.LONGDOUBLE_OK, reason="numpy.longdouble is not the 80-bit format here")
def test_sim3_opt_boundary_family_in_both_precisions(capsys):
    """The boundary family in float64 and long double: what the device test is judged against.  No scene is ill-conditioned, at most
    0.1 % of the decisions lie within 1e-3 of th2, and the two precisions agree on every decision outside that band.  The CPU time is
    printed (recorded: 2 s for the twelve scenes, so both scale modes stay at every size)."""
    t0 = time.process_time()
    fam = om.measure_entries(pb.sim3_opt_family())
    cpu = time.process_time() - t0
    decisions = sum(s["cmp"]["decisions"] for s in fam["scenes"])
    left_out = sum(s["cmp"]["left_out"] for s in fam["scenes"])
    with capsys.disabled():
        print("\nOptimizeSim3 boundary family: %d scenes, %.1f s of CPU, %d decisions, %d left out" % (len(fam["scenes"]), cpu, decisions, left_out))
        for s in fam["scenes"]:
            print("  %-30s band %-12s n_in %4d  f64 vs long double %.3g" % (s["entry"], s["band"], s["ld"]["n_in"], s["diff"]))
        for b in sorted(fam["band_max"]):
            print("  band n_in >= %d, fix_scale %d: %.3g" % (b[0], b[1], fam["band_max"][b]))
    assert [s["entry"][1] for s in fam["scenes"]] == [255, 255, 256, 256, 257, 257, 1023, 1023, 1024, 1024, 1025, 1025]
    assert all(s["cmp"]["equal"] for s in fam["scenes"]) and not any(s["ill"] for s in fam["scenes"])
    assert left_out <= 1e-3 * decisions
    assert sum(1 for s in fam["scenes"] if not s["ld"]["returned_early"] and s["ld"]["n_in"] >= 10) >= 10


@pytest.mark.parametrize("entry", pb.SIM3_OPT_PAD)
def test_sim3_opt_model_ignores_an_inert_pair(entry):
    """The float64 model with and without the inert pair: same removed flags, same trace, the same estimate to the bit, n_in + 1."""
    p = pb.sim3_opt_pad_problem(entry)
    q = pb.sim3_opt_pad_inert(p)
    assert q.n == p.n + 1 and q.n_corr == p.n_corr + 1 and q.w1[-1] == 0 and q.w2[-1] == 0 and q.X1[-1, 2] > 0 and q.X2[-1, 2] > 0
    a, b = om.optimize_sim3(p), om.optimize_sim3(q)
    assert not a["returned_early"] and a["n_in"] >= 100
    assert np.array_equal(a["removed"], b["removed"][:-1]) and b["removed"][-1] == 0 and b["n_in"] == a["n_in"] + 1
    assert om.est_diff(a, b) == 0.0 and a["trace"] == b["trace"]


# ------------------------------------------------------------------ 4. frames above 4096 features

def test_big_frame_builder(scene):
    """The real features of a filled-up frame sit on both sides of index 4096 and of 32768, every feature lies inside the bounds, the
    synthetic ones have no right coordinate, and the oracle's grid holds every feature once."""
    fr = fb.big_frame(scene, 5, 40000, 45000)
    real = np.nonzero(fr["real"])[0]
    assert 500 < len(real) < 3500
    assert (real < 4096).sum() >= 50 and ((real >= 4096) & (real < 32768)).sum() >= 300 and (real >= 32768).sum() >= 100
    k = fr["kps"]
    assert (k["x"] >= 0).all() and (k["x"] < scene.W).all() and (k["y"] >= 0).all() and (k["y"] < scene.H).all()
    assert k["octave"].min() == 0 and k["octave"].max() == 7
    assert (fr["uright"][~fr["real"]] == -1).all() and (fr["uright"][fr["real"]] >= 0).sum() > 100
    p = scene.frame_view_params()
    fv, keep = fb.views.frame_view(k, fr["desc"], fr["uright"], fr["depth"], p["bounds"], p["cam"], 8, 1.2)
    start, items = ob.build_grid(fv)
    m = int(start[-1])                                                     # (PosInGrid rounds: features in the last half cell of a row or column fall outside)
    assert 0.97 * 40000 < m <= 40000 and len(np.unique(items[:m])) == m
    amp, aob_all, aob_third = fb.occupancy(40000, 1)
    assert amp[4096] == -1 and ((amp >= 0) == (aob_all > 0)).all() and ((aob_third == 0) | (aob_third == aob_all)).all()


@pytest.mark.parametrize("n", fb.FRAME_SIZES)
@pytest.mark.parametrize("entry", fb.ENTRIES)
def test_big_frame_cases_are_not_vacuous(scene, entry, n):
    """The oracle's answers on every case of the device test: matches on features beyond 4096 (and 32768), occupancy deciding at least 20
    results, the two assigned_obs variants differing."""
    assert fb.FrameCase(scene, entry, n).check_not_vacuous()


@pytest.mark.parametrize("size", sorted(fb.RIG_SIZES))
@pytest.mark.parametrize("form", fb.RIG_FORMS)
def test_big_rig_cases_are_not_vacuous(form, size):
    assert fb.RigCase(form, size).check_not_vacuous()


def test_largest_frame_case_is_not_vacuous(scene):
    c = fb.FrameCase(scene, "mps", 65534)
    assert c.check_not_vacuous() and np.nonzero(c._newly(c.o_all, c.aob_all))[0].max() > 60000
