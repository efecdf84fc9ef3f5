"""The welding BA of LoopClosing::MergeLocal on the GPU (ba_weld_solve_h, csrc/full_ba.hip) against tests/weld_ba_model.py on the
problems of tests/weld_ba_cases.py, whose conditioning tests/test_weld_ba_cpu.py checks.  Bounds, the project's own: levels, to_erase,
rounds_run, iteration and trial counts, point_included and edge_depth_pos equal; poses and points 1e-4 after the float32 write-back;
lambda and chi2 of both traces max(1e-9, 10 x what reversing every sum of the model moves them by); edge chi2 rtol 1e-6 / atol 1e-6."""
import numpy as np
import pytest

import full_ba_cases as fc
import weld_ba_cases as wc
from multi_orbslam3_amd import api, views

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-4
INT32_MIN = np.iinfo(np.int32).min


@pytest.fixture(scope="module")
def opt():
    o = api.Optimizer()
    yield o
    o.close()


def _view(name, iterations=None, iterations_second=None):
    pr = wc.problem(name)
    _, its, its2 = wc.CASES[name]
    return views.ba_weld_problem(pr["poses"], pr["pose_fixed"], pr["pose_camera"], pr["points"], pr["edges"], pr["cameras"],
                                 iterations=its if iterations is None else iterations,
                                 iterations_second=its2 if iterations_second is None else iterations_second)


def _solve(opt, name, stop=None, iterations_second=None):
    p, keep = _view(name, iterations_second=iterations_second)
    return opt.MergeLocalBundleAdjustment(p, pbStopFlag=stop)


def _assert_trace(rows, want, rtol, what):
    print("%s: trials %s / %s" % (what, rows[:, 2].tolist(), want[:, 2].tolist()))
    assert len(rows) == len(want) and np.array_equal(rows[:, 2], want[:, 2])
    if len(rows):
        rel = np.abs(rows[:, :2] - want[:, :2]) / np.abs(want[:, :2])
        print("%s: largest relative difference of lambda %.3g, of chi2 %.3g (bound %.3g)" % (what, rel[:, 0].max(), rel[:, 1].max(), rtol))
        assert rel.max() <= rtol


def _assert_equals_model(out, m, rtol):
    print("rounds %d / %d, iters %d + %d / %d + %d, level 1: %d / %d" %
          (out.rounds_run, m.rounds_run, out.iters, out.iters_second, m.iters, m.iters_second, out.n_level1, m.n_level1))
    assert out.status == m.status
    assert out.rounds_run == m.rounds_run and out.iters == m.iters and out.iters_second == m.iters_second
    assert np.array_equal(out.edge_level, m.edge_level) and out.n_level1 == m.n_level1
    _assert_trace(out.trace_rows(), m.trace, rtol, "round 1")
    _assert_trace(out.trace_second_rows(), m.trace_second, rtol, "round 2")
    for got, want in ((out.chi2[0], m.chi2_initial), (out.chi2[1], m.chi2_final), (out.chi2_second[0], m.chi2_initial_second),
                      (out.chi2_second[1], m.chi2_final_second)):
        assert abs(got - want) <= rtol * abs(want)
    dp, dx = np.abs(out.poses - m.poses).max(), np.abs(out.points - m.points).max()
    print("poses %.3g points %.3g, edge chi2 %.3g" % (dp, dx, np.abs(out.edge_chi2 - m.edge_chi2).max() if len(m.edge_chi2) else 0.0))
    assert dp <= STATE_TOL and dx <= STATE_TOL
    assert np.isfinite(out.poses).all() and np.isfinite(out.points).all()
    assert np.array_equal(out.point_included, m.point_included)
    assert np.array_equal(out.edge_depth_pos, m.edge_depth_pos)
    assert np.allclose(out.edge_chi2, m.edge_chi2, rtol=1e-6, atol=1e-6)
    assert np.array_equal(out.to_erase, m.to_erase)


@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_equals_the_model(opt, name):
    out = _solve(opt, name)
    m = wc.model(name)
    _assert_equals_model(out, m, wc.trace_rtol(name))
    assert out.rounds_run == 2 and out.iters_second > 0
    pr = wc.problem(name)
    if name == "weld_clean":
        assert out.n_level1 == 0 and not out.edge_level.any()
    if name == "weld_points_only":
        free = pr["pose_fixed"] == 0
        first = _solve(opt, name, iterations_second=0)
        assert np.array_equal(out.poses[free], first.poses[free])            # nP = 0 in both rounds: no free pose is touched
    if name == "weld_dropped":
        # what left round 2 entirely keeps round 1's estimate: the points to the bit, the keyframe up to the renormalisation of its
        # unit quaternion by a zero step (an ulp of float64 before the float32 write-back: one float32 ulp of entries below 4)
        first = _solve(opt, name, iterations_second=0)
        gone = pr["dropped_points"]
        assert len(gone) >= len(wc.DROPPED_POINTS) and out.edge_level[np.isin(pr["edges"]["point"], gone)].all()
        assert np.array_equal(out.points[gone], first.points[gone])
        assert np.abs(out.poses[wc.DROPPED_POSE] - first.poses[wc.DROPPED_POSE]).max() <= 2.4e-7
        kept = np.setdiff1d(np.unique(pr["edges"]["point"][out.edge_level == 0]), gone)
        assert np.abs(out.points[kept] - first.points[kept]).max() > 1e-6
        k = pr["behind_edge"]                                                 # level 1 by its depth alone; the stale chi2, the fresh depth
        assert out.edge_level[k] == 1 and out.edge_chi2[k] < 3.0 and out.edge_depth_pos[k] == 0 and k in out.to_erase
        assert out.edge_chi2[k] == first.edge_chi2[k]
    if name == "weld_1100":
        assert len(pr["edges"]) > 1024 and len(pr["edges"]) % 256 != 0


def test_round_one_alone_has_the_bits_of_the_full_ba():
    pr = wc.problem("weld_small")
    h = api.FullBA()
    p, keep = _view("weld_small", iterations_second=0)
    w = h.weld(p)
    pb, keepb = views.ba_problem(pr["poses"], pr["pose_fixed"], pr["pose_camera"], pr["points"], pr["edges"], pr["cameras"], iterations=5,
                                 robust=True)
    b = h.solve(pb)
    h.close()
    assert w.rounds_run == 1 and w.iters_second == 0 and w.iters == b.iters > 0 and len(w.trace_second_rows()) == 0
    for f in ("poses", "points", "edge_chi2", "edge_depth_pos", "point_included", "trace"):
        assert np.array_equal(getattr(w, f), getattr(b, f)), f
    assert w.chi2 == b.chi2
    assert np.array_equal(w.edge_level, wc.model("weld_small").edge_level)    # the levels are still assigned


def test_the_problems_robust_field_is_not_read(opt):
    p, keep = _view("weld_small")
    a = opt.MergeLocalBundleAdjustment(p)
    p.ba.robust = 0
    b = opt.MergeLocalBundleAdjustment(p)
    _assert_same_bits(a, b)


def test_stop_forms(opt):
    name = "weld_small"
    pr = wc.problem(name)
    full = wc.model(name)
    k1 = int(full.trace[:, 2].sum())
    # after 2 trials: inside round 1 -- no level, no second round
    out = _solve(opt, name, stop=np.array([-2], np.int32))
    _assert_equals_model(out, wc.model(name, False, 2), wc.trace_rtol(name))
    assert out.rounds_run == 1 and out.iters == 2 and not out.edge_level.any()
    # after round 1's trials and three more: inside round 2
    out = _solve(opt, name, stop=np.array([-(k1 + 3)], np.int32))
    _assert_equals_model(out, wc.model(name, False, k1 + 3), wc.trace_rtol(name))
    assert out.rounds_run == 2 and out.iters_second == 3
    # before the call, both flag types: nothing launched, the input comes back
    for flag in (np.array([1], np.int32), np.array([1], np.uint8)):
        out = _solve(opt, name, stop=flag)
        assert out.status == 1 and out.rounds_run == 0 and out.iters == 0 and out.iters_second == 0     # LBA_ABORTED_BEFORE_OPT
        assert np.abs(out.poses - pr["poses"]).max() <= 1e-6 and np.array_equal(out.points, pr["points"])
        assert not out.edge_level.any() and not out.edge_chi2.any() and len(out.to_erase) == (out.edge_depth_pos == 0).sum()
    out = _solve(opt, name, stop=np.array([INT32_MIN], np.int32))
    assert out.status == 0 and out.rounds_run == 0 and np.array_equal(out.points, pr["points"])
    # a flag that stays down, as a byte: the bits of the call without a flag
    _assert_same_bits(_solve(opt, name), _solve(opt, name, stop=np.zeros(1, np.uint8)))


def _assert_same_bits(a, b):
    for f in ("poses", "points", "edge_chi2", "edge_depth_pos", "point_included", "edge_level", "trace", "trace_second"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.chi2 == b.chi2 and a.chi2_second == b.chi2_second and (a.iters, a.iters_second, a.rounds_run, a.n_level1) == (
        b.iters, b.iters_second, b.rounds_run, b.n_level1)
    assert np.array_equal(a.to_erase, b.to_erase)


def test_two_calls_return_the_same_bits():
    for name in ("weld_small", "weld_1100"):
        p, keep = _view(name)
        h = api.FullBA()
        a, b = h.weld(p), h.weld(p)
        h.close()
        h2 = api.FullBA()
        c = h2.weld(p)
        h2.close()
        assert a.rounds_run == 2 and a.iters_second > 0, name
        _assert_same_bits(a, b)
        _assert_same_bits(a, c)


def test_a_full_ba_after_a_weld_on_the_same_handle_equals_a_fresh_handles():
    """The weld exchanges the handle's edge and chi2 buffers with the level-0 ones while round 2 runs, and leaves round 2's structure
    behind: none of it may reach a later ba_solve_h."""
    _, its, robust = fc.CASES["loop_closing"]
    pr = fc.problem("loop_closing")
    pb, keepb = views.ba_problem(pr["poses"], pr["pose_fixed"], pr["pose_camera"], pr["points"], pr["edges"], pr["cameras"], iterations=its,
                                 robust=robust)
    h = api.FullBA()
    for name in ("weld_1100", "weld_dropped"):
        assert h.weld(_view(name)[0]).rounds_run == 2
    after = h.solve(pb)
    h.close()
    h2 = api.FullBA()
    fresh = h2.solve(pb)
    h2.close()
    assert fresh.iters > 0
    for f in ("poses", "points", "edge_chi2", "edge_depth_pos", "point_included", "trace"):
        assert np.array_equal(getattr(after, f), getattr(fresh, f)), f
    assert after.chi2 == fresh.chi2 and after.iters == fresh.iters
