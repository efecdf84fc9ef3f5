"""tests/weld_ba_model.py, the float64 restatement of the welding BA that tests/test_gpu_weld_ba.py holds ba_weld_solve against, pinned on
the CPU: its round against tests/full_ba_model.py, the invariants of the two rounds on every case, the two conditions on the committed
inputs that keep an edge's level from depending on the last bits, each case's own property, and what reordering every sum moves."""
import numpy as np
import pytest

import full_ba_cases as fc
import full_ba_model as fm
import weld_ba_cases as wc
import weld_ba_model as wm

NAMES = sorted(wc.CASES)


@pytest.mark.parametrize("name", ["loop_closing", "one_camera"])
def test_round_with_every_edge_active_equals_the_full_ba_model(name):
    _, its, robust = fc.CASES[name]
    pr = fc.problem(name)
    m = fc.model(name)
    r = wm.solve_round(pr, wm.state_from_float32(pr), np.ones(len(pr["edges"]), bool), robust, its)
    assert r.iters == m.iters and np.array_equal(r.trace[:, 2], m.trace[:, 2])
    rel = np.abs(r.trace[:, :2] - m.trace[:, :2]) / np.abs(m.trace[:, :2])
    dp, dx = np.abs(wm.poses64(r.state) - m.poses64).max(), np.abs(r.state.X.astype(np.float32) - m.points).max()
    print("trace %.3g poses %.3g points %.3g" % (rel.max(), dp, dx))
    assert rel.max() <= 1e-15 and dp <= 1e-15 and dx == 0
    assert r.chi2_initial == m.chi2_initial and abs(r.chi2_final - m.chi2_final) <= 1e-15 * m.chi2_final
    assert np.allclose(r.edge_chi2, m.edge_chi2, rtol=1e-15, atol=0)


@pytest.mark.parametrize("name", NAMES)
def test_two_round_invariants(name):
    pr, m = wc.problem(name), wc.model(name)
    e = pr["edges"]
    assert m.iters > 0 and m.rounds_run == 2 and m.iters_second > 0
    lvl1 = m.edge_level == 1
    # a level-1 edge was not active in round 2: chi2 of round 1's last evaluation
    assert np.array_equal(m.edge_chi2[lvl1], m.chi2_round1[lvl1])
    assert np.isfinite(m.edge_chi2).all()
    if lvl1.any() and name != "weld_clean":
        assert not np.array_equal(m.edge_chi2[~lvl1], m.chi2_round1[~lvl1])
    # a point without a level-0 edge keeps round 1's position; so does a free keyframe
    kept_points = np.zeros(len(pr["points"]), bool); kept_points[e["point"][~lvl1]] = True
    assert np.array_equal(m.state.X[~kept_points], m.state_round1.X[~kept_points])
    kept_poses = np.zeros(len(pr["poses"]), bool); kept_poses[e["pose"][~lvl1]] = True
    for i in np.flatnonzero(~kept_poses | (pr["pose_fixed"] != 0)):
        assert np.array_equal(m.state.q[i], m.state_round1.q[i]) and np.array_equal(m.state.t[i], m.state_round1.t[i])
    assert m.second.active_free == [i for i in range(len(pr["poses"])) if kept_poses[i] and not pr["pose_fixed"][i]]
    # lambda's first value of round 2: 1e-5 x the largest diagonal entry over the ACTIVE vertices, level-0 edges only, no kernels.
    # Recomputed here from the oracle's Jacobians at round 1's state
    s = m.state_round1
    md = 0.0
    Hpp = {}; Hll = {}
    for k in np.flatnonzero(~lvl1):
        i, l = int(e["pose"][k]), int(e["point"][k])
        five = np.array([np.float32(c) for c in pr["cameras"][pr["pose_camera"][i]][:5]], np.float32)
        err, A, B = wm.ob.lba_edge_eval(s.q[i], s.t[i], s.X[l], five, e[k:k + 1])
        D = 2 if e["ur"][k] < 0 else 3
        om = float(e["inv_sigma2"][k])
        if not pr["pose_fixed"][i]:
            Hpp[i] = Hpp.get(i, 0) + om * (B[:D] ** 2).sum(axis=0)
        Hll[l] = Hll.get(l, 0) + om * (A[:D] ** 2).sum(axis=0)
    for v in list(Hpp.values()) + list(Hll.values()):
        md = max(md, float(np.max(v)))
    assert abs(m.max_diagonal_second - md) <= 1e-12 * md
    assert m.lambda_first_second == 1e-5 * m.max_diagonal_second


@pytest.mark.parametrize("name", NAMES)
def test_no_level_depends_on_the_last_bits(name):
    """The product's edge chi2 is held to 1e-6: no round-1 chi2 of a committed input may lie within 1e-3 relative of its threshold,
    and no depth a depth test reads within 1e-3 of zero.  (A seed that violates this is changed, not the bound.)"""
    pr, m = wc.problem(name), wc.model(name)
    th = np.where(pr["edges"]["ur"] < 0, wm.CHI2_MONO, wm.CHI2_STEREO)
    gap = np.abs(m.chi2_round1 - th) / th
    print("closest chi2 to its threshold: %.3g relative; final check %.3g; smallest |depth| %.3g / %.3g" %
          (gap.min(), (np.abs(m.edge_chi2 - th) / th).min(), np.abs(m.depth_round1).min(), np.abs(m.depth_final).min()))
    assert gap.min() > 1e-3
    assert (np.abs(m.edge_chi2 - th) / th).min() > 1e-3          # the final check uses the same thresholds
    assert np.abs(m.depth_round1).min() > 1e-3 and np.abs(m.depth_final).min() > 1e-3


def test_cases_have_the_properties_they_exist_for():
    pr, m = wc.problem("weld_small"), wc.model("weld_small")
    e = pr["edges"]
    assert (pr["pose_fixed"] != 0).sum() == 3 and (pr["pose_fixed"] == 0).sum() == 5 and len(pr["points"]) == 90
    assert (e["ur"] < 0).any() and (e["ur"] >= 0).any() and len(set(pr["pose_camera"][e["pose"]].tolist())) == 2
    assert 0 < m.n_level1 < len(e) // 4 and len(m.to_erase) > 0
    assert (m.edge_level[e["ur"] < 0] == 1).any() and (m.edge_level[e["ur"] >= 0] == 1).any()
    # to_erase: the monocular edges first, then the stereo ones, each ascending
    te = m.to_erase
    nm = int((e["ur"][te] < 0).sum())
    assert 0 < nm < len(te) and (e["ur"][te[:nm]] < 0).all() and (e["ur"][te[nm:]] >= 0).all()
    assert (np.diff(te[:nm]) > 0).all() and (np.diff(te[nm:]) > 0).all()

    pr, m = wc.problem("weld_points_only"), wc.model("weld_points_only")
    assert (pr["pose_fixed"][pr["edges"]["pose"]] != 0).all() and (pr["pose_fixed"] == 0).sum() == 5
    assert m.first.active_free == [] and m.second.active_free == [] and m.n_level1 > 0
    assert not m.point_included.all() and m.point_included.sum() > 20
    assert np.array_equal(m.poses64.astype(np.float32).reshape(-1, 16)[:, :12], wm.poses64(wm.state_from_float32(pr)).astype(np.float32).reshape(-1, 16)[:, :12])

    pr, m = wc.problem("weld_dropped"), wc.model("weld_dropped")
    e = pr["edges"]
    gone = pr["dropped_points"]
    assert set(wc.DROPPED_POINTS) <= set(gone.tolist())
    for j in gone:
        assert (e["point"] == j).sum() >= 2 and (m.edge_level[e["point"] == j] == 1).all()
    assert (e["pose"] == wc.DROPPED_POSE).sum() > 10 and (m.edge_level[e["pose"] == wc.DROPPED_POSE] == 1).all()
    assert wc.DROPPED_POSE not in m.second.active_free and len(m.second.active_free) == 4
    k = pr["behind_edge"]
    assert e["pose"][k] == len(pr["poses"]) - 1 and e["point"][k] == pr["behind_point"]
    # below its threshold by a wide margin, level 1 by the depth test alone; in the final check: round 1's chi2, the final depth
    assert m.chi2_round1[k] < 0.5 * wm.CHI2_MONO and m.depth_round1[k] < -1.0 and m.edge_level[k] == 1
    assert m.edge_chi2[k] == m.chi2_round1[k] and m.edge_depth_pos[k] == 0 and k in m.to_erase
    assert m.depth_final[k] != m.depth_round1[k]                   # (the point moved in round 2: the depth test is a fresh one)

    pr, m = wc.problem("weld_clean"), wc.model("weld_clean")
    assert m.n_level1 == 0 and not m.edge_level.any() and len(m.to_erase) == 0

    pr, m = wc.problem("weld_1100"), wc.model("weld_1100")
    n = len(pr["edges"])
    assert n > 1024 and n % 256 != 0 and 0 < m.n_level1 and n - m.n_level1 > 1024


@pytest.mark.parametrize("name", NAMES)
def test_every_case_is_comparable(name):
    """What two float64 implementations can be held to on this input: no point of round 2 is a ray (one monocular level-0 edge and
    nothing else), and reversing every sum of the model -- a stand-in for another implementation's rounding -- moves no edge's chi2 by
    more than 1e-7, a tenth of the GPU test's bound, and no level, count or depth test at all.  (The stereo projection rounds the
    inverse depth to float32: a rounding that falls differently moves a residual by about 3e-5 px at once.  An input on which that
    happens within the iterations of its case is replaced by another seed.)"""
    pr, a, b = wc.problem(name), wc.model(name), wc.model(name, True)
    e = pr["edges"]
    l0 = a.edge_level == 0
    n0 = np.bincount(e["point"][l0], minlength=len(pr["points"]))
    st = np.bincount(e["point"][l0 & (e["ur"] >= 0)], minlength=len(pr["points"]))
    assert not ((n0 == 1) & (st == 0)).any()
    d = np.abs(a.edge_chi2 - b.edge_chi2).max()
    print("%s: edge chi2 forward against reversed %.3g" % (name, d))
    assert d <= 1e-7
    assert np.array_equal(a.edge_level, b.edge_level) and np.array_equal(a.edge_depth_pos, b.edge_depth_pos)
    assert np.array_equal(a.point_included, b.point_included) and (a.rounds_run, a.iters, a.iters_second) == (b.rounds_run, b.iters, b.iters_second)


def test_stop_forms_of_the_model():
    full = wc.model("weld_small")
    k1 = int(full.trace[:, 2].sum())
    a = wc.model("weld_small", False, 2)                           # inside round 1
    assert a.rounds_run == 1 and a.iters == 2 and not a.edge_level.any() and a.n_level1 == 0 and a.second is None
    assert np.array_equal(a.edge_chi2, a.chi2_round1)
    b = wc.model("weld_small", False, k1 + 3)                      # inside round 2
    assert b.rounds_run == 2 and b.iters == full.iters and b.iters_second == 3 and np.array_equal(b.edge_level, full.edge_level)
    c = wc.model("weld_small", False, None, True)                  # before the call
    pr = wc.problem("weld_small")
    assert c.rounds_run == 0 and c.iters == 0 and c.status == 1 and np.array_equal(c.points, pr["points"]) and not c.edge_chi2.any()
    d = wc.model("weld_small", False, None, False, 0)              # no second round asked for
    assert d.rounds_run == 1 and np.array_equal(d.edge_level, full.edge_level) and np.array_equal(d.edge_chi2, d.chi2_round1)


@pytest.mark.parametrize("name", NAMES)
def test_reordered_sums_bound_the_traces(name):
    a, b = wc.model(name), wc.model(name, True)
    assert a.iters == b.iters and a.iters_second == b.iters_second
    assert np.array_equal(a.trace[:, 2], b.trace[:, 2]) and np.array_equal(a.trace_second[:, 2], b.trace_second[:, 2])
    assert np.array_equal(a.edge_level, b.edge_level) and np.array_equal(a.to_erase, b.to_erase)
    ta, tb = np.vstack([a.trace, a.trace_second]), np.vstack([b.trace, b.trace_second])
    rel = np.abs(ta[:, :2] - tb[:, :2]) / np.abs(ta[:, :2])
    print("%s forward against reversed: lambda %.3g chi2 %.3g poses %.3g points %.3g" %
          (name, rel[:, 0].max(), rel[:, 1].max(), np.abs(a.poses64 - b.poses64).max(), np.abs(a.state.X - b.state.X).max()))
    # the figures written into weld_ba_cases.REORDER_MEASURED are these, within the last digit given there
    lam, chi = wc.REORDER_MEASURED[name]
    assert rel[:, 0].max() <= lam * 1.01 + 1e-300 and rel[:, 1].max() <= chi * 1.01 + 1e-300
    assert np.abs(a.poses64 - b.poses64).max() <= 1e-6 and np.abs(a.state.X - b.state.X).max() <= 1e-6
