"""OptimizeEssentialGraph on the device (eg_solve through api.OptimizeEssentialGraph) against the float64 model of
tests/essential_graph_model.py, with the float64-vs-long-double distance of tests/test_essential_graph_cpu.py as the yardstick."""
import threading

import numpy as np
import pytest

import essential_graph_model as em
from test_essential_graph_cpu import RING_ITERATIONS, api_arrays, ring_err0_rtol, yardstick
from multi_orbslam3_amd import _capi as capi, api

pytestmark = pytest.mark.gpu
needs_long_double = pytest.mark.skipif(not em.LONGDOUBLE_OK, reason="numpy.longdouble is not wider than float64 here")


def solve(p, **kw):
    V, E, P = api_arrays(p)
    return api.OptimizeEssentialGraph(V, E, P, **kw)


def device_trace(r):
    return [(int(t[0]), int(t[1])) for t in r.trace]


def points_from(p, est):
    """the corrected points a float64 evaluation gives for the estimates `est` (V, 8): S/Optimizer.cc:2732-2740"""
    F = np.float64
    out = np.array(p.pos, np.float32)
    m = p.ref >= 0
    if m.any():
        r = p.ref[m]
        S0, S1 = em._s3(p.q, p.t, p.s, F), em._s3(est[:, :4], est[:, 4:7], est[:, 7], F)
        Y = em.sim3_map(em.sim3_inverse(em._take(S1, r)), em.sim3_map(em._take(S0, r), [p.pos[m, i].astype(F) for i in range(3)]))
        out[m] = np.stack(Y, -1).astype(np.float32)
    return out


def judge(p, ref, ld, band_est, band_pts, label):
    """-> (device result, failures, report line).  Trace equal wherever the two model precisions agree on it; then estimates and
    corrected points within 4 x the band's float64-vs-long-double distance.  Always: the points are the float32 of what the device's
    own estimates map them to, within one float32 ulp (two float64 evaluations of the same expression differ by far less than that and
    can only round to neighbouring floats); points without a reference keep their bits; chi2 at entry at rounding level."""
    g = solve(p)
    fails = []
    models_agree = em.trace_key(ref) == em.trace_key(ld)
    d_est = em.est_diff(g.estimates, ref["est"])
    m = p.ref >= 0
    d_pts = float(np.abs(g.points[m].astype(np.float64) - ref["points"][m].astype(np.float64)).max()) if m.any() else 0.0
    if not abs(g.err0 - float(ref["err0"])) <= 1e-12 * float(ref["err0"]):
        fails.append((label, "err0", g.err0, float(ref["err0"])))
    if models_agree:
        if device_trace(g) != em.trace_key(ref):
            fails.append((label, "trace", device_trace(g), em.trace_key(ref)))
        else:
            if not d_est <= 4 * band_est:
                fails.append((label, "estimates", d_est, 4 * band_est))
            if not d_pts <= 4 * band_pts:
                fails.append((label, "points", d_pts, 4 * band_pts))
            if g.iters != ref["iters"]:
                fails.append((label, "iters", g.iters, ref["iters"]))
    own = points_from(p, g.estimates)
    ulp = np.spacing(np.abs(own)) + np.float32(1e-13)
    if not (np.abs(g.points - own) <= ulp).all():
        fails.append((label, "points vs the device's own estimates", float(np.abs(g.points - own).max())))
    if (~m).any() and g.points[~m].tobytes() != p.pos[~m].tobytes():
        fails.append((label, "a point without a reference changed"))
    fixed_in = np.concatenate([p.q, p.t, p.s[:, None]], axis=1)[p.fixed]
    if g.estimates[p.fixed].tobytes() != fixed_in.tobytes():
        fails.append((label, "a fixed vertex moved"))
    line = "%-28s trace %s%s  |d est| %.3g (4 x %.3g)  |d pts| %.3g (4 x %.3g)  chi2 %.4g -> %.6g" % (
        label, device_trace(g), "" if models_agree else " (models disagree: %s / %s)" % (em.trace_key(ref), em.trace_key(ld)), d_est, band_est, d_pts,
        band_pts, g.err0, g.errEnd)
    return g, fails, line


# ------------------------------------------------------------------ 1. the family

@needs_long_double
def test_device_against_the_float64_model_on_the_family(capsys):
    """Same scene family as the CPU yardstick, judged scene by scene (judge): trace equal wherever the two model precisions agree on
    it, estimates and corrected points within 4 x the float64-vs-long-double distance of the scene's (solver band, scale mode) -- two
    float64 evaluations in different operation orders can each sit that far from the exact value on opposite sides (x 2), and a
    maximum over a few scenes underestimates the population's (x 2).  The measured maxima are printed."""
    fam = yardstick()
    fails, lines, worst = [], [], {}
    for s in fam["scenes"]:
        g, f, line = judge(s["problem"], s["f64"], s["ld"], fam["band_est"][s["band"]], fam["band_pts"][s["band"]], "kf %d fix %d seed %d" % s["entry"])
        fails += f
        lines.append(line)
        if s["same_trace"] and not f:
            worst[s["band"]] = max(worst.get(s["band"], 0.0), em.est_diff(g.estimates, s["f64"]["est"]))
    with capsys.disabled():
        print("\nOptimizeEssentialGraph, device vs float64 model: %d scenes" % len(lines))
        for ln in lines:
            print("  " + ln)
        for b in sorted(fam["band_est"]):
            print("  free keyframes %d .. %d, fix_scale %d: device vs model max %.3g, model f64 vs long double max %.3g (tolerance 4 x)" % (
                b[0][0], b[0][1], b[1], worst.get(b, float("nan")), fam["band_est"][b]))
    assert not fails, fails


# ------------------------------------------------------------------ 2. the error on the four branches of log()

def test_initial_errors_on_the_four_branches_of_log():
    """One free vertex per case against one fixed identity vertex, identity measurement: the edge error is log() of the free vertex's
    estimate.  Cases: sigma exactly 0 with R = I (every non-loop edge of a stereo map at entry), both small branches with values just
    inside, each mixed branch, both large.  Rounding level: the inputs of log()'s library calls are the same bits on both sides (sums
    and products in the same order), the calls themselves differ by a few ulp and are amplified by factors of order 1 / sigma^3 x
    theta^2 <= 1e3 at most here: 1e-12."""
    F = np.float64
    rng = np.random.default_rng(17)
    cases = [("sigma 0, R = I", None)]
    for name, rot, sig in (("both small", 3e-6, 4e-6), ("small rotation", 3e-6, 0.2), ("small sigma", 0.4, 5e-6), ("both large", 0.7, -0.3),
                           ("near pi/2", 1.5, 0.05)):
        w = rng.normal(size=3)
        cases.append((name, np.concatenate([w / np.linalg.norm(w) * rot, rng.normal(size=3), [sig]])))
    q, t, s = [[0, 0, 0, 1.0]], [[0, 0, 0.0]], [1.0]
    for name, u in cases:
        if u is None:
            q.append([0, 0, 0, 1.0]); t.append([0.25, -1.5, 3.0]); s.append(1.0)
        else:
            S = em.sim3_exp(list(u), F)
            q.append([float(v) for v in S[0]]); t.append([float(v) for v in S[1]]); s.append(float(S[2]))
    n = len(cases)
    p = em.Problem(q, t, s, [True] + [False] * n, [False] * (n + 1), list(range(1, n + 1)), [0] * n, [[0, 0, 0, 1.0]] * n, [[0, 0, 0.0]] * n, [1.0] * n)
    g = solve(p, iterations=1)
    ref = em.edge_errors(em._s3(p.mq, p.mt, p.ms, F), em._take(em._s3(p.q, p.t, p.s, F), p.vi), em._take(em._s3(p.q, p.t, p.s, F), p.vj), F)
    assert g.edge_error0[0].tolist() == [0, 0, 0, 0.25, -1.5, 3.0, 0]           # exact
    for k, (name, u) in enumerate(cases):
        assert np.abs(g.edge_error0[k] - ref[k]).max() <= 1e-12 * max(1.0, np.abs(ref[k]).max()), (name, g.edge_error0[k], ref[k])
        if u is not None:
            assert np.abs(g.edge_error0[k] - u).max() <= 1e-9, name               # and log() undoes exp()
    assert abs(g.err0 - float((ref * ref).sum())) <= 1e-12 * float((ref * ref).sum())


# ------------------------------------------------------------------ 3. sizes where the solver changes

def _tile_rows(n):
    """ldltm::make_geo(n).T (csrc/ldlt_mfma.hpp): tile rows of the bordered system"""
    return (((n + 3) & ~3) + 1 + 15) // 16


def solver_limits():
    """Free-keyframe counts on both sides of each solver limit, n = 7 F: ldltm::supports(n) is T <= 19 (one workgroup or, where
    ldltx::supports(n), eight: T >= 9), beyond it launch_ldlt_wide."""
    first_xcd = next(F for F in range(1, 200) if _tile_rows(7 * F) >= 9)
    last_mfma = max(F for F in range(1, 200) if _tile_rows(7 * F) <= 19)
    return sorted({first_xcd - 1, first_xcd, 18, 19, last_mfma, last_mfma + 1, 43, 44})      # (18 | 19 and 43 | 44: the issue's figures)


@needs_long_double
@pytest.mark.parametrize("n_free", [17, 18, 19, 42, 43, 44, 120])
def test_sizes_on_both_sides_of_each_solver_limit(n_free):
    fam = yardstick()
    assert solver_limits() + [120] == [17, 18, 19, 42, 43, 44, 120]
    scenes = [s for s in fam["scenes"] if s["problem"].n_free == n_free]
    assert len(scenes) >= 2                                  # both scale modes
    fails = []
    for s in scenes:
        fails += judge(s["problem"], s["f64"], s["ld"], fam["band_est"][s["band"]], fam["band_pts"][s["band"]], "free %d fix %d" % (n_free, s["entry"][1]))[1]
    assert not fails, fails


@needs_long_double
@pytest.mark.parametrize("env", [{}, {"ORBG_LDLT_WIDE": "1"}, {"ORBG_LDLT_XCD": "safe"}, {"ORBG_LDLT_XCD": "0"}],
                         ids=["default", "wide", "xcd_safe", "xcd_off"])
def test_the_solver_switches_at_the_first_eight_workgroup_size(env, monkeypatch):
    """18 free keyframes, the first size on the eight-workgroup LDL^T, under each value of the two switches of csrc/ldlt_solver.hpp:
    the many-workgroup kernels, the eight-workgroup kernel with its same-L2 and with its agent-scope hand-overs, and the one-workgroup
    kernel in its place.  The work area belongs to the calling thread and reads the variables on that thread's first call: every
    variant runs in a thread of its own.  Judged as the scenes' other tests judge them."""
    fam = yardstick()
    assert solver_limits()[1] == 18
    scenes = [s for s in fam["scenes"] if s["problem"].n_free == 18]
    assert len(scenes) >= 2                                  # both scale modes
    for key in ("ORBG_LDLT_WIDE", "ORBG_LDLT_XCD"):
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    fails, judged, raised = [], [], []

    def work():
        try:
            for s in scenes:
                fails.extend(judge(s["problem"], s["f64"], s["ld"], fam["band_est"][s["band"]], fam["band_pts"][s["band"]],
                                   "free 18 fix %d %s" % (s["entry"][1], env))[1])
                judged.append(s)
        except BaseException as e:                           # (an exception must not end with the thread)
            raised.append(e)

    th = threading.Thread(target=work)
    th.start()
    th.join()
    if raised:
        raise raised[0]
    assert len(judged) == len(scenes) and not fails, fails


# ------------------------------------------------------------------ 4. structure

def _chain(n, rng, fix_scale, noise=0.02):
    """n vertices on a line one metre apart, vertex 0 fixed, estimates disturbed; returns q, t, s lists and the true Sim3s"""
    F = np.float64
    q, t, s = [], [], []
    for i in range(n):
        u = np.concatenate([rng.normal(size=3) * noise, [-float(i), 0, 0] + rng.normal(size=3) * noise, [0.0 if fix_scale[i] else rng.normal() * noise]])
        if i == 0:
            u = np.zeros(7)
        S = em.sim3_exp(list(u), F)
        q.append([float(v) for v in S[0]]); t.append([float(v) for v in S[1]]); s.append(float(S[2]))
    return q, t, s


def _measure(i, j, rng, fix_scale, noise=0.05):
    """the measurement Sji of an undisturbed chain (vertex k sits at t = (-k, 0, 0), scale 1), disturbed: the measurements contradict
    each other, so the minimum keeps a residual and the last steps of a run are decided by more than rounding"""
    u = np.concatenate([rng.normal(size=3) * noise, [float(i - j), 0, 0] + rng.normal(size=3) * noise, [0.0 if fix_scale else rng.normal() * noise]])
    S = em.sim3_exp(list(u), np.float64)
    return [float(v) for v in S[0]], [float(v) for v in S[1]], float(S[2])


def _structure_problem(edges, n, fixed, fix_scale, seed, pts=None):
    rng = np.random.default_rng(seed)
    q, t, s = _chain(n, rng, fix_scale)
    mq, mt, ms = zip(*[_measure(i, j, rng, all(fix_scale)) for i, j in edges])
    pos, ref = (None, None) if pts is None else pts
    return em.Problem(q, t, s, fixed, fix_scale, [e[0] for e in edges], [e[1] for e in edges], mq, mt, ms, pos, ref)


STRUCTURE = {
    # the smallest problem: 1 fixed + 1 free, 1 edge
    "smallest": dict(n=2, edges=[(1, 0)], fixed=[1, 0], fix_scale=[0, 0]),
    # an edge between two fixed vertices (chi2 only), edges to a fixed vertex in both orientations
    "fixed pair": dict(n=4, edges=[(1, 0), (0, 1), (2, 1), (3, 2), (0, 2), (3, 1)], fixed=[1, 1, 0, 0], fix_scale=[0, 0, 0, 0]),
    # doubled pairs in both orientations: their blocks add into one off-diagonal block
    "doubled pairs": dict(seed=7, n=4, edges=[(1, 0), (2, 1), (1, 2), (2, 1), (3, 2), (2, 3), (3, 1), (1, 3)], fixed=[1, 0, 0, 0], fix_scale=[0, 0, 0, 0]),
    # a free vertex without edges: its estimate must not move
    "isolated": dict(n=4, edges=[(1, 0), (2, 1), (2, 0)], fixed=[1, 0, 0, 0], fix_scale=[0, 0, 0, 0]),
    "mixed fix_scale": dict(n=5, edges=[(1, 0), (2, 1), (3, 2), (4, 3), (4, 0), (3, 1)], fixed=[1, 0, 0, 0, 0], fix_scale=[0, 1, 0, 1, 0]),
    "fix_scale everywhere": dict(n=5, edges=[(1, 0), (2, 1), (3, 2), (4, 3), (4, 0), (3, 1)], fixed=[1, 0, 0, 0, 0], fix_scale=[1, 1, 1, 1, 1]),
}


@needs_long_double
@pytest.mark.parametrize("name", sorted(STRUCTURE))
def test_structure_cases(name):
    c = STRUCTURE[name]
    fam = yardstick()
    pts = (np.array([[0.5, 1, 2], [-1, 0.25, 3], [2, 2, 2]], np.float32), [c["n"] - 1, -1, 0])      # one point has no reference
    p = _structure_problem(c["edges"], c["n"], c["fixed"], c["fix_scale"], c.get("seed", 8), pts)
    ref, ld = em.run(p, np.float64), em.run(p, em.L)
    key = (em.band_of(max(p.n_free, 1)), all(c["fix_scale"]))
    g, fails, line = judge(p, ref, ld, fam["band_est"][key], fam["band_pts"][key], name)
    assert not fails, (fails, line)
    assert g.errEnd < g.err0
    start = np.concatenate([p.q, p.t, p.s[:, None]], axis=1)
    if name == "isolated":
        assert g.estimates[3].tobytes() == start[3].tobytes()
        assert not np.array_equal(g.estimates[1], start[1])
    fs = np.array(c["fix_scale"], bool)
    assert g.estimates[fs, 7].tobytes() == start[fs, 7].tobytes()             # scale bits unchanged under fix_scale
    free_scale = ~fs & ~p.fixed
    if name != "isolated":
        assert (g.estimates[free_scale, 7] != start[free_scale, 7]).all()
    if name == "fixed pair":
        e01 = em.edge_errors(em._s3(p.mq[:2], p.mt[:2], p.ms[:2], np.float64), em._take(em._s3(p.q, p.t, p.s, np.float64), p.vi[:2]),
                             em._take(em._s3(p.q, p.t, p.s, np.float64), p.vj[:2]), np.float64)
        assert g.errEnd >= float((e01 * e01).sum()) * (1 - 1e-12)               # the fixed pair's edges contribute chi2 only


# ------------------------------------------------------------------ 5. the cap of 1170 free keyframes, and one size below it

@needs_long_double
@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("name", sorted(em.RING_COPIES))
def test_copies_of_a_ring_at_and_below_the_cap(name, fix_scale):
    """EG_MAX_FREE_KEYFRAMES free keyframes (8190 unknowns on k_wide_*) and 1040 (past 1024, below the cap) as interleaved disjoint
    copies of one ring of 13 free keyframes with drift, each with its own fixed keyframe: the float64 model on ONE ring is the
    reference of every copy (tests/test_essential_graph_cpu.py::test_copies_of_a_ring_follow_its_trajectory).  Trials and verdict
    per iteration equal; chi2 at entry the number of copies times the ring's, to max(1e-12, ten times what reversing that sum
    moves it by); estimates and points of every copy, and of the copies among each other, within 4 x the float64-vs-long-double
    distance of the band of 43 and more free keyframes; chi2 along the trace within 4 x the ring's own float64-vs-long-double
    distance in it (the state it is evaluated at differs by that much)."""
    fam = yardstick()
    key = (em.BANDS[-1], fix_scale)
    band_est, band_pts = fam["band_est"][key], fam["band_pts"][key]
    K = em.RING_COPIES[name]
    p = em.ring_problem(fix_scale)
    one, ld = em.run(p, np.float64, iterations=RING_ITERATIONS), em.run(p, em.L, iterations=RING_ITERATIONS)
    rp = em.replicate(p, K)
    assert rp.n_free == 13 * K and (name != "cap1170" or rp.n_free == capi.EG_MAX_FREE_KEYFRAMES)
    g = solve(rp, iterations=RING_ITERATIONS)
    assert device_trace(g) == em.trace_key(one) == em.trace_key(ld) and g.iters == one["iters"]
    rel0 = abs(g.err0 - K * float(one["err0"])) / (K * float(one["err0"]))
    chi_g, chi_1, chi_ld = g.trace[:, 2], np.array([float(t[2]) for t in one["trace"]]), np.array([float(t[2]) for t in ld["trace"]])
    band_chi = float((np.abs(chi_1 - chi_ld) / chi_ld).max())
    rel = float((np.abs(chi_g - K * chi_1) / (K * chi_1)).max())
    d_est = max(em.est_diff(g.estimates[c::K], one["est"]) for c in range(K))
    pts = g.points.reshape(-1, K, 3).astype(np.float64)
    m = p.ref >= 0
    d_pts = float(np.abs(pts[m] - one["points"][m][:, None, :]).max())
    among_est = max(em.est_diff(g.estimates[c::K], g.estimates[0::K]) for c in range(1, K))
    among_pts = float(np.abs(pts[m] - pts[m][:, :1]).max())
    print("%s fix_scale %d: err0 %.3g (bound %.3g), chi2 of the trace %.3g (4 x %.3g), |d est| %.3g among the copies %.3g (4 x %.3g), |d pts| %.3g among %.3g (4 x %.3g)" %
          (name, fix_scale, rel0, ring_err0_rtol(name, fix_scale), rel, band_chi, d_est, among_est, band_est, d_pts, among_pts, band_pts))
    assert rel0 <= ring_err0_rtol(name, fix_scale)
    assert rel <= 4 * band_chi
    assert d_est <= 4 * band_est and among_est <= 4 * band_est
    assert d_pts <= 4 * band_pts and among_pts <= 4 * band_pts
    assert abs(g.errEnd - g.trace[-1, 2]) <= 1e-12 * g.errEnd and g.errEnd < g.err0
    fixed_in = np.concatenate([rp.q, rp.t, rp.s[:, None]], axis=1)[rp.fixed]
    assert g.estimates[rp.fixed].tobytes() == fixed_in.tobytes()                      # every copy's fixed keyframe stays
    assert g.points[rp.ref < 0].tobytes() == rp.pos[rp.ref < 0].tobytes()
    if fix_scale:
        assert g.estimates[:, 7].tobytes() == rp.s.tobytes()


# ------------------------------------------------------------------ 6. determinism

def _bits(r):
    return (r.estimates.tobytes(), r.points.tobytes(), r.trace.tobytes(), r.edge_error0.tobytes(), r.err0, r.errEnd, r.iters)


def test_two_calls_give_equal_bits_and_two_threads_equal_the_serial_result():
    probs = [em.flat_problem(em.collect_loop_form(em.make_scene(n, fs, seed, drift=em.FAMILY_DRIFT))) for n, fs, seed in
             ((12, True, 21), (20, False, 41), (45, True, 71))]
    serial = [_bits(solve(p)) for p in probs]
    assert [_bits(solve(p)) for p in probs] == serial
    got = {}

    def work(tid):
        got[tid] = [_bits(solve(p)) for p in (probs if tid == 0 else probs[::-1])]

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got[0] == serial and got[1] == serial[::-1]
