"""OptimizeSim3, the parts that need no GPU: the checker (tests/sim3_opt_model.py) against known similarities and against its own
long double evaluation -- the figures the GPU tolerances are built from --, the ABI surface, and the loud failure without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim3_model as sm
import sim3_opt_model as om
from multi_orbslam3_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_long_double = pytest.mark.skipif(not om.LONGDOUBLE_OK, reason="numpy.longdouble is not the 80-bit format here")


# ------------------------------------------------------------------ 1. model sanity

def _exact_problem(seed, n, fix_scale):
    """Noise-free: X1 = s R X2 + t, observations the exact projections, every match seen in KF2, the start disturbed."""
    sc = sm.make_scene(seed, n, fix_scale, outlier_fraction=0.0, noise=0.0)
    f = np.float32
    K1, K2 = np.array(sc["K1"], f), np.array(sc["K2"], f)

    def proj(K, X):
        X = X.astype(np.float64)
        return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)
    rng = np.random.default_rng(seed + 1)
    Rp = sm.rot_from_axis_angle(rng.normal(size=3), 0.01) @ sc["R"]
    q0 = np.array(om.quat_from_R(Rp.tolist(), np.float64))
    t0 = sc["t"] + rng.normal(size=3) * 0.01
    s0 = sc["s"] * (1.0 if fix_scale else 1.01)
    w = np.ones(n, f)
    return om.Problem(sc["X1"], sc["X2"], proj(K1, sc["X1"]), proj(K2, sc["X2"]), w, w, K1, K2, fix_scale, 10.0, q0, t0, s0), sc


@pytest.mark.parametrize("fix_scale", [True, False])
def test_model_recovers_a_known_similarity(fix_scale):
    p, sc = _exact_problem(11, 60, fix_scale)
    r = om.optimize_sim3(p, np.float64)
    assert not r["returned_early"] and r["n_in"] == p.n and not r["removed"].any()
    S = om.sim3_matrix(r["q"], r["t"], r["s"])
    T = np.eye(4)
    T[:3, :3] = sc["s"] * sc["R"]
    T[:3, 3] = sc["t"]
    # (points and observations were rounded to float32: 1e-6 relative on coordinates of up to 10 m and pixels of up to 700)
    assert np.abs(S - T).max() < 1e-4
    if fix_scale:
        assert r["s"] == p.s                                   # the scale never moves
    # the final chi2 is that of float32-rounded inputs, far below one pixel^2 per edge
    assert float(r["chi2"][1]) < 1e-3 * p.n


def test_jacobian_column_seven_is_exactly_zero_with_fix_scale():
    p = om.family_problem((40100, 40, True, 0.0, None))
    for F in (np.float64, om.L):
        E = om._Edges(p, F)
        est = ([F(v) for v in p.q], [F(v) for v in p.t], F(p.s))
        J12, J21 = om.jacobians(E, est, True, F)
        for J in (J12, J21):
            assert not np.any(J[0][6]) and not np.any(J[1][6])
            assert np.any(J[0][0]) and np.any(J[1][5])
        J12f, _ = om.jacobians(E, est, False, F)
        assert np.any(J12f[0][6])


def test_sim3_exp_on_its_four_branches():
    """exp(v) * exp(-v) is the identity on each branch of Sim3(Vector7d) (theta and sigma below / above 1e-5) up to what the branch's
    own truncation leaves, and the branches join at the 1e-5 borders up to the same terms.  (Sim3::log is not restated: nothing in
    OptimizeSim3 calls it.)"""
    for th, sg in ((1e-7, 1e-7), (0.3, 1e-7), (1e-7, 0.2), (0.3, 0.2)):
        v = np.array([0.6 * th, -0.64 * th, 0.48 * th, 0.3, -0.2, 0.1, sg])
        for F in (np.float64, om.L):
            a, b = om.sim3_exp(v, F), om.sim3_exp(-v, F)
            c = om.sim3_mul(a, b)
            got = np.array([float(x) for x in c[0] + c[1] + [c[2]]])
            # the small-angle rotation I + Omega + Omega^2 is not orthonormal: its quaternion is off by O(theta^2); the small-sigma
            # branch takes C = 1 for (s - 1) / sigma = 1 + sigma / 2 + ...: the translation is off by O(sigma |upsilon|), |upsilon| < 0.4
            tol = 1e-12 + (4 * th * th if th < 1e-5 else 0) + (0.4 * sg if sg < 1e-5 else 0)
            assert np.abs(got - np.array([0, 0, 0, 1, 0, 0, 0, 1.0])).max() < tol
    # across theta = 1e-5: Omega^2 / 2 against Omega^2, 5e-11; across sigma = 1e-5: C = 1 against 1 + sigma / 2, 5e-6 |upsilon|
    for k, border, tol in ((0, 1e-5, 1e-10), (6, 1e-5, 0.4 * 1e-5)):
        v = np.array([0, 0, 0, 0.3, -0.2, 0.1, 0.0])
        lo, hi = v.copy(), v.copy()
        lo[k], hi[k] = border * (1 - 1e-6), border * (1 + 1e-6)
        a, b = om.sim3_exp(lo, np.float64), om.sim3_exp(hi, np.float64)
        da = np.array([float(x) for x in a[0] + a[1] + [a[2]]]) - np.array([float(x) for x in b[0] + b[1] + [b[2]]])
        assert np.abs(da).max() < tol


def test_nan_and_infinity_take_the_references_branches():
    """Rule 4.  z = 0 after mapping: the edge's chi2 is inf, H is NaN, every solve is refused (tempChi = DBL_MAX), the `rho > 0 &&
    isfinite` test accepts the unchanged estimate, and chi2 > th2 removes the pair.  A NaN observation: chi2 > th2 is false for that
    edge (only the pair's other edge can remove it) while every sum it enters is NaN."""
    p = om.family_problem((424242, 60, True, 0.3, "z0"))
    r = om.optimize_sim3(p, np.float64)
    assert np.isinf(r["edge_chi2"][0][0]) and r["removed"][0] == 1
    assert [t[3] for t in r["trace"]] == [1] * 5                # five iterations of one refused trial each
    p = om.family_problem((434343, 60, False, 0.3, "nan"))
    r = om.optimize_sim3(p, np.float64)
    # the NaN side never removes the pair; its other edge alone decides
    assert np.isnan(r["edge_chi2"][0][0]) and bool(r["removed"][0]) == bool(r["edge_chi2"][1][0] > p.th2)
    assert all(np.isnan(t[2]) for t in r["trace"])


# ------------------------------------------------------------------ 2. rule 1 is observable

def test_round_one_reads_the_last_trials_errors():
    """:4241 reads chi2() without computeError(): when the last LM trial of round 1 was REJECTED (ten refused trials, or a trial that
    leaves chi2 unchanged: rho == 0), the errors are those of the rejected estimate.  2756 seeded scenes were searched (n = 20 / 40 /
    80, both scale modes, 0 / 30 % wrong matches, half of them started from an already refined estimate) for one in which classifying
    from recomputed errors gives another SET: none does -- a rejected last trial sits behind a damping of 2^45 or a step that no longer
    changes chi2, so the two estimates differ by less than any chi2 differs from th2.  Eight of them differ in the VALUES read; one of
    those is pinned here, and the model is asserted to follow the reference's form."""
    p = om.make_problem(9000 + 1437, 20, True, 0.0)
    a = om.optimize_sim3(p, np.float64)
    b = om.optimize_sim3(p, np.float64, classify_round1_from="recomputed")
    r1 = [t for t in a["trace"] if t[0] == 0]
    assert r1 == [t for t in b["trace"] if t[0] == 0] and r1[-1][3] == 10          # the same round 1; it ends on ten refused trials
    assert not np.array_equal(a["edge_chi2"][0], b["edge_chi2"][0])                  # the values read at :4241 are the rejected trial's
    assert np.abs(a["edge_chi2"][0] - b["edge_chi2"][0]).max() < 1e-6
    assert np.array_equal(a["removed"], b["removed"])                                # ... and the set is the same


# ------------------------------------------------------------------ 3. the yardstick and its caps

@needs_long_double
def test_float64_model_against_long_double_on_the_family(capsys):
    """The conditions the GPU test inherits, on the models alone (float64 against long double):
      * inlier sets and return values equal after leaving out the decisions whose long double chi2 lies within 1e-3 (relative) of th2;
        at most 0.1 % of the decisions left out;
      * round-1 traces (iterations and trials per iteration) equal in at least 95 % of the scenes;
      * at most 5 % of the scenes with a non-zero return are ill-conditioned (q / t / s of the two precisions more than 1e-5 apart);
      * the family is not vacuous: at least 60 scenes, n from 10 to 2000, at least one early return and at most a quarter of them.
    Printed per (n band, scale mode): the largest well-conditioned difference -- the GPU tolerance is 4 x that figure.
    Round-2 traces are printed, not asserted: where the estimate has converged the noise of a 1e-9 central difference decides whether
    a step is accepted, in the reference as here."""
    fam = om.measure_family()
    sc = fam["scenes"]
    assert len(sc) >= 60
    ns = [s["entry"][1] for s in sc]
    assert min(ns) == 10 and max(ns) == 2000
    early = sum(bool(s["ld"]["returned_early"]) for s in sc)
    assert 1 <= early <= len(sc) / 4, early
    assert {s["entry"][3] for s in sc} == {0.0, 0.3, 0.5} and {s["entry"][2] for s in sc} == {True, False}
    assert {s["entry"][4] for s in sc} == {None, "z0", "nan"}
    decisions = sum(s["cmp"]["decisions"] for s in sc)
    left_out = sum(s["cmp"]["left_out"] for s in sc)
    same_t1 = sum(om.round_trace(s["f64"], 0) == om.round_trace(s["ld"], 0) for s in sc)
    same_t2 = sum(om.round_trace(s["f64"], 1) == om.round_trace(s["ld"], 1) for s in sc)
    nonzero = [s for s in sc if s["ld"]["n_in"] > 0]
    ill = [s for s in nonzero if s["ill"]]
    with capsys.disabled():
        print("\nOptimizeSim3 model, float64 vs long double: %d scenes (%d early returns), %d decisions, %d left out (within 1e-3 of th2)"
              % (len(sc), early, decisions, left_out))
        print("  round-1 traces equal in %d, round-2 traces in %d; %d of %d scenes with a non-zero return ill-conditioned"
              % (same_t1, same_t2, len(ill), len(nonzero)))
        for b in sorted(fam["band_max"]):
            print("  band n_in >= %d, fix_scale %d: largest well-conditioned |d(q, t, s)| = %.3g" % (b[0], b[1], fam["band_max"][b]))
        for s in sc:
            if om.round_trace(s["f64"], 1) != om.round_trace(s["ld"], 1):
                print("  round-2 trace differs in %s: %s vs %s" % (s["entry"], om.round_trace(s["f64"], 1), om.round_trace(s["ld"], 1)))
    assert all(s["cmp"]["equal"] for s in sc), [s["entry"] for s in sc if not s["cmp"]["equal"]]
    assert left_out <= 1e-3 * decisions
    assert same_t1 >= 0.95 * len(sc)
    assert len(ill) <= 0.05 * len(nonzero)
    assert set(fam["band_max"]) == {(lo, fs) for lo, _ in om.N_BANDS for fs in (True, False)}      # every band has its figure


def test_collection_loop_of_the_model():
    """Every branch of :4083-4223 on one small scene, and rules 2 and 3 on the values."""
    f = np.float32
    th = 0.3
    R2 = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], f)
    kf1 = dict(R=np.eye(3, dtype=f), t=np.array([0.5, 0, 0], f), keys=np.arange(20, dtype=f).reshape(10, 2), octave=np.arange(10) % 8,
               inv_level_sigma2=(f(1) / sm.level_sigma2()).astype(f), mp=np.array([0, 1, 2, -1, 4, 5, 6, 7, 8, 9]))
    kf2 = dict(R=R2, t=np.array([0, 0, 1], f), keys=100 + np.arange(12, dtype=f).reshape(6, 2), octave=np.array([3, 2, 1, 0, 7, 6]),
               inv_level_sigma2=(f(1) / sm.level_sigma2(scale_factor=1.5)).astype(f))
    pos = np.array([[0.1 * k, -0.2 * k, 4 + 0.5 * k] for k in range(20)], f)
    pos[17] = (0, 0, -3)                                          # behind KF2: z < 0
    bad = np.zeros(20, bool)
    bad[1] = True                                                 # a bad pMP1
    bad[12] = True                                                # a bad pMP2
    idx2 = np.full(20, -1)
    idx2[[10, 11, 12, 13, 14, 17, 18]] = [0, 1, 2, 3, 4, 5, 5]
    mps = dict(pos=pos, bad=bad, idx_in_kf2=idx2, track_scale_level=np.full(20, 3))
    #           i: 0   1(bad1) 2(bad2) 3(no MP1) 4   5(out of KF2) 6(z<0) 7(NULL) 8   9(out)
    matches = np.array([10, 11, 12, 13, 14, 15, 17, -1, 18, 16])
    for all_points, want in ((True, [0, 4, 5, 8, 9]), (False, [0, 4, 8])):
        p, index, cnt = om.collect(kf1, kf2, matches, mps, all_points, (400, 400, 320, 240), (410, 410, 300, 200), True, 10.0,
                                   [0, 0, 0, 1], [0, 0, 0], 1.0)
        assert index.tolist() == want
        assert cnt == dict(nCorrespondences=len(want), nBadMPs=2, nInKF2=3, nOutKF2=len(want) - 3, nMatchWithoutMP=1)
        assert p.n_corr == len(want) == p.n
        # rule 3: the point in camera 2 is the float of the double-accumulated product
        P = pos[10].astype(np.float64)
        want2 = (R2.astype(np.float64) @ P + np.array([0, 0, 1.0])).astype(f)
        assert np.abs(p.X2[0] - want2).max() <= np.spacing(f(8))
        assert p.X1[0].tolist() == (pos[0] + np.array([0.5, 0, 0], f)).tolist()
        assert p.obs1[1].tolist() == [8.0, 9.0] and p.w1[1] == kf1["inv_level_sigma2"][4]
        assert p.obs2[1].tolist() == [108.0, 109.0] and p.w2[1] == kf2["inv_level_sigma2"][7]
        if all_points:
            # rule 2: normalised coordinates and level 0's weight, whatever mnTrackScaleLevel says
            x2 = p.X2[2]
            assert p.obs2[2].tolist() == [x2[0] * (f(1) / x2[2]), x2[1] * (f(1) / x2[2])]
            assert p.w2[2] == kf2["inv_level_sigma2"][0] == 1.0


# ------------------------------------------------------------------ 4. the ABI surface without a device

def test_ctypes_mirrors_have_the_headers_layout(tmp_path):
    src = tmp_path / "layout.c"
    fields = {"orbm_sim3opt_problem": ("Sim3OptProblem", ["struct_size", "n", "X3Dc1", "X3Dc2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2",
                                                          "fx1", "cy1", "fx2", "cy2", "camera_model1", "camera_model2", "fix_scale", "th2",
                                                          "q", "t", "s", "n_correspondences"]),
              "orbm_sim3opt_result": ("Sim3OptResult", ["struct_size", "n_in", "returned_early", "n_bad_round1", "q", "t", "s", "removed",
                                                        "iters", "chi2", "trace", "trace_cap", "trace_len", "edge_chi2"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "orbgpu.h"', 'int main(void) {']
    for cname, (_, fl) in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fld in fl:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fld, cname, fld))
    lines += ["return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(ln.split() for ln in subprocess.check_output([exe], text=True).splitlines())
    for cname, (pyname, fl) in fields.items():
        cls = getattr(capi, pyname)
        assert int(got[cname]) == C.sizeof(cls), cname
        for fld in fl:
            assert int(got["%s.%s" % (cname, fld)]) == getattr(cls, fld).offset, (cname, fld)


def test_no_gpu_means_no_optimizer_and_bad_arguments_are_refused_first():
    from multi_orbslam3_amd import api
    lib = capi.load()
    m = om.family_problem((40100, 40, True, 0.0, None))
    p = api.Sim3OptProblem(m.X1, m.X2, m.obs1, m.obs2, m.w1, m.w2, m.K1, m.K2, m.fix_scale, m.th2, m.q, m.t, m.s)
    r = capi.Sim3OptResult()
    r.struct_size = C.sizeof(capi.Sim3OptResult)
    r.n_in = -7
    # bad arguments are refused before the device is looked for: the same answer with and without a GPU
    for change in (dict(th2=0.0), dict(camera_model1=1), dict(struct_size=4), dict(X3Dc1=None), dict(s=float("nan"))):
        st = p.struct()
        for k, v in change.items():
            setattr(st, k, v)
        assert lib.orbm_sim3_optimize(0, C.byref(st), C.byref(r)) == capi.ORBG_BAD_ARG, change
        assert r.n_in == -7
    assert lib.orbm_sim3_optimize(0, None, C.byref(r)) == capi.ORBG_BAD_ARG
    if lib.orbg_device_count() > 0:
        pytest.skip("a GPU is present: the no-device half does not apply")
    st = p.struct()
    assert lib.orbm_sim3_optimize(0, C.byref(st), C.byref(r)) == capi.ORBG_NO_DEVICE and r.n_in == -7
    with pytest.raises(capi.OrbGpuError) as e:
        api.OptimizeSim3(p)
    assert e.value.code == capi.ORBG_NO_DEVICE
    with pytest.raises(capi.OrbGpuError) as e:
        api.OptimizeSim3.batch([p, p])
    assert e.value.code == capi.ORBG_NO_DEVICE


def test_api_collection_equals_the_models():
    """api.sim3opt_collect (vectorised, what the chain test feeds the device with) against the model's literal loop, bit for bit."""
    from multi_orbslam3_amd import api
    rng = np.random.default_rng(3)
    f = np.float32
    N, M = 300, 500
    pos = np.stack([rng.uniform(-3, 3, M), rng.uniform(-2, 2, M), rng.uniform(-1, 9, M)], 1).astype(f)
    bad = rng.random(M) < 0.1
    idx2 = np.where(rng.random(M) < 0.7, rng.integers(0, 200, M), -1)
    mp1 = np.where(rng.random(N) < 0.9, rng.integers(0, M, N), -1)
    matches = np.where(rng.random(N) < 0.8, rng.integers(0, M, N), -1)
    T1, T2 = np.eye(4, dtype=f), np.eye(4, dtype=f)
    T1[:3, :3] = sm.rot_from_axis_angle([1, 2, 3], 0.2)
    T1[:3, 3] = (0.1, -0.2, 0.3)
    T2[:3, :3] = sm.rot_from_axis_angle([-1, 0.5, 2], 0.4)
    T2[:3, 3] = (-0.3, 0.1, 0.5)
    keys1, keys2 = rng.uniform(0, 700, (N, 2)).astype(f), rng.uniform(0, 700, (200, 2)).astype(f)
    oc1, oc2 = rng.integers(0, 8, N), rng.integers(0, 8, 200)
    s1, s2 = (f(1) / sm.level_sigma2()).astype(f), (f(1) / sm.level_sigma2(scale_factor=1.3)).astype(f)
    K1, K2 = (458.654, 457.296, 367.215, 248.375), (435.2, 435.2, 320.0, 240.0)
    S = ([0.01, 0.02, -0.01, 0.9997], [0.1, 0.2, 0.3], 1.1)
    for all_points in (True, False):
        kf1 = dict(R=T1[:3, :3], t=T1[:3, 3], keys=keys1, octave=oc1, inv_level_sigma2=s1, mp=mp1)
        kf2 = dict(R=T2[:3, :3], t=T2[:3, 3], keys=keys2, octave=oc2, inv_level_sigma2=s2)
        mps = dict(pos=pos, bad=bad, idx_in_kf2=idx2, track_scale_level=np.zeros(M, int))
        want, index, _ = om.collect(kf1, kf2, matches, mps, all_points, K1, K2, False, 10.0, *S)
        got = api.sim3opt_collect(T1, T2, mp1, keys1, oc1, s1, keys2, oc2, s2, matches, pos, bad, idx2, K1, K2, S, 10.0, False, all_points)
        assert got.n == want.n > 50 and np.array_equal(got.index_edge, index)
        for a, b in ((got.X1, want.X1), (got.X2, want.X2), (got.obs1, want.obs1), (got.obs2, want.obs2), (got.w1, want.w1), (got.w2, want.w2)):
            assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 5. the collection half of the glue

CPP = os.path.join(ROOT, "tests", "cpp")


def parse_glue_output(text):
    out, cur = {}, None
    for ln in text.splitlines():
        if ln.startswith("["):
            cur = out.setdefault(ln.strip("[]"), {})
        elif ":" in ln:
            k, v = ln.split(":", 1)
            cur[k] = v.split()
    return out


def glue_floats(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


def glue_scene(sc):
    """The [scene] section of glue_sim3_opt_check -> the arguments of sim3_opt_model.collect."""
    f = np.float32
    T1, T2 = glue_floats(sc["T1"]).reshape(4, 4), glue_floats(sc["T2"]).reshape(4, 4)
    kf1 = dict(R=T1[:3, :3], t=T1[:3, 3], keys=glue_floats(sc["keys1"]).reshape(-1, 2), octave=np.array(sc["oct1"], int),
               inv_level_sigma2=glue_floats(sc["inv1"]), mp=np.array(sc["mp1"], int))
    kf2 = dict(R=T2[:3, :3], t=T2[:3, 3], keys=glue_floats(sc["keys2"]).reshape(-1, 2), octave=np.array(sc["oct2"], int),
               inv_level_sigma2=glue_floats(sc["inv2"]))
    mps = dict(pos=glue_floats(sc["pos"]).reshape(-1, 3).astype(f), bad=np.array(sc["bad"], int) != 0, idx_in_kf2=np.array(sc["idx2"], int),
               track_scale_level=np.array(sc["level"], int))
    return kf1, kf2, np.array(sc["match"], int), mps


def glue_flat_equals(g, p, index, cnt):
    return ([int(v) for v in g["vnIndexEdge"]] == index.tolist() and
            [int(v) for v in g["counters"]] == [cnt[k] for k in ("nCorrespondences", "nBadMPs", "nInKF2", "nOutKF2", "nMatchWithoutMP")] and
            glue_floats(g["X3Dc1"]).tobytes() == p.X1.tobytes() and glue_floats(g["X3Dc2"]).tobytes() == p.X2.tobytes() and
            glue_floats(g["obs1"]).tobytes() == p.obs1.tobytes() and glue_floats(g["obs2"]).tobytes() == p.obs2.tobytes() and
            glue_floats(g["w1"]).tobytes() == p.w1.tobytes() and glue_floats(g["w2"]).tobytes() == p.w2.tobytes())


@pytest.mark.parametrize("strict", [False, True])
def test_glue_collect_over_mock_keyframes(tmp_path, strict):
    """orbgpu::sim3opt_collect over the mocks equals the model's collection loop bit for bit on a scene that takes every branch:
    vpMatches1[i] == NULL, a bad pMP1, a bad pMP2, pMP1 == NULL (with a good and a bad pMP2), i2 < 0 with bAllPoints true and false,
    z < 0 (seen and not seen in KF2)."""
    exe = str(tmp_path / "glue_sim3_opt_check")
    lib_dir = os.path.join(ROOT, "multi_orbslam3_amd")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", CPP,
           os.path.join(CPP, "glue_sim3_opt_check.cpp"), "-o", exe, "-pthread", "-L", lib_dir, "-lorbgpu", "-Wl,-rpath," + lib_dir,
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"] + (["-DMOCK_STRICT_ACCESS"] if strict else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = parse_glue_output(r.stdout)
    kf1, kf2, matches, mps = glue_scene(got["scene"])
    K1, K2 = (458.654, 457.296, 367.215, 248.375), (435.2, 435.2, 320.0, 240.0)
    for tag, all_points, want_index in (("all_points", True, [0, 6, 8, 10]), ("only_in_kf2", False, [0, 8, 10])):
        p, index, cnt = om.collect(kf1, kf2, matches, mps, all_points, K1, K2, True, 10.0, [0, 0, 0, 1], [0, 0, 0], 1.0)
        assert index.tolist() == want_index
        assert cnt["nBadMPs"] == 2 and cnt["nMatchWithoutMP"] == 2
        assert glue_flat_equals(got[tag], p, index, cnt), tag
        assert np.array_equal(glue_floats(got[tag]["k1"]), np.array(K1, np.float32)) and np.array_equal(glue_floats(got[tag]["k2"]), np.array(K2, np.float32))
    # rule 2 on the values: pair 6 is not seen in KF2 -- normalised coordinates, level 0's weight
    g = got["all_points"]
    x2 = glue_floats(g["X3Dc2"]).reshape(-1, 3)[1]
    invz = np.float32(1) / x2[2]
    assert glue_floats(g["obs2"]).reshape(-1, 2)[1].tolist() == [x2[0] * invz, x2[1] * invz]
    assert glue_floats(g["w2"])[1] == 1.0


def test_mock_members_are_public_in_the_reference():
    """Every `// ref: I/<Header>.h:<line> <name>` and `// ref: G/<path>.h:<line> <name>` note of tests/cpp/mock_sim3_opt.hpp: that line
    of the reference's header declares that name, in a public section."""
    import re
    from test_reference_access import REF_INC
    if not os.path.isdir(REF_INC):
        pytest.skip("the reference is only present in the build container")
    g2o = os.path.join(os.path.dirname(REF_INC), "Thirdparty", "g2o", "g2o")
    notes = re.findall(r"// ref: ([IG])/([\w/]+\.h):(\d+) (\w+)", open(os.path.join(CPP, "mock_sim3_opt.hpp")).read())
    assert len(notes) >= 6
    for root, hdr, line, name in notes:
        lines = open(os.path.join(REF_INC if root == "I" else g2o, hdr)).read().splitlines()
        assert re.search(r"\b%s\b" % name, lines[int(line) - 1]), (hdr, line, name, lines[int(line) - 1])
        labels = [m.group(1) for ln in lines[: int(line)] for m in [re.match(r"\s*(public|protected|private)\s*:", ln)] if m]
        assert labels and labels[-1] == "public", (hdr, line, name, labels[-1:])
