"""OptimizeEssentialGraph without a device: the numpy model against itself in long double (the yardstick the GPU test inherits), the
model's pieces, and what eg_solve refuses or answers before it looks for a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import essential_graph_model as em
from multi_orbslam3_amd import _capi as capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_long_double = pytest.mark.skipif(not em.LONGDOUBLE_OK, reason="numpy.longdouble is not wider than float64 here")

LEFT_OUT_CAP = 0.10      # share of a family's scenes whose LM traces may differ between the two precisions


def yardstick():
    """What the GPU test reads: the measured family with band_est / band_pts (float64 vs long double, per size band and scale mode)."""
    return em.measure_family()


def api_arrays(p):
    """an essential_graph_model.Problem as the record arrays of api.OptimizeEssentialGraph"""
    V = np.zeros(len(p.s), capi.EG_VERTEX_DTYPE)
    V["q"], V["t"], V["s"], V["fixed"], V["fix_scale"] = p.q, p.t, p.s, p.fixed, p.fix_scale
    E = np.zeros(len(p.vi), capi.EG_EDGE_DTYPE)
    E["vi"], E["vj"], E["q"], E["t"], E["s"] = p.vi, p.vj, p.mq, p.mt, p.ms
    P = np.zeros(len(p.ref), capi.EG_POINT_DTYPE)
    P["pos"], P["ref"] = p.pos, p.ref
    return V, E, P


# ------------------------------------------------------------------ 1. the pieces of the model

@pytest.mark.parametrize("F", [np.float64, em.L])
def test_log_inverts_exp_on_the_four_branches(F):
    rng = np.random.default_rng(5)
    tol = 1e-13 if F is np.float64 else 1e-15
    for rot, sig in ((1e-7, 1e-7), (1e-7, 0.2), (0.4, 1e-7), (0.4, -0.3), (0.9, 0.1)):
        for _ in range(5):
            u = np.concatenate([rng.normal(size=3) * rot, rng.normal(size=3), [sig]]).astype(F)
            back = np.array(em.sim3_log(em.sim3_exp(list(u), F), F), F).reshape(-1)
            assert np.abs(back - u).max() <= tol * max(1.0, float(np.abs(u).max())), (rot, sig)


def test_log_of_the_identity_is_zero_and_sigma_zero_is_exact():
    """sigma exactly 0 with R = I: the state of every non-loop edge of a stereo map at entry"""
    ident = ([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], 1.0)
    assert all(float(v) == 0.0 for v in em.sim3_log(ident, np.float64))
    moved = ([0.0, 0.0, 0.0, 1.0], [0.25, -1.5, 3.0], 1.0)
    got = [float(v) for v in em.sim3_log(moved, np.float64)]
    assert got == [0.0, 0.0, 0.0, 0.25, -1.5, 3.0, 0.0]


def test_lu_solve_takes_the_largest_pivot():
    W = [[np.float64(1e-20), np.float64(1.0), np.float64(0.0)], [np.float64(1.0), np.float64(1.0), np.float64(0.0)],
         [np.float64(0.0), np.float64(0.0), np.float64(2.0)]]
    x = em.lu_solve3(W, [np.float64(1.0), np.float64(2.0), np.float64(4.0)])
    assert np.allclose([float(v) for v in x], [1.0, 1.0, 2.0], rtol=1e-15)


def test_scale_column_is_exactly_zero_under_fix_scale_and_fixed_vertices_have_no_jacobian():
    p = em.flat_problem(em.collect_loop_form(em.make_scene(8, True, 3)))
    F = np.float64
    e, Ji, Jj = em.linearise(p, em._s3(p.q, p.t, p.s, F), em._s3(p.mq, p.mt, p.ms, F), F)
    assert not Ji[:, :, 6].any() and not Jj[:, :, 6].any()
    assert not Ji[p.fixed[p.vi]].any() and not Jj[p.fixed[p.vj]].any()
    assert np.abs(Ji[~p.fixed[p.vi]][:, :, :6]).max() > 0.1
    H, b, col = em.normal_equations(p, e, Ji, Jj, F)
    assert not H[6::7].any() and not H[:, 6::7].any() and not b[6::7].any()     # its diagonal entry is lambda alone


def test_model_closes_a_loop():
    """chi2 falls by an order of magnitude and a vertex without edges or a fixed one keeps its estimate"""
    p = em.flat_problem(em.collect_loop_form(em.make_scene(12, True, 22)))
    r = em.run(p)
    assert r["errEnd"] < 0.1 * r["err0"] and r["iters"] >= 2
    assert np.array_equal(r["est"][p.fixed], np.concatenate([p.q, p.t, p.s[:, None]], axis=1)[p.fixed])


def test_collection_follows_the_reference_rules():
    sc = em.make_scene(14, False, 7, bad=(5,))
    col = em.collect_loop_form(sc)
    kinds = col["kinds"]
    assert len(col["vertices"]) == 13 and 5 not in col["uids"]
    assert col["dropped_edges"] >= 2                       # the bad keyframe's own spanning-tree edge and its child's
    assert {"loop_connection", "spanning_tree", "loop_edge", "covisibility"} <= set(kinds)
    pairs = [(min(e[0], e[1]), max(e[0], e[1])) for e in col["edges"]]
    n_lc = kinds.count("loop_connection")
    assert n_lc == 3                                       # (cur, loop) below minFeat but kept, (cur, 1), (cur - 1, 1); (cur, 2) left out
    cov = [pr for pr, k in zip(pairs, kinds) if k == "covisibility"]
    assert not set(cov) & set(pairs[:n_lc])                # sInsertedEdges
    assert sum(v[3] for v in col["vertices"]) == 1 and col["vertices"][0][3]
    refs = [r for _, r in col["points"]]
    assert min(refs) >= -1 and max(refs) < 13


# ------------------------------------------------------------------ 2. the yardstick

@needs_long_double
def test_float64_model_against_long_double_on_the_family(capsys):
    """The conditions the GPU test inherits, on the models alone: per size band (solver) and scale mode the largest distance between
    the float64 and the long double run in q / t / s and in the corrected points, over the scenes whose LM traces (trials and verdict
    per iteration) agree.  At most 10 % of the family's scenes may disagree on the trace -- a +-delta evaluation that straddles a
    branch of log(), or a trial whose rho is rounding noise around 0; this test holds the committed seeds inside that cap."""
    fam = yardstick()
    sc = fam["scenes"]
    left_out = [s for s in sc if not s["same_trace"]]
    with capsys.disabled():
        print("\nOptimizeEssentialGraph model, float64 vs long double: %d scenes, %d with different LM traces" % (len(sc), len(left_out)))
        for s in left_out:
            print("  trace differs in %s: %s vs %s" % (s["entry"], em.trace_key(s["f64"]), em.trace_key(s["ld"])))
        for b in sorted(fam["band_est"]):
            print("  free keyframes %4d .. %4d, fix_scale %d: |d(q, t, s)| <= %.3g, |d points| <= %.3g" % (
                b[0][0], b[0][1], b[1], fam["band_est"][b], fam["band_pts"][b]))
    assert len(sc) >= 30
    assert len(left_out) <= LEFT_OUT_CAP * len(sc), [s["entry"] for s in left_out]
    assert set(fam["band_est"]) == {(b, fs) for b in em.BANDS for fs in (True, False)}      # every band has its figure
    assert {s["problem"].n_free for s in sc} >= {17, 18, 19, 42, 43, 44, 120}
    for s in sc:
        assert s["f64"]["errEnd"] < s["f64"]["err0"]
        assert all(t[0] >= 1 for t in s["f64"]["trace"])


RING_ITERATIONS = 3      # the ring's improvements are 0.9, 0.1 and 3e-6 of chi2; a fourth step would be decided by the noise of the numeric Jacobian
# |forward - reversed| / sum for err0 of the replicated rings, measured below and printed: the GPU bound on err0 is max(1e-12, 10 x)
RING_SUM_MEASURED = {("cap1170", True): 1.64e-16, ("cap1170", False): 6.87e-16, ("kilo1040", True): 2.03e-15, ("kilo1040", False): 1.24e-15}
# For the record, the float64 model on all 90 copies (ten seconds a run, not part of the suite): the ring's trace in both scale modes,
# err0 90 times the ring's to the bit, estimates within 3.5e-7 (fixed scale) / 8.5e-7, points within 6.4e-6 / 5.7e-6 of the ring's.


def ring_err0_rtol(name, fix_scale):
    return max(1e-12, 10.0 * RING_SUM_MEASURED[(name, fix_scale)])


@needs_long_double
@pytest.mark.parametrize("fix_scale", [True, False])
def test_copies_of_a_ring_follow_its_trajectory(fix_scale):
    """The argument the cap cases of tests/test_gpu_essential_graph.py rest on (em.RING_COPIES), on three interleaved copies where
    the model can still solve the whole problem: the trace (trials and verdict per iteration) is the ring's, chi2 at entry three
    times the ring's, every copy's estimates and points the ring's within 4 x the float64-vs-long-double distance of the band of 43
    and more free keyframes, as the device is held to.  Every verdict of the ring is decided by far more than rounding.  Prints the
    forward-against-reversed figure of the replicated chi2 sums, which is the GPU bound on err0 at 90 and 80 copies."""
    fam = yardstick()
    key = (em.band_of(em.RING_FREE * 90), fix_scale)
    assert key[0] == em.BANDS[-1] and em.RING_FREE * em.RING_COPIES["cap1170"] == capi.EG_MAX_FREE_KEYFRAMES == 1170
    assert 1024 < em.RING_FREE * em.RING_COPIES["kilo1040"] < capi.EG_MAX_FREE_KEYFRAMES
    p = em.ring_problem(fix_scale)
    one, ld = em.run(p, np.float64, iterations=RING_ITERATIONS), em.run(p, em.L, iterations=RING_ITERATIONS)
    assert p.n_free == em.RING_FREE and p.fixed.tolist() == [True] + [False] * em.RING_FREE
    assert em.trace_key(one) == em.trace_key(ld) == [(1, 1)] * RING_ITERATIONS
    chi = [float(one["err0"])] + [float(t[2]) for t in one["trace"]]
    assert min((a - b) / a for a, b in zip(chi[:-1], chi[1:])) > 1e-6           # against 1e-16 of a chi2 evaluation
    K = 3
    rp = em.replicate(p, K)
    assert rp.fixed[:K].all() and not rp.fixed[K:].any() and np.array_equal(rp.vi % K, rp.edge_copy) and np.array_equal(rp.vj % K, rp.edge_copy)
    assert (np.diff(rp.edge_copy) != 0).any() and (np.diff(rp.edge_source) < 0).any()                  # interleaved, in no order
    three = em.run(rp, np.float64, iterations=RING_ITERATIONS)
    assert em.trace_key(three) == em.trace_key(one) and three["iters"] == one["iters"]
    assert abs(float(three["err0"]) - K * float(one["err0"])) <= 1e-12 * K * float(one["err0"])
    d_est = max(em.est_diff(three["est"][c::K], one["est"]) for c in range(K))
    d_pts = float(np.abs(three["points"].reshape(-1, K, 3).astype(np.float64) - one["points"][:, None, :]).max())
    print("fix_scale %d: three copies against the ring: |d est| %.3g (4 x %.3g), |d pts| %.3g (4 x %.3g); the ring float64 vs long double %.3g" %
          (fix_scale, d_est, fam["band_est"][key], d_pts, fam["band_pts"][key], em.est_diff(one["est"], ld["est"])))
    assert d_est <= 4 * fam["band_est"][key] and d_pts <= 4 * fam["band_pts"][key]
    e0 = (np.asarray(one["edge_error0"], np.float64) ** 2).sum(axis=1)
    for name, copies in sorted(em.RING_COPIES.items()):
        f = em.reorder_figure(e0[em.replicate(p, copies).edge_source])
        print("%s fix_scale %d: err0 of %d copies forward against reversed %.3g; bound %.3g" % (name, fix_scale, copies, f, ring_err0_rtol(name, fix_scale)))
        assert f <= ring_err0_rtol(name, fix_scale) / 10 * 1.0001


# ------------------------------------------------------------------ 3. the C ABI before any device

def test_header_symbols_and_ctypes_layout(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    declared = set(re.findall(r"^int\s+(eg_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(capi.ESSENTIAL_GRAPH_SYMBOLS), declared ^ set(capi.ESSENTIAL_GRAPH_SYMBOLS)
    lib = capi.load()
    assert all(hasattr(lib, s) for s in capi.ESSENTIAL_GRAPH_SYMBOLS)
    assert "#define EG_MAX_FREE_KEYFRAMES %d" % capi.EG_MAX_FREE_KEYFRAMES in hdr and 7 * capi.EG_MAX_FREE_KEYFRAMES <= 8192
    import subprocess
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbgpu.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(eg_vertex), sizeof(eg_edge), sizeof(eg_point), sizeof(eg_problem), sizeof(eg_result), offsetof(eg_problem, lambda_init), "
                   "offsetof(eg_problem, device), offsetof(eg_result, err0), offsetof(eg_result, edge_error0)); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [capi.EG_VERTEX_DTYPE.itemsize, capi.EG_EDGE_DTYPE.itemsize, capi.EG_POINT_DTYPE.itemsize, C.sizeof(capi.EgProblem),
                   C.sizeof(capi.EgResult), capi.EgProblem.lambda_init.offset, capi.EgProblem.device.offset, capi.EgResult.err0.offset,
                   capi.EgResult.edge_error0.offset]


def _small():
    return api_arrays(em.flat_problem(em.collect_loop_form(em.make_scene(6, True, 11))))


def test_bad_arguments_are_refused_before_a_device_is_looked_for():
    """every refusal below comes back on a box without a GPU too: ORBG_NO_DEVICE would mean the device was asked first"""
    def rc_of(mut, **kw):
        V, E, P = _small()
        mut(V, E, P)
        return api.OptimizeEssentialGraph(V, E, P, raw=True, **kw)[0]

    def set_(arr, i, field, val):
        arr[field][i] = val

    assert rc_of(lambda V, E, P: set_(E, 0, "vi", len(V))) == capi.ORBG_BAD_ARG
    assert rc_of(lambda V, E, P: set_(E, 1, "vj", -1)) == capi.ORBG_BAD_ARG
    assert rc_of(lambda V, E, P: set_(E, 1, "vj", E["vi"][1])) == capi.ORBG_BAD_ARG
    assert rc_of(lambda V, E, P: set_(V, 2, "s", 0.0)) == capi.ORBG_BAD_ARG
    assert rc_of(lambda V, E, P: set_(V, 2, "s", -1.0)) == capi.ORBG_BAD_ARG
    assert rc_of(lambda V, E, P: set_(V, 1, "t", np.nan)) == capi.ORBG_BAD_ARG
    assert rc_of(lambda V, E, P: set_(E, 3, "q", np.inf)) == capi.ORBG_BAD_ARG
    assert rc_of(lambda V, E, P: set_(E, 3, "s", 0.0)) == capi.ORBG_BAD_ARG
    assert rc_of(lambda V, E, P: set_(P, 0, "ref", len(V))) == capi.ORBG_BAD_ARG
    assert rc_of(lambda V, E, P: set_(P, 0, "pos", np.nan)) == capi.ORBG_BAD_ARG
    assert rc_of(lambda V, E, P: None, lambda_init=float("nan")) == capi.ORBG_BAD_ARG
    # a short struct_size, NULL arguments
    lib = capi.load()
    V, E, P = _small()
    est = np.zeros((len(V), 8))
    pts = np.zeros((len(P), 3), np.float32)
    p = capi.EgProblem(C.sizeof(capi.EgProblem) - 4, len(V), V.ctypes.data, len(E), E.ctypes.data, 20, 1e-16, len(P), P.ctypes.data, 0)
    r = capi.EgResult(C.sizeof(capi.EgResult), est.ctypes.data, pts.ctypes.data, 0.0, 0.0, 0, None, 0, 0, None)
    assert lib.eg_solve(C.byref(p), C.byref(r)) == capi.ORBG_BAD_ARG
    p.struct_size = C.sizeof(capi.EgProblem)
    r.struct_size = 8
    assert lib.eg_solve(C.byref(p), C.byref(r)) == capi.ORBG_BAD_ARG
    assert lib.eg_solve(None, C.byref(r)) == capi.ORBG_BAD_ARG and lib.eg_solve(C.byref(p), None) == capi.ORBG_BAD_ARG


def test_too_many_free_keyframes_exceed_the_cap_before_a_device_is_looked_for():
    n = capi.EG_MAX_FREE_KEYFRAMES + 2
    V = np.zeros(n, capi.EG_VERTEX_DTYPE)
    V["q"][:, 3] = 1; V["s"] = 1; V["fixed"][0] = 1
    V["t"][:, 0] = np.arange(n)
    E = np.zeros(n - 1, capi.EG_EDGE_DTYPE)
    E["vi"], E["vj"] = np.arange(1, n), np.arange(n - 1)
    E["q"][:, 3] = 1; E["s"] = 1; E["t"][:, 0] = -1
    assert api.OptimizeEssentialGraph(V, E, raw=True)[0] == capi.ORBG_CAP_EXCEEDED
    V["fixed"][1] = 1                                     # exactly the cap: no refusal by size (no device: ORBG_NO_DEVICE)
    assert api.OptimizeEssentialGraph(V, E, iterations=0, raw=True)[0] == capi.ORBG_OK


def test_problems_that_need_no_launch_are_answered_on_the_host():
    """no free vertex, no edge, no iteration: the estimates come back as they went in, the points go through them, chi2 is evaluated"""
    p = em.flat_problem(em.collect_loop_form(em.make_scene(6, False, 12)))
    ref = em.run(p, iterations=0)
    V, E, P = api_arrays(p)
    for variant in ("iterations", "all_fixed", "no_edges"):
        V2, E2 = V.copy(), E
        kw = {}
        if variant == "iterations":
            kw["iterations"] = 0
        elif variant == "all_fixed":
            V2["fixed"] = 1
        else:
            E2 = E[:0]
        rc, out = api.OptimizeEssentialGraph(V2, E2, P, raw=True, **kw)
        assert rc == capi.ORBG_OK, variant
        assert out.iters == 0 and len(out.trace) == 0
        assert np.array_equal(out.estimates, np.concatenate([p.q, p.t, p.s[:, None]], axis=1))
        if variant == "no_edges":
            assert out.err0 == 0 and out.errEnd == 0
        else:
            assert out.err0 == out.errEnd and abs(out.err0 - float(ref["err0"])) <= 1e-12 * float(ref["err0"])
            assert np.abs(out.edge_error0 - ref["edge_error0"]).max() <= 1e-13
        keep = p.ref < 0
        assert out.points[keep].tobytes() == p.pos[keep].tobytes()
        assert np.abs(out.points - ref["points"]).max() <= 2 * np.spacing(np.float32(np.abs(ref["points"]).max()))
