"""Optimizer::InertialOptimization without a device: the kernel's edge arithmetic compiled for the host (inertial_init_host_linearize)
against tests/inertial_init_model.py and against central differences through the vertices' own oplus; the model's two solve formulations
against each other (the yardsticks of tests/test_gpu_inertial_init.py, printed); every refusal that needs no device; the scenes' distance
from every decision threshold."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import inertial_init_model as m
import pose_inertial_model as pim
from multi_orbslam3_amd import _capi as capi, views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_CASES = ("n2", "n10_mono", "n10_bias", "fork", "newest_first")


def _linearize(P):
    lib = capi.load()
    p, keep = m.to_c_problem(P)
    J = np.zeros((p.n_edges, 9, 16))
    assert lib.inertial_init_host_linearize(C.byref(p), J.ctypes.data) == capi.ORBG_OK
    return J


def _moved(P, bias=0.0):
    """the estimates handed in, with a bias away from zero and from every edge's linearisation bias (the Jacobian's general branch)"""
    P = dict(P)
    P["bg"] = (P["truth"]["bg"] + bias * np.array([1.0, -0.5, 0.25])).astype(np.float32)
    P["ba"] = (P["truth"]["ba"] + 10 * bias * np.array([0.3, 1.0, -0.6])).astype(np.float32)
    return P


@pytest.mark.parametrize("name", EDGE_CASES)
def test_kernel_edge_arithmetic_on_the_host(name):
    """EdgeInertialGS, error and all eight Jacobians (the two pose blocks do not exist: every pose is fixed), against the model.  Same
    formulas in another operation order: 1e-12 relative to the largest entry (tests/test_pose_inertial_cpu.py's tolerance for
    EdgeInertial)."""
    for bias in (0.0, 2e-3):
        P = _moved(m.build_case(name), bias)
        J = _linearize(P)
        S = m.initial_state(P)
        for e in range(len(P["edges"])):
            want = m.edge_block(P, S, e)
            assert np.abs(J[e][:, :15] - want[:, :15]).max() <= 1e-12 * np.abs(want[:, :15]).max(), (name, e)
            assert np.abs(J[e][:, 15] - want[:, 15]).max() <= 1e-12 * max(np.abs(want[:, 15]).max(), 1.0), (name, e)


def test_vectorised_model_is_the_edge_by_edge_one():
    """the model evaluates all edges at once (einsum) for speed; the edge-by-edge restatement of the reference's text is its definition"""
    for variant in ("kernel", "reference"):
        P = _moved(m.build_case("fork"), 2e-3)
        G, S = m.Graph(P), m.initial_state(P)
        err, J = m._errors_jacobians(P, G, S, variant, True)
        for e in range(G.ne):
            want = m.edge_block(P, S, e, variant)
            assert np.abs(J[e] - want[:, :15]).max() <= 1e-13 * np.abs(want[:, :15]).max()
            assert np.abs(err[e] - want[:, 15]).max() <= 1e-13 * max(np.abs(want[:, 15]).max(), 1.0)


def test_jacobians_against_central_differences():
    """The host-compiled Jacobians against central differences of the MODEL's error through each vertex's own oplus (velocities and biases
    add; VertexGDir: Rwg ExpSO3(u0, u1, 0); VertexScale: s exp(u)).  Step and tolerance as tests/test_pose_inertial_cpu.py: h = 1e-6,
    1e-6 relative to the largest Jacobian entry of the edge."""
    h, tol = 1e-6, 1e-6
    P = _moved(m.build_case("n10_mono"), 2e-3)
    J = _linearize(P)
    S = m.initial_state(P)

    def err(S2, e):
        return m.edge_block(P, S2, e)[:, 15]

    def moved(S0, col, d, k1, k2):
        T = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in S0.items()}
        if col < 3:
            T["v"][k1, col] += d
        elif col < 6:
            T["v"][k2, col - 3] += d
        elif col < 9:
            T["bg"][col - 6] += d
        elif col < 12:
            T["ba"][col - 9] += d
        elif col < 14:
            u = np.zeros(2)
            u[col - 12] = d
            T["Rwg"] = m.gdir_oplus(S0["Rwg"], u)
        else:
            T["s"] = m.scale_oplus(S0["s"], d)
        return T

    worst = 0.0
    for e, E in enumerate(P["edges"]):
        num = np.stack([(err(moved(S, c, h, E["k1"], E["k2"]), e) - err(moved(S, c, -h, E["k1"], E["k2"]), e)) / (2 * h) for c in range(15)], axis=1)
        worst = max(worst, np.abs(num - J[e][:, :15]).max() / np.abs(J[e][:, :15]).max())
    print("largest difference to central differences, relative to the edge's largest entry: %.2e" % worst)
    assert worst < tol


def test_prior_edges_keep_the_reference_sign():
    """EdgePriorAcc / EdgePriorGyro: the error is (0 - bias), linearizeOplus says +I (S/G2oTypes.cc:971-983): the model's right-hand side
    moves a bias AWAY from zero, as g2o's does with that Jacobian."""
    P = _moved(m.build_case("n10_mono"), 0.0)
    G, S = m.Graph(P), m.initial_state(P)
    L0 = m.linearise(dict(P, prior_g=0.0, prior_a=0.0), G, S, "kernel")
    L1 = m.linearise(P, G, S, "kernel")
    assert np.allclose(L1["rc"][0:3] - L0["rc"][0:3], P["prior_g"] * S["bg"], rtol=1e-9)
    assert np.allclose(L1["rc"][3:6] - L0["rc"][3:6], P["prior_a"] * S["ba"], rtol=1e-9)
    assert np.allclose(np.diag(L1["C"] - L0["C"])[:6], [P["prior_g"]] * 3 + [P["prior_a"]] * 3, rtol=1e-9)


@pytest.mark.parametrize("name", list(m.CASES))
def test_solve_formulations_and_conditions(name):
    """(a) dense normal equations against (b) the kernel's elimination order: same control flow, and their difference -- the yardstick
    of the GPU test -- printed.  No LM decision of the case, in either formulation or in reference arithmetic, lies within a relative
    1e-4 of its threshold; every case reaches what its name says."""
    P, rb, ra, rr = m.case_results(name)
    y = m.yardsticks_of(rb, ra)
    lam_b, chi_b, noise, f = m.trace_bounds(rb, ra)
    print("%s: unknowns %d iters %d trials %s | (a)-(b) state %.3e, chi2 rows %.3e; lambda amplification %.3e -> lambda bound %.3e; "
          "kernel-reference state %.3e" % (name, rb["n_unknowns"], rb["iters"], "".join("%x" % int(q) for q in rb["trace"][:, 2]), y["ab_state"], f,
                                          rb["lambda_amp"].max(initial=0.0), lam_b.max(initial=0.0), m.state_difference(rr, rb)))
    for r in (ra, rr):
        assert r["iters"] == rb["iters"] and r["solve_failed"] == rb["solve_failed"] and np.array_equal(r["trace"][:, 2], rb["trace"][:, 2])
    assert not noise.any()
    for r in (rb, ra, rr):
        if r["lm_decisions"]:
            assert not m.near_threshold(r["lm_decisions"]).any(), name
    assert y["ab_state"] < 1e-9                                    # the two formulations solve the same problem
    assert m.state_difference(rr, rb) < 1e-4                       # float round trips, no more
    G = m.Graph(P)
    q = rb["trace"][:, 2]
    ended_by_count = rb["iters"] == P["iterations"]
    if name == "n2":
        assert rb["n_unknowns"] == 15
    if name in ("n10_mono", "n10_auto_lambda", "rejected", "newest_first"):
        assert rb["n_unknowns"] == 3 * 10 + 9 or name == "newest_first"
    if name == "n10_stereo":
        assert rb["n_unknowns"] == 38 and rb["scale"] == 1.0
    if name == "n10_auto_lambda":
        assert P["lambda_init"] == 0.0
    if name == "n10_fixed_vel":
        assert rb["n_unknowns"] == 3 and np.array_equal(rb["vwb"], P["keyframes"]["v"].astype(np.float64))
    if name == "n10_bias":
        assert rb["n_unknowns"] == 36 and np.array_equal(rb["Rwg"], np.eye(3)) and rb["scale"] == 1.0
    if name == "n10_gn":
        assert P["algorithm"] == m.GN and rb["iters"] == 10 and rb["n_unknowns"] == 3 and not rb["solve_failed"]
        assert rb["chi2_final"] < 1e-2 * rb["chi2_first"]
    if name == "gn_degenerate":
        assert rb["solve_failed"] == 1 and rb["iters"] == 1 and rb["scale"] == P["scale"] and np.array_equal(rb["Rwg"], P["Rwg"])
    if name == "newest_first":
        assert np.all(G.k1 > G.k2)
    if name == "broken":
        assert (G.pred[G.in_system] < 0).sum() == 2
    if name == "isolated":
        k = m.CASES[name]["isolated"][0]
        assert not G.in_system[k] and np.array_equal(rb["vwb"][k], P["keyframes"]["v"][k].astype(np.float64))
    if name == "fork":
        assert np.bincount(G.k1).max() == 2
    if name == "rejected":
        assert any(1 < x < 10 for x in q)
    if name == "nbad_stop":
        assert not ended_by_count and q[-1] < 10
    if name == "runs_out":
        assert ended_by_count and q[-1] < 10
    if name.startswith("edges"):
        assert G.ne == int(name[5:])
    if name.startswith("tile"):
        assert G.nk == m.TILE + int(name[4:])
    if name == "cap":
        assert G.nk == capi.INERTIAL_INIT_MAX_KEYFRAMES == m.CAP


def test_near_threshold_decisions_over_every_case():
    """accept / reject, the _nBad test and pivot positivity over every case: at most BAND_CAP of them within a relative 1e-4 of a threshold"""
    dec = []
    for name in m.CASES:
        rb = m.case_results(name)[1]
        dec += rb["decisions"] + rb["lm_decisions"]
    near = m.near_threshold(dec)
    print("%d decisions, %d in the band" % (len(dec), int(near.sum())))
    assert near.mean() <= m.BAND_CAP


def test_noise_free_scene_is_recovered():
    """a consistent scene without measurement noise: the first overload finds the gravity direction and the scale the scene was made with,
    as far as the float inputs carry them"""
    P = m.make_scene(n=12, seed=3, noise=0.0, **dict(m.form_problem(1, bMono=True, priorG=0.0, priorA=0.0), iterations=30))
    r = m.solve(P)
    g_est, g_true = r["Rwg"] @ m.GI, P["truth"]["Rwg"] @ m.GI
    assert np.abs(g_est - g_true).max() < 1e-3 and abs(r["scale"] - P["truth"]["s"]) < 1e-3
    assert np.abs(r["bg"] - P["truth"]["bg"]).max() < 1e-4
    assert r["chi2_final"] < 1e-6 * r["chi2_first"]


def _small():
    P = m.build_case("n10_mono")
    p, keep = m.to_c_problem(P)
    return P, p, keep, views.InertialInitOutput(p)


def test_argument_checks_and_no_device():
    lib = capi.load()
    P, p, keep, out = _small()
    call = lambda: lib.inertial_init_solve(C.byref(p), C.byref(out.c))
    if lib.orbg_device_count() <= 0:
        assert call() == capi.ORBG_NO_DEVICE
        assert lib.inertial_init_set_stream(0, None) == capi.ORBG_NO_DEVICE
    assert lib.inertial_init_solve(None, C.byref(out.c)) == capi.ORBG_BAD_ARG
    assert lib.inertial_init_solve(C.byref(p), None) == capi.ORBG_BAD_ARG
    for field, bad in (("algorithm", 2), ("iterations", -1), ("struct_size", 8), ("n_edges", 0), ("edges", None), ("keyframes", None),
                       ("n_keyframes", -1), ("prior_g", -1.0)):
        old = getattr(p, field)
        setattr(p, field, bad)
        assert call() == capi.ORBG_BAD_ARG, field
        setattr(p, field, old)
    # no free unknown
    flags = [p.free_velocity, p.free_bias, p.free_gdir, p.free_scale]
    p.free_velocity = p.free_bias = p.free_gdir = p.free_scale = 0
    assert call() == capi.ORBG_BAD_ARG
    p.free_velocity, p.free_bias, p.free_gdir, p.free_scale = flags
    out.c.vwb, keep_v = None, out.c.vwb
    assert call() == capi.ORBG_BAD_ARG
    out.c.vwb = keep_v
    out.c.struct_size = 4
    assert call() == capi.ORBG_BAD_ARG
    out.c.struct_size = C.sizeof(capi.InertialInitResult)
    J = np.zeros((p.n_edges, 9, 16))
    assert lib.inertial_init_host_linearize(C.byref(p), None) == capi.ORBG_BAD_ARG
    assert lib.inertial_init_host_linearize(None, J.ctypes.data) == capi.ORBG_BAD_ARG


def _graph_problem(pairs, n=6):
    """the n10_mono scene's first keyframes with another edge list"""
    P = m.build_case("n10_mono")
    P = dict(P, edges=[dict(P["edges"][i % len(P["edges"])], k1=a, k2=b) for i, (a, b) in enumerate(pairs)])
    P["keyframes"] = {k: v[:n] for k, v in P["keyframes"].items()}
    return m.to_c_problem(m.finish(P))


@pytest.mark.parametrize("pairs,code", [
    ([(0, 1), (1, 6)], capi.ORBG_BAD_ARG),                     # an index out of range
    ([(0, 1), (-1, 2)], capi.ORBG_BAD_ARG),
    ([(0, 2), (1, 2)], capi.ORBG_BAD_ARG),                     # a keyframe that is k2 of two edges: two mPrevKF
    ([(0, 1), (1, 2), (2, 0)], capi.ORBG_BAD_ARG),             # a cycle
    ([(0, 1), (2, 3), (3, 2)], capi.ORBG_BAD_ARG),             # a cycle next to a chain
    ([(1, 1)], capi.ORBG_BAD_ARG),                             # the shortest cycle
    ([(0, 1), (0, 2), (0, 3), (3, 4)], None),                  # a fork is accepted
    ([(5, 4), (4, 3), (3, 2)], None),                          # newest first
])
def test_graph_checks(pairs, code):
    lib = capi.load()
    p, keep = _graph_problem(pairs)
    out = views.InertialInitOutput(p)
    rc = lib.inertial_init_solve(C.byref(p), C.byref(out.c))
    J = np.zeros((p.n_edges, 9, 16))
    rl = lib.inertial_init_host_linearize(C.byref(p), J.ctypes.data)
    if code is None:
        assert rl == capi.ORBG_OK
        assert rc == (capi.ORBG_OK if lib.orbg_device_count() > 0 else capi.ORBG_NO_DEVICE)
    else:
        assert rc == code and rl == code


def test_cap_is_checked_before_a_device_is_looked_for():
    lib = capi.load()
    n = capi.INERTIAL_INIT_MAX_KEYFRAMES + 1
    K = np.zeros((n, capi.INERTIAL_INIT_STATE_FLOATS), np.float32)
    E = np.zeros(n - 1, capi.INERTIAL_INIT_EDGE_DTYPE)
    E["k1"], E["k2"] = np.arange(n - 1), np.arange(1, n)
    p, keep = views.inertial_init_problem(K, E, np.zeros(3), np.zeros(3))
    out = views.InertialInitOutput(p)
    assert lib.inertial_init_solve(C.byref(p), C.byref(out.c)) == capi.ORBG_CAP_EXCEEDED
    assert m.kernel_constant("kIiTile") < capi.INERTIAL_INIT_MAX_KEYFRAMES


def test_ctypes_mirrors_match_the_header(tmp_path):
    """sizes and the offsets of every field of the three structs, from a C program compiled against include/orbgpu.h"""
    pairs = {"inertial_init_edge": capi.InertialInitEdge, "inertial_init_problem": capi.InertialInitProblem,
             "inertial_init_result": capi.InertialInitResult}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "orbgpu.h"', "int main(void) {",
             'printf("cap %d\\n", INERTIAL_INIT_MAX_KEYFRAMES);', 'printf("lm %d\\n", INERTIAL_INIT_LM);', 'printf("gn %d\\n", INERTIAL_INIT_GN);']
    for cname, cls in pairs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ["return 0; }"]
    src = tmp_path / "m.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "m"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, (cname, f)
    assert (int(got["cap"]), int(got["lm"]), int(got["gn"])) == (capi.INERTIAL_INIT_MAX_KEYFRAMES, capi.INERTIAL_INIT_LM, capi.INERTIAL_INIT_GN)
    assert (m.LM, m.GN) == (capi.INERTIAL_INIT_LM, capi.INERTIAL_INIT_GN)
    hdr = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    declared = set(re.findall(r"^int\s+(inertial_init_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(capi.INERTIAL_INIT_SYMBOLS)
    lib = capi.load()
    for sym in capi.INERTIAL_INIT_SYMBOLS:
        assert hasattr(lib, sym)
