"""inertial_ba_solve without a device: the numpy model itself (its Jacobians, the Schur complement against a dense brute-force solve,
its two variants, forward against reversed sums), the conditions the GPU test relies on (the decisions near a threshold, the property
every case exists for), the kernels' edge arithmetic compiled for the host, and every refusal of the C ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import inertial_ba_model as m
from multi_orbslam3_amd import _capi as capi, views

pim = m.pim
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(m.CASES)
SMALL = ("n1", "n2", "n2_recinit", "inertial_only", "no_imu_middle", "n4_newest_first", "rejected", "stale")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_library_exports_what_the_header_declares():
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    declared = set(re.findall(r"^int\s+(inertial_ba_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(capi.INERTIAL_BA_SYMBOLS), declared ^ set(capi.INERTIAL_BA_SYMBOLS)
    for s in declared:
        assert hasattr(lib, s), s


def test_structs_match_the_header(tmp_path):
    fields = {"inertial_ba_keyframe": ("InertialBaKeyframe", ["state", "fixed", "imu", "link", "prev", "last_in_window", "preint", "info9", "infoG", "infoA"]),
              "inertial_ba_problem": ("InertialBaProblem", ["struct_size", "n_keyframes", "n_edges", "keyframes", "points", "edges", "close", "rec_init",
                                                            "large", "fx", "bf", "Tcb", "device"]),
              "inertial_ba_result": ("InertialBaResult", ["struct_size", "states", "points", "edge_chi2", "edge_depth_pos", "edge_outlier", "n_outliers",
                                                          "failed", "iters", "chi2_initial", "chi2_final", "trace", "trace_cap", "trace_len"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "orbgpu.h"', 'int main(void) {']
    for cname, (_, fl) in fields.items():
        lines.append('  printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for f in fl:
            lines.append('  printf(" %%zu", offsetof(%s, %s));' % (cname, f))
        lines.append('  printf("\\n");')
    lines.append('  printf("consts %d %d %zu\\n", INERTIAL_BA_MAX_FREE_KEYFRAMES, INERTIAL_BA_MAX_EDGES, sizeof(inertial_ba_state));')
    lines.append("  return 0; }")
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    for ln in subprocess.check_output([str(exe)]).decode().splitlines():
        parts = ln.split()
        if parts[0] == "consts":
            assert [int(x) for x in parts[1:]] == [capi.INERTIAL_BA_MAX_FREE_KEYFRAMES, capi.INERTIAL_BA_MAX_EDGES, 8 * capi.INERTIAL_BA_STATE_DOUBLES]
            continue
        pyname, fl = fields[parts[0]]
        cls = getattr(capi, pyname)
        assert C.sizeof(cls) == int(parts[1]), parts[0]
        for f, off in zip(fl, parts[2:]):
            assert getattr(cls, f).offset == int(off), (parts[0], f)


def _call(P, mutate=None):
    """inertial_ba_solve on the problem of P after mutate(problem, keyframes array, keep-alive); returns the code"""
    lib = capi.load()
    p, keep = m.to_c_problem(P)
    out = views.InertialBaOutput(p)
    if mutate:
        mutate(p, keep[0], out)
    return lib.inertial_ba_solve(C.byref(p), C.byref(out.c))


def test_every_refusal_comes_before_a_device_is_looked_for():
    """BAD_ARG / CAP_EXCEEDED are what a machine without a device answers too; a problem that passes gets as far as the device"""
    lib = capi.load()
    P = m.build_case("n2")
    n_kf, n_pt, n_e = len(P["kfs"]), len(P["points"]), len(P["edges"])
    has_gpu = lib.orbg_device_count() > 0
    assert _call(P) == (capi.ORBG_OK if has_gpu else capi.ORBG_NO_DEVICE)
    assert lib.inertial_ba_solve(None, None) == capi.ORBG_BAD_ARG
    bad = {
        "problem struct_size": lambda p, K, o: setattr(p, "struct_size", C.sizeof(capi.InertialBaProblem) - 1),
        "result struct_size": lambda p, K, o: setattr(o.c, "struct_size", 8),
        "no keyframes": lambda p, K, o: setattr(p, "n_keyframes", 0),
        "negative points": lambda p, K, o: setattr(p, "n_points", -1),
        "negative edges": lambda p, K, o: setattr(p, "n_edges", -1),
        "keyframes NULL": lambda p, K, o: setattr(p, "keyframes", None),
        "states NULL": lambda p, K, o: setattr(o.c, "states", None),
        "points NULL": lambda p, K, o: setattr(p, "points", None),
        "close NULL": lambda p, K, o: setattr(p, "close", None),
        "result points NULL": lambda p, K, o: setattr(o.c, "points", None),
        "edges NULL": lambda p, K, o: setattr(p, "edges", None),
        "edges without points": lambda p, K, o: setattr(p, "n_points", 0),
        "trace_cap": lambda p, K, o: setattr(o.c, "trace_cap", -1),
        "last_in_window without link": lambda p, K, o: (setattr(K[2], "link", 0), setattr(K[2], "last_in_window", 1)),
        "link on a fixed keyframe": lambda p, K, o: setattr(K[1], "fixed", 1),
        "link without imu": lambda p, K, o: setattr(K[2], "imu", 0),
        "prev without imu": lambda p, K, o: setattr(K[0], "imu", 0),
        "prev below range": lambda p, K, o: setattr(K[1], "prev", -1),
        "prev above range": lambda p, K, o: setattr(K[1], "prev", n_kf),
        "prev is itself": lambda p, K, o: setattr(K[1], "prev", 1),
        "no free keyframe": lambda p, K, o: [setattr(K[i], "fixed", 1) for i in range(n_kf)],
    }
    for what, f in bad.items():
        assert _call(P, f) == capi.ORBG_BAD_ARG, what

    def edit_edge(k, field, value):
        def f(p, K, o):
            E = np.frombuffer(C.string_at(p.edges, n_e * capi.EDGE_DTYPE.itemsize), capi.EDGE_DTYPE).copy()
            E[field][k] = value
            f.keep = E
            p.edges = capi.ptr(E)
        return f
    E0 = np.asarray(P["edges"])
    dup = int(np.flatnonzero(E0["point"][1:] == E0["point"][:-1])[0]) + 1             # second edge of a point: make it the first one's keyframe
    for what, f in {"edge keyframe below range": edit_edge(0, "pose", -1), "edge keyframe above range": edit_edge(0, "pose", n_kf),
                    "edge point below range": edit_edge(0, "point", -1), "edge point above range": edit_edge(n_e - 1, "point", n_pt),
                    "a right-camera edge": edit_edge(3, "ur", capi.UR_RIGHT_CAMERA), "point decreases": edit_edge(n_e - 1, "point", 0),
                    "two edges of one keyframe and point": edit_edge(dup, "pose", int(E0["pose"][dup - 1]))}.items():
        assert _call(P, f) == capi.ORBG_BAD_ARG, what
    # the caps: more edges than INERTIAL_BA_MAX_EDGES (refused before an edge is read), more free keyframes than the window may hold
    assert _call(P, lambda p, K, o: setattr(p, "n_edges", capi.INERTIAL_BA_MAX_EDGES + 1)) == capi.ORBG_CAP_EXCEEDED
    big = m.make_scene(n_free=capi.INERTIAL_BA_MAX_FREE_KEYFRAMES + 1, n_points=0, seed=5, steps=2)
    assert _call(big) == capi.ORBG_CAP_EXCEEDED
    assert m.Structure(m.build_case("n32_cap")).nF == capi.INERTIAL_BA_MAX_FREE_KEYFRAMES        # (solved in tests/test_gpu_inertial_ba.py)
    assert _call(m.build_case("n32_cap")) == (capi.ORBG_OK if has_gpu else capi.ORBG_NO_DEVICE)
    # the handle form and the test aid
    assert lib.inertial_ba_create(0, None) == capi.ORBG_BAD_ARG
    assert lib.inertial_ba_destroy(None) == capi.ORBG_BAD_ARG
    assert lib.inertial_ba_solve_h(None, None, None) == capi.ORBG_BAD_ARG
    assert lib.inertial_ba_set_stream(None, None) == capi.ORBG_BAD_ARG
    assert lib.inertial_ba_host_linearize(None, None, None) == capi.ORBG_BAD_ARG
    p, keep = m.to_c_problem(P)
    assert lib.inertial_ba_host_linearize(C.byref(p), None, None) == capi.ORBG_BAD_ARG
    if not has_gpu:
        h = C.c_void_p()
        assert lib.inertial_ba_create(0, C.byref(h)) == capi.ORBG_NO_DEVICE and not h


# ------------------------------------------------------------------------------------------------ the model
def _numeric(f, n_in, h):
    cols = []
    for k in range(n_in):
        d = np.zeros(n_in)
        d[k] = h
        cols.append((f(d) - f(-d)) / (2 * h))
    return np.stack(cols, axis=1)


def test_visual_jacobians_against_central_differences():
    """EdgeMono / EdgeStereo's two blocks against central differences through the vertices' own oplus (the point: X + d; the pose:
    ImuCamPose::Update on the body).  Step and tolerance as in tests/test_pose_inertial_cpu.py: at h = 1e-6 truncation (h^2 |f'''| / 6)
    and rounding (eps |f| / h, residuals of order 1 .. 500 pixels) both stay below 1e-6 of the largest entry of the block."""
    h, tol = 1e-6, 1e-6
    P = m.build_case("n2")
    S = m.Structure(P)
    kfs, X = m.initial_state(P)
    err, Xc, c2, Rcw = m.visual_edges(P, S, kfs, X)
    Jl, Jp = m.visual_jacobians(P, S, Xc, Rcw)
    assert (~S.mono).any() and S.mono.any()
    worst = 0.0
    for k in list(np.flatnonzero(S.mono)[:6]) + list(np.flatnonzero(~S.mono)[:6]):
        def f_point(d, k=k):
            X2 = X.copy()
            X2[S.e_pt[k]] += d
            return m.visual_edges(P, S, kfs, X2)[0][k]

        def f_pose(d, k=k):
            k2 = list(kfs)
            k2[S.e_kf[k]] = pim.oplus(kfs[S.e_kf[k]], np.concatenate([d, np.zeros(9)]))
            return m.visual_edges(P, S, k2, X)[0][k]
        worst = max(worst, np.abs(Jl[k] - _numeric(f_point, 3, h)).max() / np.abs(Jl[k]).max(), np.abs(Jp[k] - _numeric(f_pose, 6, h)).max() / np.abs(Jp[k]).max())
        if S.mono[k]:
            assert not Jl[k][2].any() and not Jp[k][2].any() and err[k][2] == 0
    print("visual Jacobians against central differences: %.3e" % worst)
    assert worst <= tol


@pytest.mark.parametrize("name", SMALL)
def test_schur_complement_against_a_dense_solve(name):
    """The model with every unknown -- keyframes and points -- in one numpy.linalg.solve per trial, no Schur complement, no LDL^T: another
    order of operations on the same mathematics, held to the bounds the device is held to."""
    P, rb, rr, ra = m.case_results(name)
    d = m.solve(P, dense=True)
    y = m.yardsticks_of(rb, rr, ra)
    ds, dt = m.state_difference(d, rb), m.trace_difference(d, rb)
    print("%s: dense-Schur state %.3e (bound %.3e), trace %.3e (bound %.3e)" % (name, ds, m.MARGIN * y["fr_state"], dt, max(1e-9, 10 * y["fr_trace"])))
    assert ds <= m.MARGIN * y["fr_state"]
    assert dt <= max(1e-9, 10 * y["fr_trace"])
    assert np.array_equal(d["edge_outlier"], rb["edge_outlier"]) and d["failed"] == rb["failed"] and d["iters"] == rb["iters"]


@pytest.mark.parametrize("name", NAMES)
def test_variants_and_reversed_sums_agree_on_every_decision(name):
    """(a) against (b) and forward against reversed: the same trial counts, iterations and `failed`; the same verdicts outside the band.
    At most BAND_CAP of a case's decisions lie within a relative 1e-4 of their threshold, and none of them is an LM decision or a depth
    test: the GPU test compares those outright."""
    P, rb, rr, ra = m.case_results(name)
    S = m.Structure(P)
    near = m.near_threshold(rb["decisions"])
    n_edge = S.NE
    print("%s: %d of %d decisions in the band; yardsticks %s" % (name, int(near.sum()), len(near), {k: "%.3e" % v for k, v in m.yardsticks_of(rb, rr, ra).items() if k != "fr_rows"}))
    assert near.sum() <= m.BAND_CAP * len(near)
    assert not near[n_edge:].any()                                      # depth tests, `failed`, gain ratios, the stop rule
    for r in rr + [ra]:
        assert np.array_equal(r["trace"][:, 2], rb["trace"][:, 2]) and r["iters"] == rb["iters"] and r["failed"] == rb["failed"]
        sure = ~near[:n_edge]
        assert np.array_equal(r["edge_outlier"][sure], rb["edge_outlier"][sure])
        assert np.array_equal(r["edge_depth_pos"], rb["edge_depth_pos"])


def test_each_case_has_the_property_it_exists_for():
    res = {n: m.case_results(n) for n in NAMES}
    S = {n: m.Structure(res[n][0]) for n in NAMES}
    # n1: 15 unknowns; the only inertial edge is the window's last one: down-weighted, with a kernel
    assert S["n1"].n == 15 and S["n1"].inertial == [(0, 1, True)] and res["n1"][0]["kfs"][1]["last_in_window"]
    assert len(res["n1"][0]["points"]) == 30 and [k["fixed"] for k in res["n1"][0]["kfs"]] == [True, False]
    # n2: only the last edge has a kernel; rec_init: every one
    assert [r for _, _, r in S["n2"].inertial] == [True, False] and [r for _, _, r in S["n2_recinit"].inertial] == [True, True]
    # the kernel matters: EdgeInertial's chi2 of the first linearisation is beyond delta^2 = 16.92 on the edge that gets it only with rec_init
    kfs, _ = m.initial_state(res["n2"][0])
    e = m.inertial_edges(res["n2"][0], S["n2"], kfs)[1]
    assert float(e[4][0:9] @ (e[5] @ e[4][0:9])) > 16.92
    assert S["inertial_only"].NE == 0 and S["inertial_only"].NX == 0 and S["inertial_only"].nF == 3 and S["inertial_only"].n == 45
    # n10: the reference's normal call
    P = res["n10"][0]
    s = S["n10"]
    rb = res["n10"][1]
    assert s.nF == 10 and sum(k["fixed"] for k in P["kfs"]) == 5 and s.NX == 300 and s.mono.any() and (~s.mono).any() and not P["large"]
    assert (rb["edge_depth_pos"] == 0).any() and s.mono[rb["edge_depth_pos"] == 0].all()
    close = np.asarray(P["close"], bool)[s.e_pt]
    between = s.mono & close & (rb["edge_chi2"] > m.CHI2_MONO) & (rb["edge_chi2"] < m.CHI2_CLOSE) & (rb["edge_depth_pos"] == 1)
    assert between.any() and not rb["edge_outlier"][between].any()           # kept because the point is close
    assert (s.mono & ~close & (rb["edge_chi2"] > m.CHI2_MONO)).any() and ((~s.mono) & (rb["edge_chi2"] > m.CHI2_STEREO)).any()
    assert 0.03 < rb["n_outliers"] / s.NE < 0.08
    assert S["n19"].n == 285 and S["n25_large"].n == 375 and res["n25_large"][0]["large"] and res["n25_large"][1]["iters"] == 4
    # no_imu_middle: 15 | 6 | 15 | 15 at offsets 0, 15, 21, 36; the chain is broken at the keyframe without IMU
    s = S["no_imu_middle"]
    assert list(s.col_dim) == [15, 6, 15, 15] and list(s.col_off) == [0, 15, 21, 36] and [(a, b) for a, b, _ in s.inertial] == [(0, 1), (3, 4)]
    # rejected: an iteration in the middle of the run with more than one trial; the run ends on an accepted one
    tr = res["rejected"][1]["trace"][:, 2]
    assert tr[:-1].max() >= 2 and tr[-1] == 1 and not res["rejected"][1]["last_rejected"]
    # the glue's keyframe order: the earlier keyframe of every inertial edge between free keyframes has the larger column
    for n in ("n4_newest_first", "n10_newest_first"):
        s = S[n]
        assert all(s.kf_col[k1] > s.kf_col[k2] for k1, k2, _ in s.inertial if s.kf_col[k1] >= 0) and sum(s.kf_col[k1] >= 0 for k1, _, _ in s.inertial) == s.nF - 1
        assert s.kf_col[s.inertial[-1][0]] == -1 and s.inertial[-1][2]              # the window's last edge ends in the fixed predecessor
    # laps: points, edges of every keyframe and items of the pair one below, at and one above the lap; three full workgroups of edges
    for d in (-1, 0, 1):
        s = S["lap%+d" % d]
        assert s.NX == m.LAP + d and s.NE == 3 * (m.LAP + d) and all((s.e_kf == k).sum() == m.LAP + d for k in range(3))
    assert m.LAP == 256


def test_stale_case_ends_on_a_rejected_trial_and_the_rule_matters_there():
    """The run ends on a rejected trial, and structurally so: the observation at u = 1e33 carries a robustified chi2 that is the same
    number at every estimate, and half a unit in its last place exceeds everything else the sum holds by orders, so chi2 of the trial
    equals the current one in every order of summation: rho == 0.  A fresh evaluation at the returned estimate gives other verdicts."""
    P, rb, rr, ra = m.case_results("stale")
    s = m.Structure(P)
    for r in [rb, ra, m.solve(P, dense=True)] + rr:
        assert r["last_rejected"] and r["iters"] == 1 and r["trace"][:, 2].tolist() == [1.0] and r["chi2_final"] == r["chi2_initial"] == rb["chi2_initial"]
    big = int(np.flatnonzero(np.asarray(P["edges"])["u"] == np.float32(m.HUGE_U))[0])
    kfs0, X0 = m.initial_state(P)
    c2_start = m.visual_edges(P, s, kfs0, X0)[2]
    huge_term = float(m._huber(float(np.float32(m.HUGE_U)) ** 2 * s.om[big], m.DELTA_MONO)[0])
    for c2 in (c2_start, rb["edge_chi2"]):                                  # at the start, and at the rejected trial
        rho0 = m._huber(c2, np.where(s.mono, m.DELTA_MONO, m.DELTA_STEREO))[0]
        assert rho0[big] == huge_term                                       # u - pu == u: the projection is absorbed
        assert float(np.delete(rho0, big).sum()) < 1e-6 * 0.5 * np.spacing(huge_term)
    inertial = sum(m.inertial_chi2(ie)[0] for ie in m.inertial_edges(P, s, kfs0, with_jacobians=False))
    assert inertial < 1e-6 * 0.5 * np.spacing(huge_term) and rb["chi2_initial"] == huge_term
    # the vertices are the start's; the errors are the trial's, a full step away
    assert m.state_difference(rb, {"states": kfs0, "points": X0}) == 0.0
    assert np.abs(rb["edge_chi2"] - c2_start).max() > 1e3 and np.array_equal(rb["edge_chi2_fresh"], c2_start)
    fresh = m.solve(P, fresh_chi2=True)
    assert m.state_difference(fresh, rb) == 0.0
    assert (fresh["edge_outlier"] != rb["edge_outlier"]).sum() > 100 and rb["n_outliers"] < fresh["n_outliers"]


def test_model_restates_the_thresholds_as_floats():
    assert m.CHI2_CLOSE == float(np.float32(1.5) * np.float32(5.991)) != 1.5 * 5.991
    assert m.DELTA_MONO != np.sqrt(5.991) and m.DELTA_INERTIAL == np.sqrt(16.92)
    f = np.float32
    # the fail predicate is taken on floats: err rounds up, err_end to the same float, and 2 * err < err_end no longer holds
    err, err_end = 1.0 + 0.6 * 2.0 ** -23, 2.0 + 0.7 * 2.0 ** -22
    assert 2 * err < err_end and not bool(f(2) * f(err) < f(err_end))


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic on the host
@pytest.mark.parametrize("name", ("n2", "no_imu_middle", "n10"))
def test_host_linearize_against_the_model(name):
    """inertial_ba_host_linearize runs the device functions compiled for the host.  Both sides are double; they differ in the order of
    sums of at most nine products, i.e. by a few units in the last place of the largest term: 1e-12 of the largest entry of each block
    (errors: of the observation they are the remainder of) is two orders above that."""
    lib = capi.load()
    P = m.build_case(name)
    S = m.Structure(P)
    p, keep = m.to_c_problem(P)
    vis = np.zeros((max(S.NE, 1), 31))
    ine = np.zeros((max(len(S.inertial), 1), 15, 32))
    capi.check(lib.inertial_ba_host_linearize(C.byref(p), vis.ctypes.data, ine.ctypes.data), "inertial_ba_host_linearize")
    kfs, X = m.initial_state(P)
    err, Xc, c2, Rcw = m.visual_edges(P, S, kfs, X)
    Jl, Jp = m.visual_jacobians(P, S, Xc, Rcw)
    vis = vis[:S.NE]
    tol = 1e-12
    assert np.abs(vis[:, 0:3] - err).max() <= tol * np.abs(S.obs).max()
    c2_host = (vis[:, 0] * (S.om * vis[:, 0]) + vis[:, 1] * (S.om * vis[:, 1])) + vis[:, 2] * (S.om * vis[:, 2])
    assert np.array_equal(vis[:, 3], c2_host)                                          # chi2 = e^T (omega e) of the host's own error, term by term
    assert np.abs(vis[:, 4:13].reshape(-1, 3, 3) - Jl).max() <= tol * np.abs(Jl).max()
    assert np.abs(vis[:, 13:31].reshape(-1, 3, 6) - Jp).max() <= tol * np.abs(Jp).max()
    for q, ie in enumerate(m.inertial_edges(P, S, kfs)):
        assert np.abs(ine[q, :, :30] - ie[3]).max() <= tol * np.abs(ie[3]).max()
        assert np.abs(ine[q, :, 30] - ie[4]).max() <= tol * max(np.abs(ie[4]).max(), 1.0)
        assert not ine[q, :, 31].any()
