"""MLPnPsolver, the parts that need no GPU: the checker (tests/mlpnp_model.py) against itself -- formulation (a) against (b), the figures
the GPU test leans on --, the host side of the library (SetRansacParameters' formula, the closed form of the minimal-set draws, the
argument checks, which come before the device is looked for), the serial loop on hand-made counts, and the loud failure without a
device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mlpnp_model as mm
from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELOC = (0.99, 10, 300, 6, 0.5, 5.991)


def _problem(sc):
    return api.MLPnPProblem(sc["P2D"], sc["sigma2"], sc["bearing"], sc["P3Dw"], sc["K"], sc["kp_index"], sc["m"])


# ------------------------------------------------------------------ 1. the model against itself

def test_formulation_a_against_b_per_gap_band(capsys):
    """The yardstick of tests/test_gpu_mlpnp.py: the largest pose difference between the two formulations per eigen-gap band
    ((lambda_2 - lambda_1) / lambda_max of A^T A) over the hypotheses of mlpnp_model.CASES and of the planar scene, and the caps the GPU
    test puts on what it leaves out, held here for the model alone: decisions within a relative 1e-4 of their threshold at most 0.1 %,
    hypotheses with a gap below 1e-8 at most 2 %.  Masks of (a) and (b) are equal outside those decisions."""
    ms = mm.measure()
    with capsys.disabled():
        print("\nmlpnp model (a) vs (b): %d hypotheses, %d NaN, %d with gap < 1e-8; %d decisions, %d near a threshold" %
              (ms["total"], ms["nan"], ms["low_gap"], ms["decisions"], ms["near"]))
        for b, (lo, hi) in enumerate(mm.GAP_BANDS):
            if b in ms["bands"]:
                print("  gap in [%g, %g): max |pose(a) - pose(b)| = %.3g, max cond(J^T J) = %.3g, yardstick %.3g" %
                      (lo, hi, ms["bands"][b], ms["conds"][b], mm.yardstick(b)))
    assert ms["total"] == sum(c[2] for c in mm.CASES) + 35
    assert ms["near"] <= 1e-3 * ms["decisions"] and ms["low_gap"] <= 0.02 * ms["total"]
    for i in range(len(ms["a"])):
        sc, _ = mm.case_scene(i)
        me = mm.max_errors(sc["sigma2"], 5.991)
        for x, y in zip(ms["a"][i], ms["b"][i]):
            assert x["planar"] == y["planar"]
            if mm.band_of(y["gap"]) >= 0 and np.isfinite(y["R"]).all():
                assert not ((x["mask"] != y["mask"]) & ~mm.near_threshold(y["e2"], me)).any()
    # every band's difference is far below what a wrong branch would give (poses are O(1))
    assert max(ms["bands"].values()) < 1e-4


def test_model_recovers_the_pose_of_exact_correspondences():
    for planar in (False, True):
        sc = mm.make_scene(77, 30, 0.0, planar=planar)
        Xc = sc["P3Dw"].astype(np.float64) @ sc["R"].T + sc["t"]
        f = Xc / Xc[:, 2:3]
        for form in "ab":
            ok = 0
            for k in range(5):
                h = mm.compute_pose(sc["P3Dw"][6 * k: 6 * k + 6], f[6 * k: 6 * k + 6], form)
                assert h["planar"] == planar
                ok += int(np.abs(h["R"] - sc["R"]).max() < 1e-6 and np.abs(h["t"] - sc["t"]).max() < 1e-5)
            assert ok >= 4, (planar, form, ok)


def test_derived_jacobian_is_the_derivative():
    rng = np.random.default_rng(3)
    for _ in range(20):
        w, t, X = rng.normal(size=3) * 0.7, rng.normal(size=3), rng.normal(size=3) + np.array([0, 0, 4.0])
        nr, ns = mm.nullspace_cross(rng.normal(size=3))
        J = mm.jacobian(w, t, X, nr, ns)

        def res(x):
            v = mm.rodrigues2rot(x[:3]) @ X + x[3:]
            v = v / np.linalg.norm(v)
            return np.array([nr @ v, ns @ v])
        x0 = np.concatenate([w, t])
        num = np.stack([(res(x0 + 1e-6 * e) - res(x0 - 1e-6 * e)) / 2e-6 for e in np.eye(6)], 1)
        assert np.abs(J - num).max() < 1e-8
    assert np.isnan(mm.jacobian(np.zeros(3), t, X, nr, ns)[:, :3]).all()


def test_identity_rotation_gives_a_nan_pose_in_the_model():
    sc = mm.make_scene(1200, 6, 0.0)
    R, t = mm.refine_stage(np.eye(3), sc["t"], sc["P3Dw"], sc["bearing"])
    assert np.isnan(t).all() and np.array_equal(R, np.eye(3))       # rodrigues2rot of a NaN vector: :663 compares false
    assert not mm.check_inliers(R, t, sc["P3Dw"], sc["P2D"], mm.max_errors(sc["sigma2"], 5.991))[0].any()


def test_planar_test_is_eigens_rank():
    rng = np.random.default_rng(5)
    P = rng.normal(size=(6, 3))
    assert mm.fullpiv_rank3(P.T @ P) == 3
    P[:, 2] = 0.0
    assert mm.fullpiv_rank3(P.T @ P) == 2
    Q = P @ mm.rodrigues2rot(np.array([0.3, 0.2, -0.4])).T          # a plane through the origin, rounding-level third pivot
    assert mm.fullpiv_rank3(Q.T @ Q) == 2
    Q = Q + np.array([0.0, 0.0, 1.0])                                # off the origin: not "planar"
    assert mm.fullpiv_rank3(Q.T @ Q) == 3
    P[:, 1] = 0.0
    assert mm.fullpiv_rank3(P.T @ P) == 1


# ------------------------------------------------------------------ 2. the serial loop

def _hand(counts, n=12):
    masks = [np.arange(n) < c for c in counts]
    poses = [(mm.rodrigues2rot(np.array([0.1 * (k + 1), 0.0, 0.0])), np.array([k, 0.0, 1.0])) for k in range(len(counts))]
    return masks, poses


def test_serial_loop_exactly_min_inliers_becomes_best_and_does_not_return():
    n, counts = 12, [3, 8, 8, 5, 0]
    masks, poses = _hand(counts)
    s = mm.SerialSolver(n, n, np.arange(n), 8, 5)
    assert s.iterations_of_call(2) == 5                        # the OR: the first call runs all of mRansacMaxIts
    o = s.iterate(2, counts, masks, poses)
    assert (o["iterations_run"], o["iterations_done"], o["no_more"], o["returned"]) == (5, 5, True, True)
    assert (o["n_inliers"], o["best_iteration"], o["best_inliers"]) == (8, 1, 8)            # the FIRST 8 (> on the update)
    assert o["Tcw"].tobytes() == mm.pose_to_Tcw(*poses[1]).tobytes() and o["inliers"].sum() == 8


def test_serial_loop_second_call_returns_a_worse_hypothesis_than_the_best():
    n, counts = 12, [11, 9, 12]
    masks, poses = _hand(counts)
    s = mm.SerialSolver(n, n, np.arange(n), 8, 3)
    o = s.iterate(1, counts, masks, poses)
    assert (o["returned"], o["no_more"], o["iterations_run"], o["n_inliers"], o["best_inliers"]) == (True, False, 1, 11, 11)
    assert s.iterations_of_call(1) == 2
    o = s.iterate(1, counts[1:], masks[1:], poses[1:])
    # 9 > min_inliers returns at once, with ITS pose and inliers; the best stays the 11 of the first call
    assert (o["returned"], o["n_inliers"], o["best_inliers"], o["best_iteration"], o["iterations_done"]) == (True, 9, 11, 0, 2)
    assert o["Tcw"].tobytes() == mm.pose_to_Tcw(*poses[1]).tobytes() and o["best_Tcw"].tobytes() == mm.pose_to_Tcw(*poses[0]).tobytes()
    assert o["inliers"].sum() == 9


def test_serial_loop_never_reaching_min_inliers_and_too_few_points():
    n, counts = 12, [3, 7, 0, 7]
    masks, poses = _hand(counts)
    s = mm.SerialSolver(n, n, np.arange(n), 8, 4)
    o = s.iterate(5, counts + [2], masks + masks[:1], poses + poses[:1])      # nIterations = 5 > mRansacMaxIts: five run
    assert (o["iterations_run"], o["no_more"], o["returned"], o["have_best"], o["Tcw"]) == (5, True, False, False, None)
    s = mm.SerialSolver(7, 7, np.arange(7), 8, 4)
    assert s.iterations_of_call(5) == 0
    o = s.iterate(5, [], [], [])
    assert (o["no_more"], o["returned"], o["iterations_done"]) == (True, False, 0)


# ------------------------------------------------------------------ 3. the host side of the library

def test_ransac_iterations_of_the_library_equal_the_models():
    for n in list(range(1, 300)) + [513, 1000, 2000, 100000]:
        for par in (api.MLPNP_DEFAULTS, RELOC, (0.999, 6, 1000, 6, 0.05, 5.991)):
            its, mi, _ = mm.ransac_iterations(n, *par[:5])
            assert api.mlpnp_ransac_iterations(n, *par) == (its, mi), (n, par)
    # int(N * epsilon) truncates, min_inliers is raised to it and to min_set, pow(epsilon, 3)
    assert api.mlpnp_ransac_iterations(19, *RELOC) == (30, 10) and api.mlpnp_ransac_iterations(21, *RELOC) == (35, 10)
    assert api.mlpnp_ransac_iterations(100, *RELOC) == (35, 50) and api.mlpnp_ransac_iterations(6, *RELOC)[1] == 10
    assert api.mlpnp_ransac_iterations(6, 0.99, 3, 300, 6, 0.4) == (1, 6)
    lib = capi.load()
    out = C.c_int(0)
    assert lib.orbp_mlpnp_ransac_iterations(20, 0.99, 8, 300, 5, 0.4, C.byref(out), None) == capi.ORBG_BAD_ARG       # min_set != 6
    assert lib.orbp_mlpnp_ransac_iterations(20, 0.99, 8, 300, 6, 0.4, None, None) == capi.ORBG_BAD_ARG


def test_draw_resolution_against_a_literal_list_replay():
    for n, seed in ((6, 0), (7, 1), (8, 2), (12, 3), (64, 4), (65, 5), (2000, 6)):
        d = api.mlpnp_draws(n, 400, seed)
        d[:4] = [[n - 1 - j for j in range(6)], [0] * 6, [n - 6] * 6, [n - 1, 0, n - 3, 0, n - 5, 0]]
        got = api.mlpnp_resolve_draws(n, d)
        assert np.array_equal(got, mm.resolve_draws(n, d)), n
        assert all(len(set(t)) == 6 for t in got.tolist())
    a = api.mlpnp_draws(50, 100, 7)
    assert np.array_equal(a, api.mlpnp_draws(50, 100, 7)) and a.dtype == np.int32 and a.shape == (100, 6)
    assert np.array_equal(a, mm.draws(50, 100, 7))
    lib = capi.load()
    bad = np.array([[0, 0, 0, 0, 0, 2]], np.int32); idx = np.zeros((1, 6), np.int32)
    assert lib.orbp_mlpnp_resolve_draws(7, C.c_void_p(bad.ctypes.data), 1, C.c_void_p(idx.ctypes.data)) == capi.ORBG_BAD_ARG
    assert lib.orbp_mlpnp_resolve_draws(5, C.c_void_p(bad.ctypes.data), 1, C.c_void_p(idx.ctypes.data)) == capi.ORBG_BAD_ARG


def _batch_args(sc, par=RELOC):
    prob = _problem(sc)
    its = mm.ransac_iterations(prob.n, *par[:5])[0]
    d = mm.draws(prob.n, its, 1)
    mask = np.full(prob.m, 0xA5, np.uint8)
    r = capi.MLPnPResult()
    r.struct_size = C.sizeof(capi.MLPnPResult)
    r.inliers = capi.ptr(mask)
    r.no_more, r.returned, r.n_inliers = -7, -7, -7
    P = (capi.MLPnPProblem * 1)(prob.struct())
    Q = (capi.MLPnPParams * 1)(capi.MLPnPParams(par[0], par[1], par[2], par[3], par[4], par[5]))
    D = (C.c_void_p * 1)(d.ctypes.data)
    return prob, d, mask, r, P, Q, D


def test_bad_arguments_are_refused_before_the_device_is_looked_for():
    lib = capi.load()
    sc = mm.make_scene(1, 40, 0.3)
    prob, d, mask, r, P, Q, D = _batch_args(sc)
    call = lambda: lib.orbp_mlpnp_solve_batch(0, P, 1, Q, D, C.byref(r))      # noqa: E731
    ok = (capi.ORBG_OK, capi.ORBG_NO_DEVICE)
    assert call() in ok
    P[0].struct_size = 8
    assert call() == capi.ORBG_BAD_ARG
    P[0].struct_size = C.sizeof(capi.MLPnPProblem)
    for field in ("P2D", "sigma2", "bearing", "P3Dw", "kp_index"):
        keep = getattr(P[0], field)
        setattr(P[0], field, None)
        assert call() == capi.ORBG_BAD_ARG, field
        setattr(P[0], field, keep)
    P[0].camera.model = 1                                                     # KannalaBrandt8: refused, not approximated
    assert call() == capi.ORBG_BAD_ARG
    P[0].camera.model = 0
    Q[0].min_set = 5
    assert call() == capi.ORBG_BAD_ARG
    Q[0].min_set = 6
    d[3, 2] = prob.n - 2                                                      # draw 2 picks from n - 2 entries
    assert call() == capi.ORBG_BAD_ARG
    d[3, 2] = 0
    r.struct_size = 8
    assert call() == capi.ORBG_BAD_ARG
    r.struct_size = C.sizeof(capi.MLPnPResult)
    kp = prob.kp_index.copy(); prob.kp_index[0] = prob.m
    assert call() == capi.ORBG_BAD_ARG
    prob.kp_index[:] = kp
    assert lib.orbp_mlpnp_solve_batch(0, None, 1, Q, D, C.byref(r)) == capi.ORBG_BAD_ARG
    assert lib.orbp_mlpnp_gn(0, None, None, None, None, None, None) == capi.ORBG_BAD_ARG
    assert lib.orbp_mlpnp_create(0, None) == capi.ORBG_BAD_ARG
    assert lib.orbp_mlpnp_iterate(None, 5, None, None) == capi.ORBG_BAD_ARG
    assert call() in ok


def test_no_gpu_means_no_solver():
    lib = capi.load()
    if lib.orbg_device_count() > 0:
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    assert lib.orbp_mlpnp_create(0, C.byref(h)) == capi.ORBG_NO_DEVICE
    sc = mm.make_scene(1, 40, 0.3)
    prob, d, mask, r, P, Q, D = _batch_args(sc)
    assert lib.orbp_mlpnp_solve_batch(0, P, 1, Q, D, C.byref(r)) == capi.ORBG_NO_DEVICE
    assert (mask == 0xA5).all() and (r.no_more, r.returned, r.n_inliers) == (-7, -7, -7)      # nothing written
    with pytest.raises(capi.OrbGpuError) as e:
        api.MLPnPsolver(prob)
    assert e.value.code == capi.ORBG_NO_DEVICE
    with pytest.raises(capi.OrbGpuError) as e:
        api.MLPnPsolver.solve_batch([prob])
    assert e.value.code == capi.ORBG_NO_DEVICE
    with pytest.raises(capi.OrbGpuError) as e:
        api.mlpnp_gn(sc["P3Dw"][:6], sc["bearing"][:6], np.eye(3), np.zeros(3))
    assert e.value.code == capi.ORBG_NO_DEVICE


def test_library_exports_every_declared_symbol():
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    declared = set(re.findall(r"^int\s+(orbp_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(capi.MLPNP_SYMBOLS), declared ^ set(capi.MLPNP_SYMBOLS)
    for s in declared:
        assert hasattr(lib, s), s


def test_ctypes_mirrors_have_the_headers_layout(tmp_path):
    src = tmp_path / "layout.c"
    fields = {"orbp_mlpnp_problem": ("MLPnPProblem", ["struct_size", "n", "P2D", "kp_index", "m", "camera"]),
              "orbp_mlpnp_params": ("MLPnPParams", ["probability", "min_inliers", "min_set", "epsilon", "th2"]),
              "orbp_mlpnp_result": ("MLPnPResult", ["struct_size", "no_more", "best_inliers", "Tcw", "best_Tcw", "inliers", "hyp_planar", "hyp_masks"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "orbgpu.h"', 'int main(void) {']
    for cname, (_, fl) in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in fl:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ["return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(ln.split() for ln in subprocess.check_output([exe], text=True).splitlines())
    for cname, (pyname, fl) in fields.items():
        cls = getattr(capi, pyname)
        assert int(got[cname]) == C.sizeof(cls), cname
        for f in fl:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, (cname, f)
