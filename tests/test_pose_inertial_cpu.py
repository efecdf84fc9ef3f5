"""pose_inertial_optimize without a device: the numpy model itself (Jacobians, recovery, the stale-chi2 rule, Marginalize), the yardsticks
and conditions the GPU test relies on, the kernel's edge arithmetic compiled for the host, the host helpers and the argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_inertial_model as pm
from multi_orbslam3_amd import _capi as capi, views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = pm.CASES + pm.CAP_CASES


def _states(P):
    cur = pm.make_state(**{k: np.asarray(x, np.float64) for k, x in P["frame"].items()})
    oth = pm.make_state(**{k: np.asarray(x, np.float64) for k, x in P["other"].items()})
    return cur, oth


def _prior(P):
    pr = P["prior"]
    return {"R": pr["Rwb"], "t": pr["twb"], "v": pr["vwb"], "bg": pr["bg"], "ba": pr["ba"]}


def _numeric(f, n_in, h):
    """central differences of f(dx) at dx = 0"""
    cols = []
    for k in range(n_in):
        d = np.zeros(n_in)
        d[k] = h
        cols.append((f(d) - f(-d)) / (2 * h))
    return np.stack(cols, axis=1)


def test_jacobians_against_central_differences():
    """The analytic Jacobians of the four non-visual edge kinds and both visual kinds against central differences through the vertices' own
    oplus.  With step h the truncation error is ~ h^2 |f'''| / 6 and the rounding error ~ eps |f| / h: at h = 1e-6 and residuals of order
    1 .. 500 (pixels) both stay below 1e-6 relative to the largest Jacobian entry of the edge, which is the tolerance."""
    h, tol = 1e-6, 1e-6
    worst = {}
    for seed, bias_step in ((3, 0.0), (4, 2e-3)):
        P = pm.make_scene(pm.FORM_FRAME, 40, seed, bias_step=bias_step, prior_shift=1.0)
        cur, oth = _states(P)
        pre = P["preint"]
        # inertial: 9 x 24 over [other 15 | pose and velocity of the frame 9]
        def f_in(d):
            c = pm.oplus(cur, np.concatenate([d[15:24], np.zeros(6)]))
            return pm.inertial_error(pm.oplus(oth, d[0:15]), c, pre)
        Ja = pm.inertial_jacobian(oth, cur, pre)
        worst["inertial"] = max(worst.get("inertial", 0), np.abs(Ja - _numeric(f_in, 24, h)).max() / np.abs(Ja).max())
        # prior: 15 x 15
        pr = _prior(P)
        Jp = pm.prior_jacobian(oth, pr)
        worst["prior"] = max(worst.get("prior", 0), np.abs(Jp - _numeric(lambda d: pm.prior_error(pm.oplus(oth, d), pr), 15, h)).max() / np.abs(Jp).max())
        # random walks: error = b2 - b1
        for key, lo in (("bg", 9), ("ba", 12)):
            def f_rw(d, key=key, lo=lo):
                a, b = np.zeros(15), np.zeros(15)
                a[lo:lo + 3], b[lo:lo + 3] = d[0:3], d[3:6]
                return pm.oplus(cur, b)[key] - pm.oplus(oth, a)[key]
            Jn = _numeric(f_rw, 6, h)
            worst["walk_" + key] = max(worst.get("walk_" + key, 0), np.abs(Jn - np.hstack([-np.eye(3), np.eye(3)])).max())
        # visual: mono and stereo
        Tcb = P["Tcb"].astype(np.float64)
        cam = tuple(float(c) for c in P["cam"])
        Xw, u, v, ur = [P[k].astype(np.float64) for k in ("Xw", "u", "v", "ur")]
        Rcw, tcw = pm.camera_pose(cur, Tcb)
        _, Xc = pm.visual_error(Rcw, tcw, cam, Xw, u, v, ur)
        Jv = pm.visual_jacobian(Xc, cam, Tcb, ur < 0)
        def f_vis(d):
            R2, t2 = pm.camera_pose(pm.oplus(cur, np.concatenate([d, np.zeros(9)])), Tcb)
            return pm.visual_error(R2, t2, cam, Xw, u, v, ur)[0].ravel()
        Jn = _numeric(f_vis, 6, h).reshape(len(u), 3, 6)
        for name, sel in (("mono", ur < 0), ("stereo", ur >= 0)):
            assert sel.any()
            worst[name] = max(worst.get(name, 0), (np.abs(Jv[sel] - Jn[sel]).max(axis=(1, 2)) / np.abs(Jv[sel]).max(axis=(1, 2))).max())
    print("worst relative Jacobian error per edge kind:", {k: "%.2e" % x for k, x in worst.items()})
    assert set(worst) == {"inertial", "prior", "walk_bg", "walk_ba", "mono", "stereo"}
    for k, x in worst.items():
        assert x < tol, (k, x)


@pytest.mark.parametrize("form", [pm.FORM_KF, pm.FORM_FRAME])
def test_noise_free_scene_is_recovered(form):
    """Exact observations, the other end exact, the frame's start perturbed by three times the usual amount: the solve comes back to the
    truth as far as the float inputs carry it (1e-7 relative in points, poses and preintegration -> 1e-5 is generous and far below the start)."""
    P = pm.make_scene(form, 200, 5, noise_px=0.0, perturb_other=0.0, perturb=3.0)
    r = pm.solve(P)
    tr = P["truth"]["cur"]
    start = np.abs(P["frame"]["twb"] - tr["t"]).max()
    assert start > 1e-2
    assert np.abs(r["Rwb"] - tr["R"]).max() < 1e-5 and np.abs(r["twb"] - tr["t"]).max() < 1e-5 and np.abs(r["vwb"] - tr["v"]).max() < 1e-4
    assert r["n_bad"] == 0 and r["rounds_run"] == 4 and not r["solve_failed"]


STALE_SEEDS = (1000, 1115, 1229)     # found by a search over seeds 1000..1399 of the scene below for the property the test asserts


def test_stale_chi2_rule_is_exercised():
    """Constructed cases where an edge's stale and fresh chi2 fall on different sides of the threshold of round 0: a LastFrame problem with
    few, noisy points, where the Huber-weighted Gauss-Newton is still moving at its tenth iteration.  The edge's flag after the round flips
    when the model is switched to fresh errors, so the rule of the reference (no computeError after the last update) is exercised."""
    for seed in STALE_SEEDS:
        P = pm.make_scene(pm.FORM_FRAME, 12, seed, kind="mono", outlier_frac=0.0, perturb=6.0, noise_px=6.0, close_frac=0.0)
        da, db = np.array(pm.solve(P)["decisions"]), np.array(pm.solve(P, fresh_chi2=True)["decisions"])
        da, db = da[da[:, 0] == 0], db[db[:, 0] == 0]
        lo, hi = np.minimum(da[:, 2], da[:, 4]), np.maximum(da[:, 2], da[:, 4])
        k = np.flatnonzero((lo < da[:, 3]) & (da[:, 3] < hi) & (hi - lo > 1e-3 * da[:, 3]))
        assert len(k), seed
        for i in k:
            print("seed %d edge %d, round 0: stale chi2 %.6f, fresh %.6f, threshold %.6f" % (seed, da[i, 1], da[i, 2], da[i, 4], da[i, 3]))
            assert db[i, 2] == da[i, 4]                        # the fresh-error model classifies with the error at the final estimate
            assert (np.float32(da[i, 2]) > np.float32(da[i, 3])) != (np.float32(db[i, 2]) > np.float32(db[i, 3]))


def test_marginalize_against_schur_complement():
    rng = np.random.default_rng(7)
    A = rng.normal(size=(30, 40))
    H = A @ A.T
    for rank_deficient in (False, True):
        Hx = H.copy()
        if rank_deficient:
            B = rng.normal(size=(15, 9))
            Hx[:15, :15] = B @ B.T                         # rank 9: six singular values at rounding level, far below the 1e-6 cut
        got, s = pm.marginalize(Hx, 0, 14)
        want = Hx[15:, 15:] - Hx[15:, :15] @ np.linalg.pinv(Hx[:15, :15], rcond=1e-6 / s.max(), hermitian=True) @ Hx[:15, 15:]
        assert (s < 1e-6).sum() == (6 if rank_deficient else 0)
        assert np.abs(got[15:, 15:] - want).max() <= 1e-9 * np.abs(want).max()
        assert np.all(got[:15] == 0) and np.all(got[:, :15] == 0)


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_yardsticks_and_conditions(case):
    """The two yardsticks the GPU test imports, printed; and the GPU test's conditions on the model alone."""
    P, rb, rr, ra = pm.case_results(case)
    y = pm.yardsticks(case)
    print(case[0], {k: "%.3g" % x for k, x in y.items()})
    near = pm.near_threshold(rb["decisions"])
    assert (near.mean() if len(near) else 0.0) <= pm.BAND_CAP
    # no singular value of a marginalised block within a factor 10 of the cut
    sv = rb["marg_sv"]
    assert not np.any((sv > 1e-7) & (sv < 1e-5)), sv
    # (a) and (b) agree on every decision outside the band (and so do the reversed runs)
    d = np.array(rb["decisions"]) if rb["decisions"] else np.zeros((0, 4))
    touched = np.zeros(len(rb["outlier"]), bool)
    if len(d):
        touched[d[near, 1].astype(int)] = True
    for r in [ra] + rr:
        assert np.array_equal(r["outlier"][~touched], rb["outlier"][~touched])
        assert r["rounds_run"] == rb["rounds_run"] and r["solve_failed"] == rb["solve_failed"]
    # what the case is there for
    name = case[0]
    if name.endswith("_n6"):
        assert rb["rounds_run"] == (1 if case[1] == pm.FORM_KF else 4)
    if name.endswith("_n7"):
        assert rb["rounds_run"] == 4
    if name.endswith("_recover") or name.endswith("_recinit"):
        assert rb["n_inliers"] < 30 or name.endswith("_recover")
    if name.endswith("_behind"):
        assert rb["outlier"][:3].all()
    if name == "fr_prior_zero":
        assert rb["solve_failed"] == 1
    if name.endswith("_bias_step"):
        assert np.linalg.norm(P["preint"]["JRg"].astype(np.float64) @ (P["other"]["bg"].astype(np.float64) - P["preint"]["bg"])) > 1e-5
    elif case[1] == pm.FORM_KF and "prior" not in name:
        assert np.array_equal(P["other"]["bg"], P["preint"]["bg"])


def test_kernel_edge_arithmetic_on_the_host():
    """pose_inertial_host_linearize: the kernel's own edge functions, compiled for the host, against the model at the estimates handed in.
    Same formulas in another operation order: 1e-12 relative to the largest entry leaves three orders of magnitude above rounding."""
    lib = capi.load()
    for form in (pm.FORM_KF, pm.FORM_FRAME):
        for bias_step in (0.0, 2e-3):
            P = pm.make_scene(form, 50, 7, bias_step=bias_step, prior_shift=1.0)
            p, keep = pm.to_c_problem(P)
            J, vis = np.zeros((30, 32)), np.zeros((50, 31))
            assert lib.pose_inertial_host_linearize(C.byref(p), J.ctypes.data, vis.ctypes.data) == capi.ORBG_OK
            cur, oth = _states(P)
            NU = 30 if form == pm.FORM_FRAME else 15
            co = NU - 15
            Ji = pm.inertial_jacobian(oth, cur, P["preint"])
            Jm = np.zeros((15, NU))
            if form == pm.FORM_FRAME:
                Jm[:9, 0:15] = Ji[:, 0:15]
                Jm[9:12, 9:12] = Jm[12:15, 12:15] = -np.eye(3)
            Jm[:9, co:co + 9] = Ji[:, 15:24]
            Jm[9:12, co + 9:co + 12] = Jm[12:15, co + 12:co + 15] = np.eye(3)
            em = np.concatenate([pm.inertial_error(oth, cur, P["preint"]), cur["bg"] - oth["bg"], cur["ba"] - oth["ba"]])
            assert np.abs(J[:15, :NU] - Jm).max() <= 1e-12 * np.abs(Jm).max()
            assert np.abs(J[:15, NU] - em).max() <= 1e-12 * max(np.abs(em).max(), 1.0)
            if form == pm.FORM_FRAME:
                assert np.abs(J[15:30, :15] - pm.prior_jacobian(oth, _prior(P))).max() <= 1e-12
                assert np.abs(J[15:30, NU] - pm.prior_error(oth, _prior(P))).max() <= 1e-12
                assert np.all(J[15:30, 15:30] == 0)
            Tcb, cam = P["Tcb"].astype(np.float64), tuple(float(c) for c in P["cam"])
            Xw, u, v, ur = [P[k].astype(np.float64) for k in ("Xw", "u", "v", "ur")]
            om = P["inv_sigma2"].astype(np.float64)
            Rcw, tcw = pm.camera_pose(cur, Tcb)
            err, Xc = pm.visual_error(Rcw, tcw, cam, Xw, u, v, ur)
            Jv = pm.visual_jacobian(Xc, cam, Tcb, ur < 0)
            Hv = np.einsum("nka,nkc->nac", Jv, om[:, None, None] * Jv)
            bv = -np.einsum("nka,nk->na", Jv, om[:, None] * err)
            iu = np.triu_indices(6)
            assert np.abs(vis[:, :3] - err).max() <= 1e-12 * np.abs(err).max()
            assert np.abs(vis[:, 3] - om * (err * err).sum(axis=1)).max() <= 1e-12 * (om * (err * err).sum(axis=1)).max()
            assert np.abs(vis[:, 4:25] - Hv[:, iu[0], iu[1]]).max() <= 1e-12 * np.abs(Hv).max()
            assert np.abs(vis[:, 25:31] - bv).max() <= 1e-12 * np.abs(bv).max()


def test_host_helpers_against_numpy():
    lib = capi.load()
    for seed in (3, 4):
        Cm = pm.make_scene(pm.FORM_KF, 5, seed)["C"]
        i9, ig, ia = np.zeros(81), np.zeros(9), np.zeros(9)
        assert lib.orbg_imu_information(np.ascontiguousarray(Cm).ctypes.data, i9.ctypes.data, ig.ctypes.data, ia.ctypes.data) == capi.ORBG_OK
        a, b, c = pm.imu_information(Cm)
        # the inverse goes through float: one float ulp where a double lands next to a rounding boundary, else the eigen solvers' rounding
        assert np.abs(i9.reshape(9, 9) - a).max() <= 2.0 ** -23 * np.abs(a).max()
        assert np.abs(ig.reshape(3, 3) - b).max() <= 2.0 ** -23 * np.abs(b).max() and np.abs(ia.reshape(3, 3) - c).max() <= 2.0 ** -23 * np.abs(c).max()
        assert np.array_equal(i9.reshape(9, 9), i9.reshape(9, 9).T) or np.abs(i9.reshape(9, 9) - i9.reshape(9, 9).T).max() <= 1e-12 * np.abs(a).max()
    rng = np.random.default_rng(0)
    H = rng.normal(size=(15, 15))
    H = H @ H.T
    H[:, :3] *= 1e-8
    H[:3, :] *= 1e-8                                    # three eigenvalues below the clamp
    H[0, 1] += 1.0                                      # the upper triangle is not read (Eigen's SelfAdjointEigenSolver, numpy's eigh)
    Hc = np.ascontiguousarray(H.reshape(225)).copy()
    assert lib.orbg_condition_prior(Hc.ctypes.data) == capi.ORBG_OK
    want = pm.condition_prior(H)
    assert (np.linalg.eigvalsh(want) < 1e-13).sum() >= 3
    assert np.abs(Hc.reshape(15, 15) - want).max() <= 1e-12 * np.abs(want).max()
    assert lib.orbg_condition_prior(None) == capi.ORBG_BAD_ARG
    assert lib.orbg_imu_information(None, None, None, None) == capi.ORBG_BAD_ARG


def test_argument_checks_and_no_device():
    lib = capi.load()
    P = pm.make_scene(pm.FORM_FRAME, 20, 9)
    p, keep = pm.to_c_problem(P)
    out = views.PoseInertialOutput(p.n)
    call = lambda: lib.pose_inertial_optimize(C.byref(p), C.byref(out.c))
    if lib.orbg_device_count() <= 0:
        assert call() == capi.ORBG_NO_DEVICE
        assert lib.pose_inertial_set_stream(0, None) == capi.ORBG_NO_DEVICE
    assert lib.pose_inertial_optimize(None, C.byref(out.c)) == capi.ORBG_BAD_ARG
    assert lib.pose_inertial_optimize(C.byref(p), None) == capi.ORBG_BAD_ARG
    for field, bad in (("form", 2), ("n_left", 100), ("n", -1), ("struct_size", 8), ("u", None), ("close", None)):
        old = getattr(p, field)
        setattr(p, field, bad)
        assert call() == capi.ORBG_BAD_ARG, field
        setattr(p, field, old)
    prior, p.prior = p.prior, None                      # the LastFrame form without pFp->mpcpi
    assert call() == capi.ORBG_BAD_ARG
    p.prior = prior
    out.c.outlier, keep_o = None, out.c.outlier
    assert call() == capi.ORBG_BAD_ARG
    out.c.outlier = keep_o
    out.c.struct_size = 4
    assert call() == capi.ORBG_BAD_ARG
    out.c.struct_size = C.sizeof(capi.PoseInertialResult)
    # the cap, before any device call
    P2 = pm.make_scene(pm.FORM_KF, 4097, 9)
    p2, keep2 = pm.to_c_problem(P2)
    out2 = views.PoseInertialOutput(p2.n)
    assert lib.pose_inertial_optimize(C.byref(p2), C.byref(out2.c)) == capi.ORBG_CAP_EXCEEDED


def test_ctypes_mirrors_match_the_header(tmp_path):
    """sizes and the offsets of every field of the five structs, from a C program compiled against include/orbgpu.h"""
    pairs = {"pose_inertial_state": capi.PoseInertialState, "pose_inertial_preint": capi.PoseInertialPreint,
             "pose_inertial_prior": capi.PoseInertialPrior, "pose_inertial_problem": capi.PoseInertialProblem,
             "pose_inertial_result": capi.PoseInertialResult}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "orbgpu.h"', "int main(void) {"]
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
    hdr = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    for sym in ("pose_inertial_optimize", "pose_inertial_set_stream", "orbg_imu_information", "orbg_condition_prior"):
        assert sym in capi.EXPORTED_SYMBOLS and ("int %s(" % sym) in hdr
