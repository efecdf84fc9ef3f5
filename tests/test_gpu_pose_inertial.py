"""pose_inertial_optimize (csrc/pose_inertial.hip) against the numpy model of tests/pose_inertial_model.py.

Against model (b), kernel arithmetic: every decision (outlier flags, n_inliers, n_bad, rounds_run, solve_failed) outside the
near-threshold band is equal, and at most 0.1 % of the decisions lie in the band; state and H lie within MARGIN x the case's own
forward-vs-reversed yardstick (H relative to its Frobenius norm).  Against model (a), reference arithmetic: within the (a)-vs-(b)
difference plus that tolerance.  Each case prints its ratios; DESIGN section 5 records the worst."""
import ctypes as C
import threading

import numpy as np
import pytest

import pose_inertial_model as pm
from multi_orbslam3_amd import _capi as capi, views

pytestmark = pytest.mark.gpu


def _call(P, device=0):
    p, keep = pm.to_c_problem(P, device)
    out = views.PoseInertialOutput(p.n)
    capi.check(capi.load().pose_inertial_optimize(C.byref(p), C.byref(out.c)), "pose_inertial_optimize")
    return out.as_dict()


def _compare(name, got, rb, rr, ra):
    """the assertions of the module docstring for one call"""
    y = pm.yardsticks_of(rb, rr, ra)
    near = pm.near_threshold(rb["decisions"])
    share = float(near.mean()) if len(near) else 0.0
    d = np.array(rb["decisions"]) if rb["decisions"] else np.zeros((0, 4))
    n = len(rb["outlier"])
    touched = np.zeros(n, bool)
    if len(d):
        touched[d[near, 1].astype(int)] = True
    ds, dh = pm.state_difference(got, rb), pm.hessian_difference(got, rb)
    das, dah = pm.state_difference(got, ra), pm.hessian_difference(got, ra)
    print("%s: near-threshold %d of %d; state %.3g (yardstick %.3g, ratio %.2f); H %.3g (yardstick %.3g, ratio %.2f); vs (a): state %.3g "
          "(a-b %.3g), H %.3g (a-b %.3g)" % (name, near.sum(), len(near), ds, y["fr_state"], ds / y["fr_state"], dh, y["fr_H"], dh / y["fr_H"],
                                            das, y["ab_state"], dah, y["ab_H"]))
    assert share <= pm.BAND_CAP, (name, share)
    assert np.array_equal(got["outlier"][~touched], rb["outlier"][~touched]), name
    if not touched.any():
        assert (got["n_inliers"], got["n_bad"]) == (rb["n_inliers"], rb["n_bad"]), name
    assert got["rounds_run"] == rb["rounds_run"] and got["solve_failed"] == rb["solve_failed"], name
    assert ds <= pm.MARGIN * y["fr_state"], (name, ds, y["fr_state"])
    assert dh <= pm.MARGIN * y["fr_H"], (name, dh, y["fr_H"])
    assert das <= y["ab_state"] + pm.MARGIN * y["fr_state"], (name, das)
    assert dah <= y["ab_H"] + pm.MARGIN * y["fr_H"], (name, dah)
    k = rb["rounds_run"] - 1
    assert np.allclose(got["chi2"][: k + 1], rb["chi2"][: k + 1], rtol=1e-6, atol=1e-9), (name, got["chi2"], rb["chi2"])


@pytest.mark.parametrize("case", pm.CASES, ids=[c[0] for c in pm.CASES])
def test_case(case):
    P, rb, rr, ra = pm.case_results(case)
    _compare(case[0], _call(P), rb, rr, ra)


@pytest.mark.parametrize("case", pm.CAP_CASES, ids=[c[0] for c in pm.CAP_CASES])
def test_cap(case):
    """n = 4096: sixteen correspondences per thread, the largest staging block"""
    P, rb, rr, ra = pm.case_results(case)
    _compare(case[0], _call(P), rb, rr, ra)


def test_recovery_is_exercised():
    """the two recovery cases differ only in rec_init: recovery runs in one and changes the count"""
    by = {c[0]: c for c in pm.CASES}
    for f in ("kf", "fr"):
        a, b = _call(pm.case_results(by[f + "_recover"])[0]), _call(pm.case_results(by[f + "_recinit"])[0])
        assert pm.case_results(by[f + "_recinit"])[1]["n_inliers"] < 30
        assert a["n_bad"] <= b["n_bad"]


def test_prior_huber_is_active():
    by = {c[0]: c for c in pm.CASES}
    P = pm.case_results(by["fr_prior_huber"])[0]
    oth = pm.make_state(**{k: np.asarray(x, np.float64) for k, x in P["other"].items()})
    pr = P["prior"]
    e = pm.prior_error(oth, {"R": pr["Rwb"], "t": pr["twb"], "v": pr["vwb"], "bg": pr["bg"], "ba": pr["ba"]})
    assert pm.huber(float(e @ pr["H"] @ e), 5.0)[1] < 1.0


def test_chain():
    """five consecutive LastFrame calls, each fed the previous H through orbg_condition_prior, against the model's chain"""
    lib = capi.load()
    got = own = None
    for step in range(pm.CHAIN_LEN):
        # the device's chain: its own previous H, conditioned by the library
        Pg = pm.chain_problems(step, None)
        if got is not None:
            Hc = np.ascontiguousarray(got["H"].reshape(225)).copy()
            capi.check(lib.orbg_condition_prior(Hc.ctypes.data), "orbg_condition_prior")
            assert np.abs(Hc.reshape(15, 15) - pm.condition_prior(got["H"])).max() <= 1e-12 * np.abs(got["H"]).max()
            Pg["prior"]["H"] = Hc.reshape(15, 15)
        # the model's step on the SAME input carries the tolerances of the module docstring (a step's yardstick says nothing about a
        # difference in its inputs); the model's own chain, fed its own H, must take the same decisions
        rb, rr, ra = pm.solve(Pg, "kernel"), pm.reversed_runs(Pg), pm.solve(Pg, "reference")
        got = _call(Pg)
        _compare("chain_%d" % step, got, rb, rr, ra)
        own = pm.solve(pm.chain_problems(step, own), "kernel")
        assert np.array_equal(own["outlier"], got["outlier"]) and own["rounds_run"] == got["rounds_run"], step
        print("chain_%d: the model's own chain differs by %.3g in state, %.3g in H" % (step, pm.state_difference(got, own),
                                                                                      pm.hessian_difference(got, own)))


def test_set_stream_and_threads():
    """pose_inertial_set_stream, and two threads calling concurrently (each with its own work area): the same bits as a lone call"""
    import torch
    lib = capi.load()
    by = {c[0]: c for c in pm.CASES}
    Ps = [pm.case_results(by["kf_n257"])[0], pm.case_results(by["fr_n255"])[0]]
    want = [_call(P) for P in Ps]
    st = torch.cuda.Stream()
    capi.check(lib.pose_inertial_set_stream(0, C.c_void_p(st.cuda_stream)), "pose_inertial_set_stream")
    try:
        on_stream = [_call(P) for P in Ps]
    finally:
        capi.check(lib.pose_inertial_set_stream(0, None), "pose_inertial_set_stream")
    res = [None, None]

    def work(k):
        res[k] = [_call(Ps[k]) for _ in range(3)]
    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        for r in [on_stream[k]] + res[k]:
            for key in ("Rwb", "twb", "vwb", "bg", "ba", "outlier", "H", "chi2"):
                assert np.array_equal(np.asarray(r[key]), np.asarray(want[k][key])), (k, key)
            assert (r["n_inliers"], r["n_bad"], r["rounds_run"], r["solve_failed"]) == (want[k]["n_inliers"], want[k]["n_bad"],
                                                                                       want[k]["rounds_run"], want[k]["solve_failed"])
