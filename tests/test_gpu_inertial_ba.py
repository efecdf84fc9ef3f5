"""inertial_ba_solve (csrc/inertial_ba.hip) on the device against tests/inertial_ba_model.py, variant "kernel" (double throughout), by the
per-frame optimiser's rules (tests/test_gpu_pose_inertial.py):
  - every verdict (edge_outlier, edge_depth_pos, failed, the trial counts, iters) is equal unless a decision of the case lies within a
    relative 1e-4 of its threshold (tests/test_inertial_ba_cpu.py holds the scenes to at most BAND_CAP of such decisions; the cases
    below have none in an LM decision, so trial counts and iters are compared outright);
  - states and points (the latter are floats in the result: what they differ by beyond their rounding to float) within MARGIN = 8
    times the model's own forward-against-reversed difference of the case, floored at one unit in the last place of the largest
    component;
  - lambda and chi2 of the trace within max(1e-9, 10 f), f the model's forward / reversed difference (the full BA's rule).  A row the
    model itself does not reproduce to 1e-3 (inertial_only's last: three edges on three keyframes reach chi2 = 0 to rounding) is
    rounding noise of the residuals: it is left out of f, so that it does not loosen the other rows, and is held absolutely instead
    -- the device's chi2 is, like the model's, below 1e-12 of the first evaluation's.  The chi2 of the single edges by the same rule
    with their own f;
  - against variant "reference" (the float round trips of the reference): that bound plus the model's (a)-against-(b) difference.

What each case reaches, and the LDL^T family LdltSolver::plan picks for its unknowns (ldltm::supports / ldltx::pays restated in
ldlt_family below; by default plan picks among three: the one-workgroup column kernel up to 8 tile rows, the eight-workgroup kernel for
9 .. 19 tile rows, the many-workgroup blocked kernel beyond ldltm::supports; the one-workgroup tile kernels are reached only with
ORBG_LDLT_XCD=0 and have tests of their own):
  n1             1 free + 1 fixed keyframe, 30 points: 15 unknowns, the only inertial edge is the down-weighted Huber one     cols
  n2, n2_recinit 30 unknowns; rec_init: the Huber kernel on every inertial edge                                               cols
  inertial_only  3 free keyframes, no points, no visual edge: 45 unknowns                                                     cols
  no_imu_middle  a free keyframe without IMU (6 unknowns) between two others: the offset table, the chain broken: 51          cols
  rejected       an iteration that rejects five trials before it accepts one: 45                                              cols
  stale          a run that ENDS on a rejected trial (rho == 0 exactly, tests/inertial_ba_model.py: CASES): chi2, verdicts and
                 chi2_final of the rejected state, vertices of the accepted one: 45                                           cols
  lap-1/+0/+1    255 / 256 / 257 points, edges per keyframe and items per pair (the lap of every new kernel): 30              cols
  n4_newest_first, n10_newest_first   the keyframe list in the order the glue hands it over (window newest first, then the fixed
                 predecessor): the earlier keyframe of every inertial edge has the larger column, the couplings between free
                 keyframes are read transposed (k_iba_schur's `ro = 15, co = 0` blocks): 60 and 150                          cols, xcd
  n10            10 + 5 fixed keyframes, 300 points, stereo and mono, 5 % outliers, close points, points behind a camera: 150 xcd
  n19            19 free keyframes: 285 unknowns, the last size of ldltm::supports                                           xcd
  n25_large      25 free keyframes, lambda 1e-2, 4 iterations: 375                                                            wide
  n32_cap        32 free keyframes, the most the entry point takes: 480                                                       wide
"""
import os
import re
import threading

import numpy as np
import pytest

import inertial_ba_model as m
from multi_orbslam3_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = {"n1": "cols", "n2": "cols", "n2_recinit": "cols", "inertial_only": "cols", "no_imu_middle": "cols", "rejected": "cols", "stale": "cols",
          "lap-1": "cols", "lap+0": "cols", "lap+1": "cols", "n4_newest_first": "cols", "n10": "xcd", "n10_newest_first": "xcd", "n19": "xcd",
          "n25_large": "wide", "n32_cap": "wide"}
NAMES = list(FAMILY)


def _const(header, name):
    src = open(os.path.join(ROOT, "multi_orbslam3_amd", "csrc", header)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


def ldlt_family(n):
    """LdltSolver::plan without switches: ldltm::make_geo / supports / pick, ldltx::supports / plan_fits"""
    kColT, kMaxT, kNY, kChain, kMaxP, kWgWaves = (_const("ldlt_mfma.hpp", "kColT"), _const("ldlt_mfma.hpp", "kMaxT"), _const("ldlt_xcd.hpp", "kNY"),
                                                  _const("ldlt_xcd.hpp", "kChain"), _const("ldlt_xcd.hpp", "kMaxP"), 8)
    n_pad = (n + 3) & ~3
    T = (n_pad + 1 + 15) // 16
    if T > 19:
        return "wide"
    ntiles = T * (T + 1) // 2
    ct = sum(min(j + 1, kChain) for j in range(T))
    fits = T <= kMaxP * kWgWaves and ntiles - ct <= (kMaxP * kWgWaves - T) * 4
    if 9 <= T <= kMaxT - 1 and n_pad <= 64 * kNY and fits:
        return "xcd"
    return "cols" if T <= kColT else "tile"


@pytest.fixture(scope="module")
def opt():
    return api.Optimizer()


def _solve(opt, P, handle=None):
    p, keep = m.to_c_problem(P)
    return opt.LocalInertialBA(p, handle=handle)


_gpu = {}


def gpu_result(opt, name):
    if name not in _gpu:
        _gpu[name] = _solve(opt, m.case_results(name)[0])
    return _gpu[name]


def test_cases_take_the_families_stated():
    for name in NAMES:
        assert ldlt_family(m.Structure(m.build_case(name)).n) == FAMILY[name], name
    assert {ldlt_family(n) for n in range(6, 481)} - {"tile"} == set(FAMILY.values())
    # the tile kernels are behind ORBG_LDLT_XCD=0 only: every size they would take goes to the eight-workgroup kernel
    assert "tile" not in {ldlt_family(n) for n in range(6, 481)}


@pytest.mark.parametrize("name", NAMES)
def test_against_the_model(opt, name):
    P, rb, rr, ra = m.case_results(name)
    g = gpu_result(opt, name).as_dict()
    y = m.yardsticks_of(rb, rr, ra)
    d_state = m.state_difference(g, rb, points=False)
    d_points = m.float_points_excess(g["points"], rb)
    fr = y["fr_rows"]
    noise = fr > m.NOISE_ROW                                     # rows of the trace that are rounding noise by the model's own account
    f_trace = float(fr[~noise].max()) if (~noise).any() else 0.0
    tb = max(1e-9, 10.0 * f_trace)
    rows = m.trace_rows_difference(g, rb)
    d_trace = float("inf") if rows is None else (float(rows[~noise].max()) if (~noise).any() else 0.0)
    print("%s: unknowns %d, device-model state %.3e points beyond float rounding %.3e (yardstick %.3e, bound %.3e), trace %.3e (yardstick %.3e, "
          "bound %.3e); (a)-(b) state %.3e trace %.3e" % (name, rb["n_unknowns"], d_state, d_points, y["fr_state"], m.MARGIN * y["fr_state"], d_trace,
                                                          f_trace, tb, y["ab_state"], y["ab_trace"]))
    # the LM decisions of these cases are outside the band (test_inertial_ba_cpu.py): iterations and trial counts are the model's
    assert g["iters"] == rb["iters"]
    assert np.array_equal(g["trace"][:, 2], rb["trace"][:, 2]), (g["trace"][:, 2], rb["trace"][:, 2])
    assert d_trace <= tb
    assert np.all(g["trace"][noise, 1] <= m.NOISE_LEVEL * rb["chi2_initial"]) and np.all(rb["trace"][noise, 1] <= m.NOISE_LEVEL * rb["chi2_initial"])
    assert abs(g["chi2_initial"] - rb["chi2_initial"]) <= tb * abs(rb["chi2_initial"])
    if noise.any() and noise[-1]:
        assert g["chi2_final"] <= m.NOISE_LEVEL * rb["chi2_initial"]
    else:
        assert abs(g["chi2_final"] - rb["chi2_final"]) <= tb * abs(rb["chi2_final"])
    assert d_state <= m.MARGIN * y["fr_state"]
    assert d_points <= m.MARGIN * y["fr_state"]                  # (the result's points are floats: beyond the rounding to float)
    # verdicts: equal outside the band round their thresholds
    S = m.Structure(P)
    close = np.asarray(P["close"], bool)[S.e_pt] if S.NE else np.zeros(0, bool)
    th = np.where(S.mono, np.where(close, m.CHI2_CLOSE, m.CHI2_MONO), m.CHI2_STEREO)
    sure = np.abs(rb["edge_chi2"] - th) > m.BAND * th
    assert np.array_equal(g["edge_outlier"][sure], rb["edge_outlier"][sure])
    assert np.array_equal(g["edge_depth_pos"], rb["edge_depth_pos"])
    d_edge, eb = m.edge_chi2_difference(g, rb), max(1e-9, 10.0 * y["fr_edge"])      # (the trace's rule on the single edges' chi2)
    print("%s: edge chi2 %.3e (yardstick %.3e, bound %.3e)" % (name, d_edge, y["fr_edge"], eb))
    assert d_edge <= eb
    assert g["n_outliers"] == int(g["edge_outlier"].sum())
    assert g["failed"] == rb["failed"]
    # against the reference's float round trips
    assert m.state_difference(g, ra, points=False) <= m.MARGIN * y["fr_state"] + y["ab_state"]
    if not noise.any():
        assert m.trace_difference(g, ra, scale=rb) <= tb + y["ab_trace"]      # (both relative to the values of (b): the two bounds add up)


def test_rejected_trial_leaves_the_accepted_state(opt):
    """the case's trace has an iteration with more than one trial; the states are the model's (the rejected trials' buffers dropped)"""
    g = gpu_result(opt, "rejected").as_dict()
    assert g["trace"][:, 2].max() >= 2 and g["trace"][-1, 2] == 1


def test_run_that_ends_on_a_rejected_trial(opt):
    """`stale`: the vertices are the start's (pop() restored them), e->chi2() and the verdicts are the rejected trial's -- not those of a
    fresh evaluation at the returned estimate, which the model's fresh_chi2 switch computes and which erases 254 edges more"""
    P, rb, _, _ = m.case_results("stale")
    g = gpu_result(opt, "stale").as_dict()
    assert rb["last_rejected"] and g["iters"] == 1 and g["trace"][:, 2].tolist() == [1.0] and g["trace"][0, 0] == 2.0      # lambda * ni
    kfs, X = m.initial_state(P)
    assert m.state_difference(g, {"states": kfs, "points": X}, points=False) == 0.0 and np.array_equal(g["points"], np.asarray(P["points"], np.float32))
    assert g["chi2_final"] == g["chi2_initial"] == rb["chi2_initial"]
    fresh = m.solve(P, fresh_chi2=True)
    assert np.array_equal(g["edge_outlier"], rb["edge_outlier"]) and g["n_outliers"] == rb["n_outliers"]
    assert (g["edge_outlier"] != fresh["edge_outlier"]).sum() > 100
    assert np.abs(g["edge_chi2"] - fresh["edge_chi2"]).max() > 1e3 * np.abs(g["edge_chi2"] - rb["edge_chi2"]).max()


def test_write_back_through_the_wrapper(opt):
    """SetVelocity / SetNewBias / SetPose / SetWorldPos values in float: within 1e-4 of the model's"""
    P, rb, _, _ = m.case_results("n10")
    out = gpu_result(opt, "n10")
    kfs, pts = out.write_back(P["Tcb"])
    Tcb = np.asarray(P["Tcb"], np.float64).reshape(3, 4)
    for s, w in zip(rb["states"], kfs):
        Rcw, tcw = m.pim.camera_pose(s, Tcb)
        assert np.abs(w["Tcw"][:3, :3] - Rcw).max() <= 1e-4 and np.abs(w["Tcw"][:3, 3] - tcw).max() <= 1e-4
        assert np.abs(w["vwb"] - s["v"]).max() <= 1e-4
        assert np.abs(w["bias"] - np.concatenate([s["ba"], s["bg"]])).max() <= 1e-4
    assert np.abs(pts - rb["points"]).max() <= 1e-4


def _bits(out):
    d = out.as_dict()
    return [m.state_vector(d), d["edge_chi2"], d["edge_depth_pos"], d["edge_outlier"], d["trace"],
            np.array([d["n_outliers"], d["failed"], d["iters"], d["chi2_initial"], d["chi2_final"]])]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def test_two_solves_on_one_handle_return_the_same_bits(opt):
    h = api.InertialBA()
    try:
        for name in ("n10", "n2", "n25_large", "n10"):          # the buffers and the solver object change size in between
            P = m.case_results(name)[0]
            a, b = _solve(opt, P, h), _solve(opt, P, h)
            assert _same_bits(a, b), name
            assert _same_bits(a, gpu_result(opt, name)), name   # ... and the handle-less call's
    finally:
        h.close()


def test_set_stream_and_threads(opt):
    """inertial_ba_set_stream, and two threads solving concurrently (each with its own handle): the same bits as a lone call"""
    import torch
    names = ("n10", "no_imu_middle")
    want = [gpu_result(opt, n) for n in names]
    st = torch.cuda.Stream()
    h = api.InertialBA()
    try:
        h.set_stream(st.cuda_stream)
        on_stream = [_solve(opt, m.case_results(n)[0], h) for n in names]
        h.set_stream(None)
        back = [_solve(opt, m.case_results(n)[0], h) for n in names]
    finally:
        h.close()
    res = [None, None]

    def work(k):
        hk = api.InertialBA()
        try:
            res[k] = [_solve(opt, m.case_results(names[k])[0], hk) for _ in range(3)]
        finally:
            hk.close()
    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        for r in [on_stream[k], back[k]] + res[k]:
            assert _same_bits(r, want[k]), names[k]
