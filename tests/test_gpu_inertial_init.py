"""inertial_init_solve (csrc/inertial_init.hip) on the device, through api.Optimizer.InertialOptimization, against
tests/inertial_init_model.py, variant "kernel" (double throughout):
  - iters, the trial count of every iteration and solve_failed are the model's (tests/test_inertial_init_cpu.py holds every case to no LM
    decision within a relative 1e-4 of its threshold, so they are compared outright);
  - velocities, biases, Rwg and scale within MARGIN = 8 times the case's yardstick: the difference of the model's own two solves, (a) dense
    normal equations against (b) the kernel's elimination order, floored at one unit in the last place of the largest component;
  - chi2 of the trace within max(1e-9, 10 f), f the (a)-against-(b) difference of the trace.  A row the model's two solves do not
    reproduce to NOISE_ROW is left out of f and held absolutely (tests/test_gpu_inertial_ba.py).  lambda by the same rule plus the
    rounding of a chi2 as the gain ratio amplifies it (inertial_init_model.trace_bounds; DESIGN.md section 4 lists the yardsticks);
  - against variant "reference" (the float round trips of the reference): that bound plus the model's kernel-against-reference difference.

The cases (inertial_init_model.CASES):
  n2                     2 keyframes, 1 edge, the monocular first overload: 15 unknowns, the smallest system
  n10_mono, n10_stereo   the reference's minimum of 10 keyframes; scale free / fixed
  n10_auto_lambda        priorG = 0: lambda = tau * the largest diagonal entry
  n10_fixed_vel          bFixedVel: only the gravity direction and the scale -- the system is the corner alone
  n10_bias               second / third overload: gravity and scale fixed at I and 1
  n10_gn                 fourth overload: Gauss-Newton, 10 iterations
  gn_degenerate          fourth overload, all velocities zero and all positions equal: the scale column is exactly zero, the pivot is
                         refused, solve_failed is set, the estimates come back unchanged
  newest_first           the keyframe list reversed: k1 > k2 in every edge
  broken, isolated, fork two chains; a keyframe without an edge, whose velocity comes back bit for bit; two keyframes sharing a predecessor
  rejected               an iteration that rejects trials before it accepts one
  nbad_stop, runs_out    ends by the _nBad rule; ends by the iteration count
  edges63 .. edges257    the wavefront and workgroup laps of the edge loops and reductions, 3 iterations
  tile-1 / +0 / +1       kIiTile (read from the source) -1 / +0 / +1 keyframes: the per-vertex blocks in LDS / in global memory, 3 iterations
  cap                    4096 keyframes (velocities, gravity direction and scale free, the biases fixed), 3 iterations; 4097 are refused
                         with ORBG_CAP_EXCEEDED
"""
import threading

import numpy as np
import pytest

import inertial_init_model as m
from multi_orbslam3_amd import _capi as capi, api

pytestmark = pytest.mark.gpu

NAMES = list(m.CASES)


@pytest.fixture(scope="module")
def opt():
    return api.Optimizer()


_gpu = {}


def gpu_result(opt, name):
    if name not in _gpu:
        p, keep = m.to_c_problem(m.case_results(name)[0])
        _gpu[name] = opt.InertialOptimization(p)
    return _gpu[name]


def _bytes(out):
    d = out.as_dict()
    return b"".join(np.ascontiguousarray(d[k], np.float64).tobytes() for k in ("vwb", "bg", "ba", "Rwg", "scale", "chi2_first", "chi2_final", "trace")) + \
        bytes([d["iters"] & 255, d["solve_failed"]])


def _rel(a, b, den):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(den), 1e-300)


@pytest.mark.parametrize("name", NAMES)
def test_against_the_model(opt, name):
    P, rb, ra, rr = m.case_results(name)
    g = gpu_result(opt, name).as_dict()
    y = m.yardsticks_of(rb, ra)
    lam_b, chi_b, noise, f_trace = m.trace_bounds(rb, ra)
    d_state = m.state_difference(g, rb)
    d_ref = m.state_difference(rr, rb)
    same_flow = g["trace"].shape == rb["trace"].shape and np.array_equal(g["trace"][:, 2], rb["trace"][:, 2])
    d_lam = _rel(g["trace"][:, 0], rb["trace"][:, 0], rb["trace"][:, 0]) if same_flow else np.full(len(lam_b), np.inf)
    d_chi = _rel(g["trace"][:, 1], rb["trace"][:, 1], rb["trace"][:, 1]) if same_flow else np.full(len(chi_b), np.inf)
    print("%s: unknowns %d iters %d trials %s, device-model state %.3e (yardstick (a)-(b) %.3e, bound %.3e), chi2 rows %.3e (yardstick %.3e, bound "
          "%.3e), lambda rows %.3e (bound %.3e, amplification %.3e), kernel-reference %.3e" % (
              name, g["n_unknowns"], g["iters"], "".join("%x" % int(q) for q in g["trace"][:, 2]), d_state, y["ab_state"], m.MARGIN * y["ab_state"],
              d_chi[~noise].max(initial=0.0), f_trace, chi_b.max(initial=0.0), d_lam[~noise].max(initial=0.0), lam_b.max(initial=0.0),
              rb["lambda_amp"].max(initial=0.0), d_ref))
    assert g["n_unknowns"] == rb["n_unknowns"]
    assert g["iters"] == rb["iters"]
    assert g["solve_failed"] == rb["solve_failed"]
    assert same_flow, (g["trace"][:, 2], rb["trace"][:, 2])
    assert np.all(d_chi[~noise] <= chi_b[~noise])
    assert np.all(d_lam[~noise] <= lam_b[~noise])
    assert np.all(np.abs(g["trace"][noise, 1] - rb["trace"][noise, 1]) <= 1e-12 * rb["chi2_first"])
    tb = chi_b.max(initial=1e-9)
    assert abs(g["chi2_first"] - rb["chi2_first"]) <= tb * abs(rb["chi2_first"])
    if not (noise.any() and noise[-1]):
        assert abs(g["chi2_final"] - rb["chi2_final"]) <= tb * abs(rb["chi2_final"])
    assert d_state <= m.MARGIN * y["ab_state"]
    # against the reference's float round trips: that bound plus the model's kernel-against-reference difference
    assert m.state_difference(g, rr) <= m.MARGIN * y["ab_state"] + d_ref
    if rr["trace"].shape == rb["trace"].shape and np.array_equal(rr["trace"][:, 2], rb["trace"][:, 2]):
        den = rb["trace"]
        assert np.all(_rel(g["trace"][:, 0], rr["trace"][:, 0], den[:, 0])[~noise] <= (lam_b + _rel(rr["trace"][:, 0], den[:, 0], den[:, 0]))[~noise])
        assert np.all(_rel(g["trace"][:, 1], rr["trace"][:, 1], den[:, 1])[~noise] <= (chi_b + _rel(rr["trace"][:, 1], den[:, 1], den[:, 1]))[~noise])


def test_degenerate_gauss_newton_leaves_the_estimates(opt):
    P, rb, _, _ = m.case_results("gn_degenerate")
    g = gpu_result(opt, "gn_degenerate").as_dict()
    assert g["solve_failed"] == 1 and g["iters"] == 1
    assert np.array_equal(g["Rwg"], np.asarray(P["Rwg"], np.float64)) and g["scale"] == P["scale"]
    assert np.array_equal(g["vwb"], P["keyframes"]["v"].astype(np.float64))
    assert g["chi2_final"] == g["chi2_first"]


def test_keyframe_without_an_edge_keeps_its_velocity(opt):
    P = m.case_results("isolated")[0]
    g = gpu_result(opt, "isolated").as_dict()
    k = m.CASES["isolated"]["isolated"][0]
    assert np.array_equal(g["vwb"][k], P["keyframes"]["v"][k].astype(np.float64))
    others = [i for i in range(len(g["vwb"])) if i != k]
    assert not np.any(np.all(g["vwb"][others] == P["keyframes"]["v"][others].astype(np.float64), axis=1))


def test_fixed_velocities_come_back_as_they_went_in(opt):
    for name in ("n10_fixed_vel", "n10_gn"):
        P = m.case_results(name)[0]
        assert np.array_equal(gpu_result(opt, name).as_dict()["vwb"], P["keyframes"]["v"].astype(np.float64))


def test_one_keyframe_too_many_is_refused(opt):
    P = m.make_scene(n=capi.INERTIAL_INIT_MAX_KEYFRAMES + 1, seed=51, **dict(m.form_problem(4), iterations=1))
    p, keep = m.to_c_problem(P)
    with pytest.raises(capi.OrbGpuError) as e:
        opt.InertialOptimization(p)
    assert e.value.code == capi.ORBG_CAP_EXCEEDED


def test_two_calls_return_the_same_bytes(opt):
    p, keep = m.to_c_problem(m.case_results("n10_mono")[0])
    assert _bytes(opt.InertialOptimization(p)) == _bytes(gpu_result(opt, "n10_mono"))


def test_two_host_threads_return_those_bytes(opt):
    """each thread has a work area of its own (the staging block, the edge blocks, the trial velocities)"""
    want = _bytes(gpu_result(opt, "n10_mono"))
    P = m.case_results("n10_mono")[0]
    got, errs = [None, None], []
    start = threading.Barrier(2)

    def run(i):
        try:
            p, keep = m.to_c_problem(P)
            start.wait()
            for _ in range(8):
                got[i] = _bytes(opt.InertialOptimization(p))
                if got[i] != want:
                    break
        except Exception as ex:                                  # noqa: BLE001
            errs.append(ex)

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert got[0] == want and got[1] == want
