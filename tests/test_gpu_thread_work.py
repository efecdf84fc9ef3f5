"""The entry points without a handle keep their device buffers and their stream with the CALLING THREAD (csrc/common.hpp, WorkArea),
released when that thread exits: threads that come, call and go leave the answers of every later caller as they were."""
import ctypes as C
import threading

import numpy as np
import pytest

import sim3_model as sm
import sim3_opt_model as om
from multi_orbslam3_amd import _capi as capi, api, synth, views

pytestmark = pytest.mark.gpu


def _pose():
    pr = synth.make_pose_opt_problem(n=40, outlier_frac=0.1, mono_frac=0.5, seed=140)
    p, keep = views.pose_opt_problem(pr["Xw"], pr["u"], pr["v"], pr["ur"], pr["inv_sigma2"], pr["cam"], pr["Tcw"])
    lib = capi.load()

    def call():
        out = views.PoseOptOutput(p.n)
        capi.check(lib.pose_optimize(C.byref(p), C.byref(out.c)), "pose_optimize")
        return [out.Tcw, out.outliers, np.array(out.iters), np.array(out.chi2), np.array([out.c.n_inliers, out.c.n_bad])]
    return call, keep


def _sim3_ransac():
    rng = np.random.default_rng(3)
    scs = [sm.make_scene(611 + b, 20, b == 0, 0.3) for b in range(2)]
    probs = [api.Sim3Problem(sc["X1"], sc["X2"], sc["e1"], sc["e2"], sc["K1"], sc["K2"], b == 0) for b, sc in enumerate(scs)]
    params = [(0.99, 6, 300), (0.99, 8, 100)]
    draws = [api.sim3_draws(20, sm.ransac_iterations(20, *q), rng) for q in params]

    def call():
        out = []
        for r in api.Sim3Solver.solve_batch(probs, params, draws):
            out += [np.array([r.bNoMore, r.bConverge, r.nInliers, r.iterations_done, r.best_iteration, r.best_inliers, r.have_best,
                              r.T12 is None]), r.vbInliers, r.best_mask]
            if r.have_best:
                out += [r.best_T12, r.best_R, r.best_t, r.best_s]
        return out
    return call, None


def _sim3_opt():
    probs = []
    for e in ((30100, 30, True, 0.0, None), (30001, 30, False, 0.3, None)):
        m = om.family_problem(e)
        probs.append(api.Sim3OptProblem(m.X1, m.X2, m.obs1, m.obs2, m.w1, m.w2, m.K1, m.K2, m.fix_scale, m.th2, m.q, m.t, m.s,
                                        n_correspondences=m.n_corr))

    def call():
        out = []
        for r in api.OptimizeSim3.batch(probs):
            out += [np.array([r.nIn, r.returned_early, r.n_bad_round1]), r.q, r.t, np.float64(r.s), r.removed, np.array(r.iters),
                    np.float64(r.chi2), r.trace]
        return out
    return call, None


def _distinctive():
    rng = np.random.RandomState(4)
    desc = rng.randint(0, 256, (9, 32)).astype(np.uint8)
    start = np.array([0, 1, 4, 9], np.int32)                     # m = 3 groups of 1, 3 and 5 descriptors
    return (lambda: [api.ComputeDistinctiveDescriptors(desc, start)]), None


def _score():
    rng = np.random.RandomState(17)

    def bow(nw):
        w = np.sort(rng.choice(2000, nw, replace=False)).astype(np.int32)
        v = rng.rand(nw)
        return w, v / v.sum()
    qw, qv = bow(40)
    cands = [bow(25), (qw, qv)]
    cs = np.cumsum([0] + [len(c[0]) for c in cands]).astype(np.int32)
    cw = np.concatenate([c[0] for c in cands]); cv = np.concatenate([c[1] for c in cands])
    return (lambda: [api.BowScoreL1(qw, qv, cs, cw, cv)]), None


def _fisheye():
    fs = synth.make_fisheye_stereo_scene(n_stereo=20, n_mono_left=5, n_mono_right=5, n_distract=5)
    v, keep = views.fisheye_stereo_view(fs["kps_left"], fs["desc_left"], fs["mono_left"], fs["kps_right"], fs["desc_right"], fs["mono_right"], fs["left"],
                                        fs["right"], fs["Tlr"], fs["level_sigma2"])

    def call():
        g = api.ComputeStereoFishEyeMatches(v)
        return [g[0], g[1], g[2], g[3], np.array(g[4])]
    return call, keep


def _bits(arrays):
    return [(np.asarray(a).dtype.str, np.asarray(a).shape, np.asarray(a).tobytes()) for a in arrays]


@pytest.mark.parametrize("make", [_pose, _sim3_ransac, _sim3_opt, _distinctive, _score, _fisheye])
def test_threads_that_call_and_exit_leave_the_answers_alone(make):
    call, keep = make()
    first = _bits(call())
    assert first
    for k in range(3):                                             # one after another: each thread's work area is released when it ends
        got, err = [], []

        def work():
            try:
                got.append(_bits(call()))
                got.append(_bits(call()))
            except BaseException as e:       # noqa: BLE001 -- reported by the main thread
                err.append(repr(e))
        t = threading.Thread(target=work)
        t.start()
        t.join()
        assert not err, (k, err)
        assert len(got) == 2 and got[0] == first and got[1] == first, k
    assert _bits(call()) == first
