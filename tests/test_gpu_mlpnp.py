"""MLPnPsolver on the device against the checker of tests/mlpnp_model.py: every hypothesis (formulation (b), the kernel restated in
numpy; tolerance from the model's own (a)-vs-(b) difference), the planar branch, the replayed control flow (exact), the batch form, the
w = 0 pin and set_stream."""
import threading

import numpy as np
import pytest

import mlpnp_model as mm
from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import api

pytestmark = pytest.mark.gpu

RELOC = (0.99, 10, 300, 6, 0.5, 5.991)          # S/Tracking.cc:3401
MARGIN = 8                                       # a third implementation with another operation order: 8 x the (a)-vs-(b) difference


def _problem(sc):
    return api.MLPnPProblem(sc["P2D"], sc["sigma2"], sc["bearing"], sc["P3Dw"], sc["K"], sc["kp_index"], sc["m"])


def _all_hypotheses(sc, drw):
    """Every hypothesis of `drw` from ONE launch that cannot return early: with min_inliers = n no count exceeds it, and because the
    loop condition is an OR, iterate(H) runs H iterations whatever mRansacMaxIts is."""
    n, H = len(sc["P2D"]), len(drw)
    s = api.MLPnPsolver(_problem(sc))
    s.SetRansacParameters(0.99, n, H, 6, 0.4, 5.991)
    assert s.mRansacMinInliers == n and s.iterations_of_call(H) == H
    it = s.iterate(H, drw, per_hypothesis=True)
    s.close()
    assert it.iterations_run == H and it.hyp_n_inliers.shape == (H,) and it.hyp_masks.shape == (H, n) and it.hyp_R.shape == (H, 3, 3)
    assert np.array_equal(it.hyp_n_inliers, it.hyp_masks.sum(axis=1))
    return it


def _compare(sc, drw, model, what):
    """The assertions of test 1 for one scene.  -> (decisions, left out, hypotheses, low gap, NaN)"""
    it = _all_hypotheses(sc, drw)
    me = mm.max_errors(sc["sigma2"], 5.991)
    decisions = left_out = low_gap = nan = 0
    worst = {}
    for k, hb in enumerate(model):
        got = dict(R=it.hyp_R[k], t=it.hyp_t[k])
        nan_m, nan_p = not np.isfinite(hb["R"]).all(), not (np.isfinite(got["R"]).all() and np.isfinite(got["t"]).all())
        assert nan_m == nan_p, (what, k)
        assert bool(it.hyp_planar[k]) == hb["planar"], (what, k)
        if nan_p:
            nan += 1
            assert it.hyp_n_inliers[k] == 0, (what, k)
            continue
        near = mm.near_threshold(hb["e2"], me)
        decisions += len(me)
        left_out += int(near.sum())
        bad = (it.hyp_masks[k] != hb["mask"]) & ~near
        assert not bad.any(), (what, k, np.nonzero(bad)[0][:5].tolist())
        b = mm.band_of(hb["gap"])
        if b < 0:
            low_gap += 1
            continue
        d = mm.pose_difference(got, hb)
        worst[b] = max(worst.get(b, 0.0), d)
        assert d <= MARGIN * mm.yardstick(b), (what, k, b, d, MARGIN * mm.yardstick(b), hb["gap"])
    for b in sorted(worst):
        print("%s gap band %d: max |pose - model| = %.3g (tolerance %.3g)" % (what, b, worst[b], MARGIN * mm.yardstick(b)))
    return decisions, left_out, len(model), low_gap, nan


def test_every_hypothesis_against_the_model():
    """Masks equal, leaving out decisions whose model error2 lies within a relative 1e-4 of its threshold (at most 0.1 %); poses of
    hypotheses with an eigen gap >= 1e-8 (all but at most 2 %) within 8 x the model's yardstick of the same band (mlpnp_model.yardstick:
    the (a)-vs-(b) difference tests/test_mlpnp_cpu.py prints); NaN hypotheses NaN in both, without inliers."""
    ms = mm.measure()
    tot = np.zeros(5, np.int64)
    for i, case in enumerate(mm.CASES):
        sc, drw = mm.case_scene(i)
        tot += _compare(sc, drw, ms["b"][i], "n=%d H=%d" % (case[0], case[2]))
    print("decisions %d, left out %d; hypotheses %d, gap < 1e-8: %d, NaN: %d" % tuple(tot))
    assert tot[1] <= 1e-3 * tot[0] and tot[3] <= 0.02 * tot[2]


def test_planar_branch():
    """A scene on the world plane z = 0 has exact rank 2: every hypothesis is planar, same assertions.  A tilted plane that does not pass
    through the origin is not planar for the reference (the test matrix is not centred): no hypothesis reports it."""
    i = len(mm.CASES)
    sc, drw = mm.case_scene(i)
    hb = mm.measure()["b"][i]
    assert all(h["planar"] for h in hb) and max(h["count"] for h in hb) >= 25      # the branch really solves the scene
    d, lo, h, lg, nan = _compare(sc, drw, hb, "planar")
    assert lo <= 1e-3 * d and lg <= 0.02 * h
    sc, drw = mm.case_scene(i + 1)
    it = _all_hypotheses(sc, drw)
    assert not it.hyp_planar.any()
    assert not any(mm.compute_pose(sc["P3Dw"][ix], sc["bearing"][ix], "b")["planar"] for ix in mm.resolve_draws(40, drw))


# ------------------------------------------------------------------ control flow

def _control_case(name):
    """-> (scene, SetRansacParameters' arguments, draw seed)"""
    if name == "first_call":
        return mm.make_scene(401, 100, 0.3), RELOC, 401
    if name == "tie_no_more":                    # counts are 0 or 8 = min_inliers: never exceeded, the first 8 stays the best
        return mm.make_scene(410, 10, 0.2), (1 - 1e-9, 8, 300, 6, 0.1, 5.991), 410
    if name == "too_few":
        return mm.make_scene(420, 7, 0.0), RELOC, 420
    raise KeyError(name)


@pytest.mark.parametrize("name", ["first_call", "tie_no_more", "too_few"])
def test_control_flow_is_the_serial_loops(name):
    sc, params, seed = _control_case(name)
    n = len(sc["P2D"])
    prob = _problem(sc)
    max_its, min_inl, _ = mm.ransac_iterations(n, *params[:5])
    assert api.mlpnp_ransac_iterations(n, *params) == (max_its, min_inl)
    total = 4 * max_its + 40
    drw = mm.draws(max(n, 6), total, seed)
    if n >= min_inl:
        full = _all_hypotheses(sc, drw)
        counts, masks, poses = full.hyp_n_inliers, full.hyp_masks, list(zip(full.hyp_R, full.hyp_t))
    else:
        counts, masks, poses = np.zeros(total, np.int32), np.zeros((total, n), bool), [None] * total
    if name == "tie_no_more":
        assert counts[:max_its].max() == min_inl and (counts[:max_its] == min_inl).sum() >= 2
    for chunk in (None, 5, 1):
        s = api.MLPnPsolver(prob)
        s.SetRansacParameters(*params)
        m = mm.SerialSolver(n, sc["m"], sc["kp_index"], min_inl, max_its)
        outs = []
        for call in range(4):
            nit = max_its if chunk is None else chunk
            k = s.iterations_of_call(nit)
            assert k == m.iterations_of_call(nit), (name, chunk, call)
            k0 = m.iterations
            it = s.iterate(nit, drw[k0:k0 + k])
            o = m.iterate(nit, counts[k0:k0 + k], masks[k0:k0 + k], poses[k0:k0 + k])
            assert it.fields() == mm.SerialSolver.fields(o), (name, chunk, call)
            outs.append(it)
        s.close()
        if name == "first_call":
            assert outs[0].returned and not outs[0].bNoMore and outs[0].iterations_done < max_its
            assert outs[1].iterations_done > outs[0].iterations_done         # a second call after a return goes on in the draws
        if name == "tie_no_more":
            assert outs[0].bNoMore and outs[0].returned and outs[0].nInliers == min_inl
            assert outs[0].best_iteration == int(np.nonzero(counts[:max_its] == min_inl)[0][0])
        if name == "too_few":
            assert all(o_.bNoMore and not o_.returned and o_.iterations_done == 0 for o_ in outs)


# ------------------------------------------------------------------ batch

def _batch_inputs(B, seed):
    rng = np.random.default_rng(seed)
    ns = [40, 120, 300, 65, 513, 7, 2000, 64]
    probs, params, drw = [], [], []
    for b in range(B):
        n = ns[b % len(ns)]
        sc = mm.make_scene(500 + 10 * seed + b, n, (0.3, 0.5, 0.9)[b % 3])
        par = (RELOC, api.MLPNP_DEFAULTS, (0.99, 10, 60, 6, 0.3, 5.991))[b % 3]
        probs.append(_problem(sc)); params.append(par)
        drw.append(mm.draws(max(n, 6), mm.ransac_iterations(n, *par[:5])[0], rng))
    return probs, params, drw


@pytest.mark.parametrize("B", [1, 4, 16])
def test_batch_equals_single_solvers_bit_for_bit(B):
    probs, params, drw = _batch_inputs(B, B)
    r1 = api.MLPnPsolver.solve_batch(probs, params, drw)
    r2 = api.MLPnPsolver.solve_batch(probs, params, drw)
    assert len(r1) == B
    for b in range(B):
        s = api.MLPnPsolver(probs[b])
        s.SetRansacParameters(*params[b])
        single = s.iterate(5, drw[b])
        s.close()
        assert r1[b].fields() == single.fields(), b
        assert r1[b].fields() == r2[b].fields(), b
    assert any(r.returned for r in r1)


def test_three_solvers_from_three_threads():
    probs, params, drw = _batch_inputs(3, 7)
    want = api.MLPnPsolver.solve_batch(probs, params, drw)
    errors = []

    def work(b):
        try:
            for _ in range(5):
                s = api.MLPnPsolver(probs[b])
                s.SetRansacParameters(*params[b])
                assert s.iterate(5, drw[b]).fields() == want[b].fields()
                assert api.MLPnPsolver.solve_batch([probs[b]], [params[b]], [drw[b]])[0].fields() == want[b].fields()
                s.close()
        except BaseException as e:       # noqa: BLE001 -- reported by the main thread
            errors.append((b, repr(e)))

    th = [threading.Thread(target=work, args=(b,)) for b in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


# ------------------------------------------------------------------ pins

def test_identity_rotation_gives_a_nan_pose_without_inliers():
    """rot2rodrigues of an exact identity is zero and the reference's Jacobian divides by |omega|^2: a NaN pose (behaviour 5).  The
    step is NaN and is applied (no comparison of :738 holds); rodrigues2rot of the NaN vector is the identity (:663 compares false), so
    the pose that comes out is [I | NaN]."""
    sc = mm.make_scene(1200, 6, 0.0)
    R, t = api.mlpnp_gn(sc["P3Dw"], sc["bearing"], np.eye(3), sc["t"])
    assert np.isnan(t).all() and np.array_equal(R, np.eye(3))
    Rm, tm = mm.refine_stage(np.eye(3), sc["t"], sc["P3Dw"], sc["bearing"])
    assert np.isnan(tm).all() and np.array_equal(Rm, np.eye(3))
    mask, _ = mm.check_inliers(R, t, sc["P3Dw"], sc["P2D"], mm.max_errors(sc["sigma2"], 5.991))
    assert not mask.any()
    # the same stage away from the identity: the scene's pose, a little off, comes back refined and equal to the model's
    R0 = sc["R"] @ mm.rodrigues2rot(np.array([0.01, -0.02, 0.015]))
    R, t = api.mlpnp_gn(sc["P3Dw"], sc["bearing"], R0, sc["t"] + 0.02)
    Rm, tm = mm.refine_stage(R0, sc["t"] + 0.02, sc["P3Dw"], sc["bearing"])
    assert np.abs(R - Rm).max() < 1e-9 and np.abs(t - tm).max() < 1e-9
    assert np.abs(R - sc["R"]).max() < 2e-2


def test_set_stream_between_two_iterate_calls():
    import torch
    sc, params, seed = _control_case("first_call")
    n = len(sc["P2D"])
    max_its = mm.ransac_iterations(n, *params[:5])[0]
    drw = mm.draws(n, max_its + 40, seed)
    own = torch.cuda.Stream()
    runs = []
    for move in (False, True):
        s = api.MLPnPsolver(_problem(sc))
        s.SetRansacParameters(*params)
        outs, k0 = [], 0
        for call in range(3):
            if move and call == 1:
                s.set_stream(own.cuda_stream)
            if move and call == 2:
                s.set_stream(None)
            k = s.iterations_of_call(5)
            outs.append(s.iterate(5, drw[k0:k0 + k]))
            k0 = outs[-1].iterations_done
        runs.append(outs)
        s.close()
    for a, b in zip(*runs):
        assert a.fields() == b.fields()
    assert runs[0][0].returned


def test_other_camera_models_are_refused():
    import ctypes as C
    sc = mm.make_scene(1300, 40, 0.3)
    lib = capi.load()
    h = C.c_void_p()
    assert lib.orbp_mlpnp_create(0, C.byref(h)) == capi.ORBG_OK
    prob = _problem(sc)
    st = prob.struct(camera_model=1)
    assert lib.orbp_mlpnp_set_problem(h, C.byref(st)) == capi.ORBG_BAD_ARG
    lib.orbp_mlpnp_destroy(h)
