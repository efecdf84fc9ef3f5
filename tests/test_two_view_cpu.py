"""TwoViewReconstruction without a GPU: the numpy model (tests/two_view_model.py) on scenes with a known answer, the draw helper
against the literal list replay, the C-ABI surface and its argument checks, and the two measured figures the GPU tests lean on."""
import ctypes as C

import numpy as np
import pytest

import two_view_model as tm
from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import api


def _angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))))


def _structure_error(sc, o, baseline):
    """vP3D is in units of the baseline (t21 has unit length): median relative error of the triangulated points."""
    tri = o.vbTriangulated[sc.pos1]
    est = o.vP3D[sc.pos1][tri].astype(np.float64) * baseline
    return float(np.median(np.linalg.norm(est - sc.X[tri], axis=1) / np.linalg.norm(sc.X[tri], axis=1))), int(tri.sum())


@pytest.mark.parametrize("ft", [np.float32, np.float64])
def test_model_recovers_a_known_motion_from_a_3d_scene_through_F(ft):
    """0.02 px noise is 4e-5 rad per ray, the parallax about 0.1 rad: an eight-point estimate amplifies the noise some tens of times, so
    the rotation is good to 0.1 degree, the direction of t to 1 degree and the depths to 3 %; a wrong decomposition is off by tens of
    degrees.  One match in ten is a mismatch."""
    sc = tm.scene("3d", 300, 21, n_extra1=37, n_extra2=71, noise=0.02, baseline=1.0)
    d = tm.case_draws(300, 200, 21)
    o = tm.reconstruct(sc.keys1, sc.keys2, sc.matches12, sc.cam, 1.0, 200, d, ft)
    assert o.model == 2 and o.ok and o.n_motions == 4
    assert o.SF / (o.SH + o.SF) > 0.5
    assert _angle_deg(o.R21, sc.R) < 0.1
    assert np.degrees(np.arccos(np.clip(float(o.t21.astype(np.float64) @ sc.t), -1, 1))) < 1.0
    err, n = _structure_error(sc, o, 1.0)
    assert n >= 0.85 * 300 and err < 0.03, (n, err)
    assert abs(float(np.linalg.norm(o.t21.astype(np.float64))) - 1) < 1e-6
    # indexed by the keypoint index of frame 1: nothing is triangulated at an unmatched keypoint
    assert not o.vbTriangulated[sc.matches12 < 0].any() and not o.vP3D[sc.matches12 < 0].any()


@pytest.mark.parametrize("ft", [np.float32, np.float64])
def test_model_recovers_a_known_motion_from_a_plane_through_H(ft):
    sc, d, o32, o64 = tm.case("plane")
    o = o32 if ft is np.float32 else o64
    assert o.SH / (o.SH + o.SF) > 0.5 and o.model == 1 and o.n_motions == 8 and o.ok
    assert _angle_deg(o.R21, sc.R) < 1.0
    assert np.degrees(np.arccos(np.clip(float(o.t21.astype(np.float64) @ sc.t), -1, 1))) < 5.0
    err, n = _structure_error(sc, o, 1.0)
    assert n >= 0.8 * 150 and err < 0.05, (n, err)


@pytest.mark.parametrize("kind", ["rotation", "tiny"])
def test_model_refuses_pure_rotation_and_sub_degree_parallax(kind):
    sc = tm.scene(kind, 200, 7, n_extra1=11, n_extra2=23)
    d = tm.case_draws(200, 200, 7)
    for ft in (np.float32, np.float64):
        o = tm.reconstruct(sc.keys1, sc.keys2, sc.matches12, sc.cam, 1.0, 200, d, ft)
        assert not o.ok and o.model in (1, 2)
        if o.n_motions:
            assert float(np.max(o.motion_parallax[o.motion_nGood > 0.9 * o.n_inliers], initial=0.0)) < 1.0


def test_serial_rule_of_the_model():
    """First iteration with the strictly largest score from score = 0; zero and NaN never win; SH + SF == 0 returns false."""
    f = np.float32
    assert tm.serial_best(np.array([0, 0, 0], f)) == (0, -1)
    assert tm.serial_best(np.array([np.nan, 0, np.nan], f))[1] == -1
    assert tm.serial_best(np.array([1, 3, np.nan, 3, 2], f)) == (3, 1)
    assert tm.choose_model(f(0), f(0)) == 0
    assert tm.choose_model(f(2), f(2)) == 2 and tm.choose_model(f(2.001), f(2)) == 1 and tm.choose_model(f(1), f(0)) == 1
    # :504-574: nsimilar > 1 rejects, so does maxGood < max(0.9 N, 50); the parallax of the winner decides
    assert tm.decide_F([100, 10, 0, 0], [2.0, 9, 9, 9], 100) == 0
    assert tm.decide_F([100, 71, 0, 0], [2.0, 9, 9, 9], 100) == -1
    assert tm.decide_F([100, 70, 0, 0], [2.0, 9, 9, 9], 100) == 0
    assert tm.decide_F([89, 0, 0, 0], [2.0, 9, 9, 9], 100) == -1
    assert tm.decide_F([0, 0, 60, 0], [9, 9, 1.0, 9], 60) == -1 and tm.decide_F([0, 0, 60, 0], [9, 9, 1.5, 9], 60) == 2
    assert tm.decide_F([40, 0, 0, 0], [9, 9, 9, 9], 10) == -1
    # :693-735
    assert tm.decide_H([0, 0, 100, 74, 0, 0, 0, 0], [0, 0, 1.0, 0, 0, 0, 0, 0], 100) == 2
    assert tm.decide_H([0, 0, 100, 75, 0, 0, 0, 0], [0, 0, 1.0, 0, 0, 0, 0, 0], 100) == -1
    assert tm.decide_H([0, 0, 100, 0, 0, 0, 0, 0], [0, 0, 0.99, 0, 0, 0, 0, 0], 100) == -1
    assert tm.decide_H([50, 0, 0, 0, 0, 0, 0, 0], [5, 0, 0, 0, 0, 0, 0, 0], 50) == -1
    assert tm.decide_H([90, 0, 0, 0, 0, 0, 0, 0], [5, 0, 0, 0, 0, 0, 0, 0], 100) == -1


def test_draw_resolution_against_the_literal_list_replay():
    rng = np.random.default_rng(3)
    for n in (8, 9, 10, 15, 16, 17, 100, 1000):
        d = api.two_view_draws(n, 300, rng)
        assert d.dtype == np.int32 and d.shape == (300, 8) and (d >= 0).all() and (d <= n - 1 - np.arange(8)).all()
        d[0] = 0                                    # always the front: every later front holds a back value
        d[1] = n - 1 - np.arange(8)                 # always the back
        d[2] = np.minimum(n - 1 - np.arange(8), 3)  # one position over and over
        d[3] = [n - 8] * 8                          # the largest draw the last list allows, eight times
        idx = api.two_view_resolve_draws(n, d)
        assert np.array_equal(idx, tm.resolve_draws_literal(n, d)), n
        assert all(len(set(row)) == 8 for row in idx.tolist())
    # n = 8: every set is a permutation of all matches
    assert (np.sort(api.two_view_resolve_draws(8, api.two_view_draws(8, 50, 1)), axis=1) == np.arange(8)).all()


def _problem(n1, n2, m12, iterations=5, sigma=1.0):
    k1, k2 = np.zeros((max(n1, 1), 2), np.float32), np.zeros((max(n2, 1), 2), np.float32)
    m = np.ascontiguousarray(m12, np.int32)
    p = capi.TwoViewProblem(C.sizeof(capi.TwoViewProblem), n1, n2, capi.ptr(k1), capi.ptr(k2), capi.ptr(m), 500.0, 500.0, 320.0, 240.0,
                            sigma, iterations)
    r = capi.TwoViewResult()
    r.struct_size = C.sizeof(capi.TwoViewResult)
    return p, r, (k1, k2, m)


def test_c_abi_surface_and_argument_checks_need_no_device():
    lib = capi.load()
    import re
    header = open(capi.LIB_PATH.replace("multi_orbslam3_amd/liborbgpu.so", "include/orbgpu.h")).read()
    declared = set(re.findall(r"^int\s+(orbi_\w+)\s*\(", header, flags=re.M))
    assert declared == set(capi.INITIALISER_SYMBOLS) == {"orbi_two_view_reconstruct", "orbi_two_view_resolve_draws"}
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).restype is C.c_int
    call = lambda p, d, r: lib.orbi_two_view_reconstruct(0, C.byref(p), capi.ptr(d) if d is not None else None, C.byref(r))
    d = np.zeros((5, 8), np.int32)
    # N = 7: no minimal set can be drawn
    p, r, keep = _problem(20, 20, [i if i < 7 else -1 for i in range(20)])
    assert call(p, d, r) == capi.ORBG_BAD_ARG
    p, r, keep = _problem(20, 20, np.arange(20))
    assert call(p, None, r) == capi.ORBG_BAD_ARG
    p.struct_size -= 4
    assert call(p, d, r) == capi.ORBG_BAD_ARG
    p, r, keep = _problem(20, 20, np.arange(20)); r.struct_size = 8
    assert call(p, d, r) == capi.ORBG_BAD_ARG
    p, r, keep = _problem(20, 20, np.arange(20), iterations=0)
    assert call(p, d, r) == capi.ORBG_BAD_ARG
    p, r, keep = _problem(20, 19, np.arange(20))            # a match outside keys2
    assert call(p, d, r) == capi.ORBG_BAD_ARG
    p, r, keep = _problem(20, 20, np.arange(20))
    bad = d.copy(); bad[4, 7] = 20 - 7                      # the eighth list has 13 entries
    assert call(p, bad, r) == capi.ORBG_BAD_ARG
    bad = d.copy(); bad[0, 0] = -1
    assert call(p, bad, r) == capi.ORBG_BAD_ARG
    p, r, keep = _problem(20, 20, np.arange(20), iterations=capi.TWO_VIEW_MAX_ITERATIONS + 1)
    assert call(p, np.zeros((capi.TWO_VIEW_MAX_ITERATIONS + 1, 8), np.int32), r) == capi.ORBG_CAP_EXCEEDED
    n = capi.TWO_VIEW_MAX_MATCHES + 1
    p, r, keep = _problem(n, n, np.arange(n))
    assert call(p, d, r) == capi.ORBG_CAP_EXCEEDED
    assert lib.orbi_two_view_resolve_draws(7, capi.ptr(d), 5, capi.ptr(d.copy())) == capi.ORBG_BAD_ARG
    # a valid call: the device is looked for last; without one there is no fallback
    p, r, keep = _problem(20, 20, np.arange(20))
    rc = call(p, d, r)
    assert rc == (capi.ORBG_OK if lib.orbg_device_count() > 0 else capi.ORBG_NO_DEVICE)


def test_no_gpu_means_no_reconstruction():
    if capi.load().orbg_device_count() > 0:
        pytest.skip("a GPU is present")
    sc, d, _, _ = tm.case("p63")
    with pytest.raises(capi.OrbGpuError) as e:
        api.TwoViewReconstruction(sc.cam, 1.0, 31).Reconstruct(sc.keys1, sc.keys2, sc.matches12, draws=d)
    assert e.value.code == capi.ORBG_NO_DEVICE


def test_float32_model_against_float64_on_the_committed_cases(capsys):
    """The figures the GPU tests lean on (docs/experiments.md, "TwoViewReconstruction"; `python tests/two_view_model.py` prints them).
    Measured: largest relative chi-square difference between the two models over the pairs with chi2 in [th / 2, 2 th] on the capped
    cases 6.06e-3, so delta = 4 x = 2.42e-2; 4 of their 660 hypotheses (0.61 %) hold a pair within delta of a gate.  The cap the issue
    sets: at most 1 % -- over the capped cases together, the smallest of which has 2 hypotheses."""
    worst = tm.measured_chi_difference()
    delta = 4 * worst
    tot = out = 0
    for n in tm.CAPPED:
        sc, d, a, b = tm.case(n)
        fl = tm.flagged(b, delta)
        tot += fl.size; out += int(fl.sum())
        # outside the flagged hypotheses the two models take every gate alike
        assert ((a.masks == b.masks).all(axis=2) | fl).all(), n
        assert np.array_equal(a.sets, b.sets) and a.masks.shape == (2, tm.CASES[n][2], tm.CASES[n][1])
    with capsys.disabled():
        print("\ntwo-view: chi2 float32 / float64 %.3e, delta %.3e, %d of %d hypotheses left out" % (worst, delta, out, tot))
    assert worst > 0, "no pair of the capped cases lies around a gate: the gates are not exercised"
    assert out <= 0.01 * tot, (out, tot)
    # and the float32 model alone reproduces the float64 model's decisions on every committed case
    for n in tm.CASES:
        if tm.CASES[n][1] == 8:
            continue                    # every set is a permutation of the same eight matches: the scores differ by rounding only
        sc, d, a, b = tm.case(n)
        assert (a.model, a.bestH, a.bestF, a.ok, a.best_motion) == (b.model, b.bestH, b.bestF, b.ok, b.best_motion), n
