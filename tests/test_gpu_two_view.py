"""TwoViewReconstruction on the GPU against tests/two_view_model.py.  Bit equality to the float32 model in T1, T2, the resolved sets
and, per hypothesis, the mask and the score; only hypotheses holding a (hypothesis, match) pair that the float64 model puts within
delta relative of a chi-square gate may be left out, delta = 4 x the models' own largest relative chi-square difference around the
gates (measured on the CPU, tests/test_two_view_cpu.py, docs/experiments.md).  The serial rules are checked by feeding the PRODUCT's
scores / nGood / parallax to the model's rules; R21, t21, vP3D and the matrices are compared with the float64 model."""
import numpy as np
import pytest

import two_view_model as tm
from multi_orbslam3_amd import api

pytestmark = pytest.mark.gpu

_RUNS, _FIG = {}, {}


def _figures():
    if not _FIG:
        _FIG["delta"] = 4 * tm.measured_chi_difference()
        _FIG.update({k: 4 * v for k, v in tm.measured_output_differences().items()})
    return _FIG


def _run(name):
    if name not in _RUNS:
        sc, d, a, b = tm.case(name)
        tv = api.TwoViewReconstruction(sc.cam, 1.0, tm.CASES[name][2])
        _RUNS[name] = tv.Reconstruct(sc.keys1, sc.keys2, sc.matches12, draws=d, per_hypothesis=True)
    return _RUNS[name]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(tm.CASES))
def test_hypotheses_equal_the_float32_model_to_the_bit(name):
    sc, d, a, b = tm.case(name)
    g = _run(name)
    kind, N, H, seed, kw = tm.CASES[name]
    assert g.n_matches == N and g.hyp_scores.shape == (2, H) and g.hyp_masks.shape == (2, H, N) and g.hyp_sets.shape == (H, 8)
    assert len(sc.keys1) != len(sc.keys2) and not np.array_equal(a.i1, np.arange(N))      # match index != keypoint index, n1 != n2
    assert np.array_equal(_bits(g.T1), _bits(a.T1)) and np.array_equal(_bits(g.T2), _bits(a.T2))
    assert np.array_equal(g.hyp_sets, a.sets)
    left_out = tm.flagged(b, _figures()["delta"])
    bad_mask = (g.hyp_masks != a.masks).any(axis=2)
    bad_score = _bits(g.hyp_scores) != _bits(a.scores)
    print("%s: %d hypotheses, %d may be left out, %d masks / %d scores differ" % (name, left_out.size, left_out.sum(), bad_mask.sum(), bad_score.sum()))
    assert not (bad_mask & ~left_out).any(), np.argwhere(bad_mask & ~left_out)[:5].tolist()
    assert not (bad_score & ~left_out).any(), np.argwhere(bad_score & ~left_out)[:5].tolist()


def test_left_out_hypotheses_stay_inside_the_cap():
    delta = _figures()["delta"]
    tot = out = 0
    for name in tm.CAPPED:
        fl = tm.flagged(tm.case(name)[3], delta)
        tot += fl.size; out += int(fl.sum())
    assert out <= 0.01 * tot, (out, tot)


@pytest.mark.parametrize("name", list(tm.CASES))
def test_serial_rules_on_the_products_own_figures(name):
    """The product's per-hypothesis scores through the model's serial rule, its per-motion nGood / parallax through the model's final
    decision: best iterations, the model chosen, the success flag and the motion returned must be the product's."""
    sc, d, a, b = tm.case(name)
    g = _run(name)
    SH, bH = tm.serial_best(g.hyp_scores[0])
    SF, bF = tm.serial_best(g.hyp_scores[1])
    assert (g.best_iteration_H, g.best_iteration_F) == (bH, bF)
    assert _bits(g.SH) == _bits(SH) and _bits(g.SF) == _bits(SF)
    model = tm.choose_model(np.float32(SH), np.float32(SF))
    assert g.model == model
    if model == 1:
        assert np.array_equal(_bits(g.H21), _bits(g.hyp_models[0, bH]))
    if bF >= 0:
        assert np.array_equal(_bits(g.F21), _bits(g.hyp_models[1, bF]))
    inl = g.hyp_masks[0, bH] if model == 1 else g.hyp_masks[1, bF]
    assert g.n_inliers == int(inl.sum())
    if g.h_degenerate or model == 0:
        assert g.n_motions == 0 and not g.ok
        return
    assert g.n_motions == (8 if model == 1 else 4)
    k = (tm.decide_H if model == 1 else tm.decide_F)(g.motion_nGood, g.motion_parallax, g.n_inliers)
    assert g.best_motion == k and g.ok == (k >= 0)
    if g.ok:
        assert np.array_equal(_bits(g.R21), _bits(g.motion_R[k])) and np.array_equal(_bits(g.t21), _bits(g.motion_t[k]))
        assert not g.vbTriangulated[sc.matches12 < 0].any() and not g.vP3D[sc.matches12 < 0].any()
        assert g.vP3D.shape == (len(sc.keys1), 3) and g.vbTriangulated.shape == (len(sc.keys1),)
    else:
        assert not g.vbTriangulated.any() and not g.vP3D.any() and not g.R21.any()


@pytest.mark.parametrize("name", ["wide", "plane"])
def test_outputs_against_the_float64_model(name):
    """Tolerance: 4 x the float32-against-float64 difference of the model itself on the committed cases (docs/experiments.md)."""
    sc, d, a, b = tm.case(name)
    g = _run(name)
    fig = _figures()
    assert g.ok and b.ok and g.model == b.model and g.best_motion == b.best_motion
    assert (g.best_iteration_H, g.best_iteration_F) == (b.bestH, b.bestF)
    dM = max(np.abs(tm.unit(g.H21) - tm.unit(b.H21[b.bestH])).max(), np.abs(tm.unit(g.F21) - tm.unit(b.F21[b.bestF])).max())
    dR, dt = np.abs(g.R21 - b.R21).max(), np.abs(g.t21 - b.t21).max()
    both = g.vbTriangulated & b.vbTriangulated
    dP = np.abs(g.vP3D - b.vP3D)[both].max()
    print("%s: |M| %.3g (%.3g) |R| %.3g (%.3g) |t| %.3g (%.3g) |P| %.3g (%.3g)" % (name, dM, fig["M"], dR, fig["R"], dt, fig["t"], dP, fig["P"]))
    assert dM <= fig["M"] and dR <= fig["R"] and dt <= fig["t"] and dP <= fig["P"]
    assert np.array_equal(g.motion_nGood, b.motion_nGood)
    assert np.array_equal(g.vbTriangulated, b.vbTriangulated)
    assert both.sum() >= 0.8 * tm.CASES[name][1]


def _collinear_case():
    """The first set's eight matches lie on one line in both images (a rank-deficient design matrix: H is singular or NaN) and are
    moved to the front so that iteration 0 draws exactly them."""
    sc = tm.scene("3d", 100, 31, n_extra1=5, n_extra2=9)
    k1, k2, m12 = sc.keys1.copy(), sc.keys2.copy(), sc.matches12
    i1 = np.nonzero(m12 >= 0)[0][:8]
    for j, i in enumerate(i1):
        k1[i] = (100 + 32 * j, 50 + 16 * j)
        k2[m12[i]] = (120 + 32 * j, 60 + 16 * j)
    d = tm.case_draws(100, 33, 31)
    d[0] = [0, 1, 2, 3, 4, 5, 6, 7]      # positions not yet overwritten: matches 0 .. 7
    return k1, k2, m12, sc.cam, d


def test_a_collinear_set_never_wins_and_does_not_fault():
    k1, k2, m12, cam, d = _collinear_case()
    sets = api.two_view_resolve_draws(100, d)
    assert sorted(sets[0].tolist()) == list(range(8))
    g = api.TwoViewReconstruction(cam, 1.0, 33).Reconstruct(k1, k2, m12, draws=d, per_hypothesis=True)
    a = tm.reconstruct(k1, k2, m12, cam, 1.0, 33, d, np.float32)
    assert g.best_iteration_H != 0
    s = g.hyp_scores[0, 0]
    assert np.isnan(s) or s < g.SH
    assert np.array_equal(np.isnan(g.hyp_scores), np.isnan(a.scores))
    assert (g.best_iteration_H, g.best_iteration_F, g.model, g.ok) == (a.bestH, a.bestF, a.model, a.ok)
    # an all-collinear problem: every set is degenerate, the call answers without a fault whatever it decides
    n = 64
    kk = np.stack([100 + 4.0 * np.arange(n), 50 + 2.0 * np.arange(n)], axis=1).astype(np.float32)
    g = api.TwoViewReconstruction(cam, 1.0, 32).Reconstruct(kk, kk + np.float32(3), np.arange(n), draws=tm.case_draws(n, 32, 2))
    assert g.model in (0, 1, 2) and g.n_matches == n


def test_identical_matches_score_zero_and_return_false():
    """Every keypoint of both frames at one position: Normalize divides by a zero mean deviation, every hypothesis is NaN, no score
    is above zero, SH + SF == 0 and the call returns false (:111) without running CheckRT."""
    n = 65
    k = np.tile(np.array([[123.25, 77.5]], np.float32), (n, 1))
    g = api.TwoViewReconstruction(tm.CAM, 1.0, 33).Reconstruct(k, k, np.arange(n), draws=tm.case_draws(n, 33, 3), per_hypothesis=True)
    assert not g.ok and g.model == 0 and g.n_motions == 0
    assert g.SH == 0 and g.SF == 0 and g.best_iteration_H == -1 and g.best_iteration_F == -1
    assert not (g.hyp_scores > 0).any()
    assert not g.vbTriangulated.any() and not g.vP3D.any()


def test_two_runs_give_identical_bytes():
    sc, d, a, b = tm.case("wide")
    tv = api.TwoViewReconstruction(sc.cam, 1.0, tm.CASES["wide"][2])
    g1 = tv.Reconstruct(sc.keys1, sc.keys2, sc.matches12, draws=d, per_hypothesis=True)
    g2 = tv.Reconstruct(sc.keys1, sc.keys2, sc.matches12, draws=d, per_hypothesis=True)
    for f in ("hyp_scores", "hyp_models", "hyp_masks", "hyp_sets", "H21", "F21", "R21", "t21", "vP3D", "vbTriangulated", "motion_nGood",
              "motion_parallax", "motion_R", "motion_t", "T1", "T2"):
        assert getattr(g1, f).tobytes() == getattr(g2, f).tobytes(), f
    assert (g1.ok, g1.model, g1.best_motion, g1.SH.tobytes(), g1.SF.tobytes()) == (g2.ok, g2.model, g2.best_motion, g2.SH.tobytes(), g2.SF.tobytes())


def test_own_generator_and_defaults():
    """Without `draws` the object draws from its own seeded generator: two objects with one seed agree, and 200 iterations are the default."""
    sc, d, a, b = tm.case("wide")
    r1 = api.TwoViewReconstruction(sc.cam, seed=4).Reconstruct(sc.keys1, sc.keys2, sc.matches12)
    r2 = api.TwoViewReconstruction(sc.cam, seed=4).Reconstruct(sc.keys1, sc.keys2, sc.matches12)
    assert r1.ok and r1.model == 2 and r1.R21.tobytes() == r2.R21.tobytes() and r1.vP3D.tobytes() == r2.vP3D.tobytes()
