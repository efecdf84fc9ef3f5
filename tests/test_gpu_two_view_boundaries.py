"""TwoViewReconstruction past one LDS tile of 256 matches, at both caps, through both branches of CheckRT and around its rank switch
(the cases of tests/two_view_boundary_cases.py; their conditions, for the models alone, in tests/test_two_view_boundaries_cpu.py).
The checker is the numpy model in float32; the float64 model says which comparisons are not binding:
  near pair   a (model, hypothesis, match) whose float64 chi-square lies within delta relative of its gate.  Only these mask bits may
              differ; a hypothesis without one has the float32 model's score to the bit, the others a bound per near direction.
  open match  for a motion hypothesis: the two models give it different CheckRT gate records, or a float64 gate quantity lies within
              its margin of the gate.  nGood may differ by their number; the parallax is compared where there are none.
Every figure is printed before it is asserted (-s)."""
import threading

import numpy as np
import pytest

import two_view_boundary_cases as bc
import two_view_model as tm
from multi_orbslam3_amd import api

pytestmark = pytest.mark.gpu

FIELDS = ("H21", "F21", "R21", "t21", "vP3D", "vbTriangulated", "motion_nGood", "motion_parallax", "motion_R", "motion_t", "T1", "T2")
HYP_FIELDS = ("hyp_scores", "hyp_models", "hyp_masks", "hyp_sets")
SCALARS = ("ok", "model", "best_motion", "n_matches", "n_inliers", "n_motions", "h_degenerate", "best_iteration_H", "best_iteration_F")
ULP_CASES = ()          # cases whose parallax needed the one float32 ulp the double acos may cost: none on the MI355X
_RUNS = {}


def _reconstruct(name, per_hypothesis=True):
    sc, d, a, b = bc.tie_case()[:4] if name == "tie" else bc.case(name)
    kind, N, H, seed, kw, cam, sigma = bc.TIE if name == "tie" else bc.spec(name)
    return api.TwoViewReconstruction(cam, sigma, H).Reconstruct(sc.keys1, sc.keys2, sc.matches12, draws=d, per_hypothesis=per_hypothesis)


def _run(name):
    if name not in _RUNS:
        _RUNS[name] = _reconstruct(name)
    return _RUNS[name]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _same_bytes(g1, g2, hyp=True):
    for f in FIELDS + (HYP_FIELDS if hyp else ()):
        assert getattr(g1, f).tobytes() == getattr(g2, f).tobytes(), f
    assert tuple(getattr(g1, f) for f in SCALARS) == tuple(getattr(g2, f) for f in SCALARS)
    assert (g1.SH.tobytes(), g1.SF.tobytes()) == (g2.SH.tobytes(), g2.SF.tobytes())


def _check(name, g):
    """The assertions every call has to pass (module docstring)."""
    sc, d, a, b = bc.case(name)
    kind, N, H, seed, kw, cam, sigma = bc.spec(name)
    near, nd = bc.near(name)
    delta = bc.delta()
    n1 = len(sc.keys1)
    assert g.n_matches == N and g.hyp_scores.shape == (2, H) and g.hyp_masks.shape == (2, H, N) and g.hyp_sets.shape == (H, 8)
    assert g.vP3D.shape == (n1, 3) and g.vbTriangulated.shape == (n1,)
    # ---- to the bit: T1, T2, the sets; every mask bit outside the near pairs
    assert np.array_equal(_bits(g.T1), _bits(a.T1)) and np.array_equal(_bits(g.T2), _bits(a.T2))
    assert np.array_equal(g.hyp_sets, a.sets)
    dm = g.hyp_masks != a.masks
    print("%s: mask bits compared %d, left out %d, of those different %d" % (name, int((~near).sum()), int(near.sum()), int(dm.sum())))
    assert not (dm & ~near).any(), np.argwhere(dm & ~near)[:5].tolist()
    # ---- scores: to the bit without a near pair, else within what the near directions can move
    free = ~near.any(axis=2)
    ds = (_bits(g.hyp_scores) != _bits(a.scores)) & ~(np.isnan(g.hyp_scores) & np.isnan(a.scores))
    th = np.array([tm.TH_H, tm.TH_F], np.float64)[:, None]
    with np.errstate(all="ignore"):
        bound = nd.sum(axis=(1, 3)) * (np.float64(tm.TH_SCORE) - th + delta * th) + 2.0 * N * 2.0 ** -24 * np.abs(a.scores.astype(np.float64))
        diff = np.abs(g.hyp_scores.astype(np.float64) - a.scores.astype(np.float64))
    print("%s: hypotheses compared to the bit H %d F %d of %d, scores that differ %d (%d among the bounded)" %
          (name, int(free[0].sum()), int(free[1].sum()), H, int(ds.sum()), int((ds & ~free).sum())))
    assert not (ds & free).any(), np.argwhere(ds & free)[:5].tolist()
    assert (diff[ds] <= bound[ds]).all()
    for k in range(2):
        assert free[k].any() or k in bc.NOTHING_TO_THE_BIT.get(name, ()), "no hypothesis of model %d was compared to the bit" % k
    # ---- the serial rule on the product's own scores, and against the model's rows
    SH, bH = tm.serial_best(g.hyp_scores[0])
    SF, bF = tm.serial_best(g.hyp_scores[1])
    assert (g.best_iteration_H, g.best_iteration_F) == (bH, bF) and _bits(g.SH) == _bits(SH) and _bits(g.SF) == _bits(SF)
    assert g.model == tm.choose_model(np.float32(SH), np.float32(SF))
    nH = int(near[0, a.bestH].sum()) if a.bestH >= 0 else 0
    nF = int(near[1, a.bestF].sum()) if a.bestF >= 0 else 0
    if nH == 0 or not ds[0].any():
        assert g.best_iteration_H == a.bestH
    if nF == 0 or not ds[1].any():
        assert g.best_iteration_F == a.bestF
    if (nH == 0 and nF == 0) or not ds.any():
        assert g.model == a.model
    rows_equal = (g.best_iteration_H, g.best_iteration_F, g.model) == (a.bestH, a.bestF, a.model)
    inl_g = None if g.model == 0 else (g.hyp_masks[0, bH] if g.model == 1 else g.hyp_masks[1, bF])
    assert g.n_inliers == (0 if inl_g is None else int(inl_g.sum()))
    if rows_equal:
        assert abs(g.n_inliers - a.n_inliers) <= (nH if a.model == 1 else nF)
    # ---- CheckRT.  Where a near pair moved the winning row or its mask, the float32 model runs on the product's row
    ref, op = a, bc.open_matches(name)
    if not rows_equal or (inl_g is not None and not np.array_equal(inl_g, a.masks[0, a.bestH] if a.model == 1 else a.masks[1, a.bestF])):
        ref = tm.Out(a)
        ref.update(tm.finish(tm.Out(a, masks=g.hyp_masks), g.hyp_scores, cam, sigma, n1, np.float32))
        op = tm.open_matches(ref, b, bc.rt_margins(name)[0])
        print("%s: a near pair moved the winning row or its mask; CheckRT of the float32 model on the product's row" % name)
    assert (g.n_motions, g.h_degenerate) == (ref.n_motions, ref.h_degenerate)
    nopen = op.sum(axis=1)
    dn = np.abs(g.motion_nGood.astype(np.int64) - ref.motion_nGood)
    ulps = np.abs(_bits(g.motion_parallax).astype(np.int64) - _bits(ref.motion_parallax).astype(np.int64))
    binding = (dn == 0) & (nopen == 0)
    print("%s: nGood %s (model %s), open matches %s; parallax %s, compared %d motions (%d see an off-by-one rank), ulps %s" %
          (name, g.motion_nGood.tolist(), ref.motion_nGood.tolist(), nopen.tolist(), g.motion_parallax.tolist(), int(binding.sum()),
           int((binding & bc.rank_visible(name)).sum()) if ref is a else -1, ulps.tolist()))
    assert (dn <= nopen).all()
    assert (ulps[binding] <= (1 if name in ULP_CASES else 0)).all()
    # ---- the decision is the float32 model's on its own figures
    assert (g.best_motion, g.ok) == (ref.best_motion, ref.ok)
    assert not g.vbTriangulated[sc.matches12 < 0].any() and not g.vP3D[sc.matches12 < 0].any()
    if not g.ok:
        assert not g.vbTriangulated.any() and not g.vP3D.any() and not g.R21.any() and not g.t21.any()
        return
    k = g.best_motion
    closed = ~op[k]
    wrote, tri = g.vP3D[a.i1].any(axis=1), g.vbTriangulated[a.i1]
    assert np.array_equal(wrote[closed], ref.counted[k][closed]) and np.array_equal(tri[closed], ref.good[k][closed])
    assert not (tri & ~wrote).any()
    assert b.ok and b.best_motion == k
    tol = bc.output_tolerances()
    both = g.vbTriangulated & b.vbTriangulated
    dR, dt, dP = np.abs(g.R21 - b.R21).max(), np.abs(g.t21 - b.t21).max(), np.abs(g.vP3D - b.vP3D)[both].max()
    print("%s: against the float64 model |R| %.3g (%.3g) |t| %.3g (%.3g) |P| %.3g (%.3g) over %d points" %
          (name, dR, tol["R"], dt, tol["t"], dP, tol["P"], int(both.sum())))
    assert dR <= tol["R"] and dt <= tol["t"] and dP <= tol["P"]
    assert both.sum() >= 0.8 * ref.motion_nGood[k]


@pytest.mark.parametrize("name", list(bc.CASES))
def test_family_case_against_the_models(name):
    g = _run(name)
    sc, d, a, b = bc.case(name)
    _check(name, g)
    fam = name[0]
    if fam == "W":
        assert g.ok and g.model == 2 and g.n_motions == 4
    if fam == "Q":
        assert g.model == 1 and g.n_motions == 8 and g.ok == (name != bc.Q_REFUSED)
        if g.ok:
            assert g.best_motion == 0
    if fam == "R":
        N = bc.CASES[name][1]
        assert g.motion_nGood.tolist() == [0, N, 0, 0] and g.ok == (N >= 50)
        assert g.motion_parallax.tobytes() == a.motion_parallax.tobytes()


def test_equal_best_scores_in_two_lanes_return_the_lower_row():
    """Phase C reduces the lanes' bests with `c == s && ci < bi`: rows 37 / 38 sit in lanes 5 / 6 and are met before rows 8 / 9 in
    lanes 8 / 9, which hold the same sets and so the same scores."""
    sc, d, a, b, orig = bc.tie_case()
    g = _run("tie")
    (h0, h1), (f0, f1) = bc.TIE_ROWS["H"], bc.TIE_ROWS["F"]
    assert np.array_equal(g.hyp_sets, a.sets) and np.array_equal(g.hyp_sets[h0], g.hyp_sets[h1]) and np.array_equal(g.hyp_sets[f0], g.hyp_sets[f1])
    assert _bits(g.hyp_scores[0, h0]) == _bits(g.hyp_scores[0, h1]) and _bits(g.hyp_scores[1, f0]) == _bits(g.hyp_scores[1, f1])
    assert tm.serial_best(g.hyp_scores[0])[1] == h0 and tm.serial_best(g.hyp_scores[1])[1] == f0
    print("tie: best rows H %d F %d (the copies: %d / %d, %d / %d; before the copies: %s)" % (g.best_iteration_H, g.best_iteration_F, h0, h1, f0, f1, orig))
    assert (g.best_iteration_H, g.best_iteration_F) == (h0, f0) == (a.bestH, a.bestF)
    assert _bits(g.SH) == _bits(g.hyp_scores[0, h0]) and _bits(g.SF) == _bits(g.hyp_scores[1, f0])
    assert np.array_equal(_bits(g.F21), _bits(g.hyp_models[1, f0])) and (g.model, g.ok, g.best_motion) == (a.model, a.ok, a.best_motion)


def test_large_small_large_on_one_thread():
    """The work area is per thread and only grows, the tickets are zeroed once: 8192 matches, then 8 matches and one iteration, then
    513 matches and 65 iterations, then the first problem again."""
    names = ("W8192_33", "S8", "W513_65", "W8192_33")
    res = [_reconstruct(n) for n in names]
    for n, g in zip(names, res):
        _check(n, g)
    _same_bytes(res[0], res[3])
    _same_bytes(res[0], _run("W8192_33"))
    _same_bytes(res[2], _run("W513_65"))


def test_two_threads_at_once():
    names = ("W513_65", "W1025_33")
    single = [_run(n) for n in names]
    for n, g in zip(names, single):
        _check(n, g)
    out, err = [[], []], []

    def work(t):
        try:
            for _ in range(10):
                out[t].append(_reconstruct(names[t]))
        except Exception as e:       # noqa: BLE001
            err.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for t in range(2):
        assert len(out[t]) == 10
        for g in out[t]:
            _same_bytes(g, single[t])


@pytest.mark.parametrize("name", ["W513_65", "Q513_s105"])
def test_without_the_per_hypothesis_outputs(name):
    g0 = _run(name)
    g = _reconstruct(name, per_hypothesis=False)
    assert g.hyp_scores is None and g.hyp_models is None and g.hyp_masks is None and g.hyp_sets is None
    _same_bytes(g, g0, hyp=False)
