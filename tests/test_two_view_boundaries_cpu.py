"""The conditions tests/test_gpu_two_view_boundaries.py leans on, asserted for the two numpy models alone (no device): what each
family of tests/two_view_boundary_cases.py chooses and decides, that the two precisions agree outside the pairs the comparison may
leave out, and that those stay under their caps -- so that the comparison cannot hide a failure behind them."""
import numpy as np
import pytest

import two_view_boundary_cases as bc
import two_view_model as tm


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("name", list(bc.CASES))
def test_family_conditions(name, capsys):
    sc, d, a, b = bc.case(name)
    kind, N, H, seed, kw, cam, sigma = bc.CASES[name]
    fam = name[0]
    near, _ = bc.near(name)
    share = float(near.mean())
    op = bc.open_matches(name)
    m, w, cnt = bc.rt_margins(name)
    with capsys.disabled():
        print("\n%s: near pairs %d of %d (%.4f %%); model %d ok %s motion %d nGood %s; gate-record differences %d, open %s of %d inliers; "
              "margins e %.2e cos %.2e z %.2e" % (name, near.sum(), near.size, 100 * share, a.model, a.ok, a.best_motion, a.motion_nGood.tolist(),
                                                  int((a.gates != b.gates).sum()), op.sum(axis=1).tolist(), a.n_inliers, m["e"], m["cos"], m["z"]))
    assert a.N == N and a.masks.shape == (2, H, N) and len(sc.keys1) == N + 37 and len(sc.keys2) == N + 71
    # the two precisions: the same sets, every mask bit outside the near pairs, the same rows, model, decision
    assert np.array_equal(a.sets, b.sets)
    assert not ((a.masks != b.masks) & ~near).any()
    assert (a.model, a.bestH, a.bestF, a.ok, a.best_motion, a.n_motions) == (b.model, b.bestH, b.bestF, b.ok, b.best_motion, b.n_motions)
    assert tm.same_rt(a, b)
    assert share <= bc.NEAR_CAP[fam], share
    # hypotheses without a near pair exist in both models, so that some score is compared to the bit -- but for the listed exceptions
    none_free = tuple(k for k in range(2) if not (~near[k].any(axis=1)).any())
    assert none_free == bc.NOTHING_TO_THE_BIT.get(name, ())
    assert op.shape == (a.n_motions, N)
    assert (op.sum(axis=1) <= bc.OPEN_CAP * a.n_inliers).all(), (op.sum(axis=1).tolist(), a.n_inliers)
    differ = np.abs(a.motion_nGood.astype(int) - b.motion_nGood) <= op.sum(axis=1)
    assert differ.all()
    if fam == "P":
        assert a.model == 2 and a.n_motions == 4 and not a.ok         # an F fitted to a plane: no motion stands out
    if fam == "W":
        assert a.model == 2 and a.n_motions == 4 and a.ok and b.ok
        assert np.array_equal(a.motion_nGood, b.motion_nGood) and np.array_equal(a.gates, b.gates)
        assert 0.0029 <= share <= 0.0067
    if fam == "Q":
        assert a.model == 1 and a.n_motions == 8 and 0.0145 <= share <= 0.0204
        ng = a.motion_nGood.tolist()
        if name == bc.Q_REFUSED:
            assert not a.ok and ng[:2] == [460, 353] and ng[1] >= 0.75 * ng[0] and ng[0] > 0.9 * a.n_inliers and a.motion_parallax[0] >= 1
        else:
            assert a.ok and a.best_motion == 0
            assert ng[:3] == ([491, 326, 288] if N == 513 else [7792, 5259, 4451])
        if N == 8192:
            assert int((a.gates != b.gates).sum()) == 2 and int((a.gates[2] != b.gates[2]).sum()) == 2
        else:
            assert np.array_equal(a.gates, b.gates)
    if fam == "R":
        assert a.model == 2 and a.motion_nGood.tolist() == [0, N, 0, 0] == b.motion_nGood.tolist() and a.n_inliers == N
        assert a.ok == (N >= 50) and 4.5 <= a.motion_parallax[1] <= 5.6 and not op.any()


def test_near_pairs_of_the_families_together():
    tot = {f: [0, 0] for f in bc.FAMILY}
    for f, names in bc.FAMILY.items():
        for n in names:
            near, nd = bc.near(n)
            assert np.array_equal(near, tm.near_pairs(bc.case(n)[3], bc.delta())) and nd.shape == (2, 2) + near.shape[1:]
            tot[f][0] += int(near.sum()); tot[f][1] += near.size
    assert abs(bc.delta() - 2.424e-2) < 1e-5
    assert tot["P"][1] == 1151106 and tot["P"][0] <= 0.0002 * tot["P"][1]
    assert 0.004 <= tot["W"][0] / tot["W"][1] <= 0.0055


@pytest.mark.parametrize("name", list(bc.CASES))
def test_the_rank_selection_is_visible_in_the_parallax(name):
    """sorted[min(50, nGood - 1)]: the parallax of the ranks beside `want` must differ from the one at `want` by more than the one
    float32 ulp the comparison may allow -- otherwise an off-by-one in the selection could not be seen (bc.rank_visible).  It holds
    for the motion with the most counted matches of every W, Q and R case, whose parallax the GPU test compares to the bit."""
    sc, d, a, b = bc.case(name)
    seen = bc.rank_visible(name)
    k = int(np.argmax(a.motion_nGood)) if a.n_motions else -1
    if name[0] in "WQR":
        assert seen[k] and not bc.open_matches(name)[k].any()
        lo, at, hi = tm.rank_neighbours(a, k)
        assert at.tobytes() == a.motion_parallax[k].tobytes()
        assert all(x is None or abs(float(x) - float(at)) > _ulp(at) for x in (lo, hi))
    if name[0] == "R":
        N = bc.CASES[name][1]
        lo, at, hi = tm.rank_neighbours(a, 1)
        assert (hi is None) == (N <= 51) and lo is not None       # want = N - 1 up to 51 matches, 50 from there on


def test_the_equal_score_scene():
    sc, d, a, b, (oH, oF) = bc.tie_case()
    (h0, h1), (f0, f1) = bc.TIE_ROWS["H"], bc.TIE_ROWS["F"]
    assert np.array_equal(d[h0], d[h1]) and np.array_equal(d[f0], d[f1]) and not np.array_equal(d[h0], d[f0])
    assert a.scores[0, h0].tobytes() == a.scores[0, h1].tobytes() and a.scores[1, f0].tobytes() == a.scores[1, f1].tobytes()
    assert tm.serial_best(a.scores[0]) == (a.scores[0, h0], h0) and tm.serial_best(a.scores[1]) == (a.scores[1, f0], f0)
    assert (a.bestH, a.bestF) == (h0, f0) == (b.bestH, b.bestF)
    # no row exceeds the copies' scores (an original best row above its copies keeps its own, equal, score), no lower row reaches them,
    # and the copies sit where the workgroup's reduction meets the higher row first
    assert (a.scores[0] <= a.scores[0, h0]).all() and (a.scores[1] <= a.scores[1, f0]).all()
    assert (a.scores[0, :h0] < a.scores[0, h0]).all() and (a.scores[1, :f0] < a.scores[1, f0]).all()
    assert h1 % 32 < h0 % 32 and f1 % 32 < f0 % 32 and h1 > h0 and f1 > f0


def test_the_small_call_between_two_large_ones():
    sc, d, a, b = bc.case("S8")
    assert a.N == 8 and a.masks.shape == (2, 1, 8) and not a.ok
