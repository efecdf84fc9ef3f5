"""What tests/test_gpu_extractor_boundaries.py rests on, checked without a device: the oracle alone on the inputs of
tests/extractor_boundary_cases.py, and the reference's arithmetic (per-level split, 30-pixel tiling, roots of the quad-tree) restated.
Every Ref asserts that the oracle ran to the end on its input."""
import numpy as np
import pytest

import extractor_boundary_cases as xb
from oracle import binding as ob


# ------------------------------------------------------------------ 1. dot images

@pytest.mark.parametrize("K", xb.DOT_K)
def test_dot_images_have_exactly_k_candidates_at_level_0_and_no_other_level_near_the_limit(K):
    r = xb.dot_ref(K)
    assert r.n_cands[0] == K and r.n_cands[1] in (887, 888) and r.n_cands[2:] == [28, 0, 0, 0, 0, 0]
    assert len(r.kps) == 426 and r.per_level == [217, 181, 28, 0, 0, 0, 0, 0]
    assert r.quota == [217, 181, 151, 126, 105, 87, 73, 60]
    # level 0 is the only level that can overflow, and it does so by its candidate count alone: 217 nodes in a list of 876
    assert r.overflowing_levels() == ([0] if K > xb.KEY_CAP else [])
    assert all(r.per_level[l] <= min(4 * r.quota[l] + 8, xb.LIST_CAP) for l in range(8))
    assert xb.expected_redos(r) == int(K == 4097)


def test_dot_amplitude_12_is_the_one_that_puts_level_0_alone_at_the_limit():
    """A dot of +8 leaves the other levels empty; a dot of value 255 (+195) puts level 1 over the limit as well (4165) and level 2
    within a hundred of it (4008)."""
    weak = xb.Ref(xb.dot_image(4096, amp=8), xb.DOT_FEATURES)
    assert weak.n_cands == [4096, 0, 0, 0, 0, 0, 0, 0]
    strong = xb.Ref(xb.dot_image(4096, amp=195), xb.DOT_FEATURES)
    assert strong.n_cands[0] == 4096 and strong.n_cands[1] > xb.KEY_CAP and strong.n_cands[2] > 4000


# ------------------------------------------------------------------ 2. the per-level split

@pytest.mark.parametrize("nf", xb.SMALL_FEATURES + (100, 1000, 2000, 2346, 2347, 2350, 2351, 3500))
def test_per_level_split_is_the_constructors_formula(nf):
    quota = xb.features_per_level(nf)
    assert quota == [int(v) for v in ob.Extractor(n_features=nf).tables()[4]]
    assert sum(quota) >= nf and min(quota) >= 0
    if nf in xb.SMALL_SPLITS:
        assert quota == xb.SMALL_SPLITS[nf]
    if nf <= 9:
        assert 0 in quota                                        # every small count has a level whose target is 0
    expect0 = {2000: 434, 3500: 760, 2346: 509, 2347: 510, 2350: 510, 2351: 511}
    if nf in expect0:
        assert quota[0] == expect0[nf]
    # 4 N + 8 against the node list: N = 510 is the last target the device trees take
    assert xb.host_from_the_start(nf) == (nf >= 2351)


def test_the_node_list_edge_case_reaches_its_target_at_level_0():
    img = xb.dot_image(xb.NODE_EDGE_DOTS)
    for nf, n0 in xb.NODE_EDGE:
        r = xb.Ref(img, nf)
        assert r.quota[0] == n0 and 4 * n0 + 8 == (2048 if n0 == 510 else 2052)
        assert r.n_cands == [4000, 839, 28, 0, 0, 0, 0, 0]
        assert r.per_level[0] >= n0 and r.per_level[0] <= xb.LIST_CAP                # the tree grows to N nodes: enough isolated candidates
        if n0 == 510:
            assert r.overflowing_levels() == [] and not xb.host_from_the_start(nf)
        else:
            assert r.overflowing_levels() == [0] and xb.host_from_the_start(nf)


# ------------------------------------------------------------------ 3. small feature counts

@pytest.mark.parametrize("W,H", xb.SMALL_SHAPES)
def test_small_feature_counts_one_unconditional_pass_per_level(W, H):
    """A level whose target is 0 (or below its root count) still makes the reference's one pass: every root with more than one candidate
    splits once, so the level ends with up to 4 nodes per root.  One root at 640 x 480: at most 4 nodes in a region of at least 8, the
    frame stays on the device.  Four roots at 1241 x 376 (the FAST area is 3.5 times as wide as high at every level): 13 to 15 nodes,
    more than the 8 / 12 / 16 of a target of 0 / 1 / 2, so every one of these frames goes to the host."""
    sizes = xb.level_sizes(W, H)
    roots = [xb.n_roots(w, h) for w, h in sizes]
    assert roots == ([1] * 8 if W == 640 else [4] * 8)
    for nf in xb.SMALL_FEATURES:
        for side in (0, 1):
            r = xb.small_ref(W, H, nf, side)
            assert [r.ex.level(l).shape for l in range(8)] == [(h, w) for w, h in sizes]
            assert min(r.n_cands) > 30 and max(r.n_cands) <= xb.KEY_CAP
            assert all(1 <= r.per_level[l] <= 4 * roots[l] for l in range(8))
            assert len(r.kps) <= 2 * nf + 256                                          # what the Python wrapper sizes its outputs for
            over = r.overflowing_levels()
            if W == 640:
                assert r.per_level == [4] * 8 and over == []
            else:
                zero = [l for l in range(8) if r.quota[l] == 0]
                assert zero and all(r.per_level[l] > 8 for l in zero) and set(zero) <= set(over)
        assert xb.expected_redos(xb.small_ref(W, H, nf, 0), xb.small_ref(W, H, nf, 1)) == int(W != 640)


# ------------------------------------------------------------------ 4. large images

def _cells(w, h):
    n_cols, n_rows, _, _ = xb.cell_grid(w, h)
    return n_cols * n_rows


def test_cell_counts_of_the_large_images():
    assert _cells(1280, 720) == 41 * 22 == 902                                       # the largest image elsewhere in the suite
    for (W, H), want in xb.LARGE_CELLS.items():
        sizes = xb.level_sizes(W, H)
        assert tuple(_cells(w, h) for w, h in sizes[:len(want)]) == want
    s = xb.level_sizes(1920, 1080)
    assert [xb.cells_per_thread(_cells(w, h)) for w, h in s[:4]] == [9, 6, 4, 3]
    assert xb.cells_per_thread(_cells(992, 992)) == xb.SPEC_CELLS and _cells(992, 992) == 32 * 32
    assert xb.cells_per_thread(_cells(1022, 1022)) == xb.SPEC_CELLS + 1 and _cells(1022, 1022) == 33 * 33


@pytest.mark.parametrize("W,H", xb.LARGE_SHAPES)
def test_large_images_stay_on_the_device_and_fill_the_cells_behind_the_speculative_fetch(W, H):
    r = xb.large_ref(W, H)
    sizes = xb.level_sizes(W, H)
    assert [r.ex.level(l).shape for l in range(8)] == [(h, w) for w, h in sizes]
    assert max(r.n_cands) <= xb.KEY_CAP and min(r.n_cands) > 300 and r.overflowing_levels() == []
    assert r.quota[0] == 434 and r.per_level[0] >= 434                                # the level-0 tree reaches its target
    beyond, fullest = [], 0
    for l in range(8):
        w, h = sizes[l]
        cell = xb.cell_of_candidates(r.cands[l], w, h)
        assert (np.diff(cell) >= 0).all() and cell.min() >= 0 and cell.max() < _cells(w, h)      # candidate order is cell-major order
        cpt = xb.cells_per_thread(_cells(w, h))
        beyond.append(int((cell % cpt >= xb.SPEC_CELLS).sum()))                    # candidates of a thread's fifth and later cells
        fullest = max(fullest, int(np.bincount(cell).max()))
    assert fullest > 8                                                                 # a cell with more entries than the speculative fetch takes
    if (W, H) == (1920, 1080):
        assert beyond[0] > 1000 and beyond[1] > 500 and beyond[2:] == [0] * 6
    elif (W, H) == (1022, 1022):
        assert beyond[0] > 200 and beyond[1:] == [0] * 7
    else:
        assert beyond == [0] * 8


# ------------------------------------------------------------------ 5. the 4000-wide image

def test_wide_image_carries_x_beyond_3900_through_every_level_that_has_cells():
    W, H = xb.WIDE_SHAPE
    r = xb.wide_ref()
    sizes = xb.level_sizes(W, H, 1.2, xb.WIDE_LEVELS)
    assert sizes == [(4000, 100), (3333, 83), (2778, 69), (2315, 58)]
    assert [r.ex.level(l).shape for l in range(4)] == [(h, w) for w, h in sizes]
    assert sizes[-1][1] > 2 * xb.EDGE                                                 # the top level is larger than its border ...
    assert xb.cell_grid(*sizes[2])[1] == 1 and (sizes[3][1] - 32) // xb.CELL == 0 and r.n_cands[3] == 0      # ... but too low for a cell row
    assert [xb.n_roots(w, h) for w, h in sizes[:3]] == [58, 65, 74]                   # many roots: the plain pass loop
    assert max(r.n_cands) <= xb.KEY_CAP and r.overflowing_levels() == []
    cand_x = int(r.cands[0][:, 0].max())
    assert 3900 < cand_x + (xb.EDGE - 3) <= 3980 and cand_x < 4096                    # level coordinates fit 12 bits, barely
    assert int((r.kps["x"] > 3900).sum()) >= 8 and float(r.kps["x"].max()) > 3960
    assert {int(o) for o in r.kps["octave"][r.kps["x"] > 3900]} == {0, 1, 2}


# ------------------------------------------------------------------ 6. stereo pairs with an empty side

@pytest.mark.parametrize("case", xb.EMPTY_SIDE_CASES)
def test_empty_side_pairs_have_the_side_they_name_and_no_match(case):
    e = xb.empty_side_ref(case)
    nl, nr = len(e["refL"].kps), len(e["refR"].kps)
    assert (nl > 900) == (case in ("right_flat", "rows_apart")) and (nl == 0) == (case in ("left_flat", "both_flat"))
    assert (nr > 900) == (case in ("left_flat", "rows_apart")) and (nr == 0) == (case in ("right_flat", "both_flat"))
    assert len(e["uright"]) == nl and (e["uright"] == -1).all() and (e["depth"] == -1).all()
    assert e["refL"].overflowing_levels() == [] and e["refR"].overflowing_levels() == []
    if case == "rows_apart":
        # the row band of every right keypoint (S/Frame.cc:806-811) misses the row of every left keypoint
        kl, kr = e["refL"].kps, e["refR"].kps
        r = 2.0 * np.float32(1.2) ** kr["octave"].astype(np.float32)
        lo, hi = np.floor(kr["y"] - r).min(), np.ceil(kr["y"] + r).max()
        rows = kl["y"].astype(np.int64)
        assert rows.max() < lo and hi < 480 and lo - rows.max() > 2 * 1.2 ** 7


def test_the_frame_that_follows_an_overflow_is_an_ordinary_one():
    n = xb.normal_frame()
    assert len(n["refL"].kps) > 900 and int((n["uright"] > 0).sum()) > 200
    assert n["refL"].overflowing_levels() == [] and n["refR"].overflowing_levels() == []
