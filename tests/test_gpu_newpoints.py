"""CreateNewMapPoints on the device (csrc/newpoints.hip) against tests/newpoints_model.py.

The match stage is float32 elementary operations only and must EQUAL the float32 model; the triangulation's status codes must equal
the float64 model outside the records the model itself calls undecided (a gate within 1e-3 relative -- reprojection, scale ratio --
or 1e-6 absolute -- the cosine gates -- of its threshold), at most 1 % of the matched pairs of the family; UnprojectStereo points are
bit-equal to the float32 model; triangulated points are compared with the float64 model, per parallax band, within 4 x what the
float32 model (an SVD in the reference's precision) differs from it on the same family; the replay is checked by feeding the
device's own records to the model's replay.  Measured values: docs/experiments.md, "CreateNewMapPoints"."""
import threading

import numpy as np
import pytest

import newpoints_model as nm
from multi_orbslam3_amd import api

pytestmark = pytest.mark.gpu
SEEDS = range(8)
F32, F64 = np.float32, np.float64


def run(k1, nbs, p, dev=None):
    d1, dn = dev if dev is not None else (nm.device_keyframe(k1), [nm.device_keyframe(k) for k in nbs])
    return api.CreateNewMapPoints(d1, dn, **{k: (float(v) if k == "th_far_points" else v) for k, v in p.items()})


def check(k1, nbs, p, res=None):
    """Every property of one call that does not need the family: match stage == float32 model (outside `near`), status codes ==
    float64 model (outside `undecided`), out / matches == the model's replay of the device's own records.  Returns what it used."""
    res = run(k1, nbs, p) if res is None else res
    rec = res.records
    r32, x32, _, _ = nm.records(k1, nbs, p, F32)
    r64, x64, near, und = nm.records(k1, nbs, p, F64)
    assert rec.shape == r32.shape
    assert near.sum() <= 0.01 * max(near.size, 1)
    cmp = ~near
    assert np.array_equal(rec["idx2"][cmp], r32["idx2"][cmp]) and np.array_equal(rec["dist"][cmp], r32["dist"][cmp])
    unmatched = rec["idx2"] < 0
    assert np.array_equal(rec["status"][unmatched & cmp], r32["status"][unmatched & cmp])          # codes 1 - 4 are integer logic
    pairs = (rec["idx2"] >= 0) & (rec["idx2"] == r64["idx2"])
    assert und[pairs].sum() <= max(1, 0.01 * pairs.sum()) or pairs.sum() < 100
    decided = pairs & ~und
    assert np.array_equal(rec["status"][decided], r64["status"][decided]), \
        list(zip(*np.nonzero(decided & (rec["status"] != r64["status"]))))
    angles2 = [k["kps"]["angle"] for k in nbs]
    out, matches = nm.replay(rec, k1["has_mp"], p["check_orientation"], k1["kps"]["angle"], angles2)
    assert np.array_equal(res.matches, matches)
    assert len(res.out) == len(out)
    for got, want in zip(res.out, out):
        assert (got["neighbour"], got["idx1"], got["idx2"]) == want[:3] and got["x3D"].tobytes() == want[3].tobytes()
    return dict(res=res, r32=r32, x32=x32, r64=r64, x64=x64, near=near, und=und, pairs=pairs)


@pytest.fixture(scope="module")
def family():
    """n1 = n2 = 200 (no multiple of 64 or 16), B = 3, depths 2 - 12 m, baselines 0.15 - 0.5 m, 1 px * scale noise, 15 % gross
    mismatches, half the features stereo; 8 seeds.  Computed once, shared, never modified."""
    fam = []
    for seed in SEEDS:
        k1, nbs = nm.make_scene(seed)
        c = check(k1, nbs, nm.params())
        c.update(k1=k1, nbs=nbs)
        fam.append(c)
    return fam


def test_match_stage_equals_the_float32_model(family):
    total = left_out = 0
    for c in family:
        rec, cmp = c["res"].records, ~c["near"]
        assert np.array_equal(rec["idx2"][cmp], c["r32"]["idx2"][cmp]) and np.array_equal(rec["dist"][cmp], c["r32"]["dist"][cmp])
        total += rec.size; left_out += c["near"].sum()
        assert (rec["idx2"] >= 0).sum() > 200
    print("match stage: %d records, %d left out as within 1e-6 of a threshold" % (total, left_out))
    assert left_out <= 0.01 * total


def test_status_codes_equal_the_float64_model(family):
    pairs = und = 0
    seen = set()
    for c in family:
        rec = c["res"].records
        sel = c["pairs"]
        pairs += sel.sum(); und += (sel & c["und"]).sum()
        d = sel & ~c["und"]
        assert np.array_equal(rec["status"][d], c["r64"]["status"][d])
        seen |= set(rec["status"][sel].tolist())
    print("triangulation stage: %d matched pairs, %d undecided" % (pairs, und))
    assert und <= 0.01 * pairs
    assert {nm.ACCEPTED, nm.LOW_PARALLAX, nm.Z1, nm.REPROJ1, nm.REPROJ2} <= seen


def test_unproject_stereo_points_are_bit_equal_to_the_float32_model(family):
    n = 0
    for c in family:
        rec, r32 = c["res"].records, c["r32"]
        formed = (rec["status"] == nm.ACCEPTED) | (rec["status"] >= nm.Z1)         # a point was formed; w == 0: by UnprojectStereo
        sel = c["pairs"] & (rec["idx2"] == r32["idx2"]) & formed & (rec["w"] == 0) & (r32["w"] == 0) & (r32["status"] == rec["status"])
        assert rec["x3D"][sel].tobytes() == r32["x3D"][sel].tobytes()
        n += sel.sum()
    print("UnprojectStereo points compared: %d" % n)
    assert n >= 20


def _band_errors(family, which):
    """Per parallax band: errors of `which` ("f32 model" or "device") against the float64 model over the triangulated points."""
    errs = {0: [], 1: [], 2: []}
    for c in family:
        rec, r32, r64 = c["res"].records, c["r32"], c["r64"]
        tri64 = (r64["w"] != 0) & (r64["status"] != nm.W_ZERO) & (r64["idx2"] >= 0)
        if which == "device":
            sel, x = c["pairs"] & tri64 & (rec["w"] != 0) & (rec["status"] != nm.W_ZERO), rec["x3D"]
        else:
            sel, x = tri64 & (r32["idx2"] == r64["idx2"]) & (r32["w"] != 0) & (r32["status"] != nm.W_ZERO), c["x32"]
        # points in front of both cameras only: behind a camera (a gross mismatch) the "point" is the far side of a near-parallel pair
        sel = sel & (r64["status"] != nm.Z1) & (r64["status"] != nm.Z2)
        band = nm.parallax_band(r64["cos_parallax"])
        for b in range(3):
            s = sel & (band == b)
            errs[b] += list(nm.point_error(x[s], c["x64"][s], c["k1"]))
    return errs


def test_triangulated_points_against_the_float64_model(family):
    ref, dev = _band_errors(family, "f32 model"), _band_errors(family, "device")
    names = ["cos > 0.9998", "0.998 <= cos <= 0.9998", "cos < 0.998"]
    for b in range(3):
        assert len(ref[b]) >= 50 and len(dev[b]) >= 50
        bound = 4 * max(ref[b])
        print("band %-24s %5d points  float32 model vs float64: max %.3e  bound %.3e  device vs float64: max %.3e median %.3e" %
              (names[b], len(dev[b]), max(ref[b]), bound, max(dev[b]), float(np.median(dev[b]))))
    for b in range(3):
        assert max(dev[b]) <= 4 * max(ref[b])


def test_two_runs_give_the_same_bits(family):
    c = family[0]
    again = run(c["k1"], c["nbs"], nm.params())
    assert again.records.tobytes() == c["res"].records.tobytes() and again.out.tobytes() == c["res"].out.tobytes()


def test_a_feature_triangulable_in_two_neighbours_is_created_by_the_first(family):
    """... and with the rotation vote on, neighbour 2's vote does not see it (the replay drops claimed features before it votes)."""
    c = family[7]                                                             # (a scene on which the order of vote and drop matters)
    rec = c["res"].records
    both = np.nonzero((rec["status"][0] == 0) & (rec["status"][2] == 0) & (rec["idx2"][0] >= 0) & (rec["idx2"][2] >= 0))[0]
    assert len(both) > 5
    out = c["res"].out
    for i in both:
        assert [int(o["neighbour"]) for o in out if o["idx1"] == i] == [0]
        assert c["res"].matches[2, i] == -1 and c["res"].matches[0, i] == rec["idx2"][0, i]
    v = check(c["k1"], c["nbs"], nm.params(check_orientation=True))
    assert (v["res"].matches != c["res"].matches).any()                       # the vote removed something
    # voting over ALL of a neighbour's matches and dropping the claimed ones afterwards is a different function on this scene
    assert not np.array_equal(_vote_then_drop(v["res"].records, c["k1"], c["nbs"]), v["res"].matches)


def _vote_then_drop(rec, k1, nbs):
    """The wrong order: the rotation vote sees the features an earlier neighbour has claimed."""
    B, n1 = rec.shape
    claimed = k1["has_mp"] != 0
    matches = np.full((B, n1), -1, np.int32)
    for b in range(B):
        m12 = rec["idx2"][b].copy()
        m12[k1["has_mp"] != 0] = -1
        hist = [[] for _ in range(nm.HISTO_LENGTH)]
        for i in np.nonzero(m12 >= 0)[0]:
            hist[nm.rot_bin(k1["kps"]["angle"][i], nbs[b]["kps"]["angle"][m12[i]])].append(i)
        keep = nm.three_maxima([len(h) for h in hist])
        for k, h in enumerate(hist):
            if k not in keep:
                m12[h] = -1
        m12[claimed] = -1
        matches[b] = m12
        claimed = claimed | ((m12 >= 0) & (rec["status"][b] == nm.ACCEPTED))
    return matches


def test_node_with_70_candidates_and_node_with_one():
    k1, nbs = nm.make_scene(20, B=1)
    k2 = nbs[0]
    J = np.sort(np.random.default_rng(3).permutation(200)[:71])
    big, single = J[:70], J[70]
    n2, n1 = k2["node"].copy(), k1["node"].copy()
    n2[big] = 901; n1[k2["src"][big]] = 901
    n2[single] = 902; n1[k2["src"][single]] = 902
    nm.set_nodes(k1, n1); nm.set_nodes(k2, n2)
    k1["has_mp"][k2["src"][J]] = 0; k2["has_mp"][J] = 0
    c = check(k1, nbs, nm.params())
    rec = c["res"].records[0]
    in_big = k2["src"][big]
    won = rec["idx2"][in_big]
    assert (won >= 0).sum() >= 30
    assert (np.searchsorted(big, won[won >= 0]) >= 64).any()                  # a winner beyond the 64th list position
    assert (np.searchsorted(big, won[won >= 0]) < 16).any()
    assert rec["idx2"][k2["src"][single]] in (single, -1)
    assert rec["status"][k2["src"][single]] != nm.NO_NODE


def test_of_two_candidates_at_equal_distance_the_later_one_wins():
    k1, nbs = nm.make_scene(21, B=1)
    k2 = nbs[0]
    r, _, _, _ = nm.records(k1, nbs, nm.params(), F32)
    i = int(np.nonzero(r["idx2"][0] >= 0)[0][3])
    j = int(r["idx2"][0, i])
    for other in (j + 1 if j + 1 < 200 else j - 1, j - 1 if j >= 1 else j + 1):
        ka = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in k2.items()}
        nm.copy_feature(ka, j, other)
        c = check(k1, [ka], nm.params())
        assert c["res"].records["idx2"][0, i] == max(j, other)                # list order inside a node is ascending feature index
        assert c["res"].records["dist"][0, i] == r["dist"][0, i]


def test_two_features_matching_one_feature_are_both_created():
    k1, nbs = nm.make_scene(22, B=1)
    r, _, _, _ = nm.records(k1, nbs, nm.params(), F64)
    i = int(np.nonzero(r["status"][0] == nm.ACCEPTED)[0][2])
    twin = (i + 7) % 200
    nm.copy_feature(k1, i, twin)
    c = check(k1, nbs, nm.params())
    made = {int(o["idx1"]): int(o["idx2"]) for o in c["res"].out}
    assert made[i] == made[twin] == r["idx2"][0, i]


@pytest.mark.parametrize("case", ["only_stereo", "coarse", "far_points", "check_orientation"])
def test_parameters(case):
    k1, nbs = nm.make_scene(23)
    base = nm.records(k1, nbs, nm.params(), F32)[0]
    p = nm.params(**{case: True}, th_far_points=6.0 if case == "far_points" else 0.0)
    c = check(k1, nbs, p)
    rec = c["res"].records
    if case == "only_stereo":
        assert (rec["status"] == nm.NOT_STEREO).sum() > 50
        m = rec["idx2"] >= 0
        for b in range(3):
            i1 = np.nonzero(m[b])[0]
            assert (k1["uright"][i1] >= 0).all() and (nbs[b]["uright"][rec["idx2"][b][i1]] >= 0).all()
    elif case == "coarse":
        assert (rec["idx2"] >= 0).sum() > (base["idx2"] >= 0).sum() + 50
    elif case == "far_points":
        assert (rec["status"] == nm.FAR).sum() > 50 and (rec["status"] == nm.ACCEPTED).sum() > 50
    else:
        assert ((c["res"].matches < 0) & (rec["idx2"] >= 0) & (k1["has_mp"] == 0)[None]).sum() > 20


def test_search_for_triangulation_signature():
    k1, nbs = nm.make_scene(24, B=1)
    d1, d2 = nm.device_keyframe(k1), nm.device_keyframe(nbs[0])
    for ori in (False, True):
        for stereo in (False, True):
            got = api.SearchForTriangulation(d1, d2, only_stereo=stereo, check_orientation=ori)
            want = nm.search_for_triangulation(k1, nbs[0], nm.params(only_stereo=stereo, check_orientation=ori))
            assert len(want) > 20 and np.array_equal(got, want)


def test_empty_node_intersection():
    k1, nbs = nm.make_scene(25)
    for k in nbs:
        nm.set_nodes(k, k["node"] + 1)                                        # node ids are 7 k + 3 in KF1
    c = check(k1, nbs, nm.params())
    assert len(c["res"].out) == 0 and set(c["res"].records["status"].ravel().tolist()) <= {nm.HAS_POINT, nm.NO_NODE}
    nm.set_nodes(nbs[1], nbs[1]["node"] - 1)                                  # one neighbour shares nodes again: the launch path
    c = check(k1, nbs, nm.params())
    assert len(c["res"].out) > 50 and set(int(o["neighbour"]) for o in c["res"].out) == {1}
    assert set(c["res"].records["status"][0].tolist()) <= {nm.HAS_POINT, nm.NO_NODE}


@pytest.mark.parametrize("B", [1, 20])
def test_one_and_twenty_neighbours(B):
    k1, nbs = nm.make_scene(26, B=B)
    c = check(k1, nbs, nm.params())
    assert len(c["res"].out) > 80
    if B == 20:
        made = [int(o["neighbour"]) for o in c["res"].out]                    # later neighbours find most features claimed
        assert len(set(made)) >= 5 and max(made) >= 6


def test_a_neighbour_without_features():
    k1, nbs = nm.make_scene(27, n2=[200, 0, 130])
    c = check(k1, nbs, nm.params())
    assert (c["res"].records["status"][1] != nm.ACCEPTED).all() and (c["res"].matches[1] == -1).all()
    assert {0, 2} <= set(int(o["neighbour"]) for o in c["res"].out)
    k0, _ = nm.make_scene(27, n=0, B=0)                                       # and a current keyframe without features
    assert len(run(k0, nbs, nm.params()).out) == 0


def test_close_points_take_the_unproject_stereo_branches_with_distorted_keys():
    """Points at 0.4 - 2 m, all stereo: cosParallaxStereo is the smaller one for many pairs.  mvKeys differs from mvKeysUn."""
    k1, nbs = nm.make_scene(28, depth=(0.4, 2.0), baseline=(0.02, 0.06), stereo_fraction=1.0, mismatch=0.05)
    rng = np.random.default_rng(5)
    for k in [k1] + nbs:
        k["keys_xy"] = (np.stack([k["kps"]["x"], k["kps"]["y"]], 1) + rng.normal(size=(200, 2)) * 0.3).astype(np.float32)
    c = check(k1, nbs, nm.params())
    rec, r32 = c["res"].records, c["r32"]
    sel = (rec["idx2"] >= 0) & (rec["idx2"] == r32["idx2"]) & (rec["w"] == 0) & (r32["w"] == 0) & (rec["status"] == r32["status"]) & \
        ((rec["status"] == 0) | (rec["status"] >= nm.Z1))
    assert sel.sum() > 100 and rec["x3D"][sel].tobytes() == r32["x3D"][sel].tobytes()


def test_batch_against_single_calls():
    k1, nbs = nm.make_scene(29, B=5)
    d1, dn = nm.device_keyframe(k1), [nm.device_keyframe(k) for k in nbs]
    whole = run(k1, nbs, nm.params(), (d1, dn))
    has = k1["has_mp"].copy()
    outs = []
    for b in range(5):
        d1.has_mp = np.ascontiguousarray(has)
        one = run(k1, [nbs[b]], nm.params(), (d1, [dn[b]]))
        free = has == 0
        assert one.records[0][free].tobytes() == whole.records[b][free].tobytes()
        claimed = (has != 0) & (k1["has_mp"] == 0)
        assert (one.records["status"][0][claimed] == nm.HAS_POINT).all()
        assert np.array_equal(one.matches[0], whole.matches[b])
        o = one.out.copy(); o["neighbour"] = b
        outs.append(o)
        has[one.out["idx1"]] = 1
    assert np.concatenate(outs).tobytes() == whole.out.tobytes() and len(whole.out) > 100


def test_three_threads_three_frame_sets():
    scenes = [nm.make_scene(30 + t) for t in range(3)]
    dev = [(nm.device_keyframe(k1), [nm.device_keyframe(k) for k in nbs]) for k1, nbs in scenes]
    alone = [run(k1, nbs, nm.params(), d) for (k1, nbs), d in zip(scenes, dev)]
    got, errors = [None] * 3, []

    def work(t):
        try:
            for _ in range(5):
                got[t] = run(scenes[t][0], scenes[t][1], nm.params(), dev[t])
        except Exception as e:              # noqa: BLE001
            errors.append(e)
    th = [threading.Thread(target=work, args=(t,)) for t in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors
    for t in range(3):
        assert got[t].records.tobytes() == alone[t].records.tobytes() and got[t].out.tobytes() == alone[t].out.tobytes()
        assert np.array_equal(got[t].matches, alone[t].matches)
