"""CreateNewMapPoints, the parts that need no GPU: the exports and their refusals, the ctypes mirrors, the checker
(tests/newpoints_model.py) against itself -- the tie rule, the epipole exclusion, the replay on hand-made records -- and its own
float32-vs-float64 agreement on the scene family of tests/test_gpu_newpoints.py, the condition the GPU tolerances rest on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import newpoints_model as nm
from multi_orbslam3_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------ 1. the exports

def test_exports_are_present_and_declared():
    lib = capi.load()
    for name in ("orbm_create_new_points", "orbm_search_for_triangulation"):
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
        assert re.search(r"\bint %s\(" % name, open(os.path.join(ROOT, "include", "orbgpu.h")).read())


def test_no_gpu_means_no_new_points():
    lib = capi.load()
    if lib.orbg_device_count() > 0:
        pytest.skip("a GPU is present")
    k1, nbs = nm.make_scene(0, n=40, B=1)
    with pytest.raises(capi.OrbGpuError) as e:
        nm.device_keyframe(k1)
    assert e.value.code == capi.ORBG_NO_DEVICE


def _kf(frame=None):
    k = capi.NewPointsKF()
    k.struct_size = C.sizeof(capi.NewPointsKF)
    k.frame = frame
    k.n_levels = 8
    sf = np.ones(8, np.float32)
    k.scale_factors = k.level_sigma2 = capi.ptr(sf)
    k._keep = sf
    return k


def _params():
    p = capi.NewPointsParams()
    p.struct_size = C.sizeof(capi.NewPointsParams)
    return p


def test_argument_refusals_come_before_the_device():
    lib = capi.load()
    n = C.c_int(-7)
    out = np.zeros(4, capi.NEWPOINT_DTYPE)
    k1, kn, p = _kf(), (capi.NewPointsKF * 65)(), _params()
    call = lambda a, b, B, q, o=capi.ptr(out), cap=4, nn=C.byref(n): lib.orbm_create_new_points(a, b, B, q, o, cap, nn, None, None)
    assert call(None, C.byref(kn), 1, C.byref(p)) == capi.ORBG_BAD_ARG
    assert call(C.byref(k1), C.byref(kn), 1, None) == capi.ORBG_BAD_ARG
    assert call(C.byref(k1), None, 1, C.byref(p)) == capi.ORBG_BAD_ARG
    assert call(C.byref(k1), C.byref(kn), -1, C.byref(p)) == capi.ORBG_BAD_ARG
    assert call(C.byref(k1), C.byref(kn), 1, C.byref(p), nn=None) == capi.ORBG_BAD_ARG
    assert call(C.byref(k1), C.byref(kn), 1, C.byref(p), o=None) == capi.ORBG_BAD_ARG
    assert call(C.byref(k1), C.byref(kn), 65, C.byref(p)) == capi.ORBG_CAP_EXCEEDED             # more than ORBG_NEWPOINTS_MAX_NEIGHBOURS
    assert call(C.byref(k1), C.byref(kn), 0, C.byref(p)) == capi.ORBG_BAD_ARG                   # no frame
    bad = _params(); bad.struct_size = 8
    assert call(C.byref(k1), C.byref(kn), 1, C.byref(bad)) == capi.ORBG_BAD_ARG
    k1.struct_size = 16
    assert call(C.byref(k1), C.byref(kn), 0, C.byref(p)) == capi.ORBG_BAD_ARG
    assert n.value == -7                                                                        # nothing was written
    pairs = np.zeros((4, 2), np.int32)
    assert lib.orbm_search_for_triangulation(C.byref(_kf()), None, C.byref(p), capi.ptr(pairs), 4, C.byref(n)) == capi.ORBG_BAD_ARG
    assert lib.orbm_search_for_triangulation(C.byref(_kf()), C.byref(_kf()), C.byref(p), capi.ptr(pairs), 4, C.byref(n)) == capi.ORBG_BAD_ARG


def test_ctypes_mirrors_have_the_headers_layout(tmp_path):
    fields = {"orbm_newpoints_kf": ("NewPointsKF", ["struct_size", "frame", "featvec", "has_mp", "keys_xy", "Tcw", "Twc", "Ow", "fx", "mbf",
                                                    "n_levels", "scale_factors", "level_sigma2", "scale_factor"]),
              "orbm_newpoints_params": ("NewPointsParams", ["struct_size", "only_stereo", "coarse", "check_orientation", "far_points", "th_far_points"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "orbgpu.h"', 'int main(void) {']
    for cname, (_, fl) in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in fl:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    for cname, dt in (("orbm_newpoints_record", capi.NEWPOINTS_RECORD_DTYPE), ("orbm_newpoint", capi.NEWPOINT_DTYPE)):
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in dt.names:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append('printf("codes %d %d %d %d\\n", ORBM_NP_ACCEPTED, ORBM_NP_NO_MATCH, ORBM_NP_Z1, ORBM_NP_SCALE);')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    text = subprocess.check_output([exe], text=True).splitlines()
    got = dict(ln.split() for ln in text if not ln.startswith("codes"))
    for cname, (pyname, fl) in fields.items():
        cls = getattr(capi, pyname)
        assert int(got[cname]) == C.sizeof(cls), cname
        for f in fl:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, (cname, f)
    for cname, dt in (("orbm_newpoints_record", capi.NEWPOINTS_RECORD_DTYPE), ("orbm_newpoint", capi.NEWPOINT_DTYPE)):
        assert int(got[cname]) == dt.itemsize
        for f in dt.names:
            assert int(got["%s.%s" % (cname, f)]) == dt.fields[f][1]
    assert text[-1].split()[1:] == [str(v) for v in (nm.ACCEPTED, nm.NO_MATCH, nm.Z1, nm.SCALE)]
    assert (nm.ACCEPTED, nm.NO_MATCH, nm.Z1, nm.SCALE) == (capi.NP_ACCEPTED, capi.NP_NO_MATCH, capi.NP_Z1, capi.NP_SCALE)


def test_mock_members_are_public_in_the_reference():
    """Every `// ref: I/<Header>.h:<line> <name>` note of tests/cpp/mock_newpoints.hpp: that line of the reference's header declares
    that name, in a public section -- the glue needs no reference-side edit."""
    from test_reference_access import REF_INC
    if not os.path.isdir(REF_INC):
        pytest.skip("the reference is only present in the build container")
    notes = re.findall(r"// ref: I/(\w+\.h):(\d+) (\w+)", open(os.path.join(CPP, "mock_newpoints.hpp")).read())
    assert len(notes) >= 30
    for hdr, line, name in notes:
        lines = open(os.path.join(REF_INC, hdr)).read().splitlines()
        assert re.search(r"\b%s\b" % name, lines[int(line) - 1]), (hdr, line, name, lines[int(line) - 1])
        labels = [m.group(1) for ln in lines[: int(line)] for m in [re.match(r"\s*(public|protected|private)\s*:", ln)] if m]
        assert labels and labels[-1] == "public", (hdr, line, name, labels[-1:])


# ------------------------------------------------------------------ 2. the model against itself

def test_model_primitives_against_the_oracle():
    from oracle import binding as ob
    rng = np.random.default_rng(0)
    for _ in range(200):
        a, b = rng.uniform(0, 360, 2).astype(np.float32)
        assert nm.rot_bin(a, b) == ob.rot_bin(float(a), float(b))
        d1, d2 = rng.integers(0, 256, (2, 32), dtype=np.uint8)
        assert nm.hamming(d1, d2) == ob.hamming(d1, d2)
        sizes = rng.integers(0, 12, 30) * (rng.random(30) < 0.5)
        assert list(nm.three_maxima([int(s) for s in sizes])) == ob.three_maxima(sizes)


def _tiny_pair():
    """Two keyframes 0.3 m apart looking at one point 5 m away: features 0 of both observe it exactly; one vocabulary node."""
    k1 = nm.keyframe(np.eye(3), np.zeros(3), 1)
    k2 = nm.keyframe(np.eye(3), np.array([-0.3, 0.0, 0.0]), 3)
    X = np.array([0.4, -0.2, 5.0])
    for k, m in ((k1, 1), (k2, 3)):
        Xc = X + k["Tcw"][:, 3].astype(F64)
        k["kps"]["x"], k["kps"]["y"] = nm.FX * Xc[0] / Xc[2] + nm.CX, nm.FY * Xc[1] / Xc[2] + nm.CY
        k["desc"][:] = 0x5A
        nm.set_nodes(k, np.full(m, 7))
    return k1, k2


def test_model_tie_rule_the_last_candidate_at_the_smallest_distance_wins():
    k1, k2 = _tiny_pair()
    for T in (F32, F64):
        idx2, dist, status, _ = nm.match(k1, k2, nm.params(), T)
        assert (idx2[0], dist[0], status[0]) == (2, 0, nm.ACCEPTED)              # three equal candidates: the last in list order
        k2["desc"][2, 0] ^= 1                                                    # candidate 2 one bit worse: the tie is between 0 and 1
        assert nm.match(k1, k2, nm.params(), T)[0][0] == 1
        k2["desc"][0, 1] ^= 0xFF; k2["desc"][0, 2] ^= 0xFF                        # candidate 0 sixteen bits worse
        assert nm.match(k1, k2, nm.params(), T)[0][0] == 1
        k2["has_mp"][1] = 1                                                      # candidate 1 already holds a point
        idx2, dist, _, _ = nm.match(k1, k2, nm.params(), T)
        assert (idx2[0], dist[0]) == (2, 1)
        k2["has_mp"][1] = 0; k2["desc"][:] = 0x5A
    k2["desc"][:, :7] ^= 0xFF                                                    # 56 bits: above TH_LOW
    assert nm.match(k1, k2, nm.params(), F32)[2][0] == nm.NO_MATCH
    k1["has_mp"][0] = 1
    assert nm.match(k1, k2, nm.params(), F32)[2][0] == nm.HAS_POINT


def test_model_epipole_exclusion_applies_to_mono_mono_pairs_only():
    """KF2 half a metre ahead of KF1 on its optical axis: the epipole is the principal point.  A feature next to it is no candidate
    for a monocular pair (:1085-1093) and is one as soon as either side is stereo."""
    k1 = nm.keyframe(np.eye(3), np.zeros(3), 1)
    k2 = nm.keyframe(np.eye(3), np.array([0.0, 0.0, -0.5]), 1)
    for k in (k1, k2):
        k["kps"]["x"], k["kps"]["y"] = nm.CX + 3.0, nm.CY + 4.0                  # 5 px from the epipole: 25 < 100 * 1.0
        k["desc"][:] = 0x33
        nm.set_nodes(k, np.array([4]))
    _, ep = nm.pair_geometry(k1, k2, F32)
    assert np.allclose(ep, [nm.CX, nm.CY])
    p = nm.params(coarse=True)
    assert nm.match(k1, k2, p, F32)[2][0] == nm.NO_MATCH
    k2["kps"]["octave"] = 0; k2["kps"]["x"] += 8.0                               # 11.7 px away: 137 > 100
    assert nm.match(k1, k2, p, F32)[2][0] == nm.ACCEPTED
    k2["kps"]["x"] -= 8.0
    k2["kps"]["octave"] = 7                                                      # the threshold grows with the octave: still excluded
    assert nm.match(k1, k2, p, F32)[2][0] == nm.NO_MATCH
    k1["uright"][0], k1["depth"][0] = 300.0, 5.0                                 # a stereo feature in KF1: no exclusion
    assert nm.match(k1, k2, p, F32)[2][0] == nm.ACCEPTED
    assert nm.match(k1, k2, nm.params(coarse=True, only_stereo=True), F32)[2][0] == nm.NO_MATCH      # ... and KF2's is not stereo


def test_model_replay_on_hand_made_records():
    rec = np.zeros((3, 5), capi.NEWPOINTS_RECORD_DTYPE)
    rec["idx2"] = -1
    rec["status"] = nm.NO_MATCH

    def put(b, i, j, status, x=0.0):
        rec[b, i] = (j, 10, status, (x, x, x), 0.0, 0.5)
    put(0, 0, 4, nm.ACCEPTED, 1.0); put(2, 0, 9, nm.ACCEPTED, 2.0)               # feature 0: neighbours 0 and 2 -> only 0 creates it
    put(0, 1, 4, nm.ACCEPTED, 3.0)                                               # feature 1 shares idx2 = 4 with feature 0: both created
    put(0, 2, 6, nm.REPROJ1); put(1, 2, 7, nm.ACCEPTED, 4.0)                     # feature 2: rejected in 0, created by 1
    put(1, 3, 8, nm.ACCEPTED, 5.0)                                               # feature 3 holds a point already
    put(2, 4, 1, nm.Z1)
    has = np.array([0, 0, 0, 1, 0], np.uint8)
    out, m = nm.replay(rec, has)
    assert [(o[0], o[1], o[2], float(o[3][0])) for o in out] == [(0, 0, 4, 1.0), (0, 1, 4, 3.0), (1, 2, 7, 4.0)]
    assert m.tolist() == [[4, 4, 6, -1, -1], [-1, -1, 7, -1, -1], [-1, -1, -1, -1, 1]]
    # a prefix of the list is what an early exit at a neighbour boundary leaves
    assert [o[:3] for o in nm.replay(rec[:1], has)[0]] == [o[:3] for o in out[:2]]
    # the vote sees what is left after the drop: in neighbour 2 only feature 4 votes
    ang1 = np.zeros(5, np.float32)
    ang2 = [np.zeros(10, np.float32)] * 3
    assert np.array_equal(nm.replay(rec, has, True, ang1, ang2)[1], m)


def test_model_unprojects_and_triangulates_a_known_point():
    k1, k2 = _tiny_pair()
    X = np.array([0.4, -0.2, 5.0])
    for T, tol in ((F32, 2e-4), (F64, 2e-4)):                                   # (pixel coordinates are float32: 3e-5 px over a 27 px disparity)
        st, x, w, cosr, _ = nm.triangulate(k1, k2, np.array([0]), np.array([0]), nm.params(), T)
        assert st[0] == nm.ACCEPTED and w[0] != 0 and np.abs(x[0] - X).max() < tol and 0.99 < cosr[0] < 0.9998
    k1["depth"][0], k1["uright"][0] = 5.0, k1["kps"]["x"][0] - k1["mbf"] / 5.0
    k2m = nm.keyframe(np.eye(3), np.array([-0.01, 0.0, 0.0]), 1)                  # 1 cm baseline: the stereo parallax is the larger one
    k2m["kps"]["x"], k2m["kps"]["y"] = nm.FX * 0.39 / 5 + nm.CX, k1["kps"]["y"][0]
    st, x, w, _, _ = nm.triangulate(k1, k2m, np.array([0]), np.array([0]), nm.params(), F32)
    assert st[0] == nm.ACCEPTED and w[0] == 0 and np.abs(x[0] - X).max() < 1e-4
    st, _, _, _, _ = nm.triangulate(k1, k2m, np.array([0]), np.array([0]), nm.params(far_points=True, th_far_points=4.0), F32)
    assert st[0] == nm.FAR


# ------------------------------------------------------------------ 3. float32 against float64 on the scene family

def test_model_float32_and_float64_agree_on_the_scene_family():
    """20 seeds of the family of tests/test_gpu_newpoints.py: the matches of the float32 evaluation equal those of the float64 one
    outside the records with a candidate within 1e-6 of a threshold (at most 1 %), and the status codes outside the undecided pairs
    (at most 1 % of the matched pairs) -- no differing decision outside them."""
    records = near_n = pairs = und_n = 0
    worst = [0.0, 0.0, 0.0]
    for seed in range(20):
        k1, nbs = nm.make_scene(seed)
        r32, x32, _, _ = nm.records(k1, nbs, nm.params(), F32)
        r64, x64, near, und = nm.records(k1, nbs, nm.params(), F64)
        keep = ~near
        assert np.array_equal(r32["idx2"][keep], r64["idx2"][keep]) and np.array_equal(r32["dist"][keep], r64["dist"][keep])
        m = (r64["idx2"] >= 0) & (r32["idx2"] == r64["idx2"])
        assert np.array_equal(r32["status"][m & ~und], r64["status"][m & ~und])
        records += near.size; near_n += near.sum(); pairs += m.sum(); und_n += (m & und).sum()
        tri = m & (r64["w"] != 0) & (r32["w"] != 0) & (r64["status"] != nm.Z1) & (r64["status"] != nm.Z2) & (r64["status"] != nm.W_ZERO)
        band = nm.parallax_band(r64["cos_parallax"])
        for b in range(3):
            s = tri & (band == b)
            if s.any():
                worst[b] = max(worst[b], nm.point_error(x32[s], x64[s], k1).max())
    print("records %d near %d; matched pairs %d undecided %d; float32 vs float64 point error per band %s" % (records, near_n, pairs, und_n, worst))
    assert near_n <= 0.01 * records and und_n <= 0.01 * pairs and pairs > 5000
    assert max(worst) < 1e-4                                                     # float32 rounding over a parallax of 0.01 rad and more
