"""Fuse / SearchInNeighbors, the parts that need no GPU: the exports and their refusals, the ctypes mirrors, the checker
(tests/fuse_model.py) on known answers worked out by hand, and the share of records of the GPU tests' scene family that lie within
1e-6 of a gate -- the condition the <= 1 % exclusion of tests/test_gpu_fuse.py rests on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fuse_model as fm
from multi_orbslam3_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
F32, F64 = np.float32, np.float64
GPU_SEEDS = range(8)                 # tests/test_gpu_fuse.py: SEEDS


# ------------------------------------------------------------------ 1. the exports

def test_exports_are_present_and_declared():
    lib = capi.load()
    assert hasattr(lib, "orbm_fuse") and "orbm_fuse" in capi.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    assert re.search(r"\bint orbm_fuse\(", hdr)
    assert "#define ORBG_FUSE_CAND_CAP %d" % capi.FUSE_CAND_CAP in hdr and re.search(r"#define ORBG_FUSE_MAX_KEYFRAMES %d\b" % capi.FUSE_MAX_KEYFRAMES, hdr)


def _params():
    p = capi.FuseParams()
    p.struct_size, p.th = C.sizeof(capi.FuseParams), 3.0
    return p


def _points(m=4):
    from multi_orbslam3_amd import views
    return views.worldpoints_view(np.zeros((m, 3)), np.zeros((m, 3)), np.zeros(m), np.zeros(m), np.zeros((m, 32)), np.zeros(m), np.zeros(m))


def test_argument_refusals_come_before_the_device():
    lib = capi.load()
    view, keep = _points()
    p = _params()
    kfs = (capi.FuseKF * 513)()
    sf = np.ones(8, np.float32)
    for k in kfs:
        k.struct_size, k.n_levels, k.scale_factors, k.inv_level_sigma2 = C.sizeof(capi.FuseKF), 8, capi.ptr(sf), capi.ptr(sf)
    recs = np.zeros((513, 4), capi.FUSE_RECORD_DTYPE); recs["status"] = -7
    cand = np.zeros((513, 4, capi.FUSE_CAND_CAP), np.uint16)
    call = lambda a, K, v, q, r=capi.ptr(recs), c=capi.ptr(cand): lib.orbm_fuse(a, K, v, None, q, r, c)
    assert call(C.byref(kfs), 1, C.byref(view), None) == capi.ORBG_BAD_ARG
    assert call(C.byref(kfs), 1, None, C.byref(p)) == capi.ORBG_BAD_ARG
    assert call(None, 1, C.byref(view), C.byref(p)) == capi.ORBG_BAD_ARG
    assert call(C.byref(kfs), -1, C.byref(view), C.byref(p)) == capi.ORBG_BAD_ARG
    assert call(C.byref(kfs), 513, C.byref(view), C.byref(p)) == capi.ORBG_CAP_EXCEEDED          # more than ORBG_FUSE_MAX_KEYFRAMES
    assert call(C.byref(kfs), 2, C.byref(view), C.byref(p), r=None) == capi.ORBG_BAD_ARG          # NULL outputs
    assert call(C.byref(kfs), 2, C.byref(view), C.byref(p), c=None) == capi.ORBG_BAD_ARG
    assert call(C.byref(kfs), 2, C.byref(view), C.byref(p)) == capi.ORBG_BAD_ARG                  # no frame
    bad = _params(); bad.struct_size = 8
    assert call(C.byref(kfs), 1, C.byref(view), C.byref(bad)) == capi.ORBG_BAD_ARG
    kfs[0].struct_size = 16
    assert call(C.byref(kfs), 1, C.byref(view), C.byref(p)) == capi.ORBG_BAD_ARG
    kfs[0].struct_size = C.sizeof(capi.FuseKF); kfs[0].n_levels = 17
    assert call(C.byref(kfs), 1, C.byref(view), C.byref(p)) == capi.ORBG_BAD_ARG
    broken, keep2 = _points(); broken.desc = None
    assert call(C.byref(kfs), 1, C.byref(broken), C.byref(p)) == capi.ORBG_BAD_ARG
    assert (recs["status"] == -7).all()                                                           # nothing was written
    # nothing to do needs neither a launch nor a device
    assert call(C.byref(kfs), 0, C.byref(view), C.byref(p)) == capi.ORBG_OK


def test_without_a_device_the_refusal_is_no_device_after_the_argument_checks():
    """A keyframe cannot be made resident without a device (ORBG_NO_DEVICE from orbm_frame_create, no CPU path), so no call of
    orbm_fuse with valid arguments can be formed without one: this test does NOT call orbm_fuse.  What it shows is that the only way to a
    launch is closed with ORBG_NO_DEVICE; that wrong arguments are refused for what they are on any machine is the test above, which
    runs without a device too.  orbm_fuse's own ORBG_NO_DEVICE (a device that went away after the frames were made) is not tested."""
    lib = capi.load()
    if lib.orbg_device_count() > 0:
        kfs, pts, _ = fm.make_scene(0, K=1, n=20, P=10)
        assert fm.device_keyframe(kfs[0]).frame.n == 20
        return
    kfs, pts, _ = fm.make_scene(0, K=1, n=20, P=10)
    with pytest.raises(capi.OrbGpuError) as e:
        fm.device_keyframe(kfs[0])
    assert e.value.code == capi.ORBG_NO_DEVICE


def test_ctypes_mirrors_have_the_headers_layout(tmp_path):
    fields = {"orbm_fuse_kf": ("FuseKF", [f[0] for f in capi.FuseKF._fields_]),
              "orbm_fuse_params": ("FuseParams", [f[0] for f in capi.FuseParams._fields_])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "orbgpu.h"', 'int main(void) {']
    for cname, (_, fl) in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in fl:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append('printf("orbm_fuse_record %zu\\n", sizeof(orbm_fuse_record));')
    for f in capi.FUSE_RECORD_DTYPE.names:
        lines.append('printf("orbm_fuse_record.%s %%zu\\n", offsetof(orbm_fuse_record, %s));' % (f, f))
    lines.append('printf("codes %d %d %d %d %d %d %d %d\\n", ORBM_FUSE_CANDIDATES, ORBM_FUSE_NEG_DEPTH, ORBM_FUSE_NOT_IN_IMAGE, ORBM_FUSE_DISTANCE, '
                 'ORBM_FUSE_NORMAL, ORBM_FUSE_EMPTY_WINDOW, ORBM_FUSE_NO_CANDIDATE, ORBM_FUSE_SKIPPED);')
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
    assert int(got["orbm_fuse_record"]) == capi.FUSE_RECORD_DTYPE.itemsize
    for f in capi.FUSE_RECORD_DTYPE.names:
        assert int(got["orbm_fuse_record.%s" % f]) == capi.FUSE_RECORD_DTYPE.fields[f][1]
    codes = [int(v) for v in text[-1].split()[1:]]
    assert codes == list(range(8)) == [fm.CANDIDATES, fm.NEG_DEPTH, fm.NOT_IN_IMAGE, fm.DISTANCE, fm.NORMAL, fm.EMPTY_WINDOW, fm.NO_CANDIDATE, fm.SKIPPED]
    assert codes == [capi.FUSE_CANDIDATES, capi.FUSE_NEG_DEPTH, capi.FUSE_NOT_IN_IMAGE, capi.FUSE_DISTANCE, capi.FUSE_NORMAL,
                     capi.FUSE_EMPTY_WINDOW, capi.FUSE_NO_CANDIDATE, capi.FUSE_SKIPPED]


def test_mock_members_are_public_in_the_reference():
    """Every `// ref: I/<Header>.h:<line> <name>` note of tests/cpp/mock_fuse.hpp: that line of the reference's header declares that
    name, in a public section -- the glue needs no reference-side edit."""
    from test_reference_access import REF_INC
    notes = re.findall(r"// ref: I/(\w+\.h):(\d+) (\w+)", open(os.path.join(CPP, "mock_fuse.hpp")).read())
    assert len(notes) >= 30
    glue = open(os.path.join(ROOT, "include", "orbgpu_localmapping.hpp")).read()
    for _, _, name in notes:
        assert re.search(r"\b%s\b" % name, glue), "the mock notes a member the glue does not read: %s" % name
    if not os.path.isdir(REF_INC):
        return                                   # the reference is only present in the build container
    for hdr, line, name in notes:
        lines = open(os.path.join(REF_INC, hdr)).read().splitlines()
        assert re.search(r"\b%s\b" % name, lines[int(line) - 1]), (hdr, line, name, lines[int(line) - 1])
        labels = [m.group(1) for ln in lines[: int(line)] for m in [re.match(r"\s*(public|protected|private)\s*:", ln)] if m]
        assert labels and labels[-1] == "public", (hdr, line, name, labels[-1:])


# ------------------------------------------------------------------ 2. the inputs of the GPU tests

@pytest.mark.parametrize("sim3", [False, True])
def test_near_share_of_the_gpu_family_is_within_the_cap(sim3):
    for seed in GPU_SEEDS:
        share = fm.near_share(seed, sim3)
        assert share <= 0.01, (seed, share)


def test_float32_and_float64_models_agree_outside_near():
    kfs, pts, _ = fm.make_scene(0)
    for sim3 in (False, True):
        r32, c32, _, _ = fm.records(kfs, pts, 3.0, sim3, F32)
        r64, c64, _, near = fm.records(kfs, pts, 3.0, sim3, F64)
        differ = (r32 != r64) | (c32 != c64).any(axis=2)
        assert differ[~near].mean() <= 1e-3 and set(r32["status"].ravel().tolist()) == set(range(7))


# ------------------------------------------------------------------ 3. known answers

def one_point_scene(X=(0.0, 0.0, 5.0), level=2.5):
    """A keyframe at the origin looking down z, one point; the point's range puts PredictScale at ceil(level)."""
    X = np.asarray([X], F64)
    d = np.linalg.norm(X, axis=1)
    pts = fm.points(X, X / d[:, None], d * 1.2 ** level / 1.2 ** 7, d * 1.2 ** level, np.zeros((1, 32), np.uint8))
    return pts


def kf_with(features, n_extra=0):
    """features: list of (x, y, octave, uright, descriptor bits set)."""
    kf = fm.keyframe(np.eye(3), np.zeros(3), len(features))
    for j, (x, y, o, ur, bits) in enumerate(features):
        kf["kps"][j]["x"], kf["kps"][j]["y"], kf["kps"][j]["octave"] = x, y, o
        kf["uright"][j] = ur
        d = np.zeros(256, np.uint8); d[:bits] = 1
        kf["desc"][j] = np.packbits(d)
    kf["Scw"] = np.eye(4, dtype=F32)
    return fm.finish(kf)


def ev(kf, pts, sim3=False, T=F32, th=3.0):
    return fm.evaluate_pair(kf, pts, 0, th, sim3, T)


def test_point_behind_the_camera():
    kf = kf_with([(367.0, 248.0, 2, -1.0, 0)])
    for T in (F32, F64):
        assert ev(kf, one_point_scene((0, 0, -5.0)), T=T)["status"] == fm.NEG_DEPTH
        assert ev(kf, one_point_scene((0, 0, 5.0)), T=T)["status"] == fm.CANDIDATES


def test_image_borders_are_closed_below_and_open_above():
    """fx = fy = 1, cx = cy = 0, z = 1: the projection is the point's x, y exactly, so it can be put ON each border."""
    kf = kf_with([(1.0, 1.0, 2, -1.0, 0)])
    kf["fx"] = kf["fy"] = F32(1.0)
    kf["cx"] = kf["cy"] = F32(0.0)
    below = lambda b: np.nextafter(F32(b), F32(-1e9))

    def inside(u, v, T):
        pts = fm.points([[u, v, 1.0]], [[0, 0, 1.0]], [0.1], [1e4], np.zeros((1, 32), np.uint8))
        return fm.evaluate_pair(kf, pts, 0, 3.0, False, T)["status"] != fm.NOT_IN_IMAGE
    for T in (F32, F64):
        assert inside(0.0, 100.0, T) and not inside(below(0.0), 100.0, T)               # x >= mnMinX
        assert inside(100.0, 0.0, T) and not inside(100.0, below(0.0), T)               # y >= mnMinY
        assert not inside(752.0, 100.0, T) and inside(below(752.0), 100.0, T)           # x < mnMaxX
        assert not inside(100.0, 480.0, T) and inside(100.0, below(480.0), T)           # y < mnMaxY


def test_windows_beyond_each_grid_edge_return_empty():
    """GetFeaturesInArea's four early returns, driven directly (x, y, r as Fuse would pass them)."""
    kf = kf_with([(5.0, 5.0, 0, -1.0, 0), (740.0, 470.0, 0, -1.0, 0)])          # (a feature at 747, 475 would round to cell 64, 48: PosInGrid drops it)
    for T in (F32, F64):
        assert fm.features_in_area(kf, T(770.0), T(100.0), T(3.0), T)[0] == []          # nMinCellX >= mnGridCols
        assert fm.features_in_area(kf, T(-30.0), T(100.0), T(3.0), T)[0] == []          # nMaxCellX < 0
        assert fm.features_in_area(kf, T(100.0), T(500.0), T(3.0), T)[0] == []          # nMinCellY >= mnGridRows
        assert fm.features_in_area(kf, T(100.0), T(-30.0), T(3.0), T)[0] == []          # nMaxCellY < 0
        assert fm.features_in_area(kf, T(4.0), T(4.0), T(3.0), T)[0] == [0]
        assert fm.features_in_area(kf, T(742.0), T(472.0), T(3.0), T)[0] == [1]
        assert fm.features_in_area(kf, T(8.0), T(5.0), T(3.0), T)[0] == []              # fabs(distx) < r is strict


def test_features_in_area_order_is_ix_outer_iy_inner_then_grid_order():
    # cells are 11.75 x 10 px and PosInGrid ROUNDS: cell ix covers [(ix - 0.5) * 11.75, (ix + 0.5) * 11.75).  Five features around
    # the corner (417.125, 255) of cells (35|36, 25|26), given in scrambled order
    feats = [(418.0, 256.0, 2, -1.0, 0), (416.0, 254.0, 2, -1.0, 0), (418.5, 253.5, 2, -1.0, 0), (416.5, 256.5, 2, -1.0, 0), (416.2, 253.0, 2, -1.0, 0)]
    kf = kf_with(feats)
    for T in (F32, F64):
        got, _ = fm.features_in_area(kf, T(417.1), T(255.0), T(4.0), T)
        assert got == [1, 4, 3, 2, 0]                 # cell (35, 25): 1, 4 ascending; (35, 26): 3; (36, 25): 2; (36, 26): 0


def test_level_is_clamped_at_both_ends():
    kf = kf_with([(367.0, 248.0, 0, -1.0, 0)])
    # with the scale factor 1.2 of these keyframes ceil(q) < 0 needs mfMaxDistance < dist3D / 1.2, which the distance gate :1483 has
    # already refused: there the lower clamp only ever sees -0 ...
    assert ev(kf, one_point_scene(level=-3.5))["status"] == fm.DISTANCE
    assert ev(kf, one_point_scene(level=-0.9))["level"] == 0
    # ... but a pyramid with a smaller scale factor reaches it: q = -1.5, ceil(q) = -1, clamped to 0
    kf11, pts11 = fm.low_scale_factor_scene()
    for T in (F32, F64):
        ratio = T(pts11["max_dist"][0]) / T(5.0)
        assert np.ceil(T(np.log(F64(ratio))) / T(kf11["log_sf"])) == -1                       # the clamp has something to clamp
        o = fm.evaluate_pair(kf11, pts11, 0, 3.0, False, T)
        assert o["level"] == 0 and o["status"] == fm.CANDIDATES and o["best_idx"] == 0       # radius 3 * 1.0, octave 0 passes the level gate
        assert fm.evaluate_pair(kf11, pts11, 0, 3.0, True, T)["level"] == 0
    assert ev(kf, one_point_scene(level=0.5))["level"] == 1
    assert ev(kf, one_point_scene(level=6.5))["level"] == 7
    pts = one_point_scene(level=6.5)
    pts["max_dist"] *= F32(1.2 ** 4); pts["min_dist"] *= F32(0.5)       # ceil(10.5) = 11 -> mnScaleLevels - 1
    o = ev(kf, pts)
    assert o["level"] == 7 and o["status"] == fm.NO_CANDIDATE           # octave 0 is below nPredictedLevel - 1


def test_level_and_chi2_gates():
    # stereo feature: e2 = ex^2 + ey^2 + er^2 against 7.8 * sigma2; mono against 5.99 * sigma2 (sigma2 of octave 2 = 1.2^4)
    s2 = 1.2 ** 4
    ok_m, no_m = np.sqrt(5.9 * s2), np.sqrt(6.1 * s2)
    pts = one_point_scene(level=2.5)                                   # level 3: octaves 2 and 3 pass, r = 3 * 1.728
    ur = 367.0 - fm.MB * fm.FX / 5.0
    kf = kf_with([(367.0 + ok_m, 248.0, 2, -1.0, 0), (367.0 + no_m, 248.0, 2, -1.0, 8), (367.0, 248.0, 1, -1.0, 0), (367.0, 248.0, 4, -1.0, 0),
                  (367.0 + np.sqrt(7.7 * s2), 248.0, 2, ur, 16), (367.0, 248.0, 2, ur + np.sqrt(7.9 * s2), 0)])
    o = ev(kf, pts)
    assert sorted(o["cand"]) == [0, 4] and o["level"] == 3
    o3 = ev(kf, pts, sim3=True)
    assert sorted(o3["cand"]) == [0, 1, 4, 5]                           # the Sim3 form has the level gate only


def test_hamming_tie_goes_to_the_earlier_candidate():
    pts = one_point_scene(level=1.5)
    kf = kf_with([(368.0, 248.0, 2, -1.0, 9), (366.0, 248.0, 2, -1.0, 7), (367.0, 249.0, 2, -1.0, 7)])
    o = ev(kf, pts)
    assert o["cand"] == [0, 1, 2] and (o["best_idx"], o["best_dist"]) == (1, 7)
    assert fm.rescore([2, 1, 0], kf["desc"], pts["desc"][0]) == (2, 7)


def _fused(kf, pts, sim3, limit):
    o = ev(kf, pts, sim3=sim3)
    rp = fm.Replay([kf], [np.full(len(kf["kps"]), -1)], pts["desc"])
    return rp.commit(0, 0, o["best_idx"], o["best_dist"], limit), rp


def test_best_dist_50_fuses_and_51_does_not_and_sim3_accepts_100():
    pts = one_point_scene(level=1.5)
    for bits, lm, s3 in ((50, 1, 1), (51, 0, 1), (100, 0, 1), (101, 0, 0)):
        kf = kf_with([(367.0, 248.0, 2, -1.0, bits)])
        n, rp = _fused(kf, pts, False, fm.TH_LOW)
        assert n == lm and (rp.kf_mp[0][0] == 0) == bool(lm)
        n, _ = _fused(kf, pts, True, 100)
        assert n == s3


def test_replay_replaces_towards_the_point_with_more_observations():
    pts = fm.points(np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3), np.zeros(3), np.arange(96, dtype=np.uint8).reshape(3, 32))
    two = lambda: kf_with([(100.0, 100.0, 0, -1.0, 0), (200.0, 100.0, 0, 150.0, 1)])      # feature 0 monocular, feature 1 stereo
    kfs = [two(), two(), two()]
    # point 1: feature 1 of keyframe 0 and feature 0 of keyframe 1 (2 + 1 observations); point 0: feature 0 of keyframe 2 (1);
    # point 2: feature 1 of keyframe 2 (2)
    rp = fm.Replay(kfs, [[-1, 1], [1, -1], [0, 2]], pts["desc"])
    assert rp.n_obs.tolist() == [1, 3, 2]
    # point 0 lands on feature 1 of keyframe 0, which point 1 holds: 3 > 1, pMP->Replace(pMPinKF)
    assert rp.commit(0, 0, 1, 10) == 1
    assert rp.bad.tolist() == [True, False, False] and rp.replaced[0] == 1
    assert rp.kf_mp[2].tolist() == [1, 2] and rp.n_obs[1] == 4 and rp.n_distinctive[1] == 1
    assert rp.skipped(1, 0) and rp.skipped(2, 1)                      # bad; already in the keyframe
    # point 2 lands on feature 0 of keyframe 1, held by point 1: 4 > 2, point 2 is replaced; point 1 is in keyframe 2 already, so
    # point 2's feature there is erased (S/MapPoint.cc:404-412)
    assert rp.commit(1, 2, 0, 10) == 1
    assert rp.bad.tolist() == [True, False, True] and rp.kf_mp[2].tolist() == [1, -1] and rp.n_obs[1] == 4
    # the other direction: a point with MORE observations than the holder replaces the holder
    rp2 = fm.Replay(kfs, [[-1, 1], [1, -1], [0, 2]], pts["desc"])
    assert rp2.commit(0, 2, 1, 10) == 1                               # 3 > 2: point 2 replaced by point 1 again
    rp3 = fm.Replay(kfs, [[0, -1], [1, 1 - 2], [2, 1]], pts["desc"])   # point 0: kf0 f0 (1 obs); point 1: kf1 f0, kf2 f1 (3); point 2: kf2 f0 (1)
    assert rp3.commit(0, 1, 0, 10) == 1                               # holder point 0 has 1 < 3: pMPinKF->Replace(pMP)
    assert rp3.bad.tolist() == [True, False, False] and rp3.kf_mp[0].tolist() == [1, -1] and rp3.n_obs[1] == 4
    assert rp.commit(1, 1, 1, 51) == 0                                # above TH_LOW: nothing happens
    # an empty feature takes the observation
    rp4 = fm.Replay(kfs, [[-1, -1], [0, -1], [-1, -1]], pts["desc"])
    assert rp4.commit(0, 0, 1, 50) == 1 and rp4.kf_mp[0].tolist() == [-1, 0] and rp4.n_obs[0] == 3
