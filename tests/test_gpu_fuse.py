"""ORBmatcher::Fuse on the device (csrc/fuse.hip) against tests/fuse_model.py.

Every field of a record -- status, best_idx, best_dist, level, n_cand -- and the candidate list must EQUAL the float32 model outside
the records the float64 model calls `near` (a gate within 1e-6 relative of its threshold), at most 1 % of the records of the family;
both forms.  The serial part is checked by feeding the device's own records to the model's replay while descriptors change mid-way:
the outcome must equal the model's serial run of the reference's loop."""
import threading

import numpy as np
import pytest

import fuse_model as fm
from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import api

pytestmark = pytest.mark.gpu
SEEDS = range(8)
F32, F64 = np.float32, np.float64
TH = 3.0


def run(kfs, pts, sim3=False, skip=None, th=TH, dev=None):
    dk = dev if dev is not None else [fm.device_keyframe(k, sim3=sim3) for k in kfs]
    return api.Fuse(dk, fm.device_points(pts), th=th, sim3_form=sim3, skip=skip)


def compare(rec, cand, want_rec, want_cand, near):
    """All fields and the lists equal outside `near`; returns the number of records left out."""
    assert rec.shape == want_rec.shape and cand.shape == want_cand.shape
    cmp = ~near
    for f in ("status", "best_idx", "best_dist", "level", "n_cand"):
        bad = cmp & (rec[f] != want_rec[f])
        assert not bad.any(), (f, list(zip(*np.nonzero(bad)))[:5], rec[bad][:5], want_rec[bad][:5])
    assert np.array_equal(cand[cmp], want_cand[cmp])
    return int(near.sum())


@pytest.fixture(scope="module")
def family():
    """K = 3, 200 features per keyframe (no multiple of 16 or 64), P = 200, stereo and monocular features, depths 2 - 12 m; 8 seeds,
    both forms.  Computed once, shared, never modified."""
    fam = []
    for seed in SEEDS:
        kfs, pts, kf_mp = fm.make_scene(seed)
        c = dict(kfs=kfs, pts=pts, kf_mp=kf_mp)
        for sim3 in (False, True):
            rec, cand = run(kfs, pts, sim3)
            r32, c32, full, _ = fm.records(kfs, pts, TH, sim3, F32)
            _, _, _, near = fm.records(kfs, pts, TH, sim3, F64)
            c[sim3] = dict(rec=rec, cand=cand, r32=r32, c32=c32, full=full, near=near)
        fam.append(c)
    return fam


@pytest.mark.parametrize("sim3", [False, True])
def test_records_equal_the_float32_model(family, sim3):
    total = left_out = 0
    seen = set()
    for c in family:
        d = c[sim3]
        left_out += compare(d["rec"], d["cand"], d["r32"], d["c32"], d["near"])
        total += d["rec"].size
        seen |= set(d["rec"]["status"].ravel().tolist())
        assert (d["rec"]["n_cand"] >= 2).sum() > 20                      # windows with a choice to make
    print("fuse records (sim3_form=%d): %d records, %d left out as within 1e-6 of a threshold" % (sim3, total, left_out))
    assert left_out <= 0.01 * total
    assert seen == set(range(7))                                         # every `continue` of the reference occurs in the family


def test_forms_differ_where_the_reference_differs(family):
    """The Sim3 form has no chi2 gate: its candidate set contains the LocalMapping form's wherever both reach the window with the
    same projection (Scw = s [Rcw | tcw] projects a point where Tcw does, up to rounding)."""
    more = 0
    for c in family:
        a, b = c[False]["rec"], c[True]["rec"]
        both = (a["status"] == 0) & (b["status"] == 0) & (a["level"] == b["level"])
        assert (b["n_cand"][both] >= a["n_cand"][both]).mean() > 0.95
        more += (b["n_cand"][both] > a["n_cand"][both]).sum()
        none = b["status"] == fm.NO_CANDIDATE
        assert (b["best_dist"][none] == fm.INT_MAX).all() and (a["best_dist"][a["status"] == fm.NO_CANDIDATE] == 256).all()
    assert more > 0


def test_skip_is_honoured(family):
    c = family[0]
    rng = np.random.default_rng(5)
    skip = (rng.random((3, 200)) < 0.3).astype(np.uint8)
    rec, cand = run(c["kfs"], c["pts"], skip=skip)
    s = skip.astype(bool)
    assert (rec["status"][s] == fm.SKIPPED).all() and (rec["best_idx"][s] == -1).all() and (rec["n_cand"][s] == 0).all()
    assert (cand[s] == 0xFFFF).all()
    assert np.array_equal(rec[~s], c[False]["rec"][~s]) and np.array_equal(cand[~s], c[False]["cand"][~s])
    # bad / skip of the points view skip a point for every keyframe
    view, keep = fm.device_points(c["pts"])
    bad = np.zeros(200, np.uint8); bad[::7] = 1
    view.bad = capi.ptr(bad)
    rec2, _ = api.Fuse([fm.device_keyframe(k) for k in c["kfs"]], (view, keep), th=TH)
    assert (rec2["status"][:, ::7] == fm.SKIPPED).all()
    keepm = np.ones(200, bool); keepm[::7] = False
    assert np.array_equal(rec2[:, keepm], c[False]["rec"][:, keepm])


def test_degenerate_shapes(family):
    c = family[1]
    kfs, pts = c["kfs"], c["pts"]
    one = {f: pts[f][17:18] for f in pts}
    rec, cand = run(kfs[1:2], one)                                       # K = 1, P = 1
    assert rec.shape == (1, 1) and rec[0, 0] == c[False]["rec"][1, 17] and np.array_equal(cand[0, 0], c[False]["cand"][1, 17])
    rec, cand = run(kfs[:1], pts)                                        # K = 1
    assert np.array_equal(rec, c[False]["rec"][:1]) and np.array_equal(cand, c[False]["cand"][:1])
    none = {f: pts[f][:0] for f in pts}
    rec, cand = run(kfs, none)                                           # P = 0
    assert rec.shape == (3, 0) and cand.shape == (3, 0, capi.FUSE_CAND_CAP)
    rec, cand = run([], pts)                                             # K = 0
    assert rec.shape == (0, 200)
    empty = fm.finish(fm.keyframe(np.eye(3), np.zeros(3), 0))            # a keyframe without features: every window is empty
    empty["Tcw"], empty["Ow"] = kfs[0]["Tcw"], kfs[0]["Ow"]
    rec, _ = run([empty], pts)
    want, _, _, _ = fm.records([empty], pts, TH, False, F32)
    assert np.array_equal(rec, want) and fm.EMPTY_WINDOW in rec["status"]


def test_more_than_one_workgroup_per_keyframe():
    """P = 700: three workgroups per keyframe, the last one partly filled; 333 features."""
    kfs, pts, _ = fm.make_scene(20, K=2, n=333, P=700)
    for sim3 in (False, True):
        rec, cand = run(kfs, pts, sim3)
        r32, c32, _, _ = fm.records(kfs, pts, TH, sim3, F32)
        _, _, _, near = fm.records(kfs, pts, TH, sim3, F64)
        assert compare(rec, cand, r32, c32, near) <= 0.01 * rec.size


def test_negative_predicted_level_is_clamped_to_zero():
    """A pyramid with scale factor 1.1: points whose ratio lies between 1 / 1.2 and 1 / 1.1 pass the distance gate with ceil(q) = -1
    and must come out at level 0 (PredictScale's lower clamp); q = -0.5 gives -0, q = 0.5 and 1.5 levels 1 and 2."""
    kfs, pts = fm.low_scale_factor_scene(qs=(-1.5, -1.2, -0.5, 0.5, 1.5),
                                         features=((367.0, 248.0, 0, -1.0, 3), (368.0, 247.0, 1, -1.0, 1), (366.0, 249.0, 2, 300.0, 0)))
    kfs = [kfs]
    for sim3 in (False, True):
        rec, cand = run(kfs, pts, sim3)
        r32, c32, _, _ = fm.records(kfs, pts, TH, sim3, F32)
        _, _, _, near = fm.records(kfs, pts, TH, sim3, F64)
        assert not near.any()
        assert np.array_equal(rec, r32) and np.array_equal(cand, c32)
        assert rec["level"][0].tolist() == [0, 0, 0, 1, 2] and (rec["status"][0, :2] == fm.CANDIDATES).all()


def crowded_scene():
    """40 features of one level within 2 px of a point's projection (and 5 of a level the gate rejects in between): more candidates
    than the list holds."""
    kf = fm.keyframe(np.eye(3), np.zeros(3), 60)
    rng = np.random.default_rng(3)
    X = np.array([[0.4192, -0.0328, 5.0], [-1.0, 0.5, 6.0]])             # point 0 projects onto a corner of four grid cells
    pts = fm.points(X, X / np.linalg.norm(X, axis=1)[:, None], np.linalg.norm(X, axis=1) / 1.2 ** 5.5, np.linalg.norm(X, axis=1) * 1.2 ** 1.5,
                    rng.integers(0, 256, (2, 32), dtype=np.uint8))
    u, v = fm.FX * X[0, 0] / X[0, 2] + fm.CX, fm.FY * X[0, 1] / X[0, 2] + fm.CY
    kf["kps"]["x"] = u + rng.uniform(-2, 2, 60) * 0.7
    kf["kps"]["y"] = v + rng.uniform(-2, 2, 60) * 0.7
    kf["kps"]["octave"] = 2
    kf["kps"]["octave"][40:45] = 5
    kf["kps"]["x"][45:] = rng.uniform(20, 700, 15); kf["kps"]["y"][45:] = rng.uniform(20, 450, 15)
    order = rng.permutation(60)
    kf["kps"] = kf["kps"][order]
    kf["desc"] = rng.integers(0, 256, (60, 32), dtype=np.uint8)
    kf["Scw"] = np.eye(4, dtype=F32)
    return [fm.finish(kf)], pts


def test_crowded_window_counts_exactly_and_lists_the_first_cap():
    kfs, pts = crowded_scene()
    rec, cand = run(kfs, pts)
    r32, c32, full, _ = fm.records(kfs, pts, TH, False, F32)
    assert r32["n_cand"][0, 0] > capi.FUSE_CAND_CAP and r32["n_cand"][0, 0] >= 38
    assert np.array_equal(rec, r32) and np.array_equal(cand, c32)
    assert cand[0, 0].tolist() == full[0][0][: capi.FUSE_CAND_CAP]
    # the single-pair re-evaluation with a new descriptor equals the model
    new = pts["desc"].copy(); new[0] = np.random.default_rng(9).integers(0, 256, 32, dtype=np.uint8)
    one = {f: (new if f == "desc" else pts[f])[0:1] for f in pts}
    rec1, _ = run(kfs, one)
    want = fm.evaluate_pair(kfs[0], dict(pts, desc=new), 0, TH, False, F32)
    assert (rec1["best_idx"][0, 0], rec1["best_dist"][0, 0], rec1["n_cand"][0, 0]) == (want["best_idx"], want["best_dist"], len(want["cand"]))
    assert want["best_idx"] == fm.rescore(full[0][0], kfs[0]["desc"], new[0])[0]


def test_replay_with_descriptors_changed_midway_equals_the_serial_run(family):
    """The device's records + candidate lists through the model's replay (rescoring where a point's descriptor is no longer the one
    uploaded) against the reference's loop run serially on the same state, target by target."""
    rescored = 0
    for c in family[:4]:
        kfs, pts, kf_mp = c["kfs"], c["pts"], c["kf_mp"]
        P = len(pts["pos"])
        ids = np.arange(P)
        a, b = fm.Replay(kfs, kf_mp, pts["desc"]), fm.Replay(kfs, kf_mp, pts["desc"])
        for rp in (a, b):                                               # some descriptors are no longer the uploaded ones at entry
            rp.desc[::5] = kfs[0]["desc"][: len(rp.desc[::5])]
        skip = np.array([[a.skipped(k, p) for p in ids] for k in range(len(kfs))], np.uint8)
        rec, cand = run(kfs, pts, skip=skip)
        counters = {}
        fused_a, fused_b = [], []
        for k in range(len(kfs)):
            def reeval(i, desc, k=k):
                o = fm.evaluate_pair(kfs[k], pts, i, TH, False, F32, desc=desc)
                return o["best_idx"], o["best_dist"]
            fused_a.append(fm.replay_records(a, k, ids, rec[k], cand[k], pts["desc"], reeval, counters))
            fused_b.append(fm.serial_fuse(b, k, ids, pts, TH, F32))
        assert fused_a == fused_b and sum(fused_a) > 20
        assert a.state() == b.state()
        assert a.bad.sum() > 0                                           # points were replaced, and met again in a later keyframe
        rescored += counters.get("rescored", 0)
    assert rescored > 20


def test_two_runs_are_bit_equal(family):
    c = family[2]
    for sim3 in (False, True):
        rec, cand = run(c["kfs"], c["pts"], sim3)
        assert rec.tobytes() == c[sim3]["rec"].tobytes() and cand.tobytes() == c[sim3]["cand"].tobytes()


def test_two_threads_at_once(family):
    out = {}

    def work(j):
        c = family[j]
        dev = [fm.device_keyframe(k) for k in c["kfs"]]
        for _ in range(3):
            out[j] = run(c["kfs"], c["pts"], dev=dev)

    ts = [threading.Thread(target=work, args=(j,)) for j in (3, 4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for j in (3, 4):
        assert out[j][0].tobytes() == family[j][False]["rec"].tobytes() and out[j][1].tobytes() == family[j][False]["cand"].tobytes()


def test_refusals_on_the_device(family):
    """What needs a frame to be reached: K above the cap, NULL outputs, keyframes on two devices."""
    import ctypes as C
    lib = capi.load()
    c = family[0]
    dev = [fm.device_keyframe(k) for k in c["kfs"]]
    view, keep = fm.device_points(c["pts"])
    p = capi.FuseParams(); p.struct_size, p.th = C.sizeof(capi.FuseParams), TH
    arr = (capi.FuseKF * 513)()
    for k in range(513):
        dev[k % 3].fill(arr[k])
    rec = np.zeros((513, 200), capi.FUSE_RECORD_DTYPE); cand = np.zeros((513, 200, 16), np.uint16)
    assert lib.orbm_fuse(C.byref(arr), 513, C.byref(view), None, C.byref(p), capi.ptr(rec), capi.ptr(cand)) == capi.ORBG_CAP_EXCEEDED
    assert lib.orbm_fuse(C.byref(arr), 3, C.byref(view), None, C.byref(p), None, capi.ptr(cand)) == capi.ORBG_BAD_ARG
    assert lib.orbm_fuse(C.byref(arr), 3, C.byref(view), None, C.byref(p), capi.ptr(rec), None) == capi.ORBG_BAD_ARG
    assert lib.orbm_fuse(C.byref(arr), 512, C.byref(view), None, C.byref(p), capi.ptr(rec), capi.ptr(cand)) == capi.ORBG_OK
    assert np.array_equal(rec[509], c[False]["rec"][509 % 3])
    if lib.orbg_device_count() >= 2:
        other = fm.device_keyframe(c["kfs"][1], device=1)
        other.fill(arr[1])
        assert lib.orbm_fuse(C.byref(arr), 3, C.byref(view), None, C.byref(p), capi.ptr(rec), capi.ptr(cand)) == capi.ORBG_BAD_ARG
