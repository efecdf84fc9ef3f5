"""The staging block of the entry points (csrc/common.hpp, StageBlock over csrc/stage_layout.hpp) across a reallocation: every site
makes a small call, a larger one that forces its block to grow, and the small one again -- all on ONE thread (the sites whose buffers
belong to the calling thread) or ONE handle (Frame, LocalMap, LastFrameOnDevice).  Every call's outputs must equal, byte for byte,
those of the same call made FIRST on a fresh thread / fresh handles.  With -s every call prints a SHA-256 of its outputs."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import fuse_model as fm
import mlpnp_model as mm
import newpoints_model as nm
import sim3_opt_model as om
import two_view_model as tm
from multi_orbslam3_amd import _capi as capi, api, synth, views

pytestmark = pytest.mark.gpu
CAM = (500.0, 500.0, 320.0, 240.0, 40.0, 0.08)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
EYE = np.eye(4, dtype=np.float32)


def _arrays(x):
    """The arrays of a result, in a fixed order."""
    if x is None:
        return []
    if isinstance(x, np.ndarray):
        return [x]
    if isinstance(x, bytes):
        return [np.frombuffer(x, np.uint8)]
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in _arrays(x[k])]
    if isinstance(x, (list, tuple)):
        return [a for v in x for a in _arrays(v)]
    if hasattr(x, "__dict__"):
        return _arrays({k: v for k, v in vars(x).items() if k not in ("prob", "problem")})
    return [np.asarray(x)]


def _bits(result):
    return [(a.dtype.str, a.shape, np.ascontiguousarray(a).tobytes()) for a in _arrays(result)]


def _digest(bits):
    h = hashlib.sha256()
    for dt, shape, raw in bits:
        h.update(repr((dt, shape)).encode())
        h.update(raw)
    return h.hexdigest()


def _on_one_thread(calls):
    """The calls one after the other on a NEW thread (its work areas start empty and are released when it ends)."""
    got, err = [], []

    def work():
        try:
            for c in calls:
                got.append(_bits(c()))
        except BaseException as e:       # noqa: BLE001 -- reported by the caller
            err.append(repr(e))
    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert not err, err
    return got


def _check(name, seq, fresh):
    assert len(seq) == len(fresh) and all(seq)
    for i, (a, b) in enumerate(zip(seq, fresh)):
        print("\nsha256 %-28s call %d  %s" % (name, i, _digest(a)), end="")
        assert a == b, (name, i)


def _thread_case(name, calls):
    _check(name, _on_one_thread(calls), [_on_one_thread([c])[0] for c in calls])


def _handle_case(name, make_handles, calls):
    """calls: functions of the handles, each returning (.., .., nmatches) or a dict; one set of handles for the sequence, a fresh set per
    call for the reference.  The large call must have found something."""
    h = make_handles()
    res = [c(*h) for c in calls]
    assert res[1]["track_in_view"].all() if isinstance(res[1], dict) else res[1][2] > 0, name
    seq = [_bits(r) for r in res]
    fresh = []
    for c in calls:
        g = make_handles()
        fresh.append(_bits(c(*g)))
        for x in g:
            x.close()
    for x in h:
        x.close()
    _check(name, seq, fresh)


# ------------------------------------------------------------------ sites with the calling thread's buffers

def _pose_call(n, seed):
    pr = synth.make_pose_opt_problem(n=n, outlier_frac=0.1, mono_frac=0.5, seed=seed)
    p, keep = views.pose_opt_problem(pr["Xw"], pr["u"], pr["v"], pr["ur"], pr["inv_sigma2"], pr["cam"], pr["Tcw"])
    lib = capi.load()

    def call(p=p, keep=keep):
        out = views.PoseOptOutput(p.n)
        capi.check(lib.pose_optimize(C.byref(p), C.byref(out.c)), "pose_optimize")
        return [out.Tcw, out.outliers, np.array(out.iters), np.array(out.chi2), np.array([out.c.n_inliers, out.c.n_bad])]
    return call


@pytest.mark.parametrize("sizes", [(5, 301, 5), (1025, 7)])
def test_pose_optimize(sizes):
    """(1025, 7): from the device-copy branch (n > 1024) back to the kernel reading the pinned block in place."""
    small = _pose_call(sizes[0], 150)
    calls = [small, _pose_call(sizes[1], 151)] + ([small] if len(sizes) == 3 else [])
    _thread_case("pose_optimize %s" % (sizes,), calls)


def test_fuse():
    def call(K, P, seed, with_skip):
        kfs, pts, _ = fm.make_scene(seed, K=K, n=200, P=P)
        dk, dp = [fm.device_keyframe(k) for k in kfs], fm.device_points(pts)
        skip = (np.random.default_rng(seed).random((K, P)) < 0.3).astype(np.uint8) if with_skip else None
        return lambda: api.Fuse(dk, dp, th=3.0, skip=skip)
    small = call(1, 3, 40, False)
    _thread_case("orbm_fuse", [small, call(2, 203, 41, True), small])


def test_create_new_map_points():
    def call(seed, **kw):
        k1, nbs = nm.make_scene(seed, **kw)
        d1, dn = nm.device_keyframe(k1), [nm.device_keyframe(k) for k in nbs]
        return lambda: api.CreateNewMapPoints(d1, dn, check_orientation=True)
    small = call(50, n=60, B=1)
    _thread_case("CreateNewMapPoints", [small, call(51, n=200, B=3, n2=[200, 0, 130]), small])      # (a neighbour with an empty feature vector)


def test_sim3_optimize_batch():
    def problem(seed, n):
        m = om.make_problem(seed, max(n, 10), seed % 2 == 0, 0.2)
        return api.Sim3OptProblem(m.X1[:n], m.X2[:n], m.obs1[:n], m.obs2[:n], m.w1[:n], m.w2[:n], m.K1, m.K2, m.fix_scale, m.th2, m.q, m.t, m.s,
                                  n_correspondences=n)

    def call(probs):
        def run():
            out = []
            for r in api.OptimizeSim3.batch(probs):
                out += [np.array([r.nIn, r.returned_early, r.n_bad_round1]), r.q, r.t, np.float64(r.s), r.removed, np.array(r.iters),
                        np.float64(r.chi2), r.trace]
            return out
        return run
    small = call([problem(60, 10)])
    _thread_case("orbm_sim3_optimize_batch", [small, call([problem(61, 0), problem(62, 33), problem(63, 65)]), small])


def test_mlpnp_solve_batch():
    reloc = (0.99, 10, 300, 6, 0.5, 5.991)                    # S/Tracking.cc:3401: 7 correspondences are below min_inliers, no launch

    def call(ns, seed):
        rng = np.random.default_rng(seed)
        probs, drw = [], []
        for b, n in enumerate(ns):
            sc = mm.make_scene(seed + b, n, 0.3)
            probs.append(api.MLPnPProblem(sc["P2D"], sc["sigma2"], sc["bearing"], sc["P3Dw"], sc["K"], sc["kp_index"], sc["m"]))
            drw.append(mm.draws(max(n, 6), mm.ransac_iterations(n, *reloc[:5])[0], rng))
        return lambda: [(r.fields(), r.hyp_n_inliers, r.hyp_R, r.hyp_t, r.hyp_masks)
                        for r in api.MLPnPsolver.solve_batch(probs, [reloc] * len(ns), drw, per_hypothesis=True)]
    small = call([40], 70)
    _thread_case("orbp_mlpnp_solve_batch", [small, call([120, 7, 65], 71), small])


def test_two_view_reconstruct():
    def call(N, H, seed):
        sc = tm.scene("3d", N, seed, n_extra1=3, n_extra2=5)
        keys1, keys2, m12 = sc.keys1, sc.keys2, sc.matches12
        d = tm.case_draws(N, H, seed)
        tv = api.TwoViewReconstruction(tm.CAM, 1.0, H)
        return lambda: tv.Reconstruct(keys1, keys2, m12, draws=d, per_hypothesis=True)
    small = call(8, 1, 80)
    _thread_case("orbi_two_view_reconstruct", [small, call(130, 65, 81), small])


def test_fisheye_stereo_matches():
    def call(n_stereo, seed):
        fs = synth.make_fisheye_stereo_scene(n_stereo=n_stereo, n_mono_left=5, n_mono_right=5, n_distract=5, seed=seed)
        v, keep = views.fisheye_stereo_view(fs["kps_left"], fs["desc_left"], fs["mono_left"], fs["kps_right"], fs["desc_right"], fs["mono_right"],
                                            fs["left"], fs["right"], fs["Tlr"], fs["level_sigma2"])

        def run(v=v, keep=keep):
            g = api.ComputeStereoFishEyeMatches(v)
            return [g[0], g[1], g[2], g[3], np.array(g[4])]
        return run
    small = call(20, 90)
    _thread_case("orbx_fisheye_stereo_matches", [small, call(300, 91), small])


# ------------------------------------------------------------------ sites with a handle's buffers

def _world(m, seed):
    """m map points in front of a camera at the origin, with the distance range and the viewing direction of an observation from there."""
    rng = np.random.default_rng(seed)
    f = np.float32
    px = np.stack([rng.uniform(20, 620, m), rng.uniform(20, 460, m)], 1)
    z = rng.uniform(2.0, 10.0, m)
    pos = np.stack([(px[:, 0] - CAM[2]) / CAM[0] * z, (px[:, 1] - CAM[3]) / CAM[1] * z, z], 1).astype(f)
    dist = np.linalg.norm(pos, axis=1)
    octave = rng.integers(0, 4, m).astype(np.int32)
    max_dist = dist * 1.2 ** (octave - 0.5)                       # PredictScale from the origin gives `octave`
    return dict(pos=pos, normal=(pos / dist[:, None]).astype(f), min_dist=(dist * 0.2).astype(f), max_dist=max_dist.astype(f),
                desc=rng.integers(0, 256, (m, 32), dtype=np.uint8), px=px.astype(f), z=z.astype(f), octave=octave,
                n_obs=np.ones(m, np.int32), bad=np.zeros(m, np.uint8))


def _world_view(w, m):
    return views.worldpoints_view(w["pos"][:m], w["normal"][:m], w["min_dist"][:m], w["max_dist"][:m], w["desc"][:m], w["n_obs"][:m], w["bad"][:m])


def _frame_of(w, n, seed):
    """A Frame at the identity pose that observes the first n points of w (a pixel of noise, a few descriptor bits flipped)."""
    rng = np.random.default_rng(seed)
    kps = np.zeros(n, capi.KEYPOINT_DTYPE)
    kps["x"] = w["px"][:n, 0] + rng.normal(0, 0.7, n)
    kps["y"] = w["px"][:n, 1] + rng.normal(0, 0.7, n)
    kps["octave"] = w["octave"][:n]
    kps["angle"] = rng.uniform(0, 360, n)
    kps["size"] = 31
    desc = w["desc"][:n].copy()
    desc[:, 0] ^= rng.integers(0, 8, n, dtype=np.uint8)
    depth = w["z"][:n].copy()
    uright = (kps["x"] - np.float32(CAM[4]) / depth).astype(np.float32)
    fv, keep = views.frame_view(kps, desc, uright, depth, BOUNDS, CAM, 8, 1.2)
    return api.Frame(cap_features=16).upload(fv, keep)


@pytest.fixture(scope="module")
def world():
    return _world(5000, 100)


def test_is_in_frustum_on_one_frame(world):
    views_ = [_world_view(world, m) for m in (1, 17, 1)]
    _handle_case("orbm_is_in_frustum", lambda: (_frame_of(world, 700, 101),), [lambda F, v=v: F.isInFrustum(EYE, v[0]) for v in views_])


def test_search_by_projection_mps_on_one_frame(world):
    """4200 features: beyond the occupancy bitmask, so mvpMapPoints travels through the block's device copy."""
    n = 4200
    probe = _frame_of(world, n, 102)
    mvs = []
    for m in (1, 500, 1):
        t = probe.isInFrustum(EYE, _world_view(world, m)[0])
        mvs.append(views.mappoints_view(t["track_in_view"], world["bad"][:m], t["proj_x"], t["proj_y"], t["proj_xr"], t["track_depth"],
                                        t["scale_level"], t["view_cos"], world["desc"][:m], world["n_obs"][:m]))
    probe.close()
    amp = np.full(n, -1, np.int32); amp[::9] = 7
    aob = np.ones(n, np.int32)
    matcher = api.ORBmatcher(0.8)
    _handle_case("orbm_search_by_projection_mps", lambda: (_frame_of(world, n, 102),),
                 [lambda F, mv=mv: matcher.SearchByProjection(F, mv[0], th=3.0, assigned_mp=amp, assigned_obs=aob) for mv in mvs])


def test_map_upload_then_search(world):
    n = 700
    amp, aob = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    matcher = api.ORBmatcher(0.8)
    wvs = [_world_view(world, m) for m in (1, 1000, 1)]

    def call(F, M, wv):
        M.upload(wv[0])
        vis = np.zeros(wv[0].m, np.uint8)
        return list(matcher.SearchLocalPoints(F, M, EYE, th=3.0, assigned_mp=amp, assigned_obs=aob, in_frustum=vis)) + [vis]
    _handle_case("orbm_map_upload + search", lambda: (_frame_of(world, n, 103), api.LocalMap(cap_points=1)),
                 [lambda F, M, wv=wv: call(F, M, wv) for wv in wvs])


def test_lastview_upload_then_search(world):
    n = 700
    amp, aob = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    matcher = api.ORBmatcher(0.9, True)
    rng = np.random.default_rng(104)
    lvs = [views.lastframe_view(np.ones(m, np.uint8), np.zeros(m, np.uint8), world["pos"][:m], world["desc"][:m], world["octave"][:m],
                                rng.uniform(0, 360, m).astype(np.float32), world["n_obs"][:m], EYE) for m in (1, 1000, 1)]

    def call(F, V, lv):
        V.upload(lv[0])
        return matcher.SearchByProjectionFrameResident(F, EYE, V, 15.0, False, amp, aob)
    _handle_case("orbm_lastview_upload + search", lambda: (_frame_of(world, n, 105), api.LastFrameOnDevice(cap_features=16)),
                 [lambda F, V, lv=lv: call(F, V, lv) for lv in lvs])


def test_this_file_with_poisoned_allocations():
    """ORBG_POISON=1 fills every new device / pinned buffer with 0xA5: padding between slots and the grown blocks start as garbage, and
    every case above must still give the same bytes as its fresh run (a fresh child process; this test is left out there)."""
    env = dict(os.environ, ORBG_POISON="1")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", here, "-k", "not poisoned_allocations"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=os.path.dirname(os.path.dirname(here)))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
