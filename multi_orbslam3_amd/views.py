"""Builders for the flattened views of include/orbgpu.h from numpy arrays.

Each builder returns (ctypes struct, keepalive list): the struct only holds raw pointers, so the
caller must keep the keepalive list referenced while the struct is in use.
"""
import ctypes as C

import numpy as np

from . import _capi as capi


def _c(a, dtype):
    if a is None:
        return None
    return np.ascontiguousarray(a, dtype=dtype)


def frame_view(kps, desc, uright=None, depth=None, bounds=None, cam=None, n_levels=8, scale_factor=1.2):
    """bounds = (min_x, max_x, min_y, max_y); cam = (fx, fy, cx, cy, bf, b)."""
    kps = np.ascontiguousarray(kps, dtype=capi.KEYPOINT_DTYPE)
    desc = _c(desc, np.uint8)
    uright = _c(uright, np.float32)
    depth = _c(depth, np.float32)
    v = capi.FrameView()
    v.n = len(kps)
    v.kps, v.desc, v.uright, v.depth = capi.ptr(kps), capi.ptr(desc), capi.ptr(uright), capi.ptr(depth)
    v.min_x, v.max_x, v.min_y, v.max_y = [float(b) for b in bounds]
    v.fx, v.fy, v.cx, v.cy, v.bf, v.b = [float(c) for c in cam]
    v.n_levels = int(n_levels)
    v.scale_factor = float(scale_factor)
    return v, [kps, desc, uright, depth]


def mappoints_view(track_in_view, bad, proj_x, proj_y, proj_xr, track_depth, scale_level, view_cos, desc, n_obs):
    arrs = [_c(track_in_view, np.uint8), _c(bad, np.uint8), _c(proj_x, np.float32), _c(proj_y, np.float32),
            _c(proj_xr, np.float32), _c(track_depth, np.float32), _c(scale_level, np.int32),
            _c(view_cos, np.float32), _c(desc, np.uint8), _c(n_obs, np.int32)]
    v = capi.MapPointsView()
    v.m = len(arrs[0])
    (v.track_in_view, v.bad, v.proj_x, v.proj_y, v.proj_xr, v.track_depth, v.scale_level, v.view_cos, v.desc,
     v.n_obs) = [capi.ptr(a) for a in arrs]
    return v, arrs


def worldpoints_view(pos, normal, min_dist, max_dist, desc, n_obs, bad, skip=None):
    arrs = [_c(pos, np.float32), _c(normal, np.float32), _c(min_dist, np.float32), _c(max_dist, np.float32),
            _c(desc, np.uint8), _c(n_obs, np.int32), _c(bad, np.uint8), _c(skip, np.uint8)]
    v = capi.WorldPointsView()
    v.m = len(arrs[2])
    v.pos, v.normal, v.min_dist, v.max_dist, v.desc, v.n_obs, v.bad, v.skip = [capi.ptr(a) for a in arrs]
    return v, arrs


def lastframe_view(mp_valid, outlier, world_pos, desc, octave, angle, n_obs, Tcw):
    arrs = [_c(mp_valid, np.uint8), _c(outlier, np.uint8), _c(world_pos, np.float32), _c(desc, np.uint8),
            _c(octave, np.int32), _c(angle, np.float32), _c(n_obs, np.int32)]
    v = capi.LastFrameView()
    v.n = len(arrs[0])
    v.mp_valid, v.outlier, v.world_pos, v.desc, v.octave, v.angle, v.n_obs = [capi.ptr(a) for a in arrs]
    T = np.asarray(Tcw, dtype=np.float32).reshape(16)
    for i in range(16):
        v.Tcw[i] = float(T[i])
    return v, arrs


def featvec_view(node_id, start, feat_idx):
    arrs = [_c(node_id, np.uint32), _c(start, np.uint32), _c(feat_idx, np.uint32)]
    v = capi.FeatVecView()
    v.n_nodes = len(arrs[0])
    v.node_id, v.start, v.feat_idx = [capi.ptr(a) for a in arrs]
    return v, arrs


def featvec_from_nodes(node_of_feature):
    """Group feature indices by node id (ascending), as DBoW2::FeatureVector does (std::map + push_back)."""
    node_of_feature = np.asarray(node_of_feature, dtype=np.int64)
    order = np.argsort(node_of_feature, kind="stable")
    nodes, counts = np.unique(node_of_feature, return_counts=True)
    start = np.zeros(len(nodes) + 1, dtype=np.uint32)
    start[1:] = np.cumsum(counts)
    return nodes.astype(np.uint32), start, order.astype(np.uint32)


def vocab_view(child_start, child_ids, desc, weight, word_id, L, weighting=capi.ORBV_TF_IDF, scoring_norm=capi.ORBV_NORM_L1):
    """DBoW2 vocabulary tree flattened (include/orbgpu.h: orbv_vocab_view)."""
    arrs = [_c(child_start, np.int32), _c(child_ids, np.int32), _c(desc, np.uint8), _c(weight, np.float64), _c(word_id, np.int32)]
    v = capi.VocabView()
    v.n_nodes = len(arrs[0]) - 1
    v.L, v.weighting, v.scoring_norm = int(L), int(weighting), int(scoring_norm)
    v.child_start, v.child_ids, v.desc, v.weight, v.word_id = [capi.ptr(a) for a in arrs]
    return v, arrs


def camera_rig(left, right=None, Trl=None):
    """orbg_camera_rig from (model, fx, fy, cx, cy[, k1, k2, k3, k4]) tuples: mpCamera, mpCamera2 and mTrl (3x4 or 4x4)."""
    rig = capi.CameraRig()

    def fill(dst, cam):
        dst.model = int(cam[0])
        dst.fx, dst.fy, dst.cx, dst.cy = [float(np.float32(c)) for c in cam[1:5]]
        ks = list(cam[5:9]) + [0.0] * (4 - len(cam[5:9]))
        for i in range(4):
            dst.k[i] = float(np.float32(ks[i]))

    fill(rig.left, left)
    rig.has_right = 0 if right is None else 1
    if right is not None:
        fill(rig.right, right)
        T = np.asarray(Trl, np.float32).reshape(-1)[:12]
        for i in range(12):
            rig.Trl[i] = float(T[i])
    return rig


def fisheye_stereo_view(kps_left, desc_left, mono_left, kps_right, desc_right, mono_right, left, right, Tlr, level_sigma2):
    """orbx_fisheye_stereo_view: mvKeys / mvKeysRight with their descriptors, monoLeft / monoRight (the lapping-area features sit
    behind them), the two KannalaBrandt8 cameras as (model, fx, fy, cx, cy, k1..k4) tuples, mTlr (3x4 or 4x4), mvLevelSigma2."""
    kl = np.ascontiguousarray(kps_left, dtype=capi.KEYPOINT_DTYPE); kr = np.ascontiguousarray(kps_right, dtype=capi.KEYPOINT_DTYPE)
    dl = _c(desc_left, np.uint8); dr = _c(desc_right, np.uint8); sg = _c(level_sigma2, np.float32)
    v = capi.FisheyeStereoView()
    v.n_left, v.n_right, v.mono_left, v.mono_right = len(kl), len(kr), int(mono_left), int(mono_right)
    v.kps_left, v.kps_right, v.desc_left, v.desc_right, v.level_sigma2 = capi.ptr(kl), capi.ptr(kr), capi.ptr(dl), capi.ptr(dr), capi.ptr(sg)
    v.n_levels = len(sg)
    rig = camera_rig(left, right, np.eye(4)[:3])
    v.left, v.right = rig.left, rig.right
    T = np.asarray(Tlr, np.float32).reshape(-1)[:12]
    for i in range(12):
        v.Tlr[i] = float(T[i])
    return v, [kl, kr, dl, dr, sg]


def lba_problem(poses, pose_fixed, points, edges, cam, lambda_init=0.0, its=(5, 10), device=0, rig=None):
    """poses: (P,16) or (P,4,4) float32; edges: structured EDGE_DTYPE; cam = (fx, fy, cx, cy, bf); rig: camera_rig(...) or None."""
    poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float32).reshape(-1, 16))
    pose_fixed = _c(pose_fixed, np.uint8)
    points = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3))
    edges = np.ascontiguousarray(edges, dtype=capi.EDGE_DTYPE)
    p = capi.LbaProblem()
    p.n_poses, p.n_points, p.n_edges = len(poses), len(points), len(edges)
    p.poses, p.pose_fixed, p.points, p.edges = capi.ptr(poses), capi.ptr(pose_fixed), capi.ptr(points), capi.ptr(edges)
    p.fx, p.fy, p.cx, p.cy, p.bf = [float(c) for c in cam]
    p.lambda_init = float(lambda_init)
    p.its_round1, p.its_round2 = int(its[0]), int(its[1])
    p.device = int(device)
    if rig is not None:
        p.rig = C.pointer(rig)
    return p, [poses, pose_fixed, points, edges, rig]


class LbaOutput:
    """Owns the result arrays of one LBA call."""

    def __init__(self, n_poses, n_points, n_edges, trace_cap=64):
        self.poses = np.zeros((n_poses, 16), dtype=np.float32)
        self.points = np.zeros((n_points, 3), dtype=np.float32)
        self.edge_chi2 = np.zeros(n_edges, dtype=np.float64)
        self.edge_depth_pos = np.zeros(n_edges, dtype=np.uint8)
        self.edge_outlier = np.zeros(n_edges, dtype=np.uint8)
        self.trace = np.zeros((trace_cap, 3), dtype=np.float64)
        r = capi.LbaResult()
        r.poses, r.points = capi.ptr(self.poses), capi.ptr(self.points)
        r.edge_chi2, r.edge_depth_pos, r.edge_outlier = capi.ptr(self.edge_chi2), capi.ptr(self.edge_depth_pos), capi.ptr(self.edge_outlier)
        r.trace, r.trace_cap, r.trace_len = capi.ptr(self.trace), trace_cap, 0
        self.c = r

    @property
    def status(self):
        return self.c.status

    @property
    def iters(self):
        return (self.c.iters_round1, self.c.iters_round2)

    @property
    def n_outliers(self):
        return self.c.n_outliers

    @property
    def chi2(self):
        return (self.c.chi2_initial, self.c.chi2_final)

    def trace_rows(self):
        return self.trace[: self.c.trace_len].copy()


def ba_cameras(cameras):
    """ba_camera array from a list of dicts / tuples: (fx, fy, cx, cy, bf) for a pinhole keyframe, or
    (fx, fy, cx, cy, bf, model) with model = (model id, fx, fy, cx, cy[, k1..k4]) as camera_rig takes it."""
    arr = (capi.BaCamera * max(len(cameras), 1))()
    for i, cam in enumerate(cameras):
        five = [float(np.float32(c)) for c in cam[:5]]
        arr[i].fx, arr[i].fy, arr[i].cx, arr[i].cy, arr[i].bf = five
        model = cam[5] if len(cam) > 5 and cam[5] is not None else (capi.CAM_PINHOLE,) + tuple(five[:4])
        arr[i].model = camera_rig(model).left
    return arr


def ba_problem(poses, pose_fixed, pose_camera, points, edges, cameras, iterations=10, robust=True, device=0):
    """Optimizer::BundleAdjustment's inputs (include/orbgpu.h: ba_problem).  poses: (P,16) or (P,4,4) float32; pose_camera: (P,)
    indices into cameras; edges: structured EDGE_DTYPE, per point its observations; cameras: see ba_cameras."""
    poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float32).reshape(-1, 16))
    pose_fixed = np.ascontiguousarray(pose_fixed, dtype=np.uint8)
    pose_camera = np.ascontiguousarray(pose_camera, dtype=np.int32)
    points = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3))
    edges = np.ascontiguousarray(edges, dtype=capi.EDGE_DTYPE)
    cams = cameras if isinstance(cameras, C.Array) else ba_cameras(cameras)
    p = capi.BaProblem()
    p.n_poses, p.n_points, p.n_edges, p.n_cameras = len(poses), len(points), len(edges), len(cameras)
    p.poses, p.pose_fixed, p.pose_camera, p.points, p.edges = [capi.ptr(a) for a in (poses, pose_fixed, pose_camera, points, edges)]
    p.cameras = C.cast(cams, C.c_void_p)
    p.iterations, p.robust, p.device = int(iterations), int(bool(robust)), int(device)
    return p, [poses, pose_fixed, pose_camera, points, edges, cams]


class BaOutput:
    """Owns the result arrays of one full-BA call."""

    def __init__(self, n_poses, n_points, n_edges, trace_cap=64):
        self.poses = np.zeros((n_poses, 16), dtype=np.float32)
        self.points = np.zeros((n_points, 3), dtype=np.float32)
        self.edge_chi2 = np.zeros(n_edges, dtype=np.float64)
        self.edge_depth_pos = np.zeros(n_edges, dtype=np.uint8)
        self.point_included = np.zeros(n_points, dtype=np.uint8)
        self.trace = np.zeros((trace_cap, 3), dtype=np.float64)
        r = capi.BaResult()
        r.poses, r.points = capi.ptr(self.poses), capi.ptr(self.points)
        r.edge_chi2, r.edge_depth_pos, r.point_included = capi.ptr(self.edge_chi2), capi.ptr(self.edge_depth_pos), capi.ptr(self.point_included)
        r.trace, r.trace_cap, r.trace_len = capi.ptr(self.trace), trace_cap, 0
        self.c = r

    @property
    def status(self):
        return self.c.status

    @property
    def iters(self):
        return self.c.iters

    @property
    def chi2(self):
        return (self.c.chi2_initial, self.c.chi2_final)

    def trace_rows(self):
        return self.trace[: self.c.trace_len].copy()


def ba_weld_problem(poses, pose_fixed, pose_camera, points, edges, cameras, iterations=5, iterations_second=10, chi2_mono=5.991,
                    chi2_stereo=7.815, device=0):
    """The welding BA's inputs (include/orbgpu.h: ba_weld_problem): ba_problem's arrays, round 1's and round 2's iteration counts and
    the two chi2 thresholds of the level test (S/Optimizer.cc:6598, 6652, 6620, 6640).  Round 1 is always robust and round 2 never is:
    there is no robust argument."""
    inner, keep = ba_problem(poses, pose_fixed, pose_camera, points, edges, cameras, iterations=iterations, robust=True, device=device)
    p = capi.BaWeldProblem()
    p.struct_size = C.sizeof(capi.BaWeldProblem)
    p.ba = inner
    p.iterations_second, p.chi2_mono, p.chi2_stereo = int(iterations_second), float(chi2_mono), float(chi2_stereo)
    return p, keep


class BaWeldOutput(BaOutput):
    """Owns the result arrays of one welding-BA call: BaOutput's (round 1's trace and counts, the final estimate, the final check's
    edge_chi2 / edge_depth_pos) plus edge_level and round 2's trace.  `c` stays the ba_result, `w` is the ba_weld_result around it."""

    def __init__(self, n_poses, n_points, n_edges, trace_cap=64, chi2_mono=5.991, chi2_stereo=7.815):
        super().__init__(n_poses, n_points, n_edges, trace_cap)
        self.edge_level = np.zeros(n_edges, dtype=np.uint8)
        self.trace_second = np.zeros((trace_cap, 3), dtype=np.float64)
        self.chi2_mono, self.chi2_stereo = float(chi2_mono), float(chi2_stereo)
        w = capi.BaWeldResult()
        w.struct_size = C.sizeof(capi.BaWeldResult)
        w.ba = self.c
        w.edge_level = capi.ptr(self.edge_level)
        w.trace_second, w.trace_second_cap, w.trace_second_len = capi.ptr(self.trace_second), trace_cap, 0
        self.w = w
        self.c = w.ba                                  # (a view into w, not a copy: the library writes there)
        self._ur = None

    @property
    def rounds_run(self):
        return self.w.rounds_run

    @property
    def n_level1(self):
        return self.w.n_level1

    @property
    def iters_second(self):
        return self.w.iters_second

    @property
    def chi2_second(self):
        return (self.w.chi2_initial_second, self.w.chi2_final_second)

    def trace_second_rows(self):
        return self.trace_second[: self.w.trace_second_len].copy()

    @property
    def to_erase(self):
        """Indices of the edges the reference's final check rejects (S/Optimizer.cc:6665-6705: chi2 above the threshold or a depth that
        is not positive), in its order: the monocular edges first, then the stereo ones, each in creation order."""
        mono = self._ur < 0
        bad = (self.edge_chi2 > np.where(mono, self.chi2_mono, self.chi2_stereo)) | (self.edge_depth_pos == 0)
        return np.concatenate([np.flatnonzero(bad & mono), np.flatnonzero(bad & ~mono)]).astype(np.int64)


def pose_opt_problem(Xw, u, v, ur, inv_sigma2, cam, Tcw, device=0, rig=None):
    """cam = (fx, fy, cx, cy, bf); Tcw = pFrame->mTcw (4x4); rig: camera_rig(...) or None."""
    arrs = [_c(np.asarray(Xw, np.float32).reshape(-1, 3), np.float32), _c(u, np.float32), _c(v, np.float32), _c(ur, np.float32),
            _c(inv_sigma2, np.float32)]
    p = capi.PoseOptProblem()
    p.n = len(arrs[1])
    p.Xw, p.u, p.v, p.ur, p.inv_sigma2 = [capi.ptr(a) for a in arrs]
    p.fx, p.fy, p.cx, p.cy, p.bf = [float(c) for c in cam]
    T = np.asarray(Tcw, np.float32).reshape(16)
    for i in range(16):
        p.Tcw[i] = float(T[i])
    p.device = int(device)
    if rig is not None:
        p.rig = C.pointer(rig)
        arrs.append(rig)
    return p, arrs


class PoseOptOutput:
    def __init__(self, n):
        self.outlier = np.zeros(max(n, 1), np.uint8)
        self.c = capi.PoseOptResult()
        self.c.outlier = capi.ptr(self.outlier)
        self.n = n

    @property
    def Tcw(self):
        return np.array(list(self.c.Tcw), np.float32).reshape(4, 4)

    @property
    def n_inliers(self):
        return self.c.n_inliers

    @property
    def iters(self):
        return tuple(self.c.iters)

    @property
    def chi2(self):
        return tuple(self.c.chi2)

    @property
    def outliers(self):
        return self.outlier[: self.n].copy()


def _fill(dst, src, dtype):
    a = np.asarray(src, dtype).reshape(-1)
    assert len(a) == len(dst), (len(a), len(dst))
    for i, x in enumerate(a):
        dst[i] = float(x)


def pose_inertial_problem(form, Xw, u, v, ur, inv_sigma2, close, cam, Tcb, frame, other, preint, info9, infoG, infoA, prior=None,
                          rec_init=False, device=0, n_left=-1):
    """pose_inertial_problem of include/orbgpu.h.  form: capi.POSE_INERTIAL_LAST_KEYFRAME / _LAST_FRAME; cam = (fx, fy, cx, cy, bf); Tcb:
    mImuCalib.Tcb (3 x 4 or 4 x 4); frame / other: dicts Rwb, twb, vwb, bg, ba; preint: dict dT, dR, dV, dP, JRg, JVg, JVa, JPg, JPa, bg, ba;
    info9 / infoG / infoA: orbg_imu_information(C); prior (LAST_FRAME): dict Rwb, twb, vwb, bg, ba, H (15 x 15, conditioned).
    Returns (problem, keep-alive list)."""
    arrs = [_c(np.asarray(Xw, np.float32).reshape(-1, 3), np.float32), _c(u, np.float32), _c(v, np.float32), _c(ur, np.float32),
            _c(inv_sigma2, np.float32), _c(close, np.uint8)]
    p = capi.PoseInertialProblem()
    p.struct_size = C.sizeof(capi.PoseInertialProblem)
    p.form, p.rec_init, p.device, p.n_left = int(form), int(bool(rec_init)), int(device), int(n_left)
    p.n = len(arrs[1])
    p.Xw, p.u, p.v, p.ur, p.inv_sigma2, p.close = [capi.ptr(a) for a in arrs]
    p.fx, p.fy, p.cx, p.cy, p.bf = [float(c) for c in cam]
    _fill(p.Tcb, np.asarray(Tcb, np.float32)[:3, :4], np.float32)
    for dst, src in ((p.frame, frame), (p.other, other)):
        for k in ("Rwb", "twb", "vwb", "bg", "ba"):
            _fill(getattr(dst, k), src[k], np.float32)
    p.preint.dT = float(preint["dT"])
    for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bg", "ba"):
        _fill(getattr(p.preint, k), preint[k], np.float32)
    _fill(p.info9, info9, np.float64)
    _fill(p.infoG, infoG, np.float64)
    _fill(p.infoA, infoA, np.float64)
    if prior is not None:
        c = capi.PoseInertialPrior()
        for k in ("Rwb", "twb", "vwb", "bg", "ba", "H"):
            _fill(getattr(c, k), prior[k], np.float64)
        p.prior = C.pointer(c)
        arrs.append(c)
    return p, arrs


class PoseInertialOutput:
    def __init__(self, n):
        self.outlier = np.zeros(max(n, 1), np.uint8)
        self.c = capi.PoseInertialResult()
        self.c.struct_size = C.sizeof(capi.PoseInertialResult)
        self.c.outlier = capi.ptr(self.outlier)
        self.n = n

    def as_dict(self):
        """the result in the layout of the numpy model (tests/pose_inertial_model.py)"""
        c = self.c
        return {"Rwb": np.array(list(c.Rwb)).reshape(3, 3), "twb": np.array(list(c.twb)), "vwb": np.array(list(c.vwb)),
                "bg": np.array(list(c.bg)), "ba": np.array(list(c.ba)), "outlier": self.outlier[: self.n].copy(),
                "n_inliers": c.n_inliers, "n_bad": c.n_bad, "rounds_run": c.rounds_run, "solve_failed": c.solve_failed,
                "chi2": list(c.chi2), "H": np.array(list(c.H)).reshape(15, 15)}


def inertial_ba_problem(keyframes, points, edges, close, cam, Tcb, rec_init=False, large=False, device=0):
    """inertial_ba_problem of include/orbgpu.h.  keyframes: a list of dicts -- state (dict Rwb, twb, vwb, bg, ba), fixed, imu, and for a
    keyframe with an inertial edge to its predecessor: prev (index into the list), preint (dict as for pose_inertial_problem), info9 /
    infoG / infoA (orbg_imu_information(C)), last_in_window; points: (n, 3) float32; edges: structured EDGE_DTYPE in creation order (pose =
    keyframe index); close: per point; cam = (fx, fy, cx, cy, bf); Tcb: mImuCalib.Tcb.  Returns (problem, keep-alive list)."""
    K = (capi.InertialBaKeyframe * max(len(keyframes), 1))()
    for i, kf in enumerate(keyframes):
        c = K[i]
        for k in ("Rwb", "twb", "vwb", "bg", "ba"):
            _fill(getattr(c.state, k), kf["state"][k], np.float32)
        c.fixed, c.imu = int(bool(kf["fixed"])), int(bool(kf["imu"]))
        c.link = int(kf.get("prev") is not None)
        c.prev = int(kf["prev"]) if c.link else -1
        c.last_in_window = int(bool(kf.get("last_in_window", False)))
        if c.link:
            c.preint.dT = float(kf["preint"]["dT"])
            for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bg", "ba"):
                _fill(getattr(c.preint, k), kf["preint"][k], np.float32)
            _fill(c.info9, kf["info9"], np.float64)
            _fill(c.infoG, kf["infoG"], np.float64)
            _fill(c.infoA, kf["infoA"], np.float64)
    pts = _c(np.asarray(points, np.float32).reshape(-1, 3), np.float32)
    E = np.ascontiguousarray(edges, capi.EDGE_DTYPE)
    cl = _c(close, np.uint8)
    assert len(cl) == len(pts)
    p = capi.InertialBaProblem()
    p.struct_size = C.sizeof(capi.InertialBaProblem)
    p.n_keyframes, p.n_points, p.n_edges = len(keyframes), len(pts), len(E)
    p.keyframes = C.addressof(K)
    p.points = capi.ptr(pts) if len(pts) else None
    p.edges = capi.ptr(E) if len(E) else None
    p.close = capi.ptr(cl) if len(cl) else None
    p.rec_init, p.large, p.device = int(bool(rec_init)), int(bool(large)), int(device)
    p.fx, p.fy, p.cx, p.cy, p.bf = [float(c) for c in cam]
    _fill(p.Tcb, np.asarray(Tcb, np.float32)[:3, :4], np.float32)
    return p, [K, pts, E, cl]


def inertial_init_problem(keyframes, edges, bg, ba, Rwg=None, scale=1.0, algorithm=0, iterations=200, lambda_init=0.0, free_velocity=True,
                          free_bias=True, free_gdir=True, free_scale=True, with_priors=True, prior_g=0.0, prior_a=0.0, device=0):
    """inertial_init_problem of include/orbgpu.h.  keyframes: a list of dicts Rwb, twb, vwb (or an (n, 21) float32 array of
    pose_inertial_state); edges: a list of dicts k1, k2, preint (dict as for pose_inertial_problem), info9 (orbg_imu_information(C)), or a
    record array of capi.INERTIAL_INIT_EDGE_DTYPE; bg, ba: the front keyframe's bias; Rwg (3 x 3), scale: the estimates of the gravity
    direction and the scale.  Returns (problem, keep-alive list)."""
    if isinstance(keyframes, np.ndarray):
        K = np.ascontiguousarray(keyframes, np.float32).reshape(-1, capi.INERTIAL_INIT_STATE_FLOATS)
    else:
        K = np.zeros((len(keyframes), capi.INERTIAL_INIT_STATE_FLOATS), np.float32)
        for i, kf in enumerate(keyframes):
            K[i, 0:9] = np.asarray(kf["Rwb"], np.float32).reshape(9)
            K[i, 9:12] = np.asarray(kf["twb"], np.float32).reshape(3)
            K[i, 12:15] = np.asarray(kf["vwb"], np.float32).reshape(3)
    if isinstance(edges, np.ndarray):
        E = np.ascontiguousarray(edges, capi.INERTIAL_INIT_EDGE_DTYPE)
    else:
        E = np.zeros(len(edges), capi.INERTIAL_INIT_EDGE_DTYPE)
        for i, e in enumerate(edges):
            E[i]["k1"], E[i]["k2"] = int(e["k1"]), int(e["k2"])
            E[i]["dT"] = np.float32(e["preint"]["dT"])
            for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bg", "ba"):
                E[i][k] = np.asarray(e["preint"][k], np.float32).reshape(-1)
            E[i]["info9"] = np.asarray(e["info9"], np.float64).reshape(81)
    p = capi.InertialInitProblem()
    p.struct_size = C.sizeof(capi.InertialInitProblem)
    p.device, p.algorithm, p.iterations, p.lambda_init = int(device), int(algorithm), int(iterations), float(lambda_init)
    p.free_velocity, p.free_bias, p.free_gdir, p.free_scale = [int(bool(f)) for f in (free_velocity, free_bias, free_gdir, free_scale)]
    p.with_priors, p.prior_g, p.prior_a = int(bool(with_priors)), float(prior_g), float(prior_a)
    _fill(p.bg, bg, np.float32)
    _fill(p.ba, ba, np.float32)
    _fill(p.Rwg, np.eye(3) if Rwg is None else Rwg, np.float64)
    p.scale = float(scale)
    p.n_keyframes, p.n_edges = len(K), len(E)
    p.keyframes = capi.ptr(K) if len(K) else None
    p.edges = capi.ptr(E) if len(E) else None
    return p, [K, E]


class InertialInitOutput:
    """inertial_init_result with its arrays.  vwb: (n_keyframes, 3) double."""

    def __init__(self, problem, trace_cap=200):
        self.nk = problem.n_keyframes
        self.vwb = np.zeros((max(self.nk, 1), 3))
        self.trace = np.zeros((max(trace_cap, 1), 3))
        c = self.c = capi.InertialInitResult()
        c.struct_size = C.sizeof(capi.InertialInitResult)
        c.vwb = capi.ptr(self.vwb)
        c.trace, c.trace_cap = capi.ptr(self.trace), trace_cap

    def as_dict(self):
        """the result in the layout of the numpy model (tests/inertial_init_model.py)"""
        c = self.c
        return {"vwb": self.vwb[: self.nk].copy(), "bg": np.array(list(c.bg)), "ba": np.array(list(c.ba)),
                "Rwg": np.array(list(c.Rwg)).reshape(3, 3), "scale": c.scale, "iters": c.iters, "n_unknowns": c.n_unknowns,
                "solve_failed": c.solve_failed, "chi2_first": c.chi2_first, "chi2_final": c.chi2_final,
                "trace": self.trace[: c.trace_len].copy()}


class InertialBaOutput:
    """inertial_ba_result with its arrays.  states: (n_keyframes, 21) double = Rwb (9), twb, vwb, bg, ba."""

    def __init__(self, problem, trace_cap=16):
        nk, nx, ne = problem.n_keyframes, problem.n_points, problem.n_edges
        self.states = np.zeros((max(nk, 1), capi.INERTIAL_BA_STATE_DOUBLES))
        self.points = np.zeros((max(nx, 1), 3), np.float32)
        self.edge_chi2 = np.zeros(max(ne, 1))
        self.edge_depth_pos = np.zeros(max(ne, 1), np.uint8)
        self.edge_outlier = np.zeros(max(ne, 1), np.uint8)
        self.trace = np.zeros((max(trace_cap, 1), 3))
        self.nk, self.nx, self.ne = nk, nx, ne
        c = self.c = capi.InertialBaResult()
        c.struct_size = C.sizeof(capi.InertialBaResult)
        c.states, c.points = capi.ptr(self.states), capi.ptr(self.points)
        c.edge_chi2, c.edge_depth_pos, c.edge_outlier = capi.ptr(self.edge_chi2), capi.ptr(self.edge_depth_pos), capi.ptr(self.edge_outlier)
        c.trace, c.trace_cap = capi.ptr(self.trace), trace_cap

    def as_dict(self):
        """the result in the layout of the numpy model (tests/inertial_ba_model.py)"""
        c = self.c
        st = self.states[: self.nk]
        return {"states": [{"R": s[0:9].reshape(3, 3).copy(), "t": s[9:12].copy(), "v": s[12:15].copy(), "bg": s[15:18].copy(),
                            "ba": s[18:21].copy()} for s in st],
                "points": self.points[: self.nx].copy(), "edge_chi2": self.edge_chi2[: self.ne].copy(),
                "edge_depth_pos": self.edge_depth_pos[: self.ne].copy(), "edge_outlier": self.edge_outlier[: self.ne].copy(),
                "n_outliers": c.n_outliers, "failed": c.failed, "iters": c.iters, "chi2_initial": c.chi2_initial, "chi2_final": c.chi2_final,
                "trace": self.trace[: c.trace_len].copy()}

    def write_back(self, Tcb):
        """What the glue hands to SetVelocity / SetNewBias / SetPose / SetWorldPos (S/Optimizer.cc:5154-5213), in float: per keyframe
        (vwb, bias as IMU::Bias(b[3], b[4], b[5], b[0], b[1], b[2]) = (ba, bg), Tcw 4 x 4 from Rcw[0], tcw[0]), and the points."""
        Tcb = np.asarray(Tcb, np.float32).astype(np.float64)[:3, :4]
        Rcb, tcb = Tcb[:, :3], Tcb[:, 3]
        out = []
        for s in self.states[: self.nk]:
            Rwb, twb = s[0:9].reshape(3, 3), s[9:12]
            Tcw = np.eye(4)
            Tcw[:3, :3] = Rcb @ Rwb.T
            Tcw[:3, 3] = Rcb @ (-(Rwb.T @ twb)) + tcb
            out.append({"vwb": s[12:15].astype(np.float32), "bias": np.concatenate([s[18:21], s[15:18]]).astype(np.float32),
                        "Tcw": Tcw.astype(np.float32)})
        return out, self.points[: self.nx].copy()


def database_view(inverted_file, bow_vectors, covisible, map_id, bad, map_bad, n_words):
    """orbd_database_view (KeyFrameDatabase flattened, S/KeyFrameDatabase.cc:594-761): inverted_file = {word: [kf, ...]} in
    insertion order, bow_vectors[kf] = (words ascending, values), covisible[kf] = GetBestCovisibilityKeyFrames(10) as indices."""
    K = len(bow_vectors)
    inv_start = np.zeros(n_words + 1, np.int32)
    for w, lst in inverted_file.items():
        inv_start[w + 1] = len(lst)
    inv_start = np.cumsum(inv_start).astype(np.int32)
    inv_kf = np.zeros(max(int(inv_start[-1]), 1), np.int32)
    for w, lst in inverted_file.items():
        inv_kf[inv_start[w]: inv_start[w] + len(lst)] = lst
    bow_start = np.cumsum([0] + [len(b[0]) for b in bow_vectors]).astype(np.int32)
    bow_word = _c(np.concatenate([b[0] for b in bow_vectors]) if K else np.zeros(1), np.int32)
    bow_value = _c(np.concatenate([b[1] for b in bow_vectors]) if K else np.zeros(1), np.float64)
    covis_start = np.cumsum([0] + [len(c) for c in covisible]).astype(np.int32)
    covis_kf = _c(np.concatenate([np.asarray(c, np.int32) for c in covisible] + [np.zeros(0, np.int32)]), np.int32)
    if covis_kf.size == 0:
        covis_kf = np.zeros(1, np.int32)
    arrs = [inv_start, inv_kf, bow_start, bow_word, bow_value, covis_start, covis_kf, _c(map_id, np.int32), _c(bad, np.uint8), _c(map_bad, np.uint8)]
    v = capi.DatabaseView(K, n_words, *[capi.ptr(a) for a in arrs])
    return v, arrs
