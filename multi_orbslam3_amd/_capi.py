"""ctypes mirror of include/orbgpu.h and loader of the HIP library (liborbgpu.so).

The library is the product; there is NO CPU fallback: if the shared object is missing or cannot be
loaded, `load()` raises, and every entry point returns ORBG_NO_DEVICE when no HIP device is usable.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORBG_LIB") or os.path.join(_HERE, "liborbgpu.so")   # ORBG_LIB: an experimental build (tools/micro/variants)

ORBG_OK, ORBG_EMPTY, ORBG_BAD_ARG, ORBG_CAP_EXCEEDED, ORBG_HIP_ERROR, ORBG_NO_DEVICE, ORBG_INTERNAL = 0, -1, -2, -3, -4, -5, -6
LBA_APPLIED, LBA_ABORTED_BEFORE_OPT, LBA_REJECTED_OUTLIERS = 0, 1, 2
GRID_COLS, GRID_ROWS = 64, 48

u8p = C.POINTER(C.c_uint8)
i32p = C.POINTER(C.c_int32)
u32p = C.POINTER(C.c_uint32)
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4")])
EDGE_DTYPE = np.dtype([("pose", "<i4"), ("point", "<i4"), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"),
                       ("inv_sigma2", "<f4")])
assert KEYPOINT_DTYPE.itemsize == 24 and EDGE_DTYPE.itemsize == 24


class OrbxConfig(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("max_width", C.c_int32),
                ("max_height", C.c_int32), ("n_cams", C.c_int32), ("device", C.c_int32),
                ("gauss_taps", C.c_int32 * 4), ("octree_oldest_first", C.c_int32)]


class OrbxDistortion(C.Structure):
    """orbx_distortion: mDistCoef {k1, k2, p1, p2, k3} (S/Tracking.cc:71-81)."""
    _fields_ = [("k1", C.c_float), ("k2", C.c_float), ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float)]


class FrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("kps", C.c_void_p), ("desc", C.c_void_p), ("uright", C.c_void_p),
                ("depth", C.c_void_p), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float),
                ("max_y", C.c_float), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("bf", C.c_float), ("b", C.c_float), ("n_levels", C.c_int32),
                ("scale_factor", C.c_float)]


class MapPointsView(C.Structure):
    _fields_ = [("m", C.c_int32), ("track_in_view", C.c_void_p), ("bad", C.c_void_p), ("proj_x", C.c_void_p),
                ("proj_y", C.c_void_p), ("proj_xr", C.c_void_p), ("track_depth", C.c_void_p),
                ("scale_level", C.c_void_p), ("view_cos", C.c_void_p), ("desc", C.c_void_p),
                ("n_obs", C.c_void_p)]


class WorldPointsView(C.Structure):
    _fields_ = [("m", C.c_int32), ("pos", C.c_void_p), ("normal", C.c_void_p), ("min_dist", C.c_void_p),
                ("max_dist", C.c_void_p), ("desc", C.c_void_p), ("n_obs", C.c_void_p), ("bad", C.c_void_p),
                ("skip", C.c_void_p)]


class LastFrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("mp_valid", C.c_void_p), ("outlier", C.c_void_p), ("world_pos", C.c_void_p),
                ("desc", C.c_void_p), ("octave", C.c_void_p), ("angle", C.c_void_p), ("n_obs", C.c_void_p),
                ("Tcw", C.c_float * 16)]


class FeatVecView(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("node_id", C.c_void_p), ("start", C.c_void_p), ("feat_idx", C.c_void_p)]


class VocabView(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("L", C.c_int32), ("weighting", C.c_int32), ("scoring_norm", C.c_int32),
                ("child_start", C.c_void_p), ("child_ids", C.c_void_p), ("desc", C.c_void_p), ("weight", C.c_void_p),
                ("word_id", C.c_void_p)]


ORBV_TF_IDF, ORBV_TF, ORBV_IDF, ORBV_BINARY = 0, 1, 2, 3
ORBV_NORM_NONE, ORBV_NORM_L1, ORBV_NORM_L2 = 0, 1, 2
ORBV_TEXT_KEEP_TRAILING_NODE = 1


def vocab_view_arrays(v, k=None, scoring=None, n_words=None):
    """Copies of the arrays an orbv_vocab_view points at (a view handed out by a text loader dies with its handle)."""
    import numpy as np
    n = int(v.n_nodes)

    def arr(p, count, dt):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), shape=(count,)).copy() if count else np.zeros(0, dt)
    cs = arr(v.child_start, n + 1, C.c_int32)
    out = dict(child_start=cs, child_ids=arr(v.child_ids, int(cs[-1]), C.c_int32), desc=arr(v.desc, n * 32, C.c_uint8).reshape(n, 32),
               weight=arr(v.weight, n, C.c_double), word_id=arr(v.word_id, n, C.c_int32), L=int(v.L), weighting=int(v.weighting),
               scoring_norm=int(v.scoring_norm))
    if k is not None:
        out.update(k=int(k), scoring=int(scoring), n_words=int(n_words))
    return out


class Camera(C.Structure):
    """orbg_camera: model (0 pinhole, 1 KannalaBrandt8), fx fy cx cy, k1..k4."""
    _fields_ = [("model", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k", C.c_float * 4)]


class CameraRig(C.Structure):
    """orbg_camera_rig: mpCamera, mpCamera2 (has_right), mTrl (3 x 4 row-major)."""
    _fields_ = [("left", Camera), ("has_right", C.c_int32), ("right", Camera), ("Trl", C.c_float * 12)]


class FisheyeStereoView(C.Structure):
    """orbx_fisheye_stereo_view: the inputs of Frame::ComputeStereoFishEyeMatches."""
    _fields_ = [("n_left", C.c_int32), ("n_right", C.c_int32), ("mono_left", C.c_int32), ("mono_right", C.c_int32),
                ("kps_left", C.c_void_p), ("kps_right", C.c_void_p), ("desc_left", C.c_void_p), ("desc_right", C.c_void_p),
                ("level_sigma2", C.c_void_p), ("n_levels", C.c_int32), ("left", Camera), ("right", Camera), ("Tlr", C.c_float * 12)]


CAM_PINHOLE, CAM_KANNALA_BRANDT8 = 0, 1
UR_RIGHT_CAMERA = -2.0


class LbaProblem(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
                ("poses", C.c_void_p), ("pose_fixed", C.c_void_p), ("points", C.c_void_p), ("edges", C.c_void_p),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("lambda_init", C.c_double), ("its_round1", C.c_int32), ("its_round2", C.c_int32),
                ("device", C.c_int32), ("rig", C.POINTER(CameraRig))]


class LbaResult(C.Structure):
    _fields_ = [("poses", C.c_void_p), ("points", C.c_void_p), ("edge_chi2", C.c_void_p),
                ("edge_depth_pos", C.c_void_p), ("edge_outlier", C.c_void_p), ("status", C.c_int32),
                ("iters_round1", C.c_int32), ("iters_round2", C.c_int32), ("n_outliers", C.c_int32),
                ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("trace", C.c_void_p),
                ("trace_cap", C.c_int32), ("trace_len", C.c_int32)]


class BaCamera(C.Structure):
    """ba_camera: what one keyframe's edges read -- fx fy cx cy bf of the stereo edges, the camera model of the monocular ones."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("model", Camera)]


class BaProblem(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32), ("n_cameras", C.c_int32),
                ("poses", C.c_void_p), ("pose_fixed", C.c_void_p), ("pose_camera", C.c_void_p), ("points", C.c_void_p),
                ("edges", C.c_void_p), ("cameras", C.c_void_p), ("iterations", C.c_int32), ("robust", C.c_int32),
                ("device", C.c_int32)]


class BaResult(C.Structure):
    _fields_ = [("poses", C.c_void_p), ("points", C.c_void_p), ("edge_chi2", C.c_void_p), ("edge_depth_pos", C.c_void_p),
                ("point_included", C.c_void_p), ("status", C.c_int32), ("iters", C.c_int32), ("chi2_initial", C.c_double),
                ("chi2_final", C.c_double), ("trace", C.c_void_p), ("trace_cap", C.c_int32), ("trace_len", C.c_int32)]


class BaWeldProblem(C.Structure):
    """ba_weld_problem: `ba` is round 1's problem (its robust field is not read), then round 2's count and the two chi2 thresholds."""
    _fields_ = [("struct_size", C.c_uint32), ("ba", BaProblem), ("iterations_second", C.c_int32), ("chi2_mono", C.c_double),
                ("chi2_stereo", C.c_double)]


class BaWeldResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("ba", BaResult), ("edge_level", C.c_void_p), ("n_level1", C.c_int32),
                ("rounds_run", C.c_int32), ("iters_second", C.c_int32), ("chi2_initial_second", C.c_double),
                ("chi2_final_second", C.c_double), ("trace_second", C.c_void_p), ("trace_second_cap", C.c_int32),
                ("trace_second_len", C.c_int32)]


BA_MAX_FREE_POSES = 1365

# Optimizer::OptimizeEssentialGraph (include/orbgpu.h: eg_vertex, eg_edge, eg_point)
EG_VERTEX_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"), ("fixed", "<i4"), ("fix_scale", "<i4")])
EG_EDGE_DTYPE = np.dtype([("vi", "<i4"), ("vj", "<i4"), ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8")])
EG_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("ref", "<i4")])
assert EG_VERTEX_DTYPE.itemsize == 72 and EG_EDGE_DTYPE.itemsize == 72 and EG_POINT_DTYPE.itemsize == 16
EG_MAX_FREE_KEYFRAMES = 1170


class EgProblem(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_vertices", C.c_int32), ("vertices", C.c_void_p), ("n_edges", C.c_int32),
                ("edges", C.c_void_p), ("iterations", C.c_int32), ("lambda_init", C.c_double), ("n_points", C.c_int32),
                ("points", C.c_void_p), ("device", C.c_int32)]


class EgResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("estimates", C.c_void_p), ("points", C.c_void_p), ("err0", C.c_double),
                ("errEnd", C.c_double), ("iters", C.c_int32), ("trace", C.c_void_p), ("trace_cap", C.c_int32),
                ("trace_len", C.c_int32), ("edge_error0", C.c_void_p)]


class PoseOptProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("Xw", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("ur", C.c_void_p),
                ("inv_sigma2", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("bf", C.c_float), ("Tcw", C.c_float * 16), ("device", C.c_int32), ("rig", C.POINTER(CameraRig))]


class PoseInertialState(C.Structure):
    _fields_ = [("Rwb", C.c_float * 9), ("twb", C.c_float * 3), ("vwb", C.c_float * 3), ("bg", C.c_float * 3), ("ba", C.c_float * 3)]


class PoseInertialPreint(C.Structure):
    _fields_ = [("dT", C.c_float), ("dR", C.c_float * 9), ("dV", C.c_float * 3), ("dP", C.c_float * 3), ("JRg", C.c_float * 9),
                ("JVg", C.c_float * 9), ("JVa", C.c_float * 9), ("JPg", C.c_float * 9), ("JPa", C.c_float * 9), ("bg", C.c_float * 3),
                ("ba", C.c_float * 3)]


class PoseInertialPrior(C.Structure):
    _fields_ = [("Rwb", C.c_double * 9), ("twb", C.c_double * 3), ("vwb", C.c_double * 3), ("bg", C.c_double * 3), ("ba", C.c_double * 3),
                ("H", C.c_double * 225)]


class PoseInertialProblem(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("form", C.c_int32), ("rec_init", C.c_int32), ("device", C.c_int32), ("n_left", C.c_int32),
                ("n", C.c_int32), ("Xw", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("ur", C.c_void_p), ("inv_sigma2", C.c_void_p),
                ("close", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("Tcb", C.c_float * 12), ("frame", PoseInertialState), ("other", PoseInertialState), ("preint", PoseInertialPreint),
                ("info9", C.c_double * 81), ("infoG", C.c_double * 9), ("infoA", C.c_double * 9), ("prior", C.POINTER(PoseInertialPrior))]


class PoseInertialResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_inliers", C.c_int32), ("n_bad", C.c_int32), ("rounds_run", C.c_int32),
                ("solve_failed", C.c_int32), ("outlier", C.c_void_p), ("Rwb", C.c_double * 9), ("twb", C.c_double * 3),
                ("vwb", C.c_double * 3), ("bg", C.c_double * 3), ("ba", C.c_double * 3), ("chi2", C.c_double * 4), ("H", C.c_double * 225)]


POSE_INERTIAL_LAST_KEYFRAME, POSE_INERTIAL_LAST_FRAME = 0, 1


class InertialBaKeyframe(C.Structure):
    _fields_ = [("state", PoseInertialState), ("fixed", C.c_int32), ("imu", C.c_int32), ("link", C.c_int32), ("prev", C.c_int32),
                ("last_in_window", C.c_int32), ("preint", PoseInertialPreint), ("info9", C.c_double * 81), ("infoG", C.c_double * 9),
                ("infoA", C.c_double * 9)]


class InertialBaProblem(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_keyframes", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
                ("keyframes", C.c_void_p), ("points", C.c_void_p), ("edges", C.c_void_p), ("close", C.c_void_p), ("rec_init", C.c_int32),
                ("large", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("Tcb", C.c_float * 12), ("device", C.c_int32)]


# inertial_ba_state: Rwb (9), twb, vwb, bg, ba (3 each), double
INERTIAL_BA_STATE_DOUBLES = 21


class InertialBaResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("states", C.c_void_p), ("points", C.c_void_p), ("edge_chi2", C.c_void_p),
                ("edge_depth_pos", C.c_void_p), ("edge_outlier", C.c_void_p), ("n_outliers", C.c_int32), ("failed", C.c_int32),
                ("iters", C.c_int32), ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("trace", C.c_void_p),
                ("trace_cap", C.c_int32), ("trace_len", C.c_int32)]


INERTIAL_BA_MAX_FREE_KEYFRAMES = 32
INERTIAL_BA_MAX_EDGES = 1 << 22


class InertialInitEdge(C.Structure):
    _fields_ = [("k1", C.c_int32), ("k2", C.c_int32), ("preint", PoseInertialPreint), ("info9", C.c_double * 81)]


class InertialInitProblem(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("algorithm", C.c_int32), ("iterations", C.c_int32),
                ("lambda_init", C.c_double), ("free_velocity", C.c_int32), ("free_bias", C.c_int32), ("free_gdir", C.c_int32),
                ("free_scale", C.c_int32), ("with_priors", C.c_int32), ("prior_g", C.c_double), ("prior_a", C.c_double),
                ("bg", C.c_float * 3), ("ba", C.c_float * 3), ("Rwg", C.c_double * 9), ("scale", C.c_double), ("n_keyframes", C.c_int32),
                ("keyframes", C.c_void_p), ("n_edges", C.c_int32), ("edges", C.c_void_p)]


class InertialInitResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iters", C.c_int32), ("n_unknowns", C.c_int32), ("solve_failed", C.c_int32),
                ("vwb", C.c_void_p), ("bg", C.c_double * 3), ("ba", C.c_double * 3), ("Rwg", C.c_double * 9), ("scale", C.c_double),
                ("chi2_first", C.c_double), ("chi2_final", C.c_double), ("trace", C.c_void_p), ("trace_cap", C.c_int32),
                ("trace_len", C.c_int32)]


INERTIAL_INIT_MAX_KEYFRAMES = 4096
INERTIAL_INIT_LM, INERTIAL_INIT_GN = 0, 1
# pose_inertial_state as an array element: Rwb (9), twb, vwb, bg, ba (3 each), float
INERTIAL_INIT_STATE_FLOATS = 21
# inertial_init_edge as a numpy record, with the C compiler's alignment (held against the ctypes structure below)
INERTIAL_INIT_EDGE_DTYPE = np.dtype([("k1", "<i4"), ("k2", "<i4"), ("dT", "<f4"), ("dR", "<f4", (9,)), ("dV", "<f4", (3,)), ("dP", "<f4", (3,)),
                                     ("JRg", "<f4", (9,)), ("JVg", "<f4", (9,)), ("JVa", "<f4", (9,)), ("JPg", "<f4", (9,)),
                                     ("JPa", "<f4", (9,)), ("bg", "<f4", (3,)), ("ba", "<f4", (3,)), ("info9", "<f8", (81,))], align=True)
assert INERTIAL_INIT_EDGE_DTYPE.itemsize == C.sizeof(InertialInitEdge)
assert INERTIAL_INIT_EDGE_DTYPE.fields["info9"][1] == InertialInitEdge.info9.offset
assert C.sizeof(PoseInertialState) == 4 * INERTIAL_INIT_STATE_FLOATS


class DatabaseView(C.Structure):
    _fields_ = [("n_kfs", C.c_int32), ("n_words", C.c_int32), ("inv_start", C.c_void_p), ("inv_kf", C.c_void_p),
                ("bow_start", C.c_void_p), ("bow_word", C.c_void_p), ("bow_value", C.c_void_p), ("covis_start", C.c_void_p),
                ("covis_kf", C.c_void_p), ("map_id", C.c_void_p), ("bad", C.c_void_p), ("map_bad", C.c_void_p)]


class Sim3Problem(C.Structure):
    """orbm_sim3_problem: what Sim3Solver's constructor keeps per surviving pair, flat."""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_int32), ("X3Dc1", C.c_void_p), ("X3Dc2", C.c_void_p),
                ("max_err1", C.c_void_p), ("max_err2", C.c_void_p),
                ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float),
                ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float),
                ("camera_model1", C.c_int32), ("camera_model2", C.c_int32), ("fix_scale", C.c_int32)]


class Sim3Params(C.Structure):
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32)]


class Sim3Result(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("no_more", C.c_int32), ("converged", C.c_int32), ("n_inliers", C.c_int32),
                ("iterations_done", C.c_int32), ("iterations_run", C.c_int32), ("improved_in_this_call", C.c_int32),
                ("best_iteration", C.c_int32), ("have_best", C.c_int32), ("T12", C.c_float * 16), ("R", C.c_float * 9),
                ("t", C.c_float * 3), ("s", C.c_float), ("inliers", C.c_void_p), ("hyp_n_inliers", C.c_void_p),
                ("hyp_T12", C.c_void_p), ("hyp_masks", C.c_void_p)]


class MLPnPProblem(C.Structure):
    """orbp_mlpnp_problem: what MLPnPsolver's constructor keeps per surviving match, flat."""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_int32), ("P2D", C.c_void_p), ("sigma2", C.c_void_p), ("bearing", C.c_void_p),
                ("P3Dw", C.c_void_p), ("kp_index", C.c_void_p), ("m", C.c_int32), ("camera", Camera)]


class MLPnPParams(C.Structure):
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("min_set", C.c_int32),
                ("epsilon", C.c_float), ("th2", C.c_float)]


class MLPnPResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("no_more", C.c_int32), ("returned", C.c_int32), ("n_inliers", C.c_int32),
                ("iterations_done", C.c_int32), ("iterations_run", C.c_int32), ("best_iteration", C.c_int32), ("have_best", C.c_int32),
                ("best_inliers", C.c_int32), ("Tcw", C.c_float * 16), ("best_Tcw", C.c_float * 16), ("inliers", C.c_void_p),
                ("hyp_n_inliers", C.c_void_p), ("hyp_planar", C.c_void_p), ("hyp_R", C.c_void_p), ("hyp_t", C.c_void_p),
                ("hyp_masks", C.c_void_p)]


class Sim3OptProblem(C.Structure):
    """orbm_sim3opt_problem: what OptimizeSim3's loop over the matches hands to g2o, flat."""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_int32), ("X3Dc1", C.c_void_p), ("X3Dc2", C.c_void_p),
                ("obs1", C.c_void_p), ("obs2", C.c_void_p), ("inv_sigma2_1", C.c_void_p), ("inv_sigma2_2", C.c_void_p),
                ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float),
                ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float),
                ("camera_model1", C.c_int32), ("camera_model2", C.c_int32), ("fix_scale", C.c_int32), ("th2", C.c_float),
                ("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double), ("n_correspondences", C.c_int32)]


class Sim3OptResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_in", C.c_int32), ("returned_early", C.c_int32), ("n_bad_round1", C.c_int32),
                ("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double), ("removed", C.c_void_p),
                ("iters", C.c_int32 * 2), ("chi2", C.c_double * 2), ("trace", C.c_void_p), ("trace_cap", C.c_int32),
                ("trace_len", C.c_int32), ("edge_chi2", C.c_void_p)]


class TwoViewProblem(C.Structure):
    """orbi_two_view_problem: the arguments of TwoViewReconstruction's constructor and of Reconstruct, flat."""
    _fields_ = [("struct_size", C.c_uint32), ("n1", C.c_int32), ("n2", C.c_int32), ("keys1", C.c_void_p), ("keys2", C.c_void_p),
                ("matches12", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("sigma", C.c_float), ("iterations", C.c_int32)]


class TwoViewResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("success", C.c_int32), ("model", C.c_int32), ("best_iteration_H", C.c_int32),
                ("best_iteration_F", C.c_int32), ("n_matches", C.c_int32), ("n_inliers", C.c_int32), ("n_motions", C.c_int32),
                ("best_motion", C.c_int32), ("h_degenerate", C.c_int32), ("SH", C.c_float), ("SF", C.c_float),
                ("H21", C.c_float * 9), ("F21", C.c_float * 9), ("R21", C.c_float * 9), ("t21", C.c_float * 3),
                ("T1", C.c_float * 9), ("T2", C.c_float * 9), ("motion_nGood", C.c_int32 * 8), ("motion_parallax", C.c_float * 8),
                ("motion_R", C.c_float * 72), ("motion_t", C.c_float * 24), ("vP3D", C.c_void_p), ("vbTriangulated", C.c_void_p),
                ("hyp_scores", C.c_void_p), ("hyp_models", C.c_void_p), ("hyp_masks", C.c_void_p), ("hyp_sets", C.c_void_p)]


TWO_VIEW_MAX_MATCHES, TWO_VIEW_MAX_ITERATIONS = 8192, 4096


class NewPointsKF(C.Structure):
    """orbm_newpoints_kf: one keyframe side of CreateNewMapPoints / SearchForTriangulation."""
    _fields_ = [("struct_size", C.c_uint32), ("frame", C.c_void_p), ("featvec", FeatVecView), ("has_mp", C.c_void_p),
                ("keys_xy", C.c_void_p), ("Tcw", C.c_float * 12), ("Twc", C.c_float * 12), ("Ow", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float),
                ("invfy", C.c_float), ("mb", C.c_float), ("mbf", C.c_float), ("n_levels", C.c_int32),
                ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p), ("scale_factor", C.c_float)]


class NewPointsParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("only_stereo", C.c_int32), ("coarse", C.c_int32), ("check_orientation", C.c_int32),
                ("far_points", C.c_int32), ("th_far_points", C.c_float)]


NEWPOINTS_MAX_NEIGHBOURS = 64
# status codes of orbm_newpoints_record (include/orbgpu.h)
(NP_ACCEPTED, NP_HAS_POINT, NP_NOT_STEREO, NP_NO_NODE, NP_NO_MATCH, NP_W_ZERO, NP_LOW_PARALLAX, NP_EMPTY, NP_Z1, NP_Z2, NP_REPROJ1,
 NP_REPROJ2, NP_DIST_ZERO, NP_FAR, NP_SCALE) = range(15)
NEWPOINTS_RECORD_DTYPE = np.dtype([("idx2", "<i4"), ("dist", "<i4"), ("status", "<i4"), ("x3D", "<f4", (3,)), ("w", "<f4"),
                                   ("cos_parallax", "<f4")])
NEWPOINT_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("x3D", "<f4", (3,))])
assert NEWPOINTS_RECORD_DTYPE.itemsize == 32 and NEWPOINT_DTYPE.itemsize == 24


class FuseKF(C.Structure):
    """orbm_fuse_kf: one target keyframe of ORBmatcher::Fuse."""
    _fields_ = [("struct_size", C.c_uint32), ("frame", C.c_void_p), ("Tcw", C.c_float * 12), ("Ow", C.c_float * 3),
                ("Scw", C.c_float * 16), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("mbf", C.c_float), ("n_levels", C.c_int32), ("scale_factors", C.c_void_p), ("inv_level_sigma2", C.c_void_p),
                ("log_scale_factor", C.c_float)]


class FuseParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("th", C.c_float), ("sim3_form", C.c_int32)]


FUSE_MAX_KEYFRAMES, FUSE_CAND_CAP = 512, 16
# status codes of orbm_fuse_record (include/orbgpu.h)
(FUSE_CANDIDATES, FUSE_NEG_DEPTH, FUSE_NOT_IN_IMAGE, FUSE_DISTANCE, FUSE_NORMAL, FUSE_EMPTY_WINDOW, FUSE_NO_CANDIDATE,
 FUSE_SKIPPED) = range(8)
FUSE_RECORD_DTYPE = np.dtype([("status", "<i4"), ("best_idx", "<i4"), ("best_dist", "<i4"), ("level", "<i4"), ("n_cand", "<i4")])
assert FUSE_RECORD_DTYPE.itemsize == 20


class InitSearchParams(C.Structure):
    """orbm_init_search_params: windowSize, mfNNratio, mbCheckOrientation; list_capacity 0 = the default."""
    _fields_ = [("struct_size", C.c_uint32), ("window_size", C.c_int32), ("nn_ratio", C.c_float), ("check_orientation", C.c_int32),
                ("list_capacity", C.c_int32)]


class InitSearchDebug(C.Structure):
    _fields_ = [("list_start", C.c_void_p), ("entries", C.c_void_p), ("entries_cap", C.c_int32), ("n_queries", C.c_int32),
                ("n_candidates", C.c_int32), ("n_evictions", C.c_int32), ("n_rot_rejected", C.c_int32), ("n_regrown", C.c_int32)]


INIT_SEARCH_MAX_LIST = 1 << 26

ORBX_DEPTH_U16, ORBX_DEPTH_F32 = 0, 1


class OrbxRgbdImage(C.Structure):
    """orbx_rgbd_image: the colour / gray image and the depth image of one RGB-D frame (orbx_frame_rgbd*)."""
    _fields_ = [("struct_size", C.c_uint32), ("channels", C.c_int32), ("img", C.c_void_p), ("stride", C.c_int32),
                ("rgb_order", C.c_int32), ("depth", C.c_void_p), ("depth_type", C.c_int32), ("depth_stride", C.c_int32),
                ("depth_factor", C.c_float), ("reserved", C.c_int32)]


class PoseOptResult(C.Structure):
    _fields_ = [("Tcw", C.c_float * 16), ("outlier", C.c_void_p), ("n_inliers", C.c_int32), ("n_bad", C.c_int32),
                ("iters", C.c_int32 * 4), ("chi2", C.c_double * 4)]


def ptr(a):
    """void* of a C-contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return a.ctypes.data


# Every symbol include/orbgpu.h declares (tests assert that the library exports all of them).
EXPORTED_SYMBOLS = [
    "orbx_create", "orbx_destroy", "orbx_get_tables", "orbx_extract", "orbx_extract_stereo",
    "orbx_extract_stereo_dev", "orbx_get_level", "orbx_get_level_bordered", "orbx_get_candidates", "orbx_stereo_match",
    "orbm_frame_create", "orbm_frame_destroy", "orbm_frame_upload", "orbm_frame_from_extractor", "orbx_frame_stereo_dev", "orbx_frame_stereo", "orbx_frame_stereo_dev_submit", "orbx_frame_stereo_dev_wait", "orbx_frame_stereo_submit", "orbx_frame_stereo_wait", "orbx_set_frame_outputs",
    "orbm_frame_get_grid", "orbm_hamming_matrix", "orbm_hamming_best2", "orbm_is_in_frustum",
    "orbm_search_by_projection_mps", "orbm_is_in_frustum_rig", "orbm_search_by_projection_mps_rig", "orbm_search_by_projection_frame_rig", "orbm_search_by_bow_rig", "orbx_fisheye_stereo_matches", "orbm_map_create", "orbm_map_destroy", "orbm_map_upload",
    "orbm_search_local_points", "orbm_search_local_points_vis", "orbm_search_by_projection_frame", "orbm_search_by_bow",
    "orbm_search_by_projection_sim3", "orbm_search_by_bow_kf",
    "orbv_vocab_create", "orbv_vocab_destroy", "orbv_text_load", "orbv_text_view", "orbv_text_free", "orbv_vocab_from_text", "orbv_transform", "orbv_transform_frame", "orbv_bow_assemble",
    "orbm_distinctive_descriptors", "orbv_score_l1", "orbk_wire_bytes", "orbk_pack_frame", "orbk_frame_from_wire",
    "orbm_frame_download",
    "lba_solve", "lba_create", "lba_destroy", "lba_solve_h", "lba_solve_async", "lba_wait", "pose_optimize",
    "lba_solve_b", "lba_solve_hb", "lba_solve_async_b",
    "lba_set_profiling", "lba_get_solver_stats", "lba_event_overhead", "lba_get_watchdog_count",
    "orbd_database_create", "orbd_database_destroy", "orbd_detect_n_best_candidates", "orbd_detect_relocalization_candidates",
    "orbx_set_stream", "orbm_frame_set_stream", "orbm_map_set_stream", "lba_set_stream", "orbv_vocab_set_stream", "orbd_database_set_stream",
    "pose_opt_set_stream", "orbx_get_ctor_timeline", "orbm_map_set_observations", "orbm_search_by_projection_reloc", "orbm_search_by_projection_reloc_cam", "orbm_search_by_projection_sim3_cam", "orbm_lastview_create", "orbm_lastview_destroy", "orbm_lastview_upload",
    "orbm_search_by_projection_frame_resident", "orbg_quiesce", "orbg_set_wait_policy", "orbg_get_wait_policy",
    "orbx_frame_mono", "orbx_frame_mono_dev", "orbx_frame_mono_submit", "orbx_frame_mono_dev_submit", "orbx_frame_mono_wait",
    "orbx_set_frame_outputs_un", "orbx_undistort_points",
    "orbx_frame_rgbd", "orbx_frame_rgbd_dev", "orbx_frame_rgbd_submit", "orbx_frame_rgbd_dev_submit", "orbx_frame_rgbd_wait",
    "orbx_depth_at_points",
    "orbm_sim3_create", "orbm_sim3_destroy", "orbm_sim3_set_stream", "orbm_sim3_set_problem", "orbm_sim3_set_ransac_parameters",
    "orbm_sim3_ransac_iterations", "orbm_sim3_resolve_draws", "orbm_sim3_iterate", "orbm_sim3_solve_batch",
    "orbm_sim3_optimize", "orbm_sim3_optimize_batch",
    "orbm_create_new_points", "orbm_search_for_triangulation", "orbm_fuse", "orbm_search_for_initialization",
    "orbg_version", "orbg_strerror", "orbg_device_count", "orbx_get_timings", "orbx_event_overhead", "orbx_set_profile_interval", "orbx_set_profile_kernel", "orbx_get_fast_kernel_stats", "orbx_set_profiling",
    "orbx_get_host_redo_count",
    "pose_inertial_optimize", "pose_inertial_host_linearize", "pose_inertial_set_stream", "orbg_imu_information", "orbg_condition_prior",
]

# The initialisers (prefix orbi_): a list of its own, because tests/test_capi_cpu.py holds EXPORTED_SYMBOLS against the header's
# declarations under the prefixes above only.  build() and load() treat both lists alike; tests/test_two_view_cpu.py holds this one.
INITIALISER_SYMBOLS = ["orbi_two_view_resolve_draws", "orbi_two_view_reconstruct"]
# The full bundle adjustment (prefix ba_), likewise a list of its own; tests/test_full_ba_cpu.py holds it against the header.
FULL_BA_SYMBOLS = ["ba_solve", "ba_solve_b", "ba_create", "ba_destroy", "ba_solve_h", "ba_solve_hb", "ba_set_profiling", "ba_get_phase_ms",
                   "ba_weld_solve", "ba_weld_solve_b", "ba_weld_solve_h", "ba_weld_solve_hb"]
# The essential graph (prefix eg_), likewise; tests/test_essential_graph_cpu.py holds it against the header.
ESSENTIAL_GRAPH_SYMBOLS = ["eg_solve", "eg_set_profiling", "eg_get_phase_ms"]

# The local inertial BA (prefix inertial_ba_), likewise; tests/test_inertial_ba_cpu.py holds it against the header.
INERTIAL_BA_SYMBOLS = ["inertial_ba_solve", "inertial_ba_create", "inertial_ba_destroy", "inertial_ba_solve_h", "inertial_ba_set_stream",
                       "inertial_ba_set_profiling", "inertial_ba_get_phase_ms", "inertial_ba_host_linearize"]

# The inertial initialisation (prefix inertial_init_), likewise; tests/test_inertial_init_cpu.py holds it against the header.
INERTIAL_INIT_SYMBOLS = ["inertial_init_solve", "inertial_init_host_linearize", "inertial_init_set_stream"]

# MLPnPsolver (prefix orbp_), likewise; tests/test_mlpnp_cpu.py holds it against the header.
MLPNP_SYMBOLS = ["orbp_mlpnp_create", "orbp_mlpnp_destroy", "orbp_mlpnp_set_stream", "orbp_mlpnp_set_problem",
                 "orbp_mlpnp_set_ransac_parameters", "orbp_mlpnp_ransac_iterations", "orbp_mlpnp_iterations_of_call",
                 "orbp_mlpnp_resolve_draws", "orbp_mlpnp_iterate", "orbp_mlpnp_solve_batch", "orbp_mlpnp_gn"]

_lib = None


class OrbGpuError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        msg = "orbgpu error %d" % code
        try:
            msg += " (%s)" % load().orbg_strerror(code).decode()
        except Exception:
            pass
        super().__init__(msg + (" in " + where if where else ""))


def load():
    """Load liborbgpu.so; raise loudly if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("liborbgpu.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(expected at %s). There is no CPU fallback." % LIB_PATH)
    # ONE HIP / HSA runtime per process: PyTorch-ROCm ships its own libamdhip64 + libhsa-runtime64 and loads them by path even when
    # the system's are mapped already (the library's own dependency resolves to /opt/rocm); the second runtime then finds no
    # GPU ("No HIP GPUs are available" from the first torch.cuda call of a process that used this library before importing
    # torch).  With torch imported first the library's NEEDED entry resolves to the runtime torch mapped.  A C++ deployment
    # (no torch in the process) has the system runtime only.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.orbg_version.restype = C.c_char_p
    lib.orbg_strerror.restype = C.c_char_p
    lib.orbg_strerror.argtypes = [C.c_int]
    lib.orbm_sim3_ransac_iterations.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p]
    lib.orbm_sim3_set_ransac_parameters.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int]
    lib.orbm_sim3_optimize.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.orbm_sim3_optimize_batch.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.orbi_two_view_resolve_draws.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.orbi_two_view_reconstruct.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.orbm_create_new_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.orbm_search_for_triangulation.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.orbm_fuse.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.orbm_search_for_initialization.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rgbd_head = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float]
    lib.orbx_frame_rgbd.argtypes = rgbd_head + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    lib.orbx_frame_rgbd_dev.argtypes = rgbd_head + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    lib.orbx_frame_rgbd_submit.argtypes = rgbd_head + [C.c_int]
    lib.orbx_frame_rgbd_dev_submit.argtypes = rgbd_head
    lib.orbx_frame_rgbd_wait.argtypes = [C.c_void_p, C.c_void_p]
    lib.orbx_depth_at_points.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    lib.pose_inertial_optimize.argtypes = [C.c_void_p, C.c_void_p]
    lib.pose_inertial_host_linearize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pose_inertial_set_stream.argtypes = [C.c_int, C.c_void_p]
    lib.orbg_imu_information.argtypes = [C.c_void_p] * 4
    lib.orbg_condition_prior.argtypes = [C.c_void_p]
    lib.inertial_ba_solve.argtypes = [C.c_void_p, C.c_void_p]
    lib.inertial_ba_create.argtypes = [C.c_int, C.c_void_p]
    lib.inertial_ba_destroy.argtypes = [C.c_void_p]
    lib.inertial_ba_solve_h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.inertial_ba_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.inertial_ba_set_profiling.argtypes = [C.c_void_p, C.c_int]
    lib.inertial_ba_get_phase_ms.argtypes = [C.c_void_p, C.c_void_p]
    lib.inertial_ba_host_linearize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.inertial_init_solve.argtypes = [C.c_void_p, C.c_void_p]
    lib.inertial_init_host_linearize.argtypes = [C.c_void_p, C.c_void_p]
    lib.inertial_init_set_stream.argtypes = [C.c_int, C.c_void_p]
    lib.eg_solve.argtypes = [C.c_void_p, C.c_void_p]
    lib.eg_set_profiling.argtypes = [C.c_int]
    lib.eg_get_phase_ms.argtypes = [C.c_void_p]
    lib.orbp_mlpnp_set_ransac_parameters.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
    lib.orbp_mlpnp_ransac_iterations.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    lib.orbp_mlpnp_gn.argtypes = [C.c_int] + [C.c_void_p] * 6
    for name in EXPORTED_SYMBOLS + INITIALISER_SYMBOLS + FULL_BA_SYMBOLS + ESSENTIAL_GRAPH_SYMBOLS + MLPNP_SYMBOLS + INERTIAL_BA_SYMBOLS + INERTIAL_INIT_SYMBOLS:
        fn = getattr(lib, name)
        if name not in ("orbg_version", "orbg_strerror"):
            fn.restype = C.c_int
    _lib = lib
    return lib


def check(code, where=""):
    if code != ORBG_OK:
        raise OrbGpuError(code, where)
