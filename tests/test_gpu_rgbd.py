"""GPU parity of the RGB-D Frame constructor (orbx_frame_rgbd*, S/Tracking.cc:1086-1142 + S/Frame.cc:174-257) and of the stand-alone
depth lookup (orbx_depth_at_points) against tests/rgbd_model.py: colour -> gray, extraction in the stereo-left order, undistortion,
ComputeStereoFromRGBD, the grid; synchronous, device-image, two-halves and ingest-thread forms; mixed use of one handle; the host
quad-tree redo path; one short chain downstream (SearchByProjection + PoseOptimization on the frame it leaves on the device).
Every test runs under a time limit of its own: a step that hangs ends the process instead of the queue behind it."""
import faulthandler

import numpy as np
import pytest

from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import api, synth, views
from oracle import binding as ob
import helpers
import rgbd_model as rm

pytestmark = pytest.mark.gpu

F32 = np.float32
EUROC_DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)       # R/ros/conf/EuRoC_mono_client.yaml
DISTS = {"none": None, "euroc": EUROC_DIST}
FACTOR = rm.depth_map_factor(5000.0)
STEP_LIMIT_S = 120


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


_SCENES = {}


def _scene(size):
    if size not in _SCENES:
        _SCENES[size] = synth.Scene(640, 480) if size == 640 else synth.Scene(160, 120, tex_size=(400, 300), px_per_m=50.0)
    return _SCENES[size]


def _depth_images(sc, Tcw):
    """u16 counts (TUM: 5000 per metre) and float32 metres of the same plane, each with a hole (0 / NaN) and a far patch (+inf)."""
    d16 = sc.depth_image(Tcw, np.uint16, 5000.0)
    d32 = sc.depth_image(Tcw, np.float32)
    h, w = d16.shape
    d16[h // 4:h // 2, w // 4:w // 2] = 0
    d32[h // 4:h // 2, w // 4:w // 2] = np.nan
    d32[h // 2:3 * h // 4, w // 2:3 * w // 4] = np.inf
    d32[0:h // 8, :] = -1.0
    return d16, d32


_REF = {}


def _ref(size, k, dist_name, colour, depth_kind):
    """The model's frame, computed once per case and shared."""
    key = (size, k, dist_name, colour, depth_kind)
    if key not in _REF:
        sc = _scene(size)
        L, R, Tcw = sc.stereo_pair(k)
        d16, d32 = _depth_images(sc, Tcw)
        dep, fac = (d16, FACTOR) if depth_kind == "u16" else (d32, F32(1.0))
        img = sc.color_image(L, 3, rgb_order=True) if colour else np.ascontiguousarray(L)
        p = sc.frame_view_params()
        m = rm.rgbd_frame(img, dep, p["cam"], float(sc.cam["bf"]), fac, DISTS[dist_name], rgb_order=True)
        m.update(L=np.ascontiguousarray(L), R=np.ascontiguousarray(R), Tcw=Tcw, dep=dep, fac=fac, scene=sc)
        _REF[key] = m
    return _REF[key]


def _empty_view(sc, bounds):
    p = sc.frame_view_params()
    return views.frame_view(np.zeros(1, capi.KEYPOINT_DTYPE), np.zeros((1, 32), np.uint8), None, None, bounds, p["cam"], 8, 1.2)


def _same(res, m, what=""):
    n, kps, kun, desc, ur, dp = res
    assert n == len(m["kps"]), what
    assert kps.tobytes() == m["kps"].tobytes() and desc.tobytes() == m["desc"].tobytes(), what
    assert kun.tobytes() == m["kps_un"].tobytes(), what
    assert ur.tobytes() == m["uright"].tobytes() and dp.tobytes() == m["depth"].tobytes(), what


def _grid_same(F, m, what=""):
    gs, gi = F.grid()
    os_, oi = ob.build_grid(m["fv"])
    assert np.array_equal(gs, os_) and np.array_equal(gi, oi), what


# ---------------------------------------------------------------- orbx_depth_at_points

@pytest.mark.parametrize("kind", ["u16", "f32", "f32_factor"])
def test_depth_at_points_equals_the_model(kind):
    """17 x 9 depth image inside a padded buffer (row stride of 24 elements); points on the last row and column, just outside,
    fractional, over NaN / 0 / inf / negative pixels; n = 0, 1, 63, 64, 65, 257 (below, at and above a wavefront, more than a block)."""
    rng = np.random.RandomState(11)
    h, w = 9, 17
    if kind == "u16":
        buf = rng.randint(1, 65536, (h, 24)).astype(np.uint16)
        buf[3, 4] = 0; buf[8, 16] = 65535; buf[0, 0] = 1
        factor = FACTOR
    else:
        buf = rng.uniform(0.3, 9.0, (h, 24)).astype(F32)
        buf[3, 4] = 0.0; buf[3, 5] = np.nan; buf[3, 6] = np.inf; buf[3, 7] = -2.0; buf[3, 8] = -np.inf; buf[3, 9] = -0.0
        factor = F32(1.0) if kind == "f32" else F32(0.001)
    buf[:, w:] = 7                                        # the padding holds valid-looking depths: reading it would show
    img = buf[:, :w]
    assert img.strides[0] == 24 * buf.itemsize
    special = np.array([[16, 8], [16.999, 8.999], [17.0, 8.0], [16.0, 9.0], [17.5, 3.0], [-1.0, 2.0], [2.0, -1.0], [-0.5, -0.5], [4, 3], [5, 3],
                        [6, 3], [7, 3], [8, 3], [9, 3], [4.999, 3.999], [0, 0], [0.999, 0.999], [3.5, 2.25], [1e9, 1.0], [np.nan, 1.0],
                        [1.0, np.nan]], F32)
    for n in (0, 1, 63, 64, 65, 257):
        xy = np.concatenate([special, rng.uniform([-1.5, -1.5], [w + 1.5, h + 1.5], (max(n - len(special), 0), 2)).astype(F32)])[:n]
        xun = (xy + rng.uniform(-2, 2, xy.shape).astype(F32)).astype(F32)
        g_ur, g_dp = api.depth_at_points(xy, img, 40.0, factor, xy_un=xun)
        m_ur, m_dp = rm.depth_at_points(xy, xun[:, 0], img, factor, 40.0)
        assert len(g_ur) == n and g_dp.tobytes() == m_dp.tobytes() and g_ur.tobytes() == m_ur.tobytes(), (kind, n)
        if n >= 21:
            assert (m_dp[:8] == -1).sum() >= 5 and (m_dp > 0).sum() > n // 3
    # xy_un = NULL: uRight from the same x
    xy = special[:18]
    g_ur, g_dp = api.depth_at_points(xy, img, 40.0, factor)
    m_ur, m_dp = rm.depth_at_points(xy, xy[:, 0], img, factor, 40.0)
    assert g_dp.tobytes() == m_dp.tobytes() and g_ur.tobytes() == m_ur.tobytes()


# ---------------------------------------------------------------- the constructor

def _dev(a):
    import torch
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    torch.cuda.synchronize()
    return t


def _run_forms(ex, F, fv0, img, dep, fac, bf, dist, rgb_order, forms):
    """-> {form: (n, mvKeys, mvKeysUn, mDescriptors, mvuRight, mvDepth)} of one image pair through the named forms."""
    out = {}
    w, h = img.shape[1], img.shape[0]
    ch = img.shape[2] if img.ndim == 3 else 1
    if "sync" in forms:
        out["sync"] = ex.frame_rgbd(F, fv0, img, dep, bf, fac, dist, rgb_order)
    if "dev" in forms or "dev_submit" in forms:
        d_img, d_dep = _dev(img), _dev(dep)
        ptrs, size = (d_img.data_ptr(), d_dep.data_ptr()), (w, h, ch, w * ch, dep.dtype, w * dep.itemsize)
        if "dev" in forms:
            out["dev"] = ex.frame_rgbd(F, fv0, None, None, bf, fac, dist, rgb_order, device_ptrs=ptrs, size=size)
    halves = [f for f in ("submit", "async", "dev_submit") if f in forms]
    if halves:
        o = ex.set_frame_outputs(ex.cap)
        for f in halves:
            for a in o.values():
                a[...] = 0
            if f == "dev_submit":
                ex.frame_rgbd_submit(F, fv0, None, None, bf, fac, dist, rgb_order, device_ptrs=ptrs, size=size)
            else:
                img2, dep2 = img.copy(), dep.copy()
                ex.frame_rgbd_submit(F, fv0, img2, dep2, bf, fac, dist, rgb_order, async_ingest=(f == "async"))
                if f == "submit":                         # flags == 0: the images are the caller's again when _submit returns
                    img2[...] = 0; dep2[...] = 0
            n = ex.frame_rgbd_wait()
            out[f] = (n, o["kps"][:n].copy(), o["kps_un"][:n].copy(), o["desc"][:n].copy(), o["uright"][:n].copy(), o["depth"][:n].copy())
        ex.set_frame_outputs(0)
    return out


@pytest.mark.parametrize("dist_name", sorted(DISTS))
@pytest.mark.parametrize("size", [160, 640])
def test_rgbd_constructor_equals_the_model_in_every_form(size, dist_name):
    """Gray, RGB, BGR, RGBA and BGRA input; u16 depth with TUM's factor for the undistorted camera, float32 metres (factor 1: bits
    untouched) for the distorted one; mvKeys, mvKeysUn, mDescriptors, mvuRight, mvDepth and the frame's grid bit-equal to the model in
    the synchronous, device-image, two-halves, ingest-thread and device two-halves forms."""
    dist = DISTS[dist_name]
    depth_kind = "u16" if dist is None else "f32"
    k = 4
    sc = _scene(size)
    bf = float(sc.cam["bf"])
    ex = api.ORBextractor(1000, 1.2, 8, 20, 7, sc.W, sc.H, n_cams=1)
    F = api.Frame()
    m_gray = _ref(size, k, dist_name, False, depth_kind)
    m_col = _ref(size, k, dist_name, True, depth_kind)
    fv0, keep0 = _empty_view(sc, m_gray["bounds"])
    assert len(m_gray["kps"]) > (900 if size == 640 else 100)
    assert (m_gray["depth"] > 0).sum() > len(m_gray["kps"]) // 3 and (m_gray["depth"] == -1).sum() > 0
    if dist is not None:
        assert np.abs(m_gray["kps_un"]["x"] - m_gray["kps"]["x"]).max() > (1.0 if size == 640 else 0.25)
    else:
        assert m_gray["kps_un"].tobytes() == m_gray["kps"].tobytes()
    dep, fac = m_gray["dep"], m_gray["fac"]
    L = m_gray["L"]
    all_forms = ("sync", "dev", "submit", "async", "dev_submit")
    cases = [("gray", L, True, m_gray, all_forms),
             ("rgb", sc.color_image(L, 3, True), True, m_col, ("sync", "dev")),
             ("bgr", sc.color_image(L, 3, False), False, m_col, all_forms),
             ("rgba", sc.color_image(L, 4, True), True, m_col, ("sync", "dev", "async")),
             ("bgra", sc.color_image(L, 4, False), False, m_col, ("sync", "dev_submit"))]
    for name, img, order, m, forms in cases:
        res = _run_forms(ex, F, fv0, img, dep, fac, bf, dist, order, forms)
        assert set(res) == set(forms)
        for f, r in res.items():
            _same(r, m, (name, f))
        _grid_same(F, m, name)
    # the colour image's gray differs from the plain one (B = gray / 2), so a conversion that did nothing would show ...
    assert m_col["kps"].tobytes() != m_gray["kps"].tobytes()
    # ... and so does the channel order: the RGB image read as BGR is another frame, the model's for that order
    if size == 160:
        rgb = sc.color_image(L, 3, True)
        p = sc.frame_view_params()
        m_wrong = rm.rgbd_frame(rgb, dep, p["cam"], bf, fac, dist, rgb_order=False)
        assert m_wrong["kps"].tobytes() != m_col["kps"].tobytes()
        _same(ex.frame_rgbd(F, fv0, rgb, dep, bf, fac, dist, False), m_wrong, "rgb read as bgr")
        # rows padded on the host (image and depth): the staging copy packs them
        pad_img = np.zeros((sc.H, sc.W + 5, 3), np.uint8); pad_img[:, :sc.W] = rgb
        pad_dep = np.full((sc.H, sc.W + 3), 9, dep.dtype); pad_dep[:, :sc.W] = dep
        _same(ex.frame_rgbd(F, fv0, pad_img[:, :sc.W], pad_dep[:, :sc.W], bf, fac, dist, True), m_col, "padded rows")
    # without a frame object (undistorted cameras only): the same features, no grid
    if dist is None:
        _same(ex.frame_rgbd(None, fv0, L, dep, bf, fac, None, True), m_gray, "no frame")
    ex.close(); F.close()


def test_rgbd_keypoint_order_is_the_stereo_left_order_and_zero_depth_gives_minus_one(scene):
    """A gray RGB-D frame with an all-zero depth image is the stereo constructor's left extraction with mvuRight = mvDepth = -1; its
    keypoint order is NOT the monocular constructor's (lapping area {0, 1000}: reversed)."""
    L, R, Tcw = scene.stereo_pair(6)
    L = np.ascontiguousarray(L)
    bf, b = float(scene.cam["bf"]), float(scene.cam["b"])
    fv0, keep0 = _empty_view(scene, (0.0, 640.0, 0.0, 480.0))
    ex = api.ORBextractor(1000, 1.2, 8, 20, 7, 640, 480, n_cams=2)
    F = api.Frame()
    for dep in (np.zeros((480, 640), np.uint16), np.zeros((480, 640), F32)):
        n, kps, kun, desc, ur, dp = ex.frame_rgbd(F, fv0, L, dep, bf, FACTOR if dep.dtype == np.uint16 else 1.0)
        assert n > 900 and np.all(ur == -1) and np.all(dp == -1) and kun.tobytes() == kps.tobytes()
    ns, nr, ks, ds, us, zs = ex.frame_stereo(F, fv0, L, np.ascontiguousarray(R), bf, b)
    assert ns == n and ks.tobytes() == kps.tobytes() and ds.tobytes() == desc.tobytes()
    nm, km, kmu, dm = ex.frame_mono(F, fv0, L, None)
    assert nm == n and km.tobytes() != kps.tobytes() and km[::-1].tobytes() == kps.tobytes() and dm[::-1].tobytes() == desc.tobytes()
    ex.close(); F.close()


def test_mono_then_rgbd_then_stereo_on_one_handle_each_equals_its_stand_alone_result(scene):
    m = _ref(640, 4, "none", True, "u16")
    sc = m["scene"]
    bf, b = float(sc.cam["bf"]), float(sc.cam["b"])
    fv0, keep0 = _empty_view(sc, (0.0, 640.0, 0.0, 480.0))
    L2, R2, _ = sc.stereo_pair(7)
    L2, R2 = np.ascontiguousarray(L2), np.ascontiguousarray(R2)
    bgr = sc.color_image(m["L"], 3, False)

    def alone(fn):
        ex = api.ORBextractor(1000, 1.2, 8, 20, 7, 640, 480, n_cams=2)
        F = api.Frame()
        r = fn(ex, F)
        g = F.grid()
        ex.close(); F.close()
        return [np.asarray(x).copy() for x in r], g

    steps = [lambda ex, F: ex.frame_mono(F, fv0, L2, None),
             lambda ex, F: ex.frame_rgbd(F, fv0, bgr, m["dep"], bf, m["fac"], None, False),
             lambda ex, F: ex.frame_stereo(F, fv0, L2, R2, bf, b)]
    single = [alone(s) for s in steps]
    ex = api.ORBextractor(1000, 1.2, 8, 20, 7, 640, 480, n_cams=2)
    F = api.Frame()
    for rnd in range(2):                                     # twice: the RGB-D frame also FOLLOWS a stereo frame
        for s, (ref, g) in zip(steps, single):
            r = [np.asarray(x).copy() for x in s(ex, F)]
            assert len(r) == len(ref) and all(a.tobytes() == c.tobytes() for a, c in zip(r, ref)), rnd
            gs, gi = F.grid()
            assert np.array_equal(gs, g[0]) and np.array_equal(gi, g[1])
    _same(tuple(single[1][0]), m, "stand-alone rgbd")
    ex.close(); F.close()


def test_rgbd_argument_checks_and_the_host_quadtree_redo_path(scene):
    """What the header says is refused is refused, the handle stays usable, and a frame whose candidates overflow the device lists
    (dense noise) is redone with the host quad-trees -- the undistortion, the depth lookup and the grid with it -- in the synchronous
    and in the two-halves form."""
    sc = scene
    p = sc.frame_view_params()
    cam4 = p["cam"][:4]
    bf = float(sc.cam["bf"])
    bounds = ob.image_bounds(640, 480, cam4, EUROC_DIST)
    fv_rect, k1 = _empty_view(sc, (0.0, 640.0, 0.0, 480.0))
    fv_dist, k2 = _empty_view(sc, bounds)
    ex = api.ORBextractor(1000, 1.2, 8, 20, 7, 640, 480, n_cams=1)
    F = api.Frame()
    rng = np.random.RandomState(2)
    noise = rng.randint(0, 256, (480, 640)).astype(np.uint8)
    dep = rng.randint(0, 30000, (480, 640)).astype(np.uint16)

    def refused(code, *a, **kw):
        with pytest.raises(capi.OrbGpuError) as e:
            ex.frame_rgbd(*a, **kw)
        assert e.value.code == code, (e.value.code, code)

    refused(capi.ORBG_BAD_ARG, None, fv_dist, noise, dep, bf, FACTOR, EUROC_DIST)          # distorted camera without a frame object
    refused(capi.ORBG_BAD_ARG, F, fv_dist, noise, dep, bf, FACTOR, None)                   # undistorted, bounds not the rectangle
    refused(capi.ORBG_EMPTY, F, fv_rect, np.zeros((0, 0), np.uint8), None, bf, FACTOR)     # no image
    refused(capi.ORBG_BAD_ARG, F, fv_rect, noise, None, bf, FACTOR)                        # no depth image
    refused(capi.ORBG_BAD_ARG, F, fv_rect, noise, dep, 0.0, FACTOR)                        # bf <= 0
    refused(capi.ORBG_BAD_ARG, F, fv_rect, np.zeros((480, 640, 2), np.uint8), dep, bf, FACTOR)      # two channels
    import ctypes as C
    n = C.c_int(0)
    for bad in ("depth_type", "struct_size", "depth_stride"):
        im2, w, h, keep = ex._rgbd_image(noise, dep, FACTOR, False)
        setattr(im2, bad, {"depth_type": 7, "struct_size": 8, "depth_stride": 640}[bad])
        rc = ex.lib.orbx_frame_rgbd(ex.h, F.h, C.byref(fv_rect), None, C.byref(im2), w, h, bf, None, None, None, None, None, 0, C.byref(n))
        assert rc == capi.ORBG_BAD_ARG, bad
    ex.frame_rgbd_submit(F, fv_rect, noise, dep, bf, FACTOR)
    with pytest.raises(capi.OrbGpuError) as e:                                            # one submission per handle
        ex.frame_rgbd_submit(F, fv_rect, noise, dep, bf, FACTOR)
    assert e.value.code == capi.ORBG_BAD_ARG
    ex.frame_rgbd_wait()
    # the redo path
    m = rm.rgbd_frame(noise, dep, p["cam"], bf, FACTOR, EUROC_DIST)
    _same(ex.frame_rgbd(F, fv_dist, noise, dep, bf, FACTOR, EUROC_DIST), m, "redo, synchronous")
    _grid_same(F, m, "redo, synchronous")
    o = ex.set_frame_outputs(ex.cap)
    ex.frame_rgbd_submit(F, fv_dist, noise, dep, bf, FACTOR, EUROC_DIST)
    n = ex.frame_rgbd_wait()
    _same((n, o["kps"][:n], o["kps_un"][:n], o["desc"][:n], o["uright"][:n], o["depth"][:n]), m, "redo, two halves")
    _grid_same(F, m, "redo, two halves")
    ex.close(); F.close()


def test_downstream_chain_search_by_projection_and_pose_optimization(scene, capsys):
    """RGB-D frame k -> map points by unproject_to_world; on RGB-D frame k + 1 (built on the device) SearchByProjection(Current, Last)
    with the uRight gate and PoseOptimization with stereo edges give the oracle's results on identical inputs (matches equal, pose
    <= 1e-4, the project's bounds); the distance to the scene's true pose is printed."""
    k = 4
    last = _ref(640, k, "none", False, "u16")
    cur = _ref(640, k + 1, "none", False, "u16")
    sc = last["scene"]
    bf = float(sc.cam["bf"])
    ex = api.ORBextractor(1000, 1.2, 8, 20, 7, 640, 480, n_cams=1)
    F = api.Frame()
    fv0, keep0 = _empty_view(sc, cur["bounds"])
    res = ex.frame_rgbd(F, fv0, cur["L"], cur["dep"], bf, cur["fac"])
    _same(res, cur)
    n, kps, kun, desc, ur, dp = res
    rng = np.random.RandomState(5)
    lv, keep_l = helpers.make_lastframe(sc, dict(kps=last["kps_un"], desc=last["desc"], depth=last["depth"], Tcw=last["Tcw"]), rng)
    guess = synth.perturb_pose(cur["Tcw"], rng).astype(np.float32)
    amp = np.full(n, -1, np.int32); aob = np.zeros(n, np.int32)
    g = api.ORBmatcher(0.9, True).SearchByProjectionFrame(F, guess, lv, 7.0, False, amp, aob)
    o = ob.search_by_projection_frame(cur["fv"], guess, lv, 7.0, False, True, amp, aob)
    assert g[2] == o[2] > 100 and np.array_equal(g[0], o[0]) and np.array_equal(g[1], o[1])
    Pw, valid = synth.unproject_to_world(last["kps_un"], last["depth"], last["Tcw"], sc.cam)
    idx = np.nonzero(g[0] >= 0)[0]
    sigma2 = np.array([F32(1.2) ** (2 * l) for l in range(8)], np.float64)
    inv_s2 = (1.0 / sigma2[kun["octave"][idx]]).astype(F32)
    cam5 = sc.frame_view_params()["cam"][:5]
    pp, keep_p = views.pose_opt_problem(Pw[g[0][idx]], kun["x"][idx], kun["y"][idx], ur[idx], inv_s2, cam5, guess)
    gp = api.Optimizer().PoseOptimization(pp)
    op = ob.pose_optimize(pp)
    assert (ur[idx] > 0).sum() > 50                                        # stereo edges took part
    assert np.abs(gp.Tcw - op.Tcw).max() <= 1e-4 and np.array_equal(gp.outliers, op.outliers) and gp.n_inliers == op.n_inliers > 100
    Tt = cur["Tcw"]
    dR = gp.Tcw[:3, :3].astype(np.float64) @ Tt[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
    dt = np.linalg.norm(-gp.Tcw[:3, :3].astype(np.float64).T @ gp.Tcw[:3, 3] + Tt[:3, :3].T @ Tt[:3, 3])
    with capsys.disabled():
        print("\n[rgbd chain] matches %d, inliers %d, distance to the true pose: %.4f deg, %.4f m" % (g[2], gp.n_inliers, ang, dt))
    ex.close(); F.close()
