"""What the extract and Frame-constructor entry points of csrc/extractor.hip refuse, and with which code: one input per fault and entry
point, called through _capi (api.py turns codes into exceptions).  The expected codes are read from the entry points' own checks; the
routes do not agree everywhere (an image larger than the handle was created for is the known case) and the table says where.  A refused
call launches nothing and leaves the handle as it was: in particular the timeline row of a submission in flight.  Refusals that
test_gpu_rgbd.py, test_gpu_mono.py and test_gpu_parity.py assert already are not repeated."""
import ctypes as C
import time

import numpy as np
import pytest

from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import api, synth, views

pytestmark = pytest.mark.gpu

OK, EMPTY, BAD = capi.ORBG_OK, capi.ORBG_EMPTY, capi.ORBG_BAD_ARG
W, H = 160, 120
EUROC_DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)

# entry point -> (family, route)
ENTRIES = {
    "orbx_extract": ("extract", "sync"),
    "orbx_extract_stereo": ("xstereo", "sync"), "orbx_extract_stereo_dev": ("xstereo", "dev"),
    "orbx_frame_stereo": ("stereo", "sync"), "orbx_frame_stereo_dev": ("stereo", "dev"),
    "orbx_frame_stereo_submit": ("stereo", "submit"), "orbx_frame_stereo_dev_submit": ("stereo", "dev_submit"),
    "orbx_frame_mono": ("mono", "sync"), "orbx_frame_mono_dev": ("mono", "dev"),
    "orbx_frame_mono_submit": ("mono", "submit"), "orbx_frame_mono_dev_submit": ("mono", "dev_submit"),
    "orbx_frame_rgbd": ("rgbd", "sync"), "orbx_frame_rgbd_dev": ("rgbd", "dev"),
    "orbx_frame_rgbd_submit": ("rgbd", "submit"), "orbx_frame_rgbd_dev_submit": ("rgbd", "dev_submit"),
}
CTORS = ("stereo", "mono", "rgbd")


def _names(families=None, routes=None):
    return [n for n, (f, r) in ENTRIES.items() if (families is None or f in families) and (routes is None or r in routes)]


def _scene(w, h):
    return synth.Scene(w, h, tex_size=(max(2 * w, 400), max(2 * h, 300)), px_per_m=50.0)


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a.view(np.int16) if a.dtype == np.uint16 else a)).cuda()
    torch.cuda.synchronize()
    return t


class Good:
    """Arguments every entry point accepts for one w x h frame; a test changes one of them and calls."""

    def __init__(self, ex, w=W, h=H):
        sc = _scene(w, h)
        L, R, Tcw = sc.stereo_pair(2)
        self.sc, self.w, self.h, self.stride = sc, w, h, w
        self.L, self.R = np.ascontiguousarray(L), np.ascontiguousarray(R)
        self.dep = sc.depth_image(Tcw, np.uint16, 5000.0)
        self.d_L, self.d_R, self.d_dep = _dev(self.L), _dev(self.R), _dev(self.dep)
        self.hnd = ex.h
        self.frame = api.Frame()
        p = sc.frame_view_params()
        self.view, self.keep = views.frame_view(np.zeros(1, capi.KEYPOINT_DTYPE), np.zeros((1, 32), np.uint8), None, None, p["bounds"], p["cam"], 8, 1.2)
        self.dist = None
        self.bf, self.b = float(sc.cam["bf"]), float(sc.cam["b"])
        self.cap = ex.cap
        self.kps = np.zeros(self.cap, capi.KEYPOINT_DTYPE); self.kps_un = np.zeros(self.cap, capi.KEYPOINT_DTYPE)
        self.desc = np.zeros((self.cap, 32), np.uint8)
        self.ur = np.zeros(self.cap, np.float32); self.dp = np.zeros(self.cap, np.float32)
        self.n, self.n_right = C.c_int(-7), C.c_int(-7)
        self.has_n = True
        # the RGB-D descriptor: gray image, u16 depth; `rgbd` holds what a test changes (img / depth None = the route's own pointer)
        self.rgbd = dict(struct_size=C.sizeof(capi.OrbxRgbdImage), channels=1, img="own", stride=w, depth="own", depth_type=capi.ORBX_DEPTH_U16,
                         depth_stride=2 * w, depth_factor=1.0 / 5000.0)
        self.no_rgbd = False
        self.flags = 0

    def images(self, dev):
        return (self.d_L.data_ptr(), self.d_R.data_ptr()) if dev else (self.L.ctypes.data, self.R.ctypes.data)


def call(lib, name, g):
    """One call of entry point `name` with the arguments in g."""
    family, route = ENTRIES[name]
    dev = route in ("dev", "dev_submit")
    vp = C.c_void_p

    def arr(a):
        return vp(capi.ptr(a))

    il, ir = g.images(dev)
    if getattr(g, "null_image", False):
        il = None
    elif getattr(g, "null_right", False):
        ir = None
    fr = g.frame.h if g.frame is not None else None
    fv = C.byref(g.view) if g.view is not None else None
    n = C.byref(g.n) if g.has_n else None
    nr = C.byref(g.n_right)
    dist = C.byref(capi.OrbxDistortion(*g.dist)) if g.dist is not None else None
    fn = getattr(lib, name)
    if family == "extract":
        return fn(g.hnd, 0, vp(il), g.w, g.h, g.stride, 0, 0, arr(g.kps), arr(g.desc), g.cap, n, None)
    if family == "xstereo":
        return fn(g.hnd, vp(il), vp(ir), g.w, g.h, g.stride, arr(g.kps), arr(g.desc), g.cap, n, None, None, 0, nr)
    if family == "stereo":
        head = (g.hnd, fr, fv, vp(il), vp(ir), g.w, g.h, g.stride, C.c_float(g.bf), C.c_float(g.b))
        if route in ("sync", "dev"):
            return fn(*head, arr(g.kps), arr(g.desc), arr(g.ur), arr(g.dp), g.cap, n, nr)
        return fn(*head, g.flags) if route == "submit" else fn(*head)
    if family == "mono":
        head = (g.hnd, fr, fv, dist, vp(il), g.w, g.h, g.stride)
        if route in ("sync", "dev"):
            return fn(*head, arr(g.kps), arr(g.kps_un), arr(g.desc), g.cap, n)
        return fn(*head, g.flags) if route == "submit" else fn(*head)
    im = capi.OrbxRgbdImage()
    r = g.rgbd
    im.struct_size, im.channels, im.stride, im.rgb_order = r["struct_size"], r["channels"], r["stride"], 1
    im.depth_type, im.depth_stride, im.depth_factor = r["depth_type"], r["depth_stride"], r["depth_factor"]
    im.img = il if r["img"] == "own" else r["img"]
    own_depth = g.d_dep.data_ptr() if dev else g.dep.ctypes.data
    im.depth = own_depth + r.get("depth_offset", 0) if r["depth"] == "own" else r["depth"]
    if getattr(g, "null_image", False):
        im.img = None
    head = (g.hnd, fr, fv, dist, None if g.no_rgbd else C.byref(im), g.w, g.h, g.bf)
    if route in ("sync", "dev"):
        return fn(*head, arr(g.kps), arr(g.kps_un), arr(g.desc), arr(g.ur), arr(g.dp), g.cap, n)
    return fn(*head, g.flags) if route == "submit" else fn(*head)


@pytest.fixture(scope="module")
def rig():
    """A two-camera and a one-camera handle for 160 x 120, the accepted arguments for each, and the library."""
    ex2 = api.ORBextractor(300, 1.2, 8, 20, 7, W, H, n_cams=2)
    ex1 = api.ORBextractor(300, 1.2, 8, 20, 7, W, H, n_cams=1)
    return dict(lib=capi.load(), ex2=ex2, ex1=ex1, g2=Good(ex2), g1=Good(ex1))


def _fresh(g, **changes):
    """A shallow copy of the accepted arguments with some of them changed (rgbd_* keys change the descriptor)."""
    c = object.__new__(Good)
    c.__dict__.update(g.__dict__)
    c.rgbd = dict(g.rgbd)
    c.n, c.n_right = C.c_int(-7), C.c_int(-7)
    for k, v in changes.items():
        if k.startswith("rgbd_"):
            c.rgbd[k[5:]] = v
        else:
            setattr(c, k, v)
    return c


def _refused(rig, names, code, what, one_camera=False, **changes):
    """Every entry point in `names` answers `code` to the accepted arguments with `changes`, writes no count and leaves the handle idle."""
    base = rig["g1"] if one_camera else rig["g2"]
    ex = rig["ex1"] if one_camera else rig["ex2"]
    for name in names:
        g = _fresh(base, **changes)
        rc = call(rig["lib"], name, g)
        assert rc == code, "%s, %s: %d, expected %d" % (name, what, rc, code)
        assert g.n.value == -7, "%s, %s: a refused call wrote a count" % (name, what)
        if g.hnd is not None:
            assert rig["lib"].orbx_frame_stereo_dev_wait(ex.h, None, None) == BAD, "%s, %s: the refused call left a submission" % (name, what)


# ---------------------------------------------------------------- the faults every entry point knows

def test_accepted_arguments_are_accepted(rig):
    """The arguments the refusal rows start from pass every entry point: the synchronous forms return the same count, the submitted
    ones the same from their wait."""
    lib = rig["lib"]
    want = {}
    for name, (family, route) in ENTRIES.items():
        g = _fresh(rig["g2"])
        assert call(lib, name, g) == OK, name
        if route in ("submit", "dev_submit"):
            assert lib.orbx_frame_stereo_dev_wait(g.hnd, C.byref(g.n), C.byref(g.n_right)) == OK, name
        assert g.n.value > 50, name
        assert want.setdefault(family if family != "xstereo" else "stereo", g.n.value) == g.n.value, name
    assert want["stereo"] == want["rgbd"] == want["extract"]         # lapping area {0, 0}: the same keypoints; mono reverses them
    for name in _names(("extract", "mono", "rgbd")):
        g = _fresh(rig["g1"])
        assert call(lib, name, g) == OK, name
        if ENTRIES[name][1] in ("submit", "dev_submit"):
            assert lib.orbx_frame_stereo_dev_wait(g.hnd, C.byref(g.n), None) == OK, name
        assert g.n.value == want[ENTRIES[name][0]], name


def test_faults_of_every_entry_point(rig):
    every = _names()
    _refused(rig, every, BAD, "NULL handle", hnd=None)
    _refused(rig, _names(("xstereo", "stereo")), BAD, "a stereo entry on a one-camera handle", one_camera=True)
    _refused(rig, _names(CTORS), BAD, "a frame without a view", view=None)
    # (without a frame: the view plays no part, the image is the one fault)
    _refused(rig, every, EMPTY, "NULL image", frame=None, null_image=True)
    _refused(rig, _names(("xstereo", "stereo")), EMPTY, "NULL right image", frame=None, null_right=True)
    _refused(rig, every, EMPTY, "width 0", frame=None, w=0, stride=0, rgbd_stride=0, rgbd_depth_stride=0)
    _refused(rig, every, EMPTY, "width -1", frame=None, w=-1, stride=-1)
    _refused(rig, every, EMPTY, "height 0", frame=None, h=0)
    _refused(rig, every, BAD, "stride < width", stride=W - 1, rgbd_stride=W - 1)
    _refused(rig, _names(("extract",) + CTORS, ("sync", "dev")), BAD, "NULL count pointer", has_n=False)
    v = _fresh(rig["g2"]).view
    for field, value in (("min_x", 1.0), ("min_y", -1.0), ("max_x", W - 1.0), ("max_y", H + 0.5)):
        bad = capi.FrameView.from_buffer_copy(v)
        setattr(bad, field, value)
        _refused(rig, _names(CTORS), BAD, "undistorted camera, %s = %g" % (field, value), view=bad)


def test_faults_of_the_monocular_rules(rig):
    """A distorted camera (k1 != 0): mvKeysUn exists as the frame's features, so there must be a frame; its bounds are the undistorted
    corners, any non-empty rectangle, and fx, fy > 0.  The RGB-D constructor takes the same rules."""
    names = _names(("mono", "rgbd"))
    _refused(rig, names, BAD, "active distortion without a frame", dist=EUROC_DIST, frame=None)
    v = rig["g2"].view
    cases = (("fx", 0.0), ("fx", -1.0), ("fy", 0.0), ("max_x", float(v.min_x)), ("max_y", float(v.min_y) - 1.0))
    for field, value in cases:
        bad = capi.FrameView.from_buffer_copy(v)
        setattr(bad, field, value)
        _refused(rig, names, BAD, "distorted camera, %s = %g" % (field, value), dist=EUROC_DIST, view=bad)
    # the same bounds are fine once they are a rectangle of any size
    wide = capi.FrameView.from_buffer_copy(v)
    wide.min_x, wide.max_x = -12.5, W + 9.25
    g = _fresh(rig["g2"], dist=EUROC_DIST, view=wide)
    assert call(rig["lib"], "orbx_frame_mono", g) == OK and g.n.value > 50


def test_faults_of_the_rgbd_descriptor(rig):
    names = _names(("rgbd",))
    _refused(rig, names, BAD, "no descriptor", no_rgbd=True)
    _refused(rig, names, BAD, "short struct_size", rgbd_struct_size=C.sizeof(capi.OrbxRgbdImage) - 4)
    _refused(rig, names, BAD, "no depth image", rgbd_depth=None)
    _refused(rig, names, BAD, "unknown depth type", rgbd_depth_type=2)
    _refused(rig, names, BAD, "two channels", rgbd_channels=2, rgbd_stride=2 * W)
    _refused(rig, names, BAD, "no channel", rgbd_channels=0)
    _refused(rig, names, BAD, "bf = 0", bf=0.0)
    _refused(rig, names, BAD, "bf < 0", bf=-40.0)
    _refused(rig, names, BAD, "bf NaN", bf=float("nan"))
    _refused(rig, names, BAD, "colour stride below 3 * width", rgbd_channels=3, rgbd_stride=3 * W - 1)
    _refused(rig, names, BAD, "depth stride below 2 * width", rgbd_depth_stride=2 * W - 1)
    _refused(rig, names, BAD, "float depth stride below 4 * width", rgbd_depth_type=capi.ORBX_DEPTH_F32, rgbd_depth_stride=4 * W - 2)
    # a depth image resident in HBM is read in place: values aligned to their size.  A host image is repacked: any address.
    resident = _names(("rgbd",), ("dev", "dev_submit"))
    _refused(rig, resident, BAD, "resident depth image at an odd address", rgbd_depth_offset=1)
    _refused(rig, resident, BAD, "resident depth image with an odd stride", rgbd_depth_stride=2 * W + 1)


# ---------------------------------------------------------------- the size rule

def test_image_larger_than_the_handle_was_created_for():
    """A handle created for 160 x 120 and a 320 x 240 image.  The monocular and RGB-D constructors refuse it on every route, the stereo
    constructor on the host-image submit only; orbx_frame_stereo, _dev and _dev_submit take it, rebuild the handle's geometry and give
    what a handle created for 320 x 240 gives."""
    lib = capi.load()
    ex = api.ORBextractor(300, 1.2, 8, 20, 7, W, H, n_cams=2)
    big = api.ORBextractor(300, 1.2, 8, 20, 7, 2 * W, 2 * H, n_cams=2)
    g = Good(ex, 2 * W, 2 * H)
    r = dict(lib=lib, ex2=ex, g2=g)
    _refused(r, _names(("mono", "rgbd")) + ["orbx_frame_stereo_submit"], BAD, "320 x 240 on a 160 x 120 handle")
    _refused(r, _names(("mono", "rgbd")) + ["orbx_frame_stereo_submit"], BAD, "160 x 240 on a 160 x 120 handle", w=W, stride=2 * W)
    ref = _fresh(g, hnd=big.h)
    assert call(lib, "orbx_frame_stereo", ref) == OK and ref.n.value > 100
    ref.frame.n = ref.n.value
    want = (ref.n.value, ref.n_right.value, ref.kps.tobytes(), ref.desc.tobytes(), ref.ur.tobytes(), ref.dp.tobytes(), [a.tobytes() for a in ref.frame.grid()])
    for name in ("orbx_frame_stereo", "orbx_frame_stereo_dev", "orbx_frame_stereo_dev_submit"):
        c = _fresh(g, kps=np.zeros_like(g.kps), desc=np.zeros_like(g.desc), ur=np.zeros_like(g.ur), dp=np.zeros_like(g.dp), frame=api.Frame())
        out = ex.set_frame_outputs(ex.cap) if name.endswith("submit") else None
        assert call(lib, name, c) == OK, name
        if out is not None:
            assert lib.orbx_frame_stereo_dev_wait(ex.h, C.byref(c.n), C.byref(c.n_right)) == OK
            c.kps, c.desc, c.ur, c.dp = out["kps"], out["desc"], out["uright"], out["depth"]
            ex.set_frame_outputs(0)
        n = c.n.value
        c.frame.n = n
        got = (n, c.n_right.value, c.kps.tobytes(), c.desc.tobytes(), c.ur.tobytes(), c.dp.tobytes(), [a.tobytes() for a in c.frame.grid()])
        assert got == want, name


# ---------------------------------------------------------------- a handle with a submission in flight

def _submit_stereo(rig, g):
    assert call(rig["lib"], "orbx_frame_stereo_submit", g) == OK


def test_busy_handle_refuses_everything_and_keeps_its_frame(rig):
    lib, ex = rig["lib"], rig["ex2"]
    ref = _fresh(rig["g2"])
    assert call(lib, "orbx_frame_stereo", ref) == OK
    n = ref.frame.n = ref.n.value
    want_grid = [a.tobytes() for a in ref.frame.grid()]
    for w in ("orbx_frame_stereo_dev_wait", "orbx_frame_stereo_wait"):
        assert getattr(lib, w)(ex.h, None, None) == BAD, w + " with nothing submitted"
    for w in ("orbx_frame_mono_wait", "orbx_frame_rgbd_wait"):
        assert getattr(lib, w)(ex.h, None) == BAD, w + " with nothing submitted"
    out = ex.set_frame_outputs(ex.cap)
    pending = _fresh(rig["g2"], frame=api.Frame())
    _submit_stereo(rig, pending)
    for name in ENTRIES:
        g = _fresh(rig["g2"], frame=api.Frame())
        assert call(lib, name, g) == BAD and g.n.value == -7, name + " on a busy handle"
    spare = np.zeros(ex.cap, capi.KEYPOINT_DTYPE)
    assert lib.orbx_set_frame_outputs(ex.h, None, None, None, None, 0) == BAD
    assert lib.orbx_set_frame_outputs(ex.h, C.c_void_p(capi.ptr(spare)), None, None, None, ex.cap) == BAD
    assert lib.orbx_set_frame_outputs_un(ex.h, C.c_void_p(capi.ptr(spare))) == BAD
    assert lib.orbx_set_frame_outputs_un(ex.h, None) == BAD
    assert lib.orbx_set_stream(ex.h, None) == BAD
    assert lib.orbx_frame_stereo_dev_wait(ex.h, C.byref(pending.n), C.byref(pending.n_right)) == OK
    assert (pending.n.value, pending.n_right.value) == (n, ref.n_right.value) and n > 50
    pending.frame.n = n
    assert out["kps"][:n].tobytes() == ref.kps[:n].tobytes() and out["desc"][:n].tobytes() == ref.desc[:n].tobytes()
    assert out["uright"][:n].tobytes() == ref.ur[:n].tobytes() and out["depth"][:n].tobytes() == ref.dp[:n].tobytes()
    assert [a.tobytes() for a in pending.frame.grid()] == want_grid
    assert not spare.view(np.uint8).any()
    ex.set_frame_outputs(0)
    assert lib.orbx_frame_stereo_dev_wait(ex.h, None, None) == BAD


def test_timeline_row_survives_a_refused_call(rig):
    """A refused call happens before any side effect on the handle, the timeline scratch of the frame in flight included: the row of a
    host-image submission that waited 20 ms (far above the ~0.1 ms of the calls themselves) reports those 20 ms as latency and its own
    pack time, whatever was refused meanwhile."""
    lib, ex = rig["lib"], rig["ex2"]
    ex.ctor_timeline(reset=True)
    pending = _fresh(rig["g2"], frame=api.Frame())
    _submit_stereo(rig, pending)
    time.sleep(0.020)
    for name in ("orbx_frame_stereo", "orbx_frame_stereo_dev_submit"):
        g = _fresh(rig["g2"], frame=api.Frame())
        assert call(lib, name, g) == BAD, name
    assert lib.orbx_frame_stereo_dev_wait(ex.h, C.byref(pending.n), None) == OK and pending.n.value > 50
    rows = ex.ctor_timeline()
    assert len(rows) == 1
    queue, pack, enqueue, wait, latency = [float(v) for v in rows[0]]
    print("timeline row: queue %.1f pack %.1f enqueue %.1f wait %.1f latency %.1f us" % (queue, pack, enqueue, wait, latency))
    assert latency >= 20000.0, "the refused calls restarted the clock of the frame in flight"
    assert pack > 0.0, "the refused calls cleared the pack time of the frame in flight"
