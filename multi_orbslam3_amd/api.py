"""Python host mirror of the reference's interface for the hot path, over the C-ABI of liborbgpu.so.

Class / method names follow the reference (ORBextractor::operator(), Frame::ComputeStereoMatches,
ORBmatcher::SearchByProjection / SearchByBoW, Optimizer::LocalBundleAdjustment); arguments are the flattened
numpy views of SURVEY.md Appendix E.  Every method raises OrbGpuError on a non-zero status -- in particular
ORBG_NO_DEVICE when no MI355X is visible: there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _capi as capi
from . import views


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class ORBextractor:
    """ORB_SLAM3::ORBextractor (I/ORBextractor.h:47-113).  n_cams=2 gives the batched stereo rig."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, max_width=640,
                 max_height=480, n_cams=1, device=0, gauss_taps=None, octree_oldest_first=False):
        """gauss_taps / octree_oldest_first: the two deployment variants of orbx_config (OpenCV >= 4.5: (18, 34, 48, 56))."""
        self.lib = capi.load()
        self.cfg = capi.OrbxConfig(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, max_width, max_height,
                                   n_cams, device, (C.c_int32 * 4)(*(gauss_taps or (0, 0, 0, 0))), int(bool(octree_oldest_first)))
        self.h = C.c_void_p()
        capi.check(self.lib.orbx_create(C.byref(self.cfg), C.byref(self.h)), "orbx_create")
        self.cap = 2 * nfeatures + 256

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # getters of I/ORBextractor.h:65-85
    def tables(self):
        nl = self.cfg.n_levels
        arrs = [np.zeros(nl, np.float32) for _ in range(4)] + [np.zeros(nl, np.int32)]
        capi.check(self.lib.orbx_get_tables(self.h, *[_vp(a) for a in arrs]))
        return arrs

    def GetScaleFactors(self):
        return self.tables()[0]

    def GetInverseScaleSigmaSquares(self):
        return self.tables()[3]

    def __call__(self, image, vLappingArea=(0, 0)):
        """-> (monoIndex or -1, keypoints, descriptors): S/ORBextractor.cc:1068-1150."""
        kps = np.zeros(self.cap, dtype=capi.KEYPOINT_DTYPE)
        desc = np.zeros((self.cap, 32), np.uint8)
        n, nm = C.c_int(0), C.c_int(0)
        if image is None or image.size == 0:
            rc = self.lib.orbx_extract(self.h, 0, None, 0, 0, 0, 0, 0, _vp(kps), _vp(desc), self.cap, C.byref(n), C.byref(nm))
            assert rc == capi.ORBG_EMPTY
            return -1, kps[:0], desc[:0]
        image = np.ascontiguousarray(image, np.uint8)
        rc = self.lib.orbx_extract(self.h, 0, _vp(image), image.shape[1], image.shape[0], image.strides[0],
                                   int(vLappingArea[0]), int(vLappingArea[1]), _vp(kps), _vp(desc), self.cap,
                                   C.byref(n), C.byref(nm))
        capi.check(rc, "orbx_extract")
        return nm.value, kps[: n.value].copy(), desc[: n.value].copy()

    def extract_stereo(self, im_left, im_right, download=True):
        """Both ExtractORB calls of the stereo Frame ctor (S/Frame.cc:92-95) in one batched submission."""
        im_left = np.ascontiguousarray(im_left, np.uint8)
        im_right = np.ascontiguousarray(im_right, np.uint8)
        assert im_left.shape == im_right.shape and im_left.strides == im_right.strides
        nl, nr = C.c_int(0), C.c_int(0)
        if download:
            kl = np.zeros(self.cap, capi.KEYPOINT_DTYPE); dl = np.zeros((self.cap, 32), np.uint8)
            kr = np.zeros(self.cap, capi.KEYPOINT_DTYPE); dr = np.zeros((self.cap, 32), np.uint8)
        else:
            kl = dl = kr = dr = None
        rc = self.lib.orbx_extract_stereo(self.h, _vp(im_left), _vp(im_right), im_left.shape[1], im_left.shape[0],
                                          im_left.strides[0], _vp(kl), _vp(dl), self.cap, C.byref(nl), _vp(kr), _vp(dr),
                                          self.cap, C.byref(nr))
        capi.check(rc, "orbx_extract_stereo")
        if not download:
            return nl.value, nr.value
        return (kl[: nl.value].copy(), dl[: nl.value].copy()), (kr[: nr.value].copy(), dr[: nr.value].copy())

    def extract_stereo_dev(self, d_left, d_right, width, height, stride, download_left=False):
        """Images already in HBM (raw device pointers, e.g. torch tensor .data_ptr()).  Right-camera features always
        stay on the device; the left ones are also copied to the host when download_left is set."""
        nl, nr = C.c_int(0), C.c_int(0)
        kl = dl = None
        if download_left:
            if not hasattr(self, "_kl"):
                self._kl = np.zeros(self.cap, capi.KEYPOINT_DTYPE)
                self._dl = np.zeros((self.cap, 32), np.uint8)
            kl, dl = self._kl, self._dl
        rc = self.lib.orbx_extract_stereo_dev(self.h, C.c_void_p(d_left), C.c_void_p(d_right), width, height, stride,
                                              _vp(kl), _vp(dl), self.cap, C.byref(nl), None, None, 0, C.byref(nr))
        capi.check(rc, "orbx_extract_stereo_dev")
        if download_left:
            return nl.value, nr.value, kl[: nl.value], dl[: nl.value]
        return nl.value, nr.value

    def frame_stereo(self, frame, fv, im_left, im_right, bf, b, download=True):
        """Host-image variant of frame_stereo_dev (the actual Frame ctor hands over cv::Mat images)."""
        im_left = np.ascontiguousarray(im_left, np.uint8)
        im_right = np.ascontiguousarray(im_right, np.uint8)
        self._host_imgs = (im_left, im_right)
        return self.frame_stereo_dev(frame, fv, im_left.ctypes.data, im_right.ctypes.data, im_left.shape[1], im_left.shape[0],
                                     im_left.strides[0], bf, b, download, _fn=self.lib.orbx_frame_stereo)

    def frame_stereo_dev_submit(self, frame, fv, d_left, d_right, width, height, stride, bf, b):
        """First half of frame_stereo_dev: enqueue the Frame constructor and return; other handles / frames may be used
        until frame_stereo_dev_wait (the chain overlaps with their kernels on the GPU)."""
        self._pending = (frame, fv)                    # keep the view alive
        rc = self.lib.orbx_frame_stereo_dev_submit(self.h, frame.h if frame is not None else None, C.byref(fv), C.c_void_p(d_left),
                                                   C.c_void_p(d_right), width, height, stride, C.c_float(bf), C.c_float(b))
        capi.check(rc, "orbx_frame_stereo_dev_submit")

    def frame_stereo_submit(self, frame, fv, im_left, im_right, bf, b, async_ingest=False):
        """First half of the Frame constructor with HOST images (orbx_frame_stereo_submit): rows packed into the handle's
        pinned staging slot, one copy kernel + the constructor chain enqueued; collect with frame_stereo_dev_wait().  With
        async_ingest the packing and the launches run on the library's ingest thread and the call returns at once (the
        images are kept alive here until the wait)."""
        assert im_left.dtype == np.uint8 and im_right.dtype == np.uint8 and im_left.shape == im_right.shape
        assert im_left.strides[1] == 1 and im_right.strides == im_left.strides
        self._pending = (frame, fv, im_left, im_right)
        rc = self.lib.orbx_frame_stereo_submit(self.h, frame.h if frame is not None else None, C.byref(fv), C.c_void_p(im_left.ctypes.data),
                                               C.c_void_p(im_right.ctypes.data), im_left.shape[1], im_left.shape[0], im_left.strides[0],
                                               C.c_float(bf), C.c_float(b), 1 if async_ingest else 0)
        capi.check(rc, "orbx_frame_stereo_submit")

    def set_frame_outputs(self, cap):
        """orbx_set_frame_outputs: the two-halves constructor delivers mvKeys / mDescriptors / mvuRight / mvDepth of the left image
        into host arrays owned by this object (returned) by the time frame_stereo_dev_wait() returns; cap = 0 switches it off."""
        if cap <= 0:
            capi.check(self.lib.orbx_set_frame_outputs(self.h, None, None, None, None, 0), "orbx_set_frame_outputs")
            self._outputs = None
            return None
        out = dict(kps=np.zeros(cap, capi.KEYPOINT_DTYPE), desc=np.zeros((cap, 32), np.uint8), uright=np.zeros(cap, np.float32),
                   depth=np.zeros(cap, np.float32), kps_un=np.zeros(cap, capi.KEYPOINT_DTYPE))
        capi.check(self.lib.orbx_set_frame_outputs(self.h, C.c_void_p(capi.ptr(out["kps"])), C.c_void_p(capi.ptr(out["desc"])),
                                                   C.c_void_p(capi.ptr(out["uright"])), C.c_void_p(capi.ptr(out["depth"])), int(cap)),
                   "orbx_set_frame_outputs")
        # (mvKeysUn: delivered by the monocular constructor only)
        capi.check(self.lib.orbx_set_frame_outputs_un(self.h, C.c_void_p(capi.ptr(out["kps_un"]))), "orbx_set_frame_outputs_un")
        self._outputs = out
        return out

    # ---- the monocular Frame constructor (S/Frame.cc:260-358)
    @staticmethod
    def _dist(dist):
        """(k1, k2, p1, p2[, k3]) / capi.OrbxDistortion / None -> (keep-alive object, ctypes argument)"""
        if dist is None:
            return None, None
        d = dist if isinstance(dist, capi.OrbxDistortion) else capi.OrbxDistortion(*([float(v) for v in dist] + [0.0] * (5 - len(dist))))
        return d, C.byref(d)

    def frame_mono(self, frame, fv, image, dist=None, download=True, device_ptr=None, size=None):
        """Frame::Frame(mono): ExtractORB(0, im, 0, 1000) + UndistortKeyPoints + grid in ONE submission (orbx_frame_mono);
        -> (n, mvKeys, mvKeysUn, mDescriptors) or n.  device_ptr/size=(w, h, stride): the image is resident in HBM."""
        n = C.c_int(0)
        kps = kun = desc = None
        if download:
            kps = np.zeros(self.cap, capi.KEYPOINT_DTYPE); kun = np.zeros(self.cap, capi.KEYPOINT_DTYPE); desc = np.zeros((self.cap, 32), np.uint8)
        dk, darg = self._dist(dist)
        if device_ptr is not None:
            w, h, stride = size
            rc = self.lib.orbx_frame_mono_dev(self.h, frame.h if frame is not None else None, C.byref(fv), darg, C.c_void_p(device_ptr), w, h, stride,
                                              _vp(kps), _vp(kun), _vp(desc), self.cap, C.byref(n))
        else:
            image = np.ascontiguousarray(image, np.uint8)
            rc = self.lib.orbx_frame_mono(self.h, frame.h if frame is not None else None, C.byref(fv), darg, _vp(image), image.shape[1],
                                          image.shape[0], image.strides[0], _vp(kps), _vp(kun), _vp(desc), self.cap, C.byref(n))
        capi.check(rc, "orbx_frame_mono")
        if frame is not None:
            frame.n = n.value
        if download:
            return n.value, kps[: n.value].copy(), kun[: n.value].copy(), desc[: n.value].copy()
        return n.value

    def frame_mono_submit(self, frame, fv, image, dist=None, async_ingest=False, device_ptr=None, size=None):
        """First half of the monocular constructor (orbx_frame_mono_submit / _dev_submit); collect with frame_mono_wait()."""
        dk, darg = self._dist(dist)
        if device_ptr is not None:
            w, h, stride = size
            self._pending = (frame, fv, dk)
            rc = self.lib.orbx_frame_mono_dev_submit(self.h, frame.h if frame is not None else None, C.byref(fv), darg, C.c_void_p(device_ptr), w, h, stride)
        else:
            assert image.dtype == np.uint8 and image.strides[1] == 1
            self._pending = (frame, fv, dk, image)
            rc = self.lib.orbx_frame_mono_submit(self.h, frame.h if frame is not None else None, C.byref(fv), darg, C.c_void_p(image.ctypes.data),
                                                 image.shape[1], image.shape[0], image.strides[0], 1 if async_ingest else 0)
        capi.check(rc, "orbx_frame_mono_submit")

    def frame_mono_wait(self):
        return self.frame_stereo_dev_wait()[0]

    # ---- the RGB-D Frame constructor (S/Tracking.cc:1086-1142, S/Frame.cc:174-257)
    @staticmethod
    def _rgbd_image(image, depth, depth_factor, rgb_order, device_ptrs=None, size=None):
        """-> (orbx_rgbd_image, width, height, keep-alive).  Host arrays: image H x W (gray) or H x W x 3 / 4 uint8, depth H x W uint16 or
        float32; rows may be padded (any row stride, unit pixel stride).  device_ptrs = (image pointer, depth pointer) with
        size = (w, h, channels, stride, depth dtype, depth stride in bytes) for images resident in HBM."""
        im = capi.OrbxRgbdImage()
        im.struct_size = C.sizeof(capi.OrbxRgbdImage)
        im.rgb_order = int(bool(rgb_order))
        im.depth_factor = float(np.float32(depth_factor))
        if device_ptrs is not None:
            w, h, ch, stride, ddtype, dstride = size
            im.img, im.depth = device_ptrs
            im.channels, im.stride, im.depth_stride = int(ch), int(stride), int(dstride)
            im.depth_type = capi.ORBX_DEPTH_U16 if np.dtype(ddtype) == np.uint16 else capi.ORBX_DEPTH_F32
            return im, int(w), int(h), None
        if image is None or image.size == 0:
            return im, 0, 0, None
        assert image.dtype == np.uint8 and image.ndim in (2, 3) and image.strides[1] == (image.shape[2] if image.ndim == 3 else 1)
        assert image.ndim == 2 or image.strides[2] == 1
        im.img = image.ctypes.data
        im.channels = image.shape[2] if image.ndim == 3 else 1
        im.stride = image.strides[0]
        if depth is not None:
            assert depth.dtype in (np.uint16, np.float32) and depth.shape == image.shape[:2] and depth.strides[1] == depth.itemsize
            im.depth = depth.ctypes.data
            im.depth_type = capi.ORBX_DEPTH_U16 if depth.dtype == np.uint16 else capi.ORBX_DEPTH_F32
            im.depth_stride = depth.strides[0]
        return im, image.shape[1], image.shape[0], (image, depth)

    def frame_rgbd(self, frame, fv, image, depth, bf, depth_factor=1.0, dist=None, rgb_order=False, download=True, device_ptrs=None,
                   size=None):
        """GrabImageRGBD + Frame::Frame(RGB-D) in ONE submission (orbx_frame_rgbd / _dev): colour -> gray, ExtractORB(0, im, 0, 0),
        UndistortKeyPoints, ComputeStereoFromRGBD, grid; -> (n, mvKeys, mvKeysUn, mDescriptors, mvuRight, mvDepth) or n.
        depth_factor is Tracking's mDepthMapFactor (api.depth_map_factor of the YAML value)."""
        im, w, h, keep = self._rgbd_image(image, depth, depth_factor, rgb_order, device_ptrs, size)
        n = C.c_int(0)
        kps = kun = desc = ur = dp = None
        if download:
            kps = np.zeros(self.cap, capi.KEYPOINT_DTYPE); kun = np.zeros(self.cap, capi.KEYPOINT_DTYPE); desc = np.zeros((self.cap, 32), np.uint8)
            ur = np.zeros(self.cap, np.float32); dp = np.zeros(self.cap, np.float32)
        dk, darg = self._dist(dist)
        fn = self.lib.orbx_frame_rgbd_dev if device_ptrs is not None else self.lib.orbx_frame_rgbd
        rc = fn(self.h, frame.h if frame is not None else None, C.byref(fv) if fv is not None else None, darg, C.byref(im), w, h, float(bf),
                capi.ptr(kps), capi.ptr(kun), capi.ptr(desc), capi.ptr(ur), capi.ptr(dp), self.cap, C.byref(n))
        capi.check(rc, "orbx_frame_rgbd")
        if frame is not None:
            frame.n = n.value
        if download:
            m = n.value
            return m, kps[:m].copy(), kun[:m].copy(), desc[:m].copy(), ur[:m].copy(), dp[:m].copy()
        return n.value

    def frame_rgbd_submit(self, frame, fv, image, depth, bf, depth_factor=1.0, dist=None, rgb_order=False, async_ingest=False,
                          device_ptrs=None, size=None):
        """First half of the RGB-D constructor (orbx_frame_rgbd_submit / _dev_submit); collect with frame_rgbd_wait().  The features
        reach the arrays of set_frame_outputs()."""
        im, w, h, keep = self._rgbd_image(image, depth, depth_factor, rgb_order, device_ptrs, size)
        dk, darg = self._dist(dist)
        self._pending = (frame, fv, dk, im, keep)
        fr = frame.h if frame is not None else None
        if device_ptrs is not None:
            rc = self.lib.orbx_frame_rgbd_dev_submit(self.h, fr, C.byref(fv), darg, C.byref(im), w, h, float(bf))
        else:
            rc = self.lib.orbx_frame_rgbd_submit(self.h, fr, C.byref(fv), darg, C.byref(im), w, h, float(bf), 1 if async_ingest else 0)
        capi.check(rc, "orbx_frame_rgbd_submit")

    def frame_rgbd_wait(self):
        n = C.c_int(0)
        capi.check(self.lib.orbx_frame_rgbd_wait(self.h, C.byref(n)), "orbx_frame_rgbd_wait")
        frame = self._pending[0] if getattr(self, "_pending", None) else None
        if frame is not None:
            frame.n = n.value
        self._pending = None
        return n.value

    def frame_stereo_dev_wait(self):
        nl, nr = C.c_int(0), C.c_int(0)
        capi.check(self.lib.orbx_frame_stereo_dev_wait(self.h, C.byref(nl), C.byref(nr)), "orbx_frame_stereo_dev_wait")
        frame = self._pending[0] if getattr(self, "_pending", None) else None
        if frame is not None:
            frame.n = nl.value
        self._pending = None
        return nl.value, nr.value

    def frame_stereo_dev(self, frame, fv, d_left, d_right, width, height, stride, bf, b, download=False, _fn=None):
        """Frame::Frame(stereo) (S/Frame.cc:71-172) in one submission: extract L+R, ComputeStereoMatches and the
        feature grid, one final sync; `frame` views the left features on the device afterwards."""
        nl, nr = C.c_int(0), C.c_int(0)
        kl = dl = ur = dp = None
        if download:
            if not hasattr(self, "_kl"):
                self._kl = np.zeros(self.cap, capi.KEYPOINT_DTYPE)
                self._dl = np.zeros((self.cap, 32), np.uint8)
            if not hasattr(self, "_ur"):
                self._ur = np.zeros(self.cap, np.float32)
                self._dp = np.zeros(self.cap, np.float32)
            kl, dl, ur, dp = self._kl, self._dl, self._ur, self._dp
        fn = _fn if _fn is not None else self.lib.orbx_frame_stereo_dev
        rc = fn(self.h, frame.h if frame is not None else None, C.byref(fv), C.c_void_p(d_left),
                C.c_void_p(d_right), width, height, stride, C.c_float(bf), C.c_float(b), _vp(kl),
                _vp(dl), _vp(ur), _vp(dp), self.cap, C.byref(nl), C.byref(nr))
        capi.check(rc, "orbx_frame_stereo_dev")
        if frame is not None:
            frame.n = nl.value
        if download:
            n = nl.value
            return n, nr.value, kl[:n], dl[:n], ur[:n], dp[:n]
        return nl.value, nr.value

    def level(self, cam, level, border=False):
        """mvImagePyramid[level] (I/ORBextractor.h:87) of the last extraction; border=True includes the 19-px border."""
        w, h = C.c_int(0), C.c_int(0)
        fn = self.lib.orbx_get_level_bordered if border else self.lib.orbx_get_level
        capi.check(fn(self.h, cam, level, None, C.byref(w), C.byref(h)))
        e = 38 if border else 0
        out = np.zeros((h.value + e, w.value + e), np.uint8)
        capi.check(fn(self.h, cam, level, _vp(out), C.byref(w), C.byref(h)))
        return out

    def candidates(self, cam, level, cap=1 << 18):
        out = np.zeros((cap, 3), np.int32)
        n = C.c_int(0)
        capi.check(self.lib.orbx_get_candidates(self.h, cam, level, _vp(out), cap, C.byref(n)))
        return out[: n.value].copy()

    def ComputeStereoMatches(self, bf, b, n_left=None, download=True):
        """Frame::ComputeStereoMatches (S/Frame.cc:785-963) on the device-resident stereo extraction."""
        if not download:
            capi.check(self.lib.orbx_stereo_match(self.h, C.c_float(bf), C.c_float(b), None, None))
            return None
        ur = np.zeros(max(n_left if n_left is not None else self.cap, 1), np.float32)
        dp = np.zeros_like(ur)
        capi.check(self.lib.orbx_stereo_match(self.h, C.c_float(bf), C.c_float(b), _vp(ur), _vp(dp)), "orbx_stereo_match")
        if n_left is not None:
            return ur[:n_left], dp[:n_left]
        return ur, dp

    def ctor_timeline(self, reset=False):
        """Host-side timeline of the last Frame constructors of this handle: array [n, 5] of microseconds
        (queue, pack, enqueue, wait, latency), oldest first (orbx_get_ctor_timeline)."""
        out = np.zeros((512, 5), np.float32)
        n = C.c_int(0)
        capi.check(self.lib.orbx_get_ctor_timeline(self.h, _vp(out), 512, C.byref(n), int(bool(reset))), "orbx_get_ctor_timeline")
        return out[: n.value].copy()

    def set_profiling(self, level):
        capi.check(self.lib.orbx_set_profiling(self.h, int(level)))

    def set_profile_interval(self, interval, reset=True):
        capi.check(self.lib.orbx_set_profile_interval(self.h, int(interval), int(bool(reset))), "orbx_set_profile_interval")

    PROF_KERNELS = {"fast_cells_kernel": 0, "octree_kernel": 1, "orient_desc_gpu_kernel": 2, "pyr_tower_kernel": 3}

    def set_profile_kernel(self, name):
        """Which kernel of the constructor chain the level-1 event pair brackets (resets the accumulated times)."""
        capi.check(self.lib.orbx_set_profile_kernel(self.h, self.PROF_KERNELS[name]), "orbx_set_profile_kernel")

    def fast_kernel_stats(self):
        s, n = C.c_double(0.0), C.c_int64(0)
        capi.check(self.lib.orbx_get_fast_kernel_stats(self.h, C.byref(s), C.byref(n)), "orbx_get_fast_kernel_stats")
        return s.value, n.value

    def host_redo_count(self):
        """Frames this handle redid with the host quad-trees because a device list overflowed (orbx_get_host_redo_count)."""
        n = C.c_int64(0)
        capi.check(self.lib.orbx_get_host_redo_count(self.h, C.byref(n)), "orbx_get_host_redo_count")
        return n.value

    def event_overhead_ms(self, reps=50):
        ms = C.c_float(0.0)
        capi.check(self.lib.orbx_event_overhead(self.h, int(reps), C.byref(ms)), "orbx_event_overhead")
        return ms.value

    def timings(self):
        t = np.zeros(8, np.float32)
        capi.check(self.lib.orbx_get_timings(self.h, _vp(t)))
        return dict(pyramid_ms=float(t[0]), fast_ms=float(t[1]), octree_host_ms=float(t[2]), desc_ms=float(t[3]),
                    stereo_ms=float(t[4]), fast_kernel_ms=float(t[5]))


def undistort_points(xy, cam4, dist, device=0):
    """cv::undistortPoints(pts, pts, K, mDistCoef, Mat(), K) on the device (orbx_undistort_points): xy n x 2 float32."""
    lib = capi.load()
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out = np.zeros_like(xy)
    dk, darg = ORBextractor._dist(dist)
    capi.check(lib.orbx_undistort_points(int(device), _vp(xy), len(xy), C.c_float(cam4[0]), C.c_float(cam4[1]), C.c_float(cam4[2]),
                                         C.c_float(cam4[3]), darg, _vp(out)), "orbx_undistort_points")
    return out


def depth_map_factor(yaml_value):
    """The float Tracking holds as mDepthMapFactor (S/Tracking.cc:166-172) for the YAML's DepthMapFactor: 1 when
    fabs(value) < 1e-5, else 1.0f / value."""
    f = np.float32(yaml_value)
    return np.float32(1.0) if abs(f) < 1e-5 else np.float32(1.0) / f


def depth_at_points(xy, depth_img, bf, depth_factor=1.0, xy_un=None, device=0):
    """Frame::ComputeStereoFromRGBD on given points (orbx_depth_at_points): xy = mvKeys' n x 2 float32, xy_un = mvKeysUn's (None: xy),
    depth_img = the raw depth image (uint16 or float32, rows may be padded) -> (mvuRight, mvDepth)."""
    lib = capi.load()
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    un = None if xy_un is None else np.ascontiguousarray(xy_un, np.float32).reshape(-1, 2)
    assert un is None or len(un) == len(xy)
    assert depth_img.dtype in (np.uint16, np.float32) and depth_img.ndim == 2 and depth_img.strides[1] == depth_img.itemsize
    ur = np.zeros(len(xy), np.float32); dp = np.zeros(len(xy), np.float32)
    capi.check(lib.orbx_depth_at_points(int(device), capi.ptr(xy), capi.ptr(un), len(xy), depth_img.ctypes.data,
                                        capi.ORBX_DEPTH_U16 if depth_img.dtype == np.uint16 else capi.ORBX_DEPTH_F32,
                                        depth_img.strides[0], depth_img.shape[1], depth_img.shape[0], float(np.float32(depth_factor)),
                                        float(bf), capi.ptr(ur), capi.ptr(dp)), "orbx_depth_at_points")
    return ur, dp


def image_bounds(width, height, cam4, dist, device=0):
    """Frame::ComputeImageBounds (S/Frame.cc:756-783) -> (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    if dist is None or float(np.float32(dist[0] if not isinstance(dist, capi.OrbxDistortion) else dist.k1)) == 0.0:
        return (0.0, float(width), 0.0, float(height))
    m = undistort_points(np.array([[0, 0], [width, 0], [0, height], [width, height]], np.float32), cam4, dist, device)
    return (float(min(m[0, 0], m[2, 0])), float(max(m[1, 0], m[3, 0])), float(min(m[0, 1], m[1, 1])), float(max(m[2, 1], m[3, 1])))


class Frame:
    """Device-resident frame view (features + 64x48 grid) the matchers work on."""

    def __init__(self, cap_features=4096, device=0):
        self.lib = capi.load()
        self.h = C.c_void_p()
        capi.check(self.lib.orbm_frame_create(device, cap_features, C.byref(self.h)), "orbm_frame_create")
        self.n = 0
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbm_frame_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, fv, keep=None):
        self._keep = keep
        capi.check(self.lib.orbm_frame_upload(self.h, C.byref(fv)), "orbm_frame_upload")
        self.n = fv.n
        return self

    def from_extractor(self, extractor, fv, n_left):
        """Features, uRight and depth are taken device-to-device from the extractor's left camera."""
        fv.n = int(n_left)
        capi.check(self.lib.orbm_frame_from_extractor(self.h, extractor.h, C.byref(fv)), "orbm_frame_from_extractor")
        self.n = int(n_left)
        return self

    # ---- KeyFrame wire blocks (orb_slam3_ros/KF: N x CvKeyPoint 15 B + N x Descriptor 32 B)
    def pack_wire(self, device_ptr=None):
        """Features -> wire block; into device memory at device_ptr (for the RCCL exchange) or returned as a numpy array."""
        if device_ptr is not None:
            capi.check(self.lib.orbk_pack_frame(self.h, C.c_void_p(int(device_ptr)), 1), "orbk_pack_frame")
            return None
        wire = np.zeros(max(47 * self.n, 1), np.uint8)
        capi.check(self.lib.orbk_pack_frame(self.h, _vp(wire), 0), "orbk_pack_frame")
        return wire[: 47 * self.n]

    def from_wire(self, fv, wire=None, n=0, device_ptr=None):
        """KeyFrame received as a wire block (numpy bytes or device pointer) -> device-resident frame with its grid."""
        if device_ptr is not None:
            capi.check(self.lib.orbk_frame_from_wire(self.h, C.byref(fv), C.c_void_p(int(device_ptr)), int(n), 1), "orbk_frame_from_wire")
        else:
            wire = np.ascontiguousarray(wire, np.uint8)
            capi.check(self.lib.orbk_frame_from_wire(self.h, C.byref(fv), _vp(wire), int(n), 0), "orbk_frame_from_wire")
        self.n = int(n)
        return self

    def download(self):
        kps = np.zeros(max(self.n, 1), capi.KEYPOINT_DTYPE); desc = np.zeros((max(self.n, 1), 32), np.uint8)
        capi.check(self.lib.orbm_frame_download(self.h, _vp(kps), _vp(desc)), "orbm_frame_download")
        return kps[: self.n], desc[: self.n]

    def grid(self):
        start = np.zeros(capi.GRID_COLS * capi.GRID_ROWS + 1, np.int32)
        items = np.zeros(max(self.n, 1), np.int32)
        capi.check(self.lib.orbm_frame_get_grid(self.h, _vp(start), _vp(items)))
        return start, items[: start[-1]].copy()

    def isInFrustum(self, Tcw, wv, viewingCosLimit=0.5):
        m = wv.m
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        out = dict(track_in_view=np.zeros(m, np.uint8), proj_x=np.zeros(m, np.float32), proj_y=np.zeros(m, np.float32),
                   proj_xr=np.zeros(m, np.float32), track_depth=np.zeros(m, np.float32),
                   scale_level=np.zeros(m, np.int32), view_cos=np.zeros(m, np.float32))
        capi.check(self.lib.orbm_is_in_frustum(self.h, _vp(T), C.byref(wv), C.c_float(viewingCosLimit),
                                               *[_vp(out[k]) for k in ("track_in_view", "proj_x", "proj_y", "proj_xr",
                                                                         "track_depth", "scale_level", "view_cos")]),
                   "orbm_is_in_frustum")
        return out

    def isInFrustumRig(self, Tcw, rig, Tlr, wv, viewingCosLimit=0.5):
        """Frame::isInFrustum of a two-camera frame (S/Frame.cc:545-554,1154-1231); self is the LEFT camera's frame.  Returns the two
        cameras' track fields (left dict, right dict)."""
        m = wv.m
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        tlr = np.ascontiguousarray(np.asarray(Tlr, np.float32).reshape(-1)[:12])
        keys = ("track_in_view", "proj_x", "proj_y", "track_depth", "scale_level", "view_cos")
        mk = lambda: dict(track_in_view=np.zeros(m, np.uint8), proj_x=np.zeros(m, np.float32), proj_y=np.zeros(m, np.float32),
                          track_depth=np.zeros(m, np.float32), scale_level=np.zeros(m, np.int32), view_cos=np.zeros(m, np.float32))
        a, b = mk(), mk()
        capi.check(self.lib.orbm_is_in_frustum_rig(self.h, _vp(T), C.byref(rig), _vp(tlr), C.byref(wv), C.c_float(viewingCosLimit),
                                                   *[_vp(d[k]) for d in (a, b) for k in keys]), "orbm_is_in_frustum_rig")
        return a, b


def ComputeStereoFishEyeMatches(view, device=0):
    """Frame::ComputeStereoFishEyeMatches (S/Frame.cc:1093-1150) on an orbx_fisheye_stereo_view: (mvLeftToRightMatch, mvRightToLeftMatch,
    mvDepth, mvStereo3Dpoints as (Nleft, 3), nMatches)."""
    l2r = np.zeros(max(view.n_left, 1), np.int32); r2l = np.zeros(max(view.n_right, 1), np.int32)
    depth = np.zeros(max(view.n_left, 1), np.float32); p3d = np.zeros((max(view.n_left, 1), 3), np.float32)
    n = C.c_int(0)
    capi.check(capi.load().orbx_fisheye_stereo_matches(int(device), C.byref(view), _vp(l2r), _vp(r2l), _vp(depth), _vp(p3d), C.byref(n)),
               "orbx_fisheye_stereo_matches")
    return l2r[: view.n_left], r2l[: view.n_right], depth[: view.n_left], p3d[: view.n_left], n.value


class LocalMap:
    """Device-resident local map points (positions, normals, distances, descriptors)."""

    def __init__(self, cap_points=8192, device=0):
        self.lib = capi.load()
        self.h = C.c_void_p()
        capi.check(self.lib.orbm_map_create(device, cap_points, C.byref(self.h)), "orbm_map_create")

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbm_map_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, wv):
        capi.check(self.lib.orbm_map_upload(self.h, C.byref(wv)), "orbm_map_upload")
        self.m = wv.m
        return self


class LastFrameOnDevice:
    """mLastFrame's view for SearchByProjection(Current, Last), resident on the device (orbm_lastview_*): uploaded when the tracking
    of that frame has finished, read from HBM by the next frame's search."""

    def __init__(self, cap_features=4096, device=0):
        self.lib = capi.load()
        self.h = C.c_void_p()
        capi.check(self.lib.orbm_lastview_create(device, cap_features, C.byref(self.h)), "orbm_lastview_create")

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbm_lastview_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, lv):
        capi.check(self.lib.orbm_lastview_upload(self.h, C.byref(lv)), "orbm_lastview_upload")
        return self


class ORBmatcher:
    """ORB_SLAM3::ORBmatcher (I/ORBmatcher.h:35-108), hot-path searches only."""

    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self.lib = capi.load()
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        self.device = device

    def DescriptorDistance(self, q, t):
        """Dense Hamming matrix (S/ORBmatcher.cc:2358-2374 for every pair)."""
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        d = np.zeros((len(q), len(t)), np.int32)
        capi.check(self.lib.orbm_hamming_matrix(self.device, _vp(q), len(q), _vp(t), len(t), _vp(d)), "orbm_hamming_matrix")
        return d

    def best2(self, q, t):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        o = np.zeros((len(q), 4), np.int32)
        capi.check(self.lib.orbm_hamming_best2(self.device, _vp(q), len(q), _vp(t), len(t), _vp(o)), "orbm_hamming_best2")
        return o

    def SearchForInitialization(self, F1, F2, vbPrevMatched, windowSize=10, debug=False, list_capacity=0):
        """(Frame& F1, Frame& F2, vbPrevMatched, vnMatches12, windowSize): S/ORBmatcher.cc:702-817, on two resident monocular frames.
        -> (nmatches, vnMatches12, vbPrevMatched[, lists]); the input array is not modified.  lists (debug=True): list_start (n1 + 1),
        entries (index2 | dist << 16, in the reference's candidate order) and the counters of orbm_init_search_debug."""
        prev_in = np.ascontiguousarray(vbPrevMatched, np.float32).reshape(-1, 2)
        n1 = len(prev_in)
        prm = capi.InitSearchParams(C.sizeof(capi.InitSearchParams), int(windowSize), self.mfNNratio, int(self.mbCheckOrientation),
                                    int(list_capacity))
        cap = 1 << 18
        while True:
            prev = prev_in.copy()
            m12 = np.full(max(n1, 1), -1, np.int32)
            n = C.c_int(0)
            dbg = start = entries = None
            if debug:
                start = np.zeros(n1 + 1, np.int32); entries = np.zeros(cap, np.uint32)
                dbg = capi.InitSearchDebug(capi.ptr(start), capi.ptr(entries), cap, 0, 0, 0, 0, 0)
            rc = self.lib.orbm_search_for_initialization(F1.h, F2.h, _vp(prev), n1, C.byref(prm), _vp(m12), C.byref(n),
                                                         C.byref(dbg) if debug else None)
            if debug and rc == capi.ORBG_CAP_EXCEEDED and dbg.n_candidates > cap:      # the lists need more room: the same call again
                cap = int(dbg.n_candidates)
                continue
            capi.check(rc, "orbm_search_for_initialization")
            break
        if not debug:
            return n.value, m12[:n1], prev
        lists = dict(list_start=start, entries=entries[: int(start[n1])].copy(), n_queries=dbg.n_queries, n_candidates=dbg.n_candidates,
                     n_evictions=dbg.n_evictions, n_rot_rejected=dbg.n_rot_rejected, n_regrown=dbg.n_regrown)
        return n.value, m12[:n1], prev, lists

    def SearchByProjection(self, F, mv, th=1.0, bFarPoints=False, thFarPoints=50.0, assigned_mp=None, assigned_obs=None):
        """(Frame&, vector<MapPoint*>&, th, bFarPoints, thFarPoints): S/ORBmatcher.cc:44-214."""
        amp = np.ascontiguousarray(assigned_mp, np.int32).copy()
        aob = np.ascontiguousarray(assigned_obs, np.int32).copy()
        n = C.c_int(0)
        capi.check(self.lib.orbm_search_by_projection_mps(F.h, C.byref(mv), C.c_float(th), int(bFarPoints),
                                                          C.c_float(thFarPoints), C.c_float(self.mfNNratio), _vp(amp),
                                                          _vp(aob), C.byref(n)), "orbm_search_by_projection_mps")
        return amp, aob, n.value

    def SearchByProjectionRig(self, FL, FR, mv, mv_r, left_to_right, right_to_left, th=1.0, bFarPoints=False, thFarPoints=50.0,
                              assigned_mp=None, assigned_obs=None):
        """SearchByProjection(Frame&, vector<MapPoint*>&, ...) on a two-camera frame (S/ORBmatcher.cc:44-214 with :145-211)."""
        amp = np.ascontiguousarray(assigned_mp, np.int32).copy()
        aob = np.ascontiguousarray(assigned_obs, np.int32).copy()
        l2r = np.ascontiguousarray(left_to_right, np.int32); r2l = np.ascontiguousarray(right_to_left, np.int32)
        n = C.c_int(0)
        capi.check(self.lib.orbm_search_by_projection_mps_rig(FL.h, FR.h, C.byref(mv), C.byref(mv_r), _vp(l2r), _vp(r2l), C.c_float(th),
                                                              int(bFarPoints), C.c_float(thFarPoints), C.c_float(self.mfNNratio), _vp(amp),
                                                              _vp(aob), C.byref(n)), "orbm_search_by_projection_mps_rig")
        return amp, aob, n.value

    def SearchByProjectionFrameRig(self, FL, FR, Tcw_cur, rig, lv, th, bMono=False, assigned_mp=None, assigned_obs=None):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) on a two-camera current frame (S/ORBmatcher.cc:1970-2186 with :2092-2160);
        FR = None with a rig that has no right camera: one camera behind a model (a monocular fisheye frame)."""
        amp = np.ascontiguousarray(assigned_mp, np.int32).copy()
        aob = np.ascontiguousarray(assigned_obs, np.int32).copy()
        T = np.ascontiguousarray(Tcw_cur, np.float32).reshape(16)
        n = C.c_int(0)
        capi.check(self.lib.orbm_search_by_projection_frame_rig(FL.h, FR.h if FR is not None else None, _vp(T), C.byref(rig), C.byref(lv), C.c_float(th), int(bMono),
                                                                int(self.mbCheckOrientation), _vp(amp), _vp(aob), C.byref(n)),
                   "orbm_search_by_projection_frame_rig")
        return amp, aob, n.value

    def SearchLocalPoints(self, F, local_map, Tcw, th=1.0, bFarPoints=False, thFarPoints=50.0, assigned_mp=None,
                          assigned_obs=None, skip=None, inplace=False, in_frustum=None):
        """Fused Tracking::SearchLocalPoints body (S/Tracking.cc:3111-3153).  in_frustum: optional uint8[m] output, 1 where
        isInFrustum() returned true (the points the reference calls IncreaseVisible() for)."""
        amp, aob = self._state(assigned_mp, assigned_obs, inplace)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        n = C.c_int(0)
        if in_frustum is not None:
            assert in_frustum.dtype == np.uint8 and in_frustum.flags["C_CONTIGUOUS"]
        capi.check(self.lib.orbm_search_local_points_vis(F.h, local_map.h, _vp(T), _vp(sk), C.c_float(th), int(bFarPoints),
                                                         C.c_float(thFarPoints), C.c_float(self.mfNNratio), _vp(amp), _vp(aob),
                                                         C.byref(n), _vp(in_frustum)), "orbm_search_local_points")
        return amp, aob, n.value

    @staticmethod
    def _state(assigned_mp, assigned_obs, inplace):
        """F.mvpMapPoints flattened; inplace=True updates the caller's int32 arrays (as the C ABI does) instead of copies."""
        if inplace:
            assert assigned_mp.dtype == np.int32 and assigned_obs.dtype == np.int32
            return assigned_mp, assigned_obs
        return np.ascontiguousarray(assigned_mp, np.int32).copy(), np.ascontiguousarray(assigned_obs, np.int32).copy()

    def SearchByProjectionFrame(self, CurrentFrame, Tcw_cur, lv, th, bMono, assigned_mp, assigned_obs, inplace=False):
        """(Frame &CurrentFrame, const Frame &LastFrame, th, bMono): S/ORBmatcher.cc:1970-2186."""
        amp, aob = self._state(assigned_mp, assigned_obs, inplace)
        T = np.ascontiguousarray(Tcw_cur, np.float32).reshape(16)
        n = C.c_int(0)
        capi.check(self.lib.orbm_search_by_projection_frame(CurrentFrame.h, _vp(T), C.byref(lv), C.c_float(th), int(bMono),
                                                            int(self.mbCheckOrientation), _vp(amp), _vp(aob), C.byref(n)),
                   "orbm_search_by_projection_frame")
        return amp, aob, n.value

    def SearchByProjectionFrameResident(self, CurrentFrame, Tcw_cur, last_on_device, th, bMono, assigned_mp, assigned_obs):
        """SearchByProjection(Current, Last) on a LastFrameOnDevice (orbm_search_by_projection_frame_resident)."""
        amp, aob = self._state(assigned_mp, assigned_obs, False)
        T = np.ascontiguousarray(Tcw_cur, np.float32).reshape(16)
        n = C.c_int(0)
        capi.check(self.lib.orbm_search_by_projection_frame_resident(CurrentFrame.h, _vp(T), last_on_device.h, C.c_float(th), int(bool(bMono)),
                                                                     int(self.mbCheckOrientation), _vp(amp), _vp(aob), C.byref(n)),
                   "orbm_search_by_projection_frame_resident")
        return amp, aob, n.value

    def SearchByBoW(self, F, fvF, kf_desc, kf_mp_valid, kf_angle, fvK):
        """(KeyFrame*, Frame&, vector<MapPoint*>&): S/ORBmatcher.cc:269-471."""
        kf_desc = np.ascontiguousarray(kf_desc, np.uint8)
        kf_mp_valid = np.ascontiguousarray(kf_mp_valid, np.uint8)
        kf_angle = np.ascontiguousarray(kf_angle, np.float32)
        matches = np.zeros(max(F.n, 1), np.int32)
        n = C.c_int(0)
        capi.check(self.lib.orbm_search_by_bow(F.h, C.byref(fvF), _vp(kf_desc), len(kf_desc), _vp(kf_mp_valid), _vp(kf_angle),
                                               C.byref(fvK), C.c_float(self.mfNNratio), int(self.mbCheckOrientation),
                                               _vp(matches), C.byref(n)), "orbm_search_by_bow")
        return matches[: F.n].copy(), n.value


    def SearchByBoWRig(self, F, n_left, fvF, kf_desc, kf_mp_valid, kf_angle, fvK):
        """SearchByBoW(KeyFrame*, Frame&, ...) on a two-camera Frame (S/ORBmatcher.cc:342-430); F holds all Nleft + Nright features."""
        kf_desc = np.ascontiguousarray(kf_desc, np.uint8)
        kf_mp_valid = np.ascontiguousarray(kf_mp_valid, np.uint8)
        kf_angle = np.ascontiguousarray(kf_angle, np.float32)
        matches = np.zeros(max(F.n, 1), np.int32)
        n = C.c_int(0)
        capi.check(self.lib.orbm_search_by_bow_rig(F.h, int(n_left), C.byref(fvF), _vp(kf_desc), len(kf_desc), _vp(kf_mp_valid), _vp(kf_angle),
                                                   C.byref(fvK), C.c_float(self.mfNNratio), int(self.mbCheckOrientation), _vp(matches), C.byref(n)),
                   "orbm_search_by_bow_rig")
        return matches[: F.n].copy(), n.value

    def SearchByProjectionSim3(self, pKF, Scw, points, vpMatched, th, ratioHamming=1.0, already_found=None, with_kfs=False, camera=None):
        """(KeyFrame*, Scw, vpPoints[, vpPointsKFs], vpMatched[, vpMatchedKF], th, ratioHamming): S/ORBmatcher.cc:473-587
        (with_kfs=False) and :589-700 (with_kfs=True).  points: LocalMap resident on the device."""
        matched = np.ascontiguousarray(vpMatched, np.int32).copy()
        S = np.ascontiguousarray(Scw, np.float32).reshape(16)
        af = None if already_found is None else np.ascontiguousarray(already_found, np.uint8)
        n = C.c_int(0)
        if camera is not None:                              # pKF->mpCamera is a camera model (an orbg_camera): a fisheye keyframe
            capi.check(self.lib.orbm_search_by_projection_sim3_cam(pKF.h, points.h, _vp(S), C.byref(camera), _vp(af), int(th), C.c_float(ratioHamming),
                                                                   _vp(matched), C.byref(n)), "orbm_search_by_projection_sim3_cam")
            return matched, n.value
        capi.check(self.lib.orbm_search_by_projection_sim3(pKF.h, points.h, _vp(S), _vp(af), int(th), C.c_float(ratioHamming),
                                                           0 if with_kfs else 1, _vp(matched), C.byref(n)),
                   "orbm_search_by_projection_sim3")
        return matched, n.value

    def SearchByProjectionReloc(self, CurrentFrame, Tcw, kf_points, kf_angle, assigned_mp, th, ORBdist, already_found=None, camera=None):
        """(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist): the relocalisation overload,
        S/ORBmatcher.cc:2188-2310.  kf_points: the keyframe's map point matches, feature by feature, as a LocalMap resident on the
        device (bad = no point / isBad()); kf_angle: pKF->mvKeysUn[i].angle; assigned_mp >= 0 where the frame already holds a point."""
        amp = np.ascontiguousarray(assigned_mp, np.int32).copy()
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        ang = np.ascontiguousarray(kf_angle, np.float32)
        af = None if already_found is None else np.ascontiguousarray(already_found, np.uint8)
        n = C.c_int(0)
        if camera is not None:                              # CurrentFrame.mpCamera is a camera model (an orbg_camera): a monocular fisheye frame
            capi.check(self.lib.orbm_search_by_projection_reloc_cam(CurrentFrame.h, kf_points.h, _vp(T), C.byref(camera), _vp(af), _vp(ang), C.c_float(th),
                                                                    int(ORBdist), int(self.mbCheckOrientation), _vp(amp), C.byref(n)),
                       "orbm_search_by_projection_reloc_cam")
            return amp, n.value
        capi.check(self.lib.orbm_search_by_projection_reloc(CurrentFrame.h, kf_points.h, _vp(T), _vp(af), _vp(ang), C.c_float(th), int(ORBdist),
                                                            int(self.mbCheckOrientation), _vp(amp), C.byref(n)),
                   "orbm_search_by_projection_reloc")
        return amp, n.value

    def SearchByBoWKF(self, pKF2, fv2, mp_valid2, desc1, mp_valid1, angle1, fv1):
        """(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12): S/ORBmatcher.cc:819-959; returns matches12 (indices into pKF2)."""
        desc1 = np.ascontiguousarray(desc1, np.uint8)
        mp_valid1 = np.ascontiguousarray(mp_valid1, np.uint8)
        mp_valid2 = np.ascontiguousarray(mp_valid2, np.uint8)
        angle1 = np.ascontiguousarray(angle1, np.float32)
        matches = np.zeros(max(len(desc1), 1), np.int32)
        n = C.c_int(0)
        capi.check(self.lib.orbm_search_by_bow_kf(pKF2.h, C.byref(fv2), _vp(mp_valid2), _vp(desc1), len(desc1), _vp(mp_valid1),
                                                  _vp(angle1), C.byref(fv1), C.c_float(self.mfNNratio),
                                                  int(self.mbCheckOrientation), _vp(matches), C.byref(n)),
                   "orbm_search_by_bow_kf")
        return matches[: len(desc1)].copy(), n.value


class ORBVocabulary:
    """DBoW2 ORBVocabulary (I/ORBVocabulary.h:30) on the device: transform() of descriptors into BowVector / FeatureVector."""

    def __init__(self, view, keep=None, device=0):
        self.lib = capi.load()
        self.h = C.c_void_p()
        self._keep = keep
        if view is not None:
            capi.check(self.lib.orbv_vocab_create(device, C.byref(view), C.byref(self.h)), "orbv_vocab_create")

    @classmethod
    def loadFromTextFile(cls, path, device=0, keep_trailing_node=False):
        """ORBVocabulary::loadFromTextFile (TemplatedVocabulary.h:1338-1427): the reference's ORBvoc.txt straight onto the device."""
        voc = cls(None, None, device)
        flags = capi.ORBV_TEXT_KEEP_TRAILING_NODE if keep_trailing_node else 0
        capi.check(voc.lib.orbv_vocab_from_text(int(device), str(path).encode(), flags, C.byref(voc.h)), "orbv_vocab_from_text")
        return voc

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbv_vocab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transform_features(self, desc=None, levelsup=4, frame=None):
        """Per feature (word_id, node_id, weight): transform(feature, id, w, &nid, levelsup)."""
        if frame is not None:
            n = frame.n
        else:
            desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
            n = len(desc)
        wid = np.zeros(max(n, 1), np.int32); nid = np.zeros(max(n, 1), np.int32); w = np.zeros(max(n, 1), np.float64)
        if frame is not None:
            capi.check(self.lib.orbv_transform_frame(self.h, frame.h, int(levelsup), _vp(wid), _vp(nid), _vp(w)), "orbv_transform_frame")
        else:
            capi.check(self.lib.orbv_transform(self.h, _vp(desc), n, int(levelsup), _vp(wid), _vp(nid), _vp(w)), "orbv_transform")
        return wid[:n], nid[:n], w[:n]

    def transform(self, desc=None, levelsup=4, frame=None):
        """transform(features, BowVector&, FeatureVector&, levelsup): ((words, values), (node_id, start, feat_idx))."""
        wid, nid, w = self.transform_features(desc, levelsup, frame)
        n = len(wid)
        bw = np.zeros(max(n, 1), np.int32); bv = np.zeros(max(n, 1), np.float64)
        fn = np.zeros(max(n, 1), np.uint32); fs = np.zeros(n + 1, np.uint32); ff = np.zeros(max(n, 1), np.uint32)
        nw, nn = C.c_int32(0), C.c_int32(0)
        capi.check(self.lib.orbv_bow_assemble(self.h, _vp(wid), _vp(nid), _vp(w), n, _vp(bw), _vp(bv), C.byref(nw), _vp(fn), _vp(fs),
                                              _vp(ff), C.byref(nn)), "orbv_bow_assemble")
        k = nn.value
        return (bw[: nw.value].copy(), bv[: nw.value].copy()), (fn[:k].copy(), fs[: k + 1].copy(), ff[: int(fs[k]) if k else 0].copy())


def load_text_vocabulary(path, keep_trailing_node=False):
    """The host-only half of the loader (no GPU): dict of the flattened tree's arrays + k, scoring, n_words."""
    lib = capi.load()
    h = C.c_void_p()
    capi.check(lib.orbv_text_load(str(path).encode(), capi.ORBV_TEXT_KEEP_TRAILING_NODE if keep_trailing_node else 0, C.byref(h)), "orbv_text_load")
    try:
        v = capi.VocabView(); k, sc, nw = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        capi.check(lib.orbv_text_view(h, C.byref(v), C.byref(k), C.byref(sc), C.byref(nw)), "orbv_text_view")
        return capi.vocab_view_arrays(v, k.value, sc.value, nw.value)
    finally:
        lib.orbv_text_free(h)


def BowScoreL1(q_word, q_value, cand_start, cand_word, cand_value, device=0):
    """L1Scoring::score of one query BowVector against m candidate BowVectors (CSR): DetectNBestCandidates' inner loop."""
    lib = capi.load()
    qw = np.ascontiguousarray(q_word, np.int32); qv = np.ascontiguousarray(q_value, np.float64)
    cs = np.ascontiguousarray(cand_start, np.int32); cw = np.ascontiguousarray(cand_word, np.int32); cv = np.ascontiguousarray(cand_value, np.float64)
    m = len(cs) - 1
    out = np.zeros(max(m, 1), np.float64)
    capi.check(lib.orbv_score_l1(int(device), _vp(qw), _vp(qv), len(qw), _vp(cs), _vp(cw), _vp(cv), m, _vp(out)), "orbv_score_l1")
    return out[:m]


def ComputeDistinctiveDescriptors(desc, start, device=0):
    """MapPoint::ComputeDistinctiveDescriptors (S/MapPoint.cc:448-522) for a batch of map points (CSR lists of descriptors)."""
    lib = capi.load()
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    start = np.ascontiguousarray(start, np.int32)
    m = len(start) - 1
    best = np.zeros(max(m, 1), np.int32)
    capi.check(lib.orbm_distinctive_descriptors(int(device), _vp(desc) if len(desc) else None, _vp(start), m, _vp(best)),
               "orbm_distinctive_descriptors")
    return best[:m]


class Optimizer:
    """ORB_SLAM3::Optimizer (I/Optimizer.h:30-113): LocalBundleAdjustment numerical core."""

    def __init__(self, device=0):
        self.lib = capi.load()
        self.h = C.c_void_p()
        capi.check(self.lib.lba_create(device, 0, 0, 0, C.byref(self.h)), "lba_create")
        self.device = device

    def close(self):
        if getattr(self, "_ba", None) is not None:
            self._ba.close()
            self._ba = None
        if getattr(self, "h", None):
            self.lib.lba_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def LocalBundleAdjustmentAsync(self, problem, out, pbStopFlag=None):
        """Submit the solve to the handle's own LocalMapping thread (lba_solve_async); collect with wait()."""
        # a refused submission (one solve in flight per handle -> ORBG_BAD_ARG) must not drop the references that keep the
        # in-flight problem / result arrays alive: they are replaced only once the library has accepted the new job
        sp = None if pbStopFlag is None else C.c_void_p(pbStopFlag.ctypes.data)
        if getattr(self, "_async_keep", None) is None:
            out.c.trace_len = 0
        fn = self.lib.lba_solve_async_b if self._is_bool_flag(pbStopFlag) else self.lib.lba_solve_async
        capi.check(fn(self.h, C.byref(problem), sp, C.byref(out.c)), "lba_solve_async")
        self._async_keep = (problem, out, pbStopFlag)

    @staticmethod
    def _is_bool_flag(flag):
        """np.bool_ / np.uint8 flag = the reference's `bool* pbStopFlag` (polled as one byte, lba_solve_hb); np.int32 = the
        C-ABI's int32 flag with its deterministic test forms."""
        if flag is None:
            return False
        if flag.dtype in (np.bool_, np.uint8):
            return True
        assert flag.dtype == np.int32, "pbStopFlag must be a bool / uint8 / int32 array of one element"
        return False

    def set_profiling(self, on=True, reset=True):
        """Bracket one LDL^T launch per solve with a HIP event pair on the handle's stream (bench.py roofline)."""
        capi.check(self.lib.lba_set_profiling(self.h, int(bool(on)), int(bool(reset))), "lba_set_profiling")

    def solver_stats(self):
        """(sum of bracket times in ms, brackets, unknowns of the system, solved on the FP64 matrix cores?)"""
        s, n, nu, mc = C.c_double(0.0), C.c_int64(0), C.c_int32(0), C.c_int32(0)
        capi.check(self.lib.lba_get_solver_stats(self.h, C.byref(s), C.byref(n), C.byref(nu), C.byref(mc)), "lba_get_solver_stats")
        return s.value, n.value, nu.value, bool(mc.value)

    def watchdog_count(self):
        """Launches of the eight-workgroup LDL^T that timed out waiting for a participant (each re-solved on the one-workgroup kernels)."""
        n = C.c_int64(0)
        capi.check(self.lib.lba_get_watchdog_count(self.h, C.byref(n)), "lba_get_watchdog_count")
        return n.value

    def event_overhead_ms(self, reps=100):
        ms = C.c_float(0.0)
        capi.check(self.lib.lba_event_overhead(self.h, int(reps), C.byref(ms)), "lba_event_overhead")
        return ms.value

    def wait(self):
        ms = C.c_double(0.0)
        capi.check(self.lib.lba_wait(self.h, C.byref(ms)), "lba_wait")
        self.last_solve_ms = ms.value
        keep, self._async_keep = getattr(self, "_async_keep", None), None
        return keep[1] if keep else None

    def PoseOptimization(self, problem):
        """int Optimizer::PoseOptimization(Frame*) (S/Optimizer.cc:964-1278); problem: views.pose_opt_problem(...)[0]."""
        out = views.PoseOptOutput(problem.n)
        capi.check(self.lib.pose_optimize(C.byref(problem), C.byref(out.c)), "pose_optimize")
        return out

    def PoseInertialOptimization(self, problem):
        """int Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame(Frame*, bool) (S/Optimizer.cc:7603-8424), as problem.form says;
        problem: views.pose_inertial_problem(...)[0].  Returns a views.PoseInertialOutput."""
        out = views.PoseInertialOutput(problem.n)
        capi.check(self.lib.pose_inertial_optimize(C.byref(problem), C.byref(out.c)), "pose_inertial_optimize")
        return out

    pose_inertial_optimize = PoseInertialOptimization

    def LocalInertialBA(self, problem, handle=None, trace_cap=16):
        """The numerical core of void Optimizer::LocalInertialBA(KeyFrame*, bool*, Map*, bool bLarge, bool bRecInit)
        (S/Optimizer.cc:4556-5226); problem: views.inertial_ba_problem(...)[0]; handle: an InertialBA (device buffers, solver and stream
        kept between calls) or None.  Returns a views.InertialBaOutput: states and points, the verdicts, `failed`."""
        out = views.InertialBaOutput(problem, trace_cap)
        if handle is None:
            capi.check(self.lib.inertial_ba_solve(C.byref(problem), C.byref(out.c)), "inertial_ba_solve")
        else:
            capi.check(self.lib.inertial_ba_solve_h(handle.h, C.byref(problem), C.byref(out.c)), "inertial_ba_solve_h")
        return out

    inertial_ba_solve = LocalInertialBA

    def InertialOptimization(self, problem, trace_cap=200):
        """optimizer.optimize(its) of the four void Optimizer::InertialOptimization(...) overloads (S/Optimizer.cc:5344-5958), as the
        problem's switches say; problem: views.inertial_init_problem(...)[0].  Returns a views.InertialInitOutput: the velocities, the
        biases, Rwg and scale, the iterations and the LM trace."""
        out = views.InertialInitOutput(problem, trace_cap)
        capi.check(self.lib.inertial_init_solve(C.byref(problem), C.byref(out.c)), "inertial_init_solve")
        return out

    inertial_init_solve = InertialOptimization

    def inertial_init_linearize(self, problem):
        """TEST AID (inertial_init_host_linearize): per edge the 9 x 16 block [v1 | v2 | bg | ba | gdir | s | e]; needs no device."""
        J = np.zeros((max(problem.n_edges, 1), 9, 16))
        capi.check(self.lib.inertial_init_host_linearize(C.byref(problem), capi.ptr(J)), "inertial_init_host_linearize")
        return J[: problem.n_edges]

    def imu_information(self, C15):
        """info9, infoG, infoA of an IMU::Preintegrated's covariance C (15 x 15 float), as the edges hold them (orbg_imu_information)."""
        Cf = np.ascontiguousarray(np.asarray(C15, np.float32).reshape(225))
        i9, ig, ia = np.zeros(81), np.zeros(9), np.zeros(9)
        capi.check(self.lib.orbg_imu_information(Cf.ctypes.data, i9.ctypes.data, ig.ctypes.data, ia.ctypes.data), "orbg_imu_information")
        return i9.reshape(9, 9), ig.reshape(3, 3), ia.reshape(3, 3)

    def condition_prior(self, H):
        """the ConstraintPoseImu constructor's conditioning of a 15 x 15 H (orbg_condition_prior); returns a new array."""
        Hc = np.ascontiguousarray(np.asarray(H, np.float64).reshape(225)).copy()
        capi.check(self.lib.orbg_condition_prior(Hc.ctypes.data), "orbg_condition_prior")
        return Hc.reshape(15, 15)

    def LocalBundleAdjustment(self, problem, pbStopFlag=None, trace_cap=64, out=None):
        """problem: views.lba_problem(...)[0]; pbStopFlag: np.bool_[1] (the reference's bool) or np.int32[1], polled between LM
        iterations / trials.
        out: a views.LbaOutput of matching size to reuse (the result arrays are the caller's, as in the C ABI)."""
        if out is None:
            out = views.LbaOutput(problem.n_poses, problem.n_points, problem.n_edges, trace_cap)
        else:
            out.c.trace_len = 0
        sp = None if pbStopFlag is None else C.c_void_p(pbStopFlag.ctypes.data)
        fn = self.lib.lba_solve_hb if self._is_bool_flag(pbStopFlag) else self.lib.lba_solve_h
        capi.check(fn(self.h, C.byref(problem), sp, C.byref(out.c)), "lba_solve_h")
        return out

    def BundleAdjustment(self, p, nIterations=None, pbStopFlag=None, bRobust=None, out=None):
        """void Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, ..., bRobust) (S/Optimizer.cc:73-446), numerical
        core.  p: views.ba_problem(...)[0]; nIterations / bRobust override the problem's fields when given (None: the problem's
        own iterations / robust, which views.ba_problem sets to 10 / True by default, stay); pbStopFlag as in
        LocalBundleAdjustment (np.bool_[1] = &mbStopGBA).  The workspace is created on first use and kept."""
        if getattr(self, "_ba", None) is None:
            self._ba = FullBA(self.device)
        if nIterations is not None:
            p.iterations = int(nIterations)
        if bRobust is not None:
            p.robust = int(bool(bRobust))
        return self._ba.solve(p, pbStopFlag, out=out)

    def MergeLocalBundleAdjustment(self, problem, pbStopFlag=None, trace_cap=64, out=None):
        """void Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) (S/Optimizer.cc:6305-6983, the welding BA
        of LoopClosing::MergeLocal), numerical core: a robust round, the outlier level, a second round over the level-0 edges without
        kernels -- all on the device (ba_weld_solve_h).  problem: views.ba_weld_problem(...)[0]; pbStopFlag as in BundleAdjustment.
        Returns a views.BaWeldOutput: the BundleAdjustment result's fields plus edge_level, rounds_run, both traces and to_erase."""
        if getattr(self, "_ba", None) is None:
            self._ba = FullBA(self.device)
        return self._ba.weld(problem, pbStopFlag, trace_cap=trace_cap, out=out)


class FullBA:
    """Persistent workspace of Optimizer::BundleAdjustment (include/orbgpu.h: ba_create ... ba_solve_hb)."""

    def __init__(self, device=0, cap_poses=0, cap_points=0, cap_edges=0):
        self.lib = capi.load()
        self.h = C.c_void_p()
        capi.check(self.lib.ba_create(device, int(cap_poses), int(cap_points), int(cap_edges), C.byref(self.h)), "ba_create")

    def close(self):
        if getattr(self, "h", None):
            self.lib.ba_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, problem, pbStopFlag=None, trace_cap=64, out=None):
        if out is None:
            out = views.BaOutput(problem.n_poses, problem.n_points, problem.n_edges, trace_cap)
        else:
            out.c.trace_len = 0
        sp = None if pbStopFlag is None else C.c_void_p(pbStopFlag.ctypes.data)
        fn = self.lib.ba_solve_hb if Optimizer._is_bool_flag(pbStopFlag) else self.lib.ba_solve_h
        capi.check(fn(self.h, C.byref(problem), sp, C.byref(out.c)), "ba_solve_h")
        return out

    def weld(self, problem, pbStopFlag=None, trace_cap=64, out=None):
        """ba_weld_solve_h / ba_weld_solve_hb on this workspace; problem: views.ba_weld_problem(...)[0]."""
        b = problem.ba
        if out is None:
            out = views.BaWeldOutput(b.n_poses, b.n_points, b.n_edges, trace_cap, problem.chi2_mono, problem.chi2_stereo)
        else:
            out.c.trace_len = 0
            out.w.trace_second_len = 0
            out.chi2_mono, out.chi2_stereo = problem.chi2_mono, problem.chi2_stereo
        sp = None if pbStopFlag is None else C.c_void_p(pbStopFlag.ctypes.data)
        fn = self.lib.ba_weld_solve_hb if Optimizer._is_bool_flag(pbStopFlag) else self.lib.ba_weld_solve_h
        capi.check(fn(self.h, C.byref(problem), sp, C.byref(out.w)), "ba_weld_solve_h")
        # (mono / stereo of every edge, for to_erase's order)
        out._ur = (np.frombuffer(C.string_at(b.edges, b.n_edges * capi.EDGE_DTYPE.itemsize), capi.EDGE_DTYPE)["ur"].copy()
                   if b.n_edges > 0 else np.zeros(0, np.float32))
        return out

    def set_profiling(self, on=True):
        capi.check(self.lib.ba_set_profiling(self.h, int(bool(on))), "ba_set_profiling")

    def phase_ms(self):
        """Device time of the last solve: (structure build, linearisation, Schur complement, LDL^T, update + evaluation) in ms."""
        ms = (C.c_double * 5)()
        capi.check(self.lib.ba_get_phase_ms(self.h, ms), "ba_get_phase_ms")
        return tuple(ms)


class EssentialGraphResult:
    """What eg_solve returns: estimates (V, 8) float64 = q (x y z w), t, s per vertex; points (P, 3) float32; err0 / errEnd; iters;
    trace (iters, 4) = {trials, last trial accepted, chi2, lambda} per LM iteration; edge_error0 (E, 7)."""

    def __init__(self, estimates, points, err0, errEnd, iters, trace, edge_error0):
        self.estimates, self.points, self.err0, self.errEnd, self.iters, self.trace, self.edge_error0 = (
            estimates, points, err0, errEnd, iters, trace, edge_error0)


def OptimizeEssentialGraph(vertices, edges, points=None, iterations=20, lambda_init=1e-16, device=0, raw=False):
    """The numerical core of Optimizer::OptimizeEssentialGraph (S/Optimizer.cc:2413-2747; include/orbgpu.h: eg_solve).  vertices /
    edges / points: arrays of capi.EG_VERTEX_DTYPE / EG_EDGE_DTYPE / EG_POINT_DTYPE.  At least one vertex of
    every connected component must be fixed: that is the caller's job, as in the reference.  raw=True returns the status code with the
    result instead of raising."""
    lib = capi.load()
    V = np.ascontiguousarray(vertices, capi.EG_VERTEX_DTYPE)
    E = np.ascontiguousarray(edges, capi.EG_EDGE_DTYPE)
    P = np.zeros(0, capi.EG_POINT_DTYPE) if points is None else np.ascontiguousarray(points, capi.EG_POINT_DTYPE)
    est = np.zeros((len(V), 8), np.float64)
    pts = np.zeros((len(P), 3), np.float32)
    trace = np.zeros((max(int(iterations), 1), 4), np.float64)
    err = np.zeros((len(E), 7), np.float64)
    p = capi.EgProblem(C.sizeof(capi.EgProblem), len(V), _vp(V) if len(V) else None, len(E), _vp(E) if len(E) else None, int(iterations),
                       float(lambda_init), len(P), _vp(P) if len(P) else None, int(device))
    r = capi.EgResult(C.sizeof(capi.EgResult), _vp(est) if len(V) else None, _vp(pts) if len(P) else None, 0.0, 0.0, 0, _vp(trace), len(trace), 0,
                      _vp(err) if len(E) else None)
    rc = lib.eg_solve(C.byref(p), C.byref(r))
    out = EssentialGraphResult(est, pts, r.err0, r.errEnd, r.iters, trace[: r.trace_len].copy(), err)
    if raw:
        return rc, out
    capi.check(rc, "eg_solve")
    return out


class KeyFrameDatabase:
    """Device-resident place-recognition database (inverted file, BowVectors, covisibility lists): the compute side of
    KeyFrameDatabase::DetectNBestCandidates (S/KeyFrameDatabase.cc:594-761).  view: views.database_view(...)."""

    def __init__(self, view, keep=None, device=0):
        self.lib = capi.load()
        self.h = C.c_void_p()
        self._keep = keep
        self.n_kfs = view.n_kfs
        capi.check(self.lib.orbd_database_create(device, C.byref(view), C.byref(self.h)), "orbd_database_create")

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbd_database_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def DetectNBestCandidates(self, q_word, q_value, connected, query_map_id, nNumCandidates, place_score):
        """-> (vpLoopCand, vpMergeCand) as keyframe indices; place_score (float32[n_kfs]) is updated in place."""
        qw = np.ascontiguousarray(q_word, np.int32); qv = np.ascontiguousarray(q_value, np.float64)
        con = np.ascontiguousarray(connected, np.uint8)
        assert place_score.dtype == np.float32 and place_score.flags["C_CONTIGUOUS"] and len(place_score) == self.n_kfs
        loop = np.zeros(max(nNumCandidates, 1), np.int32); merge = np.zeros(max(nNumCandidates, 1), np.int32)
        nl, nm = C.c_int32(0), C.c_int32(0)
        capi.check(self.lib.orbd_detect_n_best_candidates(self.h, _vp(qw), _vp(qv), len(qw), _vp(con), int(query_map_id), int(nNumCandidates),
                                                          _vp(place_score), _vp(loop), C.byref(nl), _vp(merge), C.byref(nm)),
                   "orbd_detect_n_best_candidates")
        return loop[: nl.value].copy(), merge[: nm.value].copy()

    def DetectRelocalizationCandidates(self, q_word, q_value, query_map_id, reloc_score):
        """KeyFrameDatabase::DetectRelocalizationCandidates (S/KeyFrameDatabase.cc:764-876) for the query BowVector -> vpRelocCandidates
        as keyframe indices; reloc_score (float32[n_kfs], mRelocScore) is updated in place."""
        qw = np.ascontiguousarray(q_word, np.int32); qv = np.ascontiguousarray(q_value, np.float64)
        assert reloc_score.dtype == np.float32 and reloc_score.flags["C_CONTIGUOUS"] and len(reloc_score) == self.n_kfs
        cand = np.zeros(max(self.n_kfs, 1), np.int32)
        n = C.c_int32(0)
        capi.check(self.lib.orbd_detect_relocalization_candidates(self.h, _vp(qw), _vp(qv), len(qw), int(query_map_id), _vp(reloc_score),
                                                                  _vp(cand), C.byref(n)), "orbd_detect_relocalization_candidates")
        return cand[: n.value].copy()


# ---------------------------------------------------------------- Sim3Solver (S/Sim3Solver.cc)

def sim3_ransac_iterations(n, probability=0.99, minInliers=6, maxIterations=300):
    """mRansacMaxIts of Sim3Solver::SetRansacParameters (S/Sim3Solver.cc:132-157) for N = n.  Host code, needs no device."""
    out = C.c_int(0)
    capi.check(capi.load().orbm_sim3_ransac_iterations(int(n), float(probability), int(minInliers), int(maxIterations), C.byref(out)),
               "orbm_sim3_ransac_iterations")
    return out.value


def sim3_draws(n, n_iterations, rng):
    """The raw DUtils::Random::RandomInt(0, size - 1) results of n_iterations iterations (S/Sim3Solver.cc:193): int32 (n_iterations, 3),
    column j uniform in [0, n - j).  rng: a numpy Generator or a seed.  Tests, the checker and the solver below all draw through this."""
    if not isinstance(rng, np.random.Generator):
        rng = np.random.default_rng(rng)
    d = np.empty((int(n_iterations), 3), np.int32)
    for j in range(3):
        d[:, j] = rng.integers(0, max(int(n) - j, 1), size=int(n_iterations))
    return d


def sim3_resolve_draws(n, draws):
    """Raw draws -> the three correspondence indices of each minimal set (swap-with-back removal on mvAllIndices, :191-206)."""
    d = np.ascontiguousarray(draws, np.int32).reshape(-1, 3)
    idx = np.zeros_like(d)
    capi.check(capi.load().orbm_sim3_resolve_draws(int(n), _vp(d), len(d), _vp(idx)), "orbm_sim3_resolve_draws")
    return idx


class Sim3Problem:
    """The flat problem Sim3Solver's constructor builds (S/Sim3Solver.cc:38-128): camera-frame points of the kept pairs, the truncated
    thresholds 9.210 * sigma2 (uint32: the reference stores them in vector<size_t>), pinhole intrinsics (fx, fy, cx, cy) of the two
    keyframes' cameras, mbFixScale, and mvnIndices1 / mN1 to map the kept pairs back to vpMatched12."""

    def __init__(self, X3Dc1, X3Dc2, max_err1, max_err2, K1, K2, bFixScale, indices1=None, mN1=None):
        self.X1 = np.ascontiguousarray(X3Dc1, np.float32).reshape(-1, 3)
        self.X2 = np.ascontiguousarray(X3Dc2, np.float32).reshape(-1, 3)
        self.e1 = np.ascontiguousarray(max_err1, np.uint32).reshape(-1)
        self.e2 = np.ascontiguousarray(max_err2, np.uint32).reshape(-1)
        self.n = len(self.X1)
        assert len(self.X2) == self.n and len(self.e1) == self.n and len(self.e2) == self.n
        self.K1 = tuple(float(v) for v in K1)
        self.K2 = tuple(float(v) for v in K2)
        self.fix_scale = bool(bFixScale)
        self.indices1 = np.arange(self.n, dtype=np.int64) if indices1 is None else np.asarray(indices1, np.int64)
        self.mN1 = int(mN1) if mN1 is not None else (int(self.indices1.max()) + 1 if self.n else 0)

    def struct(self, camera_models=(0, 0)):
        return capi.Sim3Problem(C.sizeof(capi.Sim3Problem), self.n, capi.ptr(self.X1), capi.ptr(self.X2), capi.ptr(self.e1), capi.ptr(self.e2),
                                *self.K1, *self.K2, int(camera_models[0]), int(camera_models[1]), int(self.fix_scale))


class Sim3Iteration:
    """What one iterate() / find() call returned.  T12 is the five-argument overload's return value (the converged hypothesis, else the
    best found during THIS call, else None); T12_four the four-argument one's (None unless converged).  vbInliers has length mN1 and
    nInliers / vbInliers are zero unless converged, as in the reference.  best_* is the solver's state after the call."""

    def __init__(self, prob, r, mask, hyp):
        self.bNoMore, self.bConverge = bool(r.no_more), bool(r.converged)
        self.iterations_done, self.iterations_run, self.best_iteration = r.iterations_done, r.iterations_run, r.best_iteration
        self.improved = bool(r.improved_in_this_call)
        self.have_best = bool(r.have_best)
        self.best_T12 = np.array(r.T12, np.float32).reshape(4, 4) if self.have_best else None
        self.best_R = np.array(r.R, np.float32).reshape(3, 3) if self.have_best else None
        self.best_t = np.array(r.t, np.float32) if self.have_best else None
        self.best_s = np.float32(r.s) if self.have_best else None
        self.best_inliers = r.n_inliers
        self.best_mask = mask.astype(bool)
        self.nInliers = r.n_inliers if self.bConverge else 0
        self.vbInliers = np.zeros(prob.mN1, bool)
        if self.bConverge:
            self.vbInliers[prob.indices1[self.best_mask]] = True
        self.T12_four = self.best_T12 if self.bConverge else None
        self.T12 = self.best_T12 if (self.bConverge or self.improved) else None
        self.hyp_n_inliers, self.hyp_T12, self.hyp_masks = hyp


def _sim3_result(prob, n_hyp, per_hypothesis):
    mask = np.zeros(max(prob.n, 1), np.uint8)
    hyp = (None, None, None)
    if per_hypothesis:
        hyp = (np.zeros(max(n_hyp, 1), np.int32), np.zeros((max(n_hyp, 1), 16), np.float32),
               np.zeros((max(n_hyp, 1), max((prob.n + 63) // 64, 1)), np.uint64))
    r = capi.Sim3Result()
    r.struct_size = C.sizeof(capi.Sim3Result)
    r.inliers = capi.ptr(mask)
    r.hyp_n_inliers, r.hyp_T12, r.hyp_masks = (capi.ptr(a) for a in hyp)
    return r, mask, hyp


def _sim3_unpack(prob, r, mask, hyp, n_hyp):
    if hyp[0] is not None:
        bits = np.unpackbits(hyp[2][:n_hyp].view(np.uint8), axis=1, bitorder="little")[:, : prob.n].astype(bool)
        hyp = (hyp[0][:n_hyp], hyp[1][:n_hyp].reshape(-1, 4, 4), bits)
    return Sim3Iteration(prob, r, mask[: prob.n], hyp)


class Sim3Solver:
    """ORB_SLAM3::Sim3Solver (I/Sim3Solver.h:36-131) over a flat Sim3Problem: every hypothesis of a call in one kernel launch, the
    serial choice among them replayed on the device.  Draws come from the caller (`draws`, raw RandomInt results as sim3_draws makes
    them) or from the solver's own seeded generator."""

    def __init__(self, problem, device=0, seed=0):
        self.lib = capi.load()
        self.h = C.c_void_p()
        self.prob = problem
        self.rng = np.random.default_rng(seed)
        self.device = device
        capi.check(self.lib.orbm_sim3_create(device, C.byref(self.h)), "orbm_sim3_create")
        st = problem.struct()
        capi.check(self.lib.orbm_sim3_set_problem(self.h, C.byref(st)), "orbm_sim3_set_problem")
        self.mRansacMinInliers = 6
        self.mRansacMaxIts = sim3_ransac_iterations(problem.n, 0.99, 6, 300) if problem.n > 0 else 1
        self._last = None
        self._done = 0                       # mnIterations

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbm_sim3_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        capi.check(self.lib.orbm_sim3_set_stream(self.h, C.c_void_p(hip_stream) if hip_stream else None), "orbm_sim3_set_stream")

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        capi.check(self.lib.orbm_sim3_set_ransac_parameters(self.h, float(probability), int(minInliers), int(maxIterations)),
                   "orbm_sim3_set_ransac_parameters")
        self.mRansacMinInliers = int(minInliers)
        self._done = 0
        self.mRansacMaxIts = sim3_ransac_iterations(self.prob.n, probability, minInliers, maxIterations) if self.prob.n > 0 else max(1, int(maxIterations))

    def iterate(self, nIterations, draws=None, per_hypothesis=False):
        """-> Sim3Iteration.  draws: int32 (nIterations, 3) raw draws; None: taken from the solver's generator (all nIterations of them
        before the launch, so after an early convergence the generator is further on than a serial loop's would be)."""
        nIterations = int(nIterations)
        if draws is None:
            draws = sim3_draws(self.prob.n, nIterations, self.rng) if self.prob.n >= 3 else np.zeros((nIterations, 3), np.int32)
        d = np.ascontiguousarray(draws, np.int32).reshape(-1, 3)
        assert len(d) >= min(nIterations, max(0, self.mRansacMaxIts - self._done)), "three raw draws per iteration that can still run"
        r, mask, hyp = _sim3_result(self.prob, nIterations, per_hypothesis)
        capi.check(self.lib.orbm_sim3_iterate(self.h, nIterations, _vp(d), C.byref(r)), "orbm_sim3_iterate")
        n_hyp = min(nIterations, max(0, self.mRansacMaxIts - (r.iterations_done - r.iterations_run))) if self.prob.n >= self.mRansacMinInliers else 0
        self._done = r.iterations_done
        self._last = _sim3_unpack(self.prob, r, mask, hyp, n_hyp)
        return self._last

    def find(self, draws=None, per_hypothesis=False):
        """cv::Mat Sim3Solver::find(vbInliers12, nInliers), S/Sim3Solver.cc:294-298 -> Sim3Iteration (T12_four is find's return value)."""
        return self.iterate(self.mRansacMaxIts, draws, per_hypothesis)

    def GetEstimatedRotation(self):
        return None if self._last is None or not self._last.have_best else self._last.best_R.copy()

    def GetEstimatedTranslation(self):
        return None if self._last is None or not self._last.have_best else self._last.best_t.copy()

    def GetEstimatedScale(self):
        return None if self._last is None or not self._last.have_best else float(self._last.best_s)

    @staticmethod
    def solve_batch(problems, params=None, draws=None, device=0, seed=0, per_hypothesis=False):
        """find() of len(problems) fresh solvers in ONE launch.  params: (probability, minInliers, maxIterations) per problem (None: the
        defaults); draws: per problem the raw draws of mRansacMaxIts iterations (None: from a generator seeded with `seed`).
        -> list of Sim3Iteration."""
        lib = capi.load()
        B = len(problems)
        params = [(0.99, 6, 300)] * B if params is None else [tuple(p) for p in params]
        rng = np.random.default_rng(seed)
        its = [sim3_ransac_iterations(p.n, *q) if p.n > 0 else 1 for p, q in zip(problems, params)]
        if draws is None:
            draws = [sim3_draws(p.n, h, rng) if p.n >= 3 else np.zeros((h, 3), np.int32) for p, h in zip(problems, its)]
        ds = [np.ascontiguousarray(d, np.int32).reshape(-1, 3) for d in draws]
        for d, h, p, q in zip(ds, its, problems, params):
            assert p.n < q[1] or len(d) >= h, "three raw draws per iteration of mRansacMaxIts"
        P = (capi.Sim3Problem * max(B, 1))(*[p.struct() for p in problems])
        Q = (capi.Sim3Params * max(B, 1))(*[capi.Sim3Params(float(q[0]), int(q[1]), int(q[2])) for q in params])
        D = (C.c_void_p * max(B, 1))(*[d.ctypes.data for d in ds])
        outs = [_sim3_result(p, h, per_hypothesis) for p, h in zip(problems, its)]
        R = (capi.Sim3Result * max(B, 1))(*[o[0] for o in outs])
        capi.check(lib.orbm_sim3_solve_batch(int(device), P, B, Q, D, R), "orbm_sim3_solve_batch")
        return [_sim3_unpack(p, R[b], outs[b][1], outs[b][2], its[b] if p.n >= params[b][1] else 0) for b, p in enumerate(problems)]


# ---------------------------------------------------------------- MLPnPsolver (S/MLPnPsolver.cpp)

MLPNP_DEFAULTS = (0.99, 8, 300, 6, 0.4, 5.991)        # I/MLPnPsolver.h; Tracking::Relocalization sets (0.99, 10, 300, 6, 0.5, 5.991)


def mlpnp_ransac_iterations(n, probability=0.99, minInliers=8, maxIterations=300, minSet=6, epsilon=0.4, th2=5.991):
    """(mRansacMaxIts, mRansacMinInliers) of MLPnPsolver::SetRansacParameters (S/MLPnPsolver.cpp:218-248) for N = n.  Host code."""
    its, mi = C.c_int(0), C.c_int(0)
    capi.check(capi.load().orbp_mlpnp_ransac_iterations(int(n), float(probability), int(minInliers), int(maxIterations), int(minSet),
                                                        float(epsilon), C.byref(its), C.byref(mi)), "orbp_mlpnp_ransac_iterations")
    return its.value, mi.value


def mlpnp_draws(n, k, seed):
    """The raw DUtils::Random::RandomInt(0, size - 1) results of k iterations (S/MLPnPsolver.cpp:128): int32 (k, 6), column j uniform
    in [0, n - j).  seed: a numpy Generator or a seed."""
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    d = np.empty((int(k), 6), np.int32)
    for j in range(6):
        d[:, j] = rng.integers(0, max(int(n) - j, 1), size=int(k))
    return d


def mlpnp_resolve_draws(n, draws):
    """Raw draws -> the six correspondence indices of each minimal set (swap-with-back removal on mvAllIndices, :126-138)."""
    d = np.ascontiguousarray(draws, np.int32).reshape(-1, 6)
    idx = np.zeros_like(d)
    capi.check(capi.load().orbp_mlpnp_resolve_draws(int(n), _vp(d), len(d), _vp(idx)), "orbp_mlpnp_resolve_draws")
    return idx


def mlpnp_gn(P3Dw, bearing, R, t, device=0):
    """rot2rodrigues, mlpnp_gn, rodrigues2rot (S/MLPnPsolver.cpp:635-647) for six points on the device -> (R, t) in double."""
    X = np.ascontiguousarray(P3Dw, np.float32).reshape(6, 3)
    f = np.ascontiguousarray(bearing, np.float32).reshape(6, 3)
    R = np.ascontiguousarray(R, np.float64).reshape(3, 3)
    t = np.ascontiguousarray(t, np.float64).reshape(3)
    Ro, to = np.zeros((3, 3)), np.zeros(3)
    capi.check(capi.load().orbp_mlpnp_gn(int(device), _vp(X), _vp(f), _vp(R), _vp(t), _vp(Ro), _vp(to)), "orbp_mlpnp_gn")
    return Ro, to


class MLPnPProblem:
    """The flat problem MLPnPsolver's constructor builds (S/MLPnPsolver.cpp:54-96): per surviving match the undistorted keypoint, the
    level's sigma2, the bearing (unproject divided by z, not normalised), the map point, and its index among the m matches; `camera`
    is (fx, fy, cx, cy) of a pinhole mpCamera."""

    def __init__(self, P2D, sigma2, bearing, P3Dw, camera, kp_index=None, m=None):
        self.P2D = np.ascontiguousarray(P2D, np.float32).reshape(-1, 2)
        self.sigma2 = np.ascontiguousarray(sigma2, np.float32).reshape(-1)
        self.bearing = np.ascontiguousarray(bearing, np.float32).reshape(-1, 3)
        self.P3Dw = np.ascontiguousarray(P3Dw, np.float32).reshape(-1, 3)
        self.n = len(self.P2D)
        assert len(self.sigma2) == self.n and len(self.bearing) == self.n and len(self.P3Dw) == self.n
        self.camera = tuple(float(v) for v in camera)
        self.kp_index = np.arange(self.n, dtype=np.int32) if kp_index is None else np.ascontiguousarray(kp_index, np.int32).reshape(-1)
        self.m = int(m) if m is not None else (int(self.kp_index.max()) + 1 if self.n else 0)

    def struct(self, camera_model=0):
        cam = capi.Camera(int(camera_model), *self.camera)
        return capi.MLPnPProblem(C.sizeof(capi.MLPnPProblem), self.n, capi.ptr(self.P2D), capi.ptr(self.sigma2), capi.ptr(self.bearing),
                                 capi.ptr(self.P3Dw), capi.ptr(self.kp_index), self.m, cam)


class MLPnPIteration:
    """What one iterate() call returned.  Tcw is the reference's return value (None for an empty matrix); nInliers / vbInliers (length
    m) are zero unless a matrix came back.  best_* is the solver's persisting state.  hyp_*: per hypothesis of the launch."""

    def __init__(self, prob, r, mask, hyp):
        self.bNoMore, self.returned = bool(r.no_more), bool(r.returned)
        self.nInliers = r.n_inliers
        self.iterations_done, self.iterations_run, self.best_iteration = r.iterations_done, r.iterations_run, r.best_iteration
        self.have_best, self.best_inliers = bool(r.have_best), r.best_inliers
        self.Tcw = np.array(r.Tcw, np.float32).reshape(4, 4) if self.returned else None
        self.best_Tcw = np.array(r.best_Tcw, np.float32).reshape(4, 4) if self.have_best else None
        self.vbInliers = mask.astype(bool)
        self.hyp_n_inliers, self.hyp_planar, self.hyp_R, self.hyp_t, self.hyp_masks = hyp

    def fields(self):
        """Every field as plain values, for comparisons."""
        return (self.bNoMore, self.returned, self.nInliers, self.iterations_done, self.iterations_run, self.best_iteration, self.have_best,
                self.best_inliers, None if self.Tcw is None else self.Tcw.tobytes(),
                None if self.best_Tcw is None else self.best_Tcw.tobytes(), self.vbInliers.tobytes())


def _mlpnp_result(prob, n_hyp, per_hypothesis):
    mask = np.zeros(max(prob.m, 1), np.uint8)
    hyp = (None,) * 5
    if per_hypothesis:
        k = max(n_hyp, 1)
        hyp = (np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros((k, 3, 3)), np.zeros((k, 3)),
               np.zeros((k, max((prob.n + 63) // 64, 1)), np.uint64))
    r = capi.MLPnPResult()
    r.struct_size = C.sizeof(capi.MLPnPResult)
    r.inliers = capi.ptr(mask)
    r.hyp_n_inliers, r.hyp_planar, r.hyp_R, r.hyp_t, r.hyp_masks = (capi.ptr(a) for a in hyp)
    return r, mask, hyp


def _mlpnp_unpack(prob, r, mask, hyp, n_hyp):
    if hyp[0] is not None:
        bits = np.unpackbits(hyp[4][:n_hyp].view(np.uint8), axis=1, bitorder="little")[:, : prob.n].astype(bool)
        hyp = (hyp[0][:n_hyp], hyp[1][:n_hyp].astype(bool), hyp[2][:n_hyp], hyp[3][:n_hyp], bits)
    return MLPnPIteration(prob, r, mask[: prob.m], hyp)


class MLPnPsolver:
    """ORB_SLAM3::MLPnPsolver over a flat MLPnPProblem: every hypothesis of a call in one kernel launch, the serial loop replayed over
    the counts.  Draws come from the caller (raw RandomInt results as mlpnp_draws makes them) or from the solver's seeded generator."""

    def __init__(self, problem, device=0, seed=0):
        self.lib = capi.load()
        self.h = C.c_void_p()
        self.prob = problem
        self.rng = np.random.default_rng(seed)
        self.device = device
        capi.check(self.lib.orbp_mlpnp_create(device, C.byref(self.h)), "orbp_mlpnp_create")
        st = problem.struct()
        capi.check(self.lib.orbp_mlpnp_set_problem(self.h, C.byref(st)), "orbp_mlpnp_set_problem")
        self.mRansacMaxIts, self.mRansacMinInliers = mlpnp_ransac_iterations(problem.n, *MLPNP_DEFAULTS)

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbp_mlpnp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        capi.check(self.lib.orbp_mlpnp_set_stream(self.h, C.c_void_p(hip_stream) if hip_stream else None), "orbp_mlpnp_set_stream")

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=6, epsilon=0.4, th2=5.991):
        capi.check(self.lib.orbp_mlpnp_set_ransac_parameters(self.h, float(probability), int(minInliers), int(maxIterations), int(minSet),
                                                             float(epsilon), float(th2)), "orbp_mlpnp_set_ransac_parameters")
        self.mRansacMaxIts, self.mRansacMinInliers = mlpnp_ransac_iterations(self.prob.n, probability, minInliers, maxIterations, minSet, epsilon)

    def iterations_of_call(self, nIterations):
        k = C.c_int(0)
        capi.check(self.lib.orbp_mlpnp_iterations_of_call(self.h, int(nIterations), C.byref(k)), "orbp_mlpnp_iterations_of_call")
        return k.value

    def iterate(self, nIterations, draws=None, per_hypothesis=False):
        """-> MLPnPIteration.  draws: int32 (iterations_of_call(nIterations), 6) raw draws; None: from the solver's generator (all of
        them before the launch, so after an early return the generator is further on than a serial loop's would be)."""
        k = self.iterations_of_call(nIterations)
        if draws is None:
            draws = mlpnp_draws(self.prob.n, k, self.rng)
        d = np.ascontiguousarray(draws, np.int32).reshape(-1, 6)
        assert len(d) >= k, "six raw draws per iteration that can run"
        r, mask, hyp = _mlpnp_result(self.prob, k, per_hypothesis)
        capi.check(self.lib.orbp_mlpnp_iterate(self.h, int(nIterations), _vp(d), C.byref(r)), "orbp_mlpnp_iterate")
        return _mlpnp_unpack(self.prob, r, mask, hyp, k)

    @staticmethod
    def solve_batch(problems, params=None, draws=None, device=0, seed=0, per_hypothesis=False):
        """The first iterate() of len(problems) fresh solvers in ONE launch.  params: SetRansacParameters' six arguments per problem
        (None: the defaults); draws: per problem the raw draws of mRansacMaxIts iterations (None: from a generator seeded with
        `seed`).  -> list of MLPnPIteration."""
        lib = capi.load()
        B = len(problems)
        params = [MLPNP_DEFAULTS] * B if params is None else [tuple(p) for p in params]
        rng = np.random.default_rng(seed)
        its = [mlpnp_ransac_iterations(p.n, *q[:5]) for p, q in zip(problems, params)]
        ks = [h if p.n >= mi else 0 for p, (h, mi) in zip(problems, its)]
        if draws is None:
            draws = [mlpnp_draws(p.n, k, rng) for p, k in zip(problems, ks)]
        ds = [np.ascontiguousarray(d, np.int32).reshape(-1, 6) for d in draws]
        for d, k in zip(ds, ks):
            assert len(d) >= k, "six raw draws per iteration of mRansacMaxIts"
        P = (capi.MLPnPProblem * max(B, 1))(*[p.struct() for p in problems])
        Q = (capi.MLPnPParams * max(B, 1))(*[capi.MLPnPParams(float(q[0]), int(q[1]), int(q[2]), int(q[3]), float(q[4]), float(q[5])) for q in params])
        D = (C.c_void_p * max(B, 1))(*[d.ctypes.data for d in ds])
        outs = [_mlpnp_result(p, k, per_hypothesis) for p, k in zip(problems, ks)]
        R = (capi.MLPnPResult * max(B, 1))(*[o[0] for o in outs])
        capi.check(lib.orbp_mlpnp_solve_batch(int(device), P, B, Q, D, R), "orbp_mlpnp_solve_batch")
        return [_mlpnp_unpack(p, R[b], outs[b][1], outs[b][2], ks[b]) for b, p in enumerate(problems)]


# ---------------------------------------------------------------- TwoViewReconstruction (S/TwoViewReconstruction.cc)

def two_view_draws(n, iterations, rng):
    """The raw DUtils::Random::RandomInt(0, size - 1) results of `iterations` RANSAC iterations (S/TwoViewReconstruction.cc:88): int32
    (iterations, 8), column j uniform in [0, n - j).  rng: a numpy Generator or a seed."""
    if not isinstance(rng, np.random.Generator):
        rng = np.random.default_rng(rng)
    d = np.empty((int(iterations), 8), np.int32)
    for j in range(8):
        d[:, j] = rng.integers(0, max(int(n) - j, 1), size=int(iterations))
    return d


def two_view_resolve_draws(n, draws):
    """Raw draws -> the eight match indices of each minimal set (swap-with-back removal on vAllIndices, :81-96).  Host code."""
    d = np.ascontiguousarray(draws, np.int32).reshape(-1, 8)
    idx = np.zeros_like(d)
    capi.check(capi.load().orbi_two_view_resolve_draws(int(n), _vp(d), len(d), _vp(idx)), "orbi_two_view_resolve_draws")
    return idx


class TwoViewResult:
    """What one Reconstruct() call returned.  ok is the reference's return value; R21 (3 x 3), t21 (3), vP3D (n1 x 3) and vbTriangulated
    (n1 bool) are its outputs (zero when not ok).  model: 0 none, 1 homography, 2 fundamental.  motion_*: nGood / parallax / R / t of
    every motion hypothesis CheckRT ran, in the reference's order.  hyp_* (per_hypothesis=True): scores (2, iterations), models
    (2, iterations, 3, 3), masks (2, iterations, N) bool and the resolved sets (iterations, 8); row 0 is H, row 1 is F."""

    def __init__(self, r, vP3D, tri, hyp, iterations):
        self.ok = bool(r.success)
        self.model, self.n_matches, self.n_inliers = r.model, r.n_matches, r.n_inliers
        self.best_iteration_H, self.best_iteration_F = r.best_iteration_H, r.best_iteration_F
        self.SH, self.SF = np.float32(r.SH), np.float32(r.SF)
        self.H21 = np.array(r.H21, np.float32).reshape(3, 3)
        self.F21 = np.array(r.F21, np.float32).reshape(3, 3)
        self.R21 = np.array(r.R21, np.float32).reshape(3, 3)
        self.t21 = np.array(r.t21, np.float32)
        self.T1 = np.array(r.T1, np.float32).reshape(3, 3)
        self.T2 = np.array(r.T2, np.float32).reshape(3, 3)
        self.n_motions, self.best_motion, self.h_degenerate = r.n_motions, r.best_motion, bool(r.h_degenerate)
        self.motion_nGood = np.array(r.motion_nGood, np.int32)[: r.n_motions]
        self.motion_parallax = np.array(r.motion_parallax, np.float32)[: r.n_motions]
        self.motion_R = np.array(r.motion_R, np.float32).reshape(8, 3, 3)[: r.n_motions]
        self.motion_t = np.array(r.motion_t, np.float32).reshape(8, 3)[: r.n_motions]
        self.vP3D, self.vbTriangulated = vP3D, tri.astype(bool)
        self.hyp_scores = self.hyp_models = self.hyp_masks = self.hyp_sets = None
        if hyp is not None:
            sc, mo, ma, se = hyp
            self.hyp_scores = sc.reshape(2, iterations)
            self.hyp_models = mo.reshape(2, iterations, 3, 3)
            self.hyp_masks = np.unpackbits(ma.view(np.uint8), axis=1, bitorder="little")[:, : r.n_matches].astype(bool).reshape(2, iterations, -1)
            self.hyp_sets = se.reshape(iterations, 8)


class TwoViewReconstruction:
    """ORB_SLAM3::TwoViewReconstruction (I/TwoViewReconstruction.h): both RANSACs of a call in one kernel launch, every motion
    hypothesis of ReconstructH / ReconstructF in a second one.  K: 3 x 3 (or (fx, fy, cx, cy)).  Draws come from the caller (`draws`,
    raw RandomInt results as two_view_draws makes them) or from the object's own seeded generator."""

    def __init__(self, K, sigma=1.0, iterations=200, device=0, seed=0):
        K = np.asarray(K, np.float32)
        self.K = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])) if K.ndim == 2 else tuple(float(v) for v in K)
        self.mSigma, self.mMaxIterations = float(sigma), int(iterations)
        self.device = int(device)
        self.rng = np.random.default_rng(seed)
        self.lib = capi.load()

    def Reconstruct(self, vKeys1, vKeys2, vMatches12, draws=None, per_hypothesis=False):
        """vKeys1 / vKeys2: (n, 2) undistorted keypoint positions; vMatches12: n1 indices into vKeys2, -1 for none.  -> TwoViewResult."""
        k1 = np.ascontiguousarray(vKeys1, np.float32).reshape(-1, 2)
        k2 = np.ascontiguousarray(vKeys2, np.float32).reshape(-1, 2)
        m12 = np.ascontiguousarray(vMatches12, np.int32).reshape(-1)
        assert len(m12) == len(k1), "one entry of vMatches12 per keypoint of frame 1"
        n, H = int((m12 >= 0).sum()), self.mMaxIterations
        if draws is None:
            draws = two_view_draws(n, H, self.rng) if n >= 8 else np.zeros((max(H, 1), 8), np.int32)
        d = np.ascontiguousarray(draws, np.int32).reshape(-1, 8)
        assert len(d) >= H, "eight raw draws per iteration"
        p = capi.TwoViewProblem(C.sizeof(capi.TwoViewProblem), len(k1), len(k2), capi.ptr(k1), capi.ptr(k2), capi.ptr(m12), *self.K,
                                self.mSigma, H)
        r = capi.TwoViewResult()
        r.struct_size = C.sizeof(capi.TwoViewResult)
        vP3D, tri = np.zeros((max(len(k1), 1), 3), np.float32), np.zeros(max(len(k1), 1), np.uint8)
        r.vP3D, r.vbTriangulated = capi.ptr(vP3D), capi.ptr(tri)
        hyp = None
        if per_hypothesis:
            Hc = max(H, 1)
            hyp = (np.zeros(2 * Hc, np.float32), np.zeros((2 * Hc, 9), np.float32), np.zeros((2 * Hc, max((n + 63) // 64, 1)), np.uint64),
                   np.zeros((Hc, 8), np.int32))
            r.hyp_scores, r.hyp_models, r.hyp_masks, r.hyp_sets = (capi.ptr(a) for a in hyp)
        capi.check(self.lib.orbi_two_view_reconstruct(self.device, C.byref(p), _vp(d), C.byref(r)), "orbi_two_view_reconstruct")
        return TwoViewResult(r, vP3D[: len(k1)], tri[: len(k1)], hyp, H)


# ---------------------------------------------------------------- OptimizeSim3 (S/Optimizer.cc:4031-4310)

class Sim3OptProblem:
    """The flat problem OptimizeSim3's loop over the matches hands to g2o (S/Optimizer.cc:4083-4223): per kept match the map points
    in the two camera frames as float32 (P3D1c, P3D2c), the two observations and their invSigma2, the pinhole intrinsics
    (fx, fy, cx, cy) of pCamera1 / pCamera2, bFixScale, th2, and g2oS12 as q (x, y, z, w), t, s in float64.  index_edge = vnIndexEdge."""

    def __init__(self, X3Dc1, X3Dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2, bFixScale, th2, q, t, s, index_edge=None,
                 n_correspondences=None):
        f = np.float32
        self.X1 = np.ascontiguousarray(X3Dc1, f).reshape(-1, 3)
        self.X2 = np.ascontiguousarray(X3Dc2, f).reshape(-1, 3)
        self.obs1 = np.ascontiguousarray(obs1, f).reshape(-1, 2)
        self.obs2 = np.ascontiguousarray(obs2, f).reshape(-1, 2)
        self.w1 = np.ascontiguousarray(inv_sigma2_1, f).reshape(-1)
        self.w2 = np.ascontiguousarray(inv_sigma2_2, f).reshape(-1)
        self.n = len(self.X1)
        assert all(len(a) == self.n for a in (self.X2, self.obs1, self.obs2, self.w1, self.w2))
        self.K1 = tuple(float(v) for v in K1)
        self.K2 = tuple(float(v) for v in K2)
        self.fix_scale = bool(bFixScale)
        self.th2 = float(th2)
        self.q = np.array(q, np.float64).reshape(4)
        self.t = np.array(t, np.float64).reshape(3)
        self.s = float(s)
        self.index_edge = np.arange(self.n, dtype=np.int64) if index_edge is None else np.asarray(index_edge, np.int64)
        self.n_correspondences = self.n if n_correspondences is None else int(n_correspondences)

    def struct(self, camera_models=(0, 0)):
        st = capi.Sim3OptProblem()
        st.struct_size = C.sizeof(capi.Sim3OptProblem)
        st.n = self.n
        st.X3Dc1, st.X3Dc2, st.obs1, st.obs2 = capi.ptr(self.X1), capi.ptr(self.X2), capi.ptr(self.obs1), capi.ptr(self.obs2)
        st.inv_sigma2_1, st.inv_sigma2_2 = capi.ptr(self.w1), capi.ptr(self.w2)
        st.fx1, st.fy1, st.cx1, st.cy1 = self.K1
        st.fx2, st.fy2, st.cx2, st.cy2 = self.K2
        st.camera_model1, st.camera_model2 = int(camera_models[0]), int(camera_models[1])
        st.fix_scale = int(self.fix_scale)
        st.th2 = self.th2
        st.q[:] = self.q.tolist()
        st.t[:] = self.t.tolist()
        st.s = self.s
        st.n_correspondences = self.n_correspondences
        return st


class Sim3OptResult:
    """What OptimizeSim3 returned: nIn (its return value), returned_early (the `return 0` at :4271: q / t / s are then the input),
    q / t / s and S12 = [sR t; 0 1] (4 x 4 float64), removed (per pair: 0 kept, 1 / 2 NULL-ed in round 1 / in the final pass), trace
    (per LM iteration: round, lambda, chi2, trials), edge_chi2 (4 x n) when asked for."""

    def __init__(self, prob, r, removed, trace, edge_chi2):
        self.nIn, self.returned_early, self.n_bad_round1 = int(r.n_in), bool(r.returned_early), int(r.n_bad_round1)
        self.q, self.t, self.s = np.array(r.q[:], np.float64), np.array(r.t[:], np.float64), float(r.s)
        x, y, z, w = self.q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        self.S12 = np.eye(4)
        self.S12[:3, :3] = self.s * R
        self.S12[:3, 3] = self.t
        self.removed = removed[: prob.n].copy()
        self.iters = (int(r.iters[0]), int(r.iters[1]))
        self.chi2 = (float(r.chi2[0]), float(r.chi2[1]))
        self.trace = trace[: r.trace_len].copy()
        self.edge_chi2 = None if edge_chi2 is None else edge_chi2[:, : prob.n].copy()
        self.index_edge = prob.index_edge

    def apply(self, vpMatches1, null=-1):
        """vpMatches1[vnIndexEdge[i]] = NULL for every removed pair (:4244, :4294), in place."""
        vpMatches1[self.index_edge[self.removed != 0]] = null
        return vpMatches1


def _sim3opt_result(prob, edge_chi2):
    removed = np.zeros(max(prob.n, 1), np.uint8)
    trace = np.zeros((15, 4), np.float64)
    chi = np.zeros((4, max(prob.n, 1)), np.float64) if edge_chi2 else None
    r = capi.Sim3OptResult()
    r.struct_size = C.sizeof(capi.Sim3OptResult)
    r.removed, r.trace, r.trace_cap, r.edge_chi2 = capi.ptr(removed), capi.ptr(trace), 15, capi.ptr(chi)
    return r, removed, trace, chi


class _OptimizeSim3:
    """int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints) on a flat Sim3OptProblem:
    OptimizeSim3(problem) -> Sim3OptResult in one kernel launch; OptimizeSim3.batch([...]) refines every problem of the list in ONE
    launch and returns what the single calls return, bit for bit."""

    def __call__(self, problem, device=0, edge_chi2=False, camera_models=(0, 0)):
        st = problem.struct(camera_models)
        r, removed, trace, chi = _sim3opt_result(problem, edge_chi2)
        capi.check(capi.load().orbm_sim3_optimize(int(device), C.byref(st), C.byref(r)), "orbm_sim3_optimize")
        if chi is not None and problem.n > 0:
            chi = chi.reshape(-1)[: 4 * problem.n].reshape(4, problem.n)
        return Sim3OptResult(problem, r, removed, trace, chi)

    def batch(self, problems, device=0, edge_chi2=False):
        B = len(problems)
        P = (capi.Sim3OptProblem * max(B, 1))(*[p.struct() for p in problems])
        outs = [_sim3opt_result(p, edge_chi2) for p in problems]
        R = (capi.Sim3OptResult * max(B, 1))(*[o[0] for o in outs])
        capi.check(capi.load().orbm_sim3_optimize_batch(int(device), P, B, R), "orbm_sim3_optimize_batch")
        res = []
        for b, p in enumerate(problems):
            chi = outs[b][3]
            if chi is not None and p.n > 0:
                chi = chi.reshape(-1)[: 4 * p.n].reshape(4, p.n)
            res.append(Sim3OptResult(p, R[b], outs[b][1], outs[b][2], chi))
        return res


OptimizeSim3 = _OptimizeSim3()


def sim3opt_collect(Tcw1, Tcw2, mp_of_kp1, keys1, octave1, inv_level_sigma2_1, keys2, octave2, inv_level_sigma2_2, vpMatches1, mp_pos,
                    mp_bad, mp_index_in_kf2, K1, K2, g2oS12, th2, bFixScale, bAllPoints=True):
    """The loop of OptimizeSim3 over the matches (S/Optimizer.cc:4083-4223) on plain arrays -> Sim3OptProblem (index_edge = vnIndexEdge).
    Tcw1 / Tcw2: 4 x 4 float32 poses of pKF1 / pKF2; mp_of_kp1: map point id per keypoint of pKF1 or -1 (GetMapPointMatches); keys /
    octave: mvKeysUn pt (N x 2) and octave; vpMatches1: map point id matched to keypoint i of pKF1 or -1; mp_pos / mp_bad /
    mp_index_in_kf2: per map point GetWorldPos, isBad and GetIndexInKeyFrame(pKF2) (-1: not observed there); g2oS12 = (q xyzw, t, s).
    Points go to the camera frames the way the reference's CV_32F product does (every entry accumulated in double, rounded once)."""
    f, d = np.float32, np.float64
    vp = np.asarray(vpMatches1, np.int64)
    m1 = np.asarray(mp_of_kp1, np.int64)
    mp_pos = np.asarray(mp_pos, f).reshape(-1, 3)
    mp_bad = np.asarray(mp_bad, bool)
    idx2 = np.asarray(mp_index_in_kf2, np.int64)
    i = np.nonzero(vp >= 0)[0]                                      # :4085
    i = i[m1[i] >= 0]                                               # pMP1 == NULL: counted, skipped (:4128-4146)
    i = i[~(mp_bad[m1[i]] | mp_bad[vp[i]])]                         # :4104
    i2 = idx2[vp[i]]
    if not bAllPoints:                                              # :4148
        i, i2 = i[i2 >= 0], i2[i2 >= 0]

    def to_cam(T, P):
        T = np.asarray(T, f).astype(d)
        P = P.astype(d)
        return np.stack([((T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1]) + T[r, 2] * P[:, 2]) + T[r, 3] for r in range(3)], 1).astype(f)
    P1, P2 = to_cam(Tcw1, mp_pos[m1[i]]), to_cam(Tcw2, mp_pos[vp[i]])
    keep = ~(P2[:, 2] < 0)                                          # :4154, on the float
    i, i2, P1, P2 = i[keep], i2[keep], P1[keep], P2[keep]
    keys1, keys2 = np.asarray(keys1, f).reshape(-1, 2), np.asarray(keys2, f).reshape(-1, 2)
    s1, s2 = np.asarray(inv_level_sigma2_1, f), np.asarray(inv_level_sigma2_2, f)
    obs1, w1 = keys1[i], s1[np.asarray(octave1, np.int64)[i]]
    inside = i2 >= 0
    j2 = np.where(inside, i2, 0)
    with np.errstate(all="ignore"):
        invz = f(1) / P2[:, 2]                                      # :4194-4198: normalised coordinates as the observation
        norm = np.stack([P2[:, 0] * invz, P2[:, 1] * invz], 1).astype(f)
    obs2 = np.where(inside[:, None], keys2[j2] if len(keys2) else norm, norm).astype(f)
    # cv::KeyPoint(Point2f, mnTrackScaleLevel) sets `size`: the octave stays 0 (:4199, :4210)
    w2 = np.where(inside, s2[np.asarray(octave2, np.int64)[j2]] if len(keys2) else s2[0], s2[0]).astype(f)
    q, t, s = g2oS12
    return Sim3OptProblem(P1, P2, obs1, obs2, w1, w2, K1, K2, bFixScale, th2, q, t, s, index_edge=i)


class NewPointsKeyFrame:
    """orbm_newpoints_kf: one keyframe side of LocalMapping::CreateNewMapPoints / ORBmatcher::SearchForTriangulation.

    frame: the resident keyframe (a Frame: mvKeysUn, mDescriptors, mvuRight, mvDepth); featvec = (node_id, start, feat_idx) of mFeatVec;
    has_mp[i] = GetMapPoint(i) != NULL; Tcw / Twc (3x4 or 4x4) and Ow as the keyframe holds them; cam = (fx, fy, cx, cy); mb, mbf;
    scale_factors / level_sigma2 = mvScaleFactors / mvLevelSigma2; scale_factor = mfScaleFactor; keys_xy = mvKeys[i].pt when the
    keyframe's image is distorted (None: mvKeys == mvKeysUn); invf = (invfx, invfy), default 1.0f / fx as S/Frame.cc:140-141."""

    def __init__(self, frame, featvec, has_mp, Tcw, Twc, Ow, cam, mb, mbf, scale_factors, level_sigma2, scale_factor, keys_xy=None, invf=None):
        self.frame = frame
        self.fv, self._fv_keep = views.featvec_view(*featvec)
        self.has_mp = np.ascontiguousarray(has_mp, np.uint8)
        self.keys_xy = None if keys_xy is None else np.ascontiguousarray(np.asarray(keys_xy, np.float32).reshape(-1, 2))
        self.Tcw = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12])
        self.Twc = np.ascontiguousarray(np.asarray(Twc, np.float32).reshape(-1)[:12])
        self.Ow = np.ascontiguousarray(np.asarray(Ow, np.float32).reshape(3))
        self.cam = tuple(np.float32(c) for c in cam)
        self.invf = tuple(np.float32(v) for v in invf) if invf is not None else (np.float32(1.0) / self.cam[0], np.float32(1.0) / self.cam[1])
        self.mb, self.mbf = np.float32(mb), np.float32(mbf)
        self.scale_factors = np.ascontiguousarray(scale_factors, np.float32)
        self.level_sigma2 = np.ascontiguousarray(level_sigma2, np.float32)
        self.scale_factor = np.float32(scale_factor)

    def fill(self, k):
        k.struct_size = C.sizeof(capi.NewPointsKF)
        k.frame = self.frame.h
        k.featvec = self.fv
        k.has_mp = capi.ptr(self.has_mp)
        k.keys_xy = capi.ptr(self.keys_xy)
        for i in range(12):
            k.Tcw[i], k.Twc[i] = float(self.Tcw[i]), float(self.Twc[i])
        for i in range(3):
            k.Ow[i] = float(self.Ow[i])
        k.fx, k.fy, k.cx, k.cy = [float(c) for c in self.cam]
        k.invfx, k.invfy = float(self.invf[0]), float(self.invf[1])
        k.mb, k.mbf = float(self.mb), float(self.mbf)
        k.n_levels = len(self.scale_factors)
        k.scale_factors, k.level_sigma2 = capi.ptr(self.scale_factors), capi.ptr(self.level_sigma2)
        k.scale_factor = float(self.scale_factor)
        return k


def _newpoints_params(only_stereo, coarse, check_orientation, far_points, th_far_points):
    p = capi.NewPointsParams()
    p.struct_size = C.sizeof(capi.NewPointsParams)
    p.only_stereo, p.coarse, p.check_orientation, p.far_points = int(only_stereo), int(coarse), int(check_orientation), int(far_points)
    p.th_far_points = float(th_far_points)
    return p


class NewMapPoints:
    """Outcome of CreateNewMapPoints: out (NEWPOINT_DTYPE, the reference's creation order; the points created before the loop's
    CheckNewKeyFrames() exit at neighbour i are the prefix with neighbour < i), records (B x n1, NEWPOINTS_RECORD_DTYPE, before the
    replay) and matches (B x n1, vMatches12 per neighbour after the replay)."""

    def __init__(self, out, records, matches):
        self.out, self.records, self.matches = out, records, matches


class NewPointsCall:
    """The flattened arguments of one orbm_create_new_points call, kept for repeated calls on the same keyframes (a timing loop);
    run() is the call itself."""

    def __init__(self, kf1, neighbours, only_stereo=False, coarse=False, check_orientation=False, far_points=False, th_far_points=0.0,
                 cap=None):
        self.lib = capi.load()
        self.keep = (kf1, list(neighbours))
        self.B, self.n1 = len(neighbours), kf1.frame.n
        self.K1 = kf1.fill(capi.NewPointsKF())
        self.KN = (capi.NewPointsKF * max(self.B, 1))()
        for b, kf in enumerate(neighbours):
            kf.fill(self.KN[b])
        self.p = _newpoints_params(only_stereo, coarse, check_orientation, far_points, th_far_points)
        self.cap = self.B * self.n1 if cap is None else int(cap)
        self.out = np.zeros(max(self.cap, 1), capi.NEWPOINT_DTYPE)
        self.records = np.zeros((self.B, self.n1), capi.NEWPOINTS_RECORD_DTYPE)
        self.matches = np.full((self.B, self.n1), -1, np.int32)
        self.n = C.c_int(0)

    def run(self):
        capi.check(self.lib.orbm_create_new_points(C.byref(self.K1), C.byref(self.KN), self.B, C.byref(self.p), capi.ptr(self.out), self.cap,
                                                   C.byref(self.n), capi.ptr(self.records) if self.records.size else None,
                                                   capi.ptr(self.matches) if self.matches.size else None), "orbm_create_new_points")
        return NewMapPoints(self.out[: self.n.value].copy(), self.records, self.matches)


def CreateNewMapPoints(kf1, neighbours, only_stereo=False, coarse=False, check_orientation=False, far_points=False, th_far_points=0.0,
                       cap=None):
    """LocalMapping::CreateNewMapPoints, S/LocalMapping.cc:520-865, for the neighbours that passed the baseline gates: ONE launch for
    all of them, then the serial bookkeeping across neighbours on the host."""
    return NewPointsCall(kf1, neighbours, only_stereo, coarse, check_orientation, far_points, th_far_points, cap).run()


def SearchForTriangulation(kf1, kf2, only_stereo=False, coarse=False, check_orientation=True):
    """ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse), S/ORBmatcher.cc:961-1202: returns
    vMatchedPairs as an (n, 2) array, idx1 ascending."""
    lib = capi.load()
    K1, K2 = kf1.fill(capi.NewPointsKF()), kf2.fill(capi.NewPointsKF())
    p = _newpoints_params(only_stereo, coarse, check_orientation, False, 0.0)
    cap = max(kf1.frame.n, 1)
    pairs = np.zeros((cap, 2), np.int32)
    n = C.c_int(0)
    capi.check(lib.orbm_search_for_triangulation(C.byref(K1), C.byref(K2), C.byref(p), capi.ptr(pairs), cap, C.byref(n)),
               "orbm_search_for_triangulation")
    return pairs[: n.value].copy()


class FuseKeyFrame:
    """orbm_fuse_kf: one target keyframe of ORBmatcher::Fuse.

    frame: the resident keyframe (a Frame: mvKeysUn, mDescriptors, mvuRight, the grid, the image bounds); cam = (fx, fy, cx, cy); mbf;
    scale_factors / inv_level_sigma2 = mvScaleFactors / mvInvLevelSigma2; log_scale_factor = mfLogScaleFactor.  LocalMapping form: Tcw
    (3x4 or 4x4) and Ow as the keyframe holds them.  Sim3 form: Scw (4x4)."""

    def __init__(self, frame, cam, mbf, scale_factors, inv_level_sigma2, log_scale_factor, Tcw=None, Ow=None, Scw=None):
        self.frame = frame
        self.Tcw = np.zeros(12, np.float32) if Tcw is None else np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12])
        self.Ow = np.zeros(3, np.float32) if Ow is None else np.ascontiguousarray(np.asarray(Ow, np.float32).reshape(3))
        self.Scw = np.zeros(16, np.float32) if Scw is None else np.ascontiguousarray(np.asarray(Scw, np.float32).reshape(16))
        self.cam = tuple(np.float32(c) for c in cam)
        self.mbf = np.float32(mbf)
        self.scale_factors = np.ascontiguousarray(scale_factors, np.float32)
        self.inv_level_sigma2 = np.ascontiguousarray(inv_level_sigma2, np.float32)
        self.log_scale_factor = np.float32(log_scale_factor)

    def fill(self, k):
        k.struct_size = C.sizeof(capi.FuseKF)
        k.frame = self.frame.h
        for i in range(12):
            k.Tcw[i] = float(self.Tcw[i])
        for i in range(3):
            k.Ow[i] = float(self.Ow[i])
        for i in range(16):
            k.Scw[i] = float(self.Scw[i])
        k.fx, k.fy, k.cx, k.cy = [float(c) for c in self.cam]
        k.mbf = float(self.mbf)
        k.n_levels = len(self.scale_factors)
        k.scale_factors, k.inv_level_sigma2 = capi.ptr(self.scale_factors), capi.ptr(self.inv_level_sigma2)
        k.log_scale_factor = float(self.log_scale_factor)
        return k


def Fuse(kfs, points, th=3.0, sim3_form=False, skip=None):
    """ORBmatcher::Fuse up to bestIdx / bestDist (S/ORBmatcher.cc:1451-1566, or :1642-1716 with sim3_form) for every (keyframe, point)
    pair in ONE launch.  kfs: FuseKeyFrame list; points: (orbm_worldpoints_view, keepalive) of views.worldpoints_view; skip: K x P bytes or
    None.  Returns (records K x P of FUSE_RECORD_DTYPE, candidate lists K x P x FUSE_CAND_CAP uint16, 0xFFFF = unused); the serial
    part of Fuse is the caller's replay."""
    lib = capi.load()
    view = points[0] if isinstance(points, tuple) else points
    K, P = len(kfs), int(view.m)
    arr = (capi.FuseKF * max(K, 1))()
    for k, kf in enumerate(kfs):
        kf.fill(arr[k])
    p = capi.FuseParams()
    p.struct_size, p.th, p.sim3_form = C.sizeof(capi.FuseParams), float(th), int(bool(sim3_form))
    rec = np.zeros((K, P), capi.FUSE_RECORD_DTYPE)
    cand = np.full((K, P, capi.FUSE_CAND_CAP), 0xFFFF, np.uint16)
    if skip is not None:
        skip = np.ascontiguousarray(skip, np.uint8)
        assert skip.shape == (K, P)
    capi.check(lib.orbm_fuse(C.byref(arr), K, C.byref(view), capi.ptr(skip) if skip is not None and skip.size else None, C.byref(p),
                             capi.ptr(rec) if rec.size else None, capi.ptr(cand) if cand.size else None), "orbm_fuse")
    return rec, cand


class InertialBA:
    """inertial_ba_create / _destroy: the device buffers, the LDL^T solver object and the stream of Optimizer.LocalInertialBA calls."""

    def __init__(self, device=0):
        self.lib = capi.load()
        self.h = C.c_void_p()
        capi.check(self.lib.inertial_ba_create(int(device), C.byref(self.h)), "inertial_ba_create")

    def set_stream(self, hip_stream):
        capi.check(self.lib.inertial_ba_set_stream(self.h, C.c_void_p(hip_stream) if hip_stream else None), "inertial_ba_set_stream")

    def set_profiling(self, on):
        capi.check(self.lib.inertial_ba_set_profiling(self.h, int(bool(on))), "inertial_ba_set_profiling")

    def phase_ms(self):
        """structure, linearise, Schur, LDL^T, update of the last solve (set_profiling(True) first)"""
        ms = (C.c_double * 5)()
        capi.check(self.lib.inertial_ba_get_phase_ms(self.h, ms), "inertial_ba_get_phase_ms")
        return list(ms)

    def close(self):
        if self.h:
            self.lib.inertial_ba_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
