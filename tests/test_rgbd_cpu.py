"""CPU-side checks of the RGB-D Frame constructor: every new entry point refuses what the header says it refuses before it touches a
device, the ctypes mirror of orbx_rgbd_image has the header's layout, the model (tests/rgbd_model.py) gives the known answers of the
pinned arithmetic, real extractions never reach the in-bounds guard, and the colour formula holds on every triple the test picks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import api, synth
import rgbd_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW = ["orbx_frame_rgbd", "orbx_frame_rgbd_dev", "orbx_frame_rgbd_submit", "orbx_frame_rgbd_dev_submit", "orbx_frame_rgbd_wait",
       "orbx_depth_at_points"]


def test_new_entry_points_are_exported_and_declared():
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    for s in NEW:
        assert hasattr(lib, s) and s in capi.EXPORTED_SYMBOLS and ("int %s(" % s) in hdr, s
    assert "#define ORBX_DEPTH_U16 %d" % capi.ORBX_DEPTH_U16 in hdr and "#define ORBX_DEPTH_F32 %d" % capi.ORBX_DEPTH_F32 in hdr


def test_rgbd_image_mirror_has_the_headers_layout(tmp_path):
    fields = [f for f, _ in capi.OrbxRgbdImage._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "orbgpu.h"', 'int main(void) {',
             '  printf("%zu", sizeof(orbx_rgbd_image));']
    lines += ['  printf(" %%zu", offsetof(orbx_rgbd_image, %s));' % f for f in fields]
    lines.append('  printf("\\n"); return 0; }')
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(capi.OrbxRgbdImage)
    assert out[1:] == [getattr(capi.OrbxRgbdImage, f).offset for f in fields]
    assert capi.OrbxRgbdImage.struct_size.offset == 0


def _image(channels=1, w=64, h=48, dtype=np.uint16):
    img = np.zeros((h, w) if channels == 1 else (h, w, channels), np.uint8)
    dep = np.zeros((h, w), dtype)
    im, ww, hh, keep = api.ORBextractor._rgbd_image(img, dep, 1.0, False)
    return im, keep


def test_argument_checks_need_no_device():
    """Whatever can be refused from the arguments alone is refused before a device is selected: a NULL handle for the five constructor
    entries, every bad argument of orbx_depth_at_points; with good arguments and no GPU the latter says ORBG_NO_DEVICE."""
    lib = capi.load()
    im, keep = _image()
    n = C.c_int(0)
    byim = C.byref(im)
    assert lib.orbx_frame_rgbd(None, None, None, None, byim, 64, 48, 40.0, None, None, None, None, None, 0, C.byref(n)) == capi.ORBG_BAD_ARG
    assert lib.orbx_frame_rgbd_dev(None, None, None, None, byim, 64, 48, 40.0, None, None, None, None, None, 0, C.byref(n)) == capi.ORBG_BAD_ARG
    assert lib.orbx_frame_rgbd_submit(None, None, None, None, byim, 64, 48, 40.0, 0) == capi.ORBG_BAD_ARG
    assert lib.orbx_frame_rgbd_submit(None, None, None, None, byim, 64, 48, 40.0, 1) == capi.ORBG_BAD_ARG
    assert lib.orbx_frame_rgbd_dev_submit(None, None, None, None, byim, 64, 48, 40.0) == capi.ORBG_BAD_ARG
    assert lib.orbx_frame_rgbd_wait(None, C.byref(n)) == capi.ORBG_BAD_ARG
    xy = np.array([[1.5, 2.5], [3.0, 4.0]], F32)
    dep = np.ones((9, 17), np.uint16)
    ur = np.zeros(2, F32); dp = np.zeros(2, F32)

    def call(xy_=xy, n_=2, img=dep, typ=capi.ORBX_DEPTH_U16, stride=None, w=17, h=9, bf=40.0, ur_=ur, dp_=dp):
        return lib.orbx_depth_at_points(0, capi.ptr(xy_), None, n_, capi.ptr(img), typ, img.strides[0] if stride is None else stride, w, h,
                                        1.0 / 5000, bf, capi.ptr(ur_), capi.ptr(dp_))

    assert call(n_=-1) == capi.ORBG_BAD_ARG
    assert call(xy_=None) == capi.ORBG_BAD_ARG
    assert call(ur_=None) == capi.ORBG_BAD_ARG and call(dp_=None) == capi.ORBG_BAD_ARG
    assert call(img=None, stride=34) == capi.ORBG_BAD_ARG
    assert call(typ=2) == capi.ORBG_BAD_ARG and call(typ=-1) == capi.ORBG_BAD_ARG
    assert call(stride=33) == capi.ORBG_BAD_ARG                              # a row of 17 u16 needs 34 bytes
    assert call(typ=capi.ORBX_DEPTH_F32, stride=34) == capi.ORBG_BAD_ARG     # ... and 68 as float32
    assert call(w=0) == capi.ORBG_BAD_ARG and call(h=0) == capi.ORBG_BAD_ARG
    assert call(bf=0.0) == capi.ORBG_BAD_ARG and call(bf=-1.0) == capi.ORBG_BAD_ARG and call(bf=float("nan")) == capi.ORBG_BAD_ARG
    if lib.orbg_device_count() <= 0:
        assert call() == capi.ORBG_NO_DEVICE
        with pytest.raises(capi.OrbGpuError) as e:
            api.depth_at_points(xy, dep, 40.0, 1.0 / 5000)
        assert e.value.code == capi.ORBG_NO_DEVICE


def test_depth_map_factor_is_trackings_float():
    for y in (5000.0, 1.0, 0.0, 1e-6, -1e-6, 1000.0, 0.5, 5208.0):
        assert api.depth_map_factor(y).tobytes() == rm.depth_map_factor(y).tobytes()
    assert rm.depth_map_factor(5000.0) == F32(1.0) / F32(5000.0) and rm.depth_map_factor(0.0) == 1 and rm.depth_map_factor(9e-6) == 1
    assert rm.depth_map_factor(1.1e-5) == F32(1.0) / F32(1.1e-5)
    assert not rm.needs_convert(np.float32, 1.0) and not rm.needs_convert(np.float32, 1.000009)
    assert rm.needs_convert(np.float32, 1.00002) and rm.needs_convert(np.uint16, 1.0) and rm.needs_convert(np.float32, 0.0002)


def test_model_known_answers_u16_and_f32():
    f = rm.depth_map_factor(5000.0)
    dep = np.zeros((9, 17), np.uint16)
    dep[2, 3] = 5000; dep[4, 5] = 12345; dep[8, 16] = 65535; dep[0, 0] = 1
    xy = np.array([[3, 2], [5, 4], [16, 8], [0, 0], [1, 1]], F32)
    ur, dp = rm.depth_at_points(xy, xy[:, 0], dep, f, 40.0)
    exp = [F32(5000) * f, F32(12345) * f, F32(65535) * f, F32(1) * f]
    assert [v for v in dp[:4]] == exp and dp[4] == -1 and ur[4] == -1
    assert abs(float(dp[0]) - 1.0) < 1e-6 and abs(float(dp[1]) - 2.469) < 1e-6
    for i in range(4):
        assert ur[i] == F32(xy[i, 0] - F32(F32(40.0) / exp[i]))
    # the whole image converted first (what the reference does) gives the same bits as converting the values read
    ur2, dp2 = rm.depth_at_points(xy, xy[:, 0], dep, f, 40.0, convert_whole_image=True)
    assert ur2.tobytes() == ur.tobytes() and dp2.tobytes() == dp.tobytes()
    # f32, factor 1: the bits are untouched (a value no product by 1.0f could change anyway, so take the condition itself)
    d32 = np.zeros((9, 17), F32)
    d32[2, 3] = F32(1.2345678); d32[4, 5] = np.nextafter(F32(0), F32(1))
    ur, dp = rm.depth_at_points(xy[:2], xy[:2, 0], d32, 1.0, 40.0)
    assert dp.tobytes() == d32[[2, 4], [3, 5]].tobytes()
    # f32, factor != 1: one float32 product
    ur, dp = rm.depth_at_points(xy[:1], xy[:1, 0], d32, F32(0.001), 40.0)
    assert dp[0] == F32(F32(1.2345678) * F32(0.001)) and ur[0] == F32(F32(3) - F32(F32(40) / dp[0]))
    ur2, dp2 = rm.depth_at_points(xy[:1], xy[:1, 0], d32, F32(0.001), 40.0, convert_whole_image=True)
    assert dp2.tobytes() == dp.tobytes() and ur2.tobytes() == ur.tobytes()


def test_model_zero_negative_nan_inf_and_truncation():
    d32 = np.full((9, 17), 2.0, F32)
    d32[1, 1] = 0.0; d32[1, 2] = -1.5; d32[1, 3] = np.nan; d32[1, 4] = np.inf; d32[1, 5] = -0.0; d32[1, 6] = -np.inf
    xy = np.array([[1, 1], [2, 1], [3, 1], [4, 1], [5, 1], [6, 1]], F32)
    ur, dp = rm.depth_at_points(xy, xy[:, 0] + F32(0.25), d32, 1.0, 40.0)
    assert list(dp[:3]) == [-1, -1, -1] and list(ur[:3]) == [-1, -1, -1] and dp[4] == -1 and dp[5] == -1 and ur[5] == -1
    assert np.isinf(dp[3]) and dp[3] > 0 and ur[3] == F32(4.25)              # +inf passes d > 0; bf / inf = 0
    # .999 coordinates truncate: (3.999, 2.999) reads pixel (3, 2), not (4, 3)
    d = np.arange(9 * 17, dtype=np.uint16).reshape(9, 17) + 1
    xy = np.array([[3.999, 2.999], [4.0, 3.0], [0.999, 0.999], [16.999, 8.999]], F32)
    ur, dp = rm.depth_at_points(xy, xy[:, 0], d, 1.0, 40.0)
    assert list(dp) == [F32(d[2, 3]), F32(d[3, 4]), F32(d[0, 0]), F32(d[8, 16])]
    # outside: no read, -1 (17.0 is the first column outside; so is row 9.0); NaN coordinates too
    xy = np.array([[17.0, 1.0], [1.0, 9.0], [-1.0, 1.0], [1.0, -1.0], [np.nan, 1.0], [1e9, 1.0], [-0.5, 0.0]], F32)
    ur, dp = rm.depth_at_points(xy, xy[:, 0], d, 1.0, 40.0)
    assert list(dp[:6]) == [-1] * 6 and dp[6] == F32(d[0, 0])               # (int)(-0.5f) == 0


def test_model_distorted_camera_depth_from_the_distorted_pixel_uright_from_the_undistorted_x():
    """A TUM1-like k1: mvKeys and mvKeysUn differ by more than a pixel away from the centre, so the depth is that of the DISTORTED
    pixel and uRight is measured from the UNDISTORTED x -- and the two wrong combinations give different numbers."""
    from oracle import binding as ob
    cam4 = (517.3, 516.5, 318.6, 255.3)
    dist = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)                          # TUM1.yaml
    rng = np.random.RandomState(3)
    xy = rng.uniform([19, 19], [620, 460], (400, 2)).astype(F32)
    un = ob.undistort_points(xy, cam4, dist)
    moved = np.abs(un - xy).max(axis=1) > 1.0
    assert moved.sum() > 50
    # every pixel differs from all its neighbours within +-50 pixels
    dep = ((641 * np.arange(480)[:, None] + np.arange(640)[None, :]) % 65521 + 1).astype(np.uint16)
    f = rm.depth_map_factor(5000.0)
    ur, dp = rm.depth_at_points(xy, un[:, 0], dep, f, 40.0)
    right_d = dep[xy[:, 1].astype(int), xy[:, 0].astype(int)].astype(F32) * f
    assert dp.tobytes() == right_d.tobytes()
    assert ur.tobytes() == (un[:, 0] - F32(40.0) / right_d).astype(F32).tobytes()
    # wrong 1: depth read at the undistorted pixel; wrong 2: uRight from the distorted x
    inb = (un[:, 0] >= 0) & (un[:, 0] < 640) & (un[:, 1] >= 0) & (un[:, 1] < 480)
    ur_w1, dp_w1 = rm.depth_at_points(un, un[:, 0], dep, f, 40.0)
    ur_w2, dp_w2 = rm.depth_at_points(xy, xy[:, 0], dep, f, 40.0)
    m = moved & inb
    mx = np.abs(un[:, 0] - xy[:, 0]) > 1.0
    assert m.sum() > 50 and mx.sum() > 50 and np.all(dp_w1[m] != dp[m]) and np.all(ur_w2[mx] != ur[mx])


@pytest.mark.parametrize("name", ["extract_96x72.npz", "extract_160x120.npz", "extract_640x480.npz"])
def test_truncated_keypoint_coordinates_lie_inside_the_image_on_the_golden_extractions(name):
    """The in-bounds guard of the depth lookup never fires on what the extractor produces."""
    g = np.load(os.path.join(ROOT, "tests", "golden", name))
    h, w = g["L"].shape
    keys = [f for f in g.files if f.startswith("kps")]
    assert keys
    for key in keys:
        k = g[key]
        assert len(k) > 0
        col, row = k["x"].astype(np.int64), k["y"].astype(np.int64)
        assert col.min() >= 0 and col.max() < w and row.min() >= 0 and row.max() < h, (name, key)
        d = np.ones((h, w), np.uint16)
        ur, dp = rm.depth_at_points(np.stack([k["x"], k["y"]], axis=1), k["x"], d, 1.0, 40.0)
        assert np.all(dp == 1.0)


def test_gray_from_colour_is_opencvs_fixed_point_formula():
    rng = np.random.RandomState(7)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)])
    edges = np.array([[v, e1, e2] for v in range(256) for e1 in (0, 255) for e2 in (0, 255)])
    edges = np.concatenate([edges, edges[:, [1, 0, 2]], edges[:, [1, 2, 0]]])
    rand = rng.randint(0, 256, (200000, 3))
    grays = np.repeat(np.arange(256)[:, None], 3, axis=1)
    rgb = np.concatenate([corners, edges, rand, grays]).astype(np.uint8)
    got = rm.gray_from_color(rgb[None, :, :], True)[0]
    r, g, b = [rgb[:, i].astype(int) for i in range(3)]
    exp = [(int(r[i]) * 4899 + int(g[i]) * 9617 + int(b[i]) * 1868 + 8192) >> 14 for i in range(0, len(rgb), 37)]
    assert list(got[::37]) == exp
    assert np.array_equal(got[-256:], np.arange(256))                          # 4899 + 9617 + 1868 = 2^14: gray stays gray
    assert got.min() == 0 and got.max() == 255
    # within half a level of the real-valued weights it rounds
    assert np.abs(got - (0.299 * r + 0.587 * g + 0.114 * b)).max() < 0.51
    # BGR order = the same formula with the first and third byte swapped; a fourth channel is ignored
    assert np.array_equal(rm.gray_from_color(rgb[None, :, ::-1], False)[0], got)
    rgba = np.concatenate([rgb, rng.randint(0, 256, (len(rgb), 1)).astype(np.uint8)], axis=1)
    assert np.array_equal(rm.gray_from_color(rgba[None], True)[0], got)


def test_scene_renderings_for_rgbd(small_scene):
    sc = small_scene
    L, R, Tcw = sc.stereo_pair(3)
    # depth image: the plane's depth, consistent with depth_at of the pixel centres
    d = sc.depth_image(Tcw)
    assert d.dtype == np.float32 and d.shape == L.shape and 1.5 < d.min() and d.max() < 6.0
    k = np.zeros(3, capi.KEYPOINT_DTYPE)
    k["x"] = [10, 100, 300]; k["y"] = [20, 120, 200]
    assert np.allclose(sc.depth_at(k, Tcw), d[[20, 120, 200], [10, 100, 300]], atol=1e-5)
    d16 = sc.depth_image(Tcw, np.uint16, 5000.0)
    assert d16.dtype == np.uint16 and np.abs(d16.astype(np.float64) / 5000.0 - d).max() <= 0.5 / 5000 + 1e-6
    # colour: unequal channels -> the channel order matters
    for ch in (3, 4):
        rgb = sc.color_image(L, ch, rgb_order=True)
        bgr = sc.color_image(L, ch, rgb_order=False)
        assert rgb.shape == L.shape + (ch,) and np.array_equal(rgb[..., :3], bgr[..., 2::-1])
        right = rm.gray_from_color(rgb, True)
        assert np.array_equal(right, rm.gray_from_color(bgr, False))
        wrong = rm.gray_from_color(rgb, False)
        assert (right != wrong).mean() > 0.9
