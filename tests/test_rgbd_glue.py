"""orbgpu::FrameOnDevice::RgbdCtor and RgbdCtorSubmitHost / RgbdCtorWait (include/orbgpu_adapters.hpp): tests/cpp/rgbd_glue.cpp fills a
mock Frame from a BGR image and a 16-bit depth image of a distorted camera through both forms; what it dumps equals tests/rgbd_model.py.
Without a device the program builds warning-free and reports the missing device instead of producing a frame."""
import os
import struct
import subprocess

import numpy as np
import pytest

from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import synth
import rgbd_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)


def _build(out):
    lib_dir = os.path.join(ROOT, "multi_orbslam3_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", CPP,
                           os.path.join(CPP, "rgbd_glue.cpp"), "-o", out, "-pthread", "-L", lib_dir, "-lorbgpu",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


def _scene_file(path, img, dep, rgb_order, cam, bounds, factor, dist):
    h, w = dep.shape
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", w, h, img.shape[2] if img.ndim == 3 else 1, int(rgb_order),
                            capi.ORBX_DEPTH_U16 if dep.dtype == np.uint16 else capi.ORBX_DEPTH_F32, int(dist is not None)))
        f.write(struct.pack("<16f", *[float(c) for c in cam], bounds[0], bounds[1], bounds[2], bounds[3], float(factor), *(dist or (0,) * 5)))
        f.write(np.ascontiguousarray(img).tobytes()); f.write(np.ascontiguousarray(dep).tobytes())
    return path


def _case():
    sc = synth.Scene(160, 120, tex_size=(400, 300), px_per_m=50.0)
    L, R, Tcw = sc.stereo_pair(2)
    dep = sc.depth_image(Tcw, np.uint16, 5000.0)
    dep[30:60, 40:80] = 0
    bgr = sc.color_image(L, 3, rgb_order=False)
    return sc, bgr, dep


def test_glue_builds_warning_free_and_reports_a_missing_device(tmp_path):
    exe = _build(str(tmp_path / "rgbd_glue"))
    if capi.load().orbg_device_count() > 0:
        return
    sc, bgr, dep = _case()
    p = sc.frame_view_params()
    s = _scene_file(str(tmp_path / "s.bin"), bgr, dep, False, p["cam"], p["bounds"], rm.depth_map_factor(5000.0), None)
    r = subprocess.run([exe, s, str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 3 and "no usable HIP device" in r.stderr and not os.path.exists(str(tmp_path / "o.bin"))


@pytest.mark.gpu
def test_glue_fills_the_mock_frame_as_the_model_does(tmp_path):
    from oracle import binding as ob
    exe = os.path.join(CPP, "rgbd_glue")
    if not os.path.exists(exe):
        _build(exe)
    sc, bgr, dep = _case()
    p = sc.frame_view_params()
    fac = rm.depth_map_factor(5000.0)
    bounds = ob.image_bounds(sc.W, sc.H, p["cam"][:4], DIST)
    m = rm.rgbd_frame(bgr, dep, p["cam"], float(sc.cam["bf"]), fac, DIST, rgb_order=False)
    s = _scene_file(str(tmp_path / "s.bin"), bgr, dep, False, p["cam"], bounds, fac, DIST)
    out = str(tmp_path / "o.bin")
    r = subprocess.run([exe, s, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    n = len(m["kps"])
    assert n > 100 and r.stdout.split() == ["n", str(n), str(n), "frame_n", str(n)]
    raw = open(out, "rb").read()
    off = 0
    for form in ("synchronous", "two halves"):
        assert struct.unpack_from("<i", raw, off)[0] == n, form
        off += 4
        for name, size in (("kps", 24), ("kps_un", 24), ("desc", 32), ("uright", 4), ("depth", 4)):
            assert raw[off:off + n * size] == m[name].tobytes(), (form, name)
            off += n * size
    assert off == len(raw)
