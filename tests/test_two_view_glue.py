"""orbgpu::TwoViewReconstruction (include/orbgpu_dropin.hpp): tests/cpp/two_view_glue.cpp builds against the mock objects and against
the signature-only OpenCV stub; on the GPU its run equals the API call on the same inputs and the draws its functor took."""
import os
import struct
import subprocess

import numpy as np
import pytest

import two_view_model as tm
from multi_orbslam3_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _build(out, extra=()):
    lib_dir = os.path.join(ROOT, "multi_orbslam3_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unused-function", *extra, "-I", os.path.join(ROOT, "include"), "-I", CPP,
                           os.path.join(CPP, "two_view_glue.cpp"), "-o", out, "-pthread", "-L", lib_dir, "-lorbgpu",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


def _scene_file(path, sc):
    with open(path, "wb") as f:
        f.write(struct.pack("<ii4f", len(sc.keys1), len(sc.keys2), *sc.cam))
        f.write(np.ascontiguousarray(sc.keys1, "<f4").tobytes()); f.write(np.ascontiguousarray(sc.keys2, "<f4").tobytes())
        f.write(np.ascontiguousarray(sc.matches12, "<i4").tobytes())
    return path


def _parse(text):
    out = {}
    for line in text.splitlines():
        key, _, rest = line.partition(":") if ":" in line.split(" ")[0] else (line.split(" ")[0], "", " ".join(line.split(" ")[1:]))
        out.setdefault(key, []).append(rest.split())
    return out


def _floats(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


@pytest.mark.parametrize("flags", [("-DMOCK_STRICT_ACCESS",), ("-DHAVE_OPENCV", "-I" + os.path.join(CPP, "opencv_stub"))], ids=["mocks", "opencv_stub"])
def test_glue_builds_and_refuses_fewer_than_eight_matches_without_a_device(tmp_path, flags):
    exe = _build(str(tmp_path / "two_view_glue"), flags)
    sc = tm.scene("3d", 7, 3, n_extra1=4, n_extra2=6)
    p = subprocess.run([exe, _scene_file(str(tmp_path / "s.bin"), sc), "20"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    o = _parse(p.stdout)
    assert o["ok"] == [["0"]] and o["outputs"] == [["untouched", "1"]] and o["draws"] == [[]]


@pytest.mark.gpu
def test_glue_equals_the_api_on_the_same_inputs(tmp_path):
    exe = os.path.join(CPP, "two_view_glue")
    if not os.path.exists(exe):
        _build(exe, ("-DMOCK_STRICT_ACCESS",))
    sc, d, a, b = tm.case("wide")
    H = 200
    p = subprocess.run([exe, _scene_file(str(tmp_path / "s.bin"), sc), str(H)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    o = _parse(p.stdout)
    draws = np.array([int(w) for w in o["draws"][0]], np.int32).reshape(H, 8)
    N = tm.CASES["wide"][1]
    assert (draws >= 0).all() and (draws <= N - 1 - np.arange(8)).all()
    # RandomInt's formula over rand() after srand(0): the first process-wide draws
    import ctypes
    libc = ctypes.CDLL(None)
    libc.srand(0)
    want = [int((libc.rand() / (2147483647 + 1.0)) * (N - j)) for _ in range(2) for j in range(8)]
    assert draws[:2].reshape(-1).tolist() == want
    g = api.TwoViewReconstruction(sc.cam, 1.0, H).Reconstruct(sc.keys1, sc.keys2, sc.matches12, draws=draws)
    assert o["ok"] == [[str(int(g.ok))]] and g.ok
    assert o["model"][0][0] == str(g.model) and o["model"][0][2] == str(g.best_iteration_H) and o["model"][0][4] == str(g.best_iteration_F)
    assert _floats(o["scores"][0]).tobytes() == g.SH.tobytes() and _floats(o["scores"][1]).tobytes() == g.SF.tobytes()
    assert _floats(o["R21"][0]).tobytes() == g.R21.tobytes() and _floats(o["t21"][0]).tobytes() == g.t21.tobytes()
    assert o["sizes"] == [[str(len(sc.keys1)), str(len(sc.keys1))]]
    assert _floats(o["vP3D"][0]).tobytes() == g.vP3D.tobytes()
    assert np.array_equal(np.array([int(w) for w in o["vbTriangulated"][0]], bool), g.vbTriangulated)
