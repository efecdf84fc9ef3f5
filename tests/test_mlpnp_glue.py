"""orbgpu::MLPnPsolver (include/orbgpu_dropin.hpp) over mock Frame / MapPoint objects: the constructor half and the library's host path
without a GPU, and the --gpu run against the Python solver on the dumped problem and draws, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import mlpnp_model as mm
from multi_orbslam3_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "glue_mlpnp_check")


def _parse(text):
    out, cur = {}, None
    for ln in text.splitlines():
        if ln.startswith("["):
            cur = out.setdefault(ln.strip("[]"), {})
        elif ":" in ln:
            k, v = ln.split(":", 1)
            cur.setdefault(k, []).append(v.split())
    return out


def _floats(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


def _ints(words):
    return np.array([int(w) for w in words], np.int64)


@pytest.mark.parametrize("strict", [False, True])
def test_glue_collect_and_host_path_over_mock_frames(tmp_path, strict):
    exe = str(tmp_path / "glue_mlpnp_check")
    lib_dir = os.path.join(ROOT, "multi_orbslam3_amd")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", CPP,
           os.path.join(CPP, "glue_mlpnp_check.cpp"), "-o", exe, "-pthread", "-L", lib_dir, "-lorbgpu", "-Wl,-rpath," + lib_dir,
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"] + (["-DMOCK_STRICT_ACCESS"] if strict else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = _parse(r.stdout)
    g = got["collect"]
    # eight matches over six keypoints: 1 has no point (:68), 3 a bad one (:69), 6 and 7 lie beyond mvKeysUn (:70)
    assert _ints(g["m"][0]).tolist() == [8] and _ints(g["kp_index"][0]).tolist() == [0, 2, 4, 5]
    assert _floats(g["P2D"][0]).tolist() == [320.0, 240.0, 420.0, 160.0, 520.0, 80.0, 570.0, 40.0]
    sf = np.float32(1.0)
    sig = [np.float32(1.0)]
    for _ in range(7):
        sf = sf * np.float32(1.2)
        sig.append(sf * sf)
    assert np.array_equal(_floats(g["sigma2"][0]), np.array([sig[0], sig[2], sig[0], sig[7]], np.float32))
    # unproject: ((x - 320) / 500, (y - 240) / 400, 1), divided by z = 1: NOT unit length
    want = np.array([[0, 0, 1], [np.float32(100) / np.float32(500), np.float32(-80) / np.float32(400), 1],
                     [np.float32(200) / np.float32(500), np.float32(-160) / np.float32(400), 1], [0.5, -0.5, 1]], np.float32)
    assert np.array_equal(_floats(g["bearing"][0]).reshape(-1, 3), want)
    assert _floats(g["P3Dw"][0]).reshape(-1, 3).tolist() == [[0, 0, 4], [1, -0.5, 6], [2, -1, 8], [2.5, -1.25, 9]]
    assert _floats(g["k"][0]).tolist() == [500.0, 400.0, 320.0, 240.0] and _ints(g["model"][0]).tolist() == [0]
    # the library's host path, from C++: SetRansacParameters' formula and the minimal sets
    h = got["host"]
    for row in h["n_its_min"]:
        n, its, mi = _ints(row).tolist()
        assert (its, mi) == mm.ransac_iterations(n, 0.99, 10, 300, 6, 0.5)[:2]
    d = np.array([[6, 0, 4, 0, 2, 0], [0, 0, 0, 0, 0, 0]], np.int32)
    assert np.array_equal(_ints(h["idx"][0]).reshape(2, 6), mm.resolve_draws(7, d))
    assert _ints(h["bad_draw_rc"][0]).tolist() == [-2]


@pytest.mark.gpu
def test_glue_solver_equals_the_python_solver_bit_for_bit():
    assert os.path.exists(EXE), "build() makes tests/cpp/glue_mlpnp_check"
    r = subprocess.run([EXE, "--gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = _parse(r.stdout)
    p, o = got["problem"], got["outcome"]
    prob = api.MLPnPProblem(_floats(p["P2D"][0]).reshape(-1, 2), _floats(p["sigma2"][0]), _floats(p["bearing"][0]).reshape(-1, 3),
                            _floats(p["P3Dw"][0]).reshape(-1, 3), _floats(p["k"][0]), _ints(p["kp_index"][0]).astype(np.int32), int(p["m"][0][0]))
    assert prob.m == 140 and 100 < prob.n < 140
    draws = _ints(o["draws"][0]).astype(np.int32).reshape(-1, 6)
    s = api.MLPnPsolver(prob)
    s.SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991)
    k0 = 0
    returned = 0
    for call in range(3):
        nd, no_more, ret, n_inl = _ints(o["call%d_draws_nomore_returned_ninliers" % call][0]).tolist()
        k = s.iterations_of_call(5)
        assert nd == 6 * k, call
        it = s.iterate(5, draws[k0:k0 + k])
        k0 += k
        assert (int(it.bNoMore), int(it.returned), it.nInliers) == (no_more, ret, n_inl), call
        vb = _ints(o["call%d_vbInliers" % call][0]).astype(bool)
        if ret:
            assert np.array_equal(vb, it.vbInliers) and vb.sum() == n_inl
            assert _floats(o["call%d_Tcw" % call][0]).tobytes() == it.Tcw.tobytes()
            returned += 1
        else:
            assert len(vb) == 0                   # vbInliers.clear() (:101) and nothing else
    assert k0 == len(draws) and returned >= 1
    s.close()
