"""orbgpu::CreateNewMapPoints (include/orbgpu_localmapping.hpp): tests/cpp/new_points_glue runs the glue over liborbgpu and the serial
restatement of tests/cpp/new_points_ref.hpp on two copies of the same mock map and prints what each created.  Observations, the order
of creation, what the keyframes hold afterwards and the calls of the per-point members must be equal; positions of UnprojectStereo
points are equal to the bit, triangulated positions agree to 1e-4 of the point's distance (the restatement's SVD is a float32 Jacobi
iteration, the library's null vector is formed in float64: 25 x the 4e-6 the float32 model measures on these baselines)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "new_points_glue")


def _parse(text):
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"\[(.+)\]$", ln)
        if m:
            cur = out.setdefault(m.group(1), {"point": []})
        elif ln.startswith("point:"):
            cur["point"].append(ln.split()[1:])
        else:
            k, _, v = ln.partition(":")
            cur[k] = v.split()
    return out


def _xyz(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32).astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("stop_after", [0, 3])
def test_glue_creates_what_the_serial_restatement_creates(stop_after):
    assert os.path.exists(EXE), "build() makes tests/cpp/new_points_glue"
    r = subprocess.run([EXE, "--gpu", str(stop_after)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = _parse(r.stdout)
    for scene, n_kfs in (("stereo", 7), ("mono_inertial", 8)):
        head, g, f = got[scene], got[scene + ".glue"], got[scene + ".ref"]
        made = [int(v) for v in head["made"]]
        assert made[0] == made[1] == len(g["point"]) == len(f["point"])
        assert head["check_calls"][0] == head["check_calls"][1]
        assert made[0] > (30 if scene == "stereo" else 10)
        if stop_after:
            assert int(head["check_calls"][0]) == stop_after
        kf2_seen = set()
        for pg, pf in zip(g["point"], f["point"]):
            assert pg[:3] == pf[:3] and pg[6:] == pf[6:] == ["1", "1", "2", "1"]         # kf2 idx1 idx2 | the per-point calls, 2 observations, pRefKF
            kf2_seen.add(int(pg[0]))
            xg, xf = _xyz(pg[3:6]), _xyz(pf[3:6])
            assert np.linalg.norm(xg - xf) <= 1e-4 * np.linalg.norm(xf) + 1e-12
        for k in range(n_kfs):
            assert g["kf%d" % k] == f["kf%d" % k]
        if not stop_after:
            assert len(kf2_seen) >= 3
            # the neighbours the baseline gates leave out created nothing (kf 2 in the stereo scene, kf 3 in the monocular one)
            assert (2 if scene == "stereo" else 3) not in kf2_seen
        if scene == "mono_inertial" and not stop_after:
            assert int(head["check_calls"][0]) == 6                                      # 5 listed + 2 through mPrevKF = 7 neighbours
        assert got[scene + ".rig"]["made"] == ["-1", "0", "0"]
