"""orbgpu::LocalInertialBA (include/orbgpu_inertial.hpp) over the mock KeyFrames, MapPoints and Map of tests/cpp/mock_inertial_ba.hpp,
without a GPU: the library call is replaced by a recorder that dumps the problem and returns a canned result (and, on demand, the fail
predicate), the mocks log every visible effect in order.  What is held: the window and both branches of S/Optimizer.cc:4611-4622, the
200-keyframe cap, the SetNewBias side effect, the erase order, the fail return that leaves the stamps and the map untouched, and the
order and the values of the write-back."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
_built = {}


def _exe(tmp_path_factory, strict):
    if strict not in _built:
        exe = str(tmp_path_factory.mktemp("iba_glue") / ("inertial_ba_glue" + ("_strict" if strict else "")))
        lib_dir = os.path.join(ROOT, "multi_orbslam3_amd")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "inertial_ba_glue.cpp"),
               "-o", exe, "-L", lib_dir, "-lorbgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
        r = subprocess.run(cmd + (["-DMOCK_STRICT_ACCESS"] if strict else []), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        _built[strict] = exe
    return _built[strict]


def _run(exe, chain, in_map, extras=0, failed=0, large=0, rec_init=0, no_imu=-1, odd=0):
    r = subprocess.run([exe] + [str(x) for x in (chain, in_map, extras, failed, large, rec_init, no_imu, odd)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {"kf": [], "pt": [], "edge": [], "event": [], "stamp_kf": {}, "stamp_pt": {}}
    for ln in r.stdout.splitlines():
        k, _, v = ln.partition(" ")
        w = v.split()
        if k == "kf":
            out["kf"].append({w[i]: float(w[i + 1]) for i in range(1, 21, 2)} | {"info": [float(x) for x in w[22:25]]})
        elif k == "pt":
            out["pt"].append((float(w[1]), int(w[2])))
        elif k == "edge":
            out["edge"].append({w[i]: float(w[i + 1]) for i in range(1, 13, 2)})
        elif k == "event":
            out["event"].append(v)
        elif k == "stamp_kf":
            out["stamp_kf"][int(w[0])] = dict(local=int(w[1]), fixed=int(w[2]), v=float(w[4]), bwx=float(w[6]), bax=float(w[7]), T0=float(w[9]), T3=float(w[10]))
        elif k == "stamp_pt":
            out["stamp_pt"][int(w[0])] = dict(local=int(w[1]), pos=float(w[3]))
        else:
            out[k] = w
    return out


@pytest.mark.parametrize("strict", [False, True])
def test_window_with_a_fixed_predecessor_and_the_write_back(tmp_path_factory, strict):
    g = _run(_exe(tmp_path_factory, strict), chain=14, in_map=30, extras=2)
    assert g["head"] == ["1", "13", "11", str(len(g["edge"])), "0", "0", "0"]       # points 3 .. 11 and the observers' two: seen from the window
    assert g["cam"] == ["458", "457", "367", "248", "47.9000015"] and g["Tcb"] == "1 0 0 0.25 0 1 0 0 0 0 1 0".split()
    kf = g["kf"]
    # Nd = min(30 - 2, 10): pKF (id 14) and nine of its predecessors, newest first; then the keyframe in front (id 4), fixed with its
    # velocity and biases; then the two other observers (the mock gives them no IMU: fixed poses only)
    assert [k["twb0"] for k in kf] == [14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 1001, 1002]
    assert [k["fixed"] for k in kf] == [0] * 10 + [1] * 3 and [k["imu"] for k in kf] == [1] * 11 + [0, 0]
    assert [k["link"] for k in kf] == [1] * 10 + [0] * 3 and [k["prev"] for k in kf[:10]] == list(range(1, 11))
    assert [k["last"] for k in kf] == [0] * 9 + [1] + [0] * 3                       # i == N - 1: the edge to the fixed keyframe
    for i, k in enumerate(kf[:11]):
        kid = 14 - i
        assert (k["vwb0"], k["bg0"], k["ba0"]) == (kid + 0.5, kid + 0.25, -kid)     # GetGyroBias / GetAccBias: not swapped
    for i, k in enumerate(kf[:10]):
        kid = 14 - i
        assert abs(k["dT"] - 0.01 * kid) < 1e-7 and k["info"] == [kid, kid + 100, kid + 200]      # its own preintegration and covariance
    # the SetNewBias side effect: every linked keyframe's preintegration gets its predecessor's bias, before the solve
    ev = g["event"]
    n_pre = 10
    assert ev[:n_pre] == ["Preintegrated::SetNewBias %d %.6f" % (14 - i, 13 - i + 0.25) for i in range(10)]
    assert ev[n_pre:n_pre + 2] == ["solve", "lock"] and ev[-1] == "unlock"
    # edges: grouped per point in the order of the point list, the list in the order the window's keyframes hold the points
    assert [e["pt"] for e in g["edge"]] == sorted(e["pt"] for e in g["edge"])
    assert [p[0] for p in g["pt"]][:2] == [112.0, 113.0]                            # pKF's own points first
    assert all(e["w"] == [1.0, 0.5, 0.25][int(round(e["v"] - 1000)) % 3] for e in g["edge"])      # mvInvLevelSigma2[octave]
    stereo = [k for k, e in enumerate(g["edge"]) if e["ur"] >= 0]
    assert len(stereo) == 2 and all(g["edge"][k]["ur"] == g["edge"][k]["u"] - 3 for k in stereo)
    # the erase list: the recorder flags every third edge; mono edges in edge order first, then the stereo ones
    erase = [e for e in ev if e.startswith("Erase")]
    flagged = [k for k in range(len(g["edge"])) if k % 3 == 0]
    ids = lambda k: (int(kf[int(g["edge"][k]["kf"])]["twb0"]), int(g["pt"][int(g["edge"][k]["pt"])][0]) - 100)
    want = [ids(k) for k in flagged if k not in stereo] + [ids(k) for k in flagged if k in stereo]
    assert erase == [s for a, b in want for s in ("EraseMapPointMatch %d %d" % (a, b), "EraseObservation %d %d" % (a, b))]
    assert any(k in stereo for k in flagged)
    # the write-back, in the reference's order
    after = ev[n_pre + 2 + len(erase):-1]
    want = [s % (14 - i) for i in range(10) for s in ("SetVelocity %d", "SetNewBias %d", "SetPose %d")]
    pts = [int(p[0]) - 100 for p in g["pt"]]
    want += [s % l for l in pts for s in ("SetWorldPos %d", "UpdateNormalAndDepth %d")] + ["IncreaseChangeIndex"]
    assert after == want
    for i in range(10):
        s = g["stamp_kf"][14 - i]
        assert (s["local"], s["fixed"]) == (0, 0)
        assert (s["v"], s["bwx"], s["bax"]) == (20 + i, 0.5 + i, -0.5 - i)          # IMU::Bias(b[3], b[4], b[5], b[0], b[1], b[2])
        assert (s["T0"], s["T3"]) == (1.0, -(10 + i) + 0.25)                          # Rcw = Rcb Rwb^T, tcw = Rcb (-Rwb^T twb) + tcb
    for kid in (4, 1001, 1002):
        assert g["stamp_kf"][kid]["fixed"] == 0 and g["stamp_kf"][kid]["v"] in (4.5, kid + 0.5)
    for l in pts:
        assert g["stamp_pt"][l] == dict(local=14, pos=100.0 + l + 1)                 # (the reference never resets a point's stamp)
    assert all(g["stamp_pt"][l]["local"] == 0 for l in g["stamp_pt"] if l not in pts)


def test_oldest_keyframe_without_predecessor_becomes_the_fixed_one(tmp_path_factory):
    g = _run(_exe(tmp_path_factory, False), chain=4, in_map=30)
    kf = g["kf"]
    assert [k["twb0"] for k in kf] == [4, 3, 2, 1] and [k["fixed"] for k in kf] == [0, 0, 0, 1] and kf[3]["imu"] == 1
    assert [k["link"] for k in kf] == [1, 1, 1, 0] and [k["prev"] for k in kf[:3]] == [1, 2, 3] and [k["last"] for k in kf] == [0, 0, 1, 0]
    assert g["stamp_kf"][1] == dict(local=0, fixed=0, v=1.5, bwx=1.25, bax=-1.0, T0=0.0, T3=0.0)          # popped: fixed, never written
    assert "SetPose 1" not in g["event"] and "SetPose 2" in g["event"]


def test_window_sizes(tmp_path_factory):
    exe = _exe(tmp_path_factory, False)
    free = lambda g: sum(1 for k in g["kf"] if not k["fixed"])
    assert free(_run(exe, chain=14, in_map=5)) == 3                                  # KeyFramesInMap - 2
    assert free(_run(exe, chain=30, in_map=40)) == 10
    g = _run(exe, chain=30, in_map=40, large=1, rec_init=1)
    assert free(g) == 25 and g["head"][4:6] == ["1", "1"]


def test_fixed_list_stops_at_200_keyframes(tmp_path_factory):
    g = _run(_exe(tmp_path_factory, False), chain=14, in_map=30, extras=250)
    kf = g["kf"]
    assert len(kf) == 10 + 200 and [k["twb0"] for k in kf[10:]] == [4] + list(range(1001, 1200))
    assert g["stamp_kf"][1199]["fixed"] == 0 and g["stamp_kf"][1200]["fixed"] == 0
    assert "threw" not in g
    used = {int(e["kf"]) for e in g["edge"]}
    assert max(used) == len(kf) - 1                                                  # no edge of a keyframe beyond the cap


def test_fail_return_leaves_the_stamps_and_the_map_untouched(tmp_path_factory):
    g = _run(_exe(tmp_path_factory, False), chain=14, in_map=30, extras=2, failed=1)
    ev = g["event"]
    assert ev[-3:] == ["solve", "lock", "unlock"] and all(e.startswith("Preintegrated::SetNewBias") for e in ev[:-3])
    for i in range(10):
        kid = 14 - i
        assert g["stamp_kf"][kid] == dict(local=14, fixed=0, v=kid + 0.5, bwx=kid + 0.25, bax=-float(kid), T0=0.0, T3=0.0)
    assert g["stamp_kf"][4]["fixed"] == 14 and g["stamp_kf"][1001]["fixed"] == 14    # (:5128 returns before :5154 resets them)
    assert all(p["pos"] == 100.0 + l for l, p in g["stamp_pt"].items())


def test_keyframe_without_imu_breaks_the_chain(tmp_path_factory):
    g = _run(_exe(tmp_path_factory, False), chain=14, in_map=30, no_imu=12)
    kf = g["kf"]
    assert [k["imu"] for k in kf[:4]] == [1, 1, 0, 1] and [k["link"] for k in kf[:4]] == [1, 0, 0, 1]
    assert kf[2]["vwb0"] == 0 and kf[2]["twb0"] == 12                                # no velocity or bias is read of it
    pre = [e for e in g["event"] if e.startswith("Preintegrated")]
    assert [int(e.split()[1]) for e in pre] == [14, 11, 10, 9, 8, 7, 6, 5]
    assert "SetVelocity 12" not in g["event"] and "SetNewBias 12" not in g["event"] and "SetPose 12" in g["event"]


def test_bad_and_foreign_observers_bad_points_and_missing_indices_are_skipped(tmp_path_factory):
    """S/Optimizer.cc:4600 (a bad point is no local point), :4666-4673 (a bad observer is stamped but not listed), :4942 (an observer of
    another map is listed, fixed, but gets no edge), :4950 / :4988 (an observation without a left index gives no edge)"""
    exe = _exe(tmp_path_factory, False)
    base = _run(exe, chain=14, in_map=30, extras=2)
    ids = lambda g: [int(k["twb0"]) for k in g["kf"]]
    pts = lambda g: [int(p[0]) - 100 for p in g["pt"]]
    edges = lambda g: {(ids(g)[int(e["kf"])], pts(g)[int(e["pt"])]) for e in g["edge"]}
    g = _run(exe, chain=14, in_map=30, extras=2, odd=1)
    assert 5 in pts(base) and 5 not in pts(g) and len(pts(g)) == len(pts(base)) - 1 and g["stamp_pt"][5]["local"] == 0
    assert "SetWorldPos 5" not in g["event"]
    g = _run(exe, chain=14, in_map=30, extras=2, odd=2, failed=1)                     # (failed: the stamps stay readable)
    assert 1001 not in ids(g) and 1002 in ids(g) and g["stamp_kf"][1001]["fixed"] == 14
    assert not any(k == 1001 for k, _ in edges(g))                                   # stamped, so :4939 passes, but isBad() at :4942
    g = _run(exe, chain=14, in_map=30, extras=2, odd=4)
    assert 1002 in ids(g) and not any(k == 1002 for k, _ in edges(g)) and any(k == 1002 for k, _ in edges(base))
    g = _run(exe, chain=14, in_map=30, extras=2, odd=8)
    assert (14, 12) in edges(base) and (14, 12) not in edges(g) and (1001, 12) in edges(g) and 12 in pts(g)


def test_second_camera_is_refused(tmp_path_factory):
    g = _run(_exe(tmp_path_factory, False), chain=14, in_map=30, extras=2, odd=16)
    assert "two-camera" in " ".join(g["threw"]) and "solve" not in g["event"]
