"""The four orbgpu::InertialOptimization overloads (include/orbgpu_inertial.hpp) over the mocks of tests/cpp/mock_inertial_init.hpp, without
a GPU: the library call is replaced by a recorder that prints the problem and returns a canned result, the mocks log every visible effect
in order.  Held for each overload: the switches of the problem (S/Optimizer.cc:5344-5958), the front keyframe's bias, the keyframe and
edge lists under each filter, the SetNewBias(mPrevKF->GetImuBias()) side effect, the order and the values of the write-back with both
sides of the 0.01 branch, the outputs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
_built = {}


def _exe(tmp_path_factory, strict):
    if strict not in _built:
        exe = str(tmp_path_factory.mktemp("ii_glue") / ("inertial_init_glue" + ("_strict" if strict else "")))
        lib_dir = os.path.join(ROOT, "multi_orbslam3_amd")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "inertial_init_glue.cpp"),
               "-o", exe, "-L", lib_dir, "-lorbgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
        r = subprocess.run(cmd + (["-DMOCK_STRICT_ACCESS"] if strict else []), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        _built[strict] = exe
    return _built[strict]


def _run(exe, overload, n, scenario="plain", mono=1, fixed_vel=0, prior_g=100.0):
    r = subprocess.run([exe] + [str(x) for x in (overload, n, scenario, mono, fixed_vel, prior_g)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {"kf": [], "edge": [], "event": [], "after": {}}
    for ln in r.stdout.splitlines():
        k, _, v = ln.partition(" ")
        w = v.split()
        if k == "problem":
            out["problem"] = {"size": int(w[1]), "algorithm": int(w[3]), "iterations": int(w[5]), "lambda": float(w[7]),
                              "free": tuple(int(x) for x in w[9:13]), "priors": (int(w[14]), float(w[15]), float(w[16])), "bg": float(w[18]),
                              "ba": float(w[20]), "scale": float(w[22]), "Rwg": (float(w[24]), float(w[25])), "nk": int(w[27]), "ne": int(w[29])}
        elif k == "kf":
            out["kf"].append({"R0": float(w[2]), "t0": float(w[4]), "v0": float(w[6])})
        elif k == "edge":
            out["edge"].append({"k1": int(w[2]), "k2": int(w[4]), "dT": float(w[6]), "lbg": float(w[8]), "info": float(w[10])})
        elif k == "event":
            out["event"].append(v)
        elif k == "after":
            out["after"][int(w[0])] = {"v": float(w[2]), "bwx": float(w[4]), "bax": float(w[6])}
        elif k == "out":
            out["out"] = {"scale": float(w[1]), "Rwg": (float(w[3]), float(w[4])), "bg": float(w[6]), "ba": float(w[8]), "cov": int(w[10])}
        elif k == "threw":
            out["threw"] = v
    return out


def _ids(out):
    """mnId of the keyframe at each index of the problem: the driver gives keyframe i the rotation entry 0.5 + i and the id 10 + i"""
    return [10 + int(k["R0"] - 0.5) for k in out["kf"]]


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("mono,fixed_vel,prior_g", [(1, 0, 100.0), (0, 0, 100.0), (1, 1, 100.0), (1, 0, 0.0)])
def test_first_overload(tmp_path_factory, strict, mono, fixed_vel, prior_g):
    o = _run(_exe(tmp_path_factory, strict), 1, 5, "plain", mono, fixed_vel, prior_g)
    p = o["problem"]
    assert p["size"] == 1 and p["algorithm"] == 0 and p["iterations"] == 200
    assert p["lambda"] == (1e3 if prior_g != 0 else 0.0)                      # setUserLambdaInit(1e3) iff priorG != 0
    assert p["free"] == (1 - fixed_vel, 1 - fixed_vel, 1, mono)
    assert p["priors"] == (1, prior_g, 1e6)
    assert p["scale"] == 1.25 and p["Rwg"] == (0.75, -0.25)                   # the caller's Rwg and scale
    # every bias vertex is constructed from vpKFs.front(): the map's first keyframe is the newest one here (id 14: 0.005, 0.05)
    assert abs(p["bg"] - 0.005) < 1e-7 and abs(p["ba"] - 0.05) < 1e-7
    assert _ids(o) == [14, 13, 12, 11, 10]
    ids = _ids(o)
    assert [(ids[e["k1"]], ids[e["k2"]]) for e in o["edge"]] == [(13, 14), (12, 13), (11, 12), (10, 11)]
    # each edge carries its own keyframe's preintegration (dT = 0.1 i, b.bwx = 7 + i) and the information of ITS covariance (50 + i)
    for e in o["edge"]:
        i = ids[e["k2"]] - 10
        assert abs(e["dT"] - 0.1 * i) < 1e-6 and e["lbg"] == 7.0 + i and e["info"] == 50.0 + i
    ev = o["event"]
    k = ev.index("solve")
    # the side effect: SetNewBias(mPrevKF->GetImuBias()) on every edge's preintegration, before the solve (bwx of keyframe i is 0.001 (i + 1))
    assert ev[:k] == ["Preintegrated::SetNewBias %d %.6f" % (14 - j, 0.001 * (4 - j)) for j in range(4)]
    # the write-back in list order: SetVelocity, then SetNewBias with IMU::Bias(ba, bg); |bg - old| <= 0.01: no Reintegrate
    want = []
    for j in range(5):
        want += ["SetVelocity %d %.6f" % (14 - j, 100.0 + j), "SetNewBias %d %.6f %.6f" % (14 - j, 0.001, 0.02)]
    assert ev[k + 1:] == want
    assert o["out"] == {"scale": 1.75, "Rwg": (0.1, 0.9), "bg": 0.001, "ba": 0.02, "cov": 0}
    assert o["after"][10]["v"] == 104.0 and abs(o["after"][10]["bax"] - 0.02) < 1e-7


@pytest.mark.parametrize("overload", [2, 3])
def test_bias_only_overloads(tmp_path_factory, overload):
    o = _run(_exe(tmp_path_factory, True), overload, 5)
    p = o["problem"]
    assert p["algorithm"] == 0 and p["iterations"] == 200 and p["lambda"] == 1e3 and p["free"] == (1, 1, 0, 0) and p["priors"] == (1, 100.0, 1e5)
    assert p["scale"] == 1.0 and p["Rwg"] == (1.0, 0.0)                       # VertexGDir(I), VertexScale(1.0), both fixed
    ids = _ids(o)
    assert ids == ([14, 13, 12, 11, 10] if overload == 2 else [10, 11, 12, 13, 14])
    front = ids[0] - 10
    assert abs(p["bg"] - 0.001 * (front + 1)) < 1e-7 and abs(p["ba"] - 0.01 * (front + 1)) < 1e-7
    assert sorted((ids[e["k1"]], ids[e["k2"]]) for e in o["edge"]) == [(10, 11), (11, 12), (12, 13), (13, 14)]
    assert o["out"]["scale"] == 1.25 and o["out"]["Rwg"][0] == 0.75           # not outputs of these overloads
    assert o["out"]["bg"] == 0.001 and o["out"]["ba"] == 0.02
    assert sum(e.startswith("Preintegrated::SetNewBias") for e in o["event"]) == 4
    assert [e.split()[1] for e in o["event"] if e.startswith("SetVelocity")] == [str(i) for i in ids]


def test_fourth_overload_writes_no_keyframe(tmp_path_factory):
    o = _run(_exe(tmp_path_factory, True), 4, 5)
    p = o["problem"]
    assert p["algorithm"] == 1 and p["iterations"] == 10 and p["lambda"] == 0.0 and p["free"] == (0, 0, 1, 1) and p["priors"][0] == 0
    assert p["scale"] == 1.25 and p["Rwg"] == (0.75, -0.25)
    assert abs(p["bg"] - 0.005) < 1e-7                                       # the bias vertices of every keyframe: vpKFs.front()'s
    assert p["ne"] == 4
    assert o["event"] == ["solve"]                                           # no SetNewBias side effect, no write-back
    assert o["out"]["scale"] == 1.75 and o["out"]["Rwg"] == (0.1, 0.9)
    assert all(o["after"][10 + i]["v"] == 2.5 + i for i in range(5))


@pytest.mark.parametrize("overload", [1, 2, 4])
def test_keyframes_beyond_max_id_are_left_out(tmp_path_factory, overload):
    o = _run(_exe(tmp_path_factory, True), overload, 5, "beyond")
    ids = _ids(o)
    assert ids == [12, 11, 10]
    assert sorted((ids[e["k1"]], ids[e["k2"]]) for e in o["edge"]) == [(10, 11), (11, 12)]
    assert abs(o["problem"]["bg"] - 0.005) < 1e-7                             # ... but front() is front(), beyond maxKFid or not
    assert not any(e.split()[1] in ("13", "14") for e in o["event"] if e != "solve")
    assert o["after"][13]["v"] == 5.5 and o["after"][14]["v"] == 6.5


def test_list_overload_keeps_the_vertices_beyond_max_id(tmp_path_factory):
    """S/Optimizer.cc:5719-5720: the filter on the vertices is commented out; the edges and the write-back still have theirs"""
    o = _run(_exe(tmp_path_factory, True), 3, 5, "beyond")
    ids = _ids(o)
    assert ids == [10, 11, 12, 13, 14]
    assert sorted((ids[e["k1"]], ids[e["k2"]]) for e in o["edge"]) == [(10, 11), (11, 12)]
    assert [e.split()[1] for e in o["event"] if e.startswith("SetVelocity")] == ["10", "11", "12"]


@pytest.mark.parametrize("overload", [1, 2, 3, 4])
def test_bad_keyframe_has_no_edge(tmp_path_factory, overload):
    o = _run(_exe(tmp_path_factory, True), overload, 5, "bad")
    ids = _ids(o)
    assert sorted((ids[e["k1"]], ids[e["k2"]]) for e in o["edge"]) == [(10, 11), (12, 13), (13, 14)]      # 12 isBad(): no edge INTO it
    assert not any(e.startswith("Preintegrated::SetNewBias 12") for e in o["event"])
    if overload != 4:
        assert "SetVelocity 12 " in " ".join(o["event"]) + " "                # its velocity vertex exists and is written back


@pytest.mark.parametrize("overload", [1, 3])
def test_predecessor_that_is_not_listed(tmp_path_factory, overload):
    """the edge is skipped because a vertex is missing (:5454, :5791) -- AFTER its preintegration got the predecessor's bias"""
    o = _run(_exe(tmp_path_factory, True), overload, 5, "missing")
    ids = _ids(o)
    assert sorted(ids) == [10, 11, 13, 14]
    assert sorted((ids[e["k1"]], ids[e["k2"]]) for e in o["edge"]) == [(10, 11), (13, 14)]
    assert "Preintegrated::SetNewBias 13 0.003000" in o["event"]
    assert o["after"][12]["v"] == 4.5


@pytest.mark.parametrize("overload", [1, 2, 3])
def test_reintegrate_when_the_gyro_bias_moved(tmp_path_factory, overload):
    o = _run(_exe(tmp_path_factory, True), overload, 4, "far")
    ev = o["event"][o["event"].index("solve") + 1:]
    ids = _ids(o)
    want = []
    for j, i in enumerate(ids):
        want += ["SetVelocity %d %.6f" % (i, 100.0 + j), "SetNewBias %d %.6f %.6f" % (i, 0.5, 0.02)]
        if i != 10:                                                           # keyframe 10 has no preintegration
            want.append("Reintegrate %d" % i)
    assert ev == want
