"""orbgpu::PoseInertialOptimizationLastKeyFrame / LastFrame (include/orbgpu_inertial.hpp) over the mock Frames of
tests/cpp/mock_inertial.hpp: what the glue collects and what it writes back, without a GPU (the library call replaced by a recorder),
and the real call against the numpy model under the gpu marker."""
import os
import subprocess

import numpy as np
import pytest

import pose_inertial_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
_built = {}
FLOAT_DUMPS = ("Xw", "u", "v", "ur", "inv_sigma2", "cam", "Tcb", "frame", "other", "preint", "C", "Rwb", "twb", "Vw", "bias_g_a")


def _exe(tmp_path_factory, strict):
    if strict not in _built:
        exe = str(tmp_path_factory.mktemp("pi_glue") / ("pose_inertial_glue" + ("_strict" if strict else "")))
        lib_dir = os.path.join(ROOT, "multi_orbslam3_amd")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "pose_inertial_glue.cpp"),
               "-o", exe, "-L", lib_dir, "-lorbgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
        r = subprocess.run(cmd + (["-DMOCK_STRICT_ACCESS"] if strict else []), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        _built[strict] = exe
    return _built[strict]


def _write_input(path, P, two_cam=0, no_cpi=0):
    """The Frame of a model problem, with a feature without a map point in front of every third correspondence."""
    n = P["n"]
    inv8 = np.array([1.0 / 1.2 ** (2 * k) for k in range(8)], np.float32)
    octave = [int(np.argmin(np.abs(inv8 - w))) for w in P["inv_sigma2"]]
    assert np.array_equal(inv8[octave], P["inv_sigma2"])
    rows, feat = [], []
    for i in range(n):
        if i % 3 == 0:
            rows.append([0, 9, 9, 9, 1, 2, 0, -1, 5])
        feat.append(len(rows))
        depth = 5.0 if P["close"][i] else 20.0
        rows.append([1, *P["Xw"][i], P["u"][i], P["v"][i], octave[i], P["ur"][i], depth])
    w = ["%d %d %d %d %d" % (P["form"], P["rec_init"], len(rows), two_cam, no_cpi)]
    w += [" ".join(repr(float(x)) for x in r) for r in rows]
    fl = lambda a: " ".join(repr(float(x)) for x in np.asarray(a).ravel())
    w += [fl(inv8), fl(P["cam"]), fl(np.vstack([P["Tcb"], [[0, 0, 0, 1]]]))]
    for s in (P["frame"], P["other"]):
        w += [fl(s["Rwb"]), fl(s["twb"]), fl(s["vwb"]), fl(s["bg"]), fl(s["ba"])]
    pre = P["preint"]
    w += [fl([pre["dT"]])] + [fl(pre[k]) for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bg", "ba")] + [fl(P["C"])]
    if P["form"] == pm.FORM_FRAME and not no_cpi:
        pr = P["prior"]
        w += [fl(pr[k]) for k in ("Rwb", "twb", "vwb", "bg", "ba", "H")]
    path.write_text("\n".join(w) + "\n")
    return np.array(feat), len(rows)


def _run(exe, mode, path):
    r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for ln in r.stdout.splitlines():
        k, _, v = ln.partition(" ")
        out[k] = v if k == "threw" else np.array([float(x) for x in v.split()])
    for k in FLOAT_DUMPS:                                   # printed with nine digits: exact once read back as float
        if k in out:
            out[k] = out[k].astype(np.float32)
    return out


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("form", [pm.FORM_KF, pm.FORM_FRAME])
def test_collect_and_write_back_over_mock_frames(tmp_path, tmp_path_factory, strict, form):
    exe = _exe(tmp_path_factory, strict)
    P = pm.make_scene(form, 20, 71 + form, kind="mixed", bias_step=1e-3, rec_init=form)
    feat, N = _write_input(tmp_path / "in.txt", P)
    g = _run(exe, "--cpu", tmp_path / "in.txt")
    f32 = lambda a: np.asarray(a, np.float32).ravel()
    # ---- what the glue hands over: bit for bit what the Frame holds
    assert g["head"][1:].tolist() == [form, P["rec_init"], 0, -1, P["n"]]
    for k in ("Xw", "u", "v", "ur", "inv_sigma2"):
        assert np.array_equal(g[k], f32(P[k])), k
    assert np.array_equal(g["close"], P["close"])
    assert np.array_equal(g["cam"], f32(P["cam"])) and np.array_equal(g["Tcb"], f32(P["Tcb"]))
    st = lambda s: np.concatenate([f32(s[k]) for k in ("Rwb", "twb", "vwb", "bg", "ba")])
    assert np.array_equal(g["frame"], st(P["frame"])) and np.array_equal(g["other"], st(P["other"]))
    pre = P["preint"]
    assert np.array_equal(g["preint"], np.concatenate([f32([pre["dT"]])] + [f32(pre[k]) for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bg", "ba")]))
    assert np.array_equal(g["C"], f32(P["C"]))
    i9, ig, ia = pm.imu_information(P["C"])
    assert np.abs(g["info9"].reshape(9, 9) - i9).max() <= 2.0 ** -23 * np.abs(i9).max()
    assert np.abs(g["infoG"].reshape(3, 3) - ig).max() <= 2.0 ** -23 * np.abs(ig).max() and np.abs(g["infoA"].reshape(3, 3) - ia).max() <= 2.0 ** -23 * np.abs(ia).max()
    if form == pm.FORM_FRAME:
        pr = P["prior"]
        assert np.array_equal(g["prior"], np.concatenate([np.asarray(pr[k], np.float64).ravel() for k in ("Rwb", "twb", "vwb", "bg", "ba", "H")]))
    else:
        assert "prior" not in g
    # ---- what it writes back from the recorder's canned result
    assert g["ret"].tolist() == [77]
    want = np.ones(N)                                       # a feature without a map point keeps the flag it had (the mock starts at true)
    want[feat] = (np.arange(P["n"]) % 3 == 0)
    assert np.array_equal(g["mvbOutlier"], want)
    assert np.array_equal(g["Rwb"], f32(0.125 * np.arange(9) + 1e-9)) and np.array_equal(g["twb"], f32(10.0 + np.arange(3) + 1e-9))
    assert np.array_equal(g["Vw"], f32(20.0 + np.arange(3)))
    assert g["bias_g_a"].tolist() == [0.5, 1.5, 2.5, -0.5, -1.5, -2.5]                  # IMU::Bias(ba..., bg...): not swapped
    assert np.array_equal(g["cpi"], 0.125 * np.arange(9) + 1e-9) and np.array_equal(g["cpi_t"], 10.0 + np.arange(3) + 1e-9)   # doubles, not the floats
    assert g["cpi_bg"].tolist() == [0.5, 1.5, 2.5] and g["cpi_ba"].tolist() == [-0.5, -1.5, -2.5]
    Hc = pm.condition_prior((np.arange(225) + 1.0).reshape(15, 15))
    assert np.abs(g["cpi_H"].reshape(15, 15) - Hc).max() <= 1e-10 * np.abs(Hc).max()
    assert g["set_calls"].tolist() == [1] and g["live"].tolist() == [1]
    assert g["prev_cpi_null"].tolist() == [1]


def test_glue_refuses_what_the_entry_point_does_not_support(tmp_path, tmp_path_factory):
    exe = _exe(tmp_path_factory, False)
    P = pm.make_scene(pm.FORM_FRAME, 8, 73)
    _write_input(tmp_path / "a.txt", P, no_cpi=1)
    assert "mpcpi does not exist" in _run(exe, "--cpu", tmp_path / "a.txt")["threw"]
    _write_input(tmp_path / "b.txt", P, two_cam=1)
    assert "two-camera" in _run(exe, "--cpu", tmp_path / "b.txt")["threw"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", [pm.FORM_KF, pm.FORM_FRAME])
def test_glue_call_against_the_model(tmp_path, tmp_path_factory, form):
    """The real call through the glue: flags and count as model (b); the state the Frame holds is the model's rounded to float (one float
    ulp for a double next to a rounding boundary); the new constraint's H within the GPU test's tolerance after the same conditioning."""
    exe = _exe(tmp_path_factory, False)
    P = pm.make_scene(form, 150, 75 + form, kind="mixed", outlier_frac=0.1)
    feat, N = _write_input(tmp_path / "in.txt", P)
    g = _run(exe, "--gpu", tmp_path / "in.txt")
    rb, rr, ra = pm.solve(P, "kernel"), pm.reversed_runs(P), pm.solve(P, "reference")
    assert not pm.near_threshold(rb["decisions"]).any()
    want = np.ones(N)
    want[feat] = rb["outlier"]
    assert np.array_equal(g["mvbOutlier"], want) and g["ret"].tolist() == [rb["n_inliers"]]
    for key, m in (("Rwb", rb["Rwb"]), ("twb", rb["twb"]), ("Vw", rb["vwb"])):
        assert np.abs(g[key] - m.ravel()).max() <= 2.0 ** -23 * max(1.0, np.abs(m).max()), key
    assert np.abs(g["bias_g_a"] - np.concatenate([rb["bg"], rb["ba"]])).max() <= 2.0 ** -23
    y = pm.yardsticks_of(rb, rr, ra)
    Hc = pm.condition_prior(rb["H"])
    assert np.linalg.norm(g["cpi_H"].reshape(15, 15) - Hc) <= (pm.MARGIN * y["fr_H"] + 1e-12) * np.linalg.norm(Hc)
    assert g["prev_cpi_null"].tolist() == [1] and g["live"].tolist() == [1]
