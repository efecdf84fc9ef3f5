"""orbgpu::loopclosing::OptimizeEssentialGraph (include/orbgpu_loopclosing.hpp): tests/cpp/essential_graph_glue.cpp runs it over mock
keyframes, map points and a map (tests/cpp/mock_essential_graph.hpp) built from a scene of tests/essential_graph_model.py, with a
recording solver.  The problem handed to eg_solve must equal the Python restatement of the loop form's collection field by field --
minFeat, the parent / child / loop-edge exclusions, sInsertedEdges, NonCorrectedSim3 on either end, a bad keyframe, mnCorrectedByKF --
and the write-back must equal what the recorded answer implies.  No device is needed.  (tools/essential_graph_sanitize.sh builds the
same stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer and runs it on the CPU.)"""
import os
import subprocess

import numpy as np
import pytest

import essential_graph_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def write_scene(sc, path):
    """the scene dictionary as the whitespace-separated file tests/cpp/essential_graph_glue.cpp reads"""
    kfs = sc["kfs"]
    g = lambda v: "%.17g" % float(v)
    out = ["%d %d %d %d %d" % (len(kfs), sc["cur"], sc["loop"], sc["init_kf_id"], int(sc["fix_scale"]))]
    for k in kfs:
        row = [k["mnId"], k["uid"], int(k["bad"]), -1 if k["parent"] is None else k["parent"]]
        row += [g(v) for v in np.asarray(k["R"], np.float32).reshape(-1)] + [g(v) for v in np.asarray(k["t"], np.float32)]
        row += [len(k["children"])] + sorted(k["children"]) + [len(k["loop_edges"])] + sorted(k["loop_edges"])
        row += [len(k["covis"])] + [v for c in k["covis"] for v in c]
        out.append(" ".join(str(v) for v in row))
    for m in (sc["corrected"], sc["noncorrected"]):
        out.append(str(len(m)))
        for i in sorted(m):
            q, t, s = m[i]
            out.append(" ".join([str(i)] + [g(v) for v in q] + [g(v) for v in t] + [g(s)]))
    out.append(str(len(sc["loop_connections"])))
    for i in sorted(sc["loop_connections"]):
        c = sorted(sc["loop_connections"][i])
        out.append(" ".join(str(v) for v in [i, len(c)] + c))
    n = len(kfs)
    pairs = [(a, b, sc["weight"](a, b)) for a in range(n) for b in range(a + 1, n) if sc["weight"](a, b) > 0]
    out.append(str(len(pairs)))
    out += ["%d %d %d" % p for p in pairs]
    out.append(str(len(sc["points"])))
    for mp in sc["points"]:
        by = mp["corrected_by"] if mp["corrected_by"] >= 0 else 2 ** 40
        out.append(" ".join(str(v) for v in [int(mp["bad"])] + [g(v) for v in mp["pos"]] + [mp["ref_kf"], by, max(mp["corrected_ref"], 0)]))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def build(out, extra=()):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", *extra, "-I", os.path.join(ROOT, "include"),
                           "-I", CPP, os.path.join(CPP, "essential_graph_glue.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("eg_glue") / "essential_graph_glue"))


def run_glue(exe, sc, path):
    write_scene(sc, path)
    p = subprocess.run([exe, path], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
    rec = {}
    for line in p.stdout.splitlines():
        w = line.split()
        rec.setdefault(w[0], []).append(w[1:])
    return rec


# a different bad keyframe per scene: one in the middle of the chain, one among the corrected keyframes that a loop edge names, none
SCENES = [dict(n_kf=14, fix_scale=False, seed=7, bad=(5,)), dict(n_kf=16, fix_scale=True, seed=9, bad=(13,), n_corrected=4),
          dict(n_kf=9, fix_scale=True, seed=4, bad=())]


@pytest.mark.parametrize("spec", SCENES, ids=lambda s: "kf%d_bad%s" % (s["n_kf"], "_".join(map(str, s["bad"])) or "none"))
def test_glue_hands_over_the_python_collection_and_writes_back(exe, tmp_path, spec):
    sc = em.make_scene(**spec)
    if spec["bad"] == (13,):
        sc["kfs"][13]["loop_edges"].add(2); sc["kfs"][2]["loop_edges"].add(13)       # a loop edge to a bad keyframe
    col = em.collect_loop_form(sc)
    rec = run_glue(exe, sc, str(tmp_path / "scene.txt"))
    V, E, P = col["vertices"], col["edges"], col["points"]
    head = rec["problem"][0]
    assert [int(v) for v in head[:4]] == [len(V), len(E), len(P), 20] and float(head[4]) == 1e-16 and head[-1] == "1"
    assert len(E) > len(V) and {"loop_connection", "spanning_tree", "covisibility"} <= set(col["kinds"])
    # the problem, field by field: equal doubles (both sides evaluate the same statements in the same order)
    for got, (q, t, s, fixed, fix_scale) in zip(rec["v"], V):
        assert [float(v) for v in got[:8]] == [float(v) for v in list(q) + list(t) + [s]]
        assert [int(got[8]), int(got[9])] == [int(fixed), int(fix_scale)]
    for got, (vi, vj, q, t, s) in zip(rec["e"], E):
        assert [int(got[0]), int(got[1])] == [vi, vj]
        assert [float(v) for v in got[2:]] == [float(v) for v in list(q) + list(t) + [s]]
    for got, (pos, ref) in zip(rec.get("p", []), P):
        assert [np.float32(v) for v in got[:3]] == list(np.asarray(pos, np.float32)) and int(got[3]) == ref
    assert len(rec["v"]) == len(V) and len(rec["e"]) == len(E) and len(rec.get("p", [])) == len(P)
    n_bad = len(spec["bad"])
    rep = rec["report"][0]
    assert [int(v) for v in rep[:6]] == [len(V), len(E), len(P), col["dropped_edges"], n_bad, 7]
    assert (col["dropped_edges"] > 0) == (n_bad > 0)
    if n_bad:
        assert any(r == -1 for _, r in P)                                             # a point whose reference keyframe has no vertex
    assert any(mp["corrected_by"] >= 0 for mp in sc["points"])
    # the write-back: SetPose([R | t * (1. / s)], true) from the recorded answer, skipped for a keyframe without a vertex
    index_of = {uid: n for n, uid in enumerate(col["uids"])}
    for i, (k, got) in enumerate(zip(sc["kfs"], rec["kf"])):
        n_set, n_locked, rows, cols = [int(v) for v in got[1:5]]
        T = np.array([np.float32(v) for v in got[5:]], np.float32).reshape(4, 4)
        if k["bad"]:
            assert n_set == 0
            assert np.array_equal(T[:3, :3], np.asarray(k["R"], np.float32)) and np.array_equal(T[:3, 3], np.asarray(k["t"], np.float32))
            continue
        n = index_of[k["uid"]]
        q, t, s = V[n][0], V[n][1], V[n][2]
        t_new = [np.float64(t[0]) + 0.5 * (n + 1), np.float64(t[1]) - 0.25 * (n + 1), np.float64(t[2]) + 1.0 * (n + 1)]
        inv_s = 1. / (np.float64(s) * 1.25)
        R = np.array(em.quat_to_R([np.float64(v) for v in q]), np.float64)
        want = np.eye(4, dtype=np.float32)
        want[:3, :3] = R.astype(np.float32)
        want[:3, 3] = np.array([v * inv_s for v in t_new], np.float64).astype(np.float32)
        assert (n_set, n_locked, rows, cols) == (1, 1, 4, 4)
        assert np.array_equal(T, want), (i, T, want)
    good_points = [mp for mp in sc["points"] if not mp["bad"]]
    it = iter(P)
    for mp, got in zip(sc["points"], rec["mp"]):
        n_set, n_locked, n_normal = [int(v) for v in got[1:4]]
        pos = np.array([np.float32(v) for v in got[4:7]], np.float32)
        if mp["bad"]:
            assert (n_set, n_normal) == (0, 0) and np.array_equal(pos, mp["pos"])
            continue
        _, ref = next(it)
        assert (n_set, n_locked, n_normal) == (1, 1, 1)
        assert np.array_equal(pos, mp["pos"] + np.float32(0.5) if ref >= 0 else mp["pos"])
    assert len(good_points) == len(P)
    assert rec["map"][0] == ["1", "1", "1", "0"]          # IncreaseChangeIndex once, under mMutexMapUpdate, released afterwards
    assert rec["inertial"][0] == ["1", "0", "0"]          # D-2: thrown, nothing written, the solver not called
