"""orbgpu::SearchInNeighbors / orbgpu::Fuse (include/orbgpu_localmapping.hpp): tests/cpp/fuse_glue runs the glue over liborbgpu and the
serial restatement of tests/cpp/fuse_ref.hpp on two copies of the same mock map and prints both maps afterwards.  Everything must be
EQUAL: every keyframe's point table and mnFuseTargetForKF mark, every point's observations, bad flag, replaced pointer, descriptor,
mnFuseCandidateForKF mark and the calls of its per-point members, and the return values."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "fuse_glue")


def _parse(text):
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"\[(.+)\]$", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
        else:
            k, _, v = ln.partition(":")
            cur[k] = v.split()
    return out


@pytest.fixture(scope="module")
def runs():
    assert os.path.exists(EXE), "build() makes tests/cpp/fuse_glue"
    out = {}
    for abort_after in (0, 1, 5):
        r = subprocess.run([EXE, "--gpu", str(abort_after)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out[abort_after] = _parse(r.stdout)
    return out


def _field(words, name):
    return [w for w in words if w.startswith(name + "=")][0].split("=")[1]


@pytest.mark.gpu
@pytest.mark.parametrize("abort_after", [0, 1, 5])
def test_glue_leaves_the_map_the_serial_restatement_leaves(runs, abort_after):
    got = runs[abort_after]
    for scene in ("stereo", "mono_inertial"):
        head, g, f = got[scene], got[scene + ".glue"], got[scene + ".ref"]
        assert head["targets"][0] == head["targets"][1] and head["abort_reads"][0] == head["abort_reads"][1]
        assert g.keys() == f.keys() and len(g) > 100
        for key in g:
            assert g[key] == f[key], (scene, key, g[key], f[key])
        replaced = sum(_field(v, "bad") == "1" for k, v in g.items() if k.startswith("mp"))
        updated = sum(_field(v, "normal") == "1" for k, v in g.items() if k.startswith("mp"))
        marked = sum(_field(v, "target") == "100" for k, v in g.items() if k.startswith("kf"))
        assert marked == int(head["targets"][0])
        assert replaced > (10 if abort_after == 0 else 0)                       # direction one runs whatever the flag says (:922-928)
        # points met again with another descriptor: rescored over the record's list, and world point 0 of the scene -- more
        # candidates than the list holds -- re-evaluated singly
        assert int(_field(head["stats"], "rescored")) > 0 and int(_field(head["stats"], "relaunched")) >= 1
        if abort_after == 0:
            # 4 listed + the second neighbours they name, without the current keyframe and the bad one; the inertial scene adds the
            # three keyframes that hang on the mPrevKF chain only
            assert int(head["targets"][0]) == (8 if scene == "stereo" else 9)
            assert int(head["abort_reads"][0]) == 5 and updated > 50 and _field(g["kf0"], "connections") == "1"
        elif abort_after == 1:
            assert int(head["abort_reads"][0]) == 2                             # the break at :898 after the first target, then the return at :930
            assert updated == 0 and _field(g["kf0"], "connections") == "0"
            assert int(head["targets"][0]) < (8 if scene == "stereo" else 9)
        else:
            assert int(head["abort_reads"][0]) == 5 and updated == 0            # raised only at :930: all targets, no direction two


@pytest.mark.gpu
def test_fuse_on_its_own_and_the_rig_refusal(runs):
    got = runs[0]
    head, g, f = got["fuse"], got["fuse.glue"], got["fuse.ref"]
    assert head["fused"][0] == head["fused"][1] and int(head["fused"][0]) > 20
    assert g == f
    # a rig keyframe among the second neighbours: -1, no upload, no mark, the map as it was built
    assert got["rig"]["returned"] == ["-1"] and got["rig"]["resident"] == ["0"]
    assert got["rig.glue"] == got["rig.ref"]
    assert all(_field(v, "target") == "0" for k, v in got["rig.glue"].items() if k.startswith("kf"))
