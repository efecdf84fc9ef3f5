"""ORBmatcher::SearchForInitialization on the device (csrc/search_init.hip + csrc/init_replay.hpp) against tests/search_init_model.py.

Everything is integer or float32 arithmetic in a fixed order: matches12, n_matches, prev_matched (by bit), the counters and the
per-query candidate lists -- entry for entry, in order -- must EQUAL the model's, for every case."""
import os
import subprocess

import numpy as np
import pytest

import search_init_model as sm
from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import api, views

pytestmark = pytest.mark.gpu
CAM = (458.0, 457.0, 320.0, 240.0, 40.0, 0.08)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_frame(F, cap=None):
    fv, keep = views.frame_view(F.kps, F.desc, None, None, [float(b) for b in F.bounds], CAM, 8, 1.2)
    return api.Frame(cap_features=max(F.n, 1) if cap is None else cap).upload(fv, keep)


def product(F1, F2, prev, window, nn_ratio=0.9, check_orientation=True, list_capacity=0, frames=None):
    d1, d2 = frames if frames else (device_frame(F1), device_frame(F2))
    n, m12, pv, lists = api.ORBmatcher(nn_ratio, check_orientation).SearchForInitialization(d1, d2, prev, window, debug=True,
                                                                                            list_capacity=list_capacity)
    return dict(lists, nmatches=n, matches12=m12, prev=pv)


def product_case(c, **kw):
    return product(c["F1"], c["F2"], c["prev"], c["window"], c.get("nn_ratio", 0.9), c.get("check_orientation", True), **kw)


def assert_equal(got, want, where=""):
    assert np.array_equal(got["list_start"], want["list_start"]), where
    assert np.array_equal(got["entries"], want["entries"]), where
    assert got["nmatches"] == want["nmatches"], where
    assert np.array_equal(got["matches12"], want["matches12"]), where
    assert got["prev"].tobytes() == np.ascontiguousarray(want["prev"], np.float32).tobytes(), where
    for k in ("n_queries", "n_candidates", "n_evictions", "n_rot_rejected"):
        assert got[k] == want[k], (where, k, got[k], want[k])


@pytest.fixture(scope="module")
def family():
    """The cases and the model's results: computed once, shared, never modified."""
    cs = sm.cases()
    return {name: (c, sm.run_case(c)) for name, c in cs.items()}


NAMES = ["small", "crowded", "ties", "ties_loose", "edges", "levels_f1", "levels_f2", "window10", "big", "no_orientation"]


@pytest.mark.parametrize("name", NAMES)
def test_every_output_and_every_list_equals_the_model(family, name):
    c, want = family[name]
    got = product_case(c)
    assert_equal(got, want, name)
    assert got["n_regrown"] == 0
    if name.startswith("levels"):
        assert got["nmatches"] == 0 and (got["matches12"] == -1).all() and got["prev"].tobytes() == c["prev"].tobytes()


def test_lists_that_do_not_fit_regrow_the_buffer(family):
    c, want = family["crowded"]
    assert want["n_candidates"] > 4096
    got = product_case(c, list_capacity=4096)
    assert got["n_regrown"] >= 1
    assert_equal(got, want, "crowded, list_capacity 4096")
    again = product_case(c)                                  # and the default afterwards
    assert_equal(again, want, "crowded, default capacity")


def test_chain_of_five_calls_on_its_own_outputs():
    c = sm.case_chain()
    d1 = device_frame(c["F1"])

    def step(F1, F2, prev, window):
        return product(F1, F2, prev, window, frames=(d1, device_frame(F2)))
    want = sm.run_chain(c)
    got = sm.run_chain(c, step)
    assert len(got) == 5
    for k, (g, w) in enumerate(zip(got, want)):
        assert_equal(g, w, "chain step %d" % k)
    assert want[-1]["nmatches"] > 20


def test_one_resident_frame_serves_many_calls_and_a_new_content_rebuilds_the_view(family):
    """The level-0 view is kept per frame content: the same frames again give the same answer, and a frame object that is
    uploaded anew (other features, also fewer) is searched with its new content."""
    c, want = family["small"]
    d1, d2 = device_frame(c["F1"], cap=4096), device_frame(c["F2"], cap=4096)
    for _ in range(2):
        assert_equal(product_case(c, frames=(d1, d2)), want, "same frames again")
    c2, want2 = family["edges"]
    fv1, k1 = views.frame_view(c2["F1"].kps, c2["F1"].desc, None, None, [float(b) for b in c2["F1"].bounds], CAM, 8, 1.2)
    fv2, k2 = views.frame_view(c2["F2"].kps, c2["F2"].desc, None, None, [float(b) for b in c2["F2"].bounds], CAM, 8, 1.2)
    d1.upload(fv1, k1); d2.upload(fv2, k2)
    assert_equal(product_case(c2, frames=(d1, d2)), want2, "new content in the same frame objects")


def test_refusals_on_the_device(family):
    c, _ = family["small"]
    d1, d2 = device_frame(c["F1"]), device_frame(c["F2"])
    lib = capi.load()
    import ctypes as C
    prev = np.ascontiguousarray(c["prev"], np.float32).copy()
    m12 = np.zeros(c["F1"].n, np.int32)
    n = C.c_int(0)

    def call(prm, n_prev=c["F1"].n):
        return lib.orbm_search_for_initialization(d1.h, d2.h, prev.ctypes.data, n_prev, C.byref(prm), m12.ctypes.data, C.byref(n), None)
    good = capi.InitSearchParams(C.sizeof(capi.InitSearchParams), 100, 0.9, 1, 0)
    assert call(good) == capi.ORBG_OK
    assert call(good, n_prev=c["F1"].n - 1) == capi.ORBG_BAD_ARG
    assert call(capi.InitSearchParams(C.sizeof(capi.InitSearchParams), 0, 0.9, 1, 0)) == capi.ORBG_BAD_ARG
    assert call(capi.InitSearchParams(C.sizeof(capi.InitSearchParams) - 4, 100, 0.9, 1, 0)) == capi.ORBG_BAD_ARG
    assert call(capi.InitSearchParams(C.sizeof(capi.InitSearchParams), 100, 0.9, 1, -1)) == capi.ORBG_BAD_ARG


def test_frames_left_by_the_monocular_constructor(scene):
    """Two renders of the scene through orbx_frame_mono at 3500 features: the search on the frames the constructor leaves on the
    device equals the model on the downloaded features and the search on the same features uploaded; the matches then go through
    TwoViewReconstruction.  (The initialisation extractor of the reference asks for 5 x nFeatures = 5000; orbx_create accepts at
    most 3500, so this is the largest frame the constructor can leave.  Frames of 4100 uploaded features are the case `big`.)
    One extractor per frame, both kept alive: a frame left by the constructor reads its extractor handle's feature buffers, so a
    second extraction on the same handle would overwrite the first frame's features under it (include/orbgpu.h says so)."""
    p = scene.frame_view_params()
    out = []
    for k in (0, 3):
        L, _, _ = scene.stereo_pair(k)
        ex = api.ORBextractor(3500, 1.2, 8, 20, 7, 640, 480, n_cams=1)
        F = api.Frame(cap_features=8192)
        fv0, keep0 = views.frame_view(np.zeros(1, capi.KEYPOINT_DTYPE), np.zeros((1, 32), np.uint8), None, None, p["bounds"], p["cam"], 8, 1.2)
        n, kps, kun, desc = ex.frame_mono(F, fv0, np.ascontiguousarray(L), None)
        assert n > 1500
        out.append((ex, F, keep0, kun, desc))
    (_, D1, _, k1, c1), (_, D2, _, k2, c2) = out
    M1, M2 = sm.Frame(k1, c1, p["bounds"]), sm.Frame(k2, c2, p["bounds"])
    want = sm.search(M1, M2, M1.pts, 100)
    assert want["nmatches"] >= 50 and want["n_queries"] > 200
    got = product(M1, M2, M1.pts, 100, frames=(D1, D2))
    assert_equal(got, want, "frames of the constructor")
    up = product(M1, M2, M1.pts, 100)
    assert_equal(up, want, "the same features uploaded")
    K = np.array([[p["cam"][0], 0, p["cam"][2]], [0, p["cam"][1], p["cam"][3]], [0, 0, 1]], np.float32)
    r = api.TwoViewReconstruction(K, 1.0, 200).Reconstruct(M1.pts, M2.pts, got["matches12"])
    assert r is not None


@pytest.mark.parametrize("name", ["small", "edges", "big"])
def test_reference_signature_glue_over_mock_frames(family, name, tmp_path):
    """tests/cpp/search_init_glue --gpu: orbgpu::dropin::SearchForInitialization over mock Frames (built with -DMOCK_STRICT_ACCESS)
    equals the serial C++ restatement and the Python API on the same scene."""
    c, want = family[name]
    exe = os.path.join(ROOT, "tests", "cpp", "search_init_glue")
    assert os.path.isfile(exe), "tests/cpp/search_init_glue is not built: run __graft_entry__.build()"
    p = str(tmp_path / "scene.bin")
    sm.write_scene(p, c["F1"], c["F2"], c["prev"], c["window"], c.get("nn_ratio", 0.9), c.get("check_orientation", True))
    out = subprocess.run([exe, "--gpu", p], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "equal 1" in out.stdout, (out.stdout[-500:], out.stderr[-500:])
    glue, ref = sm.parse_program_output(out.stdout, "glue"), sm.parse_program_output(out.stdout, "ref")
    got = product_case(c)
    for r in (glue, ref):
        assert r["nmatches"] == got["nmatches"] == want["nmatches"]
        assert np.array_equal(r["matches12"], got["matches12"]) and r["prev"].tobytes() == got["prev"].tobytes()
