"""What ba_weld_solve answers without a device: every refusal with its code, and the three solves that run no iteration (the flag up
before the call, no edge, no iteration asked for), which return the input through the float32 conversions with rounds_run == 0."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import weld_ba_cases as wc
import weld_ba_model as wm
from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN = np.iinfo(np.int32).min


def _view(pr, **kw):
    return views.ba_weld_problem(pr["poses"], pr["pose_fixed"], pr["pose_camera"], pr["points"], pr["edges"], pr["cameras"], **kw)


def _solve(p, stop=None, boolean=False, out=None):
    out = views.BaWeldOutput(p.ba.n_poses, p.ba.n_points, p.ba.n_edges) if out is None else out
    lib = capi.load()
    fn = lib.ba_weld_solve_b if boolean else lib.ba_weld_solve
    return fn(C.byref(p), None if stop is None else C.c_void_p(stop.ctypes.data), C.byref(out.w)), out


def test_symbols_and_struct_layout(tmp_path):
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    for s in ("ba_weld_solve", "ba_weld_solve_b", "ba_weld_solve_h", "ba_weld_solve_hb"):
        assert hasattr(lib, s) and s in capi.FULL_BA_SYMBOLS and re.search(r"^int %s\(" % s, hdr, flags=re.M), s
    # the ctypes mirrors against the compiler's layout of the header's structs
    src = tmp_path / "layout.c"
    fields_p = ["struct_size", "ba", "iterations_second", "chi2_mono", "chi2_stereo"]
    fields_r = [f for f, _ in capi.BaWeldResult._fields_]
    body = "".join('printf("%%zu\\n", offsetof(ba_weld_problem, %s));' % f for f in fields_p)
    body += "".join('printf("%%zu\\n", offsetof(ba_weld_result, %s));' % f for f in fields_r)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "orbgpu.h"\nint main(void) { %s printf("%%zu\\n%%zu\\n", sizeof(ba_weld_problem), '
                   'sizeof(ba_weld_result)); return 0; }\n' % body)
    exe = tmp_path / "layout"
    import subprocess
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [getattr(capi.BaWeldProblem, f).offset for f in fields_p] + [getattr(capi.BaWeldResult, f).offset for f in fields_r]
    assert got == want + [C.sizeof(capi.BaWeldProblem), C.sizeof(capi.BaWeldResult)]


def test_refusals_come_before_any_device_work():
    pr = wc.problem("weld_small")
    good, keep = _view(pr)
    assert _solve(good, np.array([1], np.int32))[0] == capi.ORBG_OK          # (the reference for what follows: accepted without a device)
    lib = capi.load()
    out = views.BaWeldOutput(good.ba.n_poses, good.ba.n_points, good.ba.n_edges)
    assert lib.ba_weld_solve(None, None, C.byref(out.w)) == capi.ORBG_BAD_ARG
    assert lib.ba_weld_solve(C.byref(good), None, None) == capi.ORBG_BAD_ARG
    assert lib.ba_weld_solve_h(None, C.byref(good), None, C.byref(out.w)) == capi.ORBG_BAD_ARG
    # a short struct_size, on either side
    p, keep = _view(pr); p.struct_size -= 1
    assert _solve(p)[0] == capi.ORBG_BAD_ARG
    p, keep = _view(pr); p.struct_size = 0
    assert _solve(p)[0] == capi.ORBG_BAD_ARG
    out = views.BaWeldOutput(good.ba.n_poses, good.ba.n_points, good.ba.n_edges); out.w.struct_size -= 1
    assert _solve(good, out=out)[0] == capi.ORBG_BAD_ARG
    # negative counts
    for f in ("n_poses", "n_points", "n_edges", "n_cameras"):
        p, keep = _view(pr); setattr(p.ba, f, -1)
        assert _solve(p, out=views.BaWeldOutput(good.ba.n_poses, good.ba.n_points, good.ba.n_edges))[0] == capi.ORBG_BAD_ARG, f
    # thresholds that are not finite and positive
    for f in ("chi2_mono", "chi2_stereo"):
        for v in (0.0, -5.991, float("nan"), float("inf")):
            p, keep = _view(pr); setattr(p, f, v)
            assert _solve(p)[0] == capi.ORBG_BAD_ARG, (f, v)
    # missing output arrays
    for f in ("poses", "points"):
        out = views.BaWeldOutput(good.ba.n_poses, good.ba.n_points, good.ba.n_edges); setattr(out.c, f, None)
        assert _solve(good, out=out)[0] == capi.ORBG_BAD_ARG, f
    out = views.BaWeldOutput(good.ba.n_poses, good.ba.n_points, good.ba.n_edges); out.w.edge_level = None
    assert _solve(good, out=out)[0] == capi.ORBG_BAD_ARG
    # what ba_solve refuses: an edge of the right camera, observations of a point that are not consecutive, a camera index out of range
    e = pr["edges"].copy(); e["ur"][3] = capi.UR_RIGHT_CAMERA
    assert _solve(_view(dict(pr, edges=e))[0])[0] == capi.ORBG_BAD_ARG
    e = pr["edges"].copy(); e[[0, len(e) - 1]] = e[[len(e) - 1, 0]]
    assert _solve(_view(dict(pr, edges=e))[0])[0] == capi.ORBG_BAD_ARG
    assert _solve(_view(dict(pr, pose_camera=np.full(len(pr["poses"]), 2, np.int32)))[0])[0] == capi.ORBG_BAD_ARG
    n = capi.BA_MAX_FREE_POSES + 1
    poses = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (n, 1))
    p, keep = views.ba_weld_problem(poses, np.zeros(n, np.uint8), np.zeros(n, np.int32), pr["points"], pr["edges"][:0], pr["cameras"])
    assert _solve(p)[0] == capi.ORBG_CAP_EXCEEDED
    # the optional arrays may be missing
    out = views.BaWeldOutput(good.ba.n_poses, good.ba.n_points, good.ba.n_edges)
    out.c.edge_chi2 = None; out.c.edge_depth_pos = None; out.c.point_included = None; out.c.trace = None; out.w.trace_second = None
    assert _solve(good, np.array([1], np.int32), out=out)[0] == capi.ORBG_OK


@pytest.mark.parametrize("form", ["raised", "raised_byte", "after_precheck", "iterations0", "no_edges"])
def test_a_call_without_an_iteration_returns_the_estimate_it_was_given(form):
    pr = wc.problem("weld_small")
    if form == "no_edges":
        pr = dict(pr, edges=pr["edges"][:0])
    p, keep = _view(pr, iterations=0 if form == "iterations0" else 5)
    stop = {"raised": np.array([1], np.int32), "raised_byte": np.array([1], np.uint8), "after_precheck": np.array([INT32_MIN], np.int32)}.get(form)
    rc, out = _solve(p, stop, boolean=form == "raised_byte")
    assert rc == capi.ORBG_OK
    assert out.status == (1 if form in ("raised", "raised_byte") else 0)          # LBA_ABORTED_BEFORE_OPT / LBA_APPLIED
    assert out.rounds_run == 0 and out.iters == 0 and out.iters_second == 0 and out.n_level1 == 0
    assert out.c.trace_len == 0 and out.w.trace_second_len == 0 and out.chi2 == (0.0, 0.0) and out.chi2_second == (0.0, 0.0)
    m = wm.solve(pr, 0, 10)
    assert m.rounds_run == 0
    assert np.abs(out.poses - m.poses).max() <= 1e-6 and np.array_equal(out.points, pr["points"])
    assert np.array_equal(out.edge_depth_pos, m.edge_depth_pos) and not out.edge_chi2.any() and not out.edge_level.any()
    assert np.array_equal(out.point_included, m.point_included)
