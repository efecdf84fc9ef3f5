"""CPU-side checks of the drop-in boundary: the HIP library loads, exports every symbol include/orbgpu.h declares,
and fails loudly (ORBG_NO_DEVICE) instead of falling back when no GPU is present."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from multi_orbslam3_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+((?:orbx|orbm|orbv|orbk|orbd|lba|orbg|pose)_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(capi.EXPORTED_SYMBOLS), declared ^ set(capi.EXPORTED_SYMBOLS)
    for s in declared:
        assert hasattr(lib, s), s
    assert b"gfx950" in lib.orbg_version()
    assert lib.orbg_strerror(capi.ORBG_NO_DEVICE).startswith(b"no usable HIP device")


def test_struct_layouts_match_header():
    assert capi.KEYPOINT_DTYPE.itemsize == 24 and capi.EDGE_DTYPE.itemsize == 24
    assert C.sizeof(capi.OrbxConfig) == 56
    assert C.sizeof(capi.LbaProblem) % 8 == 0 and capi.LbaProblem.lambda_init.offset % 8 == 0


def test_ctypes_mirrors_of_the_problem_structs_have_the_headers_layout(tmp_path):
    """sizeof / offsetof of the optimiser's problem structs and the camera rig, asked of the C compiler, against the ctypes mirrors
    the Python host side fills (a field added to one side only would shift every pointer behind it)."""
    import subprocess
    src = tmp_path / "layout.c"
    fields = {"lba_problem": ("LbaProblem", ["n_poses", "poses", "edges", "fx", "lambda_init", "its_round1", "device", "rig"]),
              "pose_opt_problem": ("PoseOptProblem", ["n", "Xw", "inv_sigma2", "fx", "Tcw", "device", "rig"]),
              "orbg_camera": ("Camera", ["model", "fx", "cy", "k"]),
              "orbg_camera_rig": ("CameraRig", ["left", "has_right", "right", "Trl"]),
              "orbx_fisheye_stereo_view": ("FisheyeStereoView", ["n_left", "mono_right", "kps_left", "desc_right", "level_sigma2", "n_levels", "left", "right", "Tlr"]),
              "lba_result": ("LbaResult", ["poses", "edge_outlier", "status", "chi2_initial", "trace", "trace_len"]),
              "pose_opt_result": ("PoseOptResult", ["Tcw", "outlier", "n_inliers", "iters", "chi2"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "orbgpu.h"', 'int main(void) {']
    for cname, (_, fl) in fields.items():
        lines.append('  printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for f in fl:
            lines.append('  printf(" %%zu", offsetof(%s, %s));' % (cname, f))
        lines.append('  printf("\\n");')
    lines.append("  return 0; }")
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert len(out) == len(fields)
    for ln in out:
        parts = ln.split()
        pyname, fl = fields[parts[0]]
        cls = getattr(capi, pyname)
        assert C.sizeof(cls) == int(parts[1]), (parts[0], C.sizeof(cls), parts[1])
        for f, off in zip(fl, parts[2:]):
            assert getattr(cls, f).offset == int(off), (parts[0], f, getattr(cls, f).offset, off)
    assert capi.UR_RIGHT_CAMERA == -2.0 and "#define LBA_UR_RIGHT_CAMERA (-2.0f)" in open(os.path.join(ROOT, "include", "orbgpu.h")).read()


def test_no_gpu_means_loud_failure_not_fallback():
    lib = capi.load()
    if lib.orbg_device_count() > 0:
        pytest.skip("a GPU is present")
    cfg = capi.OrbxConfig(1000, 1.2, 8, 20, 7, 640, 480, 1, 0)
    h = C.c_void_p()
    assert lib.orbx_create(C.byref(cfg), C.byref(h)) == capi.ORBG_NO_DEVICE
    f = C.c_void_p()
    assert lib.orbm_frame_create(0, 100, C.byref(f)) == capi.ORBG_NO_DEVICE
    dv = capi.DatabaseView(0, 0, *([None] * 10))
    assert lib.orbd_database_create(0, C.byref(dv), C.byref(f)) == capi.ORBG_NO_DEVICE
    q = np.zeros((1, 32), np.uint8); d = np.zeros((1, 1), np.int32)
    assert lib.orbm_hamming_matrix(0, C.c_void_p(q.ctypes.data), 1, C.c_void_p(q.ctypes.data), 1, C.c_void_p(d.ctypes.data)) == capi.ORBG_NO_DEVICE
    from multi_orbslam3_amd import api, synth, views
    with pytest.raises(capi.OrbGpuError):
        api.ORBextractor()
    # the left-right matcher of the two-fisheye Frame constructor is a stand-alone entry point: no handle, no fallback either
    fs = synth.make_fisheye_stereo_scene(n_stereo=20, n_mono_left=5, n_mono_right=5, n_distract=5)
    v, keep = views.fisheye_stereo_view(fs["kps_left"], fs["desc_left"], fs["mono_left"], fs["kps_right"], fs["desc_right"], fs["mono_right"], fs["left"], fs["right"],
                                        fs["Tlr"], fs["level_sigma2"])
    with pytest.raises(capi.OrbGpuError) as e:
        api.ComputeStereoFishEyeMatches(v)
    assert e.value.code == capi.ORBG_NO_DEVICE
    # the other entry points without a handle (buffers of the calling thread): the same answer, and what the caller's outputs held
    # before the call is still there afterwards
    vp = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    pr = synth.make_pose_opt_problem(n=40, outlier_frac=0.0, mono_frac=0.5, seed=140)
    p, keep = views.pose_opt_problem(pr["Xw"], pr["u"], pr["v"], pr["ur"], pr["inv_sigma2"], pr["cam"], pr["Tcw"])
    out = views.PoseOptOutput(40)
    out.outlier[:] = 0xA5
    out.c.n_inliers, out.c.n_bad = -7, -7
    for i in range(16):
        out.c.Tcw[i] = -7.0
    for i in range(4):
        out.c.iters[i], out.c.chi2[i] = -7, -7.0
    assert lib.pose_optimize(C.byref(p), C.byref(out.c)) == capi.ORBG_NO_DEVICE
    assert (out.outlier == 0xA5).all() and (out.c.n_inliers, out.c.n_bad) == (-7, -7)
    assert list(out.c.Tcw) == [-7.0] * 16 and list(out.c.iters) == [-7] * 4 and list(out.c.chi2) == [-7.0] * 4
    desc = np.arange(3 * 32, dtype=np.uint8).reshape(3, 32); start = np.array([0, 1, 3, 3], np.int32)
    best = np.full(3, -7, np.int32)
    assert lib.orbm_distinctive_descriptors(0, vp(desc), vp(start), 3, vp(best)) == capi.ORBG_NO_DEVICE
    assert (best == -7).all()
    qw = np.array([1, 5], np.int32); qv = np.array([0.5, 0.5]); cs = np.array([0, 1, 3], np.int32)
    cw = np.array([5, 1, 7], np.int32); cv = np.array([1.0, 0.25, 0.75]); score = np.full(2, -7.0)
    assert lib.orbv_score_l1(0, vp(qw), vp(qv), 2, vp(cs), vp(cw), vp(cv), 2, vp(score)) == capi.ORBG_NO_DEVICE
    assert (score == -7.0).all()
    import sim3_model as sm
    sc = sm.make_scene(1, 20, True, 0.3)
    sp = api.Sim3Problem(sc["X1"], sc["X2"], sc["e1"], sc["e2"], sc["K1"], sc["K2"], True)
    H = api.sim3_ransac_iterations(20)
    draws = api.sim3_draws(20, H, np.random.default_rng(0))
    mask = np.full(20, 0xA5, np.uint8)
    r = capi.Sim3Result()
    r.struct_size = C.sizeof(capi.Sim3Result)
    r.inliers = capi.ptr(mask)
    r.no_more, r.converged, r.n_inliers, r.iterations_done, r.best_iteration, r.have_best, r.s = -7, -7, -7, -7, -7, -7, -7.0
    P = (capi.Sim3Problem * 1)(sp.struct()); Q = (capi.Sim3Params * 1)(capi.Sim3Params(0.99, 6, 300)); D = (C.c_void_p * 1)(draws.ctypes.data)
    assert lib.orbm_sim3_solve_batch(0, P, 1, Q, D, C.byref(r)) == capi.ORBG_NO_DEVICE
    assert (mask == 0xA5).all() and r.s == -7.0
    assert (r.no_more, r.converged, r.n_inliers, r.iterations_done, r.best_iteration, r.have_best) == (-7,) * 6


def test_product_never_references_the_oracle():
    """The product package and C sources must not import / include anything under oracle/."""
    pkg = os.path.join(ROOT, "multi_orbslam3_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".cpp", ".hpp", ".h", ".sh")):
                txt = open(os.path.join(dirpath, fn)).read()
                assert "liboracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, fn
                assert not re.search(r'#include\s+"[^"]*oracle/', txt), fn


def test_generated_jump_tables_are_current():
    """csrc/ldlt_jump_tables.inc (the per-tile dispatch tables of ldltm::k_ldlt_big) is generated: the committed file must be
    what tools/gen/gen_ldlt_jump_tables.py writes, and every case of a table must have the stride the computed jump assumes
    (4 matrix instructions = 32 bytes + s_branch + one s_nop = 40; 8 = 64 + 4 + 4 = 72)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_jt", os.path.join(root, "tools", "gen", "gen_ldlt_jump_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert open(gen.DST).read() == gen.render()
    for n in (32, 48):
        lines = gen.mfma4(n)
        assert sum(1 for l in lines if l.startswith("v_mfma")) == 4 * n and sum(1 for l in lines if l.startswith("s_branch")) == n
        lines = gen.get(n)
        assert sum(1 for l in lines if l.startswith("s_branch")) == n


def test_big_ldlt_kernel_keeps_the_compiler_out_of_its_tile_registers(tmp_path):
    """ldltm::k_ldlt_big48 keeps its 48 tiles in a0..a255 and v128..v255, addressed from inline assembly only; hipcc is kept out
    of them by amdgpu_num_vgpr(128) and clobber lists.  Guard: in the device assembly of lba.hip no instruction OUTSIDE the
    assembly statements touches an accumulation register or a vector register >= 128, nothing is spilled to scratch, and the
    kernel's allocation is the whole register file (512)."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "lba_dev.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                    "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S", "-o", str(out),
                    os.path.join(root, "multi_orbslam3_amd", "csrc", "lba.hip")], check=True, stderr=subprocess.DEVNULL, timeout=600)
    text = out.read_text()
    m = re.search(r"^(_ZN5ldltm12k_ldlt_big48\w*):", text, re.M)
    assert m, "kernel not found"
    name = m.group(1)
    body = text[m.start():text.index("s_endpgm", m.start())]
    assert "scratch_" not in body
    in_asm, bad = False, []
    for line in body.splitlines():
        if "#ASMSTART" in line:
            in_asm = True
            continue
        if "#ASMEND" in line:
            in_asm = False
            continue
        if in_asm:
            continue
        code = line.split(";")[0]
        if "v_accvgpr" in code or re.search(r"\ba\[?\d", code) or any(int(x) >= 128 for x in re.findall(r"\bv\[?(\d+)", code)):
            bad.append(line.strip())
    assert not bad, bad[:5]
    desc = text[text.index(".amdhsa_kernel " + name):]
    assert re.search(r"\.amdhsa_next_free_vgpr\s+512", desc[:3000]) and re.search(r"\.amdhsa_accum_offset\s+256", desc[:3000])


def test_agent_loop_library_loads_and_its_structures_match_the_binding():
    """libagentloop.so (the Tracking-thread loop above the C-ABI) links against liborbgpu.so; the ctypes mirror of agent_cfg /
    agent_stats / agent_frame_in has the C sizes (checked inside load())."""
    from multi_orbslam3_amd import agent
    lib = agent.load()
    assert lib.agent_sizeof(0) > 200 and hasattr(lib, "agent_run") and hasattr(lib, "agent_drain")


def test_wait_policy_per_thread_role():
    """orbg_set_wait_policy / orbg_get_wait_policy (include/orbgpu.h "Host threads"): per role of the waiting thread, process-wide,
    changeable at run time; the start-up policy comes from ORBG_NO_POLL.  No GPU involved."""
    import subprocess
    import sys
    code = ("from multi_orbslam3_amd import _capi\n"
            "lib = _capi.load()\n"
            "print([lib.orbg_get_wait_policy(r) for r in range(3)], lib.orbg_get_wait_policy(3), lib.orbg_set_wait_policy(7, 1))\n"
            "assert lib.orbg_set_wait_policy(1, 1) == 0 and lib.orbg_set_wait_policy(0, 0) == 0\n"
            "print([lib.orbg_get_wait_policy(r) for r in range(3)])\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for env_val, first in ((None, [1, 1, 1]), ("1", [0, 0, 0]), ("all", [0, 0, 0]), ("lba,ingest", [1, 0, 0]), ("caller", [0, 1, 1])):
        env = {k: v for k, v in os.environ.items() if k != "ORBG_NO_POLL"}
        if env_val is not None:
            env["ORBG_NO_POLL"] = env_val
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=root)
        assert r.returncode == 0, r.stderr[-1500:]
        lines = r.stdout.strip().splitlines()
        assert lines[0] == "%s -2 -2" % first, (env_val, lines)
        want = list(first); want[1] = 1; want[0] = 0
        assert lines[1] == str(want), (env_val, lines)
