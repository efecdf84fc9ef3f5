"""orbgpu::dropin::BundleAdjustment / GlobalBundleAdjustemnt (include/orbgpu_dropin.hpp): tests/cpp/full_ba_glue.cpp runs them over mock
keyframes, map points and a map -- a bad keyframe, a bad point, a point only bad keyframes observe, keyframes of two clients with two
cameras, bUseUniqueId both ways, nLoopKF equal and not equal to the origin keyframe's id -- with a recording solver, and checks the
problem handed to ba_solve and both write-back branches field by field.  No device is needed.  (tools/full_ba_sanitize.sh builds the
same stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer and runs it on the CPU.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _build(out, extra=()):
    lib_dir = os.path.join(ROOT, "multi_orbslam3_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", *extra, "-I", os.path.join(ROOT, "include"),
                           "-I", CPP, os.path.join(CPP, "full_ba_glue.cpp"), "-o", out, "-pthread", "-L", lib_dir, "-lorbgpu",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


def test_glue_hands_over_the_reference_problem_and_writes_both_branches_back(tmp_path):
    exe = _build(str(tmp_path / "full_ba_glue"))
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    words = p.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 150, p.stdout
