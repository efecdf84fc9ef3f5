"""orbgpu::dropin::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) (include/orbgpu_dropin.hpp), the welding BA of a map
merge: tests/cpp/weld_ba_glue.cpp runs it over the mocks of tests/cpp/mock_weld_ba.hpp with a recording solver -- the run where no
adjusted keyframe carries the stamp (free poses without edges) and the run where one does, a bad keyframe, a keyframe of another map, a
bad point, a point that turns bad while the solve runs, mnId > maxKFid, the throws, the erase list's order, the write-back under the
map's mutex, no write-back after the early return -- and checks the problem handed to ba_weld_solve field by field.  No device is
needed.  (tools/weld_ba_sanitize.sh builds the same stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _build(out, extra=()):
    lib_dir = os.path.join(ROOT, "multi_orbslam3_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", *extra, "-I", os.path.join(ROOT, "include"),
                           "-I", CPP, os.path.join(CPP, "weld_ba_glue.cpp"), "-o", out, "-pthread", "-L", lib_dir, "-lorbgpu",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


def test_glue_hands_over_the_reference_problem_and_writes_back_under_the_mutex(tmp_path):
    exe = _build(str(tmp_path / "weld_ba_glue"))
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    words = p.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 150, p.stdout
