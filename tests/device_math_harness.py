"""Builds and runs tools/micro/device_math_test.hip and holds its outputs against tests/device_math_model.py: what
tests/test_device_math_cpu.py (`host` mode, no GPU) and tests/test_gpu_device_math.py (device mode) share."""
import math
import os
import re
import subprocess

import mpmath
import numpy as np

import device_math_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi_orbslam3_amd", "csrc")
SRC = os.path.join(ROOT, "tools", "micro", "device_math_test.hip")
EXE = os.path.join(ROOT, "tools", "micro", "device_math_test")
HEADERS = ["wave.hpp", "lm_block.hpp", "lm_record.hpp", "lm_step.hpp", "common.hpp", "se3.hpp", "sim3_math.hpp", "pose_inertial_edges.hpp", "null_vector4.hpp"]


def build_flags():
    """the FLAGS line of csrc/build.sh, so that the harness and the library cannot drift apart"""
    text = open(os.path.join(CSRC, "build.sh")).read()
    m = re.search(r'^FLAGS="([^"]*)"$', text, re.M)
    assert m, "csrc/build.sh has no FLAGS line"
    return m.group(1).split()


def build(exe=EXE, include_dir=CSRC):
    """rebuilds when the source, a header it includes or build.sh is newer than the binary"""
    deps = [SRC, os.path.join(CSRC, "build.sh")] + [os.path.join(include_dir, h) for h in HEADERS]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build_flags() + ["-I", include_dir, "-o", exe, SRC], timeout=900)
    return exe


def run(exe, workdir, host):
    """one run of the harness over the whole case list -> the outputs per case"""
    cases = dm.build_cases()
    fin, fout = os.path.join(str(workdir), "cases.bin"), os.path.join(str(workdir), "host.bin" if host else "device.bin")
    dm.write_cases(fin, cases)
    r = subprocess.run([exe] + (["host"] if host else []) + [fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return dm.read_outputs(fout, cases)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def _null_vector_terms(c, r, v):
    """-> (kind, error of v, error of the float64 eigensolver) for a null_vector4 case that ran sweeps"""
    S = np.array(c.dv).reshape(4, 4)
    lam, vecs = r.mp
    with mpmath.workdps(dm.MP_DPS):
        Sm = mpmath.matrix(S.tolist())

        def resid(x):
            x = mpmath.matrix([mpmath.mpf(float(t)) for t in x])
            x = x / mpmath.norm(x)
            return float(abs(mpmath.norm(Sm * x) - abs(lam[0])))

        def vdist(x):
            x = [mpmath.mpf(float(t)) for t in x]
            sgn = 1 if sum(a * b for a, b in zip(x, vecs[0])) >= 0 else -1
            return float(max(abs(sgn * a - b) for a, b in zip(x, vecs[0])))
        w64, V64 = r.f64
        if lam[1] - lam[0] > mpmath.mpf(1e-6) * lam[3]:
            return "vector", vdist(v), max(vdist(V64[:, 0]), dm.ulp(1.0))
        return "residual", resid(v), max(resid(V64[:, 0]), dm.ulp(float(lam[3])))


def check_function(fid, outs, ystick=None):
    """Holds every case of one function against its references.  -> (worst ratio or None, list of failure strings)"""
    cases, refs = dm.build_cases(), dm.references()
    if ystick is None:
        ystick = dm.yardsticks(cases, refs, {fid})
    fails, worst = [], None
    group = [(c, r, o) for c, r, o in zip(cases, refs, outs) if c.fid == fid]
    assert group and all(len(o) == dm.FNS[fid][3] for _, _, o in group), "no outputs for fid %d" % fid
    # the yardstick of null_vector4: per kind, the largest error of the float64 eigensolver
    nv_y = {}
    if fid == 50:
        for c, r, o in group:
            if r.exact is None:
                kind, _, y = _null_vector_terms(c, r, o[0:4])
                nv_y[kind] = max(nv_y.get(kind, 0.0), y)
    for c, r, o in group:
        name = "%s[%s]" % (dm.FNS[fid][0], c.tag)
        if c.want is not None and r.branch != c.want:
            fails.append("%s: the model took %s, the case is meant for %s" % (name, r.branch, c.want))
        if r.exact is not None and not same_bits(o, r.exact):
            bad = np.flatnonzero(np.asarray(o).view(np.uint64) != np.asarray(r.exact, dtype=np.float64).view(np.uint64))
            fails.append("%s: bits differ at %s: got %s, expected %s" % (name, bad[:6].tolist(), [float(o[i]).hex() for i in bad[:3]], [float(r.exact[i]).hex() for i in bad[:3]]))
            continue
        ratio = None
        if fid in dm.LDLT:
            if r.mp is not None:
                n = dm.LDLT[fid][0]
                ratio = dm.tolerance_ratio(c, r, o[2:2 + n], ystick)
        elif fid in (2, 3, 4, 5):
            # a sum: the yardstick is the plain left-to-right float64 sum's distance from (mp), floored at one ulp of the largest
            # addend (an intermediate sum of that size is rounded to its ulp in any order)
            k = len(r.mp)
            cols = [c.dv[i::k] for i in range(k)] if fid == 5 else [c.dv[256 * i:256 * i + len(c.dv) // k] for i in range(k)] if fid == 3 else [c.dv]
            got = [o[0], o[256]] if fid == 3 else list(o[0:k]) if fid == 5 else [o[0]]
            ratio = 0.0
            for col, g, m in zip(cols, got, r.mp):
                seq = 0.0
                for x in col:
                    seq = seq + x
                y = max(abs(float(mpmath.mpf(seq) - m)), dm.ulp(max(abs(x) for x in col)))
                ratio = max(ratio, abs(float(mpmath.mpf(float(g)) - m)) / y if y > 0 else 0.0)
        elif fid == 33:
            cr = r.f64[0]
            ratio = abs(float(o[0]) - cr) / math.ulp(cr)
            if not ratio <= 2.0:
                fails.append("%s: d = %r: %r is %.1f ulp from the correctly rounded %r" % (name, c.dv[0], float(o[0]), ratio, cr))
            worst = max(worst or 0.0, ratio)
            continue
        elif fid == 50:
            if r.exact is None:
                kind, err, _ = _null_vector_terms(c, r, o[0:4])
                ratio = err / nv_y[kind]
        elif r.exact is None:
            ratio = dm.tolerance_ratio(c, r, o, ystick)
        if ratio is not None:
            worst = max(worst or 0.0, ratio)
            if not ratio <= dm.MARGIN:
                fails.append("%s (%s): %.3g yardsticks from (mp), more than MARGIN = %g" % (name, r.branch, ratio, dm.MARGIN))
    return worst, fails
