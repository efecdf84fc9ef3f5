"""The many-workgroup LDL^T of csrc/ldlt_wide.hpp on its own (tools/micro/ldlt_wide_test.hip): against a long-double host factorisation
up to 1542 unknowns, against Woodbury's identity on diagonal-plus-rank-3 systems up to the cap of 8192, and by its long-double
residual everywhere; the structure cases, the failing pivots and the refusal above the cap.  One run of the program."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 1, 15, 16, 17 | 31, 32, 33 | 304 .. 320 | 1023, 1024, 1025 | 1542: dense and rank 3 each; 2049, 8190, 8192: rank 3 alone
N_SIZE_LINES = 2 * (4 + 3 + 17 + 3 + 1) + 3
# at n = 100 and n = 1030: a pivot exactly 0 at 0, 7, 16, in a middle block and at n - 1; a NaN and a +Inf on a middle block's diagonal;
# at n = 112 and n = 1040 a pivot exactly 0 at n - 1, the end of a full last block (the one zero that no non-finite pivot follows)
N_PIVOT_LINES = 2 * (5 + 2 + 1)


def test_wide_ldlt_against_long_double_references_up_to_its_cap():
    src = os.path.join(ROOT, "tools", "micro", "ldlt_wide_test.hip")
    exe = os.path.join(ROOT, "tools", "micro", "ldlt_wide_test")
    hdr = os.path.join(ROOT, "multi_orbslam3_amd", "csrc", "ldlt_wide.hpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in (src, hdr)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-o", exe, src], timeout=900)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-1000:]
    lines = r.stdout.splitlines()
    assert not [ln for ln in lines if "FAIL" in ln], r.stdout[-6000:]
    sizes = [ln for ln in lines if ln.startswith("n=")]
    assert len(sizes) == N_SIZE_LINES and all(ln.endswith(" ok") for ln in sizes), sizes
    assert {int(ln[2:6]) for ln in sizes} == {1, 15, 16, 17, 31, 32, 33, *range(304, 321), 1023, 1024, 1025, 1542, 2049, 8190, 8192}
    pivots = [ln for ln in lines if ln.startswith("pivot ")]
    assert len(pivots) == N_PIVOT_LINES and all(": ok=0 x untouched 1 guards 1; the next solve on the same flag: ok=1 ok" in ln for ln in pivots), pivots
    assert sum(ln.startswith("refusal n=8193: hipErrorInvalidValue, x untouched 1 ok word -1 guards 1 ok") for ln in lines) == 1, r.stdout[-6000:]
    for head, count in (("bits ", 3), ("egfix ", 2), ("indef ", 2), ("contract ", 2), ("time ", 4)):
        assert sum(ln.startswith(head) for ln in lines) == count, (head, r.stdout[-6000:])
