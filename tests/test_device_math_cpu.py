"""The case list and the references of the device primitives (tests/device_math_model.py) checked against themselves, and the harness
(tools/micro/device_math_test.hip) in `host` mode, which evaluates the __host__ __device__ functions on the CPU.  No GPU."""
import collections

import mpmath
import numpy as np
import pytest

import device_math_harness as dh
import device_math_model as dm


@pytest.fixture(scope="module")
def host_outputs(tmp_path_factory):
    return dh.run(dh.build(), tmp_path_factory.mktemp("device_math"), host=True)


def branches_of(fid):
    return collections.Counter(r.branch for c, r in zip(dm.build_cases(), dm.references()) if c.fid == fid)


def test_the_case_file_holds_a_few_thousand_cases_with_the_counts_of_the_table():
    cases = dm.build_cases()
    assert 2000 <= len(cases) <= 5000
    assert {c.fid for c in cases} == set(dm.FNS)


def test_every_branch_of_every_function_is_taken():
    want = {
        20: {"trace", "i0", "i1", "i2"}, 23: {"flip", "keep"}, 24: {"flip", "keep"},
        40: {"small", "full"}, 42: {"small", "full"}, 43: {"small", "full"}, 45: {"small", "full"}, 46: {"small", "full"},
        41: {"out_of_range", "unscaled", "scaled"}, 34: {"pinhole", "kb8", "kb8_back"}, 35: {"pinhole", "kb8", "kb8_back"},
        50: {"diagonal", "sweeps"},
        10: {"ok", "fail_pos"}, 11: {"ok", "fail_pos"}, 12: {"ok", "fail_pos"},
        13: {"ok", "fail_pos", "fail_rel"}, 14: {"ok", "fail_pos", "fail_rel"}, 15: {"ok", "fail_pos", "fail_rel"},
        60: {"accepted_2/3", "accepted_cubic", "accepted_1/3", "rejected_rho", "rejected_not_finite"}, 61: {"2/3", "cubic", "1/3"},
        62: {"exhausted", "rho_zero", "bad", "bad_stop", "good"}, 63: {"user", "diagonal"}, 64: {"inlier", "outlier"},
    }
    for fid, need in want.items():
        assert set(branches_of(fid)) >= need, (dm.FNS[fid][0], branches_of(fid))
    # the LM verdict: every way a trial can come to be rejected, and the rejection factor doubling three times in a row
    verdict = {c.tag: (c, r) for c, r in zip(dm.build_cases(), dm.references()) if c.fid == 60}
    assert set(verdict) >= {"negative_scale_larger_chi2", "zero_scale_smaller_chi2", "rho_negative", "rho_zero", "zero_over_zero", "chi2_nan",
                            "chi2_inf", "chi2_minus_inf", "refused_solve_small_chi2"}
    assert [verdict["rejection_%d_in_a_row" % k][1].exact[3] for k in (1, 2, 3)] == [4.0, 8.0, 16.0]
    assert verdict["zero_over_zero"][1].exact[0] == dm.SENTINEL and verdict["zero_scale_smaller_chi2"][1].exact[0] == np.inf
    assert verdict["refused_solve_small_chi2"][1].exact[0] < -1e300
    huber = {c.tag: r for c, r in zip(dm.build_cases(), dm.references()) if c.fid == 64}
    assert list(huber["nan_5.991"].exact) == [dm.SENTINEL, dm.SENTINEL] and list(huber["at_5.991"].exact)[1] == 1.0
    # SE3Quat::exp: both forms of R, each low-trace branch of the quaternion, both signs before each normalisation
    for fid in (30, 31, 32):
        b = set(branches_of(fid))
        assert {x.split("/")[0] for x in b} == {"small", "full"}
        assert {x.split("/")[1] for x in b} >= {"trace", "i0", "i1", "i2"}, b
        assert {x.split("/")[2] for x in b} == {"flip", "keep"}
    # pose_oplus_series: both sides of its hand-over
    t_of = [sum(x * x for x in c.dv[7:10]) for c in dm.build_cases() if c.fid == 32]
    assert {dm.series_path(t) for t in t_of} == {"series", "handover"}
    # Sim3: the four combinations in exp and in log, the six paths of the LU in log
    for fid in (28, 29):
        b = set(branches_of(fid))
        assert {tuple(x.split("/")[0:2]) for x in b} == {(s, t) for s in ("sig_small", "sig_big") for t in ("th_small", "th_big")}, b
    assert {x.split("/")[2] for x in branches_of(29)} == {"p0n", "p0s", "p1n", "p1s", "p2n", "p2s"}
    # the pivot of lane_ldlt_solve fails at the first, a middle and the last index, in each of the four ways
    for fid, (n, _) in dm.LDLT.items():
        tags = {c.tag for c in dm.build_cases() if c.fid == fid}
        assert tags >= {"pivot_%s_k%d" % (w, k) for w in ("zero", "negative", "nan", "inf") for k in (0, n // 2, n - 1)}


def test_no_case_stands_near_a_threshold_and_both_arithmetics_take_the_same_branch():
    """A comparison passes when (a) its operands stand more than a relative 1e-3 apart in (f64) and in (mp), or (b) its operands are
    exact in float64 (the (mp) operands are the same numbers: the two cannot decide differently), or (c) its operands are EQUAL in
    both arithmetics (the exact ties).  Nothing is excluded."""
    near, differ = [], []
    with mpmath.workdps(dm.MP_DPS):
        for c, r in zip(dm.build_cases(), dm.references()):
            if r.dec64 is None:
                if r.mp_branch is not None and r.mp_branch != r.branch:
                    differ.append((dm.FNS[c.fid][0], c.tag, r.branch, r.mp_branch))
                continue
            assert len(r.dec64.compares) == len(r.decmp.compares)
            for (l64, op, r64, scale), (lmp, _, rmp, _), took in zip(r.dec64.compares, r.decmp.compares, r.dec64.taken):
                if dm.Decide.natural(lmp, op, rmp) != took:
                    differ.append((dm.FNS[c.fid][0], c.tag, op, l64, r64))
                exact = mpmath.mpf(l64) == lmp and mpmath.mpf(r64) == rmp
                tie = l64 == r64 and lmp == rmp
                apart = min(dm.compare_margin(l64, r64, scale), dm.compare_margin(lmp, rmp, scale)) > 1e-3
                if not (apart or exact or tie):
                    near.append((dm.FNS[c.fid][0], c.tag, op, l64, r64))
            if c.fid == 32:
                t64 = sum(x * x for x in c.dv[7:10])
                tmp = sum(mpmath.mpf(x) ** 2 for x in c.dv[7:10])
                assert dm.series_path(t64) == dm.series_path(tmp) and abs(t64 - 0.09) > 1e-3 * 0.09
            if r.rnd64:
                assert [float(x) for x in r.rndmp] == list(r.rnd64), ("a float32 rounding lands on different floats", c.tag)
    assert not differ, differ[:10]
    assert not near, near[:10]


def test_the_thresholds_are_approached_from_both_sides():
    tags = collections.defaultdict(set)
    for c in dm.build_cases():
        tags[c.fid].add(c.tag.rsplit("_", 1)[0] if c.fid in (30, 31, 32) else c.tag)
    for fid in (30, 31, 32):
        assert tags[fid] >= {"theta9.9e-06", "theta1.01e-05", "theta0.2995", "theta0.3005", "theta2.2", "theta3.1"}
    for fid in (13, 14, 15):
        refs = {c.tag: r.branch for c, r in zip(dm.build_cases(), dm.references()) if c.fid == fid}
        assert refs["rel_delta_2^-40"] == "fail_rel" and refs["rel_delta_2^-39"] == "ok"
    for fid in (10, 11, 12):
        refs = {c.tag: r.branch for c, r in zip(dm.build_cases(), dm.references()) if c.fid == fid}
        assert refs["rel_delta_2^-40"] == "ok" and refs["rel_delta_2^-39"] == "ok"
    ties = {c.tag: r.branch for c, r in zip(dm.build_cases(), dm.references()) if c.fid == 20}
    assert ties["exact_180_110"] == "i0" and ties["exact_180_101"] == "i0" and ties["exact_180_011"] == "i1" and ties["exact_120_111"] == "i0"
    lu = {c.tag: r.branch for c, r in zip(dm.build_cases(), dm.references()) if c.fid == 29}
    assert lu["lu_tie_first_pivot"].split("/")[2] in ("p1n", "p1s") and lu["lu_tie_first_pivot_exact_arithmetic"] in ("sig_small/th_small/p1n", "sig_small/th_small/p1s"), lu


def test_the_bit_exact_models_of_the_sums_and_of_the_serial_ldlt_agree_with_mp():
    """the references that the device is held to bit for bit are themselves held to the yardstick rule"""
    cases, refs = dm.build_cases(), dm.references()
    outs = [np.asarray(r.exact) if (c.fid in (2, 3, 4, 5) or c.fid in dm.LDLT) else np.zeros(dm.FNS[c.fid][3]) for c, r in zip(cases, refs)]
    for fid in [2, 3, 4, 5] + sorted(dm.LDLT):
        worst, fails = dh.check_function(fid, outs)
        print("%-28s model against (mp): worst ratio %.3g" % (dm.FNS[fid][0], worst))
        assert not fails, fails[:5]
    # lane l holding 2^l over half a wavefront: every addend visible in the sum, so a lane added twice or dropped shows
    assert dm.wave_tree_sum([2.0 ** l if l < 32 else 0.0 for l in range(64)]) == 2.0 ** 32 - 1
    assert dm.wave_tree_sum([2.0 ** (l - 32) if l >= 32 else 0.0 for l in range(64)]) == 2.0 ** 32 - 1


@pytest.mark.parametrize("fid", dm.HOST_FIDS, ids=[dm.FNS[f][0] for f in dm.HOST_FIDS])
def test_host_mode_meets_the_rule(host_outputs, fid):
    worst, fails = dh.check_function(fid, host_outputs)
    print("%-24s host: worst ratio %s" % (dm.FNS[fid][0], "bit-equal" if worst is None else "%.3g" % worst))
    assert not fails, "\n".join(fails[:8])


def test_host_mode_evaluates_nothing_else(host_outputs):
    for c, o in zip(dm.build_cases(), host_outputs):
        assert (len(o) > 0) == (c.fid in dm.HOST_FIDS)
