"""The shared device primitives on the device, one by one (tools/micro/device_math_test.hip): the DPP scans and sums of csrc/wave.hpp, the
lane solve and the block sums of lm_block.hpp / lm_record.hpp, the quaternion, SE3, camera, Sim3 and SO3 functions of se3.hpp,
sim3_math.hpp and pose_inertial_edges.hpp, and null_vector4.hpp, against tests/device_math_model.py.  One build, one run of the program
over the whole case file, then one assertion per function over its outputs."""
import pytest

import device_math_harness as dh
import device_math_model as dm

pytestmark = pytest.mark.gpu

FIDS = sorted(dm.FNS)


@pytest.fixture(scope="module")
def device_outputs(tmp_path_factory):
    return dh.run(dh.build(), tmp_path_factory.mktemp("device_math"), host=False)


@pytest.mark.parametrize("fid", FIDS, ids=[dm.FNS[f][0] for f in FIDS])
def test_device_meets_the_rule(device_outputs, fid):
    """integers, flags, the sums, the lane solve and the + - * / sqrt functions bit for bit; fast_rsqrt to 2 ulp of the correctly rounded
    value; everything else within MARGIN yardsticks of (mp)"""
    worst, fails = dh.check_function(fid, device_outputs)
    print("%-28s device: worst ratio %s" % (dm.FNS[fid][0], "bit-equal" if worst is None else "%.3g" % worst))
    assert not fails, "\n".join(fails[:8])
