"""What the model of LocalInertialBA restates beyond the per-frame optimiser's model, taken from the reference's own text at test time
and executed against tests/inertial_ba_model.py:
  EdgeMono / EdgeStereo::linearizeOplus                          S/G2oTypes.cc:349-427
  ImuCamPose::Project / ProjectStereo                            S/G2oTypes.cc:170-185
  the kernel and information set-up of the inertial edges        S/Optimizer.cc:4826-4863
  the thresholds and the two erase predicates                    S/Optimizer.cc:4894-4897, 5088-5119
  the lambda, the iteration count and the fail predicate         S/Optimizer.cc:4561-4567, 4690-4701, 5072-5076, 5128
(SO3, ImuCamPose::Update and EdgeInertial are held by tests/test_pose_inertial_reference.py; its translator and Eigen stand-in are
imported here, not edited.)  CPU only; nothing of the reference is stored."""
import os
import re

import numpy as np
import pytest

import inertial_ba_model as m
import test_pose_inertial_reference as pr
import test_reference_formulas as rf

pytestmark = pytest.mark.skipif(not os.path.isdir(rf.REF), reason="the reference is only present in the build container")
G2OTYPES, OPTIMIZER = pr.G2OTYPES, pr.OPTIMIZER
E = pr.E
f32 = np.float32


def _liba():
    return rf._body(OPTIMIZER, r"void Optimizer::LocalInertialBA\(KeyFrame \*pKF, bool \*pbStopFlag, Map \*pMap, bool bLarge, bool bRecInit\)")


def _scene():
    P = m.build_case("n2")
    S = m.Structure(P)
    kfs, X = m.initial_state(P)
    return P, S, kfs, X


class _Pinhole:
    """Pinhole::project / projectJac (S/CameraModels/Pinhole.cpp) as far as the edges call them"""

    def __init__(self, cam):
        self.fx, self.fy, self.cx, self.cy = cam[:4]

    def project(self, Xc):
        x, y, z = Xc.a
        return E(np.array([self.fx * x / z + self.cx, self.fy * y / z + self.cy]))

    def projectJac(self, Xc):
        x, y, z = Xc.a
        return E(np.array([[self.fx / z, 0.0, -self.fx * x / (z * z)], [0.0, self.fy / z, -self.fy * y / (z * z)]]))


def _vpose(P, s):
    Tcb = np.asarray(P["Tcb"], np.float64).reshape(3, 4)
    cam = tuple(float(c) for c in P["cam"])
    Rcw, tcw = m.pim.camera_pose(s, Tcb)
    Rcb, tcb = Tcb[:, :3], Tcb[:, 3]
    return type("VPose", (), {"Rcw": [E(Rcw)], "tcw": [E(tcw)], "Rcb": [E(Rcb)], "Rbc": [E(Rcb.T)], "tbc": [E(-(Rcb.T @ tcb))], "bf": cam[4],
                              "pCamera": [_Pinhole(cam)]})()


def _fix_elements(body):
    """Eigen's one-index element reads become Python's, the two writes into parts of a matrix become whole-matrix assignments"""
    body = re.sub(r"\b(Xb|Xc|Pc)\((\d)\)", r"\1[\2]", body)
    body = body.replace("proj_jac.block<1,3>(2,0) = proj_jac.block<1,3>(0,0)", "proj_jac.block<1,3>(2,0) = _row0(proj_jac)")
    return re.sub(r"proj_jac\(2,2\) \+= ([^;]*);", r"proj_jac.block<1,1>(2,2) = _one(proj_jac(2,2) + \1);", body)


@pytest.mark.parametrize("kind", ["EdgeMono", "EdgeStereo"])
def test_visual_linearize_oplus_is_the_references_text(kind):
    P, S, kfs, X = _scene()
    err, Xc, c2, Rcw = m.visual_edges(P, S, kfs, X)
    Jl, Jp = m.visual_jacobians(P, S, Xc, Rcw)
    mono = kind == "EdgeMono"
    ks = np.flatnonzero(S.mono == mono)[:8]
    assert len(ks) == 8
    body = pr._translate(_fix_elements(rf._body(G2OTYPES, r"void %s::linearizeOplus\(\)" % kind)), {"SE3deriv": (3, 6)})
    src = "\n".join(["def linearizeOplus(VPose, VPoint, cam_idx):", "    proj_jac = E(np.zeros((3, 3)))"] + ["    " + l for l in body] +
                    ["    return _jacobianOplusXi, _jacobianOplusXj"])
    ns = dict(pr.BASE_ENV)
    ns.update({"np": np, "_row0": lambda M: E(M.a[0:1, :]), "_one": lambda v: E(np.array([[v]]))})
    exec(src, ns)
    for k in ks:
        Ji, Jj = ns["linearizeOplus"](_vpose(P, kfs[S.e_kf[k]]), E(X[S.e_pt[k]]), 0)
        rows = 2 if mono else 3
        assert Ji.a.shape == (rows, 3) and Jj.a.shape == (rows, 6)
        # the same products in another association: a few roundings of the largest entry
        assert np.abs(Ji.a - Jl[k][:rows]).max() <= 1e-14 * np.abs(Jl[k]).max()
        assert np.abs(Jj.a - Jp[k][:rows]).max() <= 1e-14 * np.abs(Jp[k]).max()


def test_project_and_project_stereo_are_the_references_text():
    P, S, kfs, X = _scene()
    err, Xc, c2, Rcw = m.visual_edges(P, S, kfs, X)
    pre = ["Rcw, tcw, pCamera, bf = self.Rcw, self.tcw, self.pCamera, self.bf"]
    proj, _ = pr._function(G2OTYPES, r"Eigen::Vector2d ImuCamPose::Project\(const Eigen::Vector3d &Xw, int cam_idx\) const", "Project",
                           ["self", "Xw", "cam_idx"], pre=pre)
    fix = lambda b: re.sub(r"pc\(2\) = ([^;]*);", r"pc = _cat(pc, \1);", _fix_elements(b).replace("pc.head(2) =", "pc =").replace("pc(0)", "pc[0]"))
    pst, _ = pr._function(G2OTYPES, r"Eigen::Vector3d ImuCamPose::ProjectStereo\(const Eigen::Vector3d &Xw, int cam_idx\) const", "ProjectStereo",
                          ["self", "Xw", "cam_idx"], pre=pre, fix=fix)
    for k in list(np.flatnonzero(S.mono)[:6]) + list(np.flatnonzero(~S.mono)[:6]):
        vp, Xw = _vpose(P, kfs[S.e_kf[k]]), E(X[S.e_pt[k]])
        got = (proj if S.mono[k] else pst)(vp, Xw, 0).a
        rows = 2 if S.mono[k] else 3
        # computeError (I/G2oTypes.h): _error = obs - Project(...)
        assert got.shape == (rows,)
        assert np.abs((S.obs[k][:rows] - got) - err[k][:rows]).max() <= 1e-13 * np.abs(S.obs[k]).max()


def test_inertial_edge_setup_is_the_references_text():
    body = _liba()
    seg = body[body.index("vei[i] = new EdgeInertial"):body.index("// Set MapPoint vertices") if "// Set MapPoint vertices" in body else body.index("vpEdgesMono")]
    mm = re.search(r"if\(i==N-1 \|\| bRecInit\)\s*\{(.*?)\}\s*optimizer\.addEdge\(vei\[i\]\)", seg, re.S)
    assert mm
    blk = mm.group(1)
    assert "setRobustKernel(rki)" in blk
    scale = re.search(r"if\(i==N-1\)\s*vei\[i\]->setInformation\(vei\[i\]->information\(\)\*([0-9.e+-]+)\)", blk)
    delta = re.search(r"rki->setDelta\(sqrt\(([0-9.]+)\)\)", blk)
    assert float(scale.group(1)) == m.INFO_LAST and np.sqrt(float(delta.group(1))) == m.DELTA_INERTIAL
    # executed: which edges get the kernel, which the factor
    for N in (1, 3):
        for rec in (False, True):
            for i in range(N):
                robust = eval("i==N-1 or bRecInit", {"i": i, "N": N, "bRecInit": rec})
                P = {"kfs": [{"fixed": True, "imu": True, "prev": None}] +
                     [{"fixed": False, "imu": True, "prev": j, "last_in_window": j == 0} for j in range(N)], "points": np.zeros((0, 3)),
                     "edges": np.zeros(0, m.EDGE_DTYPE), "rec_init": rec}
                # the model's list runs from the oldest keyframe (the reference's i = N - 1) to the newest (i = 0)
                assert m.Structure(P).inertial[N - 1 - i][2] == robust
    # the random walks: the 3 x 3 blocks of C at 9 and 12, inverted by SVD, read as floats; no kernel
    for name, lo in (("G", 9), ("A", 12)):
        assert re.search(r"cvInfo%s = pKFi->mpImuPreintegrated->C\.rowRange\(%d,%d\)\.colRange\(%d,%d\)\.inv\(cv::DECOMP_SVD\)" % (name, lo, lo + 3, lo, lo + 3), seg)
        assert re.search(r"Info%s\(r,c\)=cvInfo%s\.at<float>\(r,c\)" % (name, name), seg)
    assert seg.count("setRobustKernel") == 1
    assert re.search(r"pKFi->mpImuPreintegrated->SetNewBias\(pKFi->mPrevKF->GetImuBias\(\)\)", body)


def test_thresholds_and_erase_predicates_are_the_references_text():
    body = _liba()
    consts = {k: f32(float(v)) for k, v in re.findall(r"const float (chi2Mono2|chi2Stereo2)\s*=\s*([0-9.]+);", body)}
    assert consts["chi2Mono2"] == f32(m.CHI2_MONO) and consts["chi2Stereo2"] == f32(m.CHI2_STEREO)
    hub = dict(re.findall(r"const float (thHuberMono|thHuberStereo)\s*=\s*sqrt\(([0-9.]+)\);", body))
    assert float(f32(np.sqrt(float(hub["thHuberMono"])))) == m.DELTA_MONO and float(f32(np.sqrt(float(hub["thHuberStereo"])))) == m.DELTA_STEREO
    assert re.search(r"bool bClose = pMP->mTrackDepth<10\.f;", body)
    conds = re.findall(r"if\((\(e->chi2\(\)>chi2Mono2[^\n]*|e->chi2\(\)>chi2Stereo2)\)\s*\{\s*KeyFrame\* pKFi = vpEdgeKF(Mono|Stereo)\[i\];", body)
    assert [c[1] for c in conds] == ["Mono", "Stereo"]                      # the erase list: mono edges first, then stereo

    class Edge:
        def __init__(self, c, d):
            self.c, self.d = c, d

        def chi2(self):
            return self.c

        def isDepthPositive(self):
            return self.d

    def run(cond, e, close):
        py = cond.replace("e->", "e.").replace("&&", " and ").replace("||", " or ").replace("!bClose", "(not bClose)").replace("!e.", "not e.")
        py = re.sub(r"(\d+\.\d+)f\*chi2Mono2", r"float(f32(\1) * f32(chi2Mono2))", py)  # a float times a float: a float product, widened by the comparison
        return bool(eval(py, {"e": e, "bClose": close, "f32": f32, **{k: float(v) for k, v in consts.items()}}))
    grid = [0.0, 5.99, float(f32(5.991)), np.nextafter(float(f32(5.991)), 9.0), 5.991, 7.0, 7.8, float(f32(7.815)), np.nextafter(float(f32(7.815)), 9.0),
            1.5 * 5.991, float(f32(1.5) * f32(5.991)), np.nextafter(float(f32(1.5) * f32(5.991)), 99.0), 8.9865, 8.98650001, 20.0]
    for c in grid:
        for close in (False, True):
            for depth in (False, True):
                assert run(conds[0][0], Edge(c, depth), close) == bool(m.erase_predicate([c], [True], [close], [depth])[0][0]), (c, close, depth)
        assert run(conds[1][0], Edge(c, True), False) == bool(m.erase_predicate([c], [False], [False], [True])[0][0]), c


def test_lambda_iterations_and_fail_predicate_are_the_references_text():
    body = _liba()
    assert re.search(r"int maxOpt=10;\s*int opt_it=(\d+);\s*if\(bLarge\)\s*\{\s*maxOpt=25;\s*opt_it=(\d+);", body)
    its = re.search(r"int opt_it=(\d+);\s*if\(bLarge\)\s*\{\s*maxOpt=25;\s*opt_it=(\d+);", body)
    assert {False: int(its.group(1)), True: int(its.group(2))} == m.ITERATIONS
    lam = re.search(r"if\(bLarge\)\s*\{[^}]*setUserLambdaInit\(([0-9.e+-]+)\)[^}]*\}\s*else\s*\{[^}]*setUserLambdaInit\(([0-9.e+-]+)\)", body)
    assert {True: float(lam.group(1)), False: float(lam.group(2))} == m.LAMBDA_INIT
    assert "OptimizationAlgorithmLevenberg" in body and "BlockSolverX" in body and "vPoint->setMarginalized(true)" in body
    # err and err_end are floats; the flag reaches the optimizer only after optimize() has returned
    seq = re.search(r"optimizer\.computeActiveErrors\(\);.*?float err = optimizer\.activeRobustChi2\(\);.*?optimizer\.optimize\(opt_it\);.*?"
                    r"float err_end = optimizer\.activeRobustChi2\(\);\s*if\(pbStopFlag\)\s*optimizer\.setForceStopFlag\(pbStopFlag\);", body, re.S)
    assert seq
    cond = re.search(r"if\((\(2\*err < err_end \|\| isnan\(err\) \|\| isnan\(err_end\)\) && !bLarge)\)", body).group(1)
    py = cond.replace("||", " or ").replace("&&", " and ").replace("!bLarge", "(not bLarge)").replace("2*err", "f32(2) * err")
    cases = [(10.0, 19.0), (10.0, 20.0), (10.0, 20.000001), (10.0, 21.0), (1.0 + 0.6 * 2.0 ** -23, 2.0 + 0.7 * 2.0 ** -22), (float("nan"), 1.0),
             (1.0, float("nan")), (0.0, 0.0), (1e30, 1e38)]
    for e0, e1 in cases:
        for large in (False, True):
            with np.errstate(over="ignore", invalid="ignore"):
                want = bool(eval(py, {"err": f32(e0), "err_end": f32(e1), "bLarge": large, "isnan": np.isnan, "f32": f32}))
            assert want == m.fail_predicate(e0, e1, large), (e0, e1, large)
    # the fail return comes before the stamps are reset and before anything is written back
    tail = body[body.index(cond):]
    assert tail.index("return;") < tail.index("mnBAFixedForKF = 0") < tail.index("SetVelocity") < tail.index("SetNewBias(IMU::Bias(b[3],b[4],b[5],b[0],b[1],b[2]))") \
        < tail.index("SetPose(Tcw") < tail.index("SetWorldPos") < tail.index("UpdateNormalAndDepth()") < tail.index("IncreaseChangeIndex()")
