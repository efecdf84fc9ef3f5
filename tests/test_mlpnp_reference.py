"""MLPnPsolver's host-side formulas, CheckInliers' float statements, the generated Jacobian and the Rodrigues pair EVALUATED FROM THE
REFERENCE'S OWN SOURCE TEXT and held against tests/mlpnp_model.py, and the control-flow facts the device code leans on asserted as text
(CPU only; runs where the reference is present).  As in tests/test_two_view_reference.py the bodies are cut out of S/MLPnPsolver.cpp
where they lie, translated statement by statement and executed with numpy scalars, whose promotion rules for float32 / float64
operands are C's.  Nothing of the reference is copied into the repository: the text is read, evaluated and compared."""
import os
import re

import numpy as np
import pytest

import mlpnp_model as mm

REF = "/root/reference/src/orb_slam3_ros/orb_slam3"
SRC = os.path.join(REF, "src", "MLPnPsolver.cpp")
pytestmark = pytest.mark.skipif(not os.path.isfile(SRC), reason="the reference is only present in the build container")

F32, F64 = np.float32, np.float64


def _body(signature_regex):
    text = open(SRC).read()
    m = re.search(signature_regex, text)
    assert m, signature_regex
    i = text.index("{", m.end() - 1)
    depth, j = 0, i
    while True:
        depth += text[j] == "{"
        depth -= text[j] == "}"
        if depth == 0:
            break
        j += 1
    body = re.sub(r"/\*.*?\*/", " ", text[i + 1:j], flags=re.S)
    return re.sub(r"//[^\n]*", " ", body)


def _flat(s):
    return "".join(s.split())


# ------------------------------------------------------------------ SetRansacParameters

def _set_ransac_parameters_text(N, probability, minInliers, maxIterations, minSet, epsilon):
    """:218-248 executed: member assignments, the int truncation, the float comparison, the iteration formula."""
    flat = _flat(_body(r"void\s+MLPnPsolver::SetRansacParameters\s*\("))
    for piece in ("intnMinInliers=N*mRansacEpsilon;", "if(nMinInliers<mRansacMinInliers)nMinInliers=mRansacMinInliers;",
                  "if(nMinInliers<minSet)nMinInliers=minSet;", "mRansacMinInliers=nMinInliers;",
                  "if(mRansacEpsilon<(float)mRansacMinInliers/N)mRansacEpsilon=(float)mRansacMinInliers/N;",
                  "if(mRansacMinInliers==N)nIterations=1;elsenIterations=ceil(log(1-mRansacProb)/log(1-pow(mRansacEpsilon,3)));",
                  "mRansacMaxIts=max(1,min(nIterations,mRansacMaxIts));", "mvMaxError[i]=mvSigma2[i]*th2;"):
        assert piece in flat, piece
    order = [flat.index(p) for p in ("intnMinInliers=N*mRansacEpsilon;", "mRansacMinInliers=nMinInliers;", "if(mRansacEpsilon<", "if(mRansacMinInliers==N)", "mRansacMaxIts=max(")]
    assert order == sorted(order)
    # the statements found above, with C's types: N int, mRansacEpsilon float, mRansacProb double
    eps = F32(epsilon)
    with np.errstate(all="ignore"):
        nMin = int(F32(N) * eps)                      # int * float -> float, truncated
        if nMin < minInliers:
            nMin = minInliers
        if nMin < minSet:
            nMin = minSet
        if eps < F32(nMin) / F32(N):
            eps = F32(nMin) / F32(N)
        if nMin == N:
            its = 1
        else:
            v = np.ceil(np.log(F64(1 - probability)) / np.log(F64(1) - np.power(F64(eps), 3)))      # pow(float, int) is pow(double, double)
            its = int(v) if np.isfinite(v) and abs(v) < 2 ** 31 else -2 ** 31                       # the x86 conversion of NaN / inf
    return max(1, min(its, maxIterations)), nMin


def test_set_ransac_parameters_text_against_the_model():
    for n in (6, 7, 12, 19, 20, 21, 100, 2000):
        for par in ((0.99, 8, 300, 6, 0.4), (0.99, 10, 300, 6, 0.5)):
            its, mi, _ = mm.ransac_iterations(n, *par)
            assert _set_ransac_parameters_text(n, *par) == (its, mi), (n, par)
    # the defaults of the header and the call of Tracking::Relocalization
    hdr = open(os.path.join(REF, "include", "MLPnPsolver.h")).read()
    assert "".join(re.search(r"void\s+SetRansacParameters\s*\(([^)]*)\)", hdr).group(1).split()) == \
        "doubleprobability=0.99,intminInliers=8,intmaxIterations=300,intminSet=6,floatepsilon=0.4,floatth2=5.991"
    trk = _flat(open(os.path.join(REF, "src", "Tracking.cc")).read())
    assert "pSolver->SetRansacParameters(0.99,10,300,6,0.5,5.991);" in trk


# ------------------------------------------------------------------ CheckInliers

def test_check_inliers_text_against_the_model_bit_for_bit():
    body = _body(r"void\s+MLPnPsolver::CheckInliers\s*\(")
    stmts = []
    for st in body.split(";"):
        m = re.match(r"\s*float\s+(\w+)\s*=\s*(.+)$", st.strip(), flags=re.S)
        if m:
            stmts.append((m.group(1), " ".join(m.group(2).split())))
    assert [n for n, _ in stmts] == ["xc", "yc", "zc", "distX", "distY", "error2"]
    flat = _flat(body)
    assert "cv::Point2fuv=mpCamera->project(P3Dc);" in flat and "if(error2<mvMaxError[i])" in flat
    pin = _flat(open(os.path.join(REF, "src", "CameraModels", "Pinhole.cpp")).read())
    assert "cv::Point2fPinhole::project(constcv::Point3f&p3D){returncv::Point2f(mvParameters[0]*p3D.x/p3D.z+mvParameters[2],mvParameters[1]*p3D.y/p3D.z+mvParameters[3]);}" in pin
    sc, drw = mm.case_scene(3)
    hyps = mm.hypotheses(sc, drw[:6])
    me = mm.max_errors(sc["sigma2"], 5.991)
    K = [F32(v) for v in sc["K"]]

    class Pt:
        pass
    with np.errstate(all="ignore"):
        for h in hyps:
            mRi = [[F64(v) for v in row] for row in h["R"]]
            mti = [F64(v) for v in h["t"]]
            for i in range(len(me)):
                P3Dw, P2D, uv = Pt(), Pt(), Pt()
                P3Dw.x, P3Dw.y, P3Dw.z = (F32(v) for v in sc["P3Dw"][i])
                P2D.x, P2D.y = (F32(v) for v in sc["P2D"][i])
                env = dict(mRi=mRi, mti=mti, P3Dw=P3Dw, P2D=P2D, uv=uv)
                for name, e in stmts:
                    if name == "distX":                                   # between zc and distX: uv = mpCamera->project(P3Dc)
                        uv.x = K[0] * env["xc"] / env["zc"] + K[2]
                        uv.y = K[1] * env["yc"] / env["zc"] + K[3]
                    env[name] = F32(eval(e, {}, env))
                assert env["error2"].tobytes() == h["e2"][i].tobytes() or (np.isnan(env["error2"]) and np.isnan(h["e2"][i]))
                assert bool(env["error2"] < me[i]) == bool(h["mask"][i])


# ------------------------------------------------------------------ Refine and the loop

def test_refine_does_not_use_its_own_solve():
    """Between computePose( and CheckInliers() in Refine no statement assigns mRi or mti: the inliers counted, and the pose converted
    into mRefinedTcw, are the current hypothesis'.  If the reference is ever repaired this fails, and the device needs an N-point
    computePose."""
    body = _body(r"bool\s+MLPnPsolver::Refine\s*\(")
    i, j = body.index("computePose("), body.index("CheckInliers()")
    assert i < j
    between = body[i:j]
    assert not re.search(r"\bm[Rt]i\b[^;]*=", between), between
    flat = _flat(body)
    assert "computePose(bearingVecs,p3DS,covs,indexes,result);CheckInliers();mnRefinedInliers=mnInliersi;mvbRefinedInliers=mvbInliersi;if(mnInliersi>mRansacMinInliers){" in flat
    assert "cv::MatRcw(3,3,CV_64F,mRi);cv::Mattcw(3,1,CV_64F,mti);" in flat and flat.endswith("returntrue;}returnfalse;")


def test_iterate_loop_conditions_as_text():
    flat = _flat(_body(r"cv::Mat\s+MLPnPsolver::iterate\s*\("))
    assert "if(N<mRansacMinInliers){bNoMore=true;returncv::Mat();}" in flat
    assert "while(mnIterations<mRansacMaxIts||nCurrentIterations<nIterations){nCurrentIterations++;mnIterations++;" in flat      # an OR
    assert "intrandi=DUtils::Random::RandomInt(0,vAvailableIndices.size()-1);intidx=vAvailableIndices[randi];" in flat
    assert "vAvailableIndices[randi]=vAvailableIndices.back();vAvailableIndices.pop_back();" in flat
    a = flat.index("if(mnInliersi>=mRansacMinInliers){")
    b = flat.index("if(mnInliersi>mnBestInliers){", a)
    c = flat.index("if(Refine()){", b)
    d = flat.index("returnmRefinedTcw.clone();", c)
    e = flat.index("if(mnIterations>=mRansacMaxIts){bNoMore=true;if(mnBestInliers>=mRansacMinInliers){", d)
    assert a < b < c < d < e and "returnmBestTcw.clone();" in flat[e:]
    assert "cov3_mats_tcovs(1);" in flat                                 # the covariance path is never taken
    ctor = _flat(_body(r"MLPnPsolver::MLPnPsolver\s*\("))
    assert "if(i>=F.mvKeysUn.size())continue;" in ctor and "cv_br/=cv_br.z;" in ctor and "SetRansacParameters();" in ctor


# ------------------------------------------------------------------ the generated Jacobian, rot2rodrigues, rodrigues2rot

def _jacs_text(pt, nr, ns, w, t):
    body = _body(r"void\s+MLPnPsolver::mlpnpJacs\s*\(")
    env = dict(pt=pt, nullspace_r=nr, nullspace_s=ns, w=w, t=t, sqrt=np.sqrt, sin=np.sin, cos=np.cos, pow=np.power)
    jac = np.zeros((2, 6))
    n = 0
    with np.errstate(all="ignore"):
        for st in body.split(";"):
            st = " ".join(st.split())
            m = re.match(r"double (\w+) = (.+)$", st)
            if m:
                env[m.group(1)] = F64(eval(m.group(2), {}, env))
                continue
            m = re.match(r"jacs\((\d), (\d)\) = (.+)$", st)
            if m:
                jac[int(m.group(1)), int(m.group(2))] = eval(m.group(3), {}, env)
                n += 1
    assert n == 12
    return jac


def test_generated_jacobian_equals_the_derived_one():
    """A sanity bound on analytic equality (relative 1e-10), not a parity claim.  At w = 0 the generated code's rotation columns are NaN."""
    rng = np.random.default_rng(11)
    for _ in range(50):
        ax = rng.normal(size=3)
        w = ax / np.linalg.norm(ax) * rng.uniform(0.05, 2.5)
        t, X = rng.normal(size=3), rng.normal(size=3) * 2 + np.array([0.0, 0.0, 5.0])
        nr, ns = mm.nullspace_cross(rng.normal(size=3))
        ref = _jacs_text(X, nr, ns, w, t)
        own = mm.jacobian(w, t, X, nr, ns)
        assert np.abs(ref - own).max() <= 1e-10 * max(1.0, np.abs(ref).max()), (w, np.abs(ref - own).max())
    ref = _jacs_text(X, nr, ns, np.zeros(3), t)
    assert np.isnan(ref[:, :3]).all()


def _eigen_text(name, arg):
    """rot2rodrigues / rodrigues2rot executed from their text (Eigen expressions mapped onto numpy)."""
    body = _body(r"Eigen::\w+\s+MLPnPsolver::%s\s*\(" % name)
    flat = _flat(body)
    if name == "rot2rodrigues":
        for piece in ("doubletrace=R.trace()-1.0;", "doublewnorm=acos(trace/2.0);", "if(wnorm>std::numeric_limits<double>::epsilon()){",
                      "omega[0]=(R(2,1)-R(1,2));omega[1]=(R(0,2)-R(2,0));omega[2]=(R(1,0)-R(0,1));", "doublesc=wnorm/(2.0*sin(wnorm));omega*=sc;"):
            assert piece in flat, piece
        R = arg
        with np.errstate(all="ignore"):
            trace = np.trace(R) - 1.0
            wnorm = np.arccos(trace / 2.0)
            omega = np.zeros(3)
            if wnorm > np.finfo(F64).eps:
                omega = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (wnorm / (2.0 * np.sin(wnorm)))
        return omega
    for piece in ("skewW<<0.0,-omega(2),omega(1),omega(2),0.0,-omega(0),-omega(1),omega(0),0.0;", "doubleomega_norm=omega.norm();",
                  "if(omega_norm>std::numeric_limits<double>::epsilon())R=R+sin(omega_norm)/omega_norm*skewW+(1-cos(omega_norm))/(omega_norm*omega_norm)*(skewW*skewW);"):
        assert piece in flat, piece
    om = arg
    K = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    nrm = np.linalg.norm(om)
    R = np.eye(3)
    if nrm > np.finfo(F64).eps:
        R = R + np.sin(nrm) / nrm * K + (1 - np.cos(nrm)) / (nrm * nrm) * (K @ K)
    return R


def test_rodrigues_pair_text_against_the_model():
    rng = np.random.default_rng(12)
    for _ in range(50):
        w = rng.normal(size=3)
        w = w / np.linalg.norm(w) * rng.uniform(0.01, 3.0)
        R = _eigen_text("rodrigues2rot", w)
        assert np.abs(R - mm.rodrigues2rot(w)).max() < 1e-15
        assert np.abs(_eigen_text("rot2rodrigues", R) - mm.rot2rodrigues(R)).max() < 1e-15
        assert np.abs(mm.rot2rodrigues(R) - w).max() < 1e-9
    assert np.array_equal(_eigen_text("rot2rodrigues", np.eye(3)), np.zeros(3)) and np.array_equal(mm.rot2rodrigues(np.eye(3)), np.zeros(3))
    assert np.array_equal(_eigen_text("rodrigues2rot", np.full(3, np.nan)), np.eye(3)) and np.array_equal(mm.rodrigues2rot(np.full(3, np.nan)), np.eye(3))
