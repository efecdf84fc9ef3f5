"""What the model of InertialOptimization restates, taken from the reference's own text at test time and executed against the model
(tests/inertial_init_model.py):
  EdgeInertialGS::computeError / linearizeOplus, its constructor     S/G2oTypes.cc:802-927
  GDirection::Update, VertexScale::oplusImpl                         I/G2oTypes.h:254-314
  EdgePriorAcc / EdgePriorGyro::computeError / linearizeOplus        I/G2oTypes.h:784-830, S/G2oTypes.cc:971-983
  the four overloads' vertex and solver set-up                       S/Optimizer.cc:5344-5958
The bodies are cut out and translated by the translator of tests/test_pose_inertial_reference.py (imported, not edited) after a few more
text-level rules for what these bodies add (a dynamic Eigen::MatrixXd, element assignment `M(i,j) = x`); the set-up statements
(`setFixed`, `setUserLambdaInit`, `int its`, the algorithm's class) are turned into assignments and executed for every value of bMono,
bFixedVel and priorG.  Nothing of the reference is stored."""
import os
import re

import numpy as np
import pytest

import inertial_init_model as m
import pose_inertial_model as pm
import test_pose_inertial_reference as tpr
import test_reference_formulas as rf

pytestmark = pytest.mark.skipif(not os.path.isdir(rf.REF), reason="the reference is only present in the build container")
G2OTYPES, OPTIMIZER = tpr.G2OTYPES, tpr.OPTIMIZER
G2OTYPES_H = os.path.join(rf.REF, "include", "G2oTypes.h")
E = tpr.E
OVERLOADS = {
    1: r"void Optimizer::InertialOptimization\(Map \*pMap, Eigen::Matrix3d &Rwg, double &scale, Eigen::Vector3d &bg, Eigen::Vector3d &ba, bool bMono[^)]*\)",
    2: r"void Optimizer::InertialOptimization\(Map \*pMap, Eigen::Vector3d &bg, Eigen::Vector3d &ba, float priorG, float priorA\)",
    3: r"void Optimizer::InertialOptimization\(vector<KeyFrame\*> vpKFs, Eigen::Vector3d &bg, Eigen::Vector3d &ba, float priorG, float priorA\)",
    4: r"void Optimizer::InertialOptimization\(Map \*pMap, Eigen::Matrix3d &Rwg, double &scale\)",
}


class B(E):
    """a Jacobian block: a 3-vector assigned to a 3 x 1 block is a column"""

    def setblock(self, i, j, r, c, val):
        self.a[i:i + r, j:j + c] = np.asarray(val.a if isinstance(val, E) else val, np.float64).reshape(r, c)


def _gravity():
    gv = re.search(r"const float GRAVITY_VALUE\s*=\s*([0-9.]+)", open(os.path.join(rf.REF, "include", "ImuTypes.h")).read())
    return float(np.float32(float(gv.group(1))))


def _gs_fix(body):
    body = re.sub(r"(?:const\s+)?Eigen::MatrixXd\s+(\w+)\s*=", r"\1 =", body)
    body = body.replace("Eigen::MatrixXd::Zero(3,2)", "Zero(3,2)")
    return re.sub(r"\b(\w+)\((\d),(\d)\)\s*=(?!=)", r"\1.a[\2,\3] =", body)


def _gs_env(P, e, S, variant="kernel"):
    """the vertices of edge e as the translated bodies name them"""
    env, _, _ = tpr._edge_env(pm.make_scene(pm.FORM_FRAME, 4, 5))          # the SO3 functions, Skew, Converter from the text
    K, Ed = P["keyframes"], P["edges"][e]
    pre = Ed["preint"]
    dR, dV, dP = pm.preint_deltas(pre, S["bg"], S["ba"], variant)
    V = lambda k: type("V", (), {"Rwb": E(K["R"][k].astype(np.float64)), "twb": E(K["t"][k].astype(np.float64))})()
    D = lambda k: E(pre[k].astype(np.float64))
    G = _gravity()
    assert G == m.GRAVITY
    env.update({"VP1": V(Ed["k1"]), "VP2": V(Ed["k2"]), "VV1": E(S["v"][Ed["k1"]]), "VV2": E(S["v"][Ed["k2"]]), "VG": E(S["bg"]), "VA": E(S["ba"]),
                "VGDir": type("GD", (), {"Rwg": E(S["Rwg"])})(), "VS": float(S["s"]), "b": None, "dt": float(pre["dT"]),
                "gI": E(np.array([0.0, 0.0, -G])), "g": E(S["Rwg"] @ np.array([0.0, 0.0, -G])),
                "mpInt": type("M", (), {"GetDeltaRotation": staticmethod(lambda b: E(dR)), "GetDeltaVelocity": staticmethod(lambda b: E(dV)),
                                         "GetDeltaPosition": staticmethod(lambda b: E(dP)), "GetDeltaBias": staticmethod(lambda b: None)}),
                "JRg": D("JRg"), "JVg": D("JVg"), "JPg": D("JPg"), "JVa": D("JVa"), "JPa": D("JPa"),
                "dbg": E(S["bg"] - pre["bg"].astype(np.float64)), "IMU": type("I", (), {"GRAVITY_VALUE": G}),
                "Zero": lambda r, c: E(np.zeros((r, c))), "np": np, "B": B})
    return env


def _state(P, bias):
    P = dict(P)
    P["bg"] = (P["truth"]["bg"] + bias * np.array([1.0, -0.5, 0.25])).astype(np.float32)
    P["ba"] = (P["truth"]["ba"] + 10 * bias * np.array([0.3, 1.0, -0.6])).astype(np.float32)
    return P, m.initial_state(P)


@pytest.mark.parametrize("bias", [0.0, 2e-3])
def test_edge_inertial_gs_is_the_references_text(bias):
    P, S = _state(m.build_case("fork"), bias)
    err_body = tpr._translate(_gs_fix(rf._body(G2OTYPES, r"void EdgeInertialGS::computeError\(\)")), {})
    lin_body = tpr._translate(_gs_fix(rf._body(G2OTYPES, r"void EdgeInertialGS::linearizeOplus\(\)")), {})
    lin_body = [l for l in lin_body if not re.match(r"\s*(db = |dbg = )", l)]               # the Bias object's members: dbg is handed in
    assert any(l.strip().startswith("g = VGDir.Rwg*gI") for l in err_body)
    for e in range(len(P["edges"])):
        ns = dict(tpr.BASE_ENV)
        ns.update(_gs_env(P, e, S))
        exec("\n".join(["def computeError():"] + ["    " + l for l in err_body] + ["    return _error"]), ns)
        exec("\n".join(["def linearizeOplus():", "    _jacobianOplus = [B(np.zeros((9, k))) for k in (6, 3, 3, 3, 6, 3, 2, 1)]"] +
                       ["    " + l for l in lin_body] + ["    return _jacobianOplus"]), ns)
        want = m.edge_block(P, S, e)
        got = ns["computeError"]().a
        assert np.abs(got - want[:, 15]).max() <= 1e-15 * max(1.0, np.abs(want[:, 15]).max())
        Js = ns["linearizeOplus"]()
        # the pose blocks belong to fixed vertices; the model keeps [v1 | v2 | bg | ba | gdir | s]
        J = np.hstack([Js[k].a for k in (1, 5, 2, 3, 6, 7)])
        assert J.shape == (9, 15)
        assert np.abs(J - want[:, :15]).max() <= 1e-14 * np.abs(want[:, :15]).max()
        assert np.array_equal(J == 0, want[:, :15] == 0)                                    # the same blocks are filled


def test_edge_inertial_gs_conditions_its_information_as_edge_inertial_does():
    """orbg_imu_information restates the EdgeInertial constructor; the EdgeInertialGS one must be the same text but for the names of the
    gravity vector and the vertex count"""
    norm = lambda b: re.sub(r"\s+", "", b)
    a = norm(rf._body(G2OTYPES, r"EdgeInertial::EdgeInertial\(IMU::Preintegrated \*pInt\)[^{]*"))
    b = norm(rf._body(G2OTYPES, r"EdgeInertialGS::EdgeInertialGS\(IMU::Preintegrated \*pInt\)[^{]*"))
    assert "resize(6);g<<0,0,-IMU::GRAVITY_VALUE;" in a and "resize(8);gI<<0,0,-IMU::GRAVITY_VALUE;" in b
    assert a.replace("resize(6);g<<", "X") == b.replace("resize(8);gI<<", "X")


def test_vertex_updates_are_the_references_text():
    exp = tpr._so3()[0]
    upd, _ = tpr._function(G2OTYPES_H, r"GDirection\(Eigen::Matrix3d pRwg\): Rwg\(pRwg\)\{\}\s*void Update\(const double \*pu\)", "Update",
                           ["Rwg", "pu"], env={"ExpSO3": exp}, post=["return Rwg"])
    rng = np.random.default_rng(4)
    R0 = pm.exp_so3(rng.normal(size=3))
    for scale in (1e-7, 1e-2, 0.7):
        u = rng.normal(size=2) * scale
        assert np.abs(upd(E(R0), list(u)).a - m.gdir_oplus(R0, u)).max() <= 4e-16
    got = []
    op, src = tpr._function(G2OTYPES_H, r"class VertexScale[\s\S]*?virtual void oplusImpl\(const double \*update_\)", "oplusImpl", ["s", "update_"],
                            env={"exp": np.exp, "setEstimate": got.append}, pre=["estimate = lambda: s"])
    assert "estimate()*exp(*update_)" in src
    for s, u in ((1.0, 0.3), (2.5, -1e-3)):
        op(s, [u])
        assert got[-1] == m.scale_oplus(s, u)


def test_prior_edges_are_the_references_text():
    """error = bprior - estimate, Jacobian = +I (the sign the model and the kernel keep)"""
    hdr = open(G2OTYPES_H).read()
    for name, vertex in (("EdgePriorAcc", "VA"), ("EdgePriorGyro", "VG")):
        cls = hdr[hdr.index("class %s " % name):]
        body = cls[cls.index("void computeError()"):]
        body = body[body.index("{") + 1:body.index("}")]
        lines = tpr._translate(body, {})
        ns = dict(tpr.BASE_ENV)
        bias = np.array([0.01, -0.02, 0.03])
        ns.update({"bprior": E(np.zeros(3)), vertex: E(bias)})
        exec("\n".join(["def computeError():"] + ["    " + l for l in lines] + ["    return _error"]), ns)
        assert np.array_equal(ns["computeError"]().a, -bias)
        lin = tpr._translate(rf._body(G2OTYPES, r"void %s::linearizeOplus\(\)" % name), {})
        ns.update({"np": np, "B": B})
        exec("\n".join(["def linearizeOplus():", "    _jacobianOplusXi = B(np.zeros((3, 3)))"] + ["    " + l for l in lin] + ["    return _jacobianOplusXi"]), ns)
        assert np.array_equal(ns["linearizeOplus"]().a, np.eye(3))
    # the model: with that Jacobian the right-hand side -J^T W e is +prior * bias
    P, S = _state(m.build_case("n10_mono"), 0.0)
    G = m.Graph(P)
    d = m.linearise(P, G, S, "kernel")["rc"] - m.linearise(dict(P, prior_g=0.0, prior_a=0.0), G, S, "kernel")["rc"]
    assert np.allclose(d[0:3], P["prior_g"] * np.eye(3) @ S["bg"], rtol=1e-9) and np.allclose(d[3:6], P["prior_a"] * np.eye(3) @ S["ba"], rtol=1e-9)


def _setup(form, bMono, bFixedVel, priorG):
    """the vertex and solver set-up of an overload, executed from its text"""
    body = rf._body(OPTIMIZER, OVERLOADS[form])
    body = body[:body.index("optimizer.initializeOptimization()")]
    stmts = []
    its = re.search(r"int its = (\d+);", body)
    stmts.append("its = %s" % its.group(1))
    alg = re.search(r"new g2o::OptimizationAlgorithm(\w+)\(solver_ptr\)", body)
    stmts.append("algorithm = %r" % alg.group(1))
    stmts.append("user_lambda = None")
    text = re.sub(r"if\s*\((\w+)\)\s*(\w+)->setFixed\(true\);\s*else\s*\2->setFixed\(false\);", r"fixed['\2'] = bool(\1);", body)
    text = re.sub(r"if\s*\(priorG!=0\.f\)\s*solver->setUserLambdaInit\(([^)]*)\);", r"user_lambda = \1 if priorG != 0 else None;", text)
    text = re.sub(r"solver->setUserLambdaInit\(([^)]*)\);", r"user_lambda = \1;", text)
    text = re.sub(r"(\w+)->setFixed\(([^;]*)\);", lambda k: "fixed['%s'] = %s;" % (k.group(1), k.group(2).replace("!", " not ").replace("true", "True").replace("false", "False")), text)
    for s in text.split(";"):
        s = s.strip()
        if s.startswith("fixed[") or s.startswith("user_lambda ="):
            stmts.append(s)
    ns = {"fixed": {}, "bMono": bMono, "bFixedVel": bFixedVel, "priorG": priorG}
    exec("\n".join(stmts), ns)
    return ns, body


@pytest.mark.parametrize("form", [1, 2, 3, 4])
def test_overload_setup_is_the_references_text(form):
    for bMono in (False, True):
        for bFixedVel in (False, True):
            for priorG in (0.0, 1e2):
                ns, body = _setup(form, bMono, bFixedVel, priorG)
                want = m.form_problem(form, bMono=bMono, bFixedVel=bFixedVel, priorG=priorG)
                fx = ns["fixed"]
                assert fx["VP"] is True
                assert (not fx["VV"], not fx["VG"] and not fx["VA"], not fx["VGDir"], not fx["VS"]) == \
                    (want["free_velocity"], want["free_bias"], want["free_gdir"], want["free_scale"])
                assert fx["VG"] == fx["VA"]
                assert ns["its"] == want["iterations"]
                assert {"Levenberg": m.LM, "GaussNewton": m.GN}[ns["algorithm"]] == want["algorithm"]
                assert (ns["user_lambda"] or 0.0) == want["lambda_init"]
                assert ("EdgePriorAcc" in body and "EdgePriorGyro" in body) == want["with_priors"]
    body = rf._body(OPTIMIZER, OVERLOADS[form])
    # every bias vertex is constructed from vpKFs.front()
    assert len(re.findall(r"new VertexGyroBias\(vpKFs\.front\(\)\)", body)) == 1 and len(re.findall(r"new VertexAccBias\(vpKFs\.front\(\)\)", body)) == 1
    assert not re.search(r"new Vertex(?:Gyro|Acc)Bias\((?!vpKFs\.front\(\)\))", body)
    # covInertial and bGauss are never read
    assert "covInertial" not in body and "bGauss" not in body
    # gravity and scale start from the caller's values, or from I and 1 where they are fixed
    if form in (1, 4):
        assert "new VertexGDir(Rwg)" in body and "new VertexScale(scale)" in body
    else:
        assert "new VertexGDir(Eigen::Matrix3d::Identity())" in body and "new VertexScale(1.0)" in body
    # the edge filter, and the SetNewBias side effect of the first three
    assert re.search(r"if\(pKFi->mPrevKF && pKFi->mnId<=maxKFid\)\s*\{\s*if\(pKFi->isBad\(\) \|\| pKFi->mPrevKF->mnId>maxKFid\)\s*continue;", body)
    assert ("pKFi->mpImuPreintegrated->SetNewBias(pKFi->mPrevKF->GetImuBias())" in body) == (form != 4)
    assert "new EdgeInertialGS(pKFi->mpImuPreintegrated)" in body
    # the vertex filter: commented out in the list overload
    kept = "if(pKFi->mnId>maxKFid)" in body[:body.index("VertexPose * VP")]
    assert kept == (form != 3)
    # the write-back
    if form != 4:
        assert re.search(r"pKFi->SetVelocity\(Converter::toCvMat\(Vw\)\);\s*if \(cv::norm\(pKFi->GetGyroBias\(\)-cvbg\)>0\.01\)", body)
        assert re.search(r"IMU::Bias b \(vb\[3\],vb\[4\],vb\[5\],vb\[0\],vb\[1\],vb\[2\]\)", body) and "Reintegrate()" in body
    else:
        assert "SetVelocity" not in body and "SetNewBias" not in body
