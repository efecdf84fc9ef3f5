"""What the model of PoseInertialOptimization restates, taken from the reference's own text at test time and executed against the model
(tests/pose_inertial_model.py):
  ExpSO3, LogSO3, RightJacobianSO3, InverseRightJacobianSO3     S/G2oTypes.cc:986-1063
  ImuCamPose::Update                                            S/G2oTypes.cc:192-220
  EdgeInertial::computeError / linearizeOplus                   S/G2oTypes.cc:720-800
  EdgePriorPoseImu::computeError / linearizeOplus               S/G2oTypes.cc:940-969
  Optimizer::Marginalize                                        S/Optimizer.cc:5228-5308
  the threshold tables, Huber deltas and cut-offs               S/Optimizer.cc:7603-8424, I/G2oTypes.h:703-719, I/ImuTypes.h:25
The bodies are cut out with the transliterator's `_body` (tests/test_reference_formulas.py, imported, not edited).  Its statement
translator handles scalar C++; these bodies are Eigen expressions, so each statement goes through a few text-level rules here
(declared types dropped, `->estimate()` and `->` flattened, `<<` initialisers, `.block<r,c>(i,j)`, `if / else return`) and is executed
over a small Eigen stand-in (`*` is the matrix product between matrices, `.transpose()`, `(i,j)`); the formulas, the branch conditions,
their constants and the order of the blocks are the text's.  Nothing of the reference is stored."""
import os
import re

import numpy as np
import pytest

import pose_inertial_model as pm
import test_reference_formulas as rf

pytestmark = pytest.mark.skipif(not os.path.isdir(rf.REF), reason="the reference is only present in the build container")
G2OTYPES = os.path.join(rf.REF, "src", "G2oTypes.cc")
OPTIMIZER = os.path.join(rf.REF, "src", "Optimizer.cc")


class E:
    """Eigen::Matrix / Vector as far as these bodies use them"""
    __array_priority__ = 100

    def __init__(self, a):
        self.a = np.array(a.a if isinstance(a, E) else a, np.float64)

    def _v(self, o):
        return o.a if isinstance(o, E) else o

    def __mul__(self, o):
        if isinstance(o, E) and self.a.ndim >= 1 and o.a.ndim >= 1:
            return E(self.a @ o.a)
        return E(self.a * self._v(o))

    def __rmul__(self, o):
        return E(o * self.a)

    def __add__(self, o):
        return E(self.a + self._v(o))

    def __sub__(self, o):
        return E(self.a - self._v(o))

    def __neg__(self):
        return E(-self.a)

    def __truediv__(self, o):
        return E(self.a / o)

    def transpose(self):
        return E(self.a.T)

    def __getitem__(self, i):
        return float(self.a[i])

    def __call__(self, i, j):
        return float(self.a[i, j])

    def setblock(self, i, j, r, c, val):
        self.a[i:i + r, j:j + c] = val.a if isinstance(val, E) else val


def _cat(*parts):
    return E(np.concatenate([np.atleast_1d(p.a if isinstance(p, E) else p) for p in parts]))


def _mat(vals, shape):
    return E(np.array(vals, np.float64).reshape(shape))


BASE_ENV = {"E": E, "_cat": _cat, "_mat": _mat, "sqrt": np.sqrt, "sin": np.sin, "cos": np.cos, "acos": np.arccos, "fabs": abs,
            "I3": E(np.eye(3))}
TYPES = r"(?:const\s+)?(?:Eigen::Matrix3d|Eigen::Vector3d|Eigen::Matrix<[^>]*>|double)\s*&?\s*"


def _translate(body, shapes):
    """statements of a reference body -> Python source; `shapes` gives the shape of every variable filled with `<<`"""
    body = re.sub(r"\bif\s*\(([^;{]*?)\)\s*return\s+([^;]*);", r"if \1 :: return \2;", body)      # one-line early returns
    out, indent = [], 0
    # braces of if / else blocks become indentation
    tokens = re.split(r"([;{}])", body)
    stmt = ""
    for tok in tokens:
        if tok == ";":
            s = stmt.strip()
            stmt = ""
            if not s:
                continue
            out.append("    " * indent + s)
        elif tok == "{":
            s = stmt.strip()
            stmt = ""
            out.append("    " * indent + s + " {")
            indent += 1
        elif tok == "}":
            indent -= 1
            stmt = ""
        else:
            stmt += tok
    py = []
    for ln in out:
        pad, s = ln[: len(ln) - len(ln.lstrip())], ln.strip()
        s = s.replace("->estimate()", "").replace("->", ".").replace("Eigen::Matrix3d::Identity()", "I3")
        s = re.sub(r"(\d)f\b", r"\1", s).replace("||", " or ").replace("&&", " and ")
        if re.match(r"if\s*\(its", s):
            continue
        if "static_cast" in s or s.startswith("const IMU::Bias") or ".setZero()" in s or s.startswith("its") or s.startswith("NormalizeRotation"):
            continue                                                     # vertex casts, Bias objects, zeroing; its / NormalizeRotation: see test_update
        m = re.match(r"(?:else\s+)?if\s*\((.*)\)\s*\{$", s)
        if m:
            py.append(pad + ("elif " if s.startswith("else") else "if ") + m.group(1) + ":")
            continue
        if s == "else {":
            py.append(pad + "else:")
            continue
        m = re.match(r"if (.*) :: return (.*)$", s)
        if m:
            py.append(pad + "if %s: return %s" % (m.group(1), m.group(2)))
            continue
        m = re.match(r"else\s+return\s+(.*)$", s)
        if m:
            py.append(pad + "return " + m.group(1))
            continue
        m = re.match(r"else\s+(.*)$", s)
        if m and not s.startswith("else {"):
            s = m.group(1)
        m = re.match(r"(\w+)\s*<<\s*(.*)$", s, re.S)
        if m:
            name, vals = m.group(1), m.group(2)
            if name in shapes:
                py.append(pad + "%s = _mat([%s], %r)" % (name, vals, shapes[name]))
            else:
                py.append(pad + "%s = _cat(%s)" % (name, vals))
            continue
        m = re.match(r"(\w+(?:\[\d+\])?)\.block<(\d+),(\d+)>\((\d+),(\d+)\)\s*=\s*(.*)$", s, re.S)
        if m:
            py.append(pad + "%s.setblock(%s, %s, %s, %s, %s)" % (m.group(1), m.group(4), m.group(5), m.group(2), m.group(3), m.group(6)))
            continue
        m = re.match(TYPES + r"(\w+(?:\s*,\s*\w+)*)\s*$", s)
        if m:
            continue                                                     # a declaration without a value
        s = re.sub(r"^" + TYPES, "", s)
        py.append(pad + s)
    return [l.replace("::", ".") for l in py]


def _function(path, sig, name, args, shapes=(), env=None, pre=(), post=(), fix=lambda b: b):
    src = ["def %s(%s):" % (name, ", ".join(args))] + ["    " + l for l in list(pre) + _translate(fix(rf._body(path, sig)), dict(shapes)) + list(post)]
    ns = dict(BASE_ENV)
    ns.update(env or {})
    exec("\n".join(src), ns)
    return ns[name], "\n".join(src)


def _so3():
    W = {"W": (3, 3)}
    exp, _ = _function(G2OTYPES, r"Eigen::Matrix3d ExpSO3\(const double x, const double y, const double z\)", "ExpSO3", ["x", "y", "z"], W,
                       env={"Converter": type("C", (), {"toMatrix3d": staticmethod(lambda m: m), "toCvMat": staticmethod(lambda m: m)}),
                            "IMU": type("I", (), {"NormalizeRotation": staticmethod(lambda m: m)})})
    log, _ = _function(G2OTYPES, r"Eigen::Vector3d LogSO3\(const Eigen::Matrix3d &R\)", "LogSO3", ["R"])
    rj, _ = _function(G2OTYPES, r"Eigen::Matrix3d RightJacobianSO3\(const double x, const double y, const double z\)", "RJ", ["x", "y", "z"], W)
    irj, _ = _function(G2OTYPES, r"Eigen::Matrix3d InverseRightJacobianSO3\(const double x, const double y, const double z\)", "IRJ", ["x", "y", "z"], W)
    return exp, log, rj, irj


def test_so3_functions_are_the_references_text():
    """both branches of each function: below and above its small-angle threshold (the float round trip of ExpSO3 is left out here as in
    the model's kernel variant: Converter and NormalizeRotation are the identity)"""
    exp, log, rj, irj = _so3()
    rng = np.random.default_rng(1)
    for scale in (1e-7, 3e-6, 2e-5, 1e-2, 1.0, 2.5):
        for _ in range(4):
            w = rng.normal(size=3)
            w *= scale / np.linalg.norm(w)
            # the same formulas; `W*sin(d)/d` is (W sin d) / d in the text and W (sin d / d) in the model: a rounding or two
            close = lambda a, b: np.abs(np.asarray(a) - b).max() <= 1e-15 * max(1.0, np.abs(b).max())
            assert close(exp(*w).a, pm.exp_so3(w))
            assert close(rj(*w).a, pm.right_jacobian_so3(w)) and close(irj(*w).a, pm.inv_right_jacobian_so3(w))
            R = pm.exp_so3(w)
            lg = log(E(R))
            assert close(lg.a if isinstance(lg, E) else lg, pm.log_so3(R))


def test_update_is_the_references_text():
    """ImuCamPose::Update: the body pose, then the camera pose of the one camera.  (`its`, and NormalizeRotation(Rwb), whose result :206
    discards, are dropped.)"""
    exp = _so3()[0]
    upd, _ = _function(G2OTYPES, r"void ImuCamPose::Update\(const double \*pu\)", "Update", ["self", "pu"], {"ur": (3,), "ut": (3,)},
                       env={"ExpSO3": lambda w: exp(w[0], w[1], w[2])},
                       pre=["twb, Rwb, Rcb, tcb, Rcw, tcw, i = self.twb, self.Rwb, self.Rcb, self.tcb, [None], [None], 0"],
                       post=["return Rwb, twb, Rcw[0], tcw[0]"],
                       fix=lambda body: re.sub(r"for\(int i=0; i<pCamera\.size\(\); i\+\+\)", "if(True)", body))
    P = pm.make_scene(pm.FORM_KF, 4, 3)
    s = pm.make_state(**{k: np.asarray(x, np.float64) for k, x in P["frame"].items()})
    Tcb = P["Tcb"].astype(np.float64)
    dx = np.random.default_rng(2).normal(size=15) * 0.01
    me = type("S", (), {"twb": E(s["t"]), "Rwb": E(s["R"]), "Rcb": [E(Tcb[:, :3])], "tcb": [E(Tcb[:, 3])]})()
    Rwb, twb, Rcw, tcw = upd(me, dx[:6])
    s2 = pm.oplus(s, dx)
    Rm, tm = pm.camera_pose(s2, Tcb)
    # the same products; numpy's order inside a product may differ from the text's by a rounding
    assert np.abs(Rwb.a - s2["R"]).max() <= 4e-16 and np.abs(twb.a - s2["t"]).max() <= 4e-16 * max(1.0, np.abs(s2["t"]).max())
    assert np.abs(Rcw.a - Rm).max() <= 4e-16 and np.abs(tcw.a - tm).max() <= 4e-16 * max(1.0, np.abs(tm).max())


def _edge_env(P, variant="kernel"):
    exp, log, rj, irj = _so3()
    cur = pm.make_state(**{k: np.asarray(x, np.float64) for k, x in P["frame"].items()})
    oth = pm.make_state(**{k: np.asarray(x, np.float64) for k, x in P["other"].items()})
    pre = P["preint"]
    dR, dV, dP = pm.preint_deltas(pre, oth["bg"], oth["ba"], variant)
    V = lambda s: type("V", (), {"Rwb": E(s["R"]), "twb": E(s["t"])})()
    D = lambda k: E(pre[k].astype(np.float64))
    env = {"VP1": V(oth), "VP2": V(cur), "VV1": E(oth["v"]), "VV2": E(cur["v"]), "VG1": E(oth["bg"]), "VA1": E(oth["ba"]),
           "LogSO3": lambda R: E(log(R)) if not isinstance(log(R), E) else log(R), "InverseRightJacobianSO3": lambda v: irj(v[0], v[1], v[2]),
           "RightJacobianSO3": lambda v: rj(v[0], v[1], v[2]), "Skew": lambda w: E(pm.skew(w.a)),
           "Converter": type("C", (), {"toMatrix3d": staticmethod(lambda m: m), "toVector3d": staticmethod(lambda m: m)}),
           "mpInt": type("M", (), {"GetDeltaRotation": staticmethod(lambda b: E(dR)), "GetDeltaVelocity": staticmethod(lambda b: E(dV)),
                                    "GetDeltaPosition": staticmethod(lambda b: E(dP)), "GetDeltaBias": staticmethod(lambda b: None)}),
           "b1": None, "dt": float(pre["dT"]), "JRg": D("JRg"), "JVg": D("JVg"), "JPg": D("JPg"), "JVa": D("JVa"), "JPa": D("JPa"),
           "dbg": E(oth["bg"] - pre["bg"].astype(np.float64))}
    g = re.search(r"g\s*<<\s*0\s*,\s*0\s*,\s*-IMU::GRAVITY_VALUE", open(G2OTYPES).read())
    assert g
    gv = re.search(r"const float GRAVITY_VALUE\s*=\s*([0-9.]+)", open(os.path.join(rf.REF, "include", "ImuTypes.h")).read())
    env["g"] = E(np.array([0.0, 0.0, -float(np.float32(float(gv.group(1))))]))
    return env, cur, oth


@pytest.mark.parametrize("bias_step", [0.0, 2e-3])
def test_edge_inertial_is_the_references_text(bias_step):
    P = pm.make_scene(pm.FORM_FRAME, 4, 5, bias_step=bias_step)
    env, cur, oth = _edge_env(P)
    err, _ = _function(G2OTYPES, r"void EdgeInertial::computeError\(\)", "computeError", [], env=env, pre=["_error = None"])
    src = "\n".join(["def computeError():"] + ["    " + l for l in _translate(rf._body(G2OTYPES, r"void EdgeInertial::computeError\(\)"), {})] + ["    return _error"])
    ns = dict(BASE_ENV)
    ns.update(env)
    exec(src, ns)
    want = pm.inertial_error(oth, cur, P["preint"])
    got = ns["computeError"]().a
    assert np.abs(got - want).max() <= 1e-15 * max(1.0, np.abs(want).max())
    body = _translate(rf._body(G2OTYPES, r"void EdgeInertial::linearizeOplus\(\)"), {})
    body = [l for l in body if not re.match(r"\s*(db = |dbg = )", l)]                     # the Bias object's members: dbg is handed in
    src = "\n".join(["def linearizeOplus():", "    _jacobianOplus = [E(np.zeros((9, k))) for k in (6, 3, 3, 3, 6, 3)]"] + ["    " + l for l in body] + ["    return _jacobianOplus"])
    ns["np"] = np
    exec(src, ns)
    J = np.hstack([j.a for j in ns["linearizeOplus"]()])
    Jm = pm.inertial_jacobian(oth, cur, P["preint"])
    assert J.shape == (9, 24)
    assert np.abs(J - Jm).max() <= 1e-14 * np.abs(Jm).max()
    assert np.array_equal(J == 0, Jm == 0)                                                  # the same blocks are filled


def test_edge_prior_is_the_references_text():
    P = pm.make_scene(pm.FORM_FRAME, 4, 7, prior_shift=1.0)
    env, cur, oth = _edge_env(P)
    pr = P["prior"]
    env.update({"VP": env["VP1"], "VV": env["VV1"], "VG": env["VG1"], "VA": env["VA1"], "Rwb": E(pr["Rwb"]), "twb": E(pr["twb"]),
                "vwb": E(pr["vwb"]), "bg": E(pr["bg"]), "ba": E(pr["ba"]), "np": np})
    ns = dict(BASE_ENV)
    ns.update(env)
    src = "\n".join(["def computeError():"] + ["    " + l for l in _translate(rf._body(G2OTYPES, r"void EdgePriorPoseImu::computeError\(\)"), {})] + ["    return _error"])
    exec(src, ns)
    prior = {"R": pr["Rwb"], "t": pr["twb"], "v": pr["vwb"], "bg": pr["bg"], "ba": pr["ba"]}
    want = pm.prior_error(oth, prior)
    assert np.abs(ns["computeError"]().a - want).max() <= 1e-15 * max(1.0, np.abs(want).max())
    body = _translate(rf._body(G2OTYPES, r"void EdgePriorPoseImu::linearizeOplus\(\)"), {})
    src = "\n".join(["def linearizeOplus():", "    _jacobianOplus = [E(np.zeros((15, k))) for k in (6, 3, 3, 3)]"] + ["    " + l for l in body] + ["    return _jacobianOplus"])
    exec(src, ns)
    J = np.hstack([j.a for j in ns["linearizeOplus"]()])
    assert np.abs(J - pm.prior_jacobian(oth, prior)).max() <= 1e-15


def test_tables_and_constants_are_read_from_the_text():
    txt = open(OPTIMIZER).read()
    kf = rf._body(OPTIMIZER, r"int Optimizer::PoseInertialOptimizationLastKeyFrame\(Frame \*pFrame, bool bRecInit\)")
    fr = rf._body(OPTIMIZER, r"int Optimizer::PoseInertialOptimizationLastFrame\(Frame \*pFrame, bool bRecInit\)")
    nums = lambda body, name: tuple(float(x.rstrip("f")) for x in re.search(name + r"\[4\]\s*=\s*\{([^}]*)\}", body).group(1).split(","))
    assert nums(kf, "chi2Mono") == pm.CHI2_MONO[pm.FORM_KF] and nums(fr, "chi2Mono") == pm.CHI2_MONO[pm.FORM_FRAME]
    assert nums(kf, "chi2Stereo") == pm.CHI2_STEREO and nums(fr, "chi2Stereo") == pm.CHI2_STEREO
    for body in (kf, fr):
        assert nums(body, "its") == (10.0, 10.0, 10.0, 10.0)
        assert re.search(r"thHuberMono\s*=\s*sqrt\(5\.991\)", body) and re.search(r"thHuberStereo\s*=\s*sqrt\(7\.815\)", body)
        assert re.search(r"chi2close\s*=\s*1\.5\*chi2Mono\[it\]", body) and re.search(r"mTrackDepth<10\.f", body)
        assert re.search(r"optimizer\.edges\(\)\.size\(\)<10", body) and re.search(r"\(nInliers<30\)\s*&&\s*!bRecInit", body)
        assert re.search(r"chi2MonoOut\s*=\s*18\.f", body) and re.search(r"chi2StereoOut\s*=\s*24\.f", body)
        assert re.search(r"if\s*\(it==2\)\s*e->setRobustKernel\(0\)", body)
        assert "OptimizationAlgorithmGaussNewton" in body and "LinearSolverDense" in body
    assert re.search(r"rkp->setDelta\(5\)", fr) and "Marginalize(H,0,14)" in fr and "rkp" not in kf
    marg = rf._body(OPTIMIZER, r"Eigen::MatrixXd Optimizer::Marginalize\(")
    assert re.search(r"singularValues_inv\(i\)>1e-6", marg)
    hdr = open(os.path.join(rf.REF, "include", "G2oTypes.h")).read()
    assert re.search(r"H = \(H\+H\)/2;\s*Eigen::SelfAdjointEigenSolver<Eigen::Matrix<double,15,15> > es\(H\);", hdr) and "eigs[i]<1e-12" in hdr
    assert txt.count("PoseInertialOptimizationLast") >= 2


def test_marginalize_is_the_references_text():
    """The block shuffles of Marginalize executed from the text around the model's pseudo-inverse: start = 0, end = 14 on a 30 x 30."""
    body = rf._body(OPTIMIZER, r"Eigen::MatrixXd Optimizer::Marginalize\(")
    # the statements that move blocks: X.block(i,j,r,c) = Y.block(i,j,r,c) [- ...]; executed with a = 0, b = 15, c = 15
    a, b, c = 0, 15, 15
    rng = np.random.default_rng(3)
    A = rng.normal(size=(30, 40))
    H = A @ A.T
    M = {"H": H, "Hn": np.zeros((30, 30)), "res": np.zeros((30, 30))}

    def blk(name, args):
        i, j, r, cc = [int(eval(x, {"a": a, "b": b, "c": c})) for x in rf._split_top(args)]
        return M[name][i:i + r, j:j + cc], (i, j, r, cc)
    inv = None
    for stmt in [s.strip() for s in body.split(";")]:
        stmt = re.sub(r"^(?:if\([^)]*\)\s*\{?\s*|\}\s*)+", "", stmt).strip()              # with a = 0 the if(a>0) blocks move nothing
        m = re.match(r"(Hn|res)\.block\(([^=]*)\)\s*=\s*(H|Hn)\.block\(([^()]*)\)$", stmt)
        if m:
            dst, (i, j, r, cc) = blk(m.group(1), m.group(2))
            src, _ = blk(m.group(3), m.group(4))
            if dst.shape == src.shape and dst.size:
                M[m.group(1)][i:i + r, j:j + cc] = src
            continue
        if stmt.startswith("Hn.block(0,0,a+c,a+c) = Hn.block(0,0,a+c,a+c) - "):
            Hbb = M["Hn"][a + c:, a + c:].copy()
            U, s, Vt = np.linalg.svd(Hbb)
            inv = Vt.T @ np.diag(np.where(s > 1e-6, 1.0 / s, 0.0)) @ U.T
            M["Hn"][:a + c, :a + c] -= M["Hn"][:a + c, a + c:] @ inv @ M["Hn"][a + c:, :a + c]
            continue
        m = re.match(r"Hn\.block\(([^=]*)\)\s*=\s*Eigen::MatrixXd::Zero", stmt)
        if m:
            _, (i, j, r, cc) = blk("Hn", m.group(1))
            M["Hn"][i:i + r, j:j + cc] = 0
    assert inv is not None
    got, _ = pm.marginalize(H, 0, 14)
    assert np.abs(M["res"] - got).max() <= 1e-9 * np.abs(got).max() and np.abs(got[15:, 15:]).max() > 0
