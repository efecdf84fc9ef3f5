"""The three pieces of g2o that OptimizeEssentialGraph's model restates, taken from the reference's own text at test time and executed
against the model (tests/essential_graph_model.py):
  Sim3::log()                                   G/types/sim3.h:148-230
  EdgeSim3::computeError()                      G/types/types_seven_dof_expmap.h:106-114
  BaseBinaryEdge::linearizeOplus() (numeric)    G/core/base_binary_edge.hpp:131-205
The bodies go through the transliterator of tests/test_reference_formulas.py (imported, not edited) after a few text-level rules that
name C++ constructs it does not know (declarations without a value, `::`, the OpenMP block, `.col(d) =`).  What the text calls --
quaternion to matrix, matrix products, the 3 x 3 LU solve, operator*, inverse(), oplus -- is supplied by small Python objects; the
control flow, the branch conditions, the coefficient formulas and the differencing are the text's.  Nothing of the reference is stored."""
import os
import re

import numpy as np
import pytest

import essential_graph_model as em
import test_reference_formulas as rf

pytestmark = pytest.mark.skipif(not os.path.isdir(rf.REF), reason="the reference is only present in the build container")
G2O = os.path.join(rf.REF, "Thirdparty", "g2o", "g2o")
F = np.float64


class Mat3:
    """Eigen::Matrix3d as far as log() uses it: M(i, j), scalar * M, M * M (matrix product), M + M, M.lu().solve(t)"""

    def __init__(self, a):
        self.a = np.asarray(a, F)

    def __call__(self, i, j):
        return self.a[i, j]

    def __mul__(self, o):
        return Mat3(self.a @ o.a) if isinstance(o, Mat3) else Mat3(self.a * o)

    def __rmul__(self, o):
        return Mat3(o * self.a)

    def __add__(self, o):
        return Mat3(self.a + o.a)

    def lu(self):
        return self

    def solve(self, t):
        return np.linalg.solve(self.a, np.asarray(t, F))


class Quat:
    def __init__(self, q):
        self.q = [F(v) for v in q]

    def toRotationMatrix(self):
        return Mat3(em.quat_to_R(self.q))


def _skew(v):
    return Mat3([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])          # G/types/se3_ops.hpp skew


def _deltaR(R):
    return np.array([R(2, 1) - R(1, 2), R(0, 2) - R(2, 0), R(1, 0) - R(0, 1)], F)   # G/types/se3_ops.hpp deltaR


def _log_program():
    body = rf._body(os.path.join(G2O, "types", "sim3.h"), r"Vector7d log\(\) const\s*\{")
    body = re.sub(r"\b(Vector7d|Vector3d|Matrix3d) \w+;", "", body)               # declarations without a value
    body = re.sub(r"\bdouble A,B,C;", "", body)
    body = body.replace("Matrix3d::Identity()", "Identity3").replace("std::log", "log")
    return rf.c_to_python(rf.cpp_prepare(body), keep_returns=False)


def reference_log(S, program=[]):
    if not program:
        program.append(_log_program())
    env = dict(rf.ENV, r=Quat(S[0]), t=np.array([F(v) for v in S[1]], F), s=F(S[2]), res=np.zeros(7, F), Identity3=Mat3(np.eye(3)),
               log=lambda v: F(np.log(v)), acos=lambda v: F(np.arccos(v)), fabs=abs, skew=_skew, deltaR=_deltaR)
    exec(program[0], env)
    return env["res"]


class S3:
    """g2o::Sim3 for the transliterated bodies: operator*, inverse() are the model's; log() is the reference's text"""

    def __init__(self, S):
        self.S = ([F(v) for v in S[0]], [F(v) for v in S[1]], F(S[2]))

    def __mul__(self, o):
        return S3(em.sim3_mul(self.S, o.S))

    def inverse(self):
        return S3(em.sim3_inverse(self.S))

    def log(self):
        return reference_log(self.S)


class Vertex:
    def __init__(self, S, fixed, fix_scale):
        self.S, self._fixed, self.fix_scale, self.stack = S3(S), fixed, fix_scale, []

    def estimate(self):
        return self.S

    def fixed(self):
        return self._fixed

    def push(self):
        self.stack.append(self.S)

    def pop(self):
        self.S = self.stack.pop()

    def oplus(self, update):
        self.S = S3(em.om.oplus(self.S.S, list(update), self.fix_scale, F))


def _random_sim3(rng, rot, sig):
    w = rng.normal(size=3)
    return em.sim3_exp(list(np.concatenate([w / np.linalg.norm(w) * rot, rng.normal(size=3), [sig]])), F)


CASES = [(3e-6, 4e-6), (3e-6, 0.2), (0.4, 5e-6), (0.7, -0.3), (1.5, 0.05), (0.0, 0.0)]


def test_log_is_the_references_text_on_its_four_branches():
    rng = np.random.default_rng(3)
    text = open(os.path.join(G2O, "types", "sim3.h")).read()
    assert "upsilon = W.lu().solve(t)" in text and "d>1-eps" in text and "fabs(sigma)<eps" in text
    for rot, sig in CASES:
        for _ in range(4):
            S = _random_sim3(rng, rot, sig) if rot else ([F(0), F(0), F(0), F(1)], [F(0.25), F(-1.5), F(3.0)], F(1))
            ref = reference_log(S)
            got = np.array([float(v) for v in em.sim3_log(S, F)])
            # the text's library calls on the same inputs; B * Omega * Omega and the LU solve in another operation order: rounding,
            # amplified by the branch's coefficients (B up to 1 / sigma^3 on a theta^2 term)
            assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (rot, sig, got, ref)
    assert reference_log(([F(0), F(0), F(0), F(1)], [F(0.25), F(-1.5), F(3.0)], F(1))).tolist() == [0, 0, 0, 0.25, -1.5, 3.0, 0]


def _edge_env(rng, fixed_i=False, fixed_j=False, fix_scale=False):
    vi = Vertex(_random_sim3(rng, 0.5, 0.0 if fix_scale else 0.1), fixed_i, fix_scale)
    vj = Vertex(_random_sim3(rng, 0.4, 0.0 if fix_scale else -0.05), fixed_j, fix_scale)
    meas = _random_sim3(rng, 0.3, 0.0 if fix_scale else 0.02)
    env = dict(rf.ENV, _vertices=[vi, vj], _measurement=S3(meas), Sim3=lambda m: m, _error=np.zeros(7, F))
    body = rf._body(os.path.join(G2O, "types", "types_seven_dof_expmap.h"), r"class EdgeSim3 [^{]*\{[^{]*void computeError\(\)\s*\{")
    body = re.sub(r"static_cast<[^>]*>\(([^)]*)\)", r"\1", body).replace("Sim3 C(_measurement)", "Sim3 C = Sim3(_measurement)")
    program = rf.c_to_python(rf.cpp_prepare(body))

    def computeError():
        exec(program, env)
    env["computeError"] = computeError
    return env, vi, vj, meas


def test_compute_error_is_the_references_text():
    rng = np.random.default_rng(4)
    for _ in range(5):
        env, vi, vj, meas = _edge_env(rng)
        env["computeError"]()
        want = em.edge_errors(em._s3([meas[0]], [meas[1]], [meas[2]], F), em._s3([vi.S.S[0]], [vi.S.S[1]], [vi.S.S[2]], F),
                              em._s3([vj.S.S[0]], [vj.S.S[1]], [vj.S.S[2]], F), F)[0]
        assert np.abs(env["_error"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("fixed_i,fixed_j,fix_scale", [(False, False, False), (True, False, False), (False, True, True), (False, False, True)])
def test_numeric_jacobian_is_the_references_text(fixed_i, fixed_j, fix_scale):
    rng = np.random.default_rng(5)
    env, vi, vj, meas = _edge_env(rng, fixed_i, fixed_j, fix_scale)
    body = rf._body(os.path.join(G2O, "core", "base_binary_edge.hpp"), r"::linearizeOplus\(\)\s*\{")
    assert "const double delta = 1e-9" in body and "scalar * errorBak" in body
    body = re.sub(r"#ifdef G2O_OPENMP.*?#endif", "", body, flags=re.S)
    body = re.sub(r"static_cast<[^>]*>\s*\(([^)]*)\)", r"\1", body)
    body = re.sub(r"if \(!iNotFixed && !jNotFixed\)\s*return;", "", body)           # (no test case has both ends fixed)
    body = re.sub(r"ErrorVector errorBak;|double add_v[ij]\[[^\]]*\];|std::fill\([^;]*\);", "", body)
    body = re.sub(r"Vertex(Xi|Xj)Type::Dimension", "7", body)
    body = re.sub(r"(_jacobianOplusX[ij])\.col\(d\) =", r"\1[:, d] =", body)
    program = rf.c_to_python(rf.cpp_prepare(body))
    env.update(add_vi=[F(0)] * 7, add_vj=[F(0)] * 7, errorBak=None, _jacobianOplusXi=np.zeros((7, 7), F), _jacobianOplusXj=np.zeros((7, 7), F))
    env["computeError"]()
    e0 = env["_error"].copy()
    exec(program, env)
    assert np.array_equal(env["_error"], e0)                                          # _error = errorBeforeNumeric
    p = em.Problem([vi.S.S[0], vj.S.S[0]], [vi.S.S[1], vj.S.S[1]], [vi.S.S[2], vj.S.S[2]], [fixed_i, fixed_j], [fix_scale] * 2, [0], [1],
                   [meas[0]], [meas[1]], [meas[2]])
    e, Ji, Jj = em.linearise(p, em._s3(p.q, p.t, p.s, F), em._s3(p.mq, p.mt, p.ms, F), F)
    # differences of errors that agree to ~1e-15, times 5e8: 1e-5 absolute on entries of order 1 is the noise of the scheme itself
    assert np.abs(env["_jacobianOplusXi"] - Ji[0]).max() <= 1e-5 and np.abs(env["_jacobianOplusXj"] - Jj[0]).max() <= 1e-5
    assert (not env["_jacobianOplusXi"].any()) == fixed_i and (not env["_jacobianOplusXj"].any()) == fixed_j
    if fix_scale:
        assert not env["_jacobianOplusXi"][:, 6].any() and not env["_jacobianOplusXj"][:, 6].any()
    assert np.abs(e[0] - e0).max() <= 1e-12
