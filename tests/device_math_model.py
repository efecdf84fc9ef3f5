"""Inputs and references for the shared device primitives (tools/micro/device_math_test.hip): nothing here touches the GPU.

Every function of csrc/wave.hpp, lm_block.hpp, lm_record.hpp, lm_step.hpp, se3.hpp, sim3_math.hpp, pose_inertial_edges.hpp (the SO3 part) and
null_vector4.hpp is restated from the formula the reference project uses, once, over an arithmetic `A`:

  (f64)  A = F64: Python floats -- IEEE double, every + - * / and sqrt correctly rounded, evaluated left to right as written, which is
         the order of operations the headers document;
  (mp)   A = MP: mpmath at 50 digits.

One text per formula, evaluated twice, so that the two cannot drift apart; what differs between them is the arithmetic alone.  The
sums, the lane solve's serial LDL^T and the integer scans have a model of their own (exact, or in the fixed order the header states).

A restatement reports the branch it took, and every threshold comparison goes through a `Decide`, which records it as (lhs, op, rhs,
scale) in the arithmetic at hand, so that a test can see how far a case stands from each threshold.  With `force=` the decisions come
from the caller instead: (mp) is walked down the branch (f64) took, the one the case is meant for, and what it would have decided by
itself is read from the operands it recorded.

Citations: G = Thirdparty/g2o/g2o of the reference, S = its src, E = Eigen 3.
  Quaterniond(Matrix3d)           E/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other,3,3>::run
  toRotationMatrix, operator*, _transformVector   same file
  SE3Quat::exp / operator* / normalizeRotation    G/types/se3quat.h:223-257, 104-110, 297-303
  Sim3(Vector7d), map, log, inverse, operator*    G/types/sim3.h:70-142, 144-146, 148-230, 233-236, 266-272
  deltaR, skew                                    G/types/se3_ops.hpp
  ExpSO3 / LogSO3 / InverseRightJacobianSO3 / RightJacobianSO3    S/G2oTypes.cc:986-1063
  IMU::NormalizeRotation                          S/ImuTypes.cc:30-36
  ImuCamPose::Update, GDirection::Update          S/G2oTypes.cc:192-220, include/G2oTypes.h:261-264
  Pinhole::project / projectJac                   S/CameraModels/Pinhole.cpp:41-47, 81-91
  KannalaBrandt8::project / projectJac            S/CameraModels/KannalaBrandt8.cpp:52-69, 166-196
  OptimizationAlgorithmLevenberg::solve, computeLambdaInit    G/core/optimization_algorithm_levenberg.cpp:118-146, 161-174
  RobustKernelHuber::robustify                    G/core/robust_kernel_impl.cpp:78-91
"""
import functools
import math
import struct

import mpmath
import numpy as np

MP_DPS = 50
MARGIN = 8.0


# ------------------------------------------------------------------------------------------------ the two arithmetics
class F64:
    name = "f64"
    num = staticmethod(float)
    sqrt = staticmethod(math.sqrt)
    sin = staticmethod(math.sin)
    cos = staticmethod(math.cos)
    acos = staticmethod(math.acos)
    exp = staticmethod(math.exp)
    log = staticmethod(math.log)
    atan2 = staticmethod(math.atan2)

    @staticmethod
    def f32(x):
        return float(np.float32(x))


class MP:
    name = "mp"
    num = staticmethod(lambda x: mpmath.mpf(x))
    sqrt = staticmethod(mpmath.sqrt)
    sin = staticmethod(mpmath.sin)
    cos = staticmethod(mpmath.cos)
    acos = staticmethod(mpmath.acos)
    exp = staticmethod(mpmath.exp)
    log = staticmethod(mpmath.log)
    atan2 = staticmethod(mpmath.atan2)

    @staticmethod
    def f32(x):                       # the nearest float32 of an mp value, rounded once
        with mpmath.workprec(24):
            y = +mpmath.mpf(x)
        return mpmath.mpf(y)


class Decide:
    """The decisions of one evaluation: recorded, or forced from a list recorded earlier."""

    def __init__(self, force=None):
        self.force = list(force) if force is not None else None
        self.taken = []
        self.compares = []

    @staticmethod
    def natural(lhs, op, rhs):
        return bool({"<": lhs < rhs, ">": lhs > rhs, ">=": lhs >= rhs}[op])

    def __call__(self, lhs, op, rhs, scale):
        natural = self.natural(lhs, op, rhs)
        self.compares.append((lhs, op, rhs, scale))
        r = natural if self.force is None else self.force[len(self.taken)]
        self.taken.append(bool(r))
        return r


def skew(A, w):
    z = A.num(0)
    return [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]


def mat3_mul(a, b):
    return [[a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def mat3_vec(a, x):
    return [a[i][0] * x[0] + a[i][1] * x[1] + a[i][2] * x[2] for i in range(3)]


def rows3(flat):
    return [list(flat[0:3]), list(flat[3:6]), list(flat[6:9])]


def flat3(m):
    return [m[i][j] for i in range(3) for j in range(3)]


# ------------------------------------------------------------------------------------------------ quaternions (Eigen)
def quat_from_R(A, m, dec):
    """Quaterniond(Matrix3d): trace > 0, or the largest diagonal entry i with (j, k) its cyclic successors.  -> (x, y, z, w), branch"""
    t = m[0][0] + m[1][1] + m[2][2]
    q = [None] * 4
    if dec(t, ">", A.num(0), 1.0):
        t = A.sqrt(t + 1)
        q[3] = A.num(0.5) * t
        t = A.num(0.5) / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
        return q, "trace"
    i = 0
    if dec(m[1][1], ">", m[0][0], 1.0):
        i = 1
    if dec(m[2][2], ">", m[i][i], 1.0):
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = A.sqrt(m[i][i] - m[j][j] - m[k][k] + 1)
    q[i] = A.num(0.5) * t
    t = A.num(0.5) / t
    q[3] = (m[k][j] - m[j][k]) * t
    q[j] = (m[j][i] + m[i][j]) * t
    q[k] = (m[k][i] + m[i][k]) * t
    return q, "i%d" % i


def quat_to_R(A, q):
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def quat_rotate(A, q, v):
    """_transformVector: uv = 2 (q.vec x v); v + w uv + q.vec x uv"""
    uv = [2 * (q[1] * v[2] - q[2] * v[1]), 2 * (q[2] * v[0] - q[0] * v[2]), 2 * (q[0] * v[1] - q[1] * v[0])]
    return [v[0] + q[3] * uv[0] + (q[1] * uv[2] - q[2] * uv[1]),
            v[1] + q[3] * uv[1] + (q[2] * uv[0] - q[0] * uv[2]),
            v[2] + q[3] * uv[2] + (q[0] * uv[1] - q[1] * uv[0])]


def quat_mul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def quat_normalize(A, q, dec):
    """SE3Quat::normalizeRotation: w made non-negative, then divided by the norm"""
    flipped = dec(q[3], "<", A.num(0), 1.0)
    if flipped:
        q = [-c for c in q]
    n = A.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [c / n for c in q], "flip" if flipped else "keep"


def se3_mul(A, a, b, dec):
    rt = quat_rotate(A, a[0:4], b[4:7])
    t = [a[4 + i] + rt[i] for i in range(3)]
    q, br = quat_normalize(A, quat_mul(a[0:4], b[0:4]), dec)
    return q + t, br


# ------------------------------------------------------------------------------------------------ SE3Quat::exp(u) * T
def pose_oplus(A, T, u, dec):
    om, ups = u[0:3], u[3:6]
    theta = A.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    Om = skew(A, om)
    Om2 = mat3_mul(Om, Om)
    I = [[A.num(1 if i == j else 0) for j in range(3)] for i in range(3)]
    if dec(theta, "<", A.num(0.00001), 1e-5):
        R = [[I[i][j] + Om[i][j] + Om2[i][j] for j in range(3)] for i in range(3)]
        V = R
        br = "small"
    else:
        a = A.sin(theta) / theta
        b = (1 - A.cos(theta)) / (theta * theta)
        c = (theta - A.sin(theta)) / (theta ** 3)
        R = [[I[i][j] + a * Om[i][j] + b * Om2[i][j] for j in range(3)] for i in range(3)]
        V = [[I[i][j] + b * Om[i][j] + c * Om2[i][j] for j in range(3)] for i in range(3)]
        br = "full"
    eq, qb = quat_from_R(A, R, dec)
    et = mat3_vec(V, ups)
    eq, _ = quat_normalize(A, eq, dec)
    out, nb = se3_mul(A, eq + et, T, dec)
    return out, "%s/%s/%s" % (br, qb, nb)


def series_path(t):
    """pose_oplus_series hands over to pose_oplus_fast above |omega|^2 = 0.09"""
    return "handover" if t > 0.09 else "series"


# ------------------------------------------------------------------------------------------------ cameras
def cam_project(A, cam, v, roundings):
    model, fx, fy, cx, cy, k1, k2, k3, k4 = cam
    if model == 1:
        x2y2 = v[0] * v[0] + v[1] * v[1]
        rho = A.f32(A.sqrt(A.f32(x2y2)))
        z = A.f32(v[2])
        theta = A.f32(A.atan2(rho, z))
        y32, x32 = A.f32(v[1]), A.f32(v[0])
        psi = A.f32(A.atan2(y32, x32))
        roundings.extend([rho, z, theta, y32, x32, psi])
        t2 = theta * theta
        t3 = theta * t2
        t5 = t3 * t2
        t7 = t5 * t2
        t9 = t7 * t2
        r = theta + k1 * t3 + k2 * t5 + k3 * t7 + k4 * t9
        return [fx * r * A.cos(psi) + cx, fy * r * A.sin(psi) + cy], "kb8_back" if v[2] < 0 else "kb8"
    return [fx * v[0] / v[2] + cx, fy * v[1] / v[2] + cy], "pinhole"


def cam_project_jac(A, cam, v):
    model, fx, fy, cx, cy, k1, k2, k3, k4 = cam
    if model == 1:
        x2, y2, z2 = v[0] * v[0], v[1] * v[1], v[2] * v[2]
        r2 = x2 + y2
        r = A.sqrt(r2)
        r3 = r2 * r
        th = A.atan2(r, v[2])
        th2 = th * th
        th3 = th2 * th
        th4 = th2 * th2
        th5 = th4 * th
        th6 = th2 * th4
        th7 = th6 * th
        th8 = th4 * th4
        th9 = th8 * th
        f = th + th3 * k1 + th5 * k2 + th7 * k3 + th9 * k4
        fd = 1 + 3 * k1 * th2 + 5 * k2 * th4 + 7 * k3 * th6 + 9 * k4 * th8
        den = r2 * (r2 + z2)
        j00 = fx * (fd * v[2] * x2 / den + f * y2 / r3)
        j10 = fy * (fd * v[2] * v[1] * v[0] / den - f * v[1] * v[0] / r3)
        j01 = fx * (fd * v[2] * v[1] * v[0] / den - f * v[1] * v[0] / r3)
        j11 = fy * (fd * v[2] * y2 / den + f * x2 / r3)
        j02 = -fx * fd * v[0] / (r2 + z2)
        j12 = -fy * fd * v[1] / (r2 + z2)
        return [j00, j01, j02, j10, j11, j12], "kb8_back" if v[2] < 0 else "kb8"
    z = A.num(0)
    return [fx / v[2], z, -fx * v[0] / (v[2] * v[2]), z, fy / v[2], -fy * v[1] / (v[2] * v[2])], "pinhole"


# ------------------------------------------------------------------------------------------------ Sim3
def s3_coeffs(A, sigma, s, theta, sig_small, th_small):
    """A, B, C of W = A Omega + B Omega^2 + C I (the same four branches in the constructor and in log())"""
    if sig_small:
        C = A.num(1)
        if th_small:
            return A.num(1) / 2, A.num(1) / 6, C
        th2 = theta * theta
        return (1 - A.cos(theta)) / th2, (theta - A.sin(theta)) / (th2 * theta), C
    C = (s - 1) / sigma
    if th_small:
        s2 = sigma * sigma
        return ((sigma - 1) * s + 1) / s2, ((A.num(0.5) * s2 - sigma + 1) * s) / (s2 * sigma), C
    a = s * A.sin(theta)
    b = s * A.cos(theta)
    th2 = theta * theta
    c = th2 + sigma * sigma
    return (a * sigma + (1 - b) * theta) / (theta * c), (C - ((b - 1) * sigma + a * theta) / c) * 1 / th2, C


def s3_exp(A, u, dec):
    om, ups, sigma = u[0:3], u[3:6], u[6]
    theta = A.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    Om = skew(A, om)
    s = A.exp(sigma)
    Om2 = mat3_mul(Om, Om)
    eps = A.num(0.00001)
    sig_small = dec(abs(sigma), "<", eps, 1e-5)
    th_small = dec(theta, "<", eps, 1e-5)
    Ac, Bc, Cc = s3_coeffs(A, sigma, s, theta, sig_small, th_small)
    I = [[A.num(1 if i == j else 0) for j in range(3)] for i in range(3)]
    if th_small:
        R = [[I[i][j] + Om[i][j] + Om2[i][j] for j in range(3)] for i in range(3)]
    else:
        ra = A.sin(theta) / theta
        rb = (1 - A.cos(theta)) / (theta * theta)
        R = [[I[i][j] + ra * Om[i][j] + rb * Om2[i][j] for j in range(3)] for i in range(3)]
    q, qb = quat_from_R(A, R, dec)
    W = [[Ac * Om[i][j] + Bc * Om2[i][j] + Cc * I[i][j] for j in range(3)] for i in range(3)]
    t = mat3_vec(W, ups)
    return q + t + [s], "%s/%s/%s" % ("sig_small" if sig_small else "sig_big", "th_small" if th_small else "th_big", qb)


def s3_mul(A, a, b):
    q = quat_mul(a[0:4], b[0:4])
    rt = quat_rotate(A, a[0:4], b[4:7])
    return q + [a[7] * rt[i] + a[4 + i] for i in range(3)] + [a[7] * b[7]]


def s3_inverse(A, a):
    qc = [-a[0], -a[1], -a[2], a[3]]
    k = A.num(-1) / a[7]
    return qc + quat_rotate(A, qc, [k * a[4], k * a[5], k * a[6]]) + [A.num(1) / a[7]]


def s3_map(A, a, X):
    r = quat_rotate(A, a[0:4], X)
    return [a[7] * r[i] + a[4 + i] for i in range(3)]


def lu3_solve(A, W, t, dec):
    """Matrix3d::lu().solve(): partial pivoting (largest |entry| of the column, the first one on a tie), unit L, forward then backward
    substitution in ascending k.  -> x, path 'p<first pivot row><s|n>' (s: the second column swaps too)"""
    M = [list(W[i]) + [t[i]] for i in range(3)]
    a0, a1, a2 = abs(M[0][0]), abs(M[1][0]), abs(M[2][0])
    # the first of the largest: row 1 when it beats row 0 and is not beaten by row 2; row 2 when it beats both
    if dec(a1, ">", a0, 1.0) and dec(a1, ">=", a2, 1.0):
        p = 1
    elif dec(a2, ">", a0, 1.0) and dec(a2, ">", a1, 1.0):
        p = 2
    else:
        p = 0
    M[0], M[p] = M[p], M[0]
    l10 = M[1][0] / M[0][0]
    l20 = M[2][0] / M[0][0]
    for j in (1, 2):
        M[1][j] = M[1][j] - l10 * M[0][j]
        M[2][j] = M[2][j] - l20 * M[0][j]
    swap2 = dec(abs(M[2][1]), ">", abs(M[1][1]), 1.0)
    if swap2:
        M[1], M[2] = M[2], M[1]
        l10, l20 = l20, l10
    l21 = M[2][1] / M[1][1]
    u22 = M[2][2] - l21 * M[1][2]
    y0 = M[0][3]
    y1 = M[1][3] - l10 * y0
    y2 = M[2][3] - l20 * y0 - l21 * y1
    x2 = y2 / u22
    x1 = (y1 - M[1][2] * x2) / M[1][1]
    x0 = (y0 - M[0][1] * x1 - M[0][2] * x2) / M[0][0]
    return [x0, x1, x2], "p%d%s" % (p, "s" if swap2 else "n")


def s3_log(A, a, dec):
    s = a[7]
    sigma = A.log(s)
    R = quat_to_R(A, a[0:4])
    d = A.num(0.5) * (R[0][0] + R[1][1] + R[2][2] - 1)
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    eps = A.num(0.00001)
    sig_small = dec(abs(sigma), "<", eps, 1e-5)
    # d > 1 - eps, looked at as (1 - d) against eps: that is the quantity whose distance from the threshold matters
    th_small = bool(dec(d, ">", 1 - eps, None))
    if th_small:
        k = A.num(0.5)
        theta = None
    else:
        theta = A.acos(d)
        k = theta / (2 * A.sqrt(1 - d * d))
    Ac, Bc, Cc = s3_coeffs(A, sigma, s, theta, sig_small, th_small)
    om = [k * dR[0], k * dR[1], k * dR[2]]
    Om = skew(A, om)
    Om2 = mat3_mul(Om, Om)
    W = [[Ac * Om[i][j] + Bc * Om2[i][j] + Cc * (1 if i == j else 0) for j in range(3)] for i in range(3)]
    ups, path = lu3_solve(A, W, a[4:7], dec)
    return om + ups + [sigma], "%s/%s/%s" % ("sig_small" if sig_small else "sig_big", "th_small" if th_small else "th_big", path)


# ------------------------------------------------------------------------------------------------ the SO3 functions of the inertial edges
def rodrigues(A, w, a, b):
    W = skew(A, w)
    W2 = mat3_mul(W, W)
    return [[A.num(1 if i == j else 0) + a * W[i][j] + b * W2[i][j] for j in range(3)] for i in range(3)]


def pi_exp_so3(A, w, dec):
    """ExpSO3 in closed form (csrc/pose_inertial_edges.hpp leaves out the float round trip and the SVD behind it)"""
    d2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    d = A.sqrt(d2)
    if dec(d, "<", A.num(1e-5), 1e-5):
        return rodrigues(A, w, A.num(1), A.num(0.5)), "small"
    return rodrigues(A, w, A.sin(d) / d, (1 - A.cos(d)) / d2), "full"


def pi_log_so3(A, R, dec):
    tr = R[0][0] + R[1][1] + R[2][2]
    w = [(R[2][1] - R[1][2]) / 2, (R[0][2] - R[2][0]) / 2, (R[1][0] - R[0][1]) / 2]
    c = (tr - 1) * A.num(0.5)
    if dec(c, ">", A.num(1), 1.0) or dec(c, "<", A.num(-1), 1.0):
        return w, "out_of_range"
    theta = A.acos(c)
    s = A.sin(theta)
    if dec(abs(s), "<", A.num(1e-5), 1e-5):
        return w, "unscaled"
    return [theta * w[i] / s for i in range(3)], "scaled"


def pi_right_jacobian(A, v, dec):
    d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    d = A.sqrt(d2)
    if dec(d, "<", A.num(1e-5), 1e-5):
        return rodrigues(A, v, A.num(0), A.num(0)), "small"
    return rodrigues(A, v, -(1 - A.cos(d)) / d2, (d - A.sin(d)) / (d2 * d)), "full"


def pi_inv_right_jacobian(A, v, dec):
    d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    d = A.sqrt(d2)
    if dec(d, "<", A.num(1e-5), 1e-5):
        return rodrigues(A, v, A.num(0), A.num(0)), "small"
    return rodrigues(A, v, A.num(0.5), 1 / d2 - (1 + A.cos(d)) / (2 * d * A.sin(d))), "full"


def polar_factor(A, X):
    """IMU::NormalizeRotation: U V^T of the SVD"""
    if A is MP:
        U, _, Vt = mpmath.svd_r(mpmath.matrix(X))
        P = U * Vt
        return [[P[i, j] for j in range(3)] for i in range(3)]
    U, _, Vt = np.linalg.svd(np.array(X, dtype=np.float64))
    return (U @ Vt).tolist()


# ------------------------------------------------------------------------------------------------ reductions, in the order the headers state
def wave_tree_sum(v):
    """wave_sum_f64: inclusive scan by 1, 2, 4, 8 inside each row of 16 lanes, lane 15 of rows 0 and 2 added to rows 1 and 3, lane 31
    added to rows 2 and 3; the value of lane 63"""
    v = [float(x) for x in v]
    for s in (1, 2, 4, 8):
        v = [v[l] + (v[l - s] if (l & 15) >= s else 0.0) for l in range(64)]
    v = [v[l] + (v[(l & ~15) - 1] if (l >> 4) in (1, 3) else 0.0) for l in range(64)]
    v = [v[l] + (v[31] if (l >> 4) >= 2 else 0.0) for l in range(64)]
    return v[63]


def block_sum(v):
    """block_sum / block_sum_256: the four wave totals added in wave order"""
    w = [wave_tree_sum(v[64 * i:64 * i + 64]) for i in range(4)]
    return ((w[0] + w[1]) + w[2]) + w[3]


def lm_block_reduce(vals):
    """vals[256][NV] -> NV sums: 8 segments of 32 threads, four interleaved running sums per segment, the partials by a fixed tree"""
    out = []
    for v in range(len(vals[0])):
        part = []
        for g in range(8):
            p = [float(vals[32 * g + j][v]) for j in range(32)]
            a = [0.0, 0.0, 0.0, 0.0]
            for j in range(8):
                for c in range(4):
                    a[c] = a[c] + p[4 * j + c]
            part.append((a[0] + a[1]) + (a[2] + a[3]))
        out.append(((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7])))
    return out


def int32(x):
    return ((int(x) + 2 ** 31) % 2 ** 32) - 2 ** 31


def wave_int(v):
    """-> the 6 x 64 outputs of fid 1 for the 64 int32 lane values v"""
    scan, acc = [], 0
    for x in v:
        acc = int32(acc + x)
        scan.append(acc)
    u = [x % 2 ** 32 for x in v]
    uscan = [s % 2 ** 32 for s in scan]
    return [float(s) for s in scan] + [float(scan[63])] * 64 + [float(max(v))] * 64 + [float(min(u))] * 64 + [float(s) for s in uscan] + [float(uscan[63])] * 64


def ldlt_solve(A, H, b, lam, rel):
    """(H + lambda I) x = b by a serial left-looking LDL^T in ascending k, without pivoting (Eigen::LDLT::isPositive as the verdict).
    -> x or None, branch"""
    n = len(b)
    a = [[A.num(H[i][j]) + A.num(lam if i == j else 0.0) for j in range(n)] for i in range(n)]
    L = [[None] * n for _ in range(n)]
    D = [None] * n
    for j in range(n):
        for i in range(j, n):
            s = a[i][j]
            for k in range(j):
                s = s - (L[i][k] * L[j][k]) * D[k]
            if i == j:
                D[j] = s
                if not (s > 0) or abs(s) == math.inf:
                    return None, "fail_pos"
                if rel and not (s > A.num(2.0 ** -40) * abs(A.num(H[j][j]))):
                    return None, "fail_rel"
            else:
                L[i][j] = s / D[j]
    y = [None] * n
    for i in range(n):
        s = A.num(b[i])
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    z = [y[i] / D[i] for i in range(n)]
    x = [None] * n
    for i in range(n - 1, -1, -1):
        s = z[i]
        for k in range(i + 1, n):
            s = s - L[k][i] * x[k]
        x[i] = s
    return x, "ok"


# ------------------------------------------------------------------------------------------------ the LM step and the Huber kernel
# (f64) only: + - * / sqrt and compares, held bit for bit.  numpy's float64 scalars, because x / 0 and inf - inf must give what IEEE
# says they give.  std::min(a, b) is (b < a) ? b : a, std::max(a, b) is (a < b) ? b : a; pow(x, 3) is restated as x * x * x (what
# the library documents for it).
def _ieee(fn):
    def wrapped(*args):
        with np.errstate(all="ignore"):
            return fn(*[np.float64(a) for a in args])
    return wrapped


def _good_step_factor(rho):
    c3 = 2 * rho - 1
    alpha = 1. - c3 * c3 * c3
    upper, lower = np.float64(2.) / 3., np.float64(1.) / 3.        # _goodStepUpperScale, _goodStepLowerScale
    alpha = upper if upper < alpha else alpha
    factor = alpha if lower < alpha else lower
    return factor, ("2/3" if factor == upper else "1/3" if factor == lower else "cubic")


@_ieee
def lm_trial_verdict(lam, ni, currentChi, ok2, tempChi, scale):
    """-> ([rho, accepted, lambda, ni, currentChi], branch)"""
    if not ok2:
        tempChi = np.float64(np.finfo(np.float64).max)
    rho = currentChi - tempChi
    scale = scale + 1e-3
    rho = rho / scale
    if rho > 0 and np.isfinite(tempChi):
        factor, br = _good_step_factor(rho)
        return [rho, 1.0, lam * factor, 2.0, tempChi], "accepted_" + br
    return [rho, 0.0, lam * ni, ni * 2, currentChi], ("rejected_rho" if not rho > 0 else "rejected_not_finite")


@_ieee
def lm_accepted_lambda(lam, rho):
    factor, br = _good_step_factor(rho)
    return [lam * factor], br


@_ieee
def lm_iteration_continues(currentChi, nBad, exhausted, rho, iniChi):
    """-> ([continues, nBad], branch)"""
    if exhausted:
        return [0.0, nBad], "exhausted"
    if rho == 0:
        return [0.0, nBad], "rho_zero"
    if (iniChi - currentChi) * 1e3 < iniChi:
        nBad = nBad + 1
        return ([0.0, nBad], "bad_stop") if nBad >= 3 else ([1.0, nBad], "bad")
    return [1.0, 0.0], "good"


@_ieee
def lm_lambda_init(user, max_diagonal):
    if user > 0:
        return [user], "user"
    return [1e-5 * max_diagonal], "diagonal"


@_ieee
def lm_huber(e, delta, dsqr):
    if e <= dsqr:
        return [e, 1.], "inlier"
    sqrte = np.sqrt(e)
    return [2 * sqrte * delta - dsqr, delta / sqrte], "outlier"


LM_STEP = {60: lm_trial_verdict, 61: lm_accepted_lambda, 62: lm_iteration_continues, 63: lm_lambda_init, 64: lm_huber}


# ------------------------------------------------------------------------------------------------ function table
# fid -> (name, n_int, n_dbl, n_out, host_device, bit_equal, output parts); the counts are the rows of kFns in the harness
LDLT = {10: (6, False), 11: (7, False), 12: (9, False), 13: (9, True), 14: (15, True), 15: (30, True)}
Q, T3, S1, R9 = ("q", 0, 4), ("t", 4, 7), ("s", 7, 8), ("R", 0, 9)
FNS = {
    1: ("wave_int", 64, 0, 384, False, True, None), 2: ("wave_sum_f64", 0, 64, 64, False, True, None),
    3: ("block_sum", 0, 512, 512, False, True, None), 4: ("block_sum_256", 0, 256, 1, False, True, None),
    5: ("lm_block_reduce28", 0, 7168, 28, False, True, None),
    20: ("quat_from_R", 0, 9, 4, True, True, None), 21: ("quat_to_R", 0, 4, 9, True, True, None),
    22: ("quat_rotate", 0, 7, 3, True, True, None), 23: ("quat_normalize", 0, 4, 4, True, True, None),
    24: ("se3_mul", 0, 14, 7, True, True, None), 25: ("s3_mul", 0, 16, 8, True, True, None),
    26: ("s3_inverse", 0, 8, 8, True, True, None), 27: ("s3_map", 0, 11, 3, True, True, None),
    28: ("s3_exp", 0, 7, 8, True, False, [Q, T3, S1]), 29: ("s3_log", 0, 8, 7, True, False, [("omega", 0, 3), ("upsilon", 3, 6), ("sigma", 6, 7)]),
    30: ("pose_oplus", 0, 13, 7, False, False, [Q, T3]), 31: ("pose_oplus_fast", 0, 13, 7, False, False, [Q, T3]),
    32: ("pose_oplus_series", 0, 13, 7, False, False, [Q, T3]), 33: ("fast_rsqrt", 0, 1, 1, False, False, None),
    34: ("cam_project", 0, 12, 2, False, False, [("uv", 0, 2)]), 35: ("cam_project_jac", 0, 12, 6, False, False, [("J", 0, 6)]),
    40: ("pi_exp_so3", 0, 3, 9, True, False, [R9]), 41: ("pi_log_so3", 0, 9, 3, True, False, [("w", 0, 3)]),
    42: ("pi_right_jacobian", 0, 3, 9, True, False, [R9]), 43: ("pi_inv_right_jacobian", 0, 3, 9, True, False, [R9]),
    44: ("pi_normalize_rotation", 0, 9, 9, True, False, [R9]), 45: ("pi_gdir_oplus", 0, 11, 9, True, False, [R9]),
    46: ("pi_oplus", 0, 36, 21, True, False, [R9, ("t", 9, 12), ("v", 12, 15), ("bg", 15, 18), ("ba", 18, 21)]),
    50: ("null_vector4", 0, 16, 8, False, False, None),
    60: ("lm_trial_verdict", 0, 6, 5, True, True, None), 61: ("lm_accepted_lambda", 0, 2, 1, True, True, None),
    62: ("lm_iteration_continues", 0, 5, 2, True, True, None), 63: ("lm_lambda_init", 0, 2, 1, True, True, None),
    64: ("lm_huber", 0, 3, 2, True, True, None),
}
for _fid, (_n, _rel) in LDLT.items():
    FNS[_fid] = ("lane_ldlt_solve<%d,%s>" % (_n, "true" if _rel else "false"), 0, _n * _n + _n + 2, 2 * _n + 2, False, True, [("x", 0, _n)])
HOST_FIDS = sorted(f for f, r in FNS.items() if r[4])
SENTINEL = -777.25


def evaluate(A, fid, dv, force=None):
    """One scalar-math case in arithmetic A.  -> (outputs, branch, Decide, float32 roundings)"""
    x = [A.num(float(c)) for c in dv]
    dec = Decide(force)
    rnd = []
    if fid == 20:
        out, br = quat_from_R(A, rows3(x), dec)
    elif fid == 21:
        out, br = flat3(quat_to_R(A, x)), "-"
    elif fid == 22:
        out, br = quat_rotate(A, x[0:4], x[4:7]), "-"
    elif fid == 23:
        out, br = quat_normalize(A, x, dec)
    elif fid == 24:
        out, br = se3_mul(A, x[0:7], x[7:14], dec)
    elif fid == 25:
        out, br = s3_mul(A, x[0:8], x[8:16]), "-"
    elif fid == 26:
        out, br = s3_inverse(A, x), "-"
    elif fid == 27:
        out, br = s3_map(A, x[0:8], x[8:11]), "-"
    elif fid == 28:
        out, br = s3_exp(A, x, dec)
    elif fid == 29:
        out, br = s3_log(A, x, dec)
    elif fid in (30, 31, 32):
        out, br = pose_oplus(A, x[0:7], x[7:13], dec)
    elif fid == 34:
        out, br = cam_project(A, [int(dv[0])] + x[1:9], x[9:12], rnd)
    elif fid == 35:
        out, br = cam_project_jac(A, [int(dv[0])] + x[1:9], x[9:12])
    elif fid == 40:
        m, br = pi_exp_so3(A, x, dec)
        out = flat3(m)
    elif fid == 41:
        out, br = pi_log_so3(A, rows3(x), dec)
    elif fid == 42:
        m, br = pi_right_jacobian(A, x, dec)
        out = flat3(m)
    elif fid == 43:
        m, br = pi_inv_right_jacobian(A, x, dec)
        out = flat3(m)
    elif fid == 44:
        out, br = flat3(polar_factor(A, rows3(x))), "-"
    elif fid == 45:
        E, br = pi_exp_so3(A, [x[9], x[10], A.num(0)], dec)
        out = flat3(mat3_mul(rows3(x[0:9]), E))
    elif fid == 46:
        R = rows3(x[0:9])
        dx = x[21:36]
        dt = mat3_vec(R, dx[3:6])
        E, br = pi_exp_so3(A, dx[0:3], dec)
        out = flat3(mat3_mul(R, E)) + [x[9 + i] + dt[i] for i in range(3)] + [x[12 + i] + dx[6 + i] for i in range(9)]
    else:
        raise KeyError(fid)
    return out, br, dec, rnd


# ------------------------------------------------------------------------------------------------ the case list
class Case:
    __slots__ = ("fid", "iv", "dv", "tag", "want", "bits")

    def __init__(self, fid, dv=(), iv=(), tag="", want=None, bits=False):
        """want: the branch the case is meant for; bits: the case uses + - * / sqrt only and is claimed bit for bit"""
        self.fid, self.iv, self.tag, self.want, self.bits = fid, [int(i) for i in iv], tag, want, bits
        self.dv = [float(d) for d in dv]
        name, ni, nd = FNS[fid][0:3]
        assert len(self.iv) == ni and len(self.dv) == nd, (name, len(self.iv), len(self.dv))


AXES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)]
ANGLES = [0.0, 1e-8, 1.0, math.radians(119), math.radians(121), math.radians(179.9), math.pi]
KB8 = [1.0] + [float(np.float32(c)) for c in (190.978, 190.973, 254.932, 256.897, 0.00348, 0.000715, -0.00205, 0.000203)]   # the synthetic rig's left camera
PIN = [0.0] + [float(np.float32(c)) for c in (458.654, 457.296, 367.215, 248.375)] + [0.0] * 4


def unit(a):
    n = math.sqrt(sum(c * c for c in a))
    return [c / n for c in a]


def rot(axis, ang):
    """a float64 rotation matrix (rows) by Rodrigues' formula: an INPUT, correct to rounding, not a reference"""
    n = unit(axis)
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return (np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K))


def quat(axis, ang, neg=False):
    n = unit(axis)
    s = math.sin(ang / 2)
    q = [n[0] * s, n[1] * s, n[2] * s, math.cos(ang / 2)]
    return [-c for c in q] if neg else q


def f32m(M):
    return np.asarray(M, dtype=np.float32).astype(np.float64)


def _spd(rng, n, cond):
    Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
    H = (Qm * np.logspace(0, -math.log10(cond), n)) @ Qm.T
    return (H + H.T) / 2


@functools.lru_cache(maxsize=1)
def build_cases():
    rng = np.random.default_rng(20240611)
    cs = []
    IMIN, IMAX = -2 ** 31, 2 ** 31 - 1

    # ---- wave int: one-hot per lane, identities, extremes in each lane, random, wrapping sums
    for l in range(64):
        v = [0] * 64
        v[l] = 1 + l
        cs.append(Case(1, iv=v, tag="onehot%d" % l))
    for l in range(0, 64, 1):
        v = [IMIN] * 64
        v[l] = IMAX if l % 2 else 5 - l
        cs.append(Case(1, iv=v, tag="max_single%d" % l))       # wave_max: identity everywhere but one lane
        v = [-1] * 64                                           # 0xFFFFFFFF: the identity of the unsigned min
        v[l] = l * 3
        cs.append(Case(1, iv=v, tag="min_single%d" % l))
    cs.append(Case(1, iv=[IMIN] * 64, tag="all_int_min"))
    cs.append(Case(1, iv=[-1] * 64, tag="all_ffffffff"))
    for k in range(8):
        cs.append(Case(1, iv=rng.integers(-1000, 1000, 64), tag="random_small%d" % k))
        cs.append(Case(1, iv=rng.integers(IMIN, IMAX, 64, dtype=np.int64), tag="random_wrapping%d" % k))

    # ---- FP64 sums
    def wide(n):
        return (rng.choice([-1.0, 1.0], n) * rng.uniform(1, 2, n) * 2.0 ** rng.integers(-15, 15, n)).tolist()
    for l in range(64):
        v = [0.0] * 64
        v[l] = 1.0 + l / 64.0
        cs.append(Case(2, v, tag="onehot%d" % l))
    cs.append(Case(2, [2.0 ** l for l in range(64)], tag="pow2_all"))
    cs.append(Case(2, [2.0 ** l if l < 32 else 0.0 for l in range(64)], tag="pow2_low"))
    cs.append(Case(2, [2.0 ** (l - 32) if l >= 32 else 0.0 for l in range(64)], tag="pow2_high"))
    cs.append(Case(2, [2.0 ** (l % 16) * 65536.0 ** (l // 16) / 2.0 ** 20 for l in range(64)], tag="pow2_rows"))
    for k in range(8):
        cs.append(Case(2, wide(64), tag="random%d" % k))
    for t in range(0, 256, 3):
        a, b = [0.0] * 256, [0.0] * 256
        a[t] = 1.0 + t / 256.0
        b[255 - t] = 3.0 + t / 256.0
        cs.append(Case(3, a + b, tag="onehot%d" % t))
    cs.append(Case(3, [2.0 ** (t % 50) for t in range(256)] + [2.0 ** ((t * 7) % 50) for t in range(256)], tag="pow2"))
    for k in range(4):
        cs.append(Case(3, wide(512), tag="random%d" % k))
    for t in range(0, 256, 3):
        a = [0.0] * 256
        a[t] = 1.0 + t / 256.0
        cs.append(Case(4, a, tag="onehot%d" % t))
    cs.append(Case(4, [2.0 ** (t % 50) for t in range(256)], tag="pow2"))
    for k in range(4):
        cs.append(Case(4, wide(256), tag="random%d" % k))
    for k in range(10):                                         # 28 one-hot values per case, each in another thread: 280 >= 256 threads
        vals = np.zeros((256, 28))
        for v in range(28):
            vals[(28 * k + v) % 256, v] = 1.0 + v / 32.0 + k
        cs.append(Case(5, vals.ravel(), tag="onehot%d" % k))
    cs.append(Case(5, np.array([[2.0 ** ((t + 3 * v) % 50) for v in range(28)] for t in range(256)]).ravel(), tag="pow2"))
    for k in range(2):
        cs.append(Case(5, wide(256 * 28), tag="random%d" % k))

    # ---- lane_ldlt_solve
    for fid, (n, rel) in LDLT.items():
        def sysm(H, b, lam, tag, want):
            cs.append(Case(fid, list(np.asarray(H, dtype=np.float64).ravel()) + list(b) + [lam, SENTINEL], tag=tag, want=want))
        for cond in (1.0, 1e3, 1e6, 1e9, 1e12):
            for lam in (0.0, 1e-3):
                H = _spd(rng, n, cond)
                if rel and cond >= 1e12 and lam == 0.0:
                    continue                                   # (the relative pivot rule sits at 9e-13: not a case for a 1e12 system)
                sysm(H, rng.standard_normal(n), lam, "spd_cond%g_lam%g" % (cond, lam), "ok")
        for k in (0, n // 2, n - 1):
            for bad, name in ((0.0, "zero"), (-1.0, "negative"), (math.nan, "nan"), (math.inf, "inf")):
                H = np.eye(n) * 2.0
                if k > 0 and bad in (0.0, -1.0):               # a coupled pair: the pivot is (1 + bad) - (1 * 1) * 1 = bad exactly
                    H[k - 1, k - 1] = 1.0
                    H[k, k - 1] = H[k - 1, k] = 1.0
                    H[k, k] = 1.0 + bad
                else:
                    H[k, k] = bad
                sysm(H, np.arange(1.0, n + 1), 0.0, "pivot_%s_k%d" % (name, k), "fail_pos")
        for e, name in ((-40, "2^-40"), (-39, "2^-39")):
            H = np.eye(n)
            m = n // 2
            H[m, m + 1] = H[m + 1, m] = 1.0
            H[m + 1, m + 1] = 1.0 + 2.0 ** e                   # second pivot of the pair: exactly 2^e
            sysm(H, np.arange(1.0, n + 1), 0.0, "rel_delta_%s" % name, "fail_rel" if (rel and e == -40) else "ok")

    # ---- quaternion / SE3 / Sim3 products
    mats = []
    for ax in AXES:
        for ang in ANGLES:
            mats.append(("rot_%s_%g" % ("".join(map(str, ax)), ang), rot(ax, ang)))
    mats.append(("exact_180_110", np.array([[0, 1, 0], [1, 0, 0], [0, 0, -1.0]])))      # m00 == m11 > m22: the first comparison ties, i = 0
    mats.append(("exact_180_101", np.array([[0, 0, 1], [0, -1, 0], [1, 0, 0.0]])))      # m22 == m00: the second comparison ties, i = 0
    mats.append(("exact_180_011", np.array([[-1, 0, 0], [0, 0, 1], [0, 1, 0.0]])))      # m22 == m11 after i = 1: ties, i = 1
    mats.append(("exact_180_x", np.diag([1.0, -1, -1])))
    mats.append(("exact_180_y", np.diag([-1.0, 1, -1])))
    mats.append(("exact_180_z", np.diag([-1.0, -1, 1])))
    mats.append(("exact_120_111", np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0.0]])))       # trace exactly 0: not > 0
    for name, M in list(mats):
        mats.append((name + "_f32", f32m(M)))
    for name, M in mats:
        cs.append(Case(20, M.ravel(), tag=name))
    quats = []
    for ax in AXES:
        for ang in ANGLES:
            for neg in (False, True):
                quats.append(("q_%s_%g%s" % ("".join(map(str, ax)), ang, "_neg" if neg else ""), quat(ax, ang, neg)))
    for i, (name, q) in enumerate(quats):
        v = (rng.standard_normal(3) * 10.0 ** rng.integers(-3, 3)).tolist()
        t = (rng.standard_normal(3) * 10.0 ** rng.integers(-3, 3)).tolist()
        m = 0
        while abs(quat_mul(q, quats[(i * 37 + 11 + m) % len(quats)][1])[3]) < 0.01:     # (a product with w next to 0 stands on the sign test)
            m += 1
        _, q2 = quats[(i * 37 + 11 + m) % len(quats)]
        t2 = (rng.standard_normal(3) * 10.0 ** rng.integers(-3, 3)).tolist()
        s, s2 = float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.5, 2.0))
        cs.append(Case(21, q, tag=name))
        cs.append(Case(22, q + v, tag=name))
        cs.append(Case(23, [c * 1.5 for c in q], tag=name))
        cs.append(Case(24, q + t + q2 + t2, tag=name))
        cs.append(Case(25, q + t + [s] + q2 + t2 + [s2], tag=name))
        cs.append(Case(26, q + t + [s], tag=name))
        cs.append(Case(27, q + t + [s] + v, tag=name))

    # ---- pose_oplus in its three forms
    thetas = [0.0, 1e-9, 0.99e-5, 1.01e-5, 1e-3, 0.1, 0.2995, 0.3005, 1.0, 2.2, 3.1]
    oplus_axes = [(0.36, -0.48, 0.8), (-0.6, 0.64, 0.48), (0.8, 0.36, -0.48)]   # generic: no two diagonal entries of R close
    k = 0
    for th in thetas:
        for ax in oplus_axes:
            for neg in (False, True):
                om = [c * th for c in unit(ax)]
                ups = (rng.standard_normal(3) * 10.0 ** [-3, -1, 0, 2][k % 4]).tolist()
                Tq = quat(oplus_axes[(k + 1) % 3], [0.4, 2.9, 1.7][k % 3], neg)
                if k % 5 == 4:                                  # exp(u) * T with a negative w before normalisation
                    Tq = quat(ax, 3.0, False)
                Tt = (rng.standard_normal(3) * 10.0 ** [0, 2, -3, -1][k % 4]).tolist()
                for fid in (30, 31, 32):
                    cs.append(Case(fid, Tq + Tt + om + ups, tag="theta%g_%d" % (th, k)))
                k += 1

    # ---- fast_rsqrt
    for d in np.concatenate([np.linspace(0.25, 4.0, 120), 1.0 + np.linspace(-1e-3, 1e-3, 81), 1.0 + 2.0 ** -52 * np.arange(-8, 9)]):
        cs.append(Case(33, [d], tag="caller_range"))
    for e in range(-300, 301, 10):
        for m in (1.0, 1.4142135623730951, 1.9999999999999998, 3.0):
            cs.append(Case(33, [m * 2.0 ** e], tag="binade%d" % e))

    # ---- cameras
    for z in (0.05, 0.3, 1.0, 7.0, 100.0):
        for xy in ((0.01, -0.02), (0.3, 0.2), (-1.1, 0.7)):
            v = [xy[0] * z, xy[1] * z, z]
            cs.append(Case(34, PIN + v, tag="pinhole_z%g" % z))
            cs.append(Case(35, PIN + v, tag="pinhole_z%g" % z))
    for r in (1e-4, 1e-2, 0.3, 1.0, 3.0, 30.0):
        for phi in (0.3, 2.0, -2.5, -0.9):
            for z in (1.0, 0.1, -0.2, -1.0):
                if z < 0 and r < 0.3:
                    continue                                    # (behind the camera and on the axis: theta = pi, no fisheye image)
                v = [r * math.cos(phi), r * math.sin(phi), z]
                cs.append(Case(34, KB8 + v, tag="kb8_r%g_z%g" % (r, z)))
                cs.append(Case(35, KB8 + v, tag="kb8_r%g_z%g" % (r, z)))

    # ---- Sim3 exp / log
    for th in (0.0, 1e-9, 0.99e-5, 1.01e-5, 1e-2, 0.7, 2.0):
        for sg in (0.0, 1e-9, 0.99e-5, -1.01e-5, math.log(0.5), math.log(2.0), 0.05):
            ax = oplus_axes[len(cs) % 3]
            cs.append(Case(28, [c * th for c in unit(ax)] + (rng.standard_normal(3) * 3).tolist() + [sg], tag="theta%g_sigma%g" % (th, sg)))
    # log: theta on both sides of d = 1 - 1e-5 (theta = 4.4721e-3), scales on both sides of |sigma| = 1e-5
    for th in (0.0, 1e-6, 4.46e-3, 4.48e-3, 0.3, 1.5):
        for s in (1.0, 1.0 + 0.99e-5, 1.0 - 1.01e-5, 0.5, 2.0, 1.3):
            ax = oplus_axes[len(cs) % 3]
            cs.append(Case(29, quat(ax, th, len(cs) % 2 == 1) + (rng.standard_normal(3) * 3).tolist() + [s], tag="theta%g_s%g" % (th, s)))
    # the six paths of the LU: large angles, found by a seeded search with the (f64) model's own report
    need = {"p0n", "p0s", "p1n", "p1s", "p2n", "p2s"}
    tries = 0
    while need and tries < 4000:
        tries += 1
        ax = rng.standard_normal(3)
        th = float(rng.choice([2.5, 2.9, 3.1]))
        s = float(rng.choice([1.0, 0.5, 2.0]))
        dv = quat(ax, th) + (rng.standard_normal(3) * 3).tolist() + [s]
        _, br, dec, _ = evaluate(F64, 29, dv)
        path = br.split("/")[2]
        if path in need and min_margin(dec) > 1e-2:
            need.discard(path)
            cs.append(Case(29, dv, tag="lu_%s_theta%g_s%g" % (path, th, s)))
    assert not need, need
    # the tie of the first pivot: q = (0, y, y, w) makes |W10| == |W20| > |W00| exactly (omega_0 = 0, omega_1 == omega_2 bit for bit)
    y = math.sin(1.5) / math.sqrt(2.0)
    cs.append(Case(29, [0.0, y, y, math.cos(1.5), 0.3, -1.2, 2.5, 1.0], tag="lu_tie_first_pivot"))
    # The same tie where no library function takes part: s = 1 (log(1) = 0) and a quaternion that is NOT of unit length, (0, y, y, w) with
    # y = 1.1e-3 and w = 900: d = 1 - 4 y^2 takes the small-angle branch (A = 1/2, B = 1/6, k = 1/2) while omega_1 = omega_2 = 2 y w = 1.98,
    # so that |W10| = |W20| = 0.99 > |W00| = 0.31.  Only + - * / from input to output: the result is claimed bit for bit, and an
    # elimination that takes another row of the tie rounds differently.
    cs.append(Case(29, [0.0, 1.1e-3, 1.1e-3, 900.0, 0.3, -1.2, 2.5, 1.0], tag="lu_tie_first_pivot_exact_arithmetic", bits=True))

    # ---- SO3 functions of the inertial edges
    for d in (0.0, 1e-9, 0.99e-5, 1.01e-5, 1e-3, 0.5, 2.0, 3.1):
        for ax in oplus_axes:
            w = [c * d for c in unit(ax)]
            for fid in (40, 42, 43):
                cs.append(Case(fid, w, tag="d%g" % d))
            Rwg = rot(oplus_axes[(len(cs) + 1) % 3], 0.8).ravel().tolist()
            if d <= 2.0:
                cs.append(Case(45, Rwg + [w[0], w[1]], tag="d%g" % d))
                st = (rng.standard_normal(12) * 2).tolist()
                cs.append(Case(46, Rwg + st + w + (rng.standard_normal(12) * 0.1).tolist(), tag="d%g" % d))
    for th in (0.05, 0.5, 2.0, 3.0):                            # (cos stands more than 1e-3 inside [-1, 1]; nearer cases follow, held exactly)
        for ax in oplus_axes:
            cs.append(Case(41, rot(ax, th).ravel(), tag="theta%.9g" % th))
    # theta = pi - 2^-20 (pi - 0.95e-6) about each axis with cos = -1 + 2^-41 and sin = 2^-20 held exactly, so that (tr - 1) / 2 is exact in
    # float64 and stands 2^-41 inside [-1, 1] in both arithmetics: sin(theta) < 1e-5, the branch that returns the vector unscaled
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        M = np.zeros((3, 3))
        M[a, a] = 1.0
        M[b, b] = M[c, c] = -1.0 + 2.0 ** -41
        M[c, b], M[b, c] = 2.0 ** -20, -2.0 ** -20
        cs.append(Case(41, M.ravel(), tag="pi_minus_2^-20_axis%d" % a, want="unscaled"))
    # the identity plus an exactly held skew part: cos = 1 exactly, theta = 0, unscaled
    cs.append(Case(41, (np.eye(3) + np.array([[0, -2.0 ** -22, 2.0 ** -23], [2.0 ** -22, 0, -2.0 ** -21], [-2.0 ** -23, 2.0 ** -21, 0]])).ravel(), tag="identity_plus_skew", want="unscaled"))
    nearI = f32m(rot((0.36, -0.48, 0.8), 3e-4))
    assert nearI[0, 0] + nearI[1, 1] + nearI[2, 2] <= 3.0
    cs.append(Case(41, nearI.ravel(), tag="f32_near_identity"))
    over = f32m(np.eye(3) + np.array([[1.2e-7, 1e-5, 0], [-1e-5, 1.2e-7, 0], [0, 0, 0]]))
    assert over[0, 0] + over[1, 1] + over[2, 2] > 3.0
    cs.append(Case(41, over.ravel(), tag="f32_trace_above_3", want="out_of_range"))
    under = np.diag([-1.0, -1.0, 1.0]) - np.diag([2.0 ** -20, 0, 0])
    cs.append(Case(41, under.ravel(), tag="cos_below_minus_1", want="out_of_range"))
    for ang in (0.0, math.radians(90), math.radians(179.9)):
        for ax in oplus_axes:
            cs.append(Case(44, f32m(rot(ax, ang)).ravel(), tag="f32_rot_%g" % ang))

    # ---- null_vector4
    def tri_rows(parallax_deg, seed):
        r2 = np.random.default_rng(seed)
        X = np.array([0.3, -0.2, 4.0])
        b = 2 * 4.0 * math.tan(math.radians(parallax_deg) / 2)
        P1 = np.hstack([np.eye(3), np.zeros((3, 1))])
        P2 = np.hstack([rot((0, 1, 0), 0.01), np.array([[-b], [0.0], [0.0]])])
        rows = []
        for P in (P1, P2):
            x = P @ np.append(X, 1.0)
            u, v = x[0] / x[2] + r2.normal() * 1e-4, x[1] / x[2] + r2.normal() * 1e-4
            rows += [u * P[2] - P[0], v * P[2] - P[1]]
        Am = f32m(np.array(rows))
        return Am.T @ Am
    for p in (10.0, 1.0, 0.01):
        for seed in range(3):
            cs.append(Case(50, tri_rows(p, seed).ravel(), tag="parallax%g" % p))
    cs.append(Case(50, np.diag([3.0, 1.0, 2.0, 5.0]).ravel(), tag="diagonal"))
    cs.append(Case(50, np.diag([3.0, 1.0, 1.0, 2.0]).ravel(), tag="diagonal_tie"))
    cs.append(Case(50, np.diag([1.0, 3.0, 2.0, 1.0]).ravel(), tag="diagonal_tie_ends"))
    cs.append(Case(50, np.zeros(16), tag="zero"))
    Sz = np.array([[4.0, 1.0, 0, 0], [1.0, 3.0, 0, 0], [0, 0, 2.0, 0.5], [0, 0, 0.5, 1.0]])
    cs.append(Case(50, Sz.ravel(), tag="zeros_off_diagonal"))
    Sz2 = np.array([[2.0, 0, 0.3, 0], [0, 1.5, 0, 0], [0.3, 0, 1.0, 0], [0, 0, 0, 0.25]])
    cs.append(Case(50, Sz2.ravel(), tag="zeros_off_diagonal_isolated"))

    # ---- the LM step.  A verdict case: lambda, ni, currentChi, the solver's flag, the trial's chi2, computeScale's sum.
    # rho = (100 - 90) / (scale + 1e-3): the three regimes of the good-step factor (2/3 up to rho = 0.8467, 1/3 from 0.9368 on)
    for rho, want in ((0.1, "2/3"), (0.5, "2/3"), (0.8, "2/3"), (0.87, "cubic"), (0.9, "cubic"), (0.92, "cubic"), (0.96, "1/3"), (1.5, "1/3"), (10.0, "1/3")):
        cs.append(Case(60, [0.37, 2.0, 100.0, 1, 90.0, 10.0 / rho - 1e-3], tag="rho%g" % rho, want="accepted_" + want))
        cs.append(Case(61, [0.37, rho], tag="rho%g" % rho, want=want))
    cs.append(Case(61, [0.37, math.inf], tag="rho_inf", want="1/3"))
    cs.append(Case(61, [0.37, 1e-300], tag="rho_tiny", want="2/3"))
    cs.append(Case(60, [0.37, 4.0, 100.0, 1, 120.0, -40.0], tag="negative_scale_larger_chi2", want="accepted_2/3"))     # g2o's quirk: rho = 0.5
    cs.append(Case(60, [0.37, 2.0, 100.0, 1, 90.0, -1e-3], tag="zero_scale_smaller_chi2", want="accepted_1/3"))         # rho = +inf
    cs.append(Case(60, [0.37, 2.0, 100.0, 1, 110.0, 20.0], tag="rho_negative", want="rejected_rho"))
    cs.append(Case(60, [0.37, 2.0, 100.0, 1, 100.0, 20.0], tag="rho_zero", want="rejected_rho"))
    cs.append(Case(60, [0.37, 2.0, 100.0, 1, 100.0, -1e-3], tag="zero_over_zero", want="rejected_rho"))
    cs.append(Case(60, [0.37, 2.0, 100.0, 1, math.nan, 20.0], tag="chi2_nan", want="rejected_rho"))
    cs.append(Case(60, [0.37, 2.0, 100.0, 1, math.inf, 20.0], tag="chi2_inf", want="rejected_rho"))
    cs.append(Case(60, [0.37, 2.0, 100.0, 1, -math.inf, 20.0], tag="chi2_minus_inf", want="rejected_not_finite"))
    cs.append(Case(60, [0.37, 2.0, 100.0, 0, 1.0, 20.0], tag="refused_solve_small_chi2", want="rejected_rho"))
    # rejections in a row: each case starts from what the one before it must leave (ni = 2 -> 4 -> 8 -> 16)
    state = [0.37, 2.0, 100.0]
    for k in range(3):
        cs.append(Case(60, state + [1, 110.0 + k, 20.0], tag="rejection_%d_in_a_row" % (k + 1), want="rejected_rho"))
        state = lm_trial_verdict(*cs[-1].dv)[0][2:5]
    assert state[1] == 16.0
    # the end of an iteration: currentChi, nBad, trials exhausted, rho, iniChi.  0.05 % and 0.2 % of iniChi stand either side of the 0.1 %
    cs.append(Case(62, [90.0, 0, 1, -0.5, 100.0], tag="trials_exhausted", want="exhausted"))
    cs.append(Case(62, [100.0, 1, 0, 0.0, 100.0], tag="rho_zero", want="rho_zero"))
    cs.append(Case(62, [99.95, 0, 0, 0.4, 100.0], tag="improved_0.05%_nbad_0", want="bad"))
    cs.append(Case(62, [99.95, 1, 0, 0.4, 100.0], tag="improved_0.05%_nbad_1", want="bad"))
    cs.append(Case(62, [99.95, 2, 0, 0.4, 100.0], tag="improved_0.05%_nbad_2", want="bad_stop"))
    cs.append(Case(62, [99.8, 2, 0, 0.4, 100.0], tag="improved_0.2%_nbad_2", want="good"))
    cs.append(Case(62, [99.8, 0, 0, 0.4, 100.0], tag="improved_0.2%_nbad_0", want="good"))
    cs.append(Case(62, [100.0, 0, 0, -0.3, 100.0], tag="every_trial_rejected", want="bad"))
    cs.append(Case(63, [0.5, 123.456], tag="user", want="user"))
    cs.append(Case(63, [0.0, 123.456], tag="user_zero", want="diagonal"))
    cs.append(Case(63, [-1.0, 123.456], tag="user_negative", want="diagonal"))
    cs.append(Case(63, [0.0, 0.0], tag="zero_diagonal", want="diagonal"))
    for chi2_95 in (5.991, 7.815):                              # the thresholds of the reprojection edges, float as the reference holds them
        delta = float(np.float32(math.sqrt(chi2_95)))
        dsqr = delta * delta
        cs.append(Case(64, [1.25, delta, dsqr], tag="below_%g" % chi2_95, want="inlier"))
        cs.append(Case(64, [dsqr, delta, dsqr], tag="at_%g" % chi2_95, want="inlier"))
        cs.append(Case(64, [float(np.nextafter(dsqr, math.inf)), delta, dsqr], tag="next_above_%g" % chi2_95, want="outlier"))
        cs.append(Case(64, [10.0, delta, dsqr], tag="above_%g" % chi2_95, want="outlier"))
        cs.append(Case(64, [3.7e6, delta, dsqr], tag="far_above_%g" % chi2_95, want="outlier"))
        cs.append(Case(64, [0.0, delta, dsqr], tag="zero_%g" % chi2_95, want="inlier"))
        cs.append(Case(64, [math.nan, delta, dsqr], tag="nan_%g" % chi2_95, want="outlier"))
    return cs


def min_margin(dec):
    """the smallest relative distance of a Decide's comparisons from their thresholds"""
    m = math.inf
    for lhs, _, rhs, scale in dec.compares:
        m = min(m, compare_margin(lhs, rhs, scale))
    return m


def compare_margin(lhs, rhs, scale):
    lhs, rhs = mpmath.mpf(lhs), mpmath.mpf(rhs)
    if scale is None:                                          # d > 1 - eps: (1 - d) against eps
        lhs, rhs, scale = 1 - lhs, 1 - rhs, 1e-5
    return float(abs(lhs - rhs) / max(abs(lhs), abs(rhs), mpmath.mpf(scale)))


# ------------------------------------------------------------------------------------------------ files
def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", 0x444d5431, len(cases)))
        for c in cases:
            f.write(struct.pack("<iiii", c.fid, len(c.iv), len(c.dv), 0))
            iv = c.iv + [0] * (len(c.iv) & 1)
            f.write(struct.pack("<%di" % len(iv), *iv))
            f.write(np.asarray(c.dv, dtype="<f8").tobytes())


def read_outputs(path, cases):
    buf = open(path, "rb").read()
    magic, n = struct.unpack_from("<ii", buf, 0)
    assert magic == 0x444d5432 and n == len(cases), (magic, n)
    off, outs = 8, []
    for c in cases:
        fid, k = struct.unpack_from("<ii", buf, off)
        assert fid == c.fid and k in (0, FNS[fid][3]), (fid, c.fid, k)
        outs.append(np.frombuffer(buf, dtype="<f8", count=k, offset=off + 8).copy())
        off += 8 + 8 * k
    assert off == len(buf)
    return outs


# ------------------------------------------------------------------------------------------------ expected values
class Ref:
    """What one case must give: f64 / mp outputs (None where the comparison is exact or special), the branch of each, the decisions."""
    __slots__ = ("f64", "mp", "branch", "mp_branch", "dec64", "decmp", "rnd64", "rndmp", "exact")


@functools.lru_cache(maxsize=1)
def references():
    """-> list of Ref, one per case of build_cases(); computed once per process"""
    refs = []
    with mpmath.workdps(MP_DPS):
        for c in build_cases():
            r = Ref()
            r.exact = r.f64 = r.mp = None
            r.dec64 = r.decmp = None
            r.rnd64 = r.rndmp = ()
            r.mp_branch = None
            fid = c.fid
            if fid == 1:
                r.exact, r.branch = np.array(wave_int(c.iv)), "-"
            elif fid == 2:
                r.exact, r.branch = np.full(64, wave_tree_sum(c.dv)), "-"
                r.mp = [mpmath.fsum(mpmath.mpf(x) for x in c.dv)]
            elif fid == 3:
                r.exact, r.branch = np.concatenate([np.full(256, block_sum(c.dv[0:256])), np.full(256, block_sum(c.dv[256:512]))]), "-"
                r.mp = [mpmath.fsum(mpmath.mpf(x) for x in c.dv[0:256]), mpmath.fsum(mpmath.mpf(x) for x in c.dv[256:512])]
            elif fid == 4:
                r.exact, r.branch = np.array([block_sum(c.dv)]), "-"
                r.mp = [mpmath.fsum(mpmath.mpf(x) for x in c.dv)]
            elif fid == 5:
                vals = np.array(c.dv).reshape(256, 28)
                r.exact, r.branch = np.array(lm_block_reduce(vals)), "-"
                r.mp = [mpmath.fsum(mpmath.mpf(float(x)) for x in vals[:, v]) for v in range(28)]
            elif fid in LDLT:
                n, rel = LDLT[fid]
                H = np.array(c.dv[0:n * n]).reshape(n, n)
                b, lam = c.dv[n * n:n * n + n], c.dv[n * n + n]
                x, r.branch = ldlt_solve(F64, H, b, lam, rel)
                xm, r.mp_branch = ldlt_solve(MP, H, b, lam, rel)
                if x is None:
                    r.exact = np.array([0.0, 0.0] + [SENTINEL] * (2 * n))
                    r.f64 = r.mp = None
                else:
                    r.exact = np.array([1.0, 1.0] + x + x)
                    r.f64, r.mp = x, xm
            elif fid == 33:
                d = mpmath.mpf(c.dv[0])
                r.mp = [1 / mpmath.sqrt(d)]
                r.f64 = [float(r.mp[0])]                       # the correctly rounded 1 / sqrt(d)
                r.branch = "-"
            elif fid == 50:
                S = np.array(c.dv).reshape(4, 4)
                w, V = np.linalg.eigh(S)
                E, Vm = mpmath.eigsy(mpmath.matrix(S.tolist()))
                r.f64 = (w, V)
                r.mp = ([E[i] for i in range(4)], [[Vm[i, j] for i in range(4)] for j in range(4)])    # eigenvalues ascending, vectors as rows
                diag = not np.any(S - np.diag(np.diag(S)))
                r.branch = "diagonal" if diag else "sweeps"
                if diag:
                    m = int(np.argmin(np.diag(S)))             # numpy's argmin: the first of equal entries
                    r.exact = np.array([1.0 if i == m else 0.0 for i in range(4)] + list(np.diag(S)))
            elif fid in LM_STEP:
                out, r.branch = LM_STEP[fid](*c.dv)
                r.exact = np.array([SENTINEL if math.isnan(v) else float(v) for v in out])     # the harness writes a NaN as the sentinel
            else:
                out, r.branch, r.dec64, r.rnd64 = evaluate(F64, fid, c.dv)
                outm, r.mp_branch, r.decmp, r.rndmp = evaluate(MP, fid, c.dv, force=r.dec64.taken)
                # (mp) was walked down the branch of (f64); its own decisions are in r.decmp.compares for the tests to look at
                r.f64, r.mp = [float(v) for v in out], outm
                if FNS[fid][5] or c.bits:
                    r.exact = np.array(r.f64)
            refs.append(r)
    return refs


def ulp(x):
    x = abs(float(x))
    return math.ulp(x) if x > 0 else 0.0


def part_list(fid):
    parts = FNS[fid][6]
    return parts if parts else [("out", 0, FNS[fid][3])]


def distance(a, b_mp, lo, hi):
    """largest |a - b| over the components lo..hi, b in mpmath"""
    with mpmath.workdps(MP_DPS):
        return float(max(abs(mpmath.mpf(float(a[i])) - b_mp[i]) for i in range(lo, hi)))


def yardsticks(cases, refs, fids):
    """-> {(fid, branch, part): largest distance of (f64) from (mp) over the cases of that function and branch}"""
    y = {}
    for c, r in zip(cases, refs):
        if c.fid not in fids or r.mp is None or c.fid in (33, 50) or c.fid <= 5:
            continue
        for name, lo, hi in part_list(c.fid):
            key = (c.fid, r.branch, name)
            y[key] = max(y.get(key, 0.0), distance(r.f64, r.mp, lo, hi))
    return y


def tolerance_ratio(c, r, got, ystick):
    """the yardstick rule for one case: the worst, over the output's parts, of  distance(got, mp) / max(yardstick, 1 ulp of the part's
    largest component).  The test asserts ratio <= MARGIN."""
    worst = 0.0
    for name, lo, hi in part_list(c.fid):
        with mpmath.workdps(MP_DPS):
            big = max(abs(float(r.mp[i])) for i in range(lo, hi))
        floor = ulp(big) if big > 0 else 5e-324
        y = max(ystick.get((c.fid, r.branch, name), 0.0), floor)
        worst = max(worst, distance(got, r.mp, lo, hi) / y)
    return worst
