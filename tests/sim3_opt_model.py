"""Checker for OptimizeSim3: a numpy restatement of the numerical core of Optimizer::OptimizeSim3 (S/Optimizer.cc:4031-4310, the
overload LoopClosing calls) and of what it runs inside g2o, vectorised over the edge pairs and parametrised by dtype.

dtype = float64 follows the reference: double wherever g2o and Eigen hold a double, float32 where the reference holds a float (the
camera-frame points, the keypoints, invSigma2, th2 and sqrt(th2)).  dtype = numpy.longdouble (80-bit where LONGDOUBLE_OK) evaluates
the same statements with 11 more bits and is the yardstick for how much of a float64 result is rounding.

Restated, with the lines they come from:
  Sim3(Vector7d), operator*, inverse, map            G/types/sim3.h:70-142, 266-272, 233-236, 144-146
  VertexSim3Expmap::oplusImpl                         I/OptimizableTypes.h:158-167
  the two computeError                                I/OptimizableTypes.h:183-190, 204-211; S/CameraModels/Pinhole.cpp:41-47
  numeric Jacobian (both linearizeOplus commented)    G/core/base_binary_edge.hpp:130-205
  constructQuadraticForm, robustInformation           G/core/base_binary_edge.hpp:55-120
  RobustKernelHuber::robustify                        G/core/robust_kernel_impl.cpp:78-91
  the Levenberg-Marquardt driver                      G/core/optimization_algorithm_levenberg.cpp:61-194, sparse_optimizer.cpp:354-419
  LinearSolverDense                                   G/solvers/linear_solver_dense.h:65-113
  the collection loop and the two rounds              S/Optimizer.cc:4083-4223, 4227-4309

Eigen is not part of the reference's source.  The choices E-1 .. E-9 made for what happens inside its calls are listed at the top of
multi_orbslam3_amd/csrc/sim3_opt.hip and restated at the lines below that apply them.

Nothing here is used by the product; the product is compared WITH it.
"""
import numpy as np

import sim3_model as sm

L = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(L).eps < 2e-19)
DBL_MAX = np.finfo(np.float64).max


# ------------------------------------------------------------------ quaternions (x, y, z, w) and 3-vectors

def quat_from_R(m, F):
    """E-1: Eigen::Quaterniond(Matrix3d) -- trace > 0: w from sqrt(trace + 1); else the largest diagonal entry.  Not renormalised."""
    t = m[0][0] + m[1][1] + m[2][2]
    q = [F(0)] * 4
    if t > 0:
        t = np.sqrt(t + F(1))
        q[3] = F(0.5) * t
        t = F(0.5) / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i][i] - m[j][j] - m[k][k] + F(1))
        q[i] = F(0.5) * t
        t = F(0.5) / t
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return q


def quat_rotate(q, v):
    """E-2: Quaterniond * Vector3d -- uv = 2 (q.vec x v); v + w uv + q.vec x uv, summed in that order.  v: three scalars or arrays."""
    uv0 = 2 * (q[1] * v[2] - q[2] * v[1])
    uv1 = 2 * (q[2] * v[0] - q[0] * v[2])
    uv2 = 2 * (q[0] * v[1] - q[1] * v[0])
    return [v[0] + q[3] * uv0 + (q[1] * uv2 - q[2] * uv1),
            v[1] + q[3] * uv1 + (q[2] * uv0 - q[0] * uv2),
            v[2] + q[3] * uv2 + (q[0] * uv1 - q[1] * uv0)]


def quat_mul(a, b):
    """E-3: Quaterniond * Quaterniond, each component left to right."""
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


# ------------------------------------------------------------------ g2o::Sim3 as (q[4], t[3], s)

def sim3_exp(u, F):
    """Sim3(const Vector7d& update), sim3.h:70-142, all four branches.  E-4: the 3x3 products and W * upsilon are row-by-column sums in k
    order, the sums of matrices left to right."""
    om = [F(u[0]), F(u[1]), F(u[2])]
    up = [F(u[3]), F(u[4]), F(u[5])]
    sigma = F(u[6])
    with np.errstate(all="ignore"):
        theta = np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
        z = F(0)
        Om = [[z, -om[2], om[1]], [om[2], z, -om[0]], [-om[1], om[0], z]]
        s = np.exp(sigma)
        Om2 = [[Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j] for j in range(3)] for i in range(3)]
        I = [[F(1) if i == j else F(0) for j in range(3)] for i in range(3)]
        eps = F(0.00001)

        def small_R():
            return [[I[i][j] + Om[i][j] + Om2[i][j] for j in range(3)] for i in range(3)]

        def full_R():
            a = np.sin(theta) / theta
            b = (1 - np.cos(theta)) / (theta * theta)
            return [[I[i][j] + a * Om[i][j] + b * Om2[i][j] for j in range(3)] for i in range(3)]

        if abs(sigma) < eps:
            C = F(1)
            if theta < eps:
                A = F(1.) / F(2.)
                B = F(1.) / F(6.)
                R = small_R()
            else:
                theta2 = theta * theta
                A = (1 - np.cos(theta)) / theta2
                B = (theta - np.sin(theta)) / (theta2 * theta)
                R = full_R()
        else:
            C = (s - 1) / sigma
            if theta < eps:
                sigma2 = sigma * sigma
                A = ((sigma - 1) * s + 1) / sigma2
                B = ((F(0.5) * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
                R = small_R()
            else:
                R = full_R()
                a = s * np.sin(theta)
                b = s * np.cos(theta)
                theta2 = theta * theta
                sigma2 = sigma * sigma
                c = theta2 + sigma2
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) * F(1.) / theta2
        r = quat_from_R(R, F)
        W = [[A * Om[i][j] + B * Om2[i][j] + C * I[i][j] for j in range(3)] for i in range(3)]
        t = [W[i][0] * up[0] + W[i][1] * up[1] + W[i][2] * up[2] for i in range(3)]
    return (r, t, s)


def sim3_mul(a, b):
    """operator*, sim3.h:266-272 (E-7): r = r * o.r; t = s * (r * o.t) + t; s = s * o.s."""
    rt = quat_rotate(a[0], b[1])
    return (quat_mul(a[0], b[0]), [a[2] * rt[0] + a[1][0], a[2] * rt[1] + a[1][1], a[2] * rt[2] + a[1][2]], a[2] * b[2])


def sim3_inverse(a):
    """inverse(), sim3.h:233-236 (E-6): Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)."""
    r, t, s = a
    with np.errstate(all="ignore"):
        rc = [-r[0], -r[1], -r[2], r[3]]
        k = -1. / s
        return (rc, quat_rotate(rc, [k * t[0], k * t[1], k * t[2]]), 1. / s)


def sim3_map(a, X):
    """map(), sim3.h:144-146: s * (r * xyz) + t.  X: three arrays."""
    rx = quat_rotate(a[0], X)
    return [a[2] * rx[0] + a[1][0], a[2] * rx[1] + a[1][1], a[2] * rx[2] + a[1][2]]


def oplus(est, update, fix_scale, F):
    """VertexSim3Expmap::oplusImpl, I/OptimizableTypes.h:158-167: update[6] = 0 INSIDE when _fix_scale, then Sim3(update) * estimate."""
    u = [F(v) for v in update]
    if fix_scale:
        u[6] = F(0)
    return sim3_mul(sim3_exp(u, F), est)


def sim3_matrix(q, t, s):
    """[sR t; 0 1] as 4 x 4 float64 (Eigen's toRotationMatrix of the quaternion as it is)."""
    x, y, z, w = [float(v) for v in q]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    T = np.eye(4)
    T[:3, :3] = float(s) * R
    T[:3, 3] = [float(v) for v in t]
    return T


# ------------------------------------------------------------------ the flat problem

class Problem:
    """What orbm_sim3opt_problem carries: X1 / X2 (n x 3 float32, P3D1c / P3D2c), obs1 / obs2 (n x 2 float32), w1 / w2 (n float32,
    invSigmaSquare), K1 / K2 (fx fy cx cy float32), fix_scale, th2 (float32), q / t / s (float64, g2oS12), n_corr."""

    def __init__(self, X1, X2, obs1, obs2, w1, w2, K1, K2, fix_scale, th2, q, t, s, n_corr=None):
        f = np.float32
        self.X1 = np.ascontiguousarray(X1, f).reshape(-1, 3)
        self.X2 = np.ascontiguousarray(X2, f).reshape(-1, 3)
        self.obs1 = np.ascontiguousarray(obs1, f).reshape(-1, 2)
        self.obs2 = np.ascontiguousarray(obs2, f).reshape(-1, 2)
        self.w1 = np.ascontiguousarray(w1, f).reshape(-1)
        self.w2 = np.ascontiguousarray(w2, f).reshape(-1)
        self.K1 = np.asarray(K1, f)
        self.K2 = np.asarray(K2, f)
        self.fix_scale = bool(fix_scale)
        self.th2 = f(th2)
        self.q = np.asarray(q, np.float64).copy()
        self.t = np.asarray(t, np.float64).copy()
        self.s = np.float64(s)
        self.n = len(self.X1)
        self.n_corr = self.n if n_corr is None else int(n_corr)


class _Edges:
    """The problem's arrays in dtype F (every float is promoted exactly)."""

    def __init__(self, p, F):
        self.n = p.n
        self.X1 = [p.X1[:, k].astype(F) for k in range(3)]
        self.X2 = [p.X2[:, k].astype(F) for k in range(3)]
        self.o1 = [p.obs1[:, k].astype(F) for k in range(2)]
        self.o2 = [p.obs2[:, k].astype(F) for k in range(2)]
        self.w1 = p.w1.astype(F)
        self.w2 = p.w2.astype(F)
        self.K1 = [F(v) for v in p.K1]
        self.K2 = [F(v) for v in p.K2]
        self.delta = F(np.sqrt(np.float32(p.th2)))          # const float deltaHuber = sqrt(th2), :4073
        self.dsqr = self.delta * self.delta                  # RobustKernel::setDelta
        self.th2 = F(p.th2)


def _project(K, P):
    """Pinhole::project(Eigen::Vector3d), Pinhole.cpp:41-47: fx * x / z + cx, left to right; nothing special-cases z <= 0."""
    return [K[0] * P[0] / P[2] + K[2], K[1] * P[1] / P[2] + K[3]]


def errors(E, est):
    """computeError of every pair: e12 = obs1 - project1(S12.map(X2)), e21 = obs2 - project2(S12.inverse().map(X1))."""
    with np.errstate(all="ignore"):
        p1 = _project(E.K1, sim3_map(est, E.X2))
        p2 = _project(E.K2, sim3_map(sim3_inverse(est), E.X1))
        return [E.o1[0] - p1[0], E.o1[1] - p1[1]], [E.o2[0] - p2[0], E.o2[1] - p2[1]]


def chi2_of(e, w):
    """BaseEdge::chi2(): _error.dot(information() * _error) with information = I * invSigma2."""
    with np.errstate(all="ignore"):
        return e[0] * (w * e[0]) + e[1] * (w * e[1])


def huber(c, delta, dsqr):
    """RobustKernelHuber::robustify, robust_kernel_impl.cpp:78-91 -> rho[0], rho[1]; `e <= dsqr` as written (NaN takes the else branch)."""
    with np.errstate(all="ignore"):
        inl = c <= dsqr
        sq = np.sqrt(c)
        return np.where(inl, c, 2 * sq * delta - dsqr), np.where(inl, np.ones_like(c), delta / sq)


def _sum_edges(v12, v21, act):
    """Serial sum in the order the edges were added: e12(0), e21(0), e12(1), ... over the active pairs."""
    a = np.stack([v12[act], v21[act]], 1).reshape(-1)
    if a.size == 0:
        return a.dtype.type(0)
    return np.add.accumulate(a)[-1]                           # (accumulate adds one element after the other; np.sum would pair them)


def jacobians(E, est, fix_scale, F):
    """BaseBinaryEdge::linearizeOplus, base_binary_edge.hpp:176-197, for the Sim3 vertex: central differences, delta = 1e-9, through
    oplusImpl.  -> J12, J21 as [row][column] arrays over the pairs.  With fix_scale both perturbed estimates of column 7 are
    Sim3(0) * estimate: the column is exactly zero."""
    delta = F(1e-9)
    scalar = F(1.0) / (2 * delta)
    J12 = [[None] * 7, [None] * 7]
    J21 = [[None] * 7, [None] * 7]
    with np.errstate(all="ignore"):
        for d in range(7):
            add = [F(0)] * 7
            add[d] = delta
            a12, a21 = errors(E, oplus(est, add, fix_scale, F))
            add[d] = -delta
            b12, b21 = errors(E, oplus(est, add, fix_scale, F))
            for k in range(2):
                J12[k][d] = scalar * (a12[k] - b12[k])
                J21[k][d] = scalar * (a21[k] - b21[k])
    return J12, J21


def solve7(H, b, lam, F):
    """LinearSolverDense::solve, linear_solver_dense.h:65-113: Eigen::LDLT, the step refused unless isPositive().  E-5: no pivoting,
    left-looking in ascending k, every pivot has to be positive and finite.  -> x or None (x is then left as it was)."""
    n = 7
    A = [[H[i][j] + (lam if i == j else F(0)) for j in range(n)] for i in range(n)]
    D = [F(0)] * n
    ok = True
    with np.errstate(all="ignore"):
        for k in range(n):
            d = A[k][k]
            if not (d > 0) or np.isinf(d):
                ok = False
            D[k] = d
            Lk = [A[i][k] / d for i in range(n)]
            for i in range(n):
                for j in range(k + 1, n):
                    A[i][j] = A[i][j] - (Lk[i] * Lk[j]) * d
            for i in range(n):
                A[i][k] = Lk[i]
        if not ok:
            return None
        y = list(b)
        for k in range(n - 1):
            for i in range(k + 1, n):
                y[i] = y[i] - A[i][k] * y[k]
        y = [y[i] / D[i] for i in range(n)]
        x = [F(0)] * n
        for i in range(n - 1, -1, -1):
            sv = y[i]
            for k in range(i + 1, n):
                sv = sv - A[k][i] * x[k]
            x[i] = sv
    return x


class _State:
    pass


def lm_optimize(E, st, act, robust, iterations, fix_scale, F, rnd, trace):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg::solve.  st: est, x (the solver's x survives a failed
    solve), c1 / c2 (chi2 of the LAST evaluation of every pair -- pop() restores estimates, not errors).  -> iterations run, last
    accepted activeRobustChi2."""
    if not act.any():
        return 0, F(0)                                        # _ivMap.size() == 0: optimize() returns at once, sparse_optimizer.cpp:356
    lam = ni = F(0)
    nbad = 0
    done = 0
    cur = F(0)
    with np.errstate(all="ignore"):
        for it in range(iterations):
            # computeActiveErrors, activeRobustChi2 (:75-85)
            e12, e21 = errors(E, st.est)
            c1, c2 = chi2_of(e12, E.w1), chi2_of(e21, E.w2)
            st.c1, st.c2 = c1, c2
            if robust:
                r1, w1 = huber(c1, E.delta, E.dsqr)
                r2, w2 = huber(c2, E.delta, E.dsqr)
            else:
                r1, w1, r2, w2 = c1, np.ones_like(c1), c2, np.ones_like(c2)
            cur = _sum_edges(r1, r2, act)
            ini = cur
            # buildSystem (:87): linearizeOplus restores _error, constructQuadraticForm per edge
            J12, J21 = jacobians(E, st.est, fix_scale, F)
            H = [[F(0)] * 7 for _ in range(7)]
            b = [F(0)] * 7
            wo1, wo2 = w1 * E.w1, w2 * E.w2                    # robustInformation: rho[1] * information (E-8: diagonal, one scalar)
            or1 = [-(E.w1 * e12[k]) * w1 for k in range(2)]    # omega_r = -omega * _error; omega_r *= rho[1]
            or2 = [-(E.w2 * e21[k]) * w2 for k in range(2)]
            for i in range(7):
                for j in range(i, 7):
                    h = _sum_edges((J12[0][i] * wo1) * J12[0][j] + (J12[1][i] * wo1) * J12[1][j],
                                   (J21[0][i] * wo2) * J21[0][j] + (J21[1][i] * wo2) * J21[1][j], act)
                    H[i][j] = H[j][i] = h
                b[i] = _sum_edges(J12[0][i] * or1[0] + J12[1][i] * or1[1], J21[0][i] * or2[0] + J21[1][i] * or2[1], act)
            if it == 0:
                # computeLambdaInit (:171-185): std::max(fabs(h_jj), maxDiagonal) returns its FIRST argument unless it is smaller
                md = F(0)
                for j in range(7):
                    a = abs(H[j][j])
                    md = md if a < md else a
                lam = F(1e-5) * md
                ni = F(2)
                nbad = 0
            rho = F(0)
            qmax = 0
            while True:
                x = solve7(H, b, lam, F)
                ok2 = x is not None
                if ok2:
                    st.x = x
                trial = oplus(st.est, st.x, fix_scale, F)      # update() runs also after a failed solve, with the x that is there
                if fix_scale:
                    st.x = list(st.x)
                    st.x[6] = F(0)                             # oplusImpl writes the zero into the solver's x (const_cast)
                t12, t21 = errors(E, trial)
                c1, c2 = chi2_of(t12, E.w1), chi2_of(t21, E.w2)
                st.c1 = np.where(act, c1, st.c1)
                st.c2 = np.where(act, c2, st.c2)
                if robust:
                    r1 = huber(c1, E.delta, E.dsqr)[0]
                    r2 = huber(c2, E.delta, E.dsqr)[0]
                else:
                    r1, r2 = c1, c2
                tmp = _sum_edges(r1, r2, act)
                if not ok2:
                    tmp = F(DBL_MAX)
                rho = cur - tmp
                scale = F(0)
                for j in range(7):
                    scale = scale + st.x[j] * (lam * st.x[j] + b[j])
                scale = scale + F(1e-3)
                rho = rho / scale
                if rho > 0 and np.isfinite(tmp):
                    alpha = 1. - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1)
                    up = F(2.) / F(3.)
                    lo = F(1.) / F(3.)
                    alpha = up if up < alpha else alpha         # std::min(alpha, _goodStepUpperScale)
                    sf = alpha if lo < alpha else lo            # std::max(_goodStepLowerScale, alpha)
                    lam = lam * sf
                    ni = F(2)
                    cur = tmp
                    st.est = trial
                else:
                    lam = lam * ni
                    ni = ni * 2
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            done += 1
            trace.append((rnd, float(lam), float(cur), qmax))
            if qmax == 10 or rho == 0:
                break
            if (ini - cur) * F(1e3) < ini:
                nbad += 1
            else:
                nbad = 0
            if nbad >= 3:
                break
    return done, cur


def optimize_sim3(p, F=np.float64, classify_round1_from="last_trial"):
    """S/Optimizer.cc:4227-4309 on the flat problem.  classify_round1_from = "recomputed" is NOT the reference: it classifies round 1
    from errors recomputed at the accepted estimate, to show that rule 1 (chi2() without computeError() at :4241) is observable."""
    E = _Edges(p, F)
    n = p.n
    st = _State()
    st.est = ([F(v) for v in p.q], [F(v) for v in p.t], F(p.s))
    st.x = [F(0)] * 7
    st.c1 = np.zeros(n, F)
    st.c2 = np.zeros(n, F)
    removed = np.zeros(n, np.uint8)
    edge_chi2 = np.zeros((4, n), F)
    trace = []
    out = dict(n_in=0, returned_early=False, n_bad_round1=0, removed=removed, trace=trace, edge_chi2=edge_chi2, iters=[0, 0],
               chi2=[F(0), F(0)], q=np.array(p.q, F), t=np.array(p.t, F), s=F(p.s))
    act = np.ones(n, bool)
    out["iters"][0], out["chi2"][0] = lm_optimize(E, st, act, True, 5, p.fix_scale, F, 0, trace)      # optimize(5), :4229
    if classify_round1_from == "recomputed":
        e12, e21 = errors(E, st.est)
        st.c1, st.c2 = chi2_of(e12, E.w1), chi2_of(e21, E.w2)
    with np.errstate(all="ignore"):
        bad = (st.c1 > E.th2) | (st.c2 > E.th2)                # :4241, NaN > th2 is false: the pair stays
    edge_chi2[0], edge_chi2[1] = st.c1, st.c2
    removed[bad] = 1
    nbad = int(bad.sum())
    out["n_bad_round1"] = nbad
    if p.n_corr - nbad < 10:                                   # :4271: return 0 WITHOUT writing g2oS12
        out["returned_early"] = True
        return out
    act = ~bad
    out["iters"][1], out["chi2"][1] = lm_optimize(E, st, act, False, 10 if nbad > 0 else 5, p.fix_scale, F, 1, trace)   # :4277
    e12, e21 = errors(E, st.est)                               # computeError, :4288-4289
    d1, d2 = chi2_of(e12, E.w1), chi2_of(e21, E.w2)
    with np.errstate(all="ignore"):
        bad2 = act & ((d1 > E.th2) | (d2 > E.th2))
    edge_chi2[2], edge_chi2[3] = np.where(act, d1, 0), np.where(act, d2, 0)
    removed[bad2] = 2
    out["n_in"] = int((act & ~bad2).sum())
    out["q"], out["t"], out["s"] = np.array(st.est[0], F), np.array(st.est[1], F), F(st.est[2])
    return out


# ------------------------------------------------------------------ the collection loop on plain arrays, :4083-4223

def camera_point(Rcw, tcw, Pw):
    """R * P + t on CV_32F matrices: one gemm, every entry accumulated in double in k order, the translation added in double, one
    rounding to float (choice C-2 of csrc/sim3.hip; INTEGRATION.md 3f, rule 3)."""
    Rcw = np.asarray(Rcw, np.float32).astype(np.float64)
    P = np.asarray(Pw, np.float32).astype(np.float64)
    t = np.asarray(tcw, np.float32).astype(np.float64)
    return np.array([((Rcw[i, 0] * P[0] + Rcw[i, 1] * P[1]) + Rcw[i, 2] * P[2]) + t[i] for i in range(3)]).astype(np.float32)


def collect(kf1, kf2, matches1, mps, all_points, K1, K2, fix_scale, th2, q, t, s):
    """kf: dict(R, t (Tcw, float32), keys (N x 2 float32, mvKeysUn[i].pt), octave (N), inv_level_sigma2 (levels), mp (N: map point id
    or -1, GetMapPointMatches)).  matches1: N map point ids or -1 (vpMatches1).  mps: dict(pos (M x 3 float32), bad (M), idx_in_kf2
    (M: GetIndexInKeyFrame(pKF2) or -1), track_scale_level (M)).  -> Problem, vnIndexEdge, counters."""
    f = np.float32
    X1, X2, o1, o2, w1, w2, index = [], [], [], [], [], [], []
    cnt = dict(nCorrespondences=0, nBadMPs=0, nInKF2=0, nOutKF2=0, nMatchWithoutMP=0)
    for i in range(len(matches1)):
        if matches1[i] < 0:                                   # :4085
            continue
        m1, m2 = int(kf1["mp"][i]), int(matches1[i])
        i2 = int(mps["idx_in_kf2"][m2])
        if m1 >= 0:
            if mps["bad"][m1] or mps["bad"][m2]:              # :4104
                cnt["nBadMPs"] += 1
                continue
            P1 = camera_point(kf1["R"], kf1["t"], mps["pos"][m1])
            P2 = camera_point(kf2["R"], kf2["t"], mps["pos"][m2])
        else:
            cnt["nMatchWithoutMP"] += 1                       # :4128-4146: pMP2->isBad() is read, the pair is skipped either way
            continue
        if i2 < 0 and not all_points:                         # :4148
            continue
        if P2[2] < 0:                                         # :4154, on the float
            continue
        cnt["nCorrespondences"] += 1
        o1.append(kf1["keys"][i])
        w1.append(f(kf1["inv_level_sigma2"][int(kf1["octave"][i])]))
        if i2 >= 0:
            o2.append(kf2["keys"][i2])
            w2.append(f(kf2["inv_level_sigma2"][int(kf2["octave"][i2])]))
            cnt["nInKF2"] += 1
        else:
            # rule 2 (:4192-4210): NORMALISED coordinates as the observation; cv::KeyPoint(Point2f, mnTrackScaleLevel) sets `size`,
            # the octave stays 0: invSigmaSquare2 = mvInvLevelSigma2[0]
            with np.errstate(all="ignore"):
                invz = f(1) / P2[2]
                o2.append(np.array([P2[0] * invz, P2[1] * invz], f))
            w2.append(f(kf2["inv_level_sigma2"][0]))
            cnt["nOutKF2"] += 1
        X1.append(P1)
        X2.append(P2)
        index.append(i)
    n = len(index)
    z3, z2 = np.zeros((0, 3), f), np.zeros((0, 2), f)
    p = Problem(np.array(X1, f) if n else z3, np.array(X2, f) if n else z3, np.array(o1, f) if n else z2, np.array(o2, f) if n else z2,
                np.array(w1, f), np.array(w2, f), K1, K2, fix_scale, th2, q, t, s, cnt["nCorrespondences"])
    return p, np.array(index, np.int32), cnt


# ------------------------------------------------------------------ seeded scenes

def make_problem(seed, n, fix_scale, outlier_fraction, out_kf2=0.15, th2=10.0, special=None):
    """A flat problem from sim3_model.make_scene: observations = projections + level noise, a fraction of gross 3-D mismatches, a
    fraction of the matches outside KF2 (rule 2's observation and weight), the start a disturbed truth as a RANSAC hypothesis from three
    noisy points would be.  special = "z0": pair 0 has X2 = 0 and the start has t_z = 0, so S12.map(X2) has z = 0 exactly;
    special = "nan": obs1 of pair 0 is NaN."""
    sc = sm.make_scene(seed, n, fix_scale, outlier_fraction)
    rng = np.random.default_rng(seed + 77)
    f = np.float32
    X1, X2 = sc["X1"], sc["X2"]
    K1, K2 = np.array(sc["K1"], f), np.array(sc["K2"], f)
    sig = sm.level_sigma2()
    inv = (f(1) / sig).astype(f)
    oc1, oc2 = rng.integers(0, 8, n), rng.integers(0, 8, n)

    def proj(K, X):
        Xd = X.astype(np.float64)
        return np.stack([K[0] * Xd[:, 0] / Xd[:, 2] + K[2], K[1] * Xd[:, 1] / Xd[:, 2] + K[3]], 1)
    obs1 = (proj(K1, X1) + rng.normal(size=(n, 2)) * np.sqrt(sig[oc1])[:, None] * 0.7).astype(f)
    obs2 = (proj(K2, X2) + rng.normal(size=(n, 2)) * np.sqrt(sig[oc2])[:, None] * 0.7).astype(f)
    w1, w2 = inv[oc1].copy(), inv[oc2].copy()
    out = rng.random(n) < out_kf2
    invz = f(1) / X2[:, 2]
    obs2[out] = np.stack([X2[:, 0] * invz, X2[:, 1] * invz], 1)[out]
    w2[out] = inv[0]
    Rp = sm.rot_from_axis_angle(rng.normal(size=3), 0.02) @ sc["R"]
    q0 = np.array(quat_from_R(Rp.tolist(), np.float64), np.float64)
    t0 = sc["t"] + rng.normal(size=3) * 0.03
    s0 = sc["s"] * (1.0 if fix_scale else 1.02)
    if special == "z0":
        X2 = X2.copy()
        X2[0] = 0
        t0[2] = 0.0
    elif special == "nan":
        obs1[0, 0] = np.nan
    p = Problem(X1, X2, obs1, obs2, w1, w2, K1, K2, fix_scale, th2, q0, t0, s0)
    p.truth = (sc["R"], sc["t"], sc["s"])
    return p


N_BANDS = ((0, 100), (100, 500), (500, 10 ** 9))


def band_of(n, fix_scale):
    """(n band, scale mode).  n is the number of pairs the SECOND round optimises (the long double model's n_in): q / t / s come out of
    that round, and how far rounding moves them goes with the number of pairs it runs on, not with the number handed in -- a scene
    of 200 pairs of which 10 survive behaves like a scene of 10."""
    for lo, hi in N_BANDS:
        if lo <= n < hi:
            return (lo, bool(fix_scale))
    raise ValueError(n)


def family():
    """The fixed scene family of the float64-vs-long-double measurement and of the GPU comparison: (seed, n, fix_scale, outlier
    fraction, special).  n = 10 ... 2000, both scale modes, 0 / 30 / 50 % wrong matches, 15 % of the matches outside KF2; the n = 10
    scenes and some of the others return early (fewer than 10 pairs survive round 1); one z = 0 scene and one NaN scene (rule 4)."""
    out = []
    for n in (10, 16, 40, 120, 200, 300, 700):
        for fs in (True, False):
            for of in (0.0, 0.3, 0.5):
                if (n == 10 and of > 0.0) or (n <= 40 and of > 0.3):
                    continue                                  # (these all return early: the family would be mostly early returns)
                for k in range(2 if 40 <= n <= 300 else 1):
                    out.append((1000 * n + 100 * int(fs) + int(of * 10) * 10 + k, n, fs, of, None))
    for fs in (True, False):
        out.append((2000000 + int(fs), 2000, fs, 0.3, None))
        out.append((1300000 + int(fs), 1300, fs, 0.0, None))
    out.append((424242, 60, True, 0.3, "z0"))
    out.append((434343, 60, False, 0.3, "nan"))
    return out


def family_problem(entry):
    seed, n, fs, of, special = entry
    return make_problem(seed, n, fs, of, special=special)


def est_diff(a, b):
    """Largest |difference| over q / t / s of two results, in long double."""
    with np.errstate(all="ignore"):
        d = [np.abs(np.asarray(a["q"], L) - np.asarray(b["q"], L)).max(), np.abs(np.asarray(a["t"], L) - np.asarray(b["t"], L)).max(),
             abs(L(a["s"]) - L(b["s"]))]
    return float(max(d))


def near_threshold(r_ref, th2, rel=1e-3):
    """(n,) bool: one of the chi2 values a classification of r_ref read lies within a relative `rel` of th2 (a pair removed in round 1
    has no round-2 decision).  A pair in the band may be classified differently by another evaluation, and so may everything AFTER it:
    a scene with a banded round-1 decision is compared on round 1 only."""
    c = np.asarray(r_ref["edge_chi2"], L)
    t = L(np.float32(th2))
    with np.errstate(all="ignore"):
        n1 = (np.abs(c[0] - t) <= rel * t) | (np.abs(c[1] - t) <= rel * t)
        n2 = (np.abs(c[2] - t) <= rel * t) | (np.abs(c[3] - t) <= rel * t)
    n2 = n2 & (r_ref["removed"] != 1)
    return n1, n2


# ------------------------------------------------------------------ the yardstick: float64 against long double on the family

ILL_CONDITIONED = 1e-5       # q / t / s of the two precisions further apart than this: the scene is ill-conditioned (the largest
                             # difference of a well-conditioned scene is 1e-7, rounding that tips a decision moves them by 1e-2 and more)


def round_trace(r, rnd):
    """(trials per LM iteration) of one round."""
    return [int(x[3]) for x in r["trace"] if int(x[0]) == rnd]


def compare_sets(ref_ld, a, b, th2):
    """Classification of a against b, leaving out the decisions whose LONG DOUBLE chi2 (ref_ld) lies within 1e-3 (relative) of th2.
    -> dict(decisions, left_out, equal): `equal` is False when a decision outside the band differs.  When the round-1 sets differ
    (inside the band) the second round ran on different edges: all of the scene's round-2 decisions are left out."""
    n1, n2 = near_threshold(ref_ld, th2)
    r1a, r1b = a["removed"] == 1, b["removed"] == 1
    n = len(r1a)
    n_round2 = int((ref_ld["removed"] != 1).sum()) if not ref_ld["returned_early"] else 0
    out = dict(decisions=n + n_round2, left_out=int(n1.sum()), equal=True, same=bool(np.array_equal(a["removed"], b["removed"])))
    if not np.array_equal(r1a[~n1], r1b[~n1]):
        out["equal"] = False
        return out
    if not np.array_equal(r1a, r1b):
        out["left_out"] += n_round2
        return out
    if bool(a["returned_early"]) != bool(b["returned_early"]):
        out["equal"] = False
        return out
    if a["returned_early"]:
        return out
    out["left_out"] += int(n2.sum())
    r2a, r2b = a["removed"] == 2, b["removed"] == 2
    if not np.array_equal(r2a[~n2], r2b[~n2]):
        out["equal"] = False
    if out["same"] and int(a["n_in"]) != int(b["n_in"]):
        out["equal"] = False
    return out


_FAMILY = {}


def measure_family():
    """Every scene of family() in float64 and in long double.  -> dict(scenes = [dict(entry, problem, f64, ld, diff, ill, band, cmp)],
    band_max = {band: largest well-conditioned |q t s (f64) - q t s (ld)| over the scenes with a non-zero return})."""
    if not _FAMILY:
        _FAMILY.update(measure_entries(family()))
    return _FAMILY


def measure_entries(entries):
    """measure_family's measurement on any list of family() entries (the boundary family of tests/path_boundary_cases.py)."""
    scenes = []
    band_max = {}
    for e in entries:
        p = family_problem(e)
        a, b = optimize_sim3(p, np.float64), optimize_sim3(p, L)
        d = est_diff(a, b)
        rec = dict(entry=e, problem=p, f64=a, ld=b, diff=d, ill=d > ILL_CONDITIONED, band=band_of(int(b["n_in"]), e[2]),
                   cmp=compare_sets(b, a, b, p.th2))
        scenes.append(rec)
        if b["n_in"] > 0 and not rec["ill"]:
            band_max[rec["band"]] = max(band_max.get(rec["band"], 0.0), d)
    return dict(scenes=scenes, band_max=band_max)
