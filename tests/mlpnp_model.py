"""Checker for MLPnPsolver (S/MLPnPsolver.cpp): numpy, float64, with the float statements of CheckInliers in np.float32.

Two formulations of computePose for a six-point minimal set:
  (a) compute_pose(..., form="a"): np.linalg.svd for the null spaces, for the 12 x 12 (9 x 9) vector and for the nearest rotation,
      np.linalg.solve for the Gauss-Newton step -- the reference's own choice of decompositions.
  (b) compute_pose(..., form="b"): what csrc/mlpnp.hip does, restated: a cross-product null-space basis, the round-robin cyclic Jacobi
      with its sweep exit, the polar factor through np.linalg.eigh, an unpivoted LDL^T.
Both share the planar test (Eigen's FullPivHouseholderQR restated), the eigen frame with its sign rule, the sign choices, the derived
Jacobian, and the stopping rules of mlpnp_gn.  SerialSolver is the loop of :99-216 over given counts and masks.
"""
import math

import numpy as np

EPS = np.finfo(np.float64).eps
K_PINHOLE = (500.0, 500.0, 320.0, 240.0)
MAX_SWEEPS = 20
SWEEP_BOUND = 1e-30


# ---------------------------------------------------------------- SetRansacParameters, :218-248

def ransac_iterations(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=6, epsilon=0.4):
    """-> (mRansacMaxIts, mRansacMinInliers, mRansacEpsilon)."""
    eps = np.float32(epsilon)
    nmin = int(np.float32(n) * eps)
    nmin = max(nmin, min_inliers, min_set)
    with np.errstate(all="ignore"):
        q = np.float32(nmin) / np.float32(n)
        if eps < q:
            eps = q
        if nmin == n:
            its = 1
        else:
            v = np.ceil(np.log(1 - probability) / np.log(1 - np.power(np.float64(eps), 3)))
            its = int(v) if np.isfinite(v) and -2147483648.0 <= v < 2147483648.0 else -2147483648
    return max(1, min(its, max_iterations)), nmin, eps


def resolve_draws(n, draws):
    """:126-138 as the list operations they are."""
    out = np.zeros((len(draws), 6), np.int32)
    for k, d in enumerate(draws):
        avail = list(range(n))
        for j in range(6):
            r = int(d[j])
            out[k, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def draws(n, k, seed):
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    d = np.empty((int(k), 6), np.int32)
    for j in range(6):
        d[:, j] = rng.integers(0, max(int(n) - j, 1), size=int(k))
    return d


# ---------------------------------------------------------------- small pieces

def rodrigues2rot(w):
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    th = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) if np.all(np.isfinite(w)) else float("nan")
    if th > EPS:
        return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / (th * th) * (K @ K)
    return np.eye(3)                 # (also for a NaN vector: the comparison at :663 is false)


def rot2rodrigues(R):
    trace = R[0, 0] + R[1, 1] + R[2, 2] - 1.0
    with np.errstate(invalid="ignore"):
        wn = np.arccos(trace / 2.0)
    w = np.zeros(3)
    if wn > EPS:
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (wn / (2.0 * math.sin(wn)))
    return w


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def jacobian(w, t, X, nr, ns):
    """d [nr, ns]^T normalize(R(w) X + t) / d (w, t), derived: N^T (I - v v^T) / |v| [ -R [X]x J_r(w) | I ], J_r the right Jacobian of
    SO(3).  0 / 0 at w = 0, as in the reference's generated code.  -> (2, 6)."""
    with np.errstate(all="ignore"):
        th2 = np.float64((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        th = np.sqrt(th2)
        a, b = (1.0 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
        W = skew(w)
        Jr = np.eye(3) - a * W + b * (W @ W)
        R = rodrigues2rot(w)
        v = R @ X + t
        nv = np.linalg.norm(v)
        vh = v / nv
        Dm = (np.eye(3) - np.outer(vh, vh)) / nv
        N = np.stack([nr, ns])
        return np.hstack([N @ Dm @ (-R @ skew(X) @ Jr), N @ Dm])


def nullspace_svd(f):
    V = np.linalg.svd(f.reshape(1, 3), full_matrices=True)[2].T
    return V[:, 1], V[:, 2]


def nullspace_cross(f):
    e = np.zeros(3)
    a = np.abs(f)
    e[0 if (a[0] <= a[1] and a[0] <= a[2]) else (1 if a[1] <= a[2] else 2)] = 1.0
    r = np.cross(f, e)
    r = r / np.linalg.norm(r)
    s = np.cross(f, r)
    return r, s / np.linalg.norm(s)


def fullpiv_rank3(M):
    """Eigen::FullPivHouseholderQR<Matrix3d>(M).rank() with the default threshold."""
    q = np.array(M, np.float64)
    prec = EPS * 3.0
    biggest = maxpivot = 0.0
    piv = []
    for k in range(3):
        blk = np.abs(q[k:, k:])
        big, br, bc = -1.0, k, k
        for j in range(blk.shape[1]):
            for i in range(blk.shape[0]):
                if blk[i, j] > big:
                    big, br, bc = blk[i, j], k + i, k + j
        if k == 0:
            biggest = big
        if big <= biggest * prec:
            break
        q[[k, br], :] = q[[br, k], :]
        q[:, [k, bc]] = q[:, [bc, k]]
        tail2 = float(np.sum(q[k + 1:, k] ** 2))
        c0 = q[k, k]
        ess = np.zeros(3)
        if tail2 <= np.finfo(np.float64).tiny:
            tau, beta = 0.0, c0
        else:
            beta = math.sqrt(c0 * c0 + tail2)
            if c0 >= 0:
                beta = -beta
            ess[k + 1:] = q[k + 1:, k] / (c0 - beta)
            tau = (beta - c0) / beta
        q[k, k] = beta
        piv.append(abs(beta))
        maxpivot = max(maxpivot, abs(beta))
        for j in range(k + 1, 3):
            wv = q[k, j] + float(ess[k + 1:] @ q[k + 1:, j])
            q[k, j] -= tau * wv
            q[k + 1:, j] -= tau * wv * ess[k + 1:]
    return sum(1 for p in piv if p > maxpivot * prec)


def eigen_frame(M):
    """eigenvectors^T of the symmetric M, ascending eigenvalues, each eigenvector signed so that its largest component is positive."""
    _, w = np.linalg.eigh(M)
    out = np.zeros((3, 3))
    for j in range(3):
        a = np.abs(w[:, j])
        lead = w[0, j] if (a[0] >= a[1] and a[0] >= a[2]) else (w[1, j] if a[1] >= a[2] else w[2, j])
        out[j] = (-1.0 if lead < 0 else 1.0) * w[:, j]
    return out


def design(P, N, planar):
    A = np.zeros((12, 9 if planar else 12))
    for i in range(6):
        for k in range(2):
            nv, p = N[i][k], P[i]
            if planar:
                A[2 * i + k] = [nv[0] * p[1], nv[0] * p[2], nv[1] * p[1], nv[1] * p[2], nv[2] * p[1], nv[2] * p[2], nv[0], nv[1], nv[2]]
            else:
                A[2 * i + k] = [nv[c // 3] * p[c % 3] for c in range(9)] + [nv[0], nv[1], nv[2]]
    return A


def jacobi_smallest(S):
    """The kernel's Jacobi: round-robin order, the six disjoint rotations of a step at once, sweep exit on off^2 <= 1e-30 diag^2.
    -> (eigenvector of the smallest eigenvalue, the first on a tie; sweeps run)."""
    m = S.shape[0]
    A = np.zeros((12, 12))
    A[:m, :m] = S
    V = np.eye(12)
    sweeps = 0
    with np.errstate(all="ignore"):
        for _ in range(MAX_SWEEPS):
            d = np.diag(A)
            off2 = float(np.sum(np.triu(A, 1) ** 2))
            if not off2 > SWEEP_BOUND * float(np.sum(d * d)):
                break
            sweeps += 1
            for step in range(11):
                J = np.eye(12)
                for k in range(6):
                    i0, i1 = (11, step) if k == 0 else ((step + k) % 11, (step + 11 - k) % 11)
                    p, q = min(i0, i1), max(i0, i1)
                    apq = A[p, q]
                    if apq == 0.0:
                        continue
                    theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                    t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0)) if np.isfinite(theta) else 0.0
                    if theta < 0:
                        t = -t
                    c = 1.0 / math.sqrt(t * t + 1.0)
                    s = t * c
                    J[p, p], J[q, p], J[p, q], J[q, q] = c, -s, s, c
                A = J.T @ A @ J
                A = np.triu(A) + np.triu(A, 1).T
                V = V @ J
    lam = np.diag(A)[:m]
    return V[:, int(np.argmin(lam))][:m], sweeps


def polar_eigh(M):
    with np.errstate(all="ignore"):
        lam, W = np.linalg.eigh(M.T @ M)
        return M @ (W @ np.diag(1.0 / np.sqrt(lam)) @ W.T)


def polar_svd(M):
    U, _, Vt = np.linalg.svd(M)
    return U @ Vt


def ldlt_solve(A, g):
    n = len(g)
    L = np.array(A, np.float64)
    with np.errstate(all="ignore"):
        for j in range(n):
            dj = L[j, j] - sum(L[j, k] * L[j, k] * L[k, k] for k in range(j))
            L[j, j] = dj
            for i in range(j + 1, n):
                L[i, j] = (L[i, j] - sum(L[i, k] * L[j, k] * L[k, k] for k in range(j))) / dj
        x = np.array(g, np.float64)
        for i in range(n):
            x[i] -= sum(L[i, k] * x[k] for k in range(i))
        for i in range(n):
            x[i] /= L[i, i]
        for i in range(n - 1, -1, -1):
            x[i] -= sum(L[k, i] * x[k] for k in range(i + 1, n))
    return x


def gauss_newton(w, t, P, N, form):
    """mlpnp_gn, :687-752.  -> (w, t)."""
    w, t = np.array(w, np.float64), np.array(t, np.float64)
    cond = 1.0
    with np.errstate(all="ignore"):
        for _ in range(5):
            R = rodrigues2rot(w)
            J = np.zeros((12, 6))
            r = np.zeros(12)
            for i in range(6):
                v = R @ P[i] + t
                vh = v / np.linalg.norm(v)
                r[2 * i], r[2 * i + 1] = N[i][0] @ vh, N[i][1] @ vh
                J[2 * i: 2 * i + 2] = jacobian(w, t, P[i], N[i][0], N[i][1])
            A, g = J.T @ J, J.T @ r
            cond = float(np.linalg.cond(A)) if np.all(np.isfinite(A)) else float("inf")
            if form == "a":
                try:
                    dx = np.linalg.solve(A, g) if np.all(np.isfinite(A)) and np.all(np.isfinite(g)) else np.full(6, np.nan)
                except np.linalg.LinAlgError:
                    dx = np.full(6, np.nan)
            else:
                dx = ldlt_solve(A, g)
            ad = np.abs(dx)
            if bool(np.any(ad > 5.0)) or bool(np.all(ad > 1.0)):
                break
            small = bool(np.all(np.abs(J @ dx) < 1e-5))
            w, t = w - dx[:3], t - dx[3:]
            if small:
                break
    return w, t, cond


def refine_stage(Rout, tout, P, f, form="b"):
    """:635-647 for a six-point set with the null spaces of `form`."""
    N = [(nullspace_svd if form == "a" else nullspace_cross)(np.asarray(f[i], np.float64)) for i in range(6)]
    w, t, _ = gauss_newton(rot2rodrigues(np.asarray(Rout, np.float64)), tout, np.asarray(P, np.float64), N, form)
    return rodrigues2rot(w), t


def compute_pose(P, f, form):
    """computePose (:345-651) for six points P (6, 3) with bearings f (6, 3), float64.  -> dict(R, t, planar, gap, sweeps, cond);
    cond: the condition number of the last Gauss-Newton normal matrix."""
    P, f = np.asarray(P, np.float64), np.asarray(f, np.float64)
    N = [(nullspace_svd if form == "a" else nullspace_cross)(f[i]) for i in range(6)]
    M = sum(np.outer(p, p) for p in P)
    planar = fullpiv_rank3(M) == 2
    eigenRot = eigen_frame(M) if planar else np.eye(3)
    Q = P @ eigenRot.T
    A = design(Q if planar else P, N, planar)
    S = A.T @ A
    lam = np.linalg.eigvalsh(S)
    gap = float((lam[1] - lam[0]) / lam[-1]) if lam[-1] > 0 else 0.0
    sweeps = 0
    with np.errstate(all="ignore"):
        if form == "a":
            x = np.linalg.svd(S)[2][-1]
        else:
            x, sweeps = jacobi_smallest(S)
        polar = polar_svd if form == "a" else polar_eigh
        if planar:
            tmp0 = np.array([[0.0, x[0], x[1]], [0.0, x[2], x[3]], [0.0, x[4], x[5]]])
            tmp0[:, 0] = np.cross(tmp0[:, 1], tmp0[:, 2])
            tmp = tmp0.T
            scale = 1.0 / math.sqrt(abs(np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])))
            try:
                R1 = polar(tmp)
            except np.linalg.LinAlgError:
                R1 = np.full((3, 3), np.nan)
            if np.linalg.det(R1) < 0:
                R1 = -R1
            R1 = eigenRot.T @ R1
            t = scale * x[6:9]
            Ra = -R1.T
            if np.linalg.det(Ra) < 0:
                Ra[:, 2] *= -1
            Rb = Ra * np.array([-1.0, -1.0, 1.0])
            Ts = [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]
            norms = []
            for Rc, tc in Ts:
                s = 0.0
                for p in range(6):
                    v = Rc @ P[p] + tc
                    s += 1.0 - (v / np.linalg.norm(v)) @ f[p]
                norms.append(s)
            best = 0
            for c in range(1, 4):
                if norms[c] < norms[best]:
                    best = c
            Rout, tout = Ts[best]
        else:
            tmp = x[:9].reshape(3, 3).T
            scale = 1.0 / np.power(abs(np.linalg.norm(tmp[:, 0]) * np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])), 1.0 / 3.0)
            try:
                R = polar(tmp)
            except np.linalg.LinAlgError:
                R = np.full((3, 3), np.nan)
            if np.linalg.det(R) < 0:
                R = -R
            t1 = R @ (scale * x[9:12])
            ti = -(R.T @ t1)
            err = []
            for sg in (1.0, -1.0):
                s = 0.0
                for p in range(6):
                    v = R.T @ P[p] + sg * ti
                    s += 1.0 - (v / np.linalg.norm(v)) @ f[p]
                err.append(s)
            tout = ti if err[0] < err[1] else -ti
            Rout = R.T
        w, t, cond = gauss_newton(rot2rodrigues(Rout), tout, P, N, form)
        R = rodrigues2rot(w)
        if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
            R, t = np.full((3, 3), np.nan), np.full(3, np.nan)
    return dict(R=R, t=t, planar=planar, gap=gap, sweeps=sweeps, cond=cond)


# ---------------------------------------------------------------- CheckInliers, :255-286

def check_inliers(R, t, P3Dw, P2D, max_err, K=K_PINHOLE):
    """-> (mask, error2 float32).  R, t float64; everything else float32, evaluated as the reference's statements are."""
    X = np.asarray(P3Dw, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        c = [(((R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1]) + R[i, 2] * X[:, 2]) + t[i]).astype(np.float32) for i in range(3)]
        fx, fy, cx, cy = (np.float32(v) for v in K)
        u = fx * c[0] / c[2] + cx
        v = fy * c[1] / c[2] + cy
        P2D = np.asarray(P2D, np.float32)
        dX, dY = P2D[:, 0] - u, P2D[:, 1] - v
        e2 = dX * dX + dY * dY
        return e2 < np.asarray(max_err, np.float32), e2


def max_errors(sigma2, th2):
    return np.asarray(sigma2, np.float32) * np.float32(th2)


def pose_to_Tcw(R, t):
    T = np.eye(4, dtype=np.float32)
    with np.errstate(all="ignore"):
        T[:3, :3] = np.asarray(R, np.float64).astype(np.float32)
        T[:3, 3] = np.asarray(t, np.float64).astype(np.float32)
    return T


# ---------------------------------------------------------------- the serial loop, :99-216

class SerialSolver:
    """MLPnPsolver::iterate over given per-hypothesis counts, masks (n bools each) and poses, with Refine() as it behaves: it returns
    the current hypothesis, exactly when its count exceeds min_inliers."""

    def __init__(self, n, m, kp_index, min_inliers, max_its):
        self.n, self.m, self.kp = n, m, np.asarray(kp_index, np.int64)
        self.min_inliers, self.max_its = min_inliers, max_its
        self.iterations, self.best_inliers, self.best_iteration = 0, 0, -1
        self.best_mask, self.best_Tcw = np.zeros(n, bool), None

    def iterations_of_call(self, n_iterations):
        return 0 if self.n < self.min_inliers else max(n_iterations, self.max_its - self.iterations)

    def iterate(self, n_iterations, counts, masks, poses):
        """counts / masks / poses of the iterations_of_call(n_iterations) hypotheses this call can run.  -> dict of every output."""
        out = dict(no_more=False, returned=False, n_inliers=0, iterations_run=0, Tcw=None, inliers=np.zeros(self.m, bool))
        if self.n < self.min_inliers:
            out["no_more"] = True
            return self._finish(out)
        cur = 0
        while self.iterations < self.max_its or cur < n_iterations:
            c = int(counts[cur])
            cur += 1
            self.iterations += 1
            if c >= self.min_inliers:
                if c > self.best_inliers:
                    self.best_inliers, self.best_iteration = c, self.iterations - 1
                    self.best_mask = np.array(masks[cur - 1], bool)
                    self.best_Tcw = pose_to_Tcw(*poses[cur - 1])
                if c > self.min_inliers:
                    out.update(returned=True, n_inliers=c, Tcw=pose_to_Tcw(*poses[cur - 1]), iterations_run=cur)
                    out["inliers"][self.kp[np.array(masks[cur - 1], bool)]] = True
                    return self._finish(out)
        out["iterations_run"] = cur
        if self.iterations >= self.max_its:
            out["no_more"] = True
            if self.best_inliers >= self.min_inliers:
                out.update(returned=True, n_inliers=self.best_inliers, Tcw=self.best_Tcw.copy())
                out["inliers"][self.kp[self.best_mask]] = True
        return self._finish(out)

    def _finish(self, out):
        out.update(iterations_done=self.iterations, have_best=self.best_Tcw is not None, best_inliers=self.best_inliers,
                   best_iteration=self.best_iteration, best_Tcw=None if self.best_Tcw is None else self.best_Tcw.copy())
        return out

    @staticmethod
    def fields(out):
        """The same tuple as api.MLPnPIteration.fields()."""
        return (out["no_more"], out["returned"], out["n_inliers"], out["iterations_done"], out["iterations_run"], out["best_iteration"],
                out["have_best"], out["best_inliers"], None if out["Tcw"] is None else out["Tcw"].tobytes(),
                None if out["best_Tcw"] is None else out["best_Tcw"].tobytes(), out["inliers"].tobytes())


# ---------------------------------------------------------------- scenes

def random_rotation(rng, min_angle=0.05, max_angle=0.6):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    return rodrigues2rot(ax * rng.uniform(min_angle, max_angle))


def make_scene(seed, n, outlier_fraction, planar=False, plane=None):
    """A 640 x 480 pinhole, points 2-8 m in front of the camera rounded to float32, 0.5 px noise, a rotation at least 0.05 rad from the
    identity.  planar: the points lie on the world plane z = 0; plane = (normal, offset): on that plane instead.
    -> dict(P2D, sigma2, bearing, P3Dw, K, R, t, kp_index, m)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K_PINHOLE
    R = random_rotation(rng)
    uv = np.stack([rng.uniform(20, 620, n), rng.uniform(20, 460, n)], 1)
    depth = rng.uniform(2.0, 8.0, n)
    rays = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(n)], 1)
    if planar or plane is not None:
        # points on the world plane z = 0 (exactly: rank 2), or on that plane tilted by `plane[0]` (a rotation vector) and lifted by
        # plane[1] along z; the camera 2 m above the origin looks down.
        # (Close on purpose: the planar branch takes its scale from the ROWS of the transposed matrix (:535-537), which mixes s and s^2
        # of the unit solution vector's scale s = 1 / sqrt(2 + |t|^2); far from the plane the translation comes out several metres off,
        # the first Gauss-Newton step exceeds 5 and is refused (:738) -- reproduced, but such a scene tests nothing else.)
        Xw = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), np.zeros(n)], 1)
        if plane is not None:
            Xw = Xw @ rodrigues2rot(np.asarray(plane[0], np.float64)).T + np.array([0.0, 0.0, float(plane[1])])
        R = R @ np.diag([1.0, -1.0, -1.0])
        t = -R @ np.array([0.3, -0.2, 2.0])
    else:
        t = rng.uniform(-0.5, 0.5, 3)
        Xc = rays * depth[:, None]
        Xw = (Xc - t) @ R                                            # R^T (Xc - t)
    Xw = Xw.astype(np.float32)
    Xc = Xw.astype(np.float64) @ R.T + t
    uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1) + rng.normal(0, 0.5, (n, 2))
    n_out = int(round(outlier_fraction * n))
    if n_out:
        bad = rng.choice(n, n_out, replace=False)
        uv[bad] = np.stack([rng.uniform(0, 640, n_out), rng.uniform(0, 480, n_out)], 1)
    P2D = uv.astype(np.float32)
    octave = rng.integers(0, 4, n)
    sigma2 = (np.float32(1.2) ** octave.astype(np.float32)) ** 2
    sigma2 = sigma2.astype(np.float32)
    # Pinhole::unproject in float, divided by its z (which is 1)
    bearing = np.stack([(P2D[:, 0] - np.float32(cx)) / np.float32(fx), (P2D[:, 1] - np.float32(cy)) / np.float32(fy), np.ones(n, np.float32)], 1).astype(np.float32)
    m = n + n // 3 + 1
    kp_index = np.sort(rng.choice(m, n, replace=False)).astype(np.int32)
    return dict(P2D=P2D, sigma2=sigma2, bearing=bearing, P3Dw=Xw, K=K_PINHOLE, R=R, t=t, kp_index=kp_index, m=m)


def hypotheses(scene, drw, th2=5.991, form="b"):
    """Every hypothesis of `drw` (k, 6) on the scene.  -> list of dict(R, t, planar, gap, mask, e2, count)."""
    n = len(scene["P2D"])
    idx = resolve_draws(n, drw)
    me = max_errors(scene["sigma2"], th2)
    out = []
    for k in range(len(drw)):
        hyp = compute_pose(scene["P3Dw"][idx[k]], scene["bearing"][idx[k]], form)
        mask, e2 = check_inliers(hyp["R"], hyp["t"], scene["P3Dw"], scene["P2D"], me, scene["K"])
        hyp.update(mask=mask, e2=e2, count=int(mask.sum()))
        out.append(hyp)
    return out


# (n, outlier fraction, H) of the GPU test's hypothesis cases; the CPU test holds both caps for the model alone on these seeds
CASES = [(6, 0.0, 1), (7, 0.15, 35), (63, 0.3, 64), (64, 0.3, 65), (65, 0.3, 63), (513, 0.5, 300), (2000, 0.3, 35)]
GAP_BANDS = [(1e-8, 1e-6), (1e-6, 1e-4), (1e-4, 1e-2), (1e-2, 1.1)]


PLANAR_CASES = [dict(planar=True), dict(plane=((0.4, -0.3, 0.0), 1.5))]      # the world plane z = 0; a tilted plane off the origin


def case_scene(i):
    """Scene and raw draws of CASES[i]; i = len(CASES), len(CASES) + 1: the two planar scenes (n = 40, H = 35)."""
    if i >= len(CASES):
        j = i - len(CASES)
        return make_scene(1100 + j, 40, 0.2, **PLANAR_CASES[j]), draws(40, 35, 2100)
    n, frac, H = CASES[i]
    sc = make_scene(1000 + i, n, frac)
    return sc, draws(n, H, 2000 + i)


def band_of(gap):
    for b, (lo, hi) in enumerate(GAP_BANDS):
        if lo <= gap < hi:
            return b
    return -1


_MEASURED = {}


def measure():
    """Formulation (a) against (b) over every hypothesis of CASES and of the planar scene z = 0, computed once per process.
    -> dict(a=[per case list of hypotheses], b=..., bands={band index: largest pose difference}, conds={band index: largest condition
    number of a Gauss-Newton normal matrix}, low_gap, nan, total, near, decisions)."""
    if _MEASURED:
        return _MEASURED
    A, B, bands, conds = [], [], {}, {}
    low_gap = nan = total = near = decisions = 0
    for i in range(len(CASES) + 1):          # (the tilted plane is degenerate for the general branch by construction: not measured)
        sc, d = case_scene(i)
        ha, hb = hypotheses(sc, d, form="a"), hypotheses(sc, d, form="b")
        me = max_errors(sc["sigma2"], 5.991)
        for x, y in zip(ha, hb):
            total += 1
            if not np.all(np.isfinite(y["R"])) or not np.all(np.isfinite(x["R"])):
                nan += 1
                continue
            b = band_of(y["gap"])
            if b < 0:
                low_gap += 1
                continue
            bands[b] = max(bands.get(b, 0.0), pose_difference(x, y))
            conds[b] = max(conds.get(b, 0.0), y["cond"])
            near += int(near_threshold(y["e2"], me).sum())
            decisions += len(me)
        A.append(ha)
        B.append(hb)
    _MEASURED.update(a=A, b=B, bands=bands, conds=conds, low_gap=low_gap, nan=nan, total=total, near=near, decisions=decisions)
    return _MEASURED


def yardstick(band):
    """What a third implementation of computePose may differ by in a gap band, before the margin: the larger of the (a)-vs-(b) difference
    measured in the band and FP64 rounding carried through the worst-conditioned six-point normal matrix of the band (a step of
    Gauss-Newton is (J^T J)^-1 J^T r: a relative rounding error eps in r or J moves the O(1) pose by up to eps * cond).  The second
    term matters where the band holds few hypotheses and (a) and (b) happen to agree to the last digits."""
    ms = measure()
    return max(ms["bands"][band], EPS * ms["conds"][band])


def near_threshold(e2, max_err, rel=1e-4):
    """Decisions whose model error2 lies within a relative `rel` of its threshold."""
    e2, me = np.asarray(e2, np.float64), np.asarray(max_err, np.float64)
    with np.errstate(invalid="ignore"):
        return np.abs(e2 - me) <= rel * me


def pose_difference(h1, h2):
    """Largest absolute difference over R and t; 0 when both are NaN, inf when one is."""
    n1, n2 = not np.all(np.isfinite(h1["R"])), not np.all(np.isfinite(h2["R"]))
    if n1 or n2:
        return 0.0 if (n1 and n2) else float("inf")
    return float(max(np.abs(h1["R"] - h2["R"]).max(), np.abs(h1["t"] - h2["t"]).max()))
