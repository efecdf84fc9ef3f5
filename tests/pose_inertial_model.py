"""numpy model of Optimizer::PoseInertialOptimizationLastKeyFrame / ...LastFrame (S/Optimizer.cc:7603-8424), restated from the
reference's text, the yardstick of pose_inertial_optimize (include/orbgpu.h).

Two variants of the same solve:
  "reference": float round trips where the reference has them -- ExpSO3 through a float32 SVD (S/G2oTypes.cc:1000,1005), the float
               GetDeltaRotation / Velocity / Position (S/ImuTypes.cc:410-431), the float state written back to the Frame;
  "kernel":    double throughout, which is what the device kernel computes.
Both share the stated deviation of the entry point: a factorisation whose pivot is not positive -- or no larger than 2^-40 of its own
diagonal entry, the rounding noise of a singular system, whose sign is arbitrary -- ends the round's iterations without an update (the
reference applies an undefined x first).  Also shared: the camera pose of the first linearisation is computed from Rwb, twb (the reference
copies the Frame's float mTcw), and tbc is -Rbc tcb (the reference reads Tbc).

Unknown layout: [other end: rotation 3, translation 3, velocity 3, gyro bias 3, accelerometer bias 3 | the frame: the same], the 30 x 30
of S/Optimizer.cc:8367-8415; the LastKeyFrame form has the frame's 15 only.
"""
import numpy as np

GRAVITY = float(np.float32(9.81))                     # IMU::GRAVITY_VALUE, a float (I/ImuTypes.h:25)
G_VEC = np.array([0.0, 0.0, -GRAVITY])
FORM_KF, FORM_FRAME = 0, 1
CHI2_MONO = {FORM_KF: (12.0, 7.5, 5.991, 5.991), FORM_FRAME: (5.991, 5.991, 5.991, 5.991)}
CHI2_STEREO = (15.6, 9.8, 7.815, 7.815)
PIVOT_REL = 2.0 ** -40                                # a pivot this small against its diagonal entry is rounding noise: not positive
f32 = np.float32


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def normalize_rotation(R, dtype=np.float64):
    """IMU::NormalizeRotation (S/ImuTypes.cc:30-36): U Vt of the SVD, in `dtype`."""
    U, _, Vt = np.linalg.svd(np.asarray(R, dtype))
    return (U @ Vt).astype(np.float64)


def exp_so3(w, variant="kernel"):
    """ExpSO3 (S/G2oTypes.cc:991-1007); "reference": its result goes through a float cv::Mat and NormalizeRotation."""
    w = np.asarray(w, np.float64)
    d2 = float(w @ w)
    d = np.sqrt(d2)
    W = skew(w)
    if d < 1e-5:
        R = np.eye(3) + W + 0.5 * (W @ W)
    else:
        R = np.eye(3) + W * (np.sin(d) / d) + (W @ W) * ((1.0 - np.cos(d)) / d2)
    if variant == "reference":
        return normalize_rotation(R.astype(f32), f32)
    return R


def exp_so3_imu_float(w):
    """IMU::ExpSO3(const cv::Mat&) (S/ImuTypes.cc:48-60): float arithmetic, eps = 1e-4."""
    x, y, z = [f32(c) for c in w]
    d2 = f32(x * x + y * y + z * z)
    d = f32(np.sqrt(d2))
    W = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], f32)
    I = np.eye(3, dtype=f32)
    if d < f32(1e-4):
        return (I + W + f32(0.5) * (W @ W)).astype(f32)
    return (I + W * f32(np.sin(np.float64(d))) / d + (W @ W) * f32(f32(1.0) - f32(np.cos(np.float64(d)))) / d2).astype(f32)


def log_so3(R):
    """LogSO3 (S/G2oTypes.cc:1009-1023)."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    w = np.array([(R[2, 1] - R[1, 2]) / 2, (R[0, 2] - R[2, 0]) / 2, (R[1, 0] - R[0, 1]) / 2])
    c = (tr - 1.0) * 0.5
    if c > 1 or c < -1:
        return w
    th = np.arccos(c)
    s = np.sin(th)
    if abs(s) < 1e-5:
        return w
    return th * w / s


def right_jacobian_so3(v):
    d2 = float(v @ v)
    d = np.sqrt(d2)
    W = skew(v)
    if d < 1e-5:
        return np.eye(3)
    return np.eye(3) - W * ((1.0 - np.cos(d)) / d2) + (W @ W) * ((d - np.sin(d)) / (d2 * d))


def inv_right_jacobian_so3(v):
    d2 = float(v @ v)
    d = np.sqrt(d2)
    W = skew(v)
    if d < 1e-5:
        return np.eye(3)
    return np.eye(3) + W / 2 + (W @ W) * (1.0 / d2 - (1.0 + np.cos(d)) / (2.0 * d * np.sin(d)))


# ------------------------------------------------------------------------------------------------ vertices
def make_state(Rwb, twb, vwb, bg, ba):
    return {"R": np.array(Rwb, np.float64).reshape(3, 3), "t": np.array(twb, np.float64).reshape(3),
            "v": np.array(vwb, np.float64).reshape(3), "bg": np.array(bg, np.float64).reshape(3),
            "ba": np.array(ba, np.float64).reshape(3)}


def oplus(s, dx, variant="kernel"):
    """ImuCamPose::Update (S/G2oTypes.cc:192-220) on the pose, plain additions on velocity and biases; dx = 15 values in the layout above."""
    return {"R": s["R"] @ exp_so3(dx[0:3], variant), "t": s["t"] + s["R"] @ dx[3:6], "v": s["v"] + dx[6:9], "bg": s["bg"] + dx[9:12],
            "ba": s["ba"] + dx[12:15]}


def camera_pose(s, Tcb):
    """Rcw = Rcb Rwb^T, tcw = Rcb (-Rwb^T twb) + tcb (S/G2oTypes.cc:211-218)."""
    Rcb, tcb = Tcb[:, :3], Tcb[:, 3]
    Rbw = s["R"].T
    return Rcb @ Rbw, Rcb @ (-(Rbw @ s["t"])) + tcb


# ------------------------------------------------------------------------------------------------ edges
def visual_error(Rcw, tcw, cam, Xw, u, v, ur, reverse=False):
    """EdgeMonoOnlyPose / EdgeStereoOnlyPose::computeError for arrays of correspondences: err (n, 3) (third 0 for mono), Xc (n, 3).
    reverse: the four terms of every camera-frame coordinate are added from the last to the first."""
    fx, fy, cx, cy, bf = cam
    if reverse:
        Xc = ((tcw + Xw[:, 2:3] * Rcw[:, 2]) + Xw[:, 1:2] * Rcw[:, 1]) + Xw[:, 0:1] * Rcw[:, 0]
    else:
        Xc = ((Xw[:, 0:1] * Rcw[:, 0] + Xw[:, 1:2] * Rcw[:, 1]) + Xw[:, 2:3] * Rcw[:, 2]) + tcw
    with np.errstate(divide="ignore", invalid="ignore"):
        pu = fx * Xc[:, 0] / Xc[:, 2] + cx
        pv = fy * Xc[:, 1] / Xc[:, 2] + cy
        pr = pu - bf * (1.0 / Xc[:, 2])
    mono = ur < 0
    err = np.stack([u - pu, v - pv, np.where(mono, 0.0, ur - pr)], axis=1)
    return err, Xc


def visual_jacobian(Xc, cam, Tcb, mono):
    """linearizeOplus of both edges (S/G2oTypes.cc:375-395, 484-508): (n, 3, 6), third row 0 for mono."""
    fx, fy, _, _, bf = cam
    Rcb, tcb = Tcb[:, :3], Tcb[:, 3]
    Rbc = Rcb.T
    tbc = -(Rbc @ tcb)
    n = len(Xc)
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    pj = np.zeros((n, 3, 3))
    pj[:, 0, 0] = fx / z
    pj[:, 0, 2] = -fx * x / (z * z)
    pj[:, 1, 1] = fy / z
    pj[:, 1, 2] = -fy * y / (z * z)
    pj[:, 2, :] = pj[:, 0, :]
    pj[:, 2, 2] += bf * (1.0 / (z * z))
    pj[mono, 2, :] = 0.0
    Xb = Xc @ Rbc.T + tbc
    M = pj @ Rcb
    S = np.zeros((n, 3, 6))
    S[:, 0, 1] = Xb[:, 2]; S[:, 0, 2] = -Xb[:, 1]
    S[:, 1, 0] = -Xb[:, 2]; S[:, 1, 2] = Xb[:, 0]
    S[:, 2, 0] = Xb[:, 1]; S[:, 2, 1] = -Xb[:, 0]
    S[:, 0, 3] = S[:, 1, 4] = S[:, 2, 5] = 1.0
    return M @ S


def preint_deltas(pre, bg, ba, variant="kernel"):
    """GetDeltaRotation / Velocity / Position (S/ImuTypes.cc:410-431) at the bias (bg, ba)."""
    if variant == "reference":
        dbg = (bg.astype(f32) - pre["bg"].astype(f32)).astype(f32)      # b_.bwx - b.bwx on float members
        dba = (ba.astype(f32) - pre["ba"].astype(f32)).astype(f32)
        dR = normalize_rotation((pre["dR"].astype(f32) @ exp_so3_imu_float(pre["JRg"].astype(f32) @ dbg)).astype(f32), f32)
        dV = (pre["dV"].astype(f32) + pre["JVg"].astype(f32) @ dbg + pre["JVa"].astype(f32) @ dba).astype(f32)
        dP = (pre["dP"].astype(f32) + pre["JPg"].astype(f32) @ dbg + pre["JPa"].astype(f32) @ dba).astype(f32)
        return dR.astype(np.float64), dV.astype(np.float64), dP.astype(np.float64)
    dbg = bg - pre["bg"].astype(np.float64)
    dba = ba - pre["ba"].astype(np.float64)
    D = lambda k: pre[k].astype(np.float64)
    dR = normalize_rotation(D("dR") @ exp_so3(D("JRg") @ dbg))
    return dR, D("dV") + D("JVg") @ dbg + D("JVa") @ dba, D("dP") + D("JPg") @ dbg + D("JPa") @ dba


def inertial_error(s1, s2, pre, variant="kernel", reverse=False):
    """EdgeInertial::computeError (S/G2oTypes.cc:720-740).  reverse: the sums inside the velocity and position residuals run from their
    last term to their first, the rotation product is associated from the right."""
    dt = float(pre["dT"])
    dR, dV, dP = preint_deltas(pre, s1["bg"], s1["ba"], variant)
    R1t = s1["R"].T
    if reverse:
        er = log_so3(dR.T @ (R1t @ s2["R"]))
        ev = -dV + R1t[:, ::-1] @ ((-(G_VEC * dt) - s1["v"]) + s2["v"])[::-1]
        ep = -dP + R1t[:, ::-1] @ (((-(G_VEC * dt * dt / 2) - s1["v"] * dt) - s1["t"]) + s2["t"])[::-1]
        return np.concatenate([er, ev, ep])
    er = log_so3(dR.T @ R1t @ s2["R"])
    ev = R1t @ (s2["v"] - s1["v"] - G_VEC * dt) - dV
    ep = R1t @ (s2["t"] - s1["t"] - s1["v"] * dt - G_VEC * dt * dt / 2) - dP
    return np.concatenate([er, ev, ep])


def inertial_jacobian(s1, s2, pre, variant="kernel"):
    """EdgeInertial::linearizeOplus (S/G2oTypes.cc:742-800): 9 x 24 = [pose1 6, v1 3, bg1 3, ba1 3 | pose2 6, v2 3]."""
    dt = float(pre["dT"])
    D = lambda k: pre[k].astype(np.float64)
    dbg = s1["bg"] - D("bg")
    if variant == "reference":
        dbg = (s1["bg"].astype(f32) - pre["bg"].astype(f32)).astype(np.float64)
    R1, R2 = s1["R"], s2["R"]
    R1t = R1.T
    dR, _, _ = preint_deltas(pre, s1["bg"], s1["ba"], variant)
    eR = dR.T @ R1t @ R2
    er = log_so3(eR)
    invJr = inv_right_jacobian_so3(er)
    J = np.zeros((9, 24))
    J[0:3, 0:3] = -invJr @ R2.T @ R1
    J[3:6, 0:3] = skew(R1t @ (s2["v"] - s1["v"] - G_VEC * dt))
    J[6:9, 0:3] = skew(R1t @ (s2["t"] - s1["t"] - s1["v"] * dt - 0.5 * G_VEC * dt * dt))
    J[6:9, 3:6] = -np.eye(3)
    J[3:6, 6:9] = -R1t
    J[6:9, 6:9] = -R1t * dt
    J[0:3, 9:12] = -invJr @ eR.T @ right_jacobian_so3(D("JRg") @ dbg) @ D("JRg")
    J[3:6, 9:12] = -D("JVg")
    J[6:9, 9:12] = -D("JPg")
    J[3:6, 12:15] = -D("JVa")
    J[6:9, 12:15] = -D("JPa")
    J[0:3, 15:18] = invJr
    J[6:9, 18:21] = R1t @ R2
    J[3:6, 21:24] = R1t
    return J


def prior_error(s, prior):
    """EdgePriorPoseImu::computeError (S/G2oTypes.cc:940-954)."""
    Rt = prior["R"].T
    return np.concatenate([log_so3(Rt @ s["R"]), Rt @ (s["t"] - prior["t"]), s["v"] - prior["v"], s["bg"] - prior["bg"], s["ba"] - prior["ba"]])


def prior_jacobian(s, prior):
    """EdgePriorPoseImu::linearizeOplus (S/G2oTypes.cc:956-969): 15 x 15."""
    Rt = prior["R"].T
    J = np.zeros((15, 15))
    J[0:3, 0:3] = inv_right_jacobian_so3(log_so3(Rt @ s["R"]))
    J[3:6, 3:6] = Rt @ s["R"]
    J[6:15, 6:15] = np.eye(9)
    return J


def huber(e2, delta):
    """RobustKernelHuber::robustify (G/core/robust_kernel_impl.cpp): rho0, rho1."""
    dsqr = delta * delta
    if e2 <= dsqr:
        return e2, 1.0
    sq = np.sqrt(e2)
    return 2 * sq * delta - dsqr, delta / sq


def ldlt_solve(H, b):
    """LDL^T without pivoting in the order of the device's lane solve; None unless every pivot is positive (beyond rounding) and finite."""
    n = len(b)
    A = H.copy()
    diag0 = np.abs(np.diag(H)).copy()
    d = np.zeros(n)
    for k in range(n):
        dk = A[k, k]
        if not (dk > PIVOT_REL * diag0[k]) or not np.isfinite(dk):
            return None
        d[k] = dk
        L = A[:, k] / dk
        for j in range(k + 1, n):
            A[j:, j] -= (L[j:] * L[j]) * dk
        A[:, k] = L
    L = np.tril(A, -1) + np.eye(n)
    y = np.zeros(n)
    for i in range(n):
        y[i] = b[i] - L[i, :i] @ y[:i]
    y /= d
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = y[i] - L[i + 1:, i] @ x[i + 1:]
    return x


def _seq_sum(a, reverse):
    """sum over axis 0 in index order (or the reverse), one addition after another"""
    if len(a) == 0:
        return np.zeros(a.shape[1:])
    return np.cumsum(a[::-1] if reverse else a, axis=0)[-1]


def marginalize(H, start, end):
    """Optimizer::Marginalize (S/Optimizer.cc:5228-5308); also returns the singular values of the marginalised block."""
    n = H.shape[0]
    b = list(range(start, end + 1))
    keep = [i for i in range(n) if i not in b]
    Hbb = H[np.ix_(b, b)]
    U, s, Vt = np.linalg.svd(Hbb)
    sinv = np.where(s > 1e-6, 1.0 / np.where(s > 1e-6, s, 1.0), 0.0)
    inv = Vt.T @ np.diag(sinv) @ U.T
    res = np.zeros_like(H)
    res[np.ix_(keep, keep)] = H[np.ix_(keep, keep)] - H[np.ix_(keep, b)] @ inv @ H[np.ix_(b, keep)]
    return res, s


def condition_prior(H):
    """the ConstraintPoseImu constructor (I/G2oTypes.h:712-718): (H + H) / 2 is H; eigenvalues below 1e-12 become 0."""
    H = (H + H) / 2
    w, V = np.linalg.eigh(H)
    w = np.where(w < 1e-12, 0.0, w)
    return V @ np.diag(w) @ V.T


def imu_information(C):
    """the three C.rowRange().inv(DECOMP_SVD) reads (S/G2oTypes.cc:702-714, S/Optimizer.cc:7798-7813): info9, infoG, infoA."""
    C = np.asarray(C, f32).astype(np.float64)
    inv = lambda M: np.linalg.pinv(M, rcond=1e-15).astype(f32).astype(np.float64)     # (.at<float> of the inverse)
    I9 = inv(C[0:9, 0:9])
    I9 = (I9 + I9.T) / 2
    w, V = np.linalg.eigh(I9)
    w = np.where(w < 1e-12, 0.0, w)
    return V @ np.diag(w) @ V.T, inv(C[9:12, 9:12]), inv(C[12:15, 12:15])


# ------------------------------------------------------------------------------------------------ the solve
def solve(P, variant="kernel", fresh_chi2=False, reverse=False, reverse_solve=False, reverse_residuals=False):
    """Both forms.  fresh_chi2: classify every edge with its error at the FINAL estimate instead of the reference's stale one (for the
    test that shows the rule matters); reverse: every accumulation of the build runs backwards -- the visual terms in reverse index order,
    the edges in reverse order, the inner sums of J^T Omega J over reversed rows; reverse_solve: the factorisation eliminates from the
    last unknown to the first; reverse_residuals: the sums inside the inertial and the visual residuals run backwards.  Together: the
    same mathematics with every order of operations another implementation is free to choose turned round (the rounding yardstick)."""
    form, n = P["form"], P["n"]
    cam = tuple(float(c) for c in P["cam"])
    Tcb = np.asarray(P["Tcb"], np.float64).reshape(3, 4)
    Xw = np.asarray(P["Xw"], np.float64).reshape(-1, 3)
    u, v, ur = [np.asarray(P[k], np.float64) for k in ("u", "v", "ur")]
    om = np.asarray(P["inv_sigma2"], np.float64)
    close = np.asarray(P["close"], bool)
    mono = ur < 0
    pre = P["preint"]
    I9, IG, IA = [np.asarray(P[k], np.float64) for k in ("info9", "infoG", "infoA")]
    cur = make_state(**{k: np.asarray(x, np.float64) for k, x in P["frame"].items()})
    oth = make_state(**{k: np.asarray(x, np.float64) for k, x in P["other"].items()})
    prior = None
    if form == FORM_FRAME:
        pr = P["prior"]
        prior = {"R": np.asarray(pr["Rwb"], np.float64).reshape(3, 3), "t": np.asarray(pr["twb"], np.float64), "v": np.asarray(pr["vwb"], np.float64),
                 "bg": np.asarray(pr["bg"], np.float64), "ba": np.asarray(pr["ba"], np.float64), "H": np.asarray(pr["H"], np.float64).reshape(15, 15)}
    NU = 30 if form == FORM_FRAME else 15
    co = NU - 15
    dM, dS = float(f32(np.sqrt(5.991))), float(f32(np.sqrt(7.815)))
    outlier = np.zeros(n, bool)
    chi2_edge = np.zeros(n)
    robust = True
    n_edges = n + (4 if form == FORM_FRAME else 3)
    chi2_rounds = [0.0] * 4
    decisions = []                                        # (round, index, chi2, threshold, chi2 at the final estimate) of every classification
    solve_failed = False
    rounds_run = 0
    n_bad = n_inl = 0

    def nonvisual(cur, oth, weights=True):
        """stacked Jacobian (rows: inertial 9, gyro walk 3, acc walk 3, prior 15), information blocks, errors, robust weights"""
        Jrows, Wblk, errs = [], [], []
        Ji = inertial_jacobian(oth, cur, pre, variant)
        J = np.zeros((9, NU))
        if form == FORM_FRAME:
            J[:, 0:15] = Ji[:, 0:15]
        J[:, co:co + 9] = Ji[:, 15:24]
        Jrows.append(J); Wblk.append(I9); errs.append(inertial_error(oth, cur, pre, variant, reverse_residuals))
        for k, (a, Iw) in enumerate((("bg", IG), ("ba", IA))):
            J = np.zeros((3, NU))
            if form == FORM_FRAME:
                J[:, 9 + 3 * k:12 + 3 * k] = -np.eye(3)
            J[:, co + 9 + 3 * k:co + 12 + 3 * k] = np.eye(3)
            Jrows.append(J); Wblk.append(Iw); errs.append(cur[a] - oth[a])
        if form == FORM_FRAME:
            J = np.zeros((15, NU))
            J[:, 0:15] = prior_jacobian(oth, prior)
            Jrows.append(J); Wblk.append(prior["H"]); errs.append(prior_error(oth, prior))
        return Jrows, Wblk, errs

    def visual_terms(cur, idx):
        Rcw, tcw = camera_pose(cur, Tcb)
        err, Xc = visual_error(Rcw, tcw, cam, Xw[idx], u[idx], v[idx], ur[idx], reverse_residuals)
        c2 = om[idx] * (err * err).sum(axis=1)
        return err, Xc, c2

    for rnd in range(4):
        rounds_run = rnd + 1
        for it in range(10):
            # computeActiveErrors, buildSystem (G/core/optimization_algorithm_gauss_newton.cpp:50-93)
            act = np.flatnonzero(~outlier)
            H = np.zeros((NU, NU))
            b = np.zeros(NU)
            chi = 0.0
            if len(act):
                err, Xc, c2 = visual_terms(cur, act)
                chi2_edge[act] = c2
                rho0, rho1 = c2.copy(), np.ones(len(act))
                if robust:
                    dl = np.where(mono[act], dM, dS)
                    big = ~(c2 <= dl * dl)
                    sq = np.sqrt(np.where(big, c2, 1.0))
                    rho0 = np.where(big, 2 * sq * dl - dl * dl, c2)
                    rho1 = np.where(big, dl / sq, 1.0)
                Jv = visual_jacobian(Xc, cam, Tcb, mono[act])
                w = (rho1 * om[act])[:, None, None]
                Hv = np.einsum("nka,nkc->nac", Jv, w * Jv)
                bv = -np.einsum("nka,nk->na", Jv, (rho1 * om[act])[:, None] * err)
                H[co:co + 6, co:co + 6] += _seq_sum(Hv, reverse)
                b[co:co + 6] += _seq_sum(bv, reverse)
                chi += float(_seq_sum(rho0, reverse))
            Jrows, Wblk, errs = nonvisual(cur, oth)
            edges = list(enumerate(zip(Jrows, Wblk, errs)))
            for k, (J, W, e) in (edges[::-1] if reverse else edges):
                if reverse:                                               # the same products with every inner sum running backwards
                    J, W, e = J[::-1], W[::-1, ::-1], e[::-1]
                e2 = float(e @ (W @ e))
                r0, r1 = huber(e2, 5.0) if k == 3 else (e2, 1.0)          # the prior edge keeps its Huber kernel (delta 5)
                H += r1 * (J.T @ (W @ J))
                b -= r1 * (J.T @ (W @ e))
                chi += r0
            chi2_rounds[rnd] = chi
            if reverse_solve:                 # the same factorisation from the last unknown to the first
                x = ldlt_solve(H[::-1, ::-1], b[::-1])
                x = None if x is None else x[::-1]
            else:
                x = ldlt_solve(H, b)
            if x is None:
                solve_failed = True
                break
            if form == FORM_FRAME:
                oth = oplus(oth, x[0:15], variant)
            cur = oplus(cur, x[co:co + 15], variant)
        # classification (S/Optimizer.cc:7836-7916, 8246-8324): stale chi2 for active edges, fresh for outliers; float comparison
        if n:
            allidx = np.arange(n)
            _, Xc_f, c2_f = visual_terms(cur, allidx)
            use = c2_f if fresh_chi2 else np.where(outlier, c2_f, chi2_edge)
            chi2_edge = use.copy()
            c2f = use.astype(f32)
            thM = f32(CHI2_MONO[form][rnd])
            thC = f32(1.5 * float(thM))
            thS = f32(CHI2_STEREO[rnd])
            th = np.where(mono, np.where(close, thC, thM), thS).astype(f32)
            with np.errstate(invalid="ignore"):
                bad = (c2f > th) | (mono & ~(Xc_f[:, 2] > 0.0))
            for i in range(n):
                decisions.append((rnd, i, float(use[i]), float(th[i]), float(c2_f[i])))
            outlier = bad
        n_bad = int(outlier.sum())
        n_inl = n - n_bad
        if rnd == 2:
            robust = False
        if n_edges < 10:
            break
    # recovery (S/Optimizer.cc:7919-7946, 8327-8355)
    if n_inl < 30 and not P["rec_init"]:
        n_bad = 0
        if n:
            _, _, c2_f = visual_terms(cur, np.arange(n))
            th = np.where(mono, 18.0, 24.0)
            with np.errstate(invalid="ignore"):
                ok = c2_f < th
            outlier = outlier & ~ok
            n_bad = int((~ok).sum())
            for i in range(n):
                decisions.append((4, i, float(c2_f[i]), float(th[i]), float(c2_f[i])))
    # the Hessian handed to the next frame: final estimate, no robust weights, the correspondences that are not outliers
    Jrows, Wblk, errs = nonvisual(cur, oth)
    H = np.zeros((NU, NU))
    pairs = list(zip(Jrows, Wblk))
    for J, W in (pairs[::-1] if reverse else pairs):
        if reverse:
            J, W = J[::-1], W[::-1, ::-1]
        H += J.T @ (W @ J)
    inl = np.flatnonzero(~outlier)
    if len(inl):
        _, Xc, _ = visual_terms(cur, inl)
        Jv = visual_jacobian(Xc, cam, Tcb, mono[inl])
        H[co:co + 6, co:co + 6] += _seq_sum(np.einsum("nka,nkc->nac", Jv, om[inl][:, None, None] * Jv), reverse)
    sv = np.zeros(0)
    H30 = H.copy()
    if form == FORM_FRAME:
        Hm, sv = marginalize(H, 0, 14)
        H = Hm[15:30, 15:30]
    out = {k: cur[k].copy() for k in cur}
    if variant == "reference":
        out = {k: x.astype(f32).astype(np.float64) for k, x in out.items()}       # SetImuPoseVelocity / IMU::Bias hold floats
    return {"Rwb": out["R"], "twb": out["t"], "vwb": out["v"], "bg": out["bg"], "ba": out["ba"], "outlier": outlier.astype(np.uint8),
            "n_inliers": n - n_bad, "n_bad": n_bad, "rounds_run": rounds_run, "chi2": chi2_rounds, "solve_failed": int(solve_failed),
            "H": H, "H_full": H30, "marg_sv": sv, "decisions": decisions}


def near_threshold(decisions, rel=1e-4):
    """decisions whose chi2 lies within a relative `rel` of its threshold (the band of mlpnp_model.near_threshold)"""
    if not decisions:
        return np.zeros(0, bool)
    d = np.array(decisions)
    return np.abs(d[:, 2] - d[:, 3]) <= rel * d[:, 3]


def state_vector(r):
    return np.concatenate([np.asarray(r["Rwb"]).ravel(), r["twb"], r["vwb"], r["bg"], r["ba"]])


def state_difference(r1, r2):
    return float(np.abs(state_vector(r1) - state_vector(r2)).max())


def hessian_difference(r1, r2):
    """relative to the Frobenius norm of the second"""
    nb = np.linalg.norm(r2["H"])
    return float(np.linalg.norm(np.asarray(r1["H"]) - r2["H"]) / (nb if nb > 0 else 1.0))


# ------------------------------------------------------------------------------------------------ scenes
def integrate_imu(acc, gyr, dt, bg, ba, sigma_g, sigma_a, sigma_gw, sigma_aw):
    """IMU::Preintegrated::IntegrateNewMeasurement (S/ImuTypes.cc:308-366) over the samples, then the members as floats."""
    dR, dV, dP = np.eye(3), np.zeros(3), np.zeros(3)
    JRg, JVg, JVa, JPg, JPa = [np.zeros((3, 3)) for _ in range(5)]
    C = np.zeros((15, 15))
    Nga = np.diag([sigma_g ** 2] * 3 + [sigma_a ** 2] * 3)
    NgaWalk = np.diag([sigma_gw ** 2] * 3 + [sigma_aw ** 2] * 3)
    dT = 0.0
    for a, w in zip(acc, gyr):
        A, B = np.eye(9), np.zeros((9, 6))
        a = a - ba
        wv = w - bg
        dP = dP + dV * dt + 0.5 * dR @ a * dt * dt
        dV = dV + dR @ a * dt
        Wacc = skew(a)
        A[3:6, 0:3] = -dR * dt @ Wacc
        A[6:9, 0:3] = -0.5 * dR * dt * dt @ Wacc
        A[6:9, 3:6] = np.eye(3) * dt
        B[3:6, 3:6] = dR * dt
        B[6:9, 3:6] = 0.5 * dR * dt * dt
        JPa = JPa + JVa * dt - 0.5 * dR * dt * dt
        JPg = JPg + JVg * dt - 0.5 * dR * dt * dt @ Wacc @ JRg
        JVa = JVa - dR * dt
        JVg = JVg - dR * dt @ Wacc @ JRg
        dRi = exp_so3(wv * dt)
        rightJ = right_jacobian_so3(wv * dt)
        dR = normalize_rotation(dR @ dRi)
        A[0:3, 0:3] = dRi.T
        B[0:3, 0:3] = rightJ * dt
        C[0:9, 0:9] = A @ C[0:9, 0:9] @ A.T + B @ Nga @ B.T
        C[9:15, 9:15] += NgaWalk
        JRg = dRi.T @ JRg - rightJ * dt
        dT += dt
    F = lambda x: np.asarray(x, f32)
    return {"dT": f32(dT), "dR": F(dR), "dV": F(dV), "dP": F(dP), "JRg": F(JRg), "JVg": F(JVg), "JVa": F(JVa), "JPg": F(JPg), "JPa": F(JPa),
            "bg": F(bg), "ba": F(ba)}, F(C)


def make_scene(form, n, seed, kind="mixed", outlier_frac=0.0, behind=0, close_frac=0.3, bias_step=0.0, rec_init=0, prior_shift=0.0,
               prior_zero=False, few_inliers=False, noise_px=0.5, perturb=1.0, perturb_other=1.0):
    """A seeded problem: a body moving with constant angular velocity and acceleration from the other end (t = 0) to the frame (t = dT),
    IMU samples at 200 Hz integrated into the preintegration, points in front of the camera, projected with noise and gross outliers.
    bias_step: the frame's and the other end's bias differ from the preintegration's linearisation bias by this much (rad/s, m/s^2)."""
    rng = np.random.default_rng(seed)
    imu_dt = 0.005
    steps = 10 if form == FORM_FRAME else 50
    bg0 = rng.normal(0, 0.01, 3)
    ba0 = rng.normal(0, 0.05, 3)
    omega = rng.normal(0, 0.3, 3)
    accw = rng.normal(0, 1.0, 3)
    R0 = exp_so3(rng.normal(0, 0.3, 3))
    p0 = rng.normal(0, 1.0, 3)
    v0 = rng.normal(0, 0.5, 3)
    sg, sa, sgw, saw = 1.7e-4 * np.sqrt(200), 2.0e-3 * np.sqrt(200), 1.9e-5 / np.sqrt(200), 3.0e-3 / np.sqrt(200)
    acc, gyr = [], []
    R = R0.copy()
    for _ in range(steps):
        gyr.append(omega + bg0)
        acc.append(R.T @ (accw - G_VEC) + ba0)
        R = R @ exp_so3(omega * imu_dt)
    lin_bg, lin_ba = bg0 - bias_step * np.array([1.0, -0.5, 0.25]), ba0 - 10 * bias_step * np.array([0.3, 1.0, -0.6])
    pre, C = integrate_imu(acc, gyr, imu_dt, lin_bg, lin_ba, sg, sa, sgw, saw)
    dT = float(pre["dT"])
    # the true end state from the preintegration at the true bias, so that the inertial edge is consistent with the trajectory
    pre_true, _ = integrate_imu(acc, gyr, imu_dt, bg0, ba0, sg, sa, sgw, saw)
    R1 = R0 @ pre_true["dR"].astype(np.float64)
    v1 = v0 + G_VEC * dT + R0 @ pre_true["dV"].astype(np.float64)
    p1 = p0 + v0 * dT + 0.5 * G_VEC * dT * dT + R0 @ pre_true["dP"].astype(np.float64)
    Tcb = np.zeros((3, 4))
    Tcb[:, :3] = exp_so3(np.array([0.02, -0.01, 1.55]))
    Tcb[:, 3] = [0.05, -0.02, 0.01]
    Tcb = Tcb.astype(f32)
    cam = tuple(f32(c) for c in (458.654, 457.296, 367.215, 248.375, 47.9))
    # points in front of the true camera
    true_cur = make_state(R1, p1, v1, bg0, ba0)
    Rcw, tcw = camera_pose(true_cur, Tcb.astype(np.float64))
    z = rng.uniform(2.0, 25.0, n)
    uu = rng.uniform(20, 730, n)
    vv = rng.uniform(20, 460, n)
    Xc = np.stack([(uu - float(cam[2])) / float(cam[0]) * z, (vv - float(cam[3])) / float(cam[1]) * z, z], axis=1)
    if behind:
        Xc[:behind, 2] *= -1.0                      # behind the camera: isDepthPositive() fails
    Xw = ((Xc - tcw) @ Rcw).astype(f32)
    err, Xc2 = visual_error(Rcw, tcw, tuple(float(c) for c in cam), Xw.astype(np.float64), np.zeros(n), np.zeros(n), np.ones(n))
    pu, pv = -err[:, 0], -err[:, 1]
    pr = 1.0 - err[:, 2]
    octave = rng.integers(0, 8, n)
    inv_sigma2 = (1.0 / 1.2 ** (2 * octave)).astype(f32)
    sig = noise_px * 1.2 ** octave
    u = pu + rng.normal(0, 1, n) * sig
    v = pv + rng.normal(0, 1, n) * sig
    r = pr + rng.normal(0, 1, n) * sig
    if kind == "mono":
        is_mono = np.ones(n, bool)
    elif kind == "stereo":
        is_mono = np.zeros(n, bool)
    else:
        is_mono = rng.random(n) < 0.5
    is_mono[:behind] = True
    nout = int(round(outlier_frac * n))
    if few_inliers:
        nout = max(n - 20, 0)
    oi = rng.permutation(n)[:nout]
    u[oi] += rng.choice([-1, 1], nout) * rng.uniform(15, 60, nout)
    v[oi] += rng.choice([-1, 1], nout) * rng.uniform(15, 60, nout)
    ur = np.where(is_mono, -1.0, np.maximum(r, 0.0)).astype(f32)
    close = ((z < 10.0) & (rng.random(n) < close_frac / 0.35)).astype(np.uint8)
    # the estimates handed in: the truth, perturbed
    pt = lambda s, k: rng.normal(0, s, k) * perturb
    frame = {"Rwb": (R1 @ exp_so3(pt(0.01, 3))).astype(f32), "twb": (p1 + pt(0.03, 3)).astype(f32), "vwb": (v1 + pt(0.05, 3)).astype(f32),
             "bg": (bg0 + pt(1e-4, 3)).astype(f32), "ba": (ba0 + pt(1e-3, 3)).astype(f32)}
    pt = lambda s, k: rng.normal(0, s, k) * perturb_other
    other = {"Rwb": (R0 @ exp_so3(pt(0.002, 3))).astype(f32), "twb": (p0 + pt(0.005, 3)).astype(f32), "vwb": (v0 + pt(0.01, 3)).astype(f32),
             "bg": (bg0 + pt(1e-4, 3)).astype(f32), "ba": (ba0 + pt(1e-3, 3)).astype(f32)}
    if bias_step == 0.0:
        # the bias at the linearisation point: dbg = dba = 0 exactly, the small-angle branches
        frame["bg"] = other["bg"] = pre["bg"].copy()
        frame["ba"] = other["ba"] = pre["ba"].copy()
    info9, infoG, infoA = imu_information(C)
    P = {"form": form, "rec_init": int(rec_init), "n": n, "Xw": Xw, "u": u.astype(f32), "v": v.astype(f32), "ur": ur, "inv_sigma2": inv_sigma2,
         "close": close, "cam": cam, "Tcb": Tcb, "frame": frame, "other": other, "preint": pre, "C": C, "info9": info9, "infoG": infoG,
         "infoA": infoA, "prior": None, "truth": {"cur": true_cur, "other": make_state(R0, p0, v0, bg0, ba0)}}
    if form == FORM_FRAME:
        o64 = {k: x.astype(np.float64) for k, x in other.items()}
        A = rng.normal(0, 1, (15, 15))
        scale = np.array([300.0] * 3 + [100.0] * 3 + [30.0] * 3 + [3000.0] * 3 + [300.0] * 3)
        Hp = np.diag(scale) @ (np.eye(15) + 0.05 * (A + A.T) / 2) @ np.diag(scale)
        Hp = condition_prior((Hp + Hp.T) / 2)
        if prior_zero:
            Hp = np.zeros((15, 15))
        sh = prior_shift
        P["prior"] = {"Rwb": o64["Rwb"] @ exp_so3(sh * np.array([0.01, -0.02, 0.015])), "twb": o64["twb"] + sh * np.array([0.05, 0.02, -0.04]),
                      "vwb": o64["vwb"] + sh * np.array([0.05, -0.1, 0.02]), "bg": o64["bg"].copy(), "ba": o64["ba"].copy(), "H": Hp}
    return P


# the cases both GPU and CPU tests run: (name, form, n, seed, scene arguments)
def _cases():
    out = []
    for form, fname in ((FORM_KF, "kf"), (FORM_FRAME, "fr")):
        for n in (0, 6, 7, 255, 256, 257, 600):
            out.append(("%s_n%d" % (fname, n), form, n, 100 + n + 1000 * form, dict(kind="mixed", outlier_frac=0.1 if n >= 255 else 0.0)))
        out.append(("%s_mono" % fname, form, 300, 11 + form, dict(kind="mono", outlier_frac=0.2)))
        out.append(("%s_stereo" % fname, form, 300, 13 + form, dict(kind="stereo", outlier_frac=0.2)))
        out.append(("%s_behind" % fname, form, 120, 15 + form, dict(kind="mixed", outlier_frac=0.2, behind=3, close_frac=0.35)))
        out.append(("%s_bias_step" % fname, form, 200, 17 + form, dict(kind="mixed", outlier_frac=0.1, bias_step=2e-3)))
        out.append(("%s_recover" % fname, form, 60, 19 + form, dict(kind="mixed", few_inliers=True, rec_init=0)))
        out.append(("%s_recinit" % fname, form, 60, 19 + form, dict(kind="mixed", few_inliers=True, rec_init=1)))
    out.append(("fr_prior_huber", FORM_FRAME, 150, 31, dict(kind="mixed", outlier_frac=0.1, prior_shift=1.0)))
    out.append(("fr_prior_zero", FORM_FRAME, 150, 33, dict(kind="mixed", outlier_frac=0.1, prior_zero=True)))
    return out


CASES = _cases()
CAP_CASES = [("kf_n4096", FORM_KF, 4096, 41, dict(kind="mixed", outlier_frac=0.1)), ("fr_n4096", FORM_FRAME, 4096, 43, dict(kind="mixed", outlier_frac=0.1))]
CHAIN_SEED, CHAIN_LEN, CHAIN_N = 51, 5, 120
MARGIN = 8                                    # "another implementation with another operation order" (tests/test_gpu_mlpnp.py)
BAND_CAP = 1e-3                               # at most 0.1 % of the decisions may lie in the near-threshold band


def build_case(case):
    _, form, n, seed, kw = case
    return make_scene(form, n, seed, **kw)


_memo = {}


def case_results(case):
    """The problem and the model runs of a case (kernel arithmetic forward, reversed_runs, reference arithmetic), computed once."""
    name = case[0]
    if name not in _memo:
        P = build_case(case)
        _memo[name] = (P, solve(P, "kernel"), reversed_runs(P), solve(P, "reference"))
    return _memo[name]


EPS = float(np.finfo(np.float64).eps)


def yardstick_floor(rb):
    """What a difference of results cannot be measured below: one unit in the last place of the largest state component, and of H's norm
    (H is compared relative to it).  A forward and a reversed run that agree to the last bit -- n = 0 has no sum to reverse -- would
    otherwise ask another implementation for the same bits, down to its sine and cosine."""
    return EPS * max(1.0, float(np.abs(state_vector(rb)).max())), EPS


def reversed_runs(P):
    """The reversed-order runs of the yardstick: the build's sums; those and the factorisation; those and the residuals' sums.  One run
    is one sample of the rounding noise, a few ulp that may come out as none; the yardstick is the largest of the three."""
    return [solve(P, "kernel", reverse=True), solve(P, "kernel", reverse=True, reverse_solve=True),
            solve(P, "kernel", reverse=True, reverse_solve=True, reverse_residuals=True)]


def yardsticks_of(rb, rr, ra):
    """rr: the list of reversed_runs"""
    fs, fh = yardstick_floor(rb)
    return {"ab_state": state_difference(ra, rb), "ab_H": hessian_difference(ra, rb),
            "fr_state": max([state_difference(r, rb) for r in rr] + [fs]), "fr_H": max([hessian_difference(r, rb) for r in rr] + [fh])}


def yardsticks(case):
    """(a)-vs-(b) and (b)-forward-vs-reversed differences of a case: state (absolute) and H (relative Frobenius); the second pair is
    floored at yardstick_floor."""
    _, rb, rr, ra = case_results(case)
    return yardsticks_of(rb, rr, ra)


def chain_problems(step, prev_result=None, prev_problem=None):
    """Problem `step` of the chain test: consecutive LastFrame calls, each with the previous call's H (through condition_prior) as the
    information of its prior; the prior's state is the scene's own other end."""
    P = make_scene(FORM_FRAME, CHAIN_N, CHAIN_SEED + step, kind="mixed", outlier_frac=0.1)
    if prev_result is not None:
        P["prior"]["H"] = condition_prior(np.asarray(prev_result["H"], np.float64).reshape(15, 15))
    return P


def to_c_problem(P, device=0):
    """The views.pose_inertial_problem of a model problem: (problem, keep-alive)."""
    from multi_orbslam3_amd import views
    prior = None
    if P["form"] == FORM_FRAME and P["prior"] is not None:
        prior = P["prior"]
    return views.pose_inertial_problem(P["form"], P["Xw"], P["u"], P["v"], P["ur"], P["inv_sigma2"], P["close"], P["cam"], P["Tcb"], P["frame"],
                                       P["other"], P["preint"], P["info9"], P["infoG"], P["infoA"], prior=prior, rec_init=P["rec_init"],
                                       device=device)
