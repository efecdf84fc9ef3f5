"""Float64 numpy restatement of the numerical core of Optimizer::BundleAdjustment (S/Optimizer.cc:73-446): every edge with the
camera of its own keyframe, Huber kernels on or off, ONE optimize(nIterations) of g2o's Levenberg-Marquardt
(G/core/optimization_algorithm_levenberg.cpp:68-159 with the reference's nBad rule), BlockSolver<6,3>'s Schur complement, and the
values the reference reads back (poses, points, e->chi2(), e->isDepthPositive(), the vertices without an edge).

Per-edge residuals and Jacobians come from the oracle's edge evaluation (oracle.binding.lba_edge_eval, called with the edge's own
camera; lba_edge_eval_rig for a KannalaBrandt8 keyframe), which tests/test_oracle_matching_lba.py and tests/test_oracle_rig.py pin
against central differences.  Everything above the edges -- normal equations, Schur complement, solve, back-substitution, the LM
control flow and its trace -- is written here, independently of the product and of the oracle's solver.
tests/test_full_ba_cpu.py pins it (against the oracle's local BA, robust against non-robust, conditioning, cameras)."""
import numpy as np

from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import views
from oracle import binding as ob

from dense_lm import oplus, quat_from_R, quat_rot

# thHuber2D = sqrt(5.99), thHuber3D = sqrt(7.815), both float (S/Optimizer.cc:131-132; the local BA has 5.991)
D_MONO, D_STEREO = float(np.float32(np.sqrt(5.99))), float(np.float32(np.sqrt(7.815)))


class BaModelResult:
    pass


def _camera_args(cameras):
    out = []
    for cam in cameras:
        five = np.array([np.float32(c) for c in cam[:5]], np.float32)
        model = cam[5] if len(cam) > 5 else None
        rig = views.camera_rig(model) if model is not None and model[0] != capi.CAM_PINHOLE else None
        out.append((five, rig))
    return out


def _rot_of(q):
    return np.array([quat_rot(q, ex) for ex in np.eye(3)]).T


def kb8_residual(model, Xc, edge, angles):
    """The residual of a monocular edge through KannalaBrandt8::project (S/CameraModels/KannalaBrandt8.cpp:52-69) as oracle/lba.cc's
    cam_project writes it, except for where theta and psi -- float32 VALUES in the reference -- come from:
    'rounded_double': the double atan2 rounded to float (what the device computes; the oracle calls the host's atan2f);
    'ulp_up' / 'ulp_down': that value moved by one float32 ulp, theta and psi of every edge in the same direction."""
    _, fx, fy, cx, cy, k1, k2, k3, k4 = [float(np.float32(c)) for c in model]
    x2y2 = Xc[0] * Xc[0] + Xc[1] * Xc[1]
    theta = np.float32(np.arctan2(float(np.sqrt(np.float32(x2y2))), float(np.float32(Xc[2]))))
    psi = np.float32(np.arctan2(float(np.float32(Xc[1])), float(np.float32(Xc[0]))))
    if angles in ("ulp_up", "ulp_down"):
        to = np.float32(np.inf if angles == "ulp_up" else -np.inf)
        theta, psi = np.nextafter(theta, to), np.nextafter(psi, to)
    else:
        assert angles == "rounded_double", angles
    theta, psi = float(theta), float(psi)
    t2 = theta * theta
    t3 = theta * t2; t5 = t3 * t2; t7 = t5 * t2; t9 = t7 * t2
    r = theta + k1 * t3 + k2 * t5 + k3 * t7 + k4 * t9
    return np.array([float(edge["u"][0]) - (fx * r * np.cos(psi) + cx), float(edge["v"][0]) - (fy * r * np.sin(psi) + cy), 0.0])


def solve(pr, iterations, robust, stop_after_trials=None, reverse_sums=False, pose_camera=None, stop_before=False, kb8_angles="oracle"):
    """pr: a synth.make_ba_problem dict (poses, pose_fixed, pose_camera, points, edges, cameras).
    stop_after_trials = k: the abort flag reads as raised once k LM trials have been evaluated (ba_solve's -k form);
    stop_before: raised before optimize() (INT32_MIN).  reverse_sums: every sum over the edges of a point, and over the points of
    a pose pair, runs in reversed order (the conditioning check).  pose_camera: override of pr['pose_camera'].
    kb8_angles: 'oracle' (atan2f of this host, inside the oracle's edge evaluation) or one of kb8_residual's forms."""
    E = pr["edges"]
    NE = len(E)
    P = len(pr["poses"])
    L = len(pr["points"])
    pcam = np.asarray(pr["pose_camera"] if pose_camera is None else pose_camera, np.int64)
    cams = _camera_args(pr["cameras"])
    free = [i for i in range(P) if not pr["pose_fixed"][i]]
    pcol = {i: c for c, i in enumerate(free)}
    nP = len(free)
    q, t = [], []
    for i in range(P):
        T = np.asarray(pr["poses"][i], np.float32).reshape(4, 4).astype(np.float64)
        qi = quat_from_R(T[:3, :3])
        q.append(qi / np.linalg.norm(qi)); t.append(T[:3, 3].copy())
    X = np.asarray(pr["points"], np.float32).astype(np.float64).reshape(-1, 3)
    e_pose = E["pose"].astype(np.int64); e_point = E["point"].astype(np.int64)
    mono = E["ur"] < 0
    om = E["inv_sigma2"].astype(np.float64)
    edge1 = [np.array([e], capi.EDGE_DTYPE) for e in E]
    pt_edges = [[] for _ in range(L)]
    for k in range(NE):
        pt_edges[e_point[k]].append(k)
    included = np.array([1 if pt_edges[l] else 0 for l in range(L)], np.uint8)
    order = (lambda lst: lst[::-1]) if reverse_sums else (lambda lst: lst)

    def evaluate(q_, t_, X_, jac):
        """chi2 per edge, rho0 / rho1, and with jac: A (d err / d point), B (d err / d pose), err"""
        chi = np.zeros(NE); rho0 = np.zeros(NE); rho1 = np.ones(NE)
        errs = np.zeros((NE, 3)); As = np.zeros((NE, 3, 3)); Bs = np.zeros((NE, 3, 6))
        for k in range(NE):
            i, l = e_pose[k], e_point[k]
            five, rig = cams[pcam[i]]
            if rig is not None:
                err, A, B, Xc = ob.lba_edge_eval_rig(q_[i], t_[i], X_[l], five, rig, edge1[k])
                if kb8_angles != "oracle" and mono[k]:
                    res.max_kb8_residual_shift = max(res.max_kb8_residual_shift, 0.0)
                    e2 = kb8_residual(pr["cameras"][pcam[i]][5], Xc, edge1[k], kb8_angles)
                    res.max_kb8_residual_shift = max(res.max_kb8_residual_shift, float(np.abs(e2[:2] - err[:2]).max()))
                    err = e2
            else:
                err, A, B = ob.lba_edge_eval(q_[i], t_[i], X_[l], five, edge1[k])
            D = 2 if mono[k] else 3
            c2 = 0.0
            for d in range(D):
                c2 += err[d] * (om[k] * err[d])
            chi[k] = c2
            res.max_edge_chi2 = max(res.max_edge_chi2, c2)
            delta = D_MONO if mono[k] else D_STEREO
            if robust and c2 > delta * delta:
                s = np.sqrt(c2)
                rho0[k] = 2 * s * delta - delta * delta; rho1[k] = delta / s
            else:
                rho0[k] = c2
            if jac:
                if D == 2:
                    err = err.copy(); err[2] = 0; A = A.copy(); A[2] = 0; B = B.copy(); B[2] = 0
                errs[k] = err; As[k] = A; Bs[k] = B
        return chi, rho0, rho1, errs, As, Bs

    res = BaModelResult()
    res.trace = []
    res.iters = 0
    res.chi2_initial = res.chi2_final = 0.0
    res.min_abs_rho = np.inf
    res.trial_gain = []                         # per trial: (chi2 before - chi2 of the trial, computeScale): rho = first / (second + 1e-3)
    res.max_kb8_residual_shift = 0.0            # px: largest difference between kb8_residual and the oracle's residual
    res.max_edge_chi2 = 0.0                     # over every evaluation of the solve, rejected trials included
    res.point_included = included
    trials_done = [0]
    last_chi = np.zeros(NE)

    def stop():
        if stop_before:
            return True
        return stop_after_trials is not None and trials_done[0] >= stop_after_trials

    lam, ni, nbad = -1.0, 2.0, 0
    cur_chi = 0.0
    ok = True
    it = 0
    n_iter = iterations if NE > 0 else 0
    while it < n_iter and not stop() and ok:
        chi, rho0, rho1, errs, As, Bs = evaluate(q, t, X, True)
        last_chi = chi
        cur_chi = float(np.sum(rho0))
        w = rho1 * om
        Hpp = np.zeros((nP, 6, 6)); bp = np.zeros((nP, 6))
        Hll = np.zeros((L, 3, 3)); bl = np.zeros((L, 3)); Hpl = {}
        for k in range(NE):
            if e_pose[k] in pcol:
                c = pcol[e_pose[k]]
                Hpp[c] += Bs[k].T @ (w[k] * Bs[k]); bp[c] -= Bs[k].T @ (w[k] * errs[k])
                Hpl[k] = Bs[k].T @ (w[k] * As[k])
        for l in range(L):
            for k in order(pt_edges[l]):
                Hll[l] += As[k].T @ (w[k] * As[k]); bl[l] -= As[k].T @ (w[k] * errs[k])
        if it == 0:
            md = 0.0
            for c in range(nP):
                md = max(md, np.abs(np.diag(Hpp[c])).max())
            for l in range(L):
                if included[l]:
                    md = max(md, np.abs(np.diag(Hll[l])).max())
            lam = 1e-5 * md
            ni, nbad = 2.0, 0
            res.chi2_initial = cur_chi
        ini_chi = cur_chi
        rho, qmax = 0.0, 0
        while True:
            Dinv = np.zeros((L, 3, 3))
            for l in range(L):
                if included[l]:
                    Dinv[l] = np.linalg.inv(Hll[l] + lam * np.eye(3))
            S = np.zeros((6 * nP, 6 * nP)); bs = np.zeros(6 * nP)
            for c in range(nP):
                S[6 * c:6 * c + 6, 6 * c:6 * c + 6] = Hpp[c] + lam * np.eye(6)
                bs[6 * c:6 * c + 6] = bp[c]
            for l in order(list(range(L))):
                fe = [k for k in pt_edges[l] if k in Hpl]
                for ka in fe:
                    ca = pcol[e_pose[ka]]
                    Wm = Hpl[ka] @ Dinv[l]
                    bs[6 * ca:6 * ca + 6] -= Wm @ bl[l]
                    for kb in fe:
                        cb = pcol[e_pose[kb]]
                        S[6 * ca:6 * ca + 6, 6 * cb:6 * cb + 6] -= Wm @ Hpl[kb].T
            solved = True
            x = np.zeros(6 * nP)
            if nP:
                try:
                    x = np.linalg.solve(S, bs)
                    solved = bool(np.all(np.isfinite(x)))
                except np.linalg.LinAlgError:
                    solved = False
                if not solved:
                    x = np.zeros(6 * nP)
            scale = 0.0
            q2, t2, X2 = list(q), list(t), X.copy()
            if solved:
                for i in free:
                    u = x[6 * pcol[i]:6 * pcol[i] + 6]
                    scale += float(np.sum(u * (lam * u + bp[pcol[i]])))
                    qn, tn = oplus(q[i], t[i], u)
                    if qn[3] < 0:
                        qn = -qn
                    q2[i] = qn / np.linalg.norm(qn); t2[i] = tn
                for l in range(L):
                    if not included[l]:
                        continue
                    rr = bl[l].copy()
                    for k in order(pt_edges[l]):
                        if k in Hpl:
                            c = pcol[e_pose[k]]
                            rr -= Hpl[k].T @ x[6 * c:6 * c + 6]
                    xl = Dinv[l] @ rr
                    scale += float(np.sum(xl * (lam * xl + bl[l])))
                    X2[l] = X[l] + xl
            chi_t, rho0_t, _, _, _, _ = evaluate(q2, t2, X2, False)
            last_chi = chi_t
            temp = float(np.sum(rho0_t)) if solved else np.finfo(np.float64).max
            rho = (cur_chi - temp) / (scale + 1e-3)
            res.min_abs_rho = min(res.min_abs_rho, abs(rho))
            res.trial_gain.append((cur_chi - temp, scale))
            if rho > 0 and np.isfinite(temp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur_chi = temp
                q, t, X = q2, t2, X2
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            trials_done[0] += 1
            if not (rho < 0 and qmax < 10 and not stop()):
                break
        it += 1
        res.iters = it
        res.chi2_final = cur_chi
        res.trace.append((lam, cur_chi, qmax))
        if qmax == 10 or rho == 0:
            ok = False
            continue
        if (ini_chi - cur_chi) * 1e3 < ini_chi:
            nbad += 1
        else:
            nbad = 0
        if nbad >= 3:
            ok = False
    res.trace = np.array(res.trace, np.float64).reshape(-1, 3)
    res.poses64 = np.zeros((P, 4, 4))
    for i in range(P):
        res.poses64[i] = np.eye(4)
        res.poses64[i, :3, :3] = _rot_of(q[i] / np.linalg.norm(q[i]))
        res.poses64[i, :3, 3] = t[i]
    res.poses = res.poses64.astype(np.float32).reshape(P, 16)
    res.points = X.astype(np.float32)
    res.edge_chi2 = last_chi if res.iters > 0 else np.zeros(NE)
    res.edge_depth_pos = np.array([1 if (quat_rot(q[e_pose[k]], X[e_point[k]]) + t[e_pose[k]])[2] > 0 else 0 for k in range(NE)], np.uint8)
    return res
