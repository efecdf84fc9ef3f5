"""numpy model of Optimizer::InertialOptimization (S/Optimizer.cc:5344-5958, four overloads), restated from the reference's text, the
yardstick of inertial_init_solve (include/orbgpu.h).

The graph: every pose fixed; one EdgeInertialGS (S/G2oTypes.cc:802-927) per keyframe with an mPrevKF over the two velocities, ONE gyro
bias, ONE accelerometer bias, the gravity direction (VertexGDir: Rwg ExpSO3(u0, u1, 0)) and the scale (VertexScale: s exp(u)); EdgePriorAcc
and EdgePriorGyro toward 0 on the biases (active only while the biases are free: g2o drops an edge whose vertices are all fixed).  What is
free, the algorithm and the iteration count are the problem's switches; form_problem() sets them as each overload does.

Two variants, as tests/pose_inertial_model.py has them (its SO3 functions and bias-corrected deltas are imported, not restated):
  "reference": float round trips where the reference has them -- ExpSO3 through a float32 SVD, the float GetDeltaRotation / Velocity /
               Position, the float velocities written back to the keyframes;
  "kernel":    double throughout, which is what the device kernel computes.
Both share the stated deviation of the entry point: a solve that meets a pivot which is not positive and finite is refused -- under LM
the trial counts as failed, under Gauss-Newton no update is applied, solve_failed is set and the run ends.

The linear solve comes in two formulations:
  (a) dense: the normal equations through numpy.linalg (solve after a Cholesky test) -- beyond DENSE_MAX unknowns, where a dense matrix
      no longer fits, the elimination below with numpy.linalg.solve on every block instead of cofactors and LDL^T;
  (b) the kernel's: every velocity eliminated after all of its successors in the mPrevKF forest (3 x 3 inverse by cofactors), the Schur
      terms subtracted from the 9 x 9 corner, the corner by LDL^T without pivoting, back-substitution in reverse order.
Their difference per case is the rounding yardstick of the GPU test.

Unknown layout of an edge's block, as inertial_init_host_linearize returns it: [v1 3 | v2 3 | bg 3 | ba 3 | gdir 2 | s 1 | e 1].
"""
import os
import re

import numpy as np

import pose_inertial_model as pim

f32 = np.float32
GRAVITY = pim.GRAVITY
LM, GN = 0, 1
DENSE_MAX = 2000
PIVOT_REL = pim.PIVOT_REL           # Gauss-Newton's corner: a pivot this small against its diagonal entry is rounding noise
BAND = 1e-4
BAND_CAP = pim.BAND_CAP
MARGIN = pim.MARGIN
NOISE_ROW = 1e-3                    # tests/inertial_ba_model.py: a trace row the model's own two solves do not reproduce to this is noise
EPS = float(np.finfo(np.float64).eps)
GI = np.array([0.0, 0.0, -GRAVITY])
GM = np.array([[0.0, -GRAVITY], [GRAVITY, 0.0], [0.0, 0.0]])


# ------------------------------------------------------------------------------------------------ vertices
def gdir_oplus(Rwg, u, variant="kernel"):
    """GDirection::Update (I/G2oTypes.h:261-264)"""
    return Rwg @ pim.exp_so3(np.array([u[0], u[1], 0.0]), variant)


def scale_oplus(s, u):
    """VertexScale::oplusImpl (I/G2oTypes.h:311-313)"""
    return s * np.exp(u)


def initial_state(P):
    K = P["keyframes"]
    return {"v": K["v"].astype(np.float64).copy(), "bg": P["bg"].astype(np.float64), "ba": P["ba"].astype(np.float64),
            "Rwg": np.array(P["Rwg"], np.float64), "s": float(P["scale"])}


# ------------------------------------------------------------------------------------------------ the edge
def gs_error(R1, t1, v1, R2, t2, v2, bg, ba, Rwg, s, pre, variant="kernel"):
    """EdgeInertialGS::computeError (S/G2oTypes.cc:826-849)"""
    dt = float(pre["dT"])
    g = Rwg @ GI
    dR, dV, dP = pim.preint_deltas(pre, bg, ba, variant)
    R1t = R1.T
    er = pim.log_so3(dR.T @ R1t @ R2)
    ev = R1t @ (s * (v2 - v1) - g * dt) - dV
    ep = R1t @ (s * (t2 - t1 - v1 * dt) - g * dt * dt / 2) - dP
    return np.concatenate([er, ev, ep])


def gs_jacobian(R1, t1, v1, R2, t2, v2, bg, ba, Rwg, s, pre, variant="kernel"):
    """EdgeInertialGS::linearizeOplus (S/G2oTypes.cc:851-927) without the (fixed) poses: 9 x 15 = [v1 | v2 | bg | ba | gdir | s]."""
    dt = float(pre["dT"])
    D = lambda k: pre[k].astype(np.float64)
    dbg = bg - D("bg")
    if variant == "reference":
        dbg = (bg.astype(f32) - pre["bg"].astype(f32)).astype(np.float64)
    R1t = R1.T
    dR, _, _ = pim.preint_deltas(pre, bg, ba, variant)
    eR = dR.T @ R1t @ R2
    invJr = pim.inv_right_jacobian_so3(pim.log_so3(eR))
    dGdTheta = Rwg @ GM
    J = np.zeros((9, 15))
    J[3:6, 0:3] = -s * R1t
    J[6:9, 0:3] = -s * R1t * dt
    J[3:6, 3:6] = s * R1t
    J[0:3, 6:9] = -invJr @ eR.T @ pim.right_jacobian_so3(D("JRg") @ dbg) @ D("JRg")
    J[3:6, 6:9] = -D("JVg")
    J[6:9, 6:9] = -D("JPg")
    J[3:6, 9:12] = -D("JVa")
    J[6:9, 9:12] = -D("JPa")
    J[3:6, 12:14] = -R1t @ dGdTheta * dt
    J[6:9, 12:14] = -0.5 * R1t @ dGdTheta * dt * dt
    J[3:6, 14] = R1t @ (v2 - v1)
    J[6:9, 14] = R1t @ (t2 - t1 - v1 * dt)
    return J


def edge_block(P, S, e, variant="kernel"):
    """the 9 x 16 block of edge e at state S, every vertex taken as free"""
    K, E = P["keyframes"], P["edges"][e]
    a = (K["R"][E["k1"]].astype(np.float64), K["t"][E["k1"]].astype(np.float64), S["v"][E["k1"]], K["R"][E["k2"]].astype(np.float64),
         K["t"][E["k2"]].astype(np.float64), S["v"][E["k2"]], S["bg"], S["ba"], S["Rwg"], S["s"], E["preint"], variant)
    return np.concatenate([gs_jacobian(*a), gs_error(*a)[:, None]], axis=1)


class Graph:
    """what the host half of the entry point derives: the forest, the elimination order, the free columns"""

    def __init__(self, P):
        self.nk, self.ne = len(P["keyframes"]["v"]), len(P["edges"])
        self.k1 = np.array([e["k1"] for e in P["edges"]], np.int64)
        self.k2 = np.array([e["k2"] for e in P["edges"]], np.int64)
        self.pred = -np.ones(self.nk, np.int64)
        self.pred[self.k2] = self.k1
        self.in_system = np.zeros(self.nk, bool)
        self.in_system[self.k1] = True
        self.in_system[self.k2] = True
        children = [[] for _ in range(self.nk)]
        for e in range(self.ne):
            children[self.k1[e]].append(int(self.k2[e]))
        order = []
        for root in range(self.nk):
            if not self.in_system[root] or self.pred[root] >= 0:
                continue
            stack, nxt = [root], {}
            while stack:
                k = stack[-1]
                i = nxt.get(k, 0)
                if i < len(children[k]):
                    nxt[k] = i + 1
                    stack.append(children[k][i])
                else:
                    order.append(k)
                    stack.pop()
        self.order = np.array(order, np.int64)
        self.nv = int(self.in_system.sum())
        assert len(order) == self.nv, "the predecessor relation has a cycle"
        self.free_v = bool(P["free_velocity"])
        fm = np.zeros(9, bool)
        fm[0:6] = bool(P["free_bias"])
        fm[6:8] = bool(P["free_gdir"])
        fm[8] = bool(P["free_scale"])
        self.fm = fm
        self.nb = int(fm.sum())
        self.priors = bool(P["with_priors"]) and bool(P["free_bias"])
        self.n_unknowns = (3 * self.nv if self.free_v else 0) + self.nb
        self.W = np.stack([np.asarray(e["info9"], np.float64).reshape(9, 9) for e in P["edges"]])


_rot_cache = {}


def _errors_jacobians(P, G, S, variant, jac):
    """e (ne, 9) and, with jac, J (ne, 9, 15) at S.  The bias-dependent part of an edge (the deltas, the rotation residual and its
    Jacobian) goes through pose_inertial_model edge by edge and is kept per bias: most problems evaluate many states at one bias."""
    K = P["keyframes"]
    key = (id(P), variant, S["bg"].tobytes(), S["ba"].tobytes())
    hit = _rot_cache.get(key)
    if hit is None or (jac and hit[3] is None):
        er, dV, dP = np.zeros((G.ne, 3)), np.zeros((G.ne, 3)), np.zeros((G.ne, 3))
        Jr = np.zeros((G.ne, 3, 3)) if jac else None
        for e, E in enumerate(P["edges"]):
            pre = E["preint"]
            R1, R2 = K["R"][E["k1"]].astype(np.float64), K["R"][E["k2"]].astype(np.float64)
            dR, dV[e], dP[e] = pim.preint_deltas(pre, S["bg"], S["ba"], variant)
            eR = dR.T @ R1.T @ R2
            er[e] = pim.log_so3(eR)
            if jac:
                JRg = pre["JRg"].astype(np.float64)
                dbg = S["bg"] - pre["bg"].astype(np.float64)
                if variant == "reference":
                    dbg = (S["bg"].astype(f32) - pre["bg"].astype(f32)).astype(np.float64)
                Jr[e] = -pim.inv_right_jacobian_so3(er[e]) @ eR.T @ pim.right_jacobian_so3(JRg @ dbg) @ JRg
        if len(_rot_cache) > 8:
            _rot_cache.clear()
        hit = _rot_cache[key] = (er, dV, dP, Jr)
    er, dV, dP, Jr = hit
    R1t = np.transpose(K["R"][G.k1].astype(np.float64), (0, 2, 1))
    t1, t2 = K["t"][G.k1].astype(np.float64), K["t"][G.k2].astype(np.float64)
    v1, v2 = S["v"][G.k1], S["v"][G.k2]
    dt = P["_dt"][:, None]
    g = S["Rwg"] @ GI
    s = S["s"]
    dvv, dpp = v2 - v1, t2 - t1 - v1 * dt
    ev = np.einsum("eij,ej->ei", R1t, s * dvv - g * dt) - dV
    ep = np.einsum("eij,ej->ei", R1t, s * dpp - g * dt * dt / 2) - dP
    err = np.concatenate([er, ev, ep], axis=1)
    if not jac:
        return err, None
    J = np.zeros((G.ne, 9, 15))
    J[:, 3:6, 0:3] = -s * R1t
    J[:, 6:9, 0:3] = -s * R1t * dt[:, :, None]
    J[:, 3:6, 3:6] = s * R1t
    J[:, 0:3, 6:9] = Jr
    J[:, 3:6, 6:9] = -P["_JVg"]
    J[:, 6:9, 6:9] = -P["_JPg"]
    J[:, 3:6, 9:12] = -P["_JVa"]
    J[:, 6:9, 9:12] = -P["_JPa"]
    RG = R1t @ (S["Rwg"] @ GM)
    J[:, 3:6, 12:14] = -RG * dt[:, :, None]
    J[:, 6:9, 12:14] = -0.5 * RG * dt[:, :, None] * dt[:, :, None]
    J[:, 3:6, 14] = np.einsum("eij,ej->ei", R1t, dvv)
    J[:, 6:9, 14] = np.einsum("eij,ej->ei", R1t, dpp)
    return err, J


def _prior_chi2(P, G, S):
    if not G.priors:
        return 0.0
    return float(np.sum(S["ba"] * (P["prior_a"] * S["ba"])) + np.sum(S["bg"] * (P["prior_g"] * S["bg"])))


def evaluate(P, G, S, variant):
    err, _ = _errors_jacobians(P, G, S, variant, False)
    We = np.einsum("eij,ej->ei", G.W, err)
    return float(np.sum(np.sum(err * We, axis=1))) + _prior_chi2(P, G, S)


def linearise(P, G, S, variant):
    """the per-vertex blocks D, O (toward the predecessor), B (toward the border), b; the corner C, its right-hand side rc; chi2"""
    err, J = _errors_jacobians(P, G, S, variant, True)
    WJ = G.W @ J
    We = np.einsum("eij,ej->ei", G.W, err)
    He = np.transpose(J, (0, 2, 1)) @ WJ
    be = -np.einsum("eri,er->ei", J, We)
    chi = float(np.sum(np.sum(err * We, axis=1))) + _prior_chi2(P, G, S)
    nk = G.nk
    D, O, B, b = np.zeros((nk, 3, 3)), np.zeros((nk, 3, 3)), np.zeros((nk, 3, 9)), np.zeros((nk, 3))
    # a vertex's contributions: its incoming edge, then its outgoing edges in edge order
    D[G.k2] = He[:, 3:6, 3:6]
    O[G.k2] = He[:, 3:6, 0:3]
    B[G.k2] = He[:, 3:6, 6:15]
    b[G.k2] = be[:, 3:6]
    np.add.at(D, G.k1, He[:, 0:3, 0:3])
    np.add.at(B, G.k1, He[:, 0:3, 6:15])
    np.add.at(b, G.k1, be[:, 0:3])
    C = np.sum(He[:, 6:15, 6:15], axis=0)
    rc = np.sum(be[:, 6:15], axis=0)
    if G.priors:
        # the prior edges' linearizeOplus is +I on an error of (0 - bias) (S/G2oTypes.cc:971-983): b = -J^T W e = +prior * bias
        C[0:3, 0:3] += P["prior_g"] * np.eye(3)
        C[3:6, 3:6] += P["prior_a"] * np.eye(3)
        rc[0:3] += P["prior_g"] * S["bg"]
        rc[3:6] += P["prior_a"] * S["ba"]
    return {"D": D, "O": O, "B": B, "b": b, "C": C, "rc": rc, "chi": chi}


# ------------------------------------------------------------------------------------------------ the solve
def ldlt_solve(H, b, rel, decisions):
    """LDL^T without pivoting in the order of the device's lane solve; None unless every pivot is positive (rel: beyond rounding) and finite"""
    n = len(b)
    A = H.copy()
    diag0 = np.abs(np.diag(H)).copy()
    d = np.zeros(n)
    for k in range(n):
        dk = A[k, k]
        if dk != 0 or diag0[k] != 0:                      # an EXACT 0 on a zero diagonal is an outcome of its own, not a near miss
            decisions.append((dk, PIVOT_REL * diag0[k] if rel else 0.0, diag0[k] if diag0[k] > 0 else 1.0))
        if not (dk > (PIVOT_REL * diag0[k] if rel else 0.0)) or not np.isfinite(dk):
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


def _inv3_cofactors(A, decisions):
    a00, a01, a02, a11, a12, a22 = A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    # the pivots of an LDL^T of the block are a00, c22 / a00 and det / c22
    decisions.extend([(a00, 0.0, abs(a00) or 1.0), (c22, 0.0, abs(a00 * a11) or 1.0), (det, 0.0, abs(a00 * a11 * a22) or 1.0)])
    if not (a00 > 0) or not (c22 > 0) or not (det > 0) or not np.isfinite(det):
        return None
    return np.array([[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]]) / det


def solve_elimination(G, L, lam, rel, decisions, blocks_by_numpy=False):
    """formulation (b); blocks_by_numpy: every block solve through numpy.linalg (the stand-in for (a) beyond DENSE_MAX).  Returns
    (xv (nk, 3), xb (9)) or None."""
    fm = G.fm
    xv, xb = np.zeros((G.nk, 3)), np.zeros(9)
    C = L["C"][np.ix_(fm, fm)] + lam * np.eye(G.nb)
    rc = L["rc"][fm].copy()
    if G.free_v:
        D, O, B, b = L["D"].copy(), L["O"], L["B"][:, :, fm].copy(), L["b"].copy()
        M = np.zeros((G.nk, 3, 3))
        for k in G.order:
            A = D[k] + lam * np.eye(3)
            if blocks_by_numpy:
                try:
                    np.linalg.cholesky(A)
                    Mk = np.linalg.inv(A)
                except np.linalg.LinAlgError:
                    return None
            else:
                Mk = _inv3_cofactors(A, decisions)
                if Mk is None:
                    return None
            M[k] = Mk
            p = G.pred[k]
            if p >= 0:
                Gm = O[k].T @ Mk
                D[p] -= Gm @ O[k]
                B[p] -= Gm @ B[k]
                b[p] -= Gm @ b[k]
        ks = G.order
        MB = M[ks] @ B[ks]
        C = C - np.sum(np.transpose(B[ks], (0, 2, 1)) @ MB, axis=0)
        rc = rc - np.sum(np.einsum("kmi,km->ki", B[ks], np.einsum("kij,kj->ki", M[ks], b[ks])), axis=0)
    if G.nb:
        if blocks_by_numpy:
            try:
                np.linalg.cholesky(C)
                xf = np.linalg.solve(C, rc)
            except np.linalg.LinAlgError:
                return None
        else:
            xf = ldlt_solve(C, rc, rel, decisions)
            if xf is None:
                return None
        xb[fm] = xf
    if G.free_v:
        for k in G.order[::-1]:
            r = b[k] - B[k] @ xb[fm]
            p = G.pred[k]
            if p >= 0:
                r = r - O[k] @ xv[p]
            xv[k] = M[k] @ r
    return xv, xb


def solve_dense(G, L, lam):
    """formulation (a): the normal equations as one dense matrix"""
    fm = np.flatnonzero(G.fm)
    n = G.n_unknowns
    H, rhs = np.zeros((n, n)), np.zeros(n)
    nv3 = 3 * G.nv if G.free_v else 0
    slot = -np.ones(G.nk, np.int64)
    if G.free_v:
        slot[G.order] = np.arange(G.nv)
        for k in G.order:
            i = 3 * slot[k]
            H[i:i + 3, i:i + 3] = L["D"][k]
            rhs[i:i + 3] = L["b"][k]
            H[i:i + 3, nv3:] = L["B"][k][:, fm]
            H[nv3:, i:i + 3] = L["B"][k][:, fm].T
            p = G.pred[k]
            if p >= 0:
                j = 3 * slot[p]
                H[i:i + 3, j:j + 3] = L["O"][k]
                H[j:j + 3, i:i + 3] = L["O"][k].T
    H[nv3:, nv3:] = L["C"][np.ix_(fm, fm)]
    rhs[nv3:] = L["rc"][fm]
    A = H + lam * np.eye(n)
    try:
        np.linalg.cholesky(A)
        x = np.linalg.solve(A, rhs)
    except np.linalg.LinAlgError:
        return None
    if not np.all(np.isfinite(x)):
        return None
    xv, xb = np.zeros((G.nk, 3)), np.zeros(9)
    if G.free_v:
        xv[G.order] = x[:nv3].reshape(-1, 3)
    xb[fm] = x[nv3:]
    return xv, xb


def apply_step(G, S, xv, xb, variant):
    T = {"v": S["v"] + xv if G.free_v else S["v"], "bg": S["bg"].copy(), "ba": S["ba"].copy(), "Rwg": S["Rwg"], "s": S["s"]}
    if G.fm[0]:
        T["bg"] = S["bg"] + xb[0:3]
        T["ba"] = S["ba"] + xb[3:6]
    if G.fm[6]:
        T["Rwg"] = gdir_oplus(S["Rwg"], xb[6:8], variant)
    if G.fm[8]:
        T["s"] = scale_oplus(S["s"], xb[8])
    return T


def solve(P, variant="kernel", dense=False):
    """optimizer.optimize(its): g2o's Levenberg-Marquardt with ORB-SLAM3's _nBad rule (G/core/optimization_algorithm_levenberg.cpp), or
    Gauss-Newton (optimization_algorithm_gauss_newton.cpp:50-93).  dense: formulation (a)."""
    G = Graph(P)
    S = initial_state(P)
    gn = P["algorithm"] == GN
    decisions, lm_decisions, trace = [], [], []
    by_numpy = dense and G.n_unknowns > DENSE_MAX

    def lin_solve(L, lam):
        if dense and not by_numpy:
            return solve_dense(G, L, lam)
        return solve_elimination(G, L, lam, gn, decisions, by_numpy)

    lam, ni, n_bad, done, failed = 0.0, 2.0, 0, 0, 0
    amp, lambda_amp = 0.0, []
    cur = chi_first = 0.0
    for it in range(P["iterations"]):
        L = linearise(P, G, S, variant)
        cur = L["chi"]
        if it == 0:
            chi_first = cur
        ini = cur
        if gn:
            sol = lin_solve(L, 0.0)
            trace.append((0.0, cur, 1))
            lambda_amp.append(0.0)
            done += 1
            if sol is None:
                failed = 1
                break
            S = apply_step(G, S, sol[0], sol[1], variant)
            continue
        if it == 0:
            if P["lambda_init"] > 0:
                lam = float(P["lambda_init"])
            else:
                md = 0.0
                if G.free_v:
                    md = max(md, float(np.abs(np.diagonal(L["D"][G.order], axis1=1, axis2=2)).max()))
                if G.nb:
                    md = max(md, float(np.abs(np.diag(L["C"])[G.fm]).max()))
                lam = 1e-5 * md
            ni, n_bad = 2.0, 0
        qmax, rho = 0, 0.0
        while True:
            sol = lin_solve(L, lam)
            temp, scale = np.finfo(np.float64).max, 0.0
            if sol is not None:
                xv, xb = sol
                T = apply_step(G, S, xv, xb, variant)
                if G.free_v:
                    scale += float(np.sum(xv[G.order] * (lam * xv[G.order] + L["b"][G.order])))
                scale += float(np.sum(xb[G.fm] * (lam * xb[G.fm] + L["rc"][G.fm])))
                temp = evaluate(P, G, T, variant)
            rho = (cur - temp) / (scale + 1e-3)
            # the gain ratio against 0 on its natural scale 1; an EXACT 0 is an outcome of its own (it ends the run), not a near miss
            lm_decisions.append((rho if rho != 0 else 1.0, 0.0, 1.0))
            if rho > 0 and np.isfinite(temp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                if 1.0 / 3.0 < alpha < 2.0 / 3.0:
                    # between its clamps lambda's factor follows rho, a quotient of a DIFFERENCE of two chi2: a relative rounding u of a
                    # chi2 moves ln(lambda) by |d ln(alpha) / d rho| (|cur| + |temp|) / (scale + 1e-3) u, and lambda keeps it from then on
                    amp += 6.0 * (2 * rho - 1) ** 2 / alpha * (abs(cur) + abs(temp)) / abs(scale + 1e-3)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = temp
                S = T
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        done += 1
        trace.append((lam, cur, qmax))
        lambda_amp.append(amp)
        if qmax == 10 or rho == 0:
            break
        lm_decisions.append(((ini - cur) * 1e3 - ini, 0.0, ini))
        n_bad = n_bad + 1 if (ini - cur) * 1e3 < ini else 0
        if n_bad >= 3:
            break
    chi_final = cur
    if gn and not failed and done > 0:
        chi_final = evaluate(P, G, S, variant)
    v = S["v"]
    if variant == "reference":                                  # SetVelocity holds floats
        v = np.where(G.in_system[:, None] & G.free_v, v.astype(f32).astype(np.float64), v)
    return {"vwb": v, "bg": S["bg"], "ba": S["ba"], "Rwg": S["Rwg"], "scale": S["s"], "iters": done, "n_unknowns": G.n_unknowns,
            "solve_failed": failed, "chi2_first": chi_first, "chi2_final": chi_final, "trace": np.array(trace, np.float64).reshape(-1, 3),
            "decisions": decisions, "lm_decisions": lm_decisions, "lambda_amp": np.array(lambda_amp, np.float64)}


def near_threshold(decisions, rel=BAND):
    """decisions (value, threshold, scale) whose value lies within rel * scale of its threshold (tests/inertial_ba_model.py)"""
    d = np.array(decisions, np.float64).reshape(-1, 3)
    return np.abs(d[:, 0] - d[:, 1]) <= rel * np.abs(d[:, 2])


def state_vector(r):
    return np.concatenate([np.asarray(r["vwb"]).ravel(), r["bg"], r["ba"], np.asarray(r["Rwg"]).ravel(), [r["scale"]]])


def state_difference(r1, r2):
    return float(np.abs(state_vector(r1) - state_vector(r2)).max())


def yardstick_floor(rb):
    """one unit in the last place of the largest state component"""
    return EPS * max(1.0, float(np.abs(state_vector(rb)).max()))


def trace_rows_difference(r1, r2):
    """per trace row the larger relative difference of lambda and chi2; None when the lengths or the trial counts differ"""
    a, b = np.asarray(r1["trace"]), np.asarray(r2["trace"])
    if a.shape != b.shape or not np.array_equal(a[:, 2], b[:, 2]):
        return None
    if len(a) == 0:
        return np.zeros(0)
    return np.max(np.abs(a[:, :2] - b[:, :2]) / np.maximum(np.abs(b[:, :2]), 1e-300), axis=1)


def yardsticks_of(rb, ra):
    """(a) against (b): the state (floored at one unit in the last place) and the trace rows"""
    rows = trace_rows_difference(ra, rb)
    return {"ab_state": max(state_difference(ra, rb), yardstick_floor(rb)), "ab_rows": rows,
            "ab_trace": float(rows[rows <= NOISE_ROW].max()) if rows is not None and np.any(rows <= NOISE_ROW) else 0.0}


def trace_bounds(rb, ra):
    """Per trace row the bounds on the relative difference of lambda and of chi2, and the rows held absolutely instead (noise).
    chi2: max(1e-9, 10 f), f the largest (a)-against-(b) difference of a row that is not noise (the bundle adjustments' rule).
    lambda: that, plus MARGIN * lambda_amp * u -- between its clamps at 1/3 and 2/3, lambda's factor 1 - (2 rho - 1)^3 follows rho, whose
    numerator is the DIFFERENCE of two chi2: near convergence a rounding of relative size u in a chi2 is amplified by
    (|cur| + |temp|) / (scale + 1e-3), up to 1e6 in these cases, and lambda carries it through every later row.  The model's two solves
    share their chi2 arithmetic, so their lambda do not show this; lambda_amp is the model's own account of the amplification
    (solve()), u the (a)-against-(b) difference f of the chi2, no smaller than one unit in the last place."""
    rows = trace_rows_difference(ra, rb)
    assert rows is not None, "the model's two solves take different trial counts"
    noise = rows > NOISE_ROW
    f = float(rows[~noise].max()) if (~noise).any() else 0.0
    tb = max(1e-9, 10.0 * f)
    return tb + MARGIN * rb["lambda_amp"] * max(f, EPS), np.full(len(rows), tb), noise, f


# ------------------------------------------------------------------------------------------------ scenes
def form_problem(form, bMono=True, bFixedVel=False, priorG=1e2, priorA=1e6):
    """the switches of each overload (S/Optimizer.cc:5344, :5534 / :5696, :5858)"""
    if form == 1:
        return dict(algorithm=LM, iterations=200, lambda_init=1e3 if priorG != 0 else 0.0, free_velocity=not bFixedVel, free_bias=not bFixedVel,
                    free_gdir=True, free_scale=bool(bMono), with_priors=True, prior_g=float(f32(priorG)), prior_a=float(f32(priorA)))
    if form in (2, 3):
        return dict(algorithm=LM, iterations=200, lambda_init=1e3, free_velocity=True, free_bias=True, free_gdir=False, free_scale=False,
                    with_priors=True, prior_g=float(f32(priorG)), prior_a=float(f32(priorA)))
    return dict(algorithm=GN, iterations=10, lambda_init=0.0, free_velocity=False, free_bias=False, free_gdir=True, free_scale=True,
                with_priors=False, prior_g=0.0, prior_a=0.0)


_pool = {}


def _segment_pool(seed=7, count=8, steps=40):
    """a few integrated IMU segments: the bias Jacobians and the covariance an edge of the scenes borrows"""
    if (seed, count, steps) not in _pool:
        rng = np.random.default_rng(seed)
        sg, sa, sgw, saw = 1.7e-4 * np.sqrt(200), 2.0e-3 * np.sqrt(200), 1.9e-5 / np.sqrt(200), 3.0e-3 / np.sqrt(200)
        out = []
        for _ in range(count):
            omega, acc = rng.normal(0, 0.3, 3), rng.normal(0, 1.0, 3) - pim.G_VEC
            pre, Cm = pim.integrate_imu([acc] * steps, [omega] * steps, 0.005, np.zeros(3), np.zeros(3), sg, sa, sgw, saw)
            out.append((pre, pim.imu_information(Cm)[0]))
        _pool[(seed, count, steps)] = out
    return _pool[(seed, count, steps)]


def make_scene(n, seed, chains=None, isolated=(), reverse=False, degenerate=False, noise=1.0, v_perturb=0.05, s_true=1.3, bias_true=1.0,
               tilt=0.2, **switches):
    """n keyframes on a smooth metric trajectory, seen in a map frame whose gravity direction is Rwg_true gI and whose unit is s_true
    metres; the edges' deltas are the trajectory's own (plus noise) at a linearisation bias next to the true one.  chains: lists of
    keyframe indices, each a run of predecessors (default: one chain over all keyframes); a keyframe that two chains start from is a fork.
    isolated: keyframes without an edge; reverse: the keyframe list newest first.  The estimates handed in: noisy velocities, zero bias,
    a tilted gravity direction, scale 1."""
    rng = np.random.default_rng(seed)
    pool = _segment_pool()
    dT = float(pool[0][0]["dT"])
    tk = np.arange(n) * dT
    amp, om, ph = rng.uniform(0.5, 2.0, 3), rng.uniform(0.5, 1.5, 3), rng.uniform(0, 6.28, 3)
    P = dict(form_problem(1))
    P.update(switches)
    Rwg_true = pim.exp_so3(np.array([0.3, -0.2, 0.0]))
    if not P["free_gdir"] and not P["free_scale"]:                 # the second and third overload: Rwg = I, scale = 1, both fixed
        Rwg_true, s_true = np.eye(3), 1.0
    p = amp * np.sin(np.outer(tk, om) + ph)
    v = amp * om * np.cos(np.outer(tk, om) + ph)
    th = 0.4 * np.sin(np.outer(tk, rng.uniform(0.3, 0.8, 3)) + rng.uniform(0, 6.28, 3))
    R = np.stack([pim.exp_so3(t) for t in th])
    if degenerate:
        p, v = np.zeros((n, 3)), np.zeros((n, 3))
    g = Rwg_true @ GI
    bg_t, ba_t = bias_true * np.array([0.004, -0.003, 0.002]), bias_true * np.array([0.03, -0.02, 0.05])
    if chains is None:
        chains = [[k for k in range(n) if k not in set(isolated)]]
    Rf, tf_, vf = R.astype(f32), (p / s_true).astype(f32), (v / s_true).astype(f32)
    edges = []
    for ch in chains:
        for a, c in zip(ch[:-1], ch[1:]):
            pre0, info9 = pool[rng.integers(len(pool))]
            pre = {k: np.array(x) for k, x in pre0.items()}
            dt = (c - a) * dT
            R1 = Rf[a].astype(np.float64)
            dR = R1.T @ Rf[c].astype(np.float64)
            dV = R1.T @ (v[c] - v[a] - g * dt)
            dP = R1.T @ (p[c] - p[a] - v[a] * dt - g * dt * dt / 2)
            lbg, lba = bg_t + rng.normal(0, 2e-4, 3), ba_t + rng.normal(0, 2e-3, 3)
            dbg, dba = bg_t - lbg, ba_t - lba
            D = lambda k: pre0[k].astype(np.float64)
            pre["dT"] = f32(dt)
            pre["dR"] = (dR @ pim.exp_so3(-D("JRg") @ dbg + noise * rng.normal(0, 1e-4, 3))).astype(f32)
            pre["dV"] = (dV - D("JVg") @ dbg - D("JVa") @ dba + noise * rng.normal(0, 2e-3, 3)).astype(f32)
            pre["dP"] = (dP - D("JPg") @ dbg - D("JPa") @ dba + noise * rng.normal(0, 2e-4, 3)).astype(f32)
            pre["bg"], pre["ba"] = lbg.astype(f32), lba.astype(f32)
            edges.append({"k1": a, "k2": c, "preint": pre, "info9": info9})
    if degenerate:
        vh = np.zeros((n, 3), f32)
    else:
        vh = (vf.astype(np.float64) + rng.normal(0, v_perturb, (n, 3))).astype(f32)
    if reverse:
        Rf, tf_, vh = Rf[::-1].copy(), tf_[::-1].copy(), vh[::-1].copy()
        for e in edges:
            e["k1"], e["k2"] = n - 1 - e["k1"], n - 1 - e["k2"]
    P.update({"keyframes": {"R": Rf, "t": tf_, "v": vh}, "edges": edges, "bg": np.zeros(3, f32), "ba": np.zeros(3, f32),
              "Rwg": Rwg_true @ pim.exp_so3(np.array([tilt, -tilt / 2, 0.0])), "scale": 1.0,
              "truth": {"Rwg": Rwg_true, "s": s_true, "bg": bg_t, "ba": ba_t, "v": v / s_true}})
    if not P["free_gdir"] and not P["free_scale"]:
        P["Rwg"], P["scale"] = np.eye(3), 1.0
    return finish(P)


def finish(P):
    """the per-edge arrays the vectorised evaluation reads"""
    E = P["edges"]
    P["_dt"] = np.array([float(e["preint"]["dT"]) for e in E])
    for k in ("JVg", "JPg", "JVa", "JPa"):
        P["_" + k] = np.stack([e["preint"][k].astype(np.float64) for e in E]) if E else np.zeros((0, 3, 3))
    return P


def kernel_constant(name):
    """a constexpr int of csrc/inertial_init.hip, read from the source"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multi_orbslam3_amd", "csrc", "inertial_init.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


TILE = kernel_constant("kIiTile")
CAP = 4096

# name -> make_scene arguments.  The large cases run 3 iterations.
CASES = {
    "n2": dict(n=2, seed=1, **dict(form_problem(1, bMono=True), iterations=2)),
    "n10_mono": dict(n=10, seed=2, **form_problem(1, bMono=True)),
    "n10_stereo": dict(n=10, seed=303, s_true=1.0, **form_problem(1, bMono=False)),
    "n10_auto_lambda": dict(n=10, seed=204, **form_problem(1, bMono=True, priorG=0.0)),
    "n10_fixed_vel": dict(n=10, seed=5, v_perturb=0.0, **form_problem(1, bMono=True, bFixedVel=True)),
    "n10_bias": dict(n=10, seed=1506, **dict(form_problem(2), iterations=3)),
    "n10_gn": dict(n=10, seed=7, v_perturb=0.0, **form_problem(4)),
    "gn_degenerate": dict(n=10, seed=8, degenerate=True, **form_problem(4)),
    "newest_first": dict(n=12, seed=209, reverse=True, **form_problem(1, bMono=True)),
    "broken": dict(n=14, seed=210, chains=[[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11, 12, 13]], **form_problem(1, bMono=True)),
    "isolated": dict(n=12, seed=11, isolated=(4,), chains=[[0, 1, 2, 3], [5, 6, 7, 8, 9, 10, 11]], **form_problem(1, bMono=True)),
    "fork": dict(n=12, seed=112, chains=[[0, 1, 2, 3, 4, 5, 6], [3, 7, 8, 9, 10, 11]], **form_problem(1, bMono=True)),
    "rejected": dict(n=10, seed=2213, tilt=0.6, **dict(form_problem(1, bMono=True, priorG=0.0), lambda_init=1e-6)),
    "nbad_stop": dict(n=16, seed=1314, **form_problem(1, bMono=True)),
    "runs_out": dict(n=10, seed=115, **dict(form_problem(1, bMono=True), iterations=4)),
}
for _d in (-1, 0, 1):
    CASES["edges%d" % (64 + _d)] = dict(n=65 + _d, seed=20 + _d, **dict(form_problem(1, bMono=True), iterations=3))
    CASES["edges%d" % (256 + _d)] = dict(n=257 + _d, seed=30 + _d, **dict(form_problem(1, bMono=True), iterations=3))
    CASES["tile%+d" % _d] = dict(n=TILE + _d, seed=40 + _d, **dict(form_problem(1, bMono=True), iterations=3))
# the cap: velocities, gravity direction and scale free, the biases fixed -- the bias-dependent part of every edge is then computed once,
# which keeps the model's share of the test short
CASES["cap"] = dict(n=CAP, seed=50, **dict(form_problem(1, bMono=True), iterations=3, free_bias=False))
# cases whose LM decisions are compared outright by the GPU test: all of them
COMPARED = list(CASES)

_memo = {}


def build_case(name):
    return make_scene(**CASES[name])


def case_results(name):
    """The problem and the model runs of a case, computed once: (b) in kernel arithmetic, (a), (b) in reference arithmetic."""
    if name not in _memo:
        P = build_case(name)
        _memo[name] = (P, solve(P, "kernel"), solve(P, "kernel", dense=True), solve(P, "reference"))
    return _memo[name]


def to_c_problem(P, device=0):
    """The views.inertial_init_problem of a model problem: (problem, keep-alive)."""
    from multi_orbslam3_amd import _capi as capi, views
    K = P["keyframes"]
    n = len(K["v"])
    Ka = np.zeros((n, capi.INERTIAL_INIT_STATE_FLOATS), f32)
    Ka[:, 0:9] = K["R"].reshape(n, 9)
    Ka[:, 9:12] = K["t"]
    Ka[:, 12:15] = K["v"]
    E = np.zeros(len(P["edges"]), capi.INERTIAL_INIT_EDGE_DTYPE)
    for i, e in enumerate(P["edges"]):
        E[i]["k1"], E[i]["k2"] = e["k1"], e["k2"]
        E[i]["dT"] = e["preint"]["dT"]
        for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bg", "ba"):
            E[i][k] = np.asarray(e["preint"][k], f32).reshape(-1)
        E[i]["info9"] = np.asarray(e["info9"], np.float64).reshape(81)
    return views.inertial_init_problem(Ka, E, P["bg"], P["ba"], P["Rwg"], P["scale"], algorithm=P["algorithm"], iterations=P["iterations"],
                                       lambda_init=P["lambda_init"], free_velocity=P["free_velocity"], free_bias=P["free_bias"],
                                       free_gdir=P["free_gdir"], free_scale=P["free_scale"], with_priors=P["with_priors"],
                                       prior_g=P["prior_g"], prior_a=P["prior_a"], device=device)
