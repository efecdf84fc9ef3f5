"""Checker for OptimizeEssentialGraph: a numpy restatement of the numerical core of Optimizer::OptimizeEssentialGraph
(S/Optimizer.cc:2413-2747) and of what it runs inside g2o, vectorised over the edges and parametrised by dtype.

dtype = float64 follows the reference; dtype = numpy.longdouble (80-bit where LONGDOUBLE_OK) evaluates the same statements with 11
more bits and is the yardstick for how much of a float64 result is rounding (through the 1 / (2e-9) of the numeric Jacobian that is
a lot more than an ulp).

Restated, with the lines they come from:
  Sim3(Vector7d), operator*, inverse, map              G/types/sim3.h:70-142, 266-272, 233-236, 144-146 (tests/sim3_opt_model.py)
  Sim3::log, all four branches, W.lu().solve(t)        G/types/sim3.h:148-230
  VertexSim3Expmap::oplusImpl                          G/types/types_seven_dof_expmap.h:60-69
  EdgeSim3::computeError                               G/types/types_seven_dof_expmap.h:106-114
  numeric Jacobian                                     G/core/base_binary_edge.hpp:131-205
  constructQuadraticForm (information = I, no kernel)  G/core/base_binary_edge.hpp:55-120
  the Levenberg-Marquardt driver                       G/core/optimization_algorithm_levenberg.cpp:61-194, sparse_optimizer.cpp:354-419
  vertex and edge collection of the loop form          S/Optimizer.cc:2446-2483, 2492-2523, 2530-2666
  the map points                                       S/Optimizer.cc:2710-2743

The linear solve is the one thing NOT restated operation by operation: float64 takes LAPACK's Cholesky factorisation, long double
refines that solution with long double residuals until the correction vanishes.  A factorisation that fails is a rejected trial.

Nothing here is used by the product; the product is compared WITH it.
"""
import functools

import numpy as np
import scipy.linalg

import sim3_opt_model as om
from sim3_opt_model import L, LONGDOUBLE_OK, quat_rotate, sim3_exp, sim3_inverse, sim3_map, sim3_mul  # noqa: F401

DELTA = 1e-9
ITERATIONS, LAMBDA_INIT = 20, 1e-16


# ------------------------------------------------------------------ Sim3::log

def quat_to_R(q):
    """E-10: Quaterniond::toRotationMatrix() as Eigen writes it (tx = 2 x, twx = tx w, ...)."""
    tx, ty, tz = 2 * q[0], 2 * q[1], 2 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def _swap(m, a, b):
    """rows a and b of the row lists where mask m holds"""
    for j in range(len(a)):
        a[j], b[j] = np.where(m, b[j], a[j]), np.where(m, a[j], b[j])


def lu_solve3(W, t):
    """E-11: Matrix3d::lu().solve(): partial pivoting (largest |entry| of the column, the first one on a tie), unit lower factor, forward
    then backward substitution.  W: 3 x 3 lists of arrays, t: 3 arrays."""
    r0, r1, r2 = [list(W[i]) + [t[i]] for i in range(3)]
    a0, a1, a2 = abs(r0[0]), abs(r1[0]), abs(r2[0])
    m1 = (a1 > a0) & (a1 >= a2)
    m2 = ~m1 & (a2 > a0) & (a2 > a1)
    _swap(m1, r0, r1)
    _swap(m2, r0, r2)
    l10, l20 = r1[0] / r0[0], r2[0] / r0[0]
    r1[1], r1[2] = r1[1] - l10 * r0[1], r1[2] - l10 * r0[2]
    r2[1], r2[2] = r2[1] - l20 * r0[1], r2[2] - l20 * r0[2]
    y0 = r0[3]
    rows1, rows2 = [r1[1], r1[2], r1[3], l10], [r2[1], r2[2], r2[3], l20]
    _swap(abs(rows2[0]) > abs(rows1[0]), rows1, rows2)
    l21 = rows2[0] / rows1[0]
    u22 = rows2[1] - l21 * rows1[1]
    y1 = rows1[2] - rows1[3] * y0
    y2 = rows2[2] - rows2[3] * y0 - l21 * y1
    x2 = y2 / u22
    x1 = (y1 - rows1[1] * x2) / rows1[0]
    x0 = (y0 - r0[1] * x1 - r0[2] * x2) / r0[0]
    return [x0, x1, x2]


def sim3_log(a, F):
    """Sim3::log(), sim3.h:148-230.  a = (q, t, s) of scalars or arrays of dtype F -> seven arrays.  Both sides of every branch are
    evaluated and the branch's own value selected, element by element."""
    q, t, s = [np.asarray(v, F) for v in a[0]], [np.asarray(v, F) for v in a[1]], np.asarray(a[2], F)
    with np.errstate(all="ignore"):
        sigma = np.log(s)
        R = quat_to_R(q)
        d = F(0.5) * (R[0][0] + R[1][1] + R[2][2] - 1)
        dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
        eps = F(0.00001)
        small_s, small_r = abs(sigma) < eps, d > 1 - eps
        theta = np.arccos(d)
        theta2 = theta * theta
        sigma2 = sigma * sigma
        k = np.where(small_r, F(0.5), theta / (2 * np.sqrt(1 - d * d)))
        C = np.where(small_s, F(1), (s - 1) / sigma)
        sa, sb = s * np.sin(theta), s * np.cos(theta)
        c = theta2 + sigma * sigma
        A = np.where(small_s,
                     np.where(small_r, F(1.) / F(2.), (1 - np.cos(theta)) / theta2),
                     np.where(small_r, ((sigma - 1) * s + 1) / sigma2, (sa * sigma + (1 - sb) * theta) / (theta * c)))
        B = np.where(small_s,
                     np.where(small_r, F(1.) / F(6.), (theta - np.sin(theta)) / (theta2 * theta)),
                     np.where(small_r, ((F(0.5) * sigma2 - sigma + 1) * s) / (sigma2 * sigma), (C - ((sb - 1) * sigma + sa * theta) / c) * F(1.) / theta2))
        om_ = [k * dR[0], k * dR[1], k * dR[2]]
        z = np.zeros_like(d)
        O = [[z, -om_[2], om_[1]], [om_[2], z, -om_[0]], [-om_[1], om_[0], z]]
        W = [[A * O[i][j] + B * (O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j]) + C * (F(1) if i == j else F(0)) for j in range(3)]
             for i in range(3)]
        ups = lu_solve3(W, t)
    return om_ + ups + [sigma]


# ------------------------------------------------------------------ the flat problem (eg_problem)

class Problem:
    """vertices: q (V, 4), t (V, 3), s (V,) float64, fixed / fix_scale (V,) bool; edges: vi / vj (E,) int, mq (E, 4), mt (E, 3), ms (E,);
    points: pos (P, 3) float32, ref (P,) int."""

    def __init__(self, q, t, s, fixed, fix_scale, vi, vj, mq, mt, ms, pos=None, ref=None):
        f = np.float64
        self.q, self.t, self.s = np.array(q, f).reshape(-1, 4), np.array(t, f).reshape(-1, 3), np.array(s, f).reshape(-1)
        self.fixed, self.fix_scale = np.array(fixed, bool).reshape(-1), np.array(fix_scale, bool).reshape(-1)
        self.vi, self.vj = np.array(vi, np.int64).reshape(-1), np.array(vj, np.int64).reshape(-1)
        self.mq, self.mt, self.ms = np.array(mq, f).reshape(-1, 4), np.array(mt, f).reshape(-1, 3), np.array(ms, f).reshape(-1)
        self.pos = np.zeros((0, 3), np.float32) if pos is None else np.array(pos, np.float32).reshape(-1, 3)
        self.ref = np.zeros(0, np.int64) if ref is None else np.array(ref, np.int64).reshape(-1)

    @property
    def n_free(self):
        return int((~self.fixed).sum())


def _s3(q, t, s, F):
    q, t = np.asarray(q, F), np.asarray(t, F)
    return ([q[..., i] for i in range(4)], [t[..., i] for i in range(3)], np.asarray(s, F))


def _take(S, idx):
    return ([c[idx] for c in S[0]], [c[idx] for c in S[1]], S[2][idx])


def edge_errors(C, Si, Sj, F):
    """EdgeSim3::computeError: log((C * v1) * v2^-1) -> (E, 7)"""
    return np.stack(sim3_log(sim3_mul(sim3_mul(C, Si), sim3_inverse(Sj)), F), axis=-1)


def _perturbed(est, d, sign, fix_scale, F):
    """oplusImpl of every vertex with update = sign * delta * e_d (update[6] zeroed under _fix_scale)"""
    u = [F(0)] * 7
    u[d] = F(sign * DELTA)
    out = sim3_mul(sim3_exp(u, F), est)
    if d == 6 and fix_scale.any():
        alt = sim3_mul(sim3_exp([F(0)] * 7, F), est)
        out = ([np.where(fix_scale, a, b) for a, b in zip(alt[0], out[0])], [np.where(fix_scale, a, b) for a, b in zip(alt[1], out[1])],
               np.where(fix_scale, alt[2], out[2]))
    return out


def linearise(p, est, C, F):
    """-> e (E, 7), Ji, Jj (E, 7, 7) [error row, update column]; a fixed vertex gets no Jacobian"""
    Si, Sj = _take(est, p.vi), _take(est, p.vj)
    e = edge_errors(C, Si, Sj, F)
    E = len(p.vi)
    J = [np.zeros((E, 7, 7), F), np.zeros((E, 7, 7), F)]
    scalar = F(1.0) / (F(2) * F(DELTA))
    for side in (0, 1):
        free = ~p.fixed[p.vj if side else p.vi]
        for d in range(7):
            ev = []
            for sign in (1, -1):
                pe = _take(_perturbed(est, d, sign, p.fix_scale, F), p.vj if side else p.vi)
                ev.append(edge_errors(C, Si, pe, F) if side else edge_errors(C, pe, Sj, F))
            J[side][:, :, d] = np.where(free[:, None], scalar * (ev[0] - ev[1]), F(0))
    return e, J[0], J[1]


def normal_equations(p, e, Ji, Jj, F):
    """H (7F x 7F, free vertices in ascending order) and b, summed in edge order"""
    col = np.full(len(p.fixed), -1)
    col[~p.fixed] = np.arange(p.n_free)
    n = 7 * p.n_free
    H, b = np.zeros((n, n), F), np.zeros(n, F)
    JiT, JjT = np.transpose(Ji, (0, 2, 1)), np.transpose(Jj, (0, 2, 1))
    Hii, Hij, Hjj = np.matmul(JiT, Ji), np.matmul(JiT, Jj), np.matmul(JjT, Jj)
    bi, bj = np.matmul(JiT, -e[:, :, None])[:, :, 0], np.matmul(JjT, -e[:, :, None])[:, :, 0]
    for k in range(len(p.vi)):
        ci, cj = col[p.vi[k]], col[p.vj[k]]
        if ci >= 0:
            H[7 * ci:7 * ci + 7, 7 * ci:7 * ci + 7] += Hii[k]
            b[7 * ci:7 * ci + 7] += bi[k]
        if cj >= 0:
            H[7 * cj:7 * cj + 7, 7 * cj:7 * cj + 7] += Hjj[k]
            b[7 * cj:7 * cj + 7] += bj[k]
        if ci >= 0 and cj >= 0:
            H[7 * ci:7 * ci + 7, 7 * cj:7 * cj + 7] += Hij[k]
            H[7 * cj:7 * cj + 7, 7 * ci:7 * ci + 7] += Hij[k].T
    return H, b, col


def solve_spd(A, b, F):
    """-> (x, ok).  float64: Cholesky; long double: the float64 solution refined with long double residuals."""
    A64 = A.astype(np.float64)
    try:
        with np.errstate(all="ignore"):
            cf = scipy.linalg.cho_factor(A64, lower=True, check_finite=False)
        if not np.all(np.isfinite(cf[0])):
            return np.zeros_like(b), False
    except np.linalg.LinAlgError:
        return np.zeros_like(b), False
    x = scipy.linalg.cho_solve(cf, b.astype(np.float64), check_finite=False).astype(F)
    if F is np.float64:
        return x, True
    for _ in range(12):
        r = b - A @ x
        dx = scipy.linalg.cho_solve(cf, r.astype(np.float64), check_finite=False).astype(F)
        x = x + dx
        if np.abs(dx).max() <= 1e-21 * max(np.abs(x).max(), 1e-300):
            break
    return x, True


def run(p, F=np.float64, iterations=ITERATIONS, lambda_init=LAMBDA_INIT):
    """-> dict(est = (V, 8) of dtype F, points (P, 3) float32, err0, errEnd, iters, trace = [(trials, accepted, chi2, lambda)],
    edge_error0 (E, 7))"""
    est = _s3(p.q, p.t, p.s, F)
    est0 = est
    C = _s3(p.mq, p.mt, p.ms, F)
    V, E = len(p.s), len(p.vi)
    out = dict(iters=0, trace=[], err0=F(0), errEnd=F(0), edge_error0=np.zeros((E, 7), F))
    if E > 0:
        e = edge_errors(C, _take(est, p.vi), _take(est, p.vj), F)
        out["edge_error0"] = e
        out["err0"] = out["errEnd"] = (e * e).sum(axis=1).sum()
    if p.n_free > 0 and E > 0 and iterations > 0:
        lam, ni, n_bad, ok = F(0), F(2), 0, True
        for it in range(iterations):
            if not ok:
                break
            e, Ji, Jj = linearise(p, est, C, F)
            H, b, col = normal_equations(p, e, Ji, Jj, F)
            cur = (e * e).sum(axis=1).sum()
            if it == 0:
                lam = F(lambda_init) if lambda_init > 0 else F(1e-5) * np.abs(np.diag(H)).max()
                ni, n_bad = F(2), 0
                out["err0"] = cur
            ini, rho, qmax, accepted = cur, F(0), 0, False
            while True:
                x, sok = solve_spd(H + lam * np.eye(len(b), dtype=F), b, F)
                trial = est
                if sok:
                    xs = np.zeros((V, 7), F)
                    xs[~p.fixed] = x.reshape(-1, 7)
                    xs[p.fix_scale, 6] = 0
                    rows = []
                    for v in range(V):
                        rows.append(sim3_mul(sim3_exp(list(xs[v]), F), _take(est, v)) if not p.fixed[v] else _take(est, v))
                    trial = ([np.array([r[0][i] for r in rows], F) for i in range(4)], [np.array([r[1][i] for r in rows], F) for i in range(3)],
                             np.array([r[2] for r in rows], F))
                te = edge_errors(C, _take(trial, p.vi), _take(trial, p.vj), F)
                tchi = (te * te).sum(axis=1).sum() if sok else F(np.finfo(np.float64).max)
                scale = (x * (lam * x + b)).sum() + F(1e-3)
                rho = (cur - tchi) / scale
                accepted = bool(rho > 0 and np.isfinite(tchi))
                if accepted:
                    c3 = 2 * rho - 1
                    alpha = min(1 - c3 * c3 * c3, F(2.) / F(3.))
                    lam = lam * max(F(1.) / F(3.), alpha)
                    ni = F(2)
                    cur = tchi
                    est = trial
                else:
                    lam = lam * ni
                    ni = ni * 2
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            out["iters"] += 1
            out["errEnd"] = cur
            out["trace"].append((qmax, int(accepted), cur, lam))
            if qmax == 10 or rho == 0:
                ok = False
            else:
                n_bad = n_bad + 1 if (ini - cur) * 1e3 < ini else 0
                ok = n_bad < 3
    out["est"] = np.concatenate([np.stack(est[0], -1), np.stack(est[1], -1), np.asarray(est[2])[:, None]], axis=1) if V else np.zeros((0, 8), F)
    pts = np.array(p.pos, np.float32)
    m = p.ref >= 0
    if m.any():
        r = p.ref[m]
        X = [p.pos[m, i].astype(F) for i in range(3)]
        Y = sim3_map(sim3_inverse(_take(est, r)), sim3_map(_take(est0, r), X))
        pts[m] = np.stack(Y, -1).astype(np.float32)
    out["points"] = pts
    return out


def trace_key(res):
    """what two runs must share to count as the same LM history: trials and the verdict of the last trial, per iteration"""
    return [(int(t[0]), int(t[1])) for t in res["trace"]]


def est_diff(a, b):
    """largest |difference| over q (up to sign), t relative to the largest |t|, s"""
    a, b = np.asarray(a, L), np.asarray(b, L)
    if len(a) == 0:
        return 0.0
    dq = np.minimum(np.abs(a[:, :4] - b[:, :4]).max(axis=1), np.abs(a[:, :4] + b[:, :4]).max(axis=1)).max()
    tn = max(float(np.abs(b[:, 4:7]).max()), 1.0)
    return float(max(dq, np.abs(a[:, 4:7] - b[:, 4:7]).max() / tn, np.abs(a[:, 7] - b[:, 7]).max()))


# ------------------------------------------------------------------ the loop form's collection (S/Optimizer.cc:2446-2666)

def _f64(S):
    return ([np.float64(v) for v in S[0]], [np.float64(v) for v in S[1]], np.float64(S[2]))


def sim3_from_pose(R, t):
    """g2o::Sim3(Rcw, tcw, 1.0) from the keyframe's float32 pose: Quaterniond(Matrix3d), E-1, not renormalised"""
    R64 = [[np.float64(np.float32(R[i][j])) for j in range(3)] for i in range(3)]
    return (om.quat_from_R(R64, np.float64), [np.float64(np.float32(v)) for v in t], np.float64(1.0))


MIN_FEAT = 100


def collect_loop_form(sc):
    """sc: a scene dict (make_scene).  -> dict(uids, vertices [(q, t, s, fixed, fix_scale)], edges [(vi, vj, q, t, s)], points
    [(pos, ref)], dropped_edges, kinds) with vertices in ascending mnUniqueId and edges in the reference's order.  A bad keyframe has
    no vertex (:2449); where the reference would dereference its null vertex (:2513, :2566, :2694) the edge is dropped and counted."""
    kfs = sc["kfs"]
    good = sorted((k["uid"], i) for i, k in enumerate(kfs) if not k["bad"])
    index_of = {i: n for n, (_, i) in enumerate(good)}
    vScw = {}
    vertices = []
    for _, i in good:
        k = kfs[i]
        S = _f64(sc["corrected"][i]) if i in sc["corrected"] else sim3_from_pose(k["R"], k["t"])
        vScw[i] = S
        vertices.append((S[0], S[1], S[2], k["mnId"] == sc["init_kf_id"], sc["fix_scale"]))
    ident = ([np.float64(0)] * 3 + [np.float64(1)], [np.float64(0)] * 3, np.float64(1))
    scw = lambda i: vScw.get(i, ident)
    non = lambda i: _f64(sc["noncorrected"][i]) if i in sc["noncorrected"] else scw(i)
    edges, kinds, dropped = [], [], 0
    inserted = set()

    def add(i, j, Sji, kind):
        nonlocal dropped
        if i not in index_of or j not in index_of:
            dropped += 1
            return
        edges.append((index_of[i], index_of[j], Sji[0], Sji[1], Sji[2]))
        kinds.append(kind)

    for i, conns in sorted(sc["loop_connections"].items()):
        Swi = sim3_inverse(scw(i))
        for j in sorted(conns):
            if (i != sc["cur"] or j != sc["loop"]) and sc["weight"](i, j) < MIN_FEAT:
                continue
            add(i, j, sim3_mul(scw(j), Swi), "loop_connection")
            inserted.add((min(kfs[i]["uid"], kfs[j]["uid"]), max(kfs[i]["uid"], kfs[j]["uid"])))
    for i, k in enumerate(kfs):
        Swi = sim3_inverse(non(i))
        par = k["parent"]
        if par is not None:
            add(i, par, sim3_mul(non(par), Swi), "spanning_tree")
        for l in sorted(k["loop_edges"]):
            if kfs[l]["uid"] < k["uid"]:
                add(i, l, sim3_mul(non(l), Swi), "loop_edge")
        for n, w in k["covis"]:
            if w < MIN_FEAT:
                continue
            if n != par and n not in k["children"] and n not in k["loop_edges"]:
                if not kfs[n]["bad"] and kfs[n]["uid"] < k["uid"]:
                    if (min(k["uid"], kfs[n]["uid"]), max(k["uid"], kfs[n]["uid"])) in inserted:
                        continue
                    add(i, n, sim3_mul(non(n), Swi), "covisibility")
    points = []
    for mp in sc["points"]:
        if mp["bad"]:
            continue
        r = mp["corrected_ref"] if mp["corrected_by"] == kfs[sc["cur"]]["uid"] else kfs[mp["ref_kf"]]["uid"]
        by_uid = {kfs[i]["uid"]: n for i, n in index_of.items()}
        points.append((mp["pos"], by_uid.get(r, -1)))
    return dict(uids=[u for u, _ in good], vertices=vertices, edges=edges, points=points, dropped_edges=dropped, kinds=kinds)


def flat_problem(col):
    v, e, pt = col["vertices"], col["edges"], col["points"]
    return Problem([a[0] for a in v], [a[1] for a in v], [a[2] for a in v], [a[3] for a in v], [a[4] for a in v],
                   [a[0] for a in e], [a[1] for a in e], [a[2] for a in e], [a[3] for a in e], [a[4] for a in e],
                   [a[0] for a in pt], [a[1] for a in pt])


# ------------------------------------------------------------------ the scene family

def _rot(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def make_scene(n_kf, fix_scale, seed, k_covis=3, n_corrected=3, n_points=40, drift=1.0, bad=(), old_loops=True):
    """A keyframe ring with accumulated drift: n_kf keyframes on a circle looking inwards, the estimate of keyframe i is the truth
    composed with i steps of a small random rotation / translation error (and a scale error when the scale is free, as a monocular
    map drifts).  Chain spanning tree, covisibility edges to the k previous keyframes (weights above and below minFeat), old loop
    edges, and one loop closure between the last keyframe and keyframe 0 whose last few keyframes carry CorrectedSim3."""
    rng = np.random.default_rng(seed)
    f = np.float32
    Twc_true = []
    for i in range(n_kf):
        a = 2 * np.pi * i / n_kf * (1 - 1.0 / n_kf)
        c = np.array([5 * np.cos(a), 5 * np.sin(a), 0.3 * np.sin(3 * a)])
        R = _rot([0, 0, 1], a + np.pi) @ _rot([1, 0, 0], 0.1 * np.sin(a))
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = c
        Twc_true.append(T)
    # drifted estimates: relative motions with an error, chained
    est = [Twc_true[0].copy()]
    scale = [1.0]
    for i in range(1, n_kf):
        rel = np.linalg.inv(Twc_true[i - 1]) @ Twc_true[i]
        err = np.eye(4)
        err[:3, :3] = _rot(rng.normal(size=3), drift * 0.004 * rng.normal())
        err[:3, 3] = drift * 0.01 * rng.normal(size=3)
        s = scale[-1] * (1.0 if fix_scale else float(np.exp(drift * 0.004 * rng.normal())))
        rel[:3, 3] *= s
        est.append(est[-1] @ rel @ err)
        scale.append(s)
    kfs = []
    for i in range(n_kf):
        Tcw = np.linalg.inv(est[i])
        kfs.append(dict(mnId=i, uid=i, bad=i in bad, R=Tcw[:3, :3].astype(f), t=Tcw[:3, 3].astype(f), parent=i - 1 if i > 0 else None,
                        children={i + 1} if i + 1 < n_kf else set(), loop_edges=set(), covis=[]))
    weights = {}
    for i in range(n_kf):
        for d in range(1, k_covis + 1):
            if i - d >= 0:
                w = int(rng.integers(60, 300)) if d > 1 else int(rng.integers(150, 400))
                weights[(i - d, i)] = w
    cur, loop = n_kf - 1, 0
    weights[(loop, cur)] = 40                                  # the closing pair is taken whatever its weight (:2506)
    if n_kf > 6:
        weights[(1, cur)] = 120
        weights[(2, cur)] = 70                                 # below minFeat: left out
    if old_loops and n_kf >= 12:
        a, b = n_kf // 3, n_kf // 3 + n_kf // 2
        kfs[a]["loop_edges"].add(b); kfs[b]["loop_edges"].add(a)
        weights[(a, b)] = 130
    for (a, b), w in weights.items():
        kfs[a]["covis"].append((b, w)); kfs[b]["covis"].append((a, w))
    for k in kfs:
        k["covis"].sort(key=lambda e: (-e[1], e[0]))
    weight = lambda i, j: weights.get((min(i, j), max(i, j)), 0)
    # the loop closure: the last keyframes are moved onto the pose the closing Sim3 gives them
    Scorr_w = np.linalg.inv(Twc_true[cur]) @ np.eye(4)         # corrected world-to-camera of the current keyframe: the truth
    s_corr = 1.0 if fix_scale else scale[cur]               # the unit of the map around the current keyframe, in units of the map at keyframe 0
    corrected, noncorrected = {}, {}
    Tcw_cur = np.linalg.inv(est[cur])
    for i in range(max(1, n_kf - n_corrected), n_kf):
        if kfs[i]["bad"]:
            continue
        Tcw_i = np.linalg.inv(est[i])
        Tic = Tcw_i @ np.linalg.inv(Tcw_cur)                   # SE3 from the current keyframe to keyframe i
        q_n, t_n, _ = sim3_from_pose(Tcw_i[:3, :3].astype(f), Tcw_i[:3, 3].astype(f))
        noncorrected[i] = (q_n, t_n, np.float64(1.0))
        Rc = Tic[:3, :3] @ Scorr_w[:3, :3]
        tc = Tic[:3, :3] @ (Scorr_w[:3, 3] * s_corr) + Tic[:3, 3]     # g2oSic * g2oCorrectedScw
        corrected[i] = (om.quat_from_R([[np.float64(v) for v in row] for row in Rc], np.float64), [np.float64(v) for v in tc], np.float64(s_corr))
    loop_connections = {cur: {loop, 1, 2} if n_kf > 6 else {loop}}
    if n_kf > 8:
        loop_connections[cur - 1] = {1}
        weights[(1, cur - 1)] = 110
        kfs[1]["covis"].append((cur - 1, 110)); kfs[cur - 1]["covis"].append((1, 110))
        for k in (kfs[1], kfs[cur - 1]):
            k["covis"].sort(key=lambda e: (-e[1], e[0]))
    points = []
    for j in range(n_points):
        r = int(rng.integers(0, n_kf))
        pc = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 6)])
        pw = (est[r] @ np.append(pc, 1.0))[:3]
        by_cur = j % 7 == 0 and corrected
        points.append(dict(bad=j % 11 == 5, pos=pw.astype(f), ref_kf=r, corrected_by=kfs[cur]["uid"] if by_cur else -1,
                           corrected_ref=kfs[sorted(corrected)[0]]["uid"] if by_cur else -1))
    return dict(kfs=kfs, corrected=corrected, noncorrected=noncorrected, loop_connections=loop_connections, weight=weight, cur=cur, loop=loop,
                init_kf_id=0, fix_scale=bool(fix_scale), points=points)


# (keyframes, seeds): the bands are the solver sizes -- one workgroup, eight workgroups, many -- by free keyframes
FAMILY = [(6, (11, 12, 13)), (12, (21, 22, 23)), (18, (35,)), (19, (31, 32)), (20, (41, 42)), (32, (51, 52)), (43, (55,)), (44, (61, 62)), (45, (71,)), (70, (81,)),
          (121, (91,))]
BANDS = [(1, 17), (18, 42), (43, 1170)]
# the drift per keyframe, in units of 0.004 rad / 0.01 m / 0.4 % of scale: large enough that the last accepted steps of a run still lower
# chi2 by more than the noise of its evaluation (with a small drift the verdict on those steps is a coin toss in either precision)
FAMILY_DRIFT = 16.0


def band_of(n_free):
    return next(b for b in BANDS if b[0] <= n_free <= b[1])


def family_entries():
    return [(n, fs, seed) for n, seeds in FAMILY for seed in seeds for fs in (True, False)]


@functools.lru_cache(maxsize=None)
def measure_family():
    """Every scene of the family in float64 and in long double.  -> dict(scenes = [dict(entry, problem, f64, ld, same_trace, d_est,
    d_pts, band)], band_est / band_pts = {(band, fix_scale): largest difference over the scenes whose traces agree})"""
    scenes, band_est, band_pts = [], {}, {}
    for n, fs, seed in family_entries():
        p = flat_problem(collect_loop_form(make_scene(n, fs, seed, drift=FAMILY_DRIFT)))
        a, b = run(p, np.float64), run(p, L)
        same = trace_key(a) == trace_key(b)
        key = (band_of(p.n_free), fs)
        d_est = est_diff(a["est"], b["est"])
        m = p.ref >= 0
        d_pts = float(np.abs(a["points"][m].astype(np.float64) - b["points"][m].astype(np.float64)).max()) if m.any() else 0.0
        if same:
            band_est[key] = max(band_est.get(key, 0.0), d_est)
            band_pts[key] = max(band_pts.get(key, 0.0), d_pts)
        scenes.append(dict(entry=(n, fs, seed), problem=p, f64=a, ld=b, same_trace=same, d_est=d_est, d_pts=d_pts, band=key))
    return dict(scenes=scenes, band_est=band_est, band_pts=band_pts)


# ------------------------------------------------------------------ the cap, against a model that stays cheap
# K disjoint copies of one component: chi2 is K times the component's and lambda starts at the user's 1e-16 whatever the size.  The
# gain ratio of a trial is K dchi2 / (K (scale) + 1e-3) against dchi2 / (scale + 1e-3): the same sign, so the same verdicts; its size
# only sets the factor on a lambda that stays far below the rounding of the diagonal it is added to (and is alone only on a
# fixed-scale diagonal, whose right-hand side is exactly 0).  The trajectory of every copy is the component's.

RING_FREE = 13
# name -> copies: 90 x 13 = 1170 = EG_MAX_FREE_KEYFRAMES (8190 unknowns); 80 x 13 = 1040 (past 1024, below the cap)
RING_COPIES = {"cap1170": 90, "kilo1040": 80}


def ring_problem(fix_scale, n_free=RING_FREE, seed=3, noise=0.02, drift=0.05):
    """A loop of n_free + 1 keyframes one metre apart, vertex 0 fixed: odometry edges (i + 1, i), a chord (i + 3, i) from every
    third vertex, the loop edge (n_free, 0).  The estimates are disturbed; the measurements are those of the undisturbed ring,
    disturbed again, so they contradict each other (drift) and the minimum keeps a residual.  One map point per keyframe and one
    without a reference."""
    rng = np.random.default_rng(seed + (100 if fix_scale else 0))
    n = n_free + 1

    def sim3(rot, trans, sig):
        S = sim3_exp([float(v) for v in rot] + [float(v) for v in trans] + [float(sig)], np.float64)
        return [float(v) for v in S[0]], [float(v) for v in S[1]], float(S[2])

    q, t, s = zip(*[sim3(np.zeros(3), np.zeros(3), 0.0) if i == 0 else
                    sim3(rng.normal(size=3) * noise, np.array([-float(i), 0, 0]) + rng.normal(size=3) * noise, 0.0 if fix_scale else rng.normal() * noise)
                    for i in range(n)])
    edges = [(i + 1, i) for i in range(n - 1)] + [(i + 3, i) for i in range(0, n - 3, 3)] + [(n - 1, 0)]
    mq, mt, ms = zip(*[sim3(rng.normal(size=3) * drift, np.array([float(i - j), 0, 0]) + rng.normal(size=3) * drift, 0.0 if fix_scale else rng.normal() * drift)
                       for i, j in edges])
    pos = rng.normal(size=(n + 1, 3)).astype(np.float32) * 2
    return Problem(q, t, s, [True] + [False] * n_free, [fix_scale] * n, [e[0] for e in edges], [e[1] for e in edges], mq, mt, ms, pos, list(range(n)) + [-1])


def replicate(p, K, seed=13):
    """K disjoint copies of p, interleaved: vertex (point) v of copy c is vertex (point) v * K + c, every copy with its own fixed
    keyframe; the edges in the order of a seeded permutation.  The result carries edge_source / edge_copy and copies."""
    rep = lambda a: np.repeat(a, K, axis=0)
    copy_v = np.tile(np.arange(K), len(p.s))
    E = len(p.vi)
    o = np.random.RandomState(seed).permutation(E * K)
    src, copy_e = np.repeat(np.arange(E), K)[o], np.tile(np.arange(K), E)[o]
    ref = np.repeat(p.ref, K)
    ref = np.where(ref >= 0, ref * K + np.tile(np.arange(K), len(p.ref)), -1)
    r = Problem(rep(p.q), rep(p.t), rep(p.s), rep(p.fixed), rep(p.fix_scale), p.vi[src] * K + copy_e, p.vj[src] * K + copy_e, p.mq[src], p.mt[src], p.ms[src],
                rep(p.pos), ref)
    r.edge_source, r.edge_copy, r.copies, r.vertex_copy = src, copy_e, K, copy_v
    return r


def reorder_figure(terms):
    """|forward sum - reversed sum| / sum of the float64 terms, added one by one"""
    fwd = rev = 0.0
    for v in np.asarray(terms, np.float64).tolist():
        fwd += v
    for v in np.asarray(terms, np.float64)[::-1].tolist():
        rev += v
    return abs(fwd - rev) / abs(fwd)
