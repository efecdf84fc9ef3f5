"""Float64 numpy restatement of the numerical core of the welding BA, Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF,
pbStopFlag) (S/Optimizer.cc:6305-6983): a robust optimize(5), the outlier level (chi2 thresholds and the depth test), optimize(10)
over the level-0 edges without kernels, and the final check the write-back reads.

Self-contained beside tests/full_ba_model.py, whose solve() rounds its input to float32 and so cannot start a second round:
solve_round() takes a float64 state, a per-edge active mask and a robust switch, and is otherwise that solve, statement by statement
(tests/test_weld_ba_cpu.py holds the two against each other).  What g2o does with the level is restated here: a vertex none of whose
edges is active is not part of the round -- it is neither in the system nor in the largest diagonal entry behind lambda's first value,
and it keeps its estimate.  Per-edge residuals and Jacobians come from oracle.binding.lba_edge_eval (pinhole keyframes only)."""
import numpy as np

from multi_orbslam3_amd import _capi as capi
from oracle import binding as ob

from dense_lm import oplus, quat_from_R, quat_rot

D_MONO, D_STEREO = float(np.float32(np.sqrt(5.99))), float(np.float32(np.sqrt(7.815)))      # S/Optimizer.cc:6459-6460
CHI2_MONO, CHI2_STEREO = 5.991, 7.815                                                        # S/Optimizer.cc:6620, 6640


class Stop:
    """The abort flag of one call: raised from the start (before), or once `after_trials` LM trials have been evaluated -- counted
    through both rounds, as ba_weld_solve's -k form counts them."""

    def __init__(self, after_trials=None, before=False):
        self.after_trials, self.before, self.trials_done = after_trials, before, 0

    def __call__(self):
        return self.before or (self.after_trials is not None and self.trials_done >= self.after_trials)


class State:
    def __init__(self, q, t, X):
        self.q, self.t, self.X = q, t, X

    def copy(self):
        return State([a.copy() for a in self.q], [a.copy() for a in self.t], self.X.copy())


def state_from_float32(pr):
    """Converter::toSE3Quat of the float32 poses, the float32 points as doubles: what every solve of the project starts from."""
    q, t = [], []
    for i in range(len(pr["poses"])):
        T = np.asarray(pr["poses"][i], np.float32).reshape(4, 4).astype(np.float64)
        qi = quat_from_R(T[:3, :3])
        q.append(qi / np.linalg.norm(qi)); t.append(T[:3, 3].copy())
    return State(q, t, np.asarray(pr["points"], np.float32).astype(np.float64).reshape(-1, 3))


class RoundResult:
    pass


def solve_round(pr, state, active, robust, iterations, stop=None, reverse_sums=False):
    """One optimize(iterations) over the edges with active[k], from `state` (not modified).  Returns a RoundResult: state, iters,
    trace (iters, 3) = lambda, chi2, trials; chi2_initial / chi2_final; edge_chi2 (the last evaluation's, active edges; NaN elsewhere);
    evaluated (an evaluation ran at all); lambda_first and max_diagonal (over the active vertices)."""
    stop = Stop() if stop is None else stop
    E = pr["edges"]
    NE, P, L = len(E), len(pr["poses"]), len(pr["points"])
    active = np.asarray(active, bool)
    pcam = np.asarray(pr["pose_camera"], np.int64)
    cams = []
    for cam in pr["cameras"]:
        assert len(cam) <= 5 or cam[5] is None or cam[5][0] == capi.CAM_PINHOLE, "pinhole keyframes only"
        cams.append(np.array([np.float32(c) for c in cam[:5]], np.float32))
    e_pose = E["pose"].astype(np.int64); e_point = E["point"].astype(np.int64)
    mono = E["ur"] < 0
    om = E["inv_sigma2"].astype(np.float64)
    edge1 = [np.array([e], capi.EDGE_DTYPE) for e in E]
    act = [k for k in range(NE) if active[k]]
    pt_edges = [[] for _ in range(L)]
    for k in act:
        pt_edges[e_point[k]].append(k)
    included = np.array([1 if pt_edges[l] else 0 for l in range(L)], np.uint8)
    has_edge = set(int(e_pose[k]) for k in act)
    free = [i for i in range(P) if not pr["pose_fixed"][i] and i in has_edge]          # the active free poses
    pcol = {i: c for c, i in enumerate(free)}
    nP = len(free)
    order = (lambda lst: lst[::-1]) if reverse_sums else (lambda lst: lst)
    q, t, X = list(state.q), list(state.t), state.X.copy()

    def evaluate(q_, t_, X_, jac):
        chi = np.full(NE, np.nan); rho0 = np.zeros(NE); rho1 = np.ones(NE)
        errs = np.zeros((NE, 3)); As = np.zeros((NE, 3, 3)); Bs = np.zeros((NE, 3, 6))
        for k in act:
            i, l = e_pose[k], e_point[k]
            err, A, B = ob.lba_edge_eval(q_[i], t_[i], X_[l], cams[pcam[i]], edge1[k])
            D = 2 if mono[k] else 3
            c2 = 0.0
            for d in range(D):
                c2 += err[d] * (om[k] * err[d])
            chi[k] = c2
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

    res = RoundResult()
    res.trace, res.iters, res.chi2_initial, res.chi2_final = [], 0, 0.0, 0.0
    res.lambda_first = res.max_diagonal = None
    res.point_included = included
    res.active_free = free
    last_chi = np.full(NE, np.nan)
    lam, ni, nbad = -1.0, 2.0, 0
    cur_chi = 0.0
    ok = True
    it = 0
    n_iter = iterations if act else 0
    while it < n_iter and not stop() and ok:
        chi, rho0, rho1, errs, As, Bs = evaluate(q, t, X, True)
        last_chi = chi
        cur_chi = float(np.sum(rho0))                # (an inactive edge contributes a zero)
        w = rho1 * om
        Hpp = np.zeros((nP, 6, 6)); bp = np.zeros((nP, 6))
        Hll = np.zeros((L, 3, 3)); bl = np.zeros((L, 3)); Hpl = {}
        for k in act:
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
            res.lambda_first, res.max_diagonal = lam, md
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
            stop.trials_done += 1
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
    res.state = State(q, t, X)
    res.edge_chi2 = last_chi
    res.evaluated = res.iters > 0
    return res


def _rot_of(q):
    return np.array([quat_rot(q, ex) for ex in np.eye(3)]).T


def poses64(state):
    out = np.zeros((len(state.q), 4, 4))
    for i, (q, t) in enumerate(zip(state.q, state.t)):
        out[i] = np.eye(4)
        out[i, :3, :3] = _rot_of(q / np.linalg.norm(q))
        out[i, :3, 3] = t
    return out


def depths(pr, state):
    """z of every edge's point in its keyframe's camera frame: what isDepthPositive() tests."""
    E = pr["edges"]
    return np.array([(quat_rot(state.q[int(e["pose"])], state.X[int(e["point"])]) + state.t[int(e["pose"])])[2] for e in E], np.float64)


class WeldModelResult:
    pass


def solve(pr, iterations=5, iterations_second=10, chi2_mono=CHI2_MONO, chi2_stereo=CHI2_STEREO, stop_after_trials=None, stop_before=False,
          reverse_sums=False):
    """Both rounds, the level between them and the final check, with the stop forms of ba_weld_solve."""
    E = pr["edges"]
    NE, P = len(E), len(pr["poses"])
    mono = E["ur"] < 0
    th = np.where(mono, chi2_mono, chi2_stereo)
    stop = Stop(stop_after_trials, stop_before)
    s0 = state_from_float32(pr)
    r = WeldModelResult()
    r.status = 1 if stop_before else 0                      # LBA_ABORTED_BEFORE_OPT
    r.edge_level = np.zeros(NE, np.uint8)
    r.n_level1, r.rounds_run, r.iters_second = 0, 0, 0
    r.trace_second = np.zeros((0, 3)); r.chi2_initial_second = r.chi2_final_second = 0.0
    r.lambda_first_second = r.max_diagonal_second = None
    first = solve_round(pr, s0, np.ones(NE, bool), True, iterations, stop, reverse_sums)
    r.first = first
    r.iters, r.trace, r.chi2_initial, r.chi2_final = first.iters, first.trace, first.chi2_initial, first.chi2_final
    r.point_included = np.zeros(len(pr["points"]), np.uint8)
    r.point_included[np.unique(E["point"])] = 1
    final = first.state
    r.chi2_round1 = first.edge_chi2.copy() if first.evaluated else np.zeros(NE)
    r.depth_round1 = depths(pr, first.state)
    r.edge_chi2 = r.chi2_round1.copy()
    r.second = None
    if first.iters > 0:
        r.rounds_run = 1
        if not stop():
            out = (r.chi2_round1 > th) | ~(r.depth_round1 > 0.0)
            r.edge_level = out.astype(np.uint8)
            r.n_level1 = int(out.sum())
            if r.n_level1 < NE and iterations_second > 0:
                second = solve_round(pr, first.state, ~out, False, iterations_second, stop, reverse_sums)
                r.second = second
                r.rounds_run = 2
                r.iters_second, r.trace_second = second.iters, second.trace
                r.chi2_initial_second, r.chi2_final_second = second.chi2_initial, second.chi2_final
                r.lambda_first_second, r.max_diagonal_second = second.lambda_first, second.max_diagonal
                final = second.state
                if second.evaluated:
                    r.edge_chi2 = np.where(~out, second.edge_chi2, r.chi2_round1)
    r.state_round1, r.state = first.state, final
    r.poses64 = poses64(final)
    r.poses = r.poses64.astype(np.float32).reshape(P, 16)
    r.points = final.X.astype(np.float32)
    r.depth_final = depths(pr, final)
    r.edge_depth_pos = (r.depth_final > 0.0).astype(np.uint8)
    bad = (r.edge_chi2 > th) | (r.edge_depth_pos == 0)
    r.to_erase = np.concatenate([np.flatnonzero(bad & mono), np.flatnonzero(bad & ~mono)]).astype(np.int64)
    return r
