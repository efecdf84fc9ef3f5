"""Numpy restatement of TwoViewReconstruction::Reconstruct (S/TwoViewReconstruction.cc) with the arithmetic choices T-1 .. T-8 of
multi_orbslam3_amd/csrc/two_view.hip: the checker of the GPU path.  No CPU oracle exists for this path (OpenCV's float SVD is not
pinned), so the model is evaluated twice: `ft = np.float32` keeps the reference's types and serial sums and is what the kernel must
equal to the bit in T1, T2, the sets, the masks and the scores; `ft = np.float64` evaluates the same formulas without the float32
roundings and says how far float32 is from the exact answer.  The null vectors follow the same rule in both (float64 cyclic Jacobi on
A^T A).  Everything is batched over the hypotheses; serial sums are ufunc.accumulate calls, which add strictly left to right."""
import numpy as np

f64 = np.float64
TH_H = np.float32(5.991)
TH_F = np.float32(3.841)
TH_SCORE = np.float32(5.991)


# ---------------------------------------------------------------------------------------------- minimal sets

def resolve_draws_literal(n, draws):
    """The loop of :81-96 as written: vAvailableIndices with swap-with-back removal."""
    d = np.asarray(draws).reshape(-1, 8)
    out = np.zeros_like(d)
    for it in range(len(d)):
        avail = list(range(n))
        for j in range(8):
            randi = int(d[it, j])
            assert 0 <= randi <= len(avail) - 1
            out[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


# ---------------------------------------------------------------------------------------------- small matrices

def serial_sum(x, ft):
    return np.add.accumulate(np.asarray(x, ft), dtype=ft)[-1] if len(x) else ft(0)


def normalize(keys, ft):
    """Normalize, :753-799 -> (vNormalizedPoints (n, 2), T (3, 3))."""
    k = np.asarray(keys, ft).reshape(-1, 2)
    n = ft(len(k))
    with np.errstate(all="ignore"):
        meanX, meanY = serial_sum(k[:, 0], ft) / n, serial_sum(k[:, 1], ft) / n
        px, py = k[:, 0] - meanX, k[:, 1] - meanY
        devX, devY = serial_sum(np.abs(px), ft) / n, serial_sum(np.abs(py), ft) / n
        sX, sY = ft(f64(1.0) / f64(devX)), ft(f64(1.0) / f64(devY))
        pn = np.stack([px * sX, py * sY], axis=1).astype(ft)
        T = np.zeros((3, 3), ft)
        T[0, 0], T[1, 1], T[2, 2], T[0, 2], T[1, 2] = sX, sY, 1, -meanX * sX, -meanY * sY
    return pn, T


def mul3(a, b, ft):
    """T-2: each entry accumulated in double in k order, rounded once."""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return ((a[..., :, 0:1] * b[..., 0:1, :] + a[..., :, 1:2] * b[..., 1:2, :]) + a[..., :, 2:3] * b[..., 2:3, :]).astype(ft)


def mulv3(a, v, ft, beta=None, alpha=None):
    a, v = np.asarray(a, f64), np.asarray(v, f64)
    s = (a[..., :, 0] * v[..., 0:1] + a[..., :, 1] * v[..., 1:2]) + a[..., :, 2] * v[..., 2:3]
    if alpha is not None:
        s = f64(alpha) * s
    if beta is not None:
        s = s + np.asarray(beta, f64)
    return s.astype(ft)


def det3(m):
    m = np.asarray(m, f64)
    a, b, c, d, e, f, g, h, i = (m[..., r, k] for r in range(3) for k in range(3))
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g)


def inv3(m, ft):
    """T-6."""
    m = np.asarray(m, f64)
    a, b, c, d, e, f, g, h, i = (m[..., r, k] for r in range(3) for k in range(3))
    with np.errstate(all="ignore"):
        det = (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g)
        idt = f64(1.0) / det
        o = [(e * i - f * h) * idt, (c * h - b * i) * idt, (b * f - c * e) * idt,
             (f * g - d * i) * idt, (a * i - c * g) * idt, (c * d - a * f) * idt,
             (d * h - e * g) * idt, (b * g - a * h) * idt, (a * e - b * d) * idt]
    return np.stack(o, axis=-1).reshape(m.shape).astype(ft)


def jacobi(S, nan_breaks=True, sweeps=60):
    """The cyclic Jacobi of T-1 on a batch of symmetric matrices (B, n, n), float64 -> (S, V).  nan_breaks: a NaN off-diagonal sum
    stops the iteration (two_view.hip); False: it does not (null_vector4.hpp, `off <= 1e-28 * diag`)."""
    S = np.array(S, f64)
    B, n = S.shape[0], S.shape[1]
    V = np.zeros_like(S)
    V[:, np.arange(n), np.arange(n)] = 1.0
    active = np.ones(B, bool)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            off, diag = np.zeros(B), np.zeros(B)
            for p in range(n):
                diag = diag + S[:, p, p] * S[:, p, p]
                for q in range(p + 1, n):
                    off = off + S[:, p, q] * S[:, p, q]
            stop = ~(off > 1e-28 * diag) if nan_breaks else (off <= 1e-28 * diag)
            active &= ~stop
            if not active.any():
                break
            for p in range(n):
                for q in range(p + 1, n):
                    spq = S[:, p, q]
                    m = active & (spq != 0.0)
                    if not m.any():
                        continue
                    tau = (S[:, q, q] - S[:, p, p]) / (2.0 * spq)
                    t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                    cs = 1.0 / np.sqrt(1.0 + t * t)
                    sn = t * cs
                    cs1, sn1, mm = cs[:, None], sn[:, None], m[:, None]
                    a, b = S[:, :, p].copy(), S[:, :, q].copy()
                    S[:, :, p] = np.where(mm, cs1 * a - sn1 * b, a); S[:, :, q] = np.where(mm, sn1 * a + cs1 * b, b)
                    a, b = S[:, p, :].copy(), S[:, q, :].copy()
                    S[:, p, :] = np.where(mm, cs1 * a - sn1 * b, a); S[:, q, :] = np.where(mm, sn1 * a + cs1 * b, b)
                    a, b = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p] = np.where(mm, cs1 * a - sn1 * b, a); V[:, :, q] = np.where(mm, sn1 * a + cs1 * b, b)
    return S, V


def null_vector(S, nan_breaks=True):
    """Eigenvector of the smallest eigenvalue (first one on a tie), float64."""
    S, V = jacobi(S, nan_breaks)
    n = S.shape[1]
    d = S[:, np.arange(n), np.arange(n)]
    m = np.zeros(len(S), np.int64)
    small = d[:, 0].copy()
    for i in range(1, n):
        lt = d[:, i] < small
        small = np.where(lt, d[:, i], small)
        m = np.where(lt, i, m)
    return V[np.arange(len(S)), :, m]


def ata(rows):
    """S = A^T A in float64, accumulated row by row.  rows: list of (B, n) arrays."""
    B, n = rows[0].shape
    S = np.zeros((B, n, n), f64)
    for a in rows:
        a = np.asarray(a, f64)
        S = S + a[:, :, None] * a[:, None, :]
    return S


def svd3(M, complete, ft):
    """T-5 on a batch (B, 3, 3) -> U (B, 3, 3), w (B, 3), V (B, 3, 3), columns are the vectors."""
    M = np.asarray(M, f64)
    S = ata([M[:, k, :] for k in range(3)])
    S, E = jacobi(S)
    lam = S[:, np.arange(3), np.arange(3)].copy()
    for a, b in ((0, 1), (1, 2), (0, 1)):
        sw = lam[:, a] < lam[:, b]
        la, lb = lam[:, a].copy(), lam[:, b].copy()
        lam[:, a] = np.where(sw, lb, la); lam[:, b] = np.where(sw, la, lb)
        ea, eb = E[:, :, a].copy(), E[:, :, b].copy()
        E[:, :, a] = np.where(sw[:, None], eb, ea); E[:, :, b] = np.where(sw[:, None], ea, eb)
    with np.errstate(all="ignore"):
        sg = np.sqrt(np.where(lam > 0, lam, 0.0))
        U = np.zeros_like(M)
        for c in range(3):
            U[:, :, c] = ((M[:, :, 0] * E[:, 0:1, c] + M[:, :, 1] * E[:, 1:2, c]) + M[:, :, 2] * E[:, 2:3, c]) / sg[:, c:c + 1]
        if complete:
            u0, u1 = U[:, :, 0], U[:, :, 1]
            U[:, 0, 2] = u0[:, 1] * u1[:, 2] - u0[:, 2] * u1[:, 1]
            U[:, 1, 2] = u0[:, 2] * u1[:, 0] - u0[:, 0] * u1[:, 2]
            U[:, 2, 2] = u0[:, 0] * u1[:, 1] - u0[:, 1] * u1[:, 0]
    return U.astype(ft), sg.astype(ft), E.astype(ft)


# ---------------------------------------------------------------------------------------------- hypotheses

def compute_H21(p1, p2, ft):
    """ComputeH21, :231-271, for a batch of sets: p1 / p2 (B, 8, 2) normalised points -> Hn (B, 3, 3)."""
    rows = []
    z, one = np.zeros(len(p1), ft), np.ones(len(p1), ft)
    for i in range(8):
        u1, v1, u2, v2 = p1[:, i, 0], p1[:, i, 1], p2[:, i, 0], p2[:, i, 1]
        rows.append(np.stack([z, z, z, -u1, -v1, -one, v2 * u1, v2 * v1, v2], axis=1))
        rows.append(np.stack([u1, v1, one, z, z, z, -u2 * u1, -u2 * v1, -u2], axis=1))
    return null_vector(ata(rows)).astype(ft).reshape(-1, 3, 3)


def compute_F21(p1, p2, ft):
    """ComputeF21, :273-308."""
    rows = []
    one = np.ones(len(p1), ft)
    for i in range(8):
        u1, v1, u2, v2 = p1[:, i, 0], p1[:, i, 1], p2[:, i, 0], p2[:, i, 1]
        rows.append(np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, one], axis=1))
    Fpre = null_vector(ata(rows)).astype(ft).reshape(-1, 3, 3)
    U, w, V = svd3(Fpre, True, ft)
    w = w.copy()
    w[:, 2] = 0
    with np.errstate(all="ignore"):
        UW = (U * w[:, None, :]).astype(ft)
    return mul3(UW, np.swapaxes(V, 1, 2), ft)


def _accumulate(c1, c2, ft):
    """score += c1; score += c2 per match, left to right.  A skipped term is +0, which leaves a non-negative sum unchanged."""
    B, N = c1.shape
    inter = np.empty((B, 2 * N), ft)
    inter[:, 0::2], inter[:, 1::2] = c1, c2
    return np.add.accumulate(inter, axis=1, dtype=ft)[:, -1]


def check_homography(H21, H12, m, sigma, ft):
    """CheckHomography, :310-393, for a batch (B, 3, 3); m = (u1, v1, u2, v2) arrays over the matches -> score (B), mask (B, N),
    chi1, chi2 (B, N)."""
    u1, v1, u2, v2 = (np.asarray(x, ft)[None, :] for x in m)
    h = [np.asarray(H21, ft)[:, r, c][:, None] for r in range(3) for c in range(3)]
    g = [np.asarray(H12, ft)[:, r, c][:, None] for r in range(3) for c in range(3)]
    th = ft(TH_H)
    with np.errstate(all="ignore"):
        inv_s2 = ft(f64(1.0) / f64(ft(sigma) * ft(sigma)))
        w2 = ft(1) / (g[6] * u2 + g[7] * v2 + g[8])
        a, b = (g[0] * u2 + g[1] * v2 + g[2]) * w2, (g[3] * u2 + g[4] * v2 + g[5]) * w2
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_s2
        w1 = ft(1) / (h[6] * u1 + h[7] * v1 + h[8])
        a, b = (h[0] * u1 + h[1] * v1 + h[2]) * w1, (h[3] * u1 + h[4] * v1 + h[5]) * w1
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_s2
        out1, out2 = chi1 > th, chi2 > th
        score = _accumulate(np.where(out1, ft(0), th - chi1), np.where(out2, ft(0), th - chi2), ft)
    return score, ~(out1 | out2), chi1, chi2


def check_fundamental(F21, m, sigma, ft):
    """CheckFundamental, :395-473."""
    u1, v1, u2, v2 = (np.asarray(x, ft)[None, :] for x in m)
    f = [np.asarray(F21, ft)[:, r, c][:, None] for r in range(3) for c in range(3)]
    th, ths = ft(TH_F), ft(TH_SCORE)
    with np.errstate(all="ignore"):
        inv_s2 = ft(f64(1.0) / f64(ft(sigma) * ft(sigma)))
        a2, b2, c2 = f[0] * u1 + f[1] * v1 + f[2], f[3] * u1 + f[4] * v1 + f[5], f[6] * u1 + f[7] * v1 + f[8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2
        a1, b1, c1 = f[0] * u2 + f[3] * v2 + f[6], f[1] * u2 + f[4] * v2 + f[7], f[2] * u2 + f[5] * v2 + f[8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2
        out1, out2 = chi1 > th, chi2 > th
        score = _accumulate(np.where(out1, ft(0), ths - chi1), np.where(out2, ft(0), ths - chi2), ft)
    return score, ~(out1 | out2), chi1, chi2


def serial_best(scores):
    """`if(currentScore>score)` from score = 0 over the iterations in order -> (score, iteration or -1)."""
    best, idx = np.float32(0) if np.asarray(scores).dtype == np.float32 else f64(0), -1
    for i, s in enumerate(np.asarray(scores)):
        if s > best:
            best, idx = s, i
    return best, idx


def choose_model(SH, SF):
    """:111-126 -> 0 (return false), 1 (ReconstructH), 2 (ReconstructF)."""
    t = type(SH)
    if t(SH + SF) == 0:
        return 0
    RH = t(SH / t(SH + SF))
    return 1 if f64(RH) > 0.50 else 2


# ---------------------------------------------------------------------------------------------- motion hypotheses, CheckRT

def _K(cam, ft):
    fx, fy, cx, cy = cam
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], ft)


def _unit(t, ft):
    t = np.asarray(t, ft)
    with np.errstate(all="ignore"):
        nrm = np.sqrt((f64(t[0]) * f64(t[0]) + f64(t[1]) * f64(t[1])) + f64(t[2]) * f64(t[2]))
        return (t * ft(f64(1.0) / nrm)).astype(ft)


def motions_F(F21, cam, ft):
    """ReconstructF :484-492 with DecomposeE :913-933 -> R (4, 3, 3), t (4, 3)."""
    K = _K(cam, ft)
    E = mul3(mul3(K.T, F21, ft), K, ft)
    U, w, V = svd3(E[None], True, ft)
    U, Vt = U[0], V[0].T
    t = _unit(U[:, 2], ft)
    uW = np.stack([U[:, 1], -U[:, 0], U[:, 2]], axis=1)
    uWt = np.stack([-U[:, 1], U[:, 0], U[:, 2]], axis=1)
    R1, R2 = mul3(uW, Vt, ft), mul3(uWt, Vt, ft)
    if det3(R1) < 0:
        R1 = -R1
    if det3(R2) < 0:
        R2 = -R2
    return np.stack([R1, R2, R1, R2]), np.stack([t, t, -t, -t])


def motions_H(H21, cam, ft):
    """ReconstructH :588-690 -> (R (8, 3, 3), t (8, 3)) or None for the d1 / d2, d2 / d3 return."""
    K = _K(cam, ft)
    A = mul3(mul3(inv3(K, ft), H21, ft), K, ft)
    U, w, V = svd3(A[None], False, ft)
    U, w, Vt = U[0], w[0], V[0].T
    with np.errstate(all="ignore"):
        s = ft(det3(U) * det3(Vt))
        d1, d2, d3 = w
        if f64(d1 / d2) < 1.00001 or f64(d2 / d3) < 1.00001:
            return None
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        st = [aux_st, -aux_st, -aux_st, aux_st]
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        Rs, ts = [], []
        for m in range(8):
            i = m & 3
            Rp = np.eye(3, dtype=ft)
            if m < 4:
                Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ct, -st[i], st[i], ct
                f, tp = d1 - d3, np.array([x1[i], 0, -x3[i]], ft)
            else:
                Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cp, sp[i], -1, sp[i], -cp
                f, tp = d1 + d3, np.array([x1[i], 0, x3[i]], ft)
            tp = (tp * ft(f)).astype(ft)
            Uf, Rpf = U.astype(f64), Rp.astype(f64)
            M1 = (f64(s) * ((Uf[:, 0:1] * Rpf[0:1, :] + Uf[:, 1:2] * Rpf[1:2, :]) + Uf[:, 2:3] * Rpf[2:3, :])).astype(ft)
            Rs.append(mul3(M1, Vt, ft))
            ts.append(_unit(mulv3(U, tp, ft), ft))
    return np.stack(Rs), np.stack(ts)


def check_rt(R, t, m, inliers, cam, sigma, ft, details=False):
    """CheckRT, :802-911, for one motion hypothesis over the matches m = (u1, v1, u2, v2) -> nGood, parallax, counted (N) bool,
    good (N) bool, p3d (N, 3), and the gate record per match (0 not an inlier, 1 non-finite, 2 depth 1, 3 depth 2, 4 reprojection 1,
    5 reprojection 2, 6 counted).  details: a seventh entry with the quantities the gates are taken on, per match and whether or not
    the match reaches the gate (e1, e2 against th2; z1, z2 against 0; cosP against 0.99998), th2 and the sorted cosP of the counted
    matches."""
    fx, fy, cx, cy = (ft(v) for v in cam)
    u1, v1, u2, v2 = (np.asarray(x, ft) for x in m)
    N = len(u1)
    K = _K(cam, ft)
    R, t = np.asarray(R, ft), np.asarray(t, ft)
    P1 = np.zeros((3, 4), ft); P1[:, :3] = K
    P2 = np.zeros((3, 4), ft)
    P2[:, :3] = mul3(K, R, ft); P2[:, 3] = mulv3(K, t, ft)
    O2 = mulv3(R.T, t, ft, alpha=-1.0)
    th2 = ft(4.0 * f64(ft(sigma) * ft(sigma)))
    with np.errstate(all="ignore"):
        rows = [u1[:, None] * P1[2][None, :] - P1[0][None, :], v1[:, None] * P1[2][None, :] - P1[1][None, :],
                u2[:, None] * P2[2][None, :] - P2[0][None, :], v2[:, None] * P2[2][None, :] - P2[1][None, :]]
        v = null_vector(ata([r.astype(ft) for r in rows]), nan_breaks=False)
        inv = (f64(1.0) / v[:, 3].astype(ft).astype(f64)).astype(ft)
        p = (v[:, :3].astype(ft) * inv[:, None]).astype(ft)
        gate = np.zeros(N, np.int32)
        alive = np.asarray(inliers, bool).copy()
        fin = np.isfinite(p).all(axis=1)
        gate[alive & ~fin] = 1; alive &= fin
        n2 = (p - O2[None, :]).astype(ft)
        pd, nd = p.astype(f64), n2.astype(f64)
        dist1 = np.sqrt((pd[:, 0] * pd[:, 0] + pd[:, 1] * pd[:, 1]) + pd[:, 2] * pd[:, 2]).astype(ft)
        dist2 = np.sqrt((nd[:, 0] * nd[:, 0] + nd[:, 1] * nd[:, 1]) + nd[:, 2] * nd[:, 2]).astype(ft)
        dot = (pd[:, 0] * nd[:, 0] + pd[:, 1] * nd[:, 1]) + pd[:, 2] * nd[:, 2]
        cosP = (dot / (dist1 * dist2).astype(ft).astype(f64)).astype(ft)
        low = cosP.astype(f64) < 0.99998
        bad = alive & (p[:, 2] <= 0) & low
        gate[bad] = 2; alive &= ~bad
        p2 = mulv3(R[None], p, ft, beta=t[None, :].astype(f64))
        bad = alive & (p2[:, 2] <= 0) & low
        gate[bad] = 3; alive &= ~bad
        invZ1 = ft(1) / p[:, 2]
        im1x, im1y = fx * p[:, 0] * invZ1 + cx, fy * p[:, 1] * invZ1 + cy
        e1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1)
        bad = alive & (e1 > th2)
        gate[bad] = 4; alive &= ~bad
        invZ2 = ft(1) / p2[:, 2]
        im2x, im2y = fx * p2[:, 0] * invZ2 + cx, fy * p2[:, 1] * invZ2 + cy
        e2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2)
        bad = alive & (e2 > th2)
        gate[bad] = 5; alive &= ~bad
        gate[alive] = 6
        nGood = int(alive.sum())
        parallax = ft(0)
        srt = np.sort(cosP[alive])
        if nGood > 0:
            c = srt[min(50, nGood - 1)]
            parallax = parallax_of(c, ft)
    res = (nGood, parallax, alive, alive & low, np.where(alive[:, None], p, ft(0)).astype(ft), gate)
    if details:
        res += (Out(e1=e1, e2=e2, z1=p[:, 2], z2=p2[:, 2], cosP=cosP, th2=th2, sorted=srt),)
    return res


def parallax_of(c, ft):
    """:898 on one cosine: acos in double, degrees as the reference's types give them (T-8)."""
    with np.errstate(all="ignore"):
        return ft(f64(ft(np.arccos(f64(c))) * ft(180)) / np.pi)


def decide_F(nGood, parallax, n_inliers, minParallax=1.0, minTriangulated=50):
    """:504-574 -> the index of the motion hypothesis returned, or -1."""
    g = [int(x) for x in nGood]
    maxGood = max(g)
    nMinGood = max(int(0.9 * n_inliers), minTriangulated)
    nsimilar = sum(1 for x in g if x > 0.7 * maxGood)
    if maxGood < nMinGood or nsimilar > 1:
        return -1
    for i in range(4):
        if maxGood == g[i]:
            return i if np.float32(parallax[i]) > np.float32(minParallax) else -1
    return -1


def decide_H(nGood, parallax, n_inliers, minParallax=1.0, minTriangulated=50):
    """:693-735."""
    bestGood, secondBestGood, bestIdx, bestParallax = 0, 0, -1, np.float32(-1)
    for i in range(8):
        n = int(nGood[i])
        if n > bestGood:
            secondBestGood, bestGood, bestIdx, bestParallax = bestGood, n, i, np.float32(parallax[i])
        elif n > secondBestGood:
            secondBestGood = n
    if secondBestGood < 0.75 * bestGood and bestParallax >= np.float32(minParallax) and bestGood > minTriangulated and bestGood > 0.9 * n_inliers:
        return bestIdx
    return -1


# ---------------------------------------------------------------------------------------------- Reconstruct

class Out(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def match_list(matches12):
    m12 = np.asarray(matches12).reshape(-1)
    i1 = np.nonzero(m12 >= 0)[0]
    return i1, m12[i1]


def reconstruct(keys1, keys2, matches12, cam, sigma, iterations, draws, ft=np.float32):
    """Reconstruct, :39-127.  cam = (fx, fy, cx, cy); draws: (iterations, 8) raw draws."""
    keys1, keys2 = np.asarray(keys1, ft).reshape(-1, 2), np.asarray(keys2, ft).reshape(-1, 2)
    i1, i2 = match_list(matches12)
    N = len(i1)
    sets = resolve_draws_literal(N, np.asarray(draws).reshape(-1, 8)[:iterations])
    pn1, T1 = normalize(keys1, ft)
    pn2, T2 = normalize(keys2, ft)
    T2inv = inv3(T2, ft)
    m = (keys1[i1, 0], keys1[i1, 1], keys2[i2, 0], keys2[i2, 1])
    p1, p2 = pn1[i1][sets], pn2[i2][sets]                      # (H, 8, 2)
    Hn = compute_H21(p1, p2, ft)
    H21 = mul3(mul3(T2inv[None], Hn, ft), T1[None], ft)
    H12 = inv3(H21, ft)
    sH, mH, chiH1, chiH2 = check_homography(H21, H12, m, sigma, ft)
    Fn = compute_F21(p1, p2, ft)
    F21 = mul3(mul3(T2.T[None], Fn, ft), T1[None], ft)
    sF, mF, chiF1, chiF2 = check_fundamental(F21, m, sigma, ft)
    o = Out(N=N, i1=i1, i2=i2, sets=sets, T1=T1, T2=T2, H21=H21, F21=F21, scores=np.stack([sH, sF]), masks=np.stack([mH, mF]),
            chi=np.stack([np.stack([chiH1, chiH2]), np.stack([chiF1, chiF2])]), m=m)
    o.update(finish(o, o.scores, cam, sigma, len(keys1), ft))
    return o


def finish(o, scores, cam, sigma, n1, ft=np.float32, motion_stats=None):
    """Everything behind the two RANSAC loops, from per-hypothesis `scores` (2, H) -- the model's own or the product's.
    motion_stats: (nGood, parallax) per motion to decide on instead of the model's own."""
    SH, bH = serial_best(scores[0])
    SF, bF = serial_best(scores[1])
    model = choose_model(ft(SH), ft(SF))
    r = Out(SH=SH, SF=SF, bestH=bH, bestF=bF, model=model, ok=False, best_motion=-1, n_motions=0, h_degenerate=False,
            motion_nGood=np.zeros(0, np.int32), motion_parallax=np.zeros(0, ft), motion_R=np.zeros((0, 3, 3), ft),
            motion_t=np.zeros((0, 3), ft), R21=np.zeros((3, 3), ft), t21=np.zeros(3, ft), vP3D=np.zeros((n1, 3), ft),
            vbTriangulated=np.zeros(n1, bool), n_inliers=0, gates=None, counted=None, good=None, rt=None)
    if model == 0:
        return r
    inl = o.masks[0, bH] if model == 1 else o.masks[1, bF]
    r.n_inliers = int(inl.sum())
    mot = motions_H(o.H21[bH], cam, ft) if model == 1 else motions_F(o.F21[bF], cam, ft)
    if mot is None:
        r.h_degenerate = True
        return r
    Rs, ts = mot
    res = [check_rt(Rs[k], ts[k], o.m, inl, cam, sigma, ft, details=True) for k in range(len(Rs))]
    r.n_motions = len(Rs)
    r.motion_R, r.motion_t = Rs, ts
    r.motion_nGood = np.array([x[0] for x in res], np.int32)
    r.motion_parallax = np.array([x[1] for x in res], ft)
    r.gates = np.stack([x[5] for x in res])
    r.counted, r.good = np.stack([x[2] for x in res]), np.stack([x[3] for x in res])
    r.rt = [x[6] for x in res]
    ng, par = (r.motion_nGood, r.motion_parallax) if motion_stats is None else motion_stats
    k = decide_H(ng, par, r.n_inliers) if model == 1 else decide_F(ng, par, r.n_inliers)
    r.best_motion = k
    if k >= 0:
        r.ok = True
        r.R21, r.t21 = Rs[k], ts[k]
        r.vP3D[o.i1[res[k][2]]] = res[k][4][res[k][2]]
        r.vbTriangulated[o.i1[res[k][3]]] = True
    return r


# ---------------------------------------------------------------------------------------------- scenes

def scene(kind, n_matches, seed, n_extra1=0, n_extra2=0, noise=0.3, baseline=0.4, outliers=0.1, cam=(520.0, 520.0, 320.0, 240.0),
          size=(640.0, 480.0), offset=None, depth=(3.0, 9.0)):
    """A synthetic two-view scene -> keys1 (n1, 2), keys2 (n2, 2), matches12 (n1), R, t (unit), X (per match, camera-1 frame).
    kind: "3d" (depths 3 .. 9), "plane" (a slanted plane), "rotation" (no translation), "tiny" (a sub-degree baseline).  Unmatched
    keypoints are interleaved on both sides, so the match index differs from the keypoint index and n1 != n2.  size: the image, in
    pixels; keypoints keep a margin of 1 / 32 of it."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = cam
    n = n_matches
    x0, x1, y0, y1 = size[0] / 32, size[0] * 31 / 32, size[1] / 32, size[1] * 31 / 32
    uv = np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)], axis=1)
    ray = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(n)], axis=1)
    if kind == "plane":
        nrm, d = np.array([0.15, -0.1, 1.0]), 5.0
        z = d / (ray @ nrm)
    else:
        z = rng.uniform(depth[0], depth[1], n)
    X = ray * z[:, None]
    ang = np.array([0.02, -0.05, 0.01])
    th = np.linalg.norm(ang)
    k = ang / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    tdir = np.array([1.0, 0.1, 0.05]); tdir /= np.linalg.norm(tdir)
    b = {"3d": baseline, "plane": baseline, "rotation": 0.0, "tiny": 0.004}[kind]
    X2 = X @ R.T + b * tdir
    uv2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], axis=1)
    uv = uv + rng.normal(0, noise, uv.shape); uv2 = uv2 + rng.normal(0, noise, uv2.shape)
    n_out = int(outliers * n)
    if n_out:
        bad = rng.choice(n, n_out, replace=False)
        if offset is None:
            uv2[bad] = np.stack([rng.uniform(x0, x1, n_out), rng.uniform(y0, y1, n_out)], axis=1)
        else:                                           # mismatches a few pixels off: their chi-squares lie around the gates
            a, r = rng.uniform(0, 2 * np.pi, n_out), rng.uniform(offset[0], offset[1], n_out)
            uv2[bad] += np.stack([r * np.cos(a), r * np.sin(a)], axis=1)
    n1, n2 = n + n_extra1, n + n_extra2
    pos1 = np.sort(rng.choice(n1, n, replace=False))
    pos2 = rng.permutation(n2)[:n]
    keys1 = np.stack([rng.uniform(x0, x1, n1), rng.uniform(y0, y1, n1)], axis=1)
    keys2 = np.stack([rng.uniform(x0, x1, n2), rng.uniform(y0, y1, n2)], axis=1)
    keys1[pos1], keys2[pos2] = uv, uv2
    m12 = np.full(n1, -1, np.int32)
    m12[pos1] = pos2
    return Out(keys1=keys1.astype(np.float32), keys2=keys2.astype(np.float32), matches12=m12, R=R, t=tdir, X=X, cam=cam, pos1=pos1)


# ---------------------------------------------------------------------------------------------- the committed cases

# name -> (kind, N matches, iterations, seed, scene keywords).  N: 8 (one possible set), 63 / 64 / 65 (mask word and wavefront edge),
# 100 (Tracking's minimum), 257 (one above the kernel's LDS tile of 256 matches); iterations: 1, 31 / 32 / 33 (one below / at / above
# the kernel's 32 hypotheses per workgroup) and 200.  The p* family is the one the bit equality is CAPPED on (docs/experiments.md,
# "TwoViewReconstruction"): a plane seen with 0.05 px noise, for which both RANSACs fit and few chi-squares lie around a gate; on a
# 3-D scene every homography hypothesis is a wrong model whose chi-squares spread over the gates, and no choice of noise or outliers
# keeps the two models inside the cap there.  "wide" is a usual initialisation (3-D, 10 % mismatches, F is chosen), "plane" the
# scene whose homography wins (RH > 0.5 needs few iterations: over 200, some F of the family [s]x H always scores higher).
_P = dict(noise=0.05, outliers=0.0, baseline=1.0)
CASES = {
    "p8": ("plane", 8, 33, 1, _P),
    "p63": ("plane", 63, 31, 2, _P),
    "p64": ("plane", 64, 32, 3, _P),
    "p65": ("plane", 65, 33, 4, _P),
    "p100": ("plane", 100, 200, 5, _P),
    "p257": ("plane", 257, 1, 6, _P),
    "wide": ("3d", 300, 200, 1, {}),
    "plane": ("plane", 150, 4, 13, dict(noise=0.6, outliers=0.0, baseline=1.0)),
}
CAPPED = ("p8", "p63", "p64", "p65", "p100", "p257")
CAM = (520.0, 520.0, 320.0, 240.0)
SIZE = (640.0, 480.0)
_cache = {}


def case_draws(N, iterations, seed):
    rng = np.random.default_rng(seed + 10)
    d = np.empty((iterations, 8), np.int32)
    for j in range(8):
        d[:, j] = rng.integers(0, max(N - j, 1), size=iterations)
    return d


def case(name):
    """-> (scene, draws, float32 model, float64 model), computed once per process and shared; callers must not modify them."""
    if name not in _cache:
        kind, N, its, seed, kw = CASES[name]
        sc = scene(kind, N, seed, n_extra1=37, n_extra2=71, cam=CAM, size=SIZE, **kw)
        d = case_draws(N, its, seed)
        o32 = reconstruct(sc.keys1, sc.keys2, sc.matches12, sc.cam, 1.0, its, d, np.float32)
        o64 = reconstruct(sc.keys1, sc.keys2, sc.matches12, sc.cam, 1.0, its, d, np.float64)
        _cache[name] = (sc, d, o32, o64)
    return _cache[name]


def gate_thresholds():
    return np.array([TH_H, TH_F], f64)[:, None, None, None]


def measured_chi_difference(names=CAPPED):
    """The largest relative chi-square difference between the float32 and the float64 model over the (hypothesis, match) pairs whose
    float64 chi-square lies in [th / 2, 2 th]."""
    worst = 0.0
    for n in names:
        _, _, o32, o64 = case(n)
        th = gate_thresholds()
        c64, c32 = o64.chi, o32.chi.astype(f64)
        with np.errstate(all="ignore"):
            band = (c64 >= th / 2) & (c64 <= 2 * th)
            rel = np.abs(c32 - c64) / c64
        if band.any():
            worst = max(worst, float(rel[band].max()))
    return worst


def flagged(o64, delta):
    """(2, H) bool: hypotheses holding a (hypothesis, match) pair whose float64 chi-square is within delta relative of its gate."""
    th = gate_thresholds()
    with np.errstate(all="ignore"):
        near = np.abs(o64.chi - th) <= delta * th
    return near.any(axis=(1, 3))


def near_directions(o64, delta):
    """(2, 2, H, N) bool: (model, direction, hypothesis, match) whose float64 chi-square is within delta relative of its gate."""
    th = gate_thresholds()
    with np.errstate(all="ignore"):
        return np.abs(o64.chi - th) <= delta * th


def near_pairs(o64, delta):
    """(2, H, N) bool: a (model, hypothesis, match) pair is near when the float64 chi-square of either direction lies within delta
    relative of its gate.  Only these mask bits may differ from the float32 model's."""
    return near_directions(o64, delta).any(axis=1)


# CheckRT's gates (:835-891): squareError1 / squareError2 > th2, z1 / z2 <= 0, cosParallax < 0.99998
COS_GATE = 0.99998
Z_BAND = 2.0        # the depth gate is 0: "within a factor 2" has no meaning there, so its band is |z| <= 2 baselines (t21 has unit length)
RT_STAGE = dict(z1=2, z2=3, e1=4, e2=5)   # the smallest gate record of a match that reached the gate on this quantity


def same_rt(a, b):
    """The two models ran CheckRT on the same thing: one model chosen, its winning row equal, as many motions."""
    if a.model != b.model or a.model == 0 or a.n_motions != b.n_motions or a.n_motions == 0:
        return False
    return a.bestH == b.bestH if a.model == 1 else a.bestF == b.bestF


def measured_rt_differences(pairs):
    """The largest float32-to-float64 difference of CheckRT's gate quantities over (float32 model, float64 model) pairs, each over the
    matches that reach the gate in the float64 model and whose float64 value lies within a factor 2 of the gate: relative for e1 / e2
    (th2 / 2 .. 2 th2); absolute for cosP, the band taken on what the gate measures, 1 - cosP within a factor 2 of 1 - 0.99998; absolute
    for z over |z| <= Z_BAND where the depth gates are live (cosP < 0.99998) -> dict(e, cos, z) and the matches in each band."""
    w, cnt = dict(e=0.0, cos=0.0, z=0.0), dict(e=0, cos=0, z=0)
    for a, b in pairs:
        if not same_rt(a, b):
            continue
        for k in range(b.n_motions):
            qa, qb, g = a.rt[k], b.rt[k], b.gates[k]
            with np.errstate(all="ignore"):
                for name in ("e1", "e2"):
                    x, y = qa[name].astype(f64), qb[name]
                    band = (g >= RT_STAGE[name]) & (y >= qb.th2 / 2) & (y <= 2 * qb.th2) & np.isfinite(x)
                    if band.any():
                        w["e"] = max(w["e"], float((np.abs(x - y) / y)[band].max())); cnt["e"] += int(band.sum())
                low = qb.cosP < COS_GATE
                for name in ("z1", "z2"):
                    x, y = qa[name].astype(f64), qb[name]
                    band = (g >= RT_STAGE[name]) & low & (np.abs(y) <= Z_BAND) & np.isfinite(x)
                    if band.any():
                        w["z"] = max(w["z"], float(np.abs(x - y)[band].max())); cnt["z"] += int(band.sum())
                x, y = qa.cosP.astype(f64), qb.cosP
                band = (g >= 2) & (1 - y >= (1 - COS_GATE) / 2) & (1 - y <= 2 * (1 - COS_GATE)) & np.isfinite(x)
                if band.any():
                    w["cos"] = max(w["cos"], float(np.abs(x - y)[band].max())); cnt["cos"] += int(band.sum())
    return w, cnt


def open_matches(a, b, margins):
    """(n_motions of a, N) bool: the matches of each motion hypothesis on which the float32 model's CheckRT record is not binding.
    A match is open when the two models give it different gate records, or when a float64 gate quantity it reaches lies within its
    margin of the gate (margins: dict(e relative, cos absolute, z absolute), 4 x measured_rt_differences).  Where the two models did
    not run CheckRT on the same thing (same_rt) every match is open.  Formed from the models alone."""
    if a.n_motions == 0:
        return np.zeros((0, a.N), bool)
    if not same_rt(a, b):
        return np.ones((a.n_motions, a.N), bool)
    op = a.gates != b.gates
    for k in range(b.n_motions):
        q, g = b.rt[k], b.gates[k]
        with np.errstate(all="ignore"):
            op[k] |= (g >= RT_STAGE["e1"]) & (np.abs(q.e1 - q.th2) <= margins["e"] * q.th2)
            op[k] |= (g >= RT_STAGE["e2"]) & (np.abs(q.e2 - q.th2) <= margins["e"] * q.th2)
            low = q.cosP < COS_GATE                      # a depth gate is live; a cosP near its gate opens the match by itself
            op[k] |= (g >= RT_STAGE["z1"]) & low & (np.abs(q.z1) <= margins["z"])
            op[k] |= (g >= RT_STAGE["z2"]) & low & (np.abs(q.z2) <= margins["z"])
            op[k] |= (g >= 2) & (np.abs(q.cosP - COS_GATE) <= margins["cos"])
    return op


def rank_neighbours(r, k):
    """The parallax CheckRT would return for motion k had it taken rank want - 1 / want / want + 1 of the sorted cosines (None where the
    rank does not exist), want = min(50, nGood - 1)."""
    srt = r.rt[k].sorted
    n = len(srt)
    if n == 0:
        return None, None, None
    want = min(50, n - 1)
    ft = srt.dtype.type
    return tuple(parallax_of(srt[j], ft) if 0 <= j < n else None for j in (want - 1, want, want + 1))


def unit(M):
    """A homogeneous matrix (or a batch) with unit Frobenius norm and a positive largest entry: what H21 / F21 are compared as."""
    M = np.asarray(M, f64)
    flat = M.reshape(M.shape[:-2] + (9,))
    with np.errstate(all="ignore"):
        flat = flat / np.sqrt((flat * flat).sum(axis=-1, keepdims=True))
    k = np.abs(np.nan_to_num(flat)).argmax(axis=-1)
    sgn = np.sign(np.take_along_axis(flat, k[..., None], axis=-1))
    return (flat * sgn).reshape(M.shape)


def measured_output_differences(names=CASES, case_fn=None):
    """max |float32 model - float64 model| of the best H21 / F21 (as unit()), R21, t21 and vP3D over the committed cases (or over
    `names` as `case_fn` makes them)."""
    w = dict(M=0.0, R=0.0, t=0.0, P=0.0)
    for n in names:
        _, _, a, b = (case_fn or case)(n)
        if a.bestH == b.bestH and a.bestH >= 0:
            w["M"] = max(w["M"], float(np.abs(unit(a.H21[a.bestH]) - unit(b.H21[b.bestH])).max()))
        if a.bestF == b.bestF and a.bestF >= 0:
            w["M"] = max(w["M"], float(np.abs(unit(a.F21[a.bestF]) - unit(b.F21[b.bestF])).max()))
        if a.ok and b.ok and a.best_motion == b.best_motion:
            w["R"] = max(w["R"], float(np.abs(a.R21 - b.R21).max()))
            w["t"] = max(w["t"], float(np.abs(a.t21 - b.t21).max()))
            both = a.vbTriangulated & b.vbTriangulated
            w["P"] = max(w["P"], float((np.abs(a.vP3D - b.vP3D)[both]).max()))
    return w


if __name__ == "__main__":
    d = measured_chi_difference()
    print("largest relative chi2 difference float32 / float64 in [th/2, 2 th] over the capped cases: %.3e -> delta = 4 x = %.3e" % (d, 4 * d))
    for n in CASES:
        _, _, o32, o64 = case(n)
        fl = flagged(o64, 4 * d)
        ok = (o32.masks == o64.masks).all(axis=2) | fl
        print("%-6s hypotheses %4d flagged %3d (%.2f %%) masks equal outside the flagged: %s; model %d / %d ok %s / %s" %
              (n, fl.size, fl.sum(), 100.0 * fl.mean(), bool(ok.all()), o32.model, o64.model, o32.ok, o64.ok))
    w = measured_output_differences()
    print("float32 - float64 model: unit H21 / F21 %.3e, R21 %.3e, t21 %.3e, vP3D %.3e (tolerances: 4 x)" % (w["M"], w["R"], w["t"], w["P"]))
