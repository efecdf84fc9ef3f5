"""numpy restatement of ORBmatcher::SearchForTriangulation (S/ORBmatcher.cc:961-1202) + the triangulation loop of
LocalMapping::CreateNewMapPoints (S/LocalMapping.cc:616-863) + the serial bookkeeping across neighbours: the checker of
multi_orbslam3_amd/csrc/newpoints.hip.  Test infrastructure, never used by the product.

Every function takes the number type T.  With T = np.float32 the matcher performs exactly the operations the header of newpoints.hip
lists (N-1 .. N-7, N-9): float32 elementary operations, float64 where the reference's C++ promotes or where cv::gemm / dot / norm
accumulate, one rounding where they round.  With T = np.float64 every rounding is the identity: that is the float64 evaluation of the
same formulas on the same float32 inputs, and it also reports how close each gate came to its threshold.
The one step that is not pinned (N-8, cv::SVD::compute of the 4 x 4 A) is numpy's SVD of A here.  numpy.linalg computes in double
whatever the input type and rounds the result, so in the float32 model the null vector is the float64 one of the FLOAT32 matrix A,
rounded to float32 -- which is what the kernel's choice (the smallest eigenvector of A^T A in float64; null="eigh" restates it)
amounts to; the float32 model's distance from the float64 model is then the rounding of A and of what follows, nothing else.
A keyframe is a dict: kps (KEYPOINT_DTYPE: mvKeysUn), desc (n x 32), uright, depth, has_mp, Tcw / Twc (3 x 4), Ow, fx fy cx cy invfx
invfy mb mbf, sf (mvScaleFactors), sigma2 (mvLevelSigma2), scale_factor, fv = (node_id, start, feat_idx), keys_xy (or None)."""
import numpy as np

from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import views

TH_LOW = 50
HISTO_LENGTH = 30
(ACCEPTED, HAS_POINT, NOT_STEREO, NO_NODE, NO_MATCH, W_ZERO, LOW_PARALLAX, EMPTY, Z1, Z2, REPROJ1, REPROJ2, DIST_ZERO, FAR,
 SCALE) = range(15)
F64 = np.float64
_POPC = np.array([bin(i).count("1") for i in range(256)], np.int64)


def params(only_stereo=False, coarse=False, check_orientation=False, far_points=False, th_far_points=0.0):
    return dict(only_stereo=bool(only_stereo), coarse=bool(coarse), check_orientation=bool(check_orientation),
                far_points=bool(far_points), th_far_points=np.float32(th_far_points))


def hamming(a, b):
    return _POPC[np.bitwise_xor(a, b)].sum(-1)


def dot3(a, b, T, add=None):
    """N-2 / N-3: three products summed in float64 in k order (+ add, in float64), rounded once to T."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    s = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    if add is not None:
        s = s + np.asarray(add, F64)
    return s.astype(T)


def gemm33(A, B, T):
    return dot3(A[:, None, :], B.T[None, :, :], T)


def inv33(S, T):
    """N-4: cv::invert of a 3 x 3: cofactors and determinant in float64, d = 1 / det, one rounding per entry."""
    s = np.asarray(S, F64)
    d = s[0, 0] * (s[1, 1] * s[2, 2] - s[1, 2] * s[2, 1]) - s[0, 1] * (s[1, 0] * s[2, 2] - s[1, 2] * s[2, 0]) + \
        s[0, 2] * (s[1, 0] * s[2, 1] - s[1, 1] * s[2, 0])
    if d == 0:
        return np.zeros((3, 3), T)
    d = 1. / d
    t = [(s[1, 1] * s[2, 2] - s[1, 2] * s[2, 1]) * d, (s[0, 2] * s[2, 1] - s[0, 1] * s[2, 2]) * d, (s[0, 1] * s[1, 2] - s[0, 2] * s[1, 1]) * d,
         (s[1, 2] * s[2, 0] - s[1, 0] * s[2, 2]) * d, (s[0, 0] * s[2, 2] - s[0, 2] * s[2, 0]) * d, (s[0, 2] * s[1, 0] - s[0, 0] * s[1, 2]) * d,
         (s[1, 0] * s[2, 1] - s[1, 1] * s[2, 0]) * d, (s[0, 1] * s[2, 0] - s[0, 0] * s[2, 1]) * d, (s[0, 0] * s[1, 1] - s[0, 1] * s[1, 0]) * d]
    return np.array(t, F64).reshape(3, 3).astype(T)


def pair_geometry(k1, k2, T):
    """The epipole (S/ORBmatcher.cc:968-973), R12 / t12 (:987-988) and F12 (S/CameraModels/Pinhole.cpp:123-126)."""
    R1w, t1w = k1["Tcw"][:, :3].astype(T), k1["Tcw"][:, 3].astype(T)
    R2w, t2w = k2["Tcw"][:, :3].astype(T), k2["Tcw"][:, 3].astype(T)
    C2 = dot3(R2w, k1["Ow"].astype(T)[None, :], T, add=t2w)
    fx2, fy2, cx2, cy2 = [T(k2[c]) for c in ("fx", "fy", "cx", "cy")]
    fx1, fy1, cx1, cy1 = [T(k1[c]) for c in ("fx", "fy", "cx", "cy")]
    with np.errstate(all="ignore"):
        ep = np.array([fx2 * C2[0] / C2[2] + cx2, fy2 * C2[1] / C2[2] + cy2], T)
    R12 = gemm33(R1w, R2w.T, T)
    t12 = dot3(-R12, t2w[None, :], T, add=t1w)
    z = T(0)
    t12x = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], T)
    K1t = np.array([[fx1, 0, 0], [0, fy1, 0], [cx1, cy1, 1]], T)
    K2 = np.array([[fx2, 0, cx2], [0, fy2, cy2], [0, 0, 1]], T)
    F12 = gemm33(gemm33(gemm33(inv33(K1t, T), t12x, T), R12, T), inv33(K2, T), T)
    return F12, ep


def _level(o):
    return np.clip(o, 0, 15)


def _pad16(a):
    out = np.zeros(16, np.float32)
    out[: len(a)] = a
    return out


def candidate_ranges(fv1, fv2, n1):
    """The merge-join of the two feature vectors: per idx1 the [begin, end) of its node's list in KF2 (-1: no common node)."""
    rng = np.full((n1, 2), -1, np.int64)
    n2 = {int(nid): j for j, nid in enumerate(fv2[0])}
    for i, nid in enumerate(fv1[0]):
        j = n2.get(int(nid))
        if j is None:
            continue
        rng[fv1[2][fv1[1][i]: fv1[1][i + 1]]] = (fv2[1][j], fv2[1][j + 1])
    return rng


def match(k1, k2, p, T):
    """SearchForTriangulation's loops :1021-1155 for every idx1 independently.  Returns idx2 (-1), dist, status (HAS_POINT .. NO_MATCH,
    or ACCEPTED for a match) and `near`: a candidate's epipole distance or epipolar dsqr came within 1e-6 relative of its threshold."""
    n1 = len(k1["kps"])
    idx2 = np.full(n1, -1, np.int64); dist = np.zeros(n1, np.int64); near = np.zeros(n1, bool)
    rng = candidate_ranges(k1["fv"], k2["fv"], n1)
    st1_all = k1["uright"] >= 0
    status = np.full(n1, NO_MATCH, np.int64)
    status[p["only_stereo"] & ~st1_all] = NOT_STEREO
    status[rng[:, 0] < 0] = NO_NODE
    status[k1["has_mp"] != 0] = HAS_POINT
    live = np.nonzero((status == NO_MATCH) & (rng[:, 1] > rng[:, 0]))[0]
    if len(live) == 0:
        return idx2, dist, status, near
    cnt = rng[live, 1] - rng[live, 0]
    i1 = np.repeat(live, cnt)
    pos = np.concatenate([np.arange(c) for c in cnt])
    i2 = k2["fv"][2][rng[i1, 0] + pos].astype(np.int64)
    F12, ep = pair_geometry(k1, k2, T)
    st1, st2 = st1_all[i1], k2["uright"][i2] >= 0
    pre = k2["has_mp"][i2] == 0
    if p["only_stereo"]:
        pre &= st2
    d = hamming(k1["desc"][i1], k2["desc"][i2])
    pre &= d <= TH_LOW
    x1, y1 = k1["kps"]["x"][i1].astype(T), k1["kps"]["y"][i1].astype(T)
    x2, y2 = k2["kps"]["x"][i2].astype(T), k2["kps"]["y"][i2].astype(T)
    o2 = _level(k2["kps"]["octave"][i2])
    with np.errstate(all="ignore"):
        distex, distey = ep[0] - x2, ep[1] - y2
        lhs = distex * distex + distey * distey
        thr = T(100) * _pad16(k2["sf"]).astype(T)[o2]                       # int * float: a float product (N-1)
        mono = ~st1 & ~st2
        ok = pre & ~(mono & (lhs < thr))
        near_c = pre & mono & (np.abs(lhs.astype(F64) - thr) <= 1e-6 * thr)
        a = x1 * F12[0, 0] + y1 * F12[1, 0] + F12[2, 0]
        b = x1 * F12[0, 1] + y1 * F12[1, 1] + F12[2, 1]
        c = x1 * F12[0, 2] + y1 * F12[1, 2] + F12[2, 2]
        num = a * x2 + b * y2 + c
        den = a * a + b * b
        dsqr = num * num / den
        thr2 = 3.84 * _pad16(k2["sigma2"]).astype(T)[o2].astype(F64)
        if not p["coarse"]:
            near_c |= ok & (np.abs(dsqr.astype(F64) - thr2) <= 1e-6 * thr2)
            ok &= (den != 0) & (dsqr.astype(F64) < thr2)
    np.logical_or.at(near, i1, near_c)
    key = (d << 40) | ((0xFFFFF - pos) << 20) | i2                          # smallest distance, last list position on ties
    best = np.full(n1, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(best, i1[ok], key[ok])
    got = best != np.iinfo(np.int64).max
    idx2[got] = best[got] & 0xFFFFF
    dist[got] = best[got] >> 40
    status[got] = ACCEPTED
    return idx2, dist, status, near


def _cos_stereo(mb, depth, T):
    """N-7: cos(2 * atan2(mb / 2, depth)) through the float overloads."""
    with np.errstate(all="ignore"):
        ang = np.arctan2(F64(T(mb) / T(2)), depth.astype(F64)).astype(T)
        return np.cos((T(2) * ang).astype(F64)).astype(T)


def _unproject_stereo(k, i, T):
    z = k["depth"][i].astype(T)
    xy = k["keys_xy"][i] if k.get("keys_xy") is not None else np.stack([k["kps"]["x"][i], k["kps"]["y"][i]], 1)
    u, v = xy[:, 0].astype(T), xy[:, 1].astype(T)
    c = np.stack([(u - T(k["cx"])) * z * T(k["invfx"]), (v - T(k["cy"])) * z * T(k["invfy"]), z], 1)
    Twc = k["Twc"].astype(T)
    return dot3(Twc[None, :, :3], c[:, None, :], T, add=Twc[None, :, 3]), z > 0


def _reproj(k, mbf, X, z, stereo, kp, ur, T):
    Tcw = k["Tcw"].astype(T)
    sigma = _pad16(k["sigma2"]).astype(T)[_level(kp["octave"])]
    x, y = dot3(Tcw[0, :3], X, T, add=Tcw[0, 3]), dot3(Tcw[1, :3], X, T, add=Tcw[1, 3])
    fx, fy, cx, cy = [T(k[c]) for c in ("fx", "fy", "cx", "cy")]
    kx, ky = kp["x"].astype(T), kp["y"].astype(T)
    with np.errstate(all="ignore"):
        invz = (1.0 / z.astype(F64)).astype(T)
        ex, ey = (fx * x / z + cx) - kx, (fy * y / z + cy) - ky
        lhs_m, thr_m = ex * ex + ey * ey, 5.991 * sigma.astype(F64)
        u = fx * x * invz + cx
        u_r = u - T(mbf) * invz
        v = fy * y * invz + cy
        ex, ey, er = u - kx, v - ky, u_r - ur.astype(T)
        lhs_s, thr_s = ex * ex + ey * ey + er * er, 7.8 * sigma.astype(F64)
        lhs, thr = np.where(stereo, lhs_s, lhs_m).astype(F64), np.where(stereo, thr_s, thr_m)
        return lhs > thr, np.abs(lhs - thr) <= 1e-3 * thr


def triangulate(k1, k2, i1, i2, p, T, null="svd"):
    """S/LocalMapping.cc:707-844 for the pairs (i1[k], i2[k]).  Returns status, x3D, w, cosParallaxRays and `undecided`: a gate the
    evaluation reached lies within 1e-3 relative (reprojection, scale ratio) or 1e-6 absolute (the cosine gates) of its threshold."""
    m = len(i1)
    status = np.full(m, -1, np.int64)
    und = np.zeros(m, bool)
    kp1, kp2 = k1["kps"][i1], k2["kps"][i2]
    ur1, ur2 = k1["uright"][i1], k2["uright"][i2]
    st1, st2 = ur1 >= 0, ur2 >= 0
    Tcw1, Tcw2 = k1["Tcw"].astype(T), k2["Tcw"].astype(T)
    one = np.ones(m, T)
    with np.errstate(all="ignore"):
        xn1 = np.stack([(kp1["x"].astype(T) - T(k1["cx"])) / T(k1["fx"]), (kp1["y"].astype(T) - T(k1["cy"])) / T(k1["fy"]), one], 1)
        xn2 = np.stack([(kp2["x"].astype(T) - T(k2["cx"])) / T(k2["fx"]), (kp2["y"].astype(T) - T(k2["cy"])) / T(k2["fy"]), one], 1)
        ray1 = dot3(Tcw1[:, :3].T[None], xn1[:, None, :], T)
        ray2 = dot3(Tcw2[:, :3].T[None], xn2[:, None, :], T)
        cosr = (dot3(ray1, ray2, F64) / (np.sqrt(dot3(ray1, ray1, F64)) * np.sqrt(dot3(ray2, ray2, F64)))).astype(T)
        cs = cosr + T(1)
        c1 = np.where(st1, _cos_stereo(k1["mb"], k1["depth"][i1], T), cs)
        c2 = np.where(~st1 & st2, _cos_stereo(k2["mb"], k2["depth"][i2], T), cs)
        cst = np.minimum(c1, c2)
        tri = (cosr < cst) & (cosr > 0) & (st1 | st2 | (cosr.astype(F64) < 0.9998))
        und |= (np.abs(cosr.astype(F64) - cst) < 1e-6) | (np.abs(cosr.astype(F64)) < 1e-6)
        und |= ~st1 & ~st2 & (np.abs(cosr.astype(F64) - 0.9998) < 1e-6)
        us1 = ~tri & st1 & (c1 < c2)
        us2 = ~tri & ~us1 & st2 & (c2 < c1)
        und |= ~tri & (st1 | st2) & (np.abs(c1.astype(F64) - c2) < 1e-6)
        status[~tri & ~us1 & ~us2] = LOW_PARALLAX
        # linear triangulation (N-5, N-8, N-6)
        A = np.stack([xn1[:, 0:1] * Tcw1[2][None] - Tcw1[0][None], xn1[:, 1:2] * Tcw1[2][None] - Tcw1[1][None],
                      xn2[:, 0:1] * Tcw2[2][None] - Tcw2[0][None], xn2[:, 1:2] * Tcw2[2][None] - Tcw2[1][None]], 1)
        if null == "svd":
            v = np.linalg.svd(np.where(np.isfinite(A), A, 0))[2][:, 3, :] if m else np.zeros((0, 4), T)
        else:
            Ad = A.astype(F64)
            v = np.linalg.eigh(np.einsum("mki,mkj->mij", Ad, Ad))[1][:, :, 0] if m else np.zeros((0, 4))
        v = v.astype(T)
        w = np.where(tri, v[:, 3], T(0)).astype(T)
        Xt = v[:, :3] * (1.0 / v[:, 3].astype(F64)).astype(T)[:, None]
        status[tri & (v[:, 3] == 0) & (status < 0)] = W_ZERO
        X1, ok1 = _unproject_stereo(k1, i1, T)
        X2, ok2 = _unproject_stereo(k2, i2, T)
        status[(us1 & ~ok1) | (us2 & ~ok2)] = EMPTY
        X = np.where(tri[:, None], Xt, np.where(us1[:, None], X1, X2)).astype(T)
        formed = status < 0

        def gate(fail, code, near=None):
            reached = status < 0
            status[reached & fail] = code
            if near is not None:
                und[reached & near] = True

        z1 = dot3(Tcw1[2, :3], X, T, add=Tcw1[2, 3]); gate(z1 <= 0, Z1)
        z2 = dot3(Tcw2[2, :3], X, T, add=Tcw2[2, 3]); gate(z2 <= 0, Z2)
        f, nr = _reproj(k1, k1["mbf"], X, z1, st1, kp1, ur1, T); gate(f, REPROJ1, nr)
        f, nr = _reproj(k2, k1["mbf"], X, z2, st2, kp2, ur2, T); gate(f, REPROJ2, nr)          # KF1's mbf for KF2 too (:818)
        nv1, nv2 = X - k1["Ow"].astype(T)[None], X - k2["Ow"].astype(T)[None]
        d1, d2 = np.sqrt(dot3(nv1, nv1, F64)).astype(T), np.sqrt(dot3(nv2, nv2, F64)).astype(T)
        gate((d1 == 0) | (d2 == 0), DIST_ZERO)
        if p["far_points"]:
            gate((d1 >= T(p["th_far_points"])) | (d2 >= T(p["th_far_points"])), FAR)
        rd = d2 / d1
        ro = _pad16(k1["sf"]).astype(T)[_level(kp1["octave"])] / _pad16(k2["sf"]).astype(T)[_level(kp2["octave"])]
        rf = T(np.float32(1.5) * np.float32(k1["scale_factor"]))
        lo, hi = rd * rf, ro * rf
        gate((lo < ro) | (rd > hi), SCALE, (np.abs(lo.astype(F64) - ro) <= 1e-3 * ro) | (np.abs(rd.astype(F64) - hi) <= 1e-3 * hi))
        status[status < 0] = ACCEPTED
    X = np.where(formed[:, None], X, T(0)).astype(T)
    return status, X, w, cosr, und


def records(k1, nbs, p, T, null="svd"):
    """The B x n1 records of a call, with the model's flags: near (match stage) and undecided (triangulation stage)."""
    n1, B = len(k1["kps"]), len(nbs)
    rec = np.zeros((B, n1), capi.NEWPOINTS_RECORD_DTYPE)
    x3d = np.zeros((B, n1, 3), T)
    near, und = np.zeros((B, n1), bool), np.zeros((B, n1), bool)
    for b, k2 in enumerate(nbs):
        idx2, dist, status, near[b] = match(k1, k2, p, T)
        i1 = np.nonzero(idx2 >= 0)[0]
        st, X, w, cosr, u = triangulate(k1, k2, i1, idx2[i1], p, T, null)
        status[i1] = st
        rec["idx2"][b], rec["dist"][b], rec["status"][b] = idx2, dist, status
        rec["x3D"][b][i1], rec["w"][b][i1], rec["cos_parallax"][b][i1] = X, w, cosr
        x3d[b][i1] = X
        und[b][i1] = u
    return rec, x3d, near, und


def rot_bin(a1, a2):
    """S/ORBmatcher.cc:1145-1150 with factor = 1.0f / HISTO_LENGTH."""
    rot = np.float32(a1) - np.float32(a2)
    if rot < 0.0:
        rot = np.float32(rot + np.float32(360.0))
    x = float(np.float32(rot * np.float32(np.float32(1.0) / np.float32(HISTO_LENGTH))))
    b = int(np.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)                  # std::round: halves away from zero
    return 0 if b == HISTO_LENGTH else b


def three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima, S/ORBmatcher.cc:2312-2353."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1, ind3, ind2, ind1 = max2, max1, s, ind2, ind1, i
        elif s > max2:
            max3, max2, ind3, ind2 = max2, s, ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif max3 < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def replay(rec, has_mp1, check_orientation=False, angle1=None, angles2=None):
    """The serial part of CreateNewMapPoints over the B x n1 records, in plain Python: per neighbour drop what an earlier neighbour
    has claimed (S/ORBmatcher.cc:1029-1035), vote (:1143-1189), walk the survivors in ascending idx1 (:1194-1199); an accepted record
    creates a point and claims idx1 (S/LocalMapping.cc:847-852).  Returns (out list of (b, idx1, idx2, x3D), matches B x n1)."""
    B, n1 = rec.shape
    claimed = [bool(v) for v in has_mp1]
    out, matches = [], np.full((B, n1), -1, np.int32)
    for b in range(B):
        m12 = [int(rec["idx2"][b, i]) if (rec["idx2"][b, i] >= 0 and not claimed[i]) else -1 for i in range(n1)]
        if check_orientation:
            hist = [[] for _ in range(HISTO_LENGTH)]
            for i in range(n1):
                if m12[i] >= 0:
                    hist[rot_bin(angle1[i], angles2[b][m12[i]])].append(i)
            keep = three_maxima([len(h) for h in hist])
            for k, h in enumerate(hist):
                if k not in keep:
                    for i in h:
                        m12[i] = -1
        for i in range(n1):
            if m12[i] >= 0 and rec["status"][b, i] == ACCEPTED:
                out.append((b, i, m12[i], rec["x3D"][b, i].copy()))
                claimed[i] = True
        matches[b] = m12
    return out, matches


def search_for_triangulation(k1, k2, p, T=np.float32):
    """vMatchedPairs of one SearchForTriangulation call."""
    idx2, _, _, _ = match(k1, k2, p, T)
    m12 = [int(v) for v in idx2]
    if p["check_orientation"]:
        hist = [[] for _ in range(HISTO_LENGTH)]
        for i, j in enumerate(m12):
            if j >= 0:
                hist[rot_bin(k1["kps"]["angle"][i], k2["kps"]["angle"][j])].append(i)
        keep = three_maxima([len(h) for h in hist])
        for k, h in enumerate(hist):
            if k not in keep:
                for i in h:
                    m12[i] = -1
    return np.array([(i, j) for i, j in enumerate(m12) if j >= 0], np.int32).reshape(-1, 2)


# ------------------------------------------------------------------ scenes

FX, FY, CX, CY = 458.0, 457.0, 367.0, 248.0
MB = 0.11
N_LEVELS, SCALE_FACTOR = 8, 1.2


def _rot(rng, deg):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    a = np.deg2rad(deg) * rng.uniform(-1, 1)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def keyframe(Rcw, tcw, n):
    """An empty keyframe dict at pose [Rcw | tcw]; Twc / Ow as KeyFrame::SetPose forms them (Rwc = Rcw.t(), Ow = -Rwc * tcw, N-2)."""
    Tcw = np.concatenate([Rcw, tcw[:, None]], 1).astype(np.float32)
    Rwc = Tcw[:, :3].T.copy()
    Ow = (-dot3(Rwc, Tcw[None, :, 3], F64)).astype(np.float32)
    sf = np.empty(N_LEVELS, np.float32); sf[0] = 1.0
    for i in range(1, N_LEVELS):
        sf[i] = sf[i - 1] * np.float32(SCALE_FACTOR)
    fx, fy = np.float32(FX), np.float32(FY)
    return dict(kps=np.zeros(n, capi.KEYPOINT_DTYPE), desc=np.zeros((n, 32), np.uint8), uright=np.full(n, -1, np.float32),
                depth=np.full(n, -1, np.float32), has_mp=np.zeros(n, np.uint8), Tcw=Tcw, Twc=np.concatenate([Rwc, Ow[:, None]], 1),
                Ow=Ow, fx=fx, fy=fy, cx=np.float32(CX), cy=np.float32(CY), invfx=np.float32(1.0) / fx, invfy=np.float32(1.0) / fy,
                mb=np.float32(MB), mbf=np.float32(np.float32(MB) * fx), sf=sf, sigma2=sf * sf, scale_factor=np.float32(SCALE_FACTOR),
                fv=views.featvec_from_nodes(np.zeros(n, np.int64)), keys_xy=None)


def set_nodes(k, node):
    """mFeatVec of keyframe k from the vocabulary node of every feature (kept as k["node"])."""
    k["node"] = np.asarray(node, np.int64).copy()
    if len(k["node"]):
        k["fv"] = views.featvec_from_nodes(k["node"])
    else:
        k["fv"] = (np.zeros(0, np.uint32), np.zeros(1, np.uint32), np.zeros(0, np.uint32))


def copy_feature(k, src, dst):
    """Feature dst of keyframe k becomes a copy of feature src (keypoint, descriptor, stereo fields, map point flag, node)."""
    for f in ("kps", "desc", "uright", "depth", "has_mp"):
        k[f][dst] = k[f][src]
    node = k["node"].copy(); node[dst] = node[src]
    set_nodes(k, node)


def device_keyframe(k, device=0):
    """The keyframe dict resident on the device: an api.NewPointsKeyFrame over an uploaded api.Frame."""
    from multi_orbslam3_amd import api
    fvw, keep = views.frame_view(k["kps"], k["desc"], k["uright"], k["depth"], bounds=(0.0, 752.0, 0.0, 480.0),
                                 cam=(k["fx"], k["fy"], k["cx"], k["cy"], k["mbf"], k["mb"]), n_levels=N_LEVELS, scale_factor=SCALE_FACTOR)
    fr = api.Frame(max(len(k["kps"]), 1), device).upload(fvw, keep)
    return api.NewPointsKeyFrame(fr, k["fv"], k["has_mp"], k["Tcw"], k["Twc"], k["Ow"], (k["fx"], k["fy"], k["cx"], k["cy"]), k["mb"],
                                 k["mbf"], k["sf"], k["sigma2"], k["scale_factor"], keys_xy=k.get("keys_xy"), invf=(k["invfx"], k["invfy"]))


def _observe(rng, k, Xw, octave, noise, stereo_fraction):
    """Fills kps / uright / depth of keyframe k with the projections of Xw (+ noise px * scale of the octave)."""
    n = len(Xw)
    Xc = Xw @ k["Tcw"][:, :3].astype(F64).T + k["Tcw"][:, 3].astype(F64)
    s = k["sf"].astype(F64)[octave]
    u = FX * Xc[:, 0] / Xc[:, 2] + CX + rng.normal(size=n) * noise * s
    v = FY * Xc[:, 1] / Xc[:, 2] + CY + rng.normal(size=n) * noise * s
    k["kps"]["x"], k["kps"]["y"], k["kps"]["octave"] = u, v, octave
    k["kps"]["size"] = 31 * s
    st = rng.random(n) < stereo_fraction
    z = Xc[:, 2] * (1 + rng.normal(size=n) * 0.002)
    k["depth"] = np.where(st, z, -1).astype(np.float32)
    k["uright"] = np.where(st, u - MB * FX / z, -1).astype(np.float32)
    return Xc


def make_scene(seed, n=200, B=3, n_nodes=25, noise=1.0, mismatch=0.15, stereo_fraction=0.5, has_mp_fraction=0.2, depth=(2.0, 12.0),
               baseline=(0.15, 0.5), n2=None):
    """The scene family of the tests: n points at `depth` metres seen by KF1 and by B neighbours `baseline` metres away; `noise`
    px * scale on every observation, a fraction `mismatch` of a neighbour's features moved somewhere else, `stereo_fraction` of the
    features with mvuRight / mvDepth.  Descriptors cluster around one centre per vocabulary node, so that a node holds several
    candidates under TH_LOW and the epipolar gates decide.  Returns (kf1, [neighbours])."""
    rng = np.random.default_rng(1000 + seed)
    R1 = _rot(rng, 20)
    k1 = keyframe(R1, rng.normal(size=3) * 2, n)
    octave = rng.integers(0, N_LEVELS, n)
    px = np.stack([rng.uniform(20, 730, n), rng.uniform(20, 470, n)], 1)
    z = rng.uniform(depth[0], depth[1], n)
    Xc = np.stack([(px[:, 0] - CX) / FX * z, (px[:, 1] - CY) / FY * z, z], 1)
    Xw = (Xc - k1["Tcw"][:, 3].astype(F64)) @ k1["Tcw"][:, :3].astype(F64)
    node = rng.integers(0, n_nodes, n) * 7 + 3
    centre = rng.integers(0, 256, (n_nodes * 7 + 3, 32), dtype=np.uint8)

    def descriptors(flips):
        d = np.unpackbits(centre[node], axis=1)
        for i in range(n):
            d[i, rng.choice(256, flips, replace=False)] ^= 1
        return np.packbits(d, axis=1)

    base = descriptors(18)

    def noisy(b, flips):
        d = np.unpackbits(b, axis=1)
        for i in range(len(d)):
            d[i, rng.choice(256, rng.integers(0, flips + 1), replace=False)] ^= 1
        return np.packbits(d, axis=1)

    _observe(rng, k1, Xw, octave, noise, stereo_fraction)
    k1["desc"] = noisy(base, 6)
    k1["kps"]["angle"] = rng.uniform(0, 360, n)
    k1["has_mp"] = (rng.random(n) < has_mp_fraction).astype(np.uint8)
    set_nodes(k1, node)
    nbs = []
    for b in range(B):
        m = n if n2 is None else n2[b]
        d = rng.normal(size=3); d[2] *= 0.3; d /= np.linalg.norm(d)
        C = k1["Ow"].astype(F64) + k1["Tcw"][:, :3].astype(F64).T @ d * rng.uniform(*baseline)
        R2 = _rot(rng, 4) @ R1
        k2 = keyframe(R2, -R2 @ C, m)
        if m:
            src = rng.permutation(n)[:m]                                     # feature j of the neighbour observes point src[j]
            oct2 = np.clip(octave[src] + rng.integers(-1, 2, m) * (rng.random(m) < 0.2), 0, N_LEVELS - 1)
            _observe(rng, k2, Xw[src], oct2, noise, stereo_fraction)
            bad = rng.random(m) < mismatch                                   # gross mismatches: the same descriptor somewhere else
            k2["kps"]["x"][bad] = rng.uniform(20, 730, bad.sum())
            k2["kps"]["y"][bad] = rng.uniform(20, 470, bad.sum())
            k2["uright"][bad & (k2["uright"] >= 0)] = (k2["kps"]["x"] - MB * FX / np.maximum(k2["depth"], 0.1))[bad & (k2["uright"] >= 0)]
            k2["desc"] = noisy(base[src], 6)
            rot = rng.uniform(0, 360)
            k2["kps"]["angle"] = np.where(rng.random(m) < 0.8, (k1["kps"]["angle"][src] - rot + rng.normal(size=m) * 4) % 360, rng.uniform(0, 360, m))
            k2["has_mp"] = (rng.random(m) < has_mp_fraction).astype(np.uint8)
            nd = np.where(rng.random(m) < 0.05, rng.integers(0, n_nodes + 3, m) * 7 + 3, node[src])
            set_nodes(k2, nd)
            k2["src"] = src
        else:
            set_nodes(k2, np.zeros(0, np.int64))
            k2["src"] = np.zeros(0, np.int64)
        nbs.append(k2)
    return k1, nbs


def parallax_band(cosr):
    """0: cosParallaxRays above 0.9998, 1: down to 0.998, 2: below."""
    c = np.asarray(cosr, F64)
    return np.where(c > 0.9998, 0, np.where(c >= 0.998, 1, 2))


def point_error(x, x64, k1):
    """Distance between two evaluations of a point, relative to its distance from KF1's centre."""
    x64 = np.asarray(x64, F64)
    return np.linalg.norm(np.asarray(x, F64) - x64, axis=-1) / np.linalg.norm(x64 - k1["Ow"].astype(F64), axis=-1)
