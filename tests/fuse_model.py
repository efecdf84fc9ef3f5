"""ORBmatcher::Fuse restated in numpy, statement by statement: the LocalMapping overload (S/ORBmatcher.cc:1395-1605, bRight = false)
and the Sim3 overload (:1607-1742), in float32 (what csrc/fuse.hip computes) and in float64 (the yardstick for `near`).

    records()      everything up to bestIdx / bestDist for every (keyframe, point) pair, against the state at entry: what the kernel
                   returns.  A record is `near` when a gate of the float64 evaluation lies within NEAR_REL of its threshold.
    rescore()      the host's rescoring of a record whose point has a new descriptor.
    Replay         :1431-1448 and :1569-1590 over plain arrays: occupancy per keyframe, observation counts, MapPoint::Replace
                   (S/MapPoint.cc:367-419) as index bookkeeping, ComputeDistinctiveDescriptors as a deterministic descriptor change.
    serial_fuse()  the reference's loop itself, pair by pair with the descriptors as they are at that moment (no records).

Arithmetic (csrc/fuse.hip header): p3Dc = Rcw p3Dw + tcw in T, k order; cv::norm with double accumulation; PO.dot(Pn) in double against
0.5 * dist3D; PredictScale through (T)log((double)ratio); Pinhole::project fx * x / z + cx left to right; the chi2 product in T against
the double literals 7.8 / 5.99.  With T = float64 every step is double."""
import numpy as np

from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import views

F32, F64 = np.float32, np.float64
TH_LOW = 50
CAP = capi.FUSE_CAND_CAP
GRID_COLS, GRID_ROWS = 64, 48                  # FRAME_GRID_COLS / ROWS, I/Frame.h
NEAR_REL = 1e-6
INT_MAX = 2 ** 31 - 1
(CANDIDATES, NEG_DEPTH, NOT_IN_IMAGE, DISTANCE, NORMAL, EMPTY_WINDOW, NO_CANDIDATE, SKIPPED) = range(8)

_POPC = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming(a, b):
    return int(_POPC[np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))].sum())


# ------------------------------------------------------------------ the keyframe as Fuse reads it

FX, FY, CX, CY = 458.0, 457.0, 367.0, 248.0
MB = 0.11
N_LEVELS, SCALE_FACTOR = 8, 1.2
BOUNDS = (0.0, 752.0, 0.0, 480.0)              # mnMinX, mnMaxX, mnMinY, mnMaxY


def build_grid(kps, bounds=BOUNDS):
    """Frame::AssignFeaturesToGrid / PosInGrid (S/Frame.cc:360-391, 699-709) as the KeyFrame copies it: CSR over cell = ix * 48 + iy,
    ascending feature index inside a cell; float32 as the frame computes it."""
    min_x, max_x, min_y, max_y = [F32(b) for b in bounds]
    w_inv, h_inv = F32(GRID_COLS) / (max_x - min_x), F32(GRID_ROWS) / (max_y - min_y)
    px = (kps["x"].astype(F32) - min_x) * w_inv
    py = (kps["y"].astype(F32) - min_y) * h_inv
    rnd = lambda a: np.where(a >= 0, np.floor(a.astype(F64) + 0.5), np.ceil(a.astype(F64) - 0.5)).astype(np.int64)   # roundf
    ix, iy = rnd(px), rnd(py)
    ok = (ix >= 0) & (ix < GRID_COLS) & (iy >= 0) & (iy < GRID_ROWS)
    cell = np.where(ok, ix * GRID_ROWS + iy, -1)
    start = np.zeros(GRID_COLS * GRID_ROWS + 1, np.int64)
    np.add.at(start, cell[ok] + 1, 1)
    start = np.cumsum(start)
    order = np.argsort(cell[ok], kind="stable")
    items = np.nonzero(ok)[0][order]
    return start, items, w_inv, h_inv


def keyframe(Rcw, tcw, n, scale_factor=SCALE_FACTOR):
    """An empty keyframe dict at pose [Rcw | tcw]; Ow as KeyFrame::SetPose forms it (-Rcw.t() * tcw, double accumulation).  The scale
    tables are the extractor's for `scale_factor`."""
    Tcw = np.concatenate([np.asarray(Rcw, F64), np.asarray(tcw, F64)[:, None]], 1).astype(F32)
    R, t = Tcw[:, :3].astype(F64), Tcw[:, 3].astype(F64)
    Ow = np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)]).astype(F32)
    sf = np.empty(N_LEVELS, F32); sf[0] = 1.0
    for i in range(1, N_LEVELS):
        sf[i] = sf[i - 1] * F32(scale_factor)
    sigma2 = sf * sf
    fx = F32(FX)
    return dict(kps=np.zeros(n, capi.KEYPOINT_DTYPE), desc=np.zeros((n, 32), np.uint8), uright=np.full(n, -1, F32), depth=np.full(n, -1, F32),
                Tcw=Tcw, Ow=Ow, Scw=None, fx=fx, fy=F32(FY), cx=F32(CX), cy=F32(CY), mb=F32(MB), mbf=F32(F32(MB) * fx), sf=sf,
                inv_sigma2=(F32(1.0) / sigma2).astype(F32), log_sf=F32(np.log(F32(scale_factor))), bounds=BOUNDS, scale_factor=scale_factor)


def finish(k):
    """(Re)builds the grid after the features have been set."""
    k["grid"] = build_grid(k["kps"], k["bounds"])
    return k


def pose_of(k, sim3, T):
    """Rcw, tcw, Ow in T.  Sim3 form: :1616-1620 as the library decomposes Scw (scw from row 0 in double, the entries scaled by
    (T)(1 / scw), Ow = -Rcw^T tcw accumulated in double)."""
    if not sim3:
        return k["Tcw"][:, :3].astype(T), k["Tcw"][:, 3].astype(T), k["Ow"].astype(T)
    S = np.asarray(k["Scw"], F32).reshape(4, 4)
    s0 = S[0, :3].astype(F64)
    scw = T(np.sqrt((s0[0] * s0[0] + s0[1] * s0[1]) + s0[2] * s0[2]))
    alpha = T(F64(1.0) / F64(scw))
    R = (S[:3, :3].astype(T) * alpha).astype(T)
    t = (S[:3, 3].astype(T) * alpha).astype(T)
    Rd, td = R.astype(F64), t.astype(F64)
    Ow = np.array([-((Rd[0, i] * td[0] + Rd[1, i] * td[1]) + Rd[2, i] * td[2]) for i in range(3)]).astype(T)
    return R, t, Ow


def _near(value, threshold, scale=None):
    s = max(abs(float(threshold)), abs(float(value)), 1e-30) if scale is None else float(scale)
    return abs(float(value) - float(threshold)) <= NEAR_REL * s


def features_in_area(k, x, y, r, T):
    """KeyFrame::GetFeaturesInArea, S/KeyFrame.cc:889-940 (NLeft == -1, bRight = false).  Returns (vIndices, near)."""
    start, items, w_inv, h_inv = k["grid"]
    min_x, _, min_y, _ = [T(b) for b in k["bounds"]]
    w_inv, h_inv = T(w_inv), T(h_inv)
    near = False
    qs = [(x - min_x - r) * w_inv, (x - min_x + r) * w_inv, (y - min_y - r) * h_inv, (y - min_y + r) * h_inv]
    for q in qs:                                                   # floor / ceil flip at an integer
        near = near or _near(q, np.rint(q), max(abs(float(q)), 1.0))
    nMinCellX = max(0, int(np.floor(qs[0])))
    if nMinCellX >= GRID_COLS:
        return [], near
    nMaxCellX = min(GRID_COLS - 1, int(np.ceil(qs[1])))
    if nMaxCellX < 0:
        return [], near
    nMinCellY = max(0, int(np.floor(qs[2])))
    if nMinCellY >= GRID_ROWS:
        return [], near
    nMaxCellY = min(GRID_ROWS - 1, int(np.ceil(qs[3])))
    if nMaxCellY < 0:
        return [], near
    out = []
    kx, ky = k["kps"]["x"], k["kps"]["y"]
    for ix in range(nMinCellX, nMaxCellX + 1):
        for iy in range(nMinCellY, nMaxCellY + 1):
            c = ix * GRID_ROWS + iy
            for j in items[start[c]:start[c + 1]]:
                distx, disty = T(kx[j]) - x, T(ky[j]) - y
                near = near or _near(abs(distx), r) or _near(abs(disty), r)
                if abs(distx) < r and abs(disty) < r:
                    out.append(int(j))
    return out, near


def evaluate_pair(k, pts, i, th, sim3, T, desc=None):
    """One (keyframe, point) pair up to bestIdx / bestDist.  Returns dict(status, best_idx, best_dist, level, cand (ALL gated
    candidates in vIndices order), near).  desc: the point's descriptor (default pts["desc"][i])."""
    init = INT_MAX if sim3 else 256
    out = dict(status=NEG_DEPTH, best_idx=-1, best_dist=init, level=-1, cand=[], near=False)
    R, t, Ow = pose_of(k, sim3, T)
    X = pts["pos"][i].astype(T)
    Pc = np.array([(R[a, 0] * X[0] + R[a, 1] * X[1] + R[a, 2] * X[2]) + t[a] for a in range(3)], T)   # cv::Mat product, k order
    out["near"] = _near(Pc[2], 0.0, np.abs(Pc).max())
    if Pc[2] < T(0.0):                                              # :1455 | :1648
        return out
    with np.errstate(all="ignore"):
        invz = T(1.0) / Pc[2]                                       # :1461
        u = T(k["fx"]) * Pc[0] / Pc[2] + T(k["cx"])                 # Pinhole::project
        v = T(k["fy"]) * Pc[1] / Pc[2] + T(k["cy"])
    min_x, max_x, min_y, max_y = [T(b) for b in k["bounds"]]
    out["status"] = NOT_IN_IMAGE
    out["near"] = out["near"] or _near(u, min_x, 752) or _near(u, max_x, 752) or _near(v, min_y, 480) or _near(v, max_y, 480)
    if not (u >= min_x and u < max_x and v >= min_y and v < max_y):   # KeyFrame::IsInImage, :1469 | :1659
        return out
    ur = u - T(k["mbf"]) * invz                                     # :1475
    max_raw = T(pts["max_dist"][i])
    maxDistance, minDistance = T(F32(1.2)) * max_raw, T(F32(0.8)) * T(pts["min_dist"][i])   # the float literals 1.2f / 0.8f
    PO = X - Ow
    POd = PO.astype(F64)
    dist3D = T(np.sqrt((POd[0] * POd[0] + POd[1] * POd[1]) + POd[2] * POd[2]))   # cv::norm
    out["status"] = DISTANCE
    out["near"] = out["near"] or _near(dist3D, minDistance) or _near(dist3D, maxDistance)
    if dist3D < minDistance or dist3D > maxDistance:                # :1483 | :1669
        return out
    Pn = pts["normal"][i].astype(T).astype(F64)
    dot = (POd[0] * Pn[0] + POd[1] * Pn[1]) + POd[2] * Pn[2]
    out["status"] = NORMAL
    out["near"] = out["near"] or _near(dot, 0.5 * F64(dist3D), F64(dist3D))
    if dot < 0.5 * F64(dist3D):                                     # :1492 | :1676
        return out
    ratio = max_raw / dist3D                                        # MapPoint::PredictScale, S/MapPoint.cc:629-644
    lg = T(np.log(F64(ratio)))
    q = lg / T(k["log_sf"])
    out["near"] = out["near"] or _near(q, np.rint(q), max(abs(float(q)), 1.0))
    n_levels = len(k["sf"])
    level = min(max(int(np.ceil(q)), 0), n_levels - 1)
    out["level"] = level
    r = T(th) * T(k["sf"][level])                                   # :1501 | :1684
    vIndices, nr = features_in_area(k, u, v, r, T)
    out["near"] = out["near"] or nr
    out["status"] = EMPTY_WINDOW
    if not vIndices:                                                # :1505 | :1688
        return out
    d = pts["desc"][i] if desc is None else desc
    best_dist, best_idx = init, -1
    for idx in vIndices:
        kp = k["kps"][idx]
        kpLevel = int(kp["octave"])
        if kpLevel < level - 1 or kpLevel > level:                  # :1526 | :1703
            continue
        if not sim3:
            ex, ey = u - T(kp["x"]), v - T(kp["y"])
            w = T(k["inv_sigma2"][kpLevel])
            if k["uright"][idx] >= 0:                               # :1529-1542
                er = ur - T(k["uright"][idx])
                e2 = ex * ex + ey * ey + er * er
                lim = 7.8
            else:                                                   # :1543-1553
                e2 = ex * ex + ey * ey
                lim = 5.99
            out["near"] = out["near"] or _near(F64(e2 * w), lim)
            if F64(e2 * w) > lim:
                continue
        out["cand"].append(idx)
        dist = hamming(d, k["desc"][idx])
        if dist < best_dist:                                        # :1561 | :1711
            best_dist, best_idx = dist, idx
    out["status"] = CANDIDATES if out["cand"] else NO_CANDIDATE
    out["best_idx"], out["best_dist"] = best_idx, best_dist
    return out


def records(kfs, pts, th, sim3, T, skip=None):
    """What orbm_fuse returns: (records K x P, cand K x P x CAP, all-candidates lists [k][i], near K x P)."""
    K, P = len(kfs), len(pts["pos"])
    rec = np.zeros((K, P), capi.FUSE_RECORD_DTYPE)
    cand = np.full((K, P, CAP), 0xFFFF, np.uint16)
    full = [[[] for _ in range(P)] for _ in range(K)]
    near = np.zeros((K, P), bool)
    for k in range(K):
        for i in range(P):
            if skip is not None and skip[k][i]:
                rec[k, i] = (SKIPPED, -1, INT_MAX if sim3 else 256, -1, 0)
                continue
            o = evaluate_pair(kfs[k], pts, i, th, sim3, T)
            rec[k, i] = (o["status"], o["best_idx"], o["best_dist"], o["level"], len(o["cand"]))
            c = o["cand"][:CAP]
            cand[k, i, :len(c)] = c
            full[k][i] = o["cand"]
            near[k, i] = o["near"]
    return rec, cand, full, near


def rescore(cand_list, kf_desc, desc, sim3=False):
    """The host's rescoring: first strict minimum over the gated candidates, from bestDist = 256 | INT_MAX."""
    best_dist, best_idx = (INT_MAX if sim3 else 256), -1
    for idx in cand_list:
        dist = hamming(desc, kf_desc[int(idx)])
        if dist < best_dist:
            best_dist, best_idx = dist, int(idx)
    return best_idx, best_dist


# ------------------------------------------------------------------ the serial part over plain arrays

class Replay:
    """The host objects Fuse touches, as arrays.  kf_mp[k][idx]: the point feature idx of keyframe k holds (-1: none); obs[p]: {k: idx};
    n_obs[p]: Observations() (2 for a stereo feature, S/MapPoint.cc:251-254); bad[p]; replaced[p]; desc[p]."""

    def __init__(self, kfs, kf_mp, desc):
        self.kfs = kfs
        self.kf_mp = [np.asarray(m, np.int64).copy() for m in kf_mp]
        self.desc = np.asarray(desc, np.uint8).copy()
        P = len(self.desc)
        self.bad = np.zeros(P, bool)
        self.replaced = np.full(P, -1, np.int64)
        self.obs = [dict() for _ in range(P)]
        self.n_obs = np.zeros(P, np.int64)
        self.n_distinctive = np.zeros(P, np.int64)
        for k, m in enumerate(self.kf_mp):
            for idx, p in enumerate(m):
                if p >= 0:
                    self.add_observation(int(p), k, idx)

    def weight(self, k, idx):
        return 2 if self.kfs[k]["uright"][idx] >= 0 else 1

    def add_observation(self, p, k, idx):                            # S/MapPoint.cc:231-264: the index is overwritten, nObs grows
        self.obs[p][k] = idx
        self.n_obs[p] += self.weight(k, idx)

    def compute_distinctive_descriptors(self, p):
        """Stands in for MapPoint::ComputeDistinctiveDescriptors: a descriptor change that depends on the point's observations only."""
        self.n_distinctive[p] += 1
        ks = sorted(self.obs[p])
        if ks:
            k = ks[(len(ks) - 1) // 2]
            self.desc[p] = self.kfs[k]["desc"][self.obs[p][k]]

    def replace(self, a, b):                                         # a->Replace(b), S/MapPoint.cc:367-419
        if a == b:
            return
        obs, self.obs[a] = self.obs[a], dict()
        self.bad[a] = True
        self.replaced[a] = b
        for k in sorted(obs):
            idx = obs[k]
            if k not in self.obs[b]:
                self.kf_mp[k][idx] = b
                self.add_observation(b, k, idx)
            else:
                self.kf_mp[k][idx] = -1
        self.compute_distinctive_descriptors(b)

    def commit(self, k, p, best_idx, best_dist, limit=TH_LOW):
        """:1569-1590.  Returns 1 when nFused counts the pair."""
        if not best_dist <= limit:
            return 0
        q = int(self.kf_mp[k][best_idx])
        if q >= 0:
            if not self.bad[q]:
                if self.n_obs[q] > self.n_obs[p]:
                    self.replace(p, q)
                else:
                    self.replace(q, p)
        else:
            self.add_observation(p, k, best_idx)
            self.kf_mp[k][best_idx] = p
        return 1

    def skipped(self, k, p):                                         # :1431-1448
        return p < 0 or self.bad[p] or k in self.obs[p]

    def state(self):
        return ([m.tolist() for m in self.kf_mp], self.bad.tolist(), self.replaced.tolist(), self.n_obs.tolist(), self.desc.tolist(),
                [sorted(o.items()) for o in self.obs])


def replay_records(rp, k, point_ids, rec_k, cand_k, uploaded_desc, reeval, counters=None):
    """The glue's replay of one Fuse call over the records of keyframe k.  point_ids[i]: the point of list entry i (-1: NULL);
    uploaded_desc[i]: the 32 bytes the launch saw; reeval(i, desc) -> (best_idx, best_dist): the single-pair re-evaluation for a
    record with more than CAP candidates.  Returns nFused."""
    n_fused = 0
    for i, p in enumerate(point_ids):
        if rp.skipped(k, int(p)):
            continue
        r = rec_k[i]
        if r["status"] != CANDIDATES:
            continue
        best_idx, best_dist = int(r["best_idx"]), int(r["best_dist"])
        if not np.array_equal(rp.desc[p], uploaded_desc[i]):
            if r["n_cand"] > CAP:
                best_idx, best_dist = reeval(i, rp.desc[p])
                if counters is not None:
                    counters["relaunched"] = counters.get("relaunched", 0) + 1
            else:
                best_idx, best_dist = rescore(cand_k[i][: r["n_cand"]], rp.kfs[k]["desc"], rp.desc[p])
                if counters is not None:
                    counters["rescored"] = counters.get("rescored", 0) + 1
        n_fused += rp.commit(k, int(p), best_idx, best_dist)
    return n_fused


def serial_fuse(rp, k, point_ids, pts, th, T):
    """The reference's loop :1427-1592 itself over the Replay state: each pair is evaluated when its turn comes, with the point's
    descriptor as it is then."""
    n_fused = 0
    for i, p in enumerate(point_ids):
        if rp.skipped(k, int(p)):
            continue
        o = evaluate_pair(rp.kfs[k], pts, i, th, False, T, desc=rp.desc[p])
        if o["status"] != CANDIDATES:
            continue
        n_fused += rp.commit(k, int(p), o["best_idx"], o["best_dist"])
    return n_fused


# ------------------------------------------------------------------ scenes

def _rot(rng, deg):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    a = np.deg2rad(deg) * rng.uniform(-1, 1)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def points(pos, normal, min_dist, max_dist, desc):
    return dict(pos=np.ascontiguousarray(pos, F32).reshape(-1, 3), normal=np.ascontiguousarray(normal, F32).reshape(-1, 3),
                min_dist=np.ascontiguousarray(min_dist, F32), max_dist=np.ascontiguousarray(max_dist, F32),
                desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32))


def make_scene(seed, K=3, n=200, P=200, stereo_fraction=0.5, depth=(2.0, 12.0), noise=1.0):
    """The scene family of the tests: P map points at `depth` metres in front of a current keyframe, K target keyframes 0.15-0.5 m
    away that observe n of them (noise px * scale of the octave, every eighth feature somewhere else), a mix of stereo and monocular
    features.  A point's distance range and normal are what UpdateNormalAndDepth would give for its reference observation; every
    fifth point gets a range or a normal that fails its gate in some keyframes.  Sim3 form: Scw = s * [Rcw | tcw] with s in
    [0.8, 1.25].  Returns (kfs, pts, kf_mp): kf_mp[k][idx] = the point feature idx of keyframe k holds (-1: none)."""
    rng = np.random.default_rng(7000 + seed)
    R1 = _rot(rng, 20)
    t1 = rng.normal(size=3) * 2
    C1 = -R1.T @ t1
    px = np.stack([rng.uniform(-60, 810, P), rng.uniform(-40, 520, P)], 1)      # some outside the image
    z = rng.uniform(depth[0], depth[1], P)
    z[rng.random(P) < 0.03] *= -1                                               # some behind the camera
    Xc = np.stack([(px[:, 0] - CX) / FX * z, (px[:, 1] - CY) / FY * z, z], 1)
    Xw = (Xc - t1) @ R1
    octave = rng.integers(0, N_LEVELS, P)
    sf = F64(SCALE_FACTOR) ** np.arange(N_LEVELS)
    PO = Xw - C1
    d0 = np.linalg.norm(PO, axis=1)
    max_dist = d0 * sf[octave]                                                  # S/MapPoint.cc:560-566
    min_dist = max_dist / sf[N_LEVELS - 1]
    normal = PO / d0[:, None]
    odd = rng.random(P) < 0.3
    shrink = odd & (rng.random(P) < 0.5)
    max_dist = np.where(shrink, max_dist * rng.uniform(0.3, 1.0, P), max_dist)
    min_dist = np.where(shrink & (rng.random(P) < 0.5), max_dist / sf[N_LEVELS - 1] * rng.uniform(1.0, 8.0, P), min_dist)
    flip = odd & ~shrink
    normal[flip] = np.stack([_rot(rng, 90) @ nv for nv in normal[flip]]) if flip.any() else normal[flip]
    base = rng.integers(0, 256, (P, 32), dtype=np.uint8)

    def noisy(b, flips):
        d = np.unpackbits(b, axis=1)
        for r in d:
            r[rng.choice(256, rng.integers(0, flips + 1), replace=False)] ^= 1
        return np.packbits(d, axis=1)

    pts = points(Xw, normal, min_dist, max_dist, noisy(base, 10))
    kfs, kf_mp = [], []
    for k in range(K):
        dirn = rng.normal(size=3); dirn[2] *= 0.3; dirn /= np.linalg.norm(dirn)
        C = C1 + R1.T @ dirn * rng.uniform(0.15, 0.5)
        R2 = _rot(rng, 4) @ R1
        kf = keyframe(R2, -R2 @ C, n)
        first = rng.permutation(P)[: max(n // 2, 1)]                             # half of the features observe a point a second time:
        src = np.concatenate([first, first[rng.integers(0, len(first), n - len(first))]]) if n > 1 else first[:n]   # windows hold several candidates
        src = src[rng.permutation(n)]
        Xk = Xw[src] @ kf["Tcw"][:, :3].astype(F64).T + kf["Tcw"][:, 3].astype(F64)
        zk = np.where(np.abs(Xk[:, 2]) < 0.1, 0.1, Xk[:, 2])
        dk = np.linalg.norm(Xw[src] - kf["Ow"].astype(F64), axis=1)
        lvl = np.clip(np.ceil(np.log(max_dist[src] / dk) / np.log(SCALE_FACTOR)) - (rng.random(n) < 0.5) + (rng.random(n) < 0.1) * 2, 0, N_LEVELS - 1).astype(int)
        s = sf[lvl]
        u = FX * Xk[:, 0] / zk + CX + rng.normal(size=n) * noise * s
        v = FY * Xk[:, 1] / zk + CY + rng.normal(size=n) * noise * s
        gross = (rng.random(n) < 0.125) | (zk <= 0.1)
        u[gross] = rng.uniform(-5, 757, gross.sum()); v[gross] = rng.uniform(-5, 485, gross.sum())
        kf["kps"]["x"], kf["kps"]["y"], kf["kps"]["octave"], kf["kps"]["size"] = u, v, lvl, 31 * s
        kf["kps"]["angle"] = rng.uniform(0, 360, n)
        st = (rng.random(n) < stereo_fraction) & (zk > 0.1)
        kf["depth"] = np.where(st, zk, -1).astype(F32)
        kf["uright"] = np.where(st, u - MB * FX / zk + rng.normal(size=n) * 0.5 * s, -1).astype(F32)
        kf["desc"] = noisy(pts["desc"][src], 75)
        sc = rng.uniform(0.8, 1.25)
        S = np.eye(4); S[:3, :3] = sc * kf["Tcw"][:, :3].astype(F64); S[:3, 3] = sc * kf["Tcw"][:, 3].astype(F64)
        kf["Scw"] = S.astype(F32)
        kfs.append(finish(kf))
        mp = np.full(n, -1, np.int64)
        holds = rng.random(n) < 0.4
        other = rng.integers(0, P, n)                                            # a keyframe holds a point once
        seen = set()
        for j in np.nonzero(holds)[0]:
            p = int(src[j]) if rng.random() < 0.3 else int(other[j])
            if p not in seen:
                seen.add(p); mp[j] = p
        kf_mp.append(mp)
    return kfs, pts, kf_mp


def low_scale_factor_scene(scale_factor=1.1, qs=(-1.5,), features=((367.0, 248.0, 0, -1.0, 0),)):
    """A keyframe at the origin whose pyramid has a scale factor below 1.2, and one point per entry of qs, 5 m in front of it, with
    mfMaxDistance = d * scale_factor^q.  The distance gate (:1483) only asks dist3D <= 1.2f * mfMaxDistance, i.e. ratio >= 1 / 1.2,
    while ceil(q) < 0 needs ratio <= 1 / mfScaleFactor: with a scale factor below 1.2 a point passes every gate with a NEGATIVE
    nScale, and PredictScale's `if(nScale<0) nScale = 0` acts.  features: (x, y, octave, uright, descriptor bits set)."""
    kf = keyframe(np.eye(3), np.zeros(3), len(features), scale_factor=scale_factor)
    for j, (x, y, o, ur, bits) in enumerate(features):
        kf["kps"][j]["x"], kf["kps"][j]["y"], kf["kps"][j]["octave"] = x, y, o
        kf["uright"][j] = ur
        d = np.zeros(256, np.uint8); d[:bits] = 1
        kf["desc"][j] = np.packbits(d)
    kf["Scw"] = np.eye(4, dtype=F32)
    n = len(qs)
    maxd = np.array([5.0 * scale_factor ** q for q in qs])
    pts = points(np.tile([0.0, 0.0, 5.0], (n, 1)), np.tile([0.0, 0.0, 1.0], (n, 1)), maxd / scale_factor ** 7, maxd, np.zeros((n, 32), np.uint8))
    return finish(kf), pts


def near_share(seed, sim3, **kw):
    kfs, pts, _ = make_scene(seed, **kw)
    _, _, _, near = records(kfs, pts, 3.0, sim3, F64)
    return near.mean()


# ------------------------------------------------------------------ the device side

def device_keyframe(k, device=0, sim3=False):
    """The keyframe dict resident on the device: an api.FuseKeyFrame over an uploaded api.Frame."""
    from multi_orbslam3_amd import api
    fvw, keep = views.frame_view(k["kps"], k["desc"], k["uright"], k["depth"], bounds=k["bounds"],
                                 cam=(k["fx"], k["fy"], k["cx"], k["cy"], k["mbf"], k["mb"]), n_levels=len(k["sf"]), scale_factor=k["scale_factor"])
    fr = api.Frame(max(len(k["kps"]), 1), device).upload(fvw, keep)
    return api.FuseKeyFrame(fr, (k["fx"], k["fy"], k["cx"], k["cy"]), k["mbf"], k["sf"], k["inv_sigma2"], k["log_sf"], Tcw=k["Tcw"], Ow=k["Ow"],
                            Scw=k["Scw"] if sim3 else None)


def device_points(pts):
    P = len(pts["pos"])
    return views.worldpoints_view(pts["pos"], pts["normal"], pts["min_dist"], pts["max_dist"], pts["desc"], np.zeros(P, np.int32), np.zeros(P, np.uint8))
