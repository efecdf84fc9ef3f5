"""ORBmatcher::SearchForInitialization (S/ORBmatcher.cc:702-817) with Frame::GetFeaturesInArea (S/Frame.cc:628-697) restated in numpy:
float32 cell arithmetic, the serial loop, the rotation vote.  `lists()` gathers the per-query candidate lists in the reference's
order, `replay()` applies the serial rules to lists wherever they come from (the device's, for instance), `search()` is both.
`brute_lists()` finds the same lists from all pairs.  The named cases of the tests live here too; every case is deterministic.

An entry of a list is  index2 | dist << 16."""
import numpy as np

F32 = np.float32
COLS, ROWS = 64, 48
INT_MAX = 2 ** 31 - 1
TH_LOW, HISTO_LENGTH = 50, 30
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def round_away(v):
    """roundf / std::round of a float32 value (half away from zero), exact through float64."""
    v = float(v)
    return int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


class Frame:
    """What the search reads of a monocular Frame: mvKeysUn, mDescriptors, the image bounds and mGrid."""

    def __init__(self, kps, desc, bounds=(0.0, 640.0, 0.0, 480.0)):
        self.kps = np.ascontiguousarray(kps, KP)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        assert len(self.kps) == len(self.desc)
        self.bounds = tuple(F32(b) for b in bounds)
        self.min_x, self.max_x, self.min_y, self.max_y = self.bounds
        self.w_inv = F32(COLS) / F32(self.max_x - self.min_x)             # S/Frame.cc:127-144
        self.h_inv = F32(ROWS) / F32(self.max_y - self.min_y)
        self.n = len(self.kps)
        self.cell_of = np.full(self.n, -1, np.int64)
        self.grid = [[] for _ in range(COLS * ROWS)]                      # Frame::AssignFeaturesToGrid / PosInGrid, :360-391, :699-709
        for i in range(self.n):
            px = round_away((self.kps["x"][i] - self.min_x) * self.w_inv)
            py = round_away((self.kps["y"][i] - self.min_y) * self.h_inv)
            if px < 0 or px >= COLS or py < 0 or py >= ROWS:
                continue
            self.cell_of[i] = px * ROWS + py
            self.grid[px * ROWS + py].append(i)

    @property
    def pts(self):
        return np.stack([self.kps["x"], self.kps["y"]], 1).astype(F32)


def cell_bounds(F, x, y, r):
    """S/Frame.cc:639-661 -> (nMinCellX, nMaxCellX, nMinCellY, nMaxCellY) or None at one of the four early returns."""
    x, y, r = F32(x), F32(y), F32(r)
    with np.errstate(all="ignore"):
        a0 = int(np.floor((x - F.min_x - r) * F.w_inv)); a1 = int(np.ceil((x - F.min_x + r) * F.w_inv))
        b0 = int(np.floor((y - F.min_y - r) * F.h_inv)); b1 = int(np.ceil((y - F.min_y + r) * F.h_inv))
    n_min_x = max(0, a0)
    if n_min_x >= COLS:
        return None
    n_max_x = min(COLS - 1, a1)
    if n_max_x < 0:
        return None
    n_min_y = max(0, b0)
    if n_min_y >= ROWS:
        return None
    n_max_y = min(ROWS - 1, b1)
    if n_max_y < 0:
        return None
    return n_min_x, n_max_x, n_min_y, n_max_y


def features_in_area(F, x, y, r, level=0):
    """Frame::GetFeaturesInArea(x, y, r, level, level): indices in the reference's order."""
    cb = cell_bounds(F, x, y, r)
    out = []
    if cb is None:
        return out
    x, y, r = F32(x), F32(y), F32(r)
    kx, ky, ko = F.kps["x"], F.kps["y"], F.kps["octave"]
    for ix in range(cb[0], cb[1] + 1):
        for iy in range(cb[2], cb[3] + 1):
            for i in F.grid[ix * ROWS + iy]:
                if ko[i] != level:
                    continue
                if abs(F32(kx[i] - x)) < r and abs(F32(ky[i] - y)) < r:       # strict, :690
                    out.append(i)
    return out


def hamming(d, D):
    return POP[np.bitwise_xor(D, d[None, :])].sum(1).astype(np.int64)


def _pack(per_query, n1):
    start = np.zeros(n1 + 1, np.int32)
    for i in range(n1):
        start[i + 1] = start[i] + (len(per_query[i]) if per_query[i] is not None else 0)
    ent = np.zeros(int(start[n1]), np.uint32)
    for i in range(n1):
        if per_query[i] is not None and len(per_query[i]):
            ent[start[i]: start[i + 1]] = per_query[i]
    return start, ent


def lists(F1, F2, prev, window):
    """-> (list_start (n1 + 1), entries): the candidates of every octave-0 feature of F1 around prev[i1] (NOT around the keypoint)."""
    prev = np.asarray(prev, F32).reshape(-1, 2)
    per = [None] * F1.n
    for i1 in range(F1.n):
        if F1.kps["octave"][i1] > 0:
            continue
        idx = features_in_area(F2, prev[i1, 0], prev[i1, 1], window)
        if idx:
            idx = np.asarray(idx, np.int64)
            per[i1] = (idx | (hamming(F1.desc[i1], F2.desc[idx]) << 16)).astype(np.uint32)
        else:
            per[i1] = np.zeros(0, np.uint32)
    return _pack(per, F1.n)


def brute_lists(F1, F2, prev, window):
    """The same lists from all pairs: every octave-0 feature of F2 whose cell lies inside the query's cell bounds and that passes the
    window test, sorted by (ix * 48 + iy, index)."""
    prev = np.asarray(prev, F32).reshape(-1, 2)
    per = [None] * F1.n
    lvl0 = np.nonzero((F2.kps["octave"] == 0) & (F2.cell_of >= 0))[0]
    cx, cy = F2.cell_of[lvl0] // ROWS, F2.cell_of[lvl0] % ROWS
    r = F32(window)
    for i1 in range(F1.n):
        if F1.kps["octave"][i1] > 0:
            continue
        per[i1] = np.zeros(0, np.uint32)
        cb = cell_bounds(F2, prev[i1, 0], prev[i1, 1], window)
        if cb is None:
            continue
        dx = np.abs((F2.kps["x"][lvl0] - prev[i1, 0]).astype(F32)); dy = np.abs((F2.kps["y"][lvl0] - prev[i1, 1]).astype(F32))
        ok = (cx >= cb[0]) & (cx <= cb[1]) & (cy >= cb[2]) & (cy <= cb[3]) & (dx < r) & (dy < r)
        idx = lvl0[ok]
        idx = idx[np.lexsort((idx, F2.cell_of[idx]))]
        if len(idx):
            per[i1] = (idx | (hamming(F1.desc[i1], F2.desc[idx]) << 16)).astype(np.uint32)
    return _pack(per, F1.n)


def rot_bin(a1, a2):
    rot = F32(a1) - F32(a2)
    if rot < 0.0:
        rot = F32(rot + F32(360.0))
    b = round_away(F32(rot * (F32(1.0) / F32(HISTO_LENGTH))))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima, S/ORBmatcher.cc:2312-2353."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if F32(max2) < F32(0.1) * F32(max1):
        ind2 = ind3 = -1
    elif F32(max3) < F32(0.1) * F32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def replay(list_start, entries, octave1, angle1, angle2, pts2, prev, nn_ratio=0.9, check_orientation=True, skip_rule=True):
    """S/ORBmatcher.cc:704-816 over given lists -> dict(nmatches, matches12, prev, n_queries, n_candidates, n_evictions,
    n_rot_rejected).  skip_rule=False leaves out `if (vMatchedDistance[i2] <= dist) continue;` (:741), to show that it matters."""
    n1, n2 = len(octave1), len(angle2)
    prev = np.array(prev, F32).reshape(-1, 2).copy()
    m12 = np.full(n1, -1, np.int32)
    m21 = np.full(n2, -1, np.int64)
    mdist = np.full(n2, INT_MAX, np.int64)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = n_queries = n_evictions = n_rot = 0
    for i1 in range(n1):
        if octave1[i1] > 0:
            continue
        n_queries += 1
        best, best2, best_idx = INT_MAX, INT_MAX, -1
        for e in entries[list_start[i1]: list_start[i1 + 1]]:
            i2, dist = int(e) & 0xFFFF, int(e) >> 16
            if skip_rule and mdist[i2] <= dist:
                continue
            if dist < best:
                best2, best, best_idx = best, dist, i2
            elif dist < best2:
                best2 = dist
        if best <= TH_LOW and F32(best) < F32(F32(best2) * F32(nn_ratio)):
            if m21[best_idx] >= 0:
                m12[m21[best_idx]] = -1
                nmatches -= 1
                n_evictions += 1
            m12[i1] = best_idx
            m21[best_idx] = i1
            mdist[best_idx] = best
            nmatches += 1
            if check_orientation:
                hist[rot_bin(angle1[i1], angle2[best_idx])].append(i1)            # an evicted i1 stays in its bin
    if check_orientation:
        keep = three_maxima([len(h) for h in hist])
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for i1 in hist[b]:
                if m12[i1] >= 0:
                    m12[i1] = -1
                    nmatches -= 1
                    n_rot += 1
    for i1 in range(n1):
        if m12[i1] >= 0:
            prev[i1] = pts2[m12[i1]]
    return dict(nmatches=nmatches, matches12=m12, prev=prev, n_queries=n_queries, n_candidates=int(list_start[n1]),
                n_evictions=n_evictions, n_rot_rejected=n_rot)


def search(F1, F2, prev, window=100, nn_ratio=0.9, check_orientation=True, skip_rule=True, given_lists=None):
    start, ent = given_lists if given_lists is not None else lists(F1, F2, prev, window)
    out = replay(start, ent, F1.kps["octave"], F1.kps["angle"], F2.kps["angle"], F2.pts, prev, nn_ratio, check_orientation, skip_rule)
    out["list_start"], out["entries"] = start, ent
    return out


# ------------------------------------------------------------------------------------------------ cases

def level_population(rng, n, n_levels=8, sf=1.2):
    """Octaves drawn like mnFeaturesPerLevel (S/ORBextractor.cc:429-441): a geometric share per level, level 0 about one in five."""
    w = np.array([(1.0 / sf) ** l for l in range(n_levels)])
    return rng.choice(n_levels, size=n, p=w / w.sum()).astype(np.int32)


def flip_bits(rng, d, k):
    d = d.copy()
    for b in rng.choice(256, size=k, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def make_kps(x, y, octave, angle):
    k = np.zeros(len(x), KP)
    k["x"], k["y"], k["octave"], k["angle"] = x, y, octave, angle
    k["size"] = (31.0 * 1.2 ** np.asarray(octave)).astype(np.int64)
    k["response"] = 20.0
    return k


def make_pair(seed, n1, n2, width=640, height=480, motion=30.0, dup=0.15, bounds=None):
    """F1 with random features; F2 sees min(n1, n2) of them again, moved by one image motion plus jitter, a few descriptor bits flipped,
    in another order, and n2 - n1 new ones.  dup of F1's features carry (almost) the descriptor of a neighbour: they compete for the
    same feature of F2, which is what evictions and the vMatchedDistance skip are about."""
    rng = np.random.default_rng(seed)
    x1 = rng.uniform(20, width - 20, n1).astype(F32); y1 = rng.uniform(20, height - 20, n1).astype(F32)
    o1 = level_population(rng, n1)
    a1 = rng.uniform(0, 360, n1).astype(F32)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    lvl0 = np.nonzero(o1 == 0)[0]
    for i in rng.choice(n1, int(dup * n1), replace=False):
        if o1[i] != 0 or len(lvl0) < 2:
            j = rng.integers(n1)
        else:                                                   # the nearest other octave-0 feature
            dd = (x1[lvl0] - x1[i]) ** 2 + (y1[lvl0] - y1[i]) ** 2
            dd[lvl0 == i] = np.inf
            j = lvl0[np.argmin(dd)]
        d1[i] = flip_bits(rng, d1[j], int(rng.integers(0, 3)))
    shift = rng.uniform(-motion, motion, 2) * 0.7
    m = min(n1, n2)
    seen = rng.permutation(n1)[:m]
    x2 = np.concatenate([x1[seen] + shift[0] + rng.normal(0, 1.5, m), rng.uniform(20, width - 20, n2 - m)]).astype(F32)
    y2 = np.concatenate([y1[seen] + shift[1] + rng.normal(0, 1.5, m), rng.uniform(20, height - 20, n2 - m)]).astype(F32)
    o2 = np.concatenate([o1[seen], level_population(rng, n2 - m)])
    rot = rng.uniform(-8, 8)
    a2 = np.concatenate([(a1[seen] + rot + rng.normal(0, 2, m)) % 360.0, rng.uniform(0, 360, n2 - m)]).astype(F32)
    a2[rng.random(n2) < 0.1] = F32(rng.uniform(0, 360))        # some angles disagree: the rotation vote has something to reject
    d2 = np.concatenate([np.stack([flip_bits(rng, d1[i], int(rng.integers(0, 25))) for i in seen]),
                         rng.integers(0, 256, (n2 - m, 32), dtype=np.uint8)])
    p = rng.permutation(n2)
    b = bounds or (0.0, float(width), 0.0, float(height))
    F1 = Frame(make_kps(x1, y1, o1, a1), d1, b)
    F2 = Frame(make_kps(x2[p], y2[p], o2[p], a2[p]), d2[p], b)
    return F1, F2


def case_small():
    F1, F2 = make_pair(11, 600, 670)
    return dict(F1=F1, F2=F2, prev=F1.pts, window=100)


def case_big():
    F1, F2 = make_pair(12, 4100, 4100)
    return dict(F1=F1, F2=F2, prev=F1.pts, window=100)


def case_crowded():
    """300 octave-0 features of F2 inside a 150 x 150 px square, 300 queries aimed at it, descriptors from 8 prototypes with <= 3 flipped
    bits: lists of 300 entries, ties everywhere."""
    rng = np.random.default_rng(21)
    proto = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    n = 300

    def side(extra):
        x = np.concatenate([rng.uniform(250, 400, n), rng.uniform(20, 620, extra)]).astype(F32)
        y = np.concatenate([rng.uniform(150, 300, n), rng.uniform(20, 460, extra)]).astype(F32)
        o = np.concatenate([np.zeros(n, np.int32), 1 + level_population(rng, extra, 7)])
        d = np.stack([flip_bits(rng, proto[rng.integers(8)], int(rng.integers(0, 4))) for _ in range(n + extra)])
        a = ((rng.integers(0, 3, n + extra) * 40.0) + rng.normal(0, 1, n + extra)) % 360.0
        p = rng.permutation(n + extra)
        return Frame(make_kps(x[p], y[p], o[p], a[p].astype(F32)), d[p])
    F1, F2 = side(40), side(57)
    return dict(F1=F1, F2=F2, prev=F1.pts, window=100)


def case_ties(nn_ratio=0.9):
    """Identical descriptors in F2 in the same cell, in another iy of the same ix and in another ix, with feature indices that run
    AGAINST the reference's order.  Cells are 10 x 10 px here."""
    rng = np.random.default_rng(31)
    D = rng.integers(0, 256, 32, dtype=np.uint8)
    other = rng.integers(0, 256, 32, dtype=np.uint8)
    # F2 (index: position): 0 (323, 203) cell (32, 20) | 1 (301, 222) cell (30, 22) | 2 (302, 201) cell (30, 20) | 3 (303, 202) same cell
    # reference order around (310, 210): ix 30: iy 20: 2, 3; iy 22: 1; ix 32: 0
    x2 = np.array([323, 301, 302, 303, 100, 500], F32); y2 = np.array([203, 222, 201, 202, 100, 400], F32)
    d2 = np.stack([D, D, D, D, other, flip_bits(rng, other, 40)])
    F2 = Frame(make_kps(x2, y2, np.zeros(6, np.int32), np.full(6, 10.0, F32)), d2)
    # F1: 0 sees the four copies at distance 7 each; 1 sees only feature 4, at distance 0; 2 sees nothing
    x1 = np.array([310, 100, 600], F32); y1 = np.array([210, 100, 50], F32)
    d1 = np.stack([flip_bits(rng, D, 7), other, D])
    F1 = Frame(make_kps(x1, y1, np.zeros(3, np.int32), np.full(3, 10.0, F32)), d1)
    return dict(F1=F1, F2=F2, prev=F1.pts, window=30, nn_ratio=nn_ratio, expect_order=[2, 3, 1, 0])


def case_edges():
    """Query points 150 px outside each bound (the four early returns), a feature at |dx| == windowSize exactly and one just inside,
    bounds that are neither integers nor positive (an undistorted image).  prev differs from the keypoints throughout."""
    bounds = (-12.7, 655.3, -7.4, 489.6)
    rng = np.random.default_rng(41)
    n2 = 400
    x2 = rng.uniform(-10, 650, n2).astype(F32); y2 = rng.uniform(-5, 485, n2).astype(F32)
    x2[:4] = [400.0, 399.5, 250.0, 250.0]; y2[:4] = [250.0, 250.0, 350.0, 349.75]
    o2 = np.where(rng.random(n2) < 0.6, 0, 1).astype(np.int32); o2[:4] = 0
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    F2 = Frame(make_kps(x2, y2, o2, rng.uniform(0, 360, n2).astype(F32)), d2, bounds)
    prev = np.array([[-12.7 - 150, 240], [655.3 + 150, 240], [320, -7.4 - 150], [320, 489.6 + 150],      # the four early returns
                     [300.0, 250.0],            # feature 0 at dx == 100 exactly: out; feature 1 at 99.5: in
                     [300.0, 250.0],            # (the same query point again, another descriptor)
                     [200.0, 250.0],            # feature 2 at dy == 100 exactly: out; feature 3 at 99.75: in
                     [-12.7 - 99.0, -7.4 - 99.0],   # reaches the first cells only
                     [655.3 + 99.0, 489.6 + 99.0],
                     [3.0e9, 3.0e9], [-3.0e9, 10.0]], F32)                  # far outside int range of a cell index
    n1 = len(prev)
    x1 = rng.uniform(50, 600, n1).astype(F32); y1 = rng.uniform(50, 400, n1).astype(F32)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    d1[4] = flip_bits(rng, d2[1], 3); d1[6] = flip_bits(rng, d2[3], 2)
    F1 = Frame(make_kps(x1, y1, np.zeros(n1, np.int32), rng.uniform(0, 360, n1).astype(F32)), d1, bounds)
    return dict(F1=F1, F2=F2, prev=prev, window=100)


def case_levels(which):
    F1, F2 = make_pair(51, 200, 210)
    F = F1 if which == 1 else F2
    k = F.kps.copy()
    k["octave"] = np.maximum(k["octave"], 1)
    G = Frame(k, F.desc, F.bounds)
    F1, F2 = (G, F2) if which == 1 else (F1, G)
    return dict(F1=F1, F2=F2, prev=F1.pts, window=100)


def case_chain(steps=5):
    """Five calls, F2 moving on by the same motion each time; every call is given the prev_matched the previous one returned."""
    F1, F2 = make_pair(61, 500, 500, motion=12.0)
    rng = np.random.default_rng(62)
    frames = [F2]
    for s in range(1, steps):
        k = frames[-1].kps.copy()
        k["x"] = (k["x"] + F32(27.0) + rng.normal(0, 0.7, len(k))).astype(F32)
        k["y"] = (k["y"] - F32(15.0) + rng.normal(0, 0.7, len(k))).astype(F32)
        d = np.stack([flip_bits(rng, r, int(rng.integers(0, 6))) for r in frames[-1].desc])
        frames.append(Frame(k, d, F2.bounds))
    return dict(F1=F1, F2=frames, prev=F1.pts, window=100)


def cases():
    """name -> dict(F1, F2, prev, window[, nn_ratio, check_orientation, list_capacity]); chain: F2 is a list of frames."""
    small = case_small()
    return {
        "small": small,
        "crowded": case_crowded(),
        "ties": case_ties(),
        "ties_loose": case_ties(nn_ratio=1.5),
        "edges": case_edges(),
        "levels_f1": case_levels(1),
        "levels_f2": case_levels(2),
        "window10": dict(small, window=10),
        "big": case_big(),
        "no_orientation": dict(small, check_orientation=False),
    }


def run_case(c, **kw):
    return search(c["F1"], c["F2"], c["prev"], c["window"], c.get("nn_ratio", 0.9), c.get("check_orientation", True), **kw)


def run_chain(c, step_fn=None):
    """-> the results of the calls; step_fn(F1, F2, prev, window) -> dict with `prev` replaces the model (the product, in a GPU test)."""
    prev, out = c["prev"], []
    for F2 in c["F2"]:
        r = step_fn(c["F1"], F2, prev, c["window"]) if step_fn else search(c["F1"], F2, prev, c["window"])
        out.append(r)
        prev = r["prev"]
    return out


# ------------------------------------------------------------------------------------------------ files for the C++ programs

def write_scene(path, F1, F2, prev, window, nn_ratio=0.9, check_orientation=True):
    """The scene file tests/cpp/search_init_ref.hpp reads (both frames share F2's bounds there: the cases' frames do)."""
    assert F1.bounds == F2.bounds
    with open(path, "wb") as f:
        f.write(np.array([F1.n, F2.n, int(window), int(check_orientation)], np.int32).tobytes())
        f.write(np.array([nn_ratio] + [float(b) for b in F2.bounds], np.float32).tobytes())
        for F in (F1, F2):
            f.write(F.kps.tobytes()); f.write(F.desc.tobytes())
        f.write(np.ascontiguousarray(prev, F32).tobytes())


def write_lists(path, r, F1, F2, prev, nn_ratio=0.9, check_orientation=True):
    """The lists file tests/cpp/init_replay_check.cpp reads; r = a result of search()."""
    with open(path, "wb") as f:
        f.write(np.array([F1.n, F2.n, int(check_orientation)], np.int32).tobytes())
        f.write(np.array([nn_ratio], np.float32).tobytes())
        f.write(np.ascontiguousarray(r["list_start"], np.int32).tobytes()); f.write(np.ascontiguousarray(r["entries"], np.uint32).tobytes())
        f.write(np.ascontiguousarray(F1.kps["octave"], np.int32).tobytes()); f.write(np.ascontiguousarray(F1.kps["angle"], F32).tobytes())
        f.write(np.ascontiguousarray(F2.kps["angle"], F32).tobytes()); f.write(np.ascontiguousarray(F2.pts, F32).tobytes())
        f.write(np.ascontiguousarray(prev, F32).tobytes())


def parse_program_output(text, tag=""):
    """`<tag> nmatches N`, `<tag> matches12: ...`, `<tag> prev: <hex bits>`, optionally `counters`, `list_start`, `entries` lines."""
    out = {}
    pre = tag + " " if tag else ""
    for line in text.splitlines():
        if not line.startswith(pre):
            continue
        key, _, rest = line[len(pre):].partition(" ")
        key = key.rstrip(":")
        vals = rest.split()
        if key == "nmatches":
            out["nmatches"] = int(vals[0])
        elif key == "prev":
            out["prev"] = np.array([int(v, 16) for v in vals], np.uint32).view(F32).reshape(-1, 2)
        elif key in ("matches12", "list_start", "counters"):
            out[key] = np.array([int(v) for v in vals], np.int32)
        elif key == "entries":
            out[key] = np.array([int(v) for v in vals], np.uint32)
    return out
