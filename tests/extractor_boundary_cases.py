"""Inputs of the extractor boundary tests (tests/test_gpu_extractor_boundaries.py on the device, tests/test_extractor_boundaries_cpu.py
for the conditions those rest on): images that sit at the limits of the device quad-tree of csrc/extractor.hip and of the stereo matcher
behind it.  Nothing here touches the GPU; numpy and the oracle are the only things that run, and an oracle result is computed once per
input and shared by every test that needs it."""
import functools

import numpy as np

from multi_orbslam3_amd import synth
from oracle import binding as ob

# The limits of octree_kernel as csrc/extractor.hip documents them: candidates per (camera, level) held in registers, nodes alive at once
# in LDS.  A level's selection region holds min(4 N + 8, LIST_CAP) nodes for a per-level target of N.
KEY_CAP = 4096
LIST_CAP = 2048
SPEC_CELLS = 4                   # cells per thread fetched speculatively; a thread's further cells are taken by two plain loops
OCT_THREADS = 256
EDGE = 19                        # EDGE_THRESHOLD; the FAST area starts EDGE - 3 pixels inside the level
CELL = 30                        # the reference's cell size W of ComputeKeyPointsOctTree


# ------------------------------------------------------------------ restatements of the reference's arithmetic

def features_per_level(n_features, scale_factor=1.2, n_levels=8):
    """mnFeaturesPerLevel of ORBextractor's constructor (S/ORBextractor.cc:434-444): a geometric share per level in float, cvRound, the
    rest (never below 0) to the top level."""
    f32 = np.float32
    factor = f32(1.0) / f32(scale_factor)
    desired = f32(n_features) * (f32(1) - factor) / (f32(1) - f32(float(factor) ** n_levels))
    out, total = [], 0
    for _ in range(n_levels - 1):
        out.append(int(np.rint(np.float64(desired))))          # cvRound: to nearest, ties to even
        total += out[-1]
        desired = f32(desired * factor)
    out.append(max(n_features - total, 0))
    return out


def level_sizes(W, H, scale_factor=1.2, n_levels=8):
    """(width, height) of every pyramid level: cvRound(size * mvInvScaleFactor[level]) in float (S/ORBextractor.cc:1158-1160)."""
    f32 = np.float32
    s, out = f32(1.0), []
    for l in range(n_levels):
        inv = f32(1.0) / s
        out.append((int(np.rint(np.float64(f32(W) * inv))), int(np.rint(np.float64(f32(H) * inv)))))
        s = f32(s * f32(scale_factor))
    return out


def cell_grid(w, h):
    """(nCols, nRows, wCell, hCell) of the 30-pixel tiling of a w x h level (S/ORBextractor.cc:782-790)."""
    width, height = w - 2 * (EDGE - 3), h - 2 * (EDGE - 3)
    n_cols, n_rows = width // CELL, height // CELL
    return n_cols, n_rows, -(-width // n_cols), -(-height // n_rows)


def cell_of_candidates(cands, w, h):
    """Cell index (row-major) of every candidate (x, y relative to the FAST area) of a w x h level: a cell's window starts at
    (j * wCell, i * hCell) and FAST answers from 3 pixels inside it.  This indexes the nominal nCols x nRows grid: the reference (and
    the library's geometry) skip a cell whose window starts beyond the border, which renumbers the cells behind it.  No level of the
    shapes used here has such a cell (the CPU test holds the candidate order against this index); on a shape that has, the index
    and the cells-per-thread arithmetic built on it would be off."""
    n_cols, n_rows, wc, hc = cell_grid(w, h)
    return ((cands[:, 1] - 3) // hc) * n_cols + (cands[:, 0] - 3) // wc


def cells_per_thread(n_cells):
    return -(-n_cells // OCT_THREADS)


def n_roots(w, h):
    """nIni of DistributeOctTree (S/ORBextractor.cc:541): round((maxX - minX) / (maxY - minY)) of the level's FAST area."""
    return max(int(np.floor(np.float32(w - 2 * (EDGE - 3)) / np.float32(h - 2 * (EDGE - 3)) + np.float32(0.5))), 1)


# ------------------------------------------------------------------ the oracle, once per input

class Ref:
    """The oracle's answer on one image: keypoints, descriptors, the candidates and the pyramid of every level."""

    def __init__(self, img, n_features, n_levels=8):
        H, W = img.shape
        self.img, self.n_features, self.n_levels, self.W, self.H = img, n_features, n_levels, W, H
        self.ex = ob.Extractor(n_features=n_features, n_levels=n_levels, max_width=W, max_height=H)
        rc, self.kps, self.desc, self.n_mono = self.ex.extract(img, cap=8192)
        assert rc == 0, "the oracle did not run to the end (status %d)" % rc
        self.quota = [int(v) for v in self.ex.tables()[4]]
        self.cands = [self.ex.candidates(l) for l in range(n_levels)]
        self.n_cands = [len(c) for c in self.cands]
        self.per_level = [int(v) for v in np.bincount(self.kps["octave"], minlength=n_levels)]       # = nodes at the end of each tree

    def overflowing_levels(self):
        """Levels the device quad-tree cannot hold, from the documented constants alone: more than KEY_CAP candidates, a node list bound
        4 N + 8 beyond LIST_CAP, or more final nodes (one keypoint each) than the level's region of min(4 N + 8, LIST_CAP).
        Only the list at the END of a tree is modelled, not the kernel's guards on a list that passes LIST_CAP between two passes.
        That is enough for the inputs of this module and for nothing else: a list only grows, phase 1 keeps nodes + 3 * expandable
        <= N and phase 2 stops at the first node that reaches N, so with 4 N + 8 <= LIST_CAP no intermediate list is longer than
        the final one allows.  Do not reuse it for inputs where a pass could carry a list beyond 2048 nodes."""
        return [l for l in range(self.n_levels)
                if self.n_cands[l] > KEY_CAP or 4 * self.quota[l] + 8 > LIST_CAP or self.per_level[l] > min(4 * self.quota[l] + 8, LIST_CAP)]


def expected_redos(*refs):
    """Frames redone on the host per call that extracts these images together: one if any level of any image overflows."""
    return int(any(r.overflowing_levels() for r in refs))


def host_from_the_start(n_features, scale_factor=1.2, n_levels=8):
    """A handle whose per-level target alone exceeds the node list (4 N + 8 > LIST_CAP at some level) never launches the device
    quad-tree: its frames go to the host trees once, which is no redo."""
    return any(4 * n + 8 > LIST_CAP for n in features_per_level(n_features, scale_factor, n_levels))


# ------------------------------------------------------------------ 1. dot images: K candidates at level 0

DOT_K = (4095, 4096, 4097)
DOT_STEREO = ((4096, 4096), (4097, 4096), (4096, 4097))
DOT_LATTICE = 5270
DOT_FEATURES = 1000


@functools.lru_cache(maxsize=None)
def dot_image(K, amp=12):
    """A flat 640 x 480 image of value 60 with the first K points (row by row) of the 7-pixel lattice from (24, 24) raised by amp."""
    img = np.full((480, 640), 60, np.uint8)
    ys, xs = np.meshgrid(np.arange(24, 480 - 24, 7), np.arange(24, 640 - 24, 7), indexing="ij")
    assert xs.size == DOT_LATTICE and K <= DOT_LATTICE
    img[ys.ravel()[:K], xs.ravel()[:K]] = 60 + amp
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def dot_ref(K, n_features=DOT_FEATURES):
    return Ref(dot_image(K), n_features)


# ------------------------------------------------------------------ 2. the node-list edge: N = 510 / 511 at level 0

NODE_EDGE = ((2350, 510), (2351, 511))         # (n_features, level-0 target)
NODE_EDGE_DOTS = 4000


# ------------------------------------------------------------------ 3. small feature counts: levels whose target is 0

SMALL_FEATURES = (1, 2, 3, 5, 8, 9)
SMALL_SHAPES = ((640, 480), (1241, 376))
SMALL_SPLITS = {1: [0, 0, 0, 0, 0, 0, 0, 1], 2: [0, 0, 0, 0, 0, 0, 0, 2], 3: [1, 1, 0, 0, 0, 0, 0, 1], 8: [2, 1, 1, 1, 1, 1, 1, 0]}


@functools.lru_cache(maxsize=None)
def textured_scene(W, H):
    if (W, H) == (640, 480):
        return synth.Scene(640, 480)
    return synth.Scene(W, H, tex_size=(max(2 * W, 800), max(2 * H, 600)), px_per_m=100.0)


@functools.lru_cache(maxsize=None)
def small_pair(W, H):
    L, R, Tcw = textured_scene(W, H).stereo_pair(2)
    return np.ascontiguousarray(L), np.ascontiguousarray(R), Tcw


@functools.lru_cache(maxsize=None)
def small_ref(W, H, n_features, side):
    return Ref(small_pair(W, H)[side], n_features)


# ------------------------------------------------------------------ 4. large images: more than 1024 cells per level

LARGE_SHAPES = ((1920, 1080), (992, 992), (1022, 1022))
LARGE_FEATURES = 2000
LARGE_CELLS = {(1920, 1080): (2108, 1456, 989), (992, 992): (1024,), (1022, 1022): (1089,)}        # levels 0, 1, 2 as the issue lists them


def blocks_image(W, H, seed, n_blocks, n_dots, max_w=80, max_h=60, amp=40):
    """Random rectangles on a ramp (large flat areas, cells that fall back to minThFAST or stay empty), as the extractor's image-shape
    tests use them, and n_dots single pixels raised by amp on a 7-pixel lattice: isolated candidates in a number that is chosen here."""
    rng = np.random.RandomState(seed)
    img = np.tile((np.arange(W) * 40 // W + 60).astype(np.uint8), (H, 1))
    for _ in range(n_blocks):
        x0, y0 = rng.randint(0, W - 8), rng.randint(0, H - 8)
        img[y0:y0 + rng.randint(4, max_h), x0:x0 + rng.randint(4, max_w)] = rng.randint(0, 200)
    ys, xs = np.meshgrid(np.arange(24, H - 24, 7), np.arange(24, W - 24, 7), indexing="ij")
    pick = rng.choice(xs.size, n_dots, replace=False)
    img[ys.ravel()[pick], xs.ravel()[pick]] += amp
    return np.ascontiguousarray(img)


@functools.lru_cache(maxsize=None)
def large_image(W, H):
    img = blocks_image(W, H, W * 1000 + H, (W * H) // 5000, (W * H) // 700)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def large_ref(W, H):
    return Ref(large_image(W, H), LARGE_FEATURES)


# ------------------------------------------------------------------ 5. coordinates in 12 bits: 4000 x 100, four levels

WIDE_SHAPE = (4000, 100)
WIDE_LEVELS = 4
WIDE_FEATURES = 500
WIDE_AMP = 150


@functools.lru_cache(maxsize=None)
def wide_image():
    """Blocks on a ramp over the whole width, and a column of small bright squares within the last 40 columns."""
    W, H = WIDE_SHAPE
    img = blocks_image(W, H, 4100, 150, 600, max_w=60, max_h=40)
    img[:, W - 44:] = 70
    for y0 in range(24, H - 24, 7):
        for x0 in (W - 36, W - 29, W - 22):                # level-0 x up to 3978 of the 3980 that FAST can answer
            img[y0, x0] = 70 + WIDE_AMP
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def wide_ref():
    return Ref(wide_image(), WIDE_FEATURES, WIDE_LEVELS)


# ------------------------------------------------------------------ 6. stereo pairs with an empty side

STEREO_FEATURES = 1000
EMPTY_SIDE_CASES = ("right_flat", "left_flat", "rows_apart", "both_flat")
FLAT = 128


@functools.lru_cache(maxsize=None)
def empty_side_pair(case):
    """(left, right) 640 x 480 images.  rows_apart: the left image keeps the scene's rows 60 ... 199 and is flat elsewhere, the right image
    shows the same rows at 280 ... 419: 80 rows between the two bands, more than 2 * scale[7] = 7.2 plus the patch radius of any level."""
    L, R, _ = textured_scene(640, 480).stereo_pair(2)
    flat = np.full((480, 640), FLAT, np.uint8)
    if case == "right_flat":
        pair = (L, flat)
    elif case == "left_flat":
        pair = (flat, R)
    elif case == "both_flat":
        pair = (flat, flat)
    else:
        a, b = flat.copy(), flat.copy()
        a[60:200] = L[60:200]
        b[280:420] = R[60:200]
        pair = (a, b)
    out = tuple(np.ascontiguousarray(p) for p in pair)
    for p in out:
        p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def empty_side_ref(case):
    """dict(refL, refR, uright, depth): the oracle's two extractions and its ComputeStereoMatches on them."""
    cam = textured_scene(640, 480).cam
    L, R = empty_side_pair(case)
    rl, rr = Ref(L, STEREO_FEATURES), Ref(R, STEREO_FEATURES)
    ur, dp = ob.stereo_match(rl.ex, rr.ex, rl.kps, rl.desc, rr.kps, rr.desc, float(cam["bf"]), float(cam["b"]))
    return dict(refL=rl, refR=rr, uright=ur, depth=dp)


@functools.lru_cache(maxsize=None)
def normal_frame(k=4):
    """An ordinary stereo frame of the 640 x 480 scene, extracted and matched by the oracle: what a handle is given after an overflow."""
    cam = textured_scene(640, 480).cam
    L, R, Tcw = textured_scene(640, 480).stereo_pair(k)
    L, R = np.ascontiguousarray(L), np.ascontiguousarray(R)
    rl, rr = Ref(L, DOT_FEATURES), Ref(R, DOT_FEATURES)
    ur, dp = ob.stereo_match(rl.ex, rr.ex, rl.kps, rl.desc, rr.kps, rr.desc, float(cam["bf"]), float(cam["b"]))
    return dict(L=L, R=R, Tcw=Tcw, refL=rl, refR=rr, uright=ur, depth=dp)
