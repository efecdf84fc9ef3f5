"""Inputs of tests/test_gpu_two_view_boundaries.py: TwoViewReconstruction past one LDS tile of 256 matches, at both caps (8192 matches,
4096 iterations), through both branches of CheckRT and around its rank switch.  Everything here is formed from the numpy model
(tests/two_view_model.py) in float32 and float64; tests/test_two_view_boundaries_cpu.py asserts, without a device, the conditions
the comparison leans on.  640 x 480 images, 37 / 71 unmatched keypoints interleaved, draws from case_draws(N, H, seed).

Families, name -> (kind, N, H, seed, scene keywords, camera, sigma):
  P  the slanted plane of the capped cases (0.05 px noise, no mismatches, 1 m baseline) at 511 / 512 / 513 / 1025 matches, at the cap of
     8192 matches and at the cap of 4096 iterations.
  W  a usual initialisation (3-D, 0.3 px noise, one match in ten a mismatch: F is chosen and succeeds) at every tile, mask-word and
     workgroup edge up to both caps, with a camera whose fx != fy and with sigma = 2.
  Q  the plane with 0.6 px noise and 4 iterations: H is chosen, eight motions; two successes and one refusal by secondBestGood.
  R  3-D scenes of 49 .. 53 matches, all of them counted by one motion: min(50, nGood - 1) and nGood >= 50 on both sides."""
import numpy as np

import two_view_model as tm

_P = dict(noise=0.05, outliers=0.0, baseline=1.0)
_Q = dict(noise=0.6, outliers=0.0, baseline=1.0)
CAM2 = (458.654, 457.296, 367.215, 248.375)

CASES = {}
# P at 513 and 1025 matches: the seeds first listed (23 and 24) leave 3.1 % and 4.2 % of the inliers open in one motion (an F fitted to a
# plane gives motions whose reprojection errors differ by 2e-2 relative between the precisions); 25 and 28 are the next seeds that
# keep every condition of test_two_view_boundaries_cpu.py (24 at 513 and 25 - 27 at 1025 miss the same cap)
for _n, _h, _s in ((511, 33, 21), (512, 32, 22), (513, 65, 25), (1025, 33, 28), (8192, 8, 26), (100, 4096, 67)):
    CASES["P%d_%d" % (_n, _h)] = ("plane", _n, _h, _s, _P, tm.CAM, 1.0)
for _n, _h, _s in ((63, 33, 31), (64, 32, 32), (65, 33, 33), (255, 31, 61), (256, 32, 62), (257, 33, 34), (511, 33, 63), (512, 32, 35),
                   (513, 65, 36), (1025, 33, 37), (8191, 33, 64), (8192, 33, 38), (100, 4096, 65), (64, 4095, 66)):
    CASES["W%d_%d" % (_n, _h)] = ("3d", _n, _h, _s, {}, tm.CAM, 1.0)
CASES["W300_cam"] = ("3d", 300, 33, 81, {}, CAM2, 1.0)
CASES["W300_sigma2"] = ("3d", 300, 33, 82, {}, tm.CAM, 2.0)
for _s in (105, 118):
    CASES["Q513_s%d" % _s] = ("plane", 513, 4, _s, _Q, tm.CAM, 1.0)
CASES["Q8192_s115"] = ("plane", 8192, 4, 115, _Q, tm.CAM, 1.0)
for _n in (49, 50, 51, 52, 53):
    CASES["R%d" % _n] = ("3d", _n, 33, 50 + _n, _P, tm.CAM, 1.0)

FAMILY = {f: tuple(n for n in CASES if n[0] == f) for f in "PWQR"}
NEAR_CAP = dict(P=0.001, W=0.01, Q=0.025, R=0.01)       # the share of near pairs a case may have; R is a W scene with less noise
OPEN_CAP = 0.01                                         # open matches per motion, as a share of the inliers
Q_REFUSED = "Q513_s118"
# case -> the models (0 H, 1 F) of which NO hypothesis is free of near pairs, so that none of its scores is compared to the bit and all
# are held to the bound per near direction: with a share s of near pairs a hypothesis is free with probability (1 - s)^N, which is
# e^-40 for F at 8192 matches of W and less for Q (s = 2 %, 513 matches and more).  Asserted for the models on the CPU.
NOTHING_TO_THE_BIT = {"W8192_33": (1,), "Q513_s105": (0, 1), "Q513_s118": (0, 1), "Q8192_s115": (0, 1)}

# outside the families: the small call between two large ones, and the scene of the equal-score test
EXTRA = {"S8": ("plane", 8, 1, 91, _P, tm.CAM, 1.0)}
TIE = ("3d", 300, 65, 71, {}, tm.CAM, 1.0)
TIE_ROWS = dict(H=(9, 38), F=(8, 37))

_cache, _fig = {}, {}


def _models(spec, draws=None):
    kind, N, H, seed, kw, cam, sigma = spec
    sc = tm.scene(kind, N, seed, n_extra1=37, n_extra2=71, cam=cam, size=tm.SIZE, **kw)
    d = tm.case_draws(N, H, seed) if draws is None else draws
    o32 = tm.reconstruct(sc.keys1, sc.keys2, sc.matches12, sc.cam, sigma, H, d, np.float32)
    o64 = tm.reconstruct(sc.keys1, sc.keys2, sc.matches12, sc.cam, sigma, H, d, np.float64)
    return sc, d, o32, o64


def spec(name):
    return CASES[name] if name in CASES else EXTRA[name]


def case(name):
    """-> (scene, draws, float32 model, float64 model), computed once per process and shared; callers must not modify them."""
    if name not in _cache:
        _cache[name] = _models(spec(name))
    return _cache[name]


def tie_case():
    """The equal-score scene: the draw row of the unmodified model's best H set copied into rows 9 and 38, the best F set's into rows 8
    and 37; an original best row below its copies gets its neighbour's draws.  Rows 8 / 9 are held by higher lanes of the serial
    rule's workgroup than rows 37 / 38 (lane = row mod 32), and the lower row must win.  -> (scene, draws, float32 model,
    float64 model, (original best H row, original best F row))."""
    if "tie" not in _cache:
        sc, d, a, _ = _models(TIE)
        bH, bF = a.bestH, a.bestF
        assert bH >= 0 and bF >= 0 and bH != bF
        d = d.copy()
        rowH, rowF = d[bH].copy(), d[bF].copy()
        for b, lo in ((bH, TIE_ROWS["H"][0]), (bF, TIE_ROWS["F"][0])):
            if b < lo:
                nb = b + 1
                while nb in (bH, bF):
                    nb += 1
                d[b] = d[nb]
        d[list(TIE_ROWS["H"])] = rowH
        d[list(TIE_ROWS["F"])] = rowF
        _cache["tie"] = _models(TIE, d) + ((bH, bF),)
    return _cache["tie"]


def delta():
    """The chi-square band of the committed suite: 4 x the models' largest relative difference around the gates on tm.CAPPED."""
    if "delta" not in _fig:
        _fig["delta"] = 4 * tm.measured_chi_difference()
    return _fig["delta"]


def near(name):
    """(2, H, N) near pairs and (2, 2, H, N) near directions of a case, from the float64 model."""
    k = ("near", name)
    if k not in _cache:
        b = (tie_case() if name == "tie" else case(name))[3]
        nd = tm.near_directions(b, delta())
        _cache[k] = (nd.any(axis=1), nd)
    return _cache[k]


def rt_margins(name):
    """CheckRT's margins of a case: 4 x the largest float32-to-float64 difference of each gate quantity around its gate over the
    motions of that case (tm.measured_rt_differences) -> (dict(e, cos, z), the measured differences, the matches in each band).  Per
    case, because the differences follow the conditioning of the case's motions: a fundamental matrix fitted to a plane (P) gives
    motions whose triangulations differ a thousand times more between the two precisions than those of a 3-D scene (W, R)."""
    k = ("rt", name)
    if k not in _cache:
        w, cnt = tm.measured_rt_differences([case(name)[2:4]])
        _cache[k] = ({q: 4 * v for q, v in w.items()}, w, cnt)
    return _cache[k]


def open_matches(name):
    """(n_motions, N) bool of a case (tm.open_matches), from the models alone."""
    k = ("open", name)
    if k not in _cache:
        _, _, a, b = case(name)
        _cache[k] = tm.open_matches(a, b, rt_margins(name)[0])
    return _cache[k]


def rank_visible(name):
    """Per motion of a case: the parallax comparison can see an off-by-one in sorted[min(50, nGood - 1)].  The motion has no open
    match and at least two counted ones, and the float32 model's parallax at the ranks beside `want` differs from the one at `want`
    by more than the one float32 ulp the comparison may allow."""
    _, _, a, _ = case(name)
    op = open_matches(name)
    out = np.zeros(a.n_motions, bool)
    for k in range(a.n_motions):
        lo, at, hi = tm.rank_neighbours(a, k)
        if at is None or op[k].any() or (lo is None and hi is None):
            continue
        ulp = float(np.spacing(np.float32(abs(at))))
        out[k] = all(x is None or abs(float(x) - float(at)) > ulp for x in (lo, hi))
    return out


def output_tolerances():
    """4 x the float32-to-float64 difference of the models in R21, t21, vP3D (and the unit matrices) over the family cases."""
    if "out" not in _fig:
        _fig["out"] = {k: 4 * v for k, v in tm.measured_output_differences(list(CASES), case_fn=case).items()}
    return _fig["out"]


if __name__ == "__main__":
    import time
    print("delta %.3e" % delta())
    for n in CASES:
        t0 = time.time()
        sc, d, a, b = case(n)
        np_, _ = near(n)
        dif = (a.masks != b.masks) & ~np_
        op = open_matches(n)
        m, w, cnt = rt_margins(n)
        print("%-12s model %d/%d ok %s/%s rows %s/%s motion %d/%d near %6d of %8d (%.4f %%) mask diffs outside %d; nGood %s / %s parallax %s; "
              "gate diffs %d open %s inliers %d; margins e %.2e (%d) cos %.2e (%d) z %.2e (%d)  [%.1f s]" %
              (n, a.model, b.model, a.ok, b.ok, (a.bestH, a.bestF), (b.bestH, b.bestF), a.best_motion, b.best_motion, np_.sum(), np_.size,
               100.0 * np_.mean(), dif.sum(), a.motion_nGood.tolist(), b.motion_nGood.tolist(), np.round(a.motion_parallax, 3).tolist(),
               int((a.gates != b.gates).sum()) if tm.same_rt(a, b) else -1, op.sum(axis=1).tolist(), a.n_inliers,
               m["e"], cnt["e"], m["cos"], cnt["cos"], m["z"], cnt["z"], time.time() - t0))
    t = output_tolerances()
    print("tolerances (4 x float32 - float64 model): M %.3e R %.3e t %.3e P %.3e" % (t["M"], t["R"], t["t"], t["P"]))
    sc, d, a, b, orig = tie_case()
    print("tie: original best rows %s -> model best H %d F %d; scores H %s F %s" %
          (orig, a.bestH, a.bestF, a.scores[0, list(TIE_ROWS["H"])].tolist(), a.scores[1, list(TIE_ROWS["F"])].tolist()))
