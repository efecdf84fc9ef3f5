"""The frame constructor of csrc/extractor.hip at the limits of its device quad-tree, and the stereo matcher with an empty side: inputs and
reasons in tests/extractor_boundary_cases.py, their conditions without a device in tests/test_extractor_boundaries_cpu.py.  Every
comparison of outputs is bit equality with the oracle.  orbx_get_host_redo_count tells a frame that stayed on the device from one that
was redone with the host quad-trees; what it must read comes from the documented limits (4096 candidates, 2048 nodes, a region of
min(4 N + 8, 2048) per level) and the oracle's counts (Ref.overflowing_levels), never from the device."""
import numpy as np
import pytest

import extractor_boundary_cases as xb
import helpers
from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import api, synth, views
from oracle import binding as ob
from test_gpu_parity import _assert_extract_equal

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_levels_and_candidates(ex, cam, ref, what, levels=True):
    for l in range(ref.n_levels):
        assert np.array_equal(ex.candidates(cam, l), ref.cands[l]), "%s: FAST candidates of level %d (camera %d)" % (what, l, cam)
        if levels:
            assert np.array_equal(ex.level(cam, l), ref.ex.level(l)), "%s: pyramid level %d (camera %d)" % (what, l, cam)


def _host_trees_ran(ex):
    """The host quad-trees ran in the handle's last call (their wall time is recorded then, and zeroed by a call that stayed on the device)."""
    return ex.timings()["octree_host_ms"] > 0


def _mono_on(ex, ref, what, calls=2):
    for _ in range(calls):
        nm, kps, desc = ex(ref.img, (0, 0))
        _assert_extract_equal((kps, desc), (ref.kps, ref.desc), what)
        assert nm == ref.n_mono == len(kps)


def _stereo_on(ex, refl, refr, what, calls=2):
    for _ in range(calls):
        (kl, dl), (kr, dr) = ex.extract_stereo(refl.img, refr.img)
        _assert_extract_equal((kl, dl), (refl.kps, refl.desc), what + " left")
        _assert_extract_equal((kr, dr), (refr.kps, refr.desc), what + " right")


def _oracle_matches(refl, refr, cam):
    return ob.stereo_match(refl.ex, refr.ex, refl.kps, refl.desc, refr.kps, refr.desc, float(cam["bf"]), float(cam["b"]))


def _frame_view(scene, kps, desc, ur, dp, n_levels=8):
    p = scene.frame_view_params()
    if len(kps) == 0:              # a view needs arrays to point at; n = 0 says that nothing is in them
        fv, keep = views.frame_view(np.zeros(1, capi.KEYPOINT_DTYPE), np.zeros((1, 32), np.uint8), np.full(1, -1, np.float32),
                                    np.full(1, -1, np.float32), p["bounds"], p["cam"], n_levels, 1.2)
        fv.n = 0
        return fv, keep
    return views.frame_view(kps, desc, ur, dp, p["bounds"], p["cam"], n_levels, 1.2)


def _fused_stereo_on(ex, F, scene, refl, refr, our, odp, what):
    """orbx_frame_stereo: both feature sets' counts, the left features, uRight / depth as bits, the grid."""
    cam = scene.cam
    fv, keep = _frame_view(scene, refl.kps, refl.desc, our, odp)
    n, nr, kl, dl, ur, dp = ex.frame_stereo(F, fv, refl.img, refr.img, float(cam["bf"]), float(cam["b"]), download=True)
    assert n == len(refl.kps) and nr == len(refr.kps), what
    _assert_extract_equal((kl, dl), (refl.kps, refl.desc), what + " fused left")
    assert np.array_equal(_bits(ur), _bits(our)) and np.array_equal(_bits(dp), _bits(odp)), what + ": uRight / depth"
    gs, gi = F.grid()
    os_, oi = ob.build_grid(fv)
    assert np.array_equal(gs, os_) and np.array_equal(gi, oi), what + ": grid"
    return fv, keep


def _normal_frame_on(ex, what):
    """An ordinary scene on a handle that has just overflowed (or not): extraction and stereo matches as the oracle's, and no redo."""
    nf = xb.normal_frame()
    before = ex.host_redo_count()
    _stereo_on(ex, nf["refL"], nf["refR"], what + ", then a scene", calls=1)
    cam = xb.textured_scene(640, 480).cam
    ur, dp = ex.ComputeStereoMatches(float(cam["bf"]), float(cam["b"]), n_left=len(nf["refL"].kps))
    assert np.array_equal(_bits(ur), _bits(nf["uright"])) and np.array_equal(_bits(dp), _bits(nf["depth"])), what + ", then a scene: matches"
    assert ex.host_redo_count() == before and not _host_trees_ran(ex), what + ": the overflow left something behind"


# ------------------------------------------------------------------ 1. 4095 / 4096 / 4097 candidates at level 0

@pytest.mark.parametrize("K", xb.DOT_K)
def test_dot_images_at_the_candidate_limit_through_the_monocular_extractor(K):
    """kOctKeyCap = 4096 candidates per (camera, level), 16 per thread in registers: 4095 and 4096 stay on the device (no redo), 4097 is
    redone on the host once per call; the results are the oracle's either way, twice on one handle, on a one- and a two-camera handle,
    and the scene that follows is untouched by the overflow."""
    ref = xb.dot_ref(K)
    redo = xb.expected_redos(ref)
    assert redo == int(K > xb.KEY_CAP)
    for n_cams in (1, 2):
        ex = api.ORBextractor(xb.DOT_FEATURES, 1.2, 8, 20, 7, 640, 480, n_cams=n_cams)
        assert ex.host_redo_count() == 0
        _mono_on(ex, ref, "%d dots, %d-camera handle" % (K, n_cams))
        assert ex.host_redo_count() == 2 * redo and _host_trees_ran(ex) == bool(redo)
        _assert_levels_and_candidates(ex, 0, ref, "%d dots" % K)
        if n_cams == 2:
            _normal_frame_on(ex, "%d dots" % K)
            assert ex.host_redo_count() == 2 * redo
        else:
            nf = xb.normal_frame()
            nm, kps, desc = ex(nf["L"], (0, 0))
            _assert_extract_equal((kps, desc), (nf["refL"].kps, nf["refL"].desc), "%d dots, then a scene" % K)
            assert ex.host_redo_count() == 2 * redo and not _host_trees_ran(ex)


@pytest.mark.parametrize("kl,kr", xb.DOT_STEREO)
def test_dot_images_at_the_candidate_limit_through_the_stereo_forms(kl, kr):
    """The over-limit level on either camera of extract_stereo and of the fused constructor: one redo per call whichever camera
    overflows, none for (4096, 4096); both feature sets, the candidates of both cameras, the stereo matches and the grid are the oracle's."""
    scene = xb.textured_scene(640, 480)
    refl, refr = xb.dot_ref(kl), xb.dot_ref(kr)
    redo = xb.expected_redos(refl, refr)
    assert redo == int(max(kl, kr) > xb.KEY_CAP)
    what = "dots (%d, %d)" % (kl, kr)
    ex = api.ORBextractor(xb.DOT_FEATURES, 1.2, 8, 20, 7, 640, 480, n_cams=2)
    _stereo_on(ex, refl, refr, what)
    assert ex.host_redo_count() == 2 * redo and _host_trees_ran(ex) == bool(redo)
    _assert_levels_and_candidates(ex, 0, refl, what)
    _assert_levels_and_candidates(ex, 1, refr, what)
    our, odp = _oracle_matches(refl, refr, scene.cam)
    ur, dp = ex.ComputeStereoMatches(float(scene.cam["bf"]), float(scene.cam["b"]), n_left=len(refl.kps))
    assert np.array_equal(_bits(ur), _bits(our)) and np.array_equal(_bits(dp), _bits(odp)), what
    _normal_frame_on(ex, what)
    # the fused constructor: the chained stereo / grid kernels stay idle on overflow and the host redoes the whole frame
    F = api.Frame()
    for _ in range(2):
        _fused_stereo_on(ex, F, scene, refl, refr, our, odp, what)
    assert ex.host_redo_count() == 4 * redo and _host_trees_ran(ex) == bool(redo)
    # the two-halves constructor acts on the overflow flag in its wait
    fv, keep = _frame_view(scene, refl.kps, refl.desc, our, odp)
    ex.frame_stereo_submit(F, fv, refl.img, refr.img, float(scene.cam["bf"]), float(scene.cam["b"]))
    n, nr = ex.frame_stereo_dev_wait()
    assert n == len(refl.kps) and nr == len(refr.kps) and ex.host_redo_count() == 5 * redo and _host_trees_ran(ex) == bool(redo)
    kd, dd = F.download()[:2]
    _assert_extract_equal((kd, dd), (refl.kps, refl.desc), what + " two halves")
    gs, gi = F.grid()
    os_, oi = ob.build_grid(fv)
    assert np.array_equal(gs, os_) and np.array_equal(gi, oi), what + ": grid of the two-halves constructor"
    nf = xb.normal_frame()
    _fused_stereo_on(ex, F, scene, nf["refL"], nf["refR"], nf["uright"], nf["depth"], what + ", then a scene")
    assert ex.host_redo_count() == 5 * redo and not _host_trees_ran(ex)


# ------------------------------------------------------------------ 2. N = 510 / 511 at level 0

@pytest.mark.parametrize("nf,n0", xb.NODE_EDGE)
def test_level_0_target_at_the_node_list_limit(nf, n0):
    """kOctListCap = 2048 nodes, a level needs 4 N + 8: N = 510 (n_features 2350) is the last target the device trees take, and they
    take it without a redo.  N = 511 (n_features 2351) needs 2052: the handle is set up for the host trees from its first frame, like
    ORBG_HOST_OCTREE=1 -- the trees run once, on the host, which is no redo, so the counter stays at 0 and the host trees are seen to
    have run.  Mono and stereo, twice each."""
    scene = xb.textured_scene(640, 480)
    ref = xb.Ref(xb.dot_image(xb.NODE_EDGE_DOTS), nf)
    assert ref.quota[0] == n0 and ref.per_level[0] >= n0
    host = xb.host_from_the_start(nf)
    assert host == (4 * n0 + 8 > xb.LIST_CAP) and (ref.overflowing_levels() == []) == (not host)
    ex = api.ORBextractor(nf, 1.2, 8, 20, 7, 640, 480, n_cams=1)
    _mono_on(ex, ref, "N = %d mono" % n0)
    assert ex.host_redo_count() == 0 and _host_trees_ran(ex) == host
    _assert_levels_and_candidates(ex, 0, ref, "N = %d" % n0)
    ex2 = api.ORBextractor(nf, 1.2, 8, 20, 7, 640, 480, n_cams=2)
    _stereo_on(ex2, ref, ref, "N = %d stereo" % n0)
    assert ex2.host_redo_count() == 0 and _host_trees_ran(ex2) == host
    our, odp = _oracle_matches(ref, ref, scene.cam)
    F = api.Frame()
    _fused_stereo_on(ex2, F, scene, ref, ref, our, odp, "N = %d" % n0)
    assert ex2.host_redo_count() == 0 and _host_trees_ran(ex2) == host


# ------------------------------------------------------------------ 3. levels whose target is 0

@pytest.mark.parametrize("nf", xb.SMALL_FEATURES)
@pytest.mark.parametrize("W,H", xb.SMALL_SHAPES)
def test_small_feature_counts_through_every_constructor(W, H, nf):
    """n_features 1 ... 9: levels whose target is 0 still make the reference's one pass.  One root at 640 x 480 (4 nodes per level, a
    region of 8 or more): no redo.  Four roots at 1241 x 376 (13 to 15 nodes per level, regions of 8 / 12 / 16): the frame goes to the
    host cleanly, one redo per call.  The extractor, the fused stereo constructor (features, uRight, depth, grid) and the fused
    monocular constructor against the oracle.  The monocular constructor's lapping area {0, 1000} holds all of a 640-wide image
    (reversed order, device trees) and a part of a 1241-wide one: that frame goes to the host trees at once, which is no redo.
    At 1241 x 376 and 8 features, the stereo, monocular and RGB-D constructors through every two-halves route (inline, ingest thread,
    device images) with the arrays of orbx_set_frame_outputs(_un) set: the bytes and the grid of the synchronous call."""
    scene = xb.textured_scene(W, H)
    refl, refr = xb.small_ref(W, H, nf, 0), xb.small_ref(W, H, nf, 1)
    redo = xb.expected_redos(refl, refr)
    assert redo == int((W, H) != (640, 480)) == xb.expected_redos(refl)
    what = "%d features at %d x %d" % (nf, W, H)
    ex = api.ORBextractor(nf, 1.2, 8, 20, 7, W, H, n_cams=1)
    _mono_on(ex, refl, what)
    assert ex.host_redo_count() == 2 * redo and _host_trees_ran(ex) == bool(redo)
    _assert_levels_and_candidates(ex, 0, refl, what, levels=False)
    # Frame::Frame(mono)
    rc, okps, odesc, onm = refl.ex.extract(refl.img, (0, 1000), cap=8192)
    assert rc == 0
    whole = W <= 1000
    assert (onm == 0 and np.array_equal(okps, refl.kps[::-1]) and np.array_equal(odesc, refl.desc[::-1])) if whole else 0 < onm < len(okps)
    fvm, keepm = _frame_view(scene, okps, odesc, None, None)
    F = api.Frame()
    n, kps, kun, desc = ex.frame_mono(F, fvm, refl.img, None)
    assert n == len(okps)
    _assert_extract_equal((kps, desc), (okps, odesc), what + " fused mono")
    assert kun.tobytes() == okps.tobytes()
    gs, gi = F.grid()
    os_, oi = ob.build_grid(fvm)
    assert np.array_equal(gs, os_) and np.array_equal(gi, oi), what + ": mono grid"
    assert ex.host_redo_count() == (3 if whole else 2) * redo and _host_trees_ran(ex) == (bool(redo) or not whole)
    # Frame::Frame(stereo)
    ex2 = api.ORBextractor(nf, 1.2, 8, 20, 7, W, H, n_cams=2)
    our, odp = _oracle_matches(refl, refr, scene.cam)
    F2 = api.Frame()
    for _ in range(2):
        _fused_stereo_on(ex2, F2, scene, refl, refr, our, odp, what)
    assert ex2.host_redo_count() == 2 * redo and _host_trees_ran(ex2) == bool(redo)
    # every two-halves route with host outputs, through the redo (one feature count at the shape that makes one)
    if redo and nf == xb.SMALL_FEATURES[-2]:
        fv, keep = _frame_view(scene, refl.kps, refl.desc, our, odp)
        _stereo_routes(ex2, F2, fv, refl.img, refr.img, scene.cam, redo, what)
        # the lapping area {0, 1000} splits the 1241-wide image: host trees at once, which is no redo (a monocular redo:
        # test_monocular_two_halves_routes_through_a_redo)
        _mono_routes(ex, F, fvm, refl.img, 0 if not whole else redo, what)
        dep = scene.depth_image(xb.small_pair(W, H)[2], np.uint16, 5000.0)
        _rgbd_routes(ex, F, fvm, refl.img, dep, float(scene.cam["bf"]), redo, what)


TWO_HALVES_ROUTES = ("submit", "async", "dev_submit")


def _dev(a):
    import torch
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    torch.cuda.synchronize()
    return t


def _two_halves_equal_the_synchronous_call(ex, F, sync, submit, redo, what):
    """sync() -> {name: array} of the synchronous constructor's host outputs, names as in set_frame_outputs(); submit(route) starts the
    two-halves constructor on the same images.  Every route delivers the same bytes into the arrays of orbx_set_frame_outputs(_un),
    leaves the same grid, and the redo counter moves by `redo` per call, the synchronous one included."""
    before = ex.host_redo_count()
    want = {k: v.copy() for k, v in sync().items()}
    n = len(want["kps"])
    want_grid = [g.tobytes() for g in F.grid()]
    assert ex.host_redo_count() == before + redo, what
    out = ex.set_frame_outputs(ex.cap)
    for route in TWO_HALVES_ROUTES:
        for a in out.values():
            a[...] = 0
        before = ex.host_redo_count()
        submit(route)
        assert ex.frame_stereo_dev_wait()[0] == n, (what, route)
        assert ex.host_redo_count() == before + redo, (what, route)
        for k, v in want.items():
            assert out[k][:n].tobytes() == v.tobytes(), (what, route, k)
        assert [g.tobytes() for g in F.grid()] == want_grid, (what, route)
    ex.set_frame_outputs(0)


def _mono_routes(ex, F, fv, img, redo, what):
    d_img = _dev(img)
    H, W = img.shape

    def sync():
        n, kps, kun, desc = ex.frame_mono(F, fv, img, None)
        return dict(kps=kps, kps_un=kun, desc=desc)

    def submit(route):
        if route == "dev_submit":
            ex.frame_mono_submit(F, fv, None, None, device_ptr=d_img.data_ptr(), size=(W, H, W))
        else:
            ex.frame_mono_submit(F, fv, img, None, async_ingest=(route == "async"))

    _two_halves_equal_the_synchronous_call(ex, F, sync, submit, redo, what + " mono")


def _stereo_routes(ex, F, fv, L, R, cam, redo, what):
    d_l, d_r = _dev(L), _dev(R)
    H, W = L.shape
    bf, b = float(cam["bf"]), float(cam["b"])

    def sync():
        n, nr, kl, dl, ur, dp = ex.frame_stereo(F, fv, L, R, bf, b, download=True)
        return dict(kps=kl, desc=dl, uright=ur, depth=dp)

    def submit(route):
        if route == "dev_submit":
            ex.frame_stereo_dev_submit(F, fv, d_l.data_ptr(), d_r.data_ptr(), W, H, W, bf, b)
        else:
            ex.frame_stereo_submit(F, fv, L, R, bf, b, async_ingest=(route == "async"))

    _two_halves_equal_the_synchronous_call(ex, F, sync, submit, redo, what + " stereo")


def _rgbd_routes(ex, F, fv, img, dep, bf, redo, what):
    fac = api.depth_map_factor(5000.0)
    d_img, d_dep = _dev(img), _dev(dep)
    H, W = img.shape
    ptrs, size = (d_img.data_ptr(), d_dep.data_ptr()), (W, H, 1, W, dep.dtype, W * dep.itemsize)

    def sync():
        n, kps, kun, desc, ur, dp = ex.frame_rgbd(F, fv, img, dep, bf, fac)
        assert (dp > 0).any()
        return dict(kps=kps, kps_un=kun, desc=desc, uright=ur, depth=dp)

    def submit(route):
        if route == "dev_submit":
            ex.frame_rgbd_submit(F, fv, None, None, bf, fac, device_ptrs=ptrs, size=size)
        else:
            ex.frame_rgbd_submit(F, fv, img, dep, bf, fac, async_ingest=(route == "async"))

    _two_halves_equal_the_synchronous_call(ex, F, sync, submit, redo, what + " RGB-D")


def test_monocular_two_halves_routes_through_a_redo():
    """The monocular constructor's lapping area {0, 1000} holds all of a 640-wide image, so its frames stay on the device unless a level
    overflows: 4097 dots do, once per call (test_dot_images_at_the_candidate_limit_through_the_monocular_extractor).  Every two-halves
    route, with host outputs, against the synchronous call."""
    ref = xb.dot_ref(4097)
    assert xb.expected_redos(ref) == 1
    fv, keep = _frame_view(xb.textured_scene(640, 480), ref.kps[:0], None, None, None)
    ex = api.ORBextractor(xb.DOT_FEATURES, 1.2, 8, 20, 7, 640, 480, n_cams=1)
    _mono_routes(ex, api.Frame(), fv, np.ascontiguousarray(ref.img), 1, "4097 dots")


# ------------------------------------------------------------------ 4. more than 1024 cells per level

@pytest.mark.parametrize("no_jump", [False, True])
@pytest.mark.parametrize("W,H", xb.LARGE_SHAPES)
def test_large_images_whose_threads_take_more_cells_than_the_speculative_fetch(monkeypatch, W, H, no_jump):
    """1920 x 1080 (9 / 6 / 4 cells per thread at levels 0 / 1 / 2), 992 x 992 (1024 cells: the last size on the speculative fetch
    alone) and 1022 x 1022 (1089: the first on the two plain loops): the candidates of every level, keypoints and descriptors, on the
    device without a redo; and with ORBG_OCT_NO_JUMP=1 in the environment when the handle is created (every pass replayed one by one)."""
    ref = xb.large_ref(W, H)
    assert xb.expected_redos(ref) == 0
    # the switch is per handle: the library reads it (getenv) whenever a handle sets up its geometry -- in orbx_create for
    # max_width x max_height, the size of the image here -- and the handle keeps what it read; so it is set in this process around
    # the handle's creation and extraction
    if no_jump:
        monkeypatch.setenv("ORBG_OCT_NO_JUMP", "1")
    else:
        monkeypatch.delenv("ORBG_OCT_NO_JUMP", raising=False)
    ex = api.ORBextractor(xb.LARGE_FEATURES, 1.2, 8, 20, 7, W, H, n_cams=1)
    what = "%d x %d%s" % (W, H, " without the jump start" if no_jump else "")
    _mono_on(ex, ref, what, calls=1)
    monkeypatch.delenv("ORBG_OCT_NO_JUMP", raising=False)
    assert ex.host_redo_count() == 0 and not _host_trees_ran(ex)
    _assert_levels_and_candidates(ex, 0, ref, what, levels=not no_jump)


# ------------------------------------------------------------------ 5. x beyond 3900 in a 12-bit field

def test_wide_image_with_keypoints_in_its_last_columns():
    """4000 x 100, four levels (the top one has no cell row), 58 / 65 / 74 roots: pyramid, candidates with x up to 3978 at level 0, and
    keypoints with x beyond 3900 at levels 0, 1 and 2 as the oracle's, on the device."""
    W, H = xb.WIDE_SHAPE
    ref = xb.wide_ref()
    assert xb.expected_redos(ref) == 0 and float(ref.kps["x"].max()) > 3900
    ex = api.ORBextractor(xb.WIDE_FEATURES, 1.2, xb.WIDE_LEVELS, 20, 7, W, H, n_cams=1)
    _mono_on(ex, ref, "4000 x 100")
    assert ex.host_redo_count() == 0 and not _host_trees_ran(ex)
    _assert_levels_and_candidates(ex, 0, ref, "4000 x 100")
    # the mono constructor's lapping area {0, 1000} splits this image: host trees at once, which is no redo
    rc, okps, odesc, onm = ref.ex.extract(ref.img, (0, 1000), cap=8192)
    nm, kps, desc = ex(ref.img, (0, 1000))
    assert rc == 0 and nm == onm and 0 < nm < len(kps)
    _assert_extract_equal((kps, desc), (okps, odesc), "4000 x 100, lapping area {0, 1000}")
    assert ex.host_redo_count() == 0 and _host_trees_ran(ex)


# ------------------------------------------------------------------ 6. the stereo matcher with an empty side

@pytest.mark.parametrize("case", xb.EMPTY_SIDE_CASES)
def test_stereo_matcher_with_an_empty_side(case):
    """A right image without features (the matcher's first right keypoint is requested before its loop), a left one without, features on
    both sides but none in any left keypoint's row band, both flat: ComputeStereoMatches on the extraction and the fused constructor
    give the oracle's uRight / depth (all -1: the median over zero matches is never taken), the grid is the oracle's, and
    SearchByProjection(Current, Last) on the frame the constructor leaves answers as the oracle does."""
    scene = xb.textured_scene(640, 480)
    cam = scene.cam
    e = xb.empty_side_ref(case)
    refl, refr, our, odp = e["refL"], e["refR"], e["uright"], e["depth"]
    assert (our == -1).all() and xb.expected_redos(refl, refr) == 0
    ex = api.ORBextractor(xb.STEREO_FEATURES, 1.2, 8, 20, 7, 640, 480, n_cams=2)
    F = api.Frame()
    nf = xb.normal_frame()
    last = dict(kps=nf["refL"].kps, desc=nf["refL"].desc, depth=nf["depth"], Tcw=nf["Tcw"])
    lv, keep_l = helpers.make_lastframe(scene, last, np.random.RandomState(11))
    T = synth.perturb_pose(scene.stereo_pair(2)[2], np.random.RandomState(12)).astype(np.float32)
    for _ in range(2):
        _stereo_on(ex, refl, refr, case, calls=1)
        ur, dp = ex.ComputeStereoMatches(float(cam["bf"]), float(cam["b"]), n_left=len(refl.kps))
        assert len(ur) == len(our) and np.array_equal(_bits(ur), _bits(our)) and np.array_equal(_bits(dp), _bits(odp)), case
        fv, keep = _fused_stereo_on(ex, F, scene, refl, refr, our, odp, case)
        n = len(refl.kps)
        a0, b0 = np.full(max(n, 1), -1, np.int32), np.zeros(max(n, 1), np.int32)
        g = api.ORBmatcher(0.9, True).SearchByProjectionFrame(F, T, lv, 7.0, False, a0, b0)
        o = ob.search_by_projection_frame(fv, T, lv, 7.0, False, True, a0, b0)
        assert g[2] == o[2] and np.array_equal(g[0], o[0]) and np.array_equal(g[1], o[1]), case
        assert (o[2] > 50) == (n > 0)                                  # a frame with features is found again, stereo matches or not
    assert ex.host_redo_count() == 0 and not _host_trees_ran(ex)
    _normal_frame_on(ex, case)
