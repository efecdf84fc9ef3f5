"""Frames of more than 4096 features for the frame searches of csrc/matcher.hip (tests/test_gpu_path_boundaries.py on the device,
tests/test_path_boundaries_cpu.py for the oracle's side).  stage_occupancy passes "this feature already holds a map point" as a
bitmask in the kernel arguments up to kOccBits = 4096 features and as two device arrays beyond; feature indices travel in 16 bits, so
ORBG_MAX_FRAME_FEATURES - 1 = 65534 is the largest frame.  The extractor never gives more than 3500 features, so the frames here are
an oracle frame of the scene (real matches exist) filled up with synthetic features and permuted.  Nothing here touches the GPU."""
import numpy as np

import helpers
from multi_orbslam3_amd import _capi as capi
from multi_orbslam3_amd import synth, views
from oracle import binding as ob

FRAME_SIZES = (4096, 4097, 40000)
ENTRIES = ("mps", "local", "frame", "reloc", "sim3")
_FRAMES = {}


def _oracle_frame(scene, k):
    if k not in _FRAMES:
        _FRAMES[k] = helpers.oracle_stereo_frame(scene, k)
    return _FRAMES[k]


def fill_features(kps, desc, n, rng, width, height, uright=None, depth=None):
    """kps / desc (and uright / depth) followed by synthetic features up to n: position uniform inside the bounds, octave 0 - 7, a random
    angle, a random descriptor, uright = -1 (no depth)."""
    n0 = len(kps)
    assert n >= n0
    e = n - n0
    k = np.zeros(n, capi.KEYPOINT_DTYPE)
    k[:n0] = kps
    k["x"][n0:] = rng.uniform(1.0, width - 1.0, e)
    k["y"][n0:] = rng.uniform(1.0, height - 1.0, e)
    k["octave"][n0:] = rng.randint(0, 8, e)
    k["angle"][n0:] = rng.uniform(0.0, 360.0, e)
    k["size"][n0:] = 31.0
    k["response"][n0:] = rng.uniform(20.0, 120.0, e)
    d = np.concatenate([desc, rng.randint(0, 256, (e, 32)).astype(np.uint8)])
    ur = None if uright is None else np.concatenate([uright, np.full(e, -1.0, np.float32)])
    dp = None if depth is None else np.concatenate([depth, np.full(e, -1.0, np.float32)])
    return k, d, ur, dp


def big_frame(scene, k, n, seed):
    """Oracle frame k of the scene filled up to n features and permuted with a fixed seed, so that its real features sit on both sides
    of index 4096 (and of 32768).  -> dict(kps, desc, uright, depth, Tcw, real: bool per feature)."""
    fr = _oracle_frame(scene, k)
    rng = np.random.RandomState(seed)
    kps, desc, ur, dp = fill_features(fr["kps"], fr["desc"], n, rng, scene.W, scene.H, fr["uright"], fr["depth"])
    perm = rng.permutation(n)
    return dict(kps=np.ascontiguousarray(kps[perm]), desc=np.ascontiguousarray(desc[perm]), uright=np.ascontiguousarray(ur[perm]),
                depth=np.ascontiguousarray(dp[perm]), Tcw=fr["Tcw"], real=perm < len(fr["kps"]))


def swap_features(fr, i, j):
    for key in ("kps", "desc", "uright", "depth", "real"):
        a = fr[key]
        t = a[i].copy(); a[i] = a[j]; a[j] = t


def occupancy(n, seed):
    """-> (assigned_mp with 30 % of the features holding a point, assigned_obs with every such point observed, assigned_obs with a
    third of them at 0 observations: those features count as free).  Feature 4096 holds nothing."""
    rng = np.random.RandomState(seed)
    amp = np.full(n, -1, np.int32)
    occ = rng.rand(n) < 0.3
    if n > 4096:
        occ[4096] = False
    amp[occ] = rng.randint(0, 1000, int(occ.sum()))
    aob_all = np.where(occ, rng.randint(1, 5, n), 0).astype(np.int32)
    aob_third = np.where(rng.rand(n) < 1.0 / 3.0, 0, aob_all).astype(np.int32)
    return amp, aob_all, aob_third


class FrameCase:
    """One entry point on one frame size: the frame, the call's other inputs, the occupancy variants and the oracle's answers.
    run(amp, aob) -> (assigned_mp out, assigned_obs out or None, number of matches) of the oracle; the device test supplies its own."""

    def __init__(self, scene, entry, n):
        self.entry, self.n, self.scene = entry, n, scene
        rng = np.random.RandomState(1000 + ENTRIES.index(entry))
        cur_k = dict(mps=5, local=5, frame=11, reloc=20, sim3=14)[entry]
        self.fr = big_frame(scene, cur_k, n, 5000 + n)
        self.T = synth.perturb_pose(self.fr["Tcw"], rng).astype(np.float32)
        self.has_obs = entry in ("mps", "local", "frame")
        if entry in ("mps", "local"):
            self.mp = helpers.local_map_from(scene, [_oracle_frame(scene, k) for k in (0, 4, 8)], rng)
            self.skip = (rng.rand(len(self.mp["pos"])) < 0.05).astype(np.uint8)
        elif entry == "frame":
            self.lv, self._keep_lv = helpers.make_lastframe(scene, _oracle_frame(scene, 10), rng)
        elif entry == "reloc":
            kf = _oracle_frame(scene, 18)
            mp = synth.map_from_frame(kf["kps"], kf["desc"], kf["depth"], kf["Tcw"], scene.cam)
            nk = len(kf["kps"])
            pos = np.zeros((nk, 3), np.float32); nrm = np.zeros((nk, 3), np.float32); dmin = np.zeros(nk, np.float32); dmax = np.ones(nk, np.float32)
            desc = np.zeros((nk, 32), np.uint8); bad = np.ones(nk, np.uint8)
            idx = mp["src_idx"]
            pos[idx] = mp["pos"]; nrm[idx] = mp["normal"]; dmin[idx] = mp["min_dist"]; dmax[idx] = mp["max_dist"]; desc[idx] = mp["desc"]; bad[idx] = 0
            self.kf_angle = kf["kps"]["angle"].copy()
            self.found = np.zeros(nk, np.uint8); self.found[idx[rng.rand(len(idx)) < 0.1]] = 1
            self.wv, self._keep_wv = views.worldpoints_view(pos, nrm, dmin, dmax, desc, np.full(nk, 2, np.int32), bad, None)
        elif entry == "sim3":
            self.mp = helpers.local_map_from(scene, [_oracle_frame(scene, k) for k in (12, 16)], rng)
            self.found = (rng.rand(len(self.mp["pos"])) < 0.1).astype(np.uint8)
            self.skip = (rng.rand(len(self.mp["pos"])) < 0.05).astype(np.uint8)
            self.S = self.T.copy()
            self.S[:3, :] *= np.float32(1.3)
        self.amp0, self.aob_all, self.aob_third = occupancy(n, 6000 + n)
        self.none = np.full(n, -1, np.int32)
        self._views()
        if n == 4097:
            self._pin_a_match_on_feature_4096()
        self.o_none = self.run(self.none, np.zeros(n, np.int32))
        self.o_all = self.run(self.amp0, self.aob_all)
        self.o_third = self.run(self.amp0, self.aob_third) if self.has_obs else None

    def _views(self):
        """The frame view (the oracle and orbm_frame_upload take the same one) and the views that are computed from it."""
        p = self.scene.frame_view_params()
        fr = self.fr
        self.fv, self._keep_fv = views.frame_view(fr["kps"], fr["desc"], fr["uright"], fr["depth"], p["bounds"], p["cam"], 8, 1.2)
        if self.entry in ("mps", "local"):
            mp = self.mp
            self.wv, self._keep_wv = helpers.world_view_of(mp)
            self.wv_skip, self._keep_wv2 = helpers.world_view_of(mp, self.skip)
            tr = ob.is_in_frustum(self.fv, self.T, self.wv)
            self.mv, self._keep_mv = views.mappoints_view(tr["track_in_view"], mp["bad"], tr["proj_x"], tr["proj_y"], tr["proj_xr"], tr["track_depth"],
                                                          tr["scale_level"], tr["view_cos"], mp["desc"], mp["n_obs"])
            self.want_vis = np.asarray(tr["track_in_view"]).astype(np.uint8) * (1 - self.skip) * (1 - mp["bad"])
        elif self.entry == "sim3":
            self.wv, self._keep_wv = helpers.world_view_of(self.mp, self.skip)

    def run(self, amp, aob):
        e = self.entry
        if e == "mps":
            return ob.search_by_projection_mps(self.fv, self.mv, 3.0, True, 4.0, 0.8, amp, aob)
        if e == "local":
            return ob.search_local_points(self.fv, self.wv_skip, self.T, 3.0, False, 0.0, 0.8, amp, aob)
        if e == "frame":
            return ob.search_by_projection_frame(self.fv, self.T, self.lv, 7.0, False, True, amp, aob)
        if e == "reloc":
            a, c = ob.search_by_projection_reloc(self.fv, self.T, self.wv, self.kf_angle, amp, 10.0, 100, True, self.found)
            return a, None, c
        a, c = ob.search_by_projection_sim3(self.fv, self.wv, self.S, amp, 8, 1.5, self.found, False)
        return a, None, c

    def _newly(self, o, aob):
        """Features that hold a point after the call and were free before it."""
        free = (self.amp0 < 0) | ((aob <= 0) if self.has_obs else False)
        return free & (o[0] >= 0) & (o[0] != self.amp0)

    def _pin_a_match_on_feature_4096(self):
        """n = 4097 has ONE feature beyond 4096: a real feature that the occupied call matches changes places with it."""
        o = self.run(self.amp0, self.aob_all)
        cand = np.nonzero(self._newly(o, self.aob_all) & (self.amp0 < 0))[0]
        assert len(cand) > 0
        if not self._newly(o, self.aob_all)[4096]:
            swap_features(self.fr, int(cand[len(cand) // 2]), 4096)
            self._views()

    def check_not_vacuous(self):
        """The issue's conditions on every case, from the oracle's answers (the device must give those bit for bit)."""
        n = self.n
        assert self.fv.n == n and len(self.amp0) == n
        assert 0.25 * n < (self.amp0 >= 0).sum() < 0.35 * n
        runs = [(self.o_all, self.aob_all)] + ([(self.o_third, self.aob_third)] if self.has_obs else [])
        for o, aob in runs:
            new = np.nonzero(self._newly(o, aob))[0]
            assert len(new) >= 20
            if n > 4096:
                assert (new >= 4096).any(), "no match on a feature beyond 4096"
            if n > 32768:
                assert (new >= 32768).sum() >= 5, "no match on a feature beyond 32768"
            # occupancy decided something: features the free call matches keep the point they held
            occupied = (self.amp0 >= 0) & ((aob > 0) if self.has_obs else True)
            blocked = occupied & (self.o_none[0] >= 0)
            assert blocked.sum() >= 20 and np.array_equal(o[0][occupied], self.amp0[occupied])
            assert (o[0][blocked] != self.o_none[0][blocked]).sum() >= 20           # results that differ from the free call's
        if self.has_obs:
            freed = (self.amp0 >= 0) & (self.aob_third <= 0)
            assert 0.08 * n < freed.sum() < 0.12 * n
            assert (self.o_third[0] != self.o_all[0]).sum() >= 5 and (self.o_third[0][freed] != self.amp0[freed]).sum() >= 5
        return True


# ------------------------------------------------------------------ two-camera frames
# The rig forms stage each camera's occupancy for that camera's frame object, so the device arrays are reached by a camera of more
# than 4096 features, not by left + right > 4096: "sum" (2400 + 1697 = 4097, the global index crosses 4096 inside the right camera)
# stays on the bitmasks, "left" (5000 + 1697) takes the arrays for the left camera.
RIG_SIZES = {"sum": (2400, 1697), "left": (5000, 1697)}
RIG_FORMS = ("mps_rig", "frame_rig")


class RigCase:
    """synth.make_rig_track_scene with both cameras' features filled up to (n_left, n_right) and permuted, the stereo partner tables
    carried along; 30 % of all features hold a point, with the two assigned_obs variants of the single-camera cases."""

    def __init__(self, form, size):
        self.form, self.size = form, size
        nl, nr = RIG_SIZES[size]
        self.nl, self.nr = nl, nr
        sc = dict(synth.make_rig_track_scene(occupied_frac=0.0))
        rng = np.random.RandomState(77 + nl)
        nl0, nr0 = len(sc["kps_left"]), len(sc["kps_right"])
        kl, dl, _, _ = fill_features(sc["kps_left"], sc["desc_left"], nl, rng, sc["size"], sc["size"])
        kr, dr, _, _ = fill_features(sc["kps_right"], sc["desc_right"], nr, rng, sc["size"], sc["size"])
        pl, pr = rng.permutation(nl), rng.permutation(nr)               # new index i holds old feature p[i]
        il, ir = np.argsort(pl), np.argsort(pr)                        # old -> new
        l2r = np.full(nl, -1, np.int32); r2l = np.full(nr, -1, np.int32)
        old = np.nonzero(sc["left_to_right"] >= 0)[0]
        l2r[il[old]] = ir[sc["left_to_right"][old]]
        r2l[l2r[l2r >= 0]] = np.nonzero(l2r >= 0)[0]
        sc.update(kps_left=np.ascontiguousarray(kl[pl]), desc_left=np.ascontiguousarray(dl[pl]), kps_right=np.ascontiguousarray(kr[pr]),
                  desc_right=np.ascontiguousarray(dr[pr]), left_to_right=l2r, right_to_left=r2l)
        self.sc = sc
        self.real = np.concatenate([pl < nl0, pr < nr0])
        n = nl + nr
        self.n = n
        self.amp0, self.aob_all, self.aob_third = occupancy(n, 6100 + n)
        if form == "frame_rig":
            last = synth.rig_last_frame(sc, motion=(0.03, 0.01, 0.02))
            self.lv, self._keep_lv = views.lastframe_view(last["mp_valid"], last["outlier"], last["world_pos"], last["desc"], last["octave"], last["angle"],
                                                          last["n_obs"], last["Tcw"])
        self._views()
        if n == 4097:
            self._pin_a_match_on_feature_4096()
        self.none = np.full(n, -1, np.int32)
        self.o_none = self.run(self.none, np.zeros(n, np.int32))
        self.o_all = self.run(self.amp0, self.aob_all)
        self.o_third = self.run(self.amp0, self.aob_third)

    def _views(self):
        sc = self.sc
        self.fl, self.fr, self.wv, self.rig, self._keep = helpers.rig_track_views(sc)
        if self.form == "mps_rig":
            a, b = ob.is_in_frustum_rig(self.fl, sc["Tcw"], self.rig, sc["Tlr"], self.wv)
            self.mv, self.mvr, self._keep2 = helpers.rig_mappoint_views(sc, a, b)

    def run(self, amp, aob):
        sc = self.sc
        if self.form == "mps_rig":
            return ob.search_by_projection_mps_rig(self.fl, self.fr, self.mv, self.mvr, sc["left_to_right"], sc["right_to_left"], 3.0, True, 6.0, 0.8, amp, aob)
        return ob.search_by_projection_frame_rig(self.fl, self.fr, sc["Tcw"], self.rig, self.lv, 7.0, False, True, amp, aob)

    def _newly(self, o, aob):
        return ((self.amp0 < 0) | (aob <= 0)) & (o[0] >= 0) & (o[0] != self.amp0)

    def _pin_a_match_on_feature_4096(self):
        """left + right = 4097: global index 4096 is the right camera's last feature; a right feature that the occupied call matches changes
        places with it."""
        sc, nl = self.sc, self.nl
        o = self.run(self.amp0, self.aob_all)
        new = self._newly(o, self.aob_all)
        if new[4096]:
            return
        last = 4096 - nl
        cand = np.nonzero(new[nl:] & (self.amp0[nl:] < 0))[0]
        assert len(cand) > 0
        j = int(cand[len(cand) // 2])
        for key in ("kps_right", "desc_right", "right_to_left"):
            t = sc[key][j].copy(); sc[key][j] = sc[key][last]; sc[key][last] = t
        for x in (j, last):                                              # the left partners follow
            if sc["right_to_left"][x] >= 0:
                sc["left_to_right"][sc["right_to_left"][x]] = x
        self.real[[nl + j, nl + last]] = self.real[[nl + last, nl + j]]
        self._views()

    def check_not_vacuous(self):
        nl, n = self.nl, self.n
        sc = self.sc
        assert self.fl.n == nl and self.fr.n == self.nr and (sc["left_to_right"] >= 0).sum() == (sc["right_to_left"] >= 0).sum() > 50
        pairs = np.nonzero(sc["left_to_right"] >= 0)[0]
        assert np.array_equal(sc["right_to_left"][sc["left_to_right"][pairs]], pairs)
        for o, aob in ((self.o_all, self.aob_all), (self.o_third, self.aob_third)):
            new = np.nonzero(self._newly(o, aob))[0]
            assert (new < nl).sum() >= 20 and (new >= nl).sum() >= 20
            assert (new >= 4096).any()
            if self.size == "left":
                assert ((new >= 4096) & (new < nl)).sum() >= 5          # left features beyond 4096: the camera whose occupancy travels in arrays
            occupied = (self.amp0 >= 0) & (aob > 0)
            blocked = occupied & (self.o_none[0] >= 0)
            assert blocked.sum() >= 20 and (o[0][blocked] != self.o_none[0][blocked]).sum() >= 20
        assert (self.o_third[0] != self.o_all[0]).sum() >= 5
        return True
