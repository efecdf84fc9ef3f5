"""Tracking::Relocalization's five numerical steps chained on the synthetic scene, every one on the device: candidates from a 20-keyframe
database, SearchByBoW against each, MLPnPsolver for all of them in one launch, PoseOptimization on the returned pose with the inlier
matches, the guided SearchByProjection.  A sanity check on the chain, not a parity bound."""
import numpy as np
import pytest

import helpers
from multi_orbslam3_amd import api, synth, views

pytestmark = pytest.mark.gpu

RELOC = (0.99, 10, 300, 6, 0.5, 5.991)


def _bow(fr, n_words=4096):
    """A stand-in vocabulary: the word of a feature is 12 bits of its descriptor; L1-normalised counts."""
    w = (fr["desc"][:, 0].astype(np.int64) << 4) | (fr["desc"][:, 1].astype(np.int64) >> 4)
    words, counts = np.unique(w, return_counts=True)
    return words.astype(np.int32), counts / counts.sum()


def _nodes(fr):
    return (fr["desc"][:, 0].astype(np.int64) >> 3) * 2 + (fr["kps"]["octave"] // 4)


def test_chain_candidates_bow_mlpnp_pose_projection(scene):
    cam = scene.cam
    K = tuple(float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    ids = list(range(0, 40, 2))
    kfs = [helpers.oracle_stereo_frame(scene, k, n_features=600) for k in ids]
    cur = helpers.oracle_stereo_frame(scene, 21, n_features=600)
    n_cur = len(cur["kps"])
    # 1. DetectRelocalizationCandidates on a database of the 20 keyframes (one map; neighbours in time are covisible)
    bows = [_bow(f) for f in kfs]
    inv = {}
    for k, (w, _) in enumerate(bows):
        for x in w:
            inv.setdefault(int(x), []).append(k)
    covis = [[j for j in (k - 1, k + 1) if 0 <= j < 20] for k in range(20)]
    dv, dkeep = views.database_view(inv, bows, covis, np.zeros(20, np.int32), np.zeros(20, np.uint8), np.zeros(20, np.uint8), 4096)
    D = api.KeyFrameDatabase(dv, dkeep)
    qw, qv = _bow(cur)
    cands = D.DetectRelocalizationCandidates(qw, qv, 0, np.zeros(20, np.float32))
    assert len(cands) >= 1 and (10 in cands or 11 in cands)          # frames 20 / 22 are the neighbours of frame 21
    # 2. SearchByBoW(pKF, mCurrentFrame, vvpMapPointMatches[i]) and the solvers' constructors
    fvc, keepc = helpers.frame_view_of(scene, cur)
    F = api.Frame().upload(fvc, keepc)
    fv_cur, kc = views.featvec_view(*views.featvec_from_nodes(_nodes(cur)))
    sig2 = (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2
    xy = np.stack([cur["kps"]["x"], cur["kps"]["y"]], 1).astype(np.float32)
    bearing = np.stack([(xy[:, 0] - np.float32(K[2])) / np.float32(K[0]), (xy[:, 1] - np.float32(K[3])) / np.float32(K[1]), np.ones(n_cur, np.float32)], 1)
    probs, kept, all_matches, world = [], [], {}, {}
    matcher = api.ORBmatcher(0.75, True)
    for c in cands.tolist():
        kf = kfs[c]
        valid = (kf["depth"] > 0).astype(np.uint8)
        fv_kf, kk = views.featvec_view(*views.featvec_from_nodes(_nodes(kf)))
        matches, nm = matcher.SearchByBoW(F, fv_cur, kf["desc"], valid, kf["kps"]["angle"], fv_kf)
        if nm < 15:
            continue
        Pw, _ = synth.unproject_to_world(kf["kps"], kf["depth"], kf["Tcw"], cam)
        i = np.nonzero(matches >= 0)[0]
        probs.append(api.MLPnPProblem(xy[i], sig2[cur["kps"]["octave"][i]], bearing[i], Pw[matches[i]], K, i, n_cur))
        kept.append(c); all_matches[c] = matches; world[c] = Pw.astype(np.float32)
    assert probs
    # 3. every candidate's first iterate(5) in one launch
    res = api.MLPnPsolver.solve_batch(probs, [RELOC] * len(probs), seed=5)
    ok = [b for b, r in enumerate(res) if r.returned]
    assert ok, [(r.bNoMore, r.best_inliers) for r in res]
    b = ok[0]
    c, r = kept[b], res[b]
    kf, matches, Pw = kfs[c], all_matches[c], world[c]
    assert r.vbInliers.sum() == r.nInliers > 10
    # 4. PoseOptimization on the returned pose with the inlier matches
    j = np.nonzero(r.vbInliers)[0]
    p, keepp = views.pose_opt_problem(Pw[matches[j]], xy[j, 0], xy[j, 1], np.full(len(j), -1, np.float32), 1.0 / sig2[cur["kps"]["octave"][j]],
                                      K + (float(cam["bf"]),), r.Tcw)
    po = api.Optimizer().PoseOptimization(p)
    n_good = int(po.n_inliers)
    T = po.Tcw
    Tgt = np.asarray(cur["Tcw"], np.float64)
    centre = lambda M: -M[:3, :3].T @ M[:3, 3]          # noqa: E731
    d_pos = np.linalg.norm(centre(T.astype(np.float64)) - centre(Tgt))
    d_ang = np.degrees(np.arccos(np.clip((np.trace(T[:3, :3].astype(np.float64) @ Tgt[:3, :3].T) - 1) / 2, -1, 1)))
    print("candidates %s, solver of keyframe %d returned %d inliers, PoseOptimization %d good, %.4f m / %.3f deg from the truth" %
          (cands.tolist(), ids[c], r.nInliers, n_good, d_pos, d_ang))
    assert d_pos < 0.05 and d_ang < 1.0
    # 5. SearchByProjection(mCurrentFrame, pKF, sFound, 10, 100)
    amp = np.full(n_cur, -1, np.int32)
    good = j[po.outlier[: len(j)] == 0]
    amp[good] = matches[good]
    nk = len(kf["kps"])
    mp = synth.map_from_frame(kf["kps"], kf["desc"], kf["depth"], kf["Tcw"], cam)
    pos = np.zeros((nk, 3), np.float32); nrm = np.zeros((nk, 3), np.float32); dmin = np.zeros(nk, np.float32); dmax = np.ones(nk, np.float32)
    desc = np.zeros((nk, 32), np.uint8); bad = np.ones(nk, np.uint8)
    ix = mp["src_idx"]
    pos[ix] = mp["pos"]; nrm[ix] = mp["normal"]; dmin[ix] = mp["min_dist"]; dmax[ix] = mp["max_dist"]; desc[ix] = mp["desc"]; bad[ix] = 0
    wv, keepw = views.worldpoints_view(pos, nrm, dmin, dmax, desc, np.full(nk, 2, np.int32), bad, None)
    KP = api.LocalMap().upload(wv)
    found = np.zeros(nk, np.uint8); found[matches[good]] = 1
    amp2, n_add = api.ORBmatcher(0.9, True).SearchByProjectionReloc(F, T, KP, kf["kps"]["angle"], amp, 10, 100, found)
    print("guided search: %d additional, %d in all" % (n_add, n_good + n_add))
    assert n_good + n_add >= 50 and (amp2 >= 0).sum() >= 50
