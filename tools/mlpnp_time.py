"""Wall time of MLPnPsolver and DetectRelocalizationCandidates on the device: median of >= 200 synchronised calls after warm-up, for
one solve_batch of B = 1, 5 and 20 candidate keyframes at n = 30 and n = 200 matches each (Relocalization's parameters, 50 % wrong
matches: 35 hypotheses per solver), and for one DetectRelocalizationCandidates query on a database of 400 keyframes.

    python tools/mlpnp_time.py [--reps 200] [--one N]      (--one N: a single solve_batch of 5 at n = N and exit: for a kernel trace)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers                                  # noqa: E402  (the seeded database)
import mlpnp_model as mm                        # noqa: E402  (the seeded scenes; nothing of the model runs here)
from multi_orbslam3_amd import api, views       # noqa: E402

RELOC = (0.99, 10, 300, 6, 0.5, 5.991)


def problem(n, seed):
    sc = mm.make_scene(seed, n, 0.5)
    return api.MLPnPProblem(sc["P2D"], sc["sigma2"], sc["bearing"], sc["P3Dw"], sc["K"], sc["kp_index"], sc["m"])


def median_us(fn, reps, warm=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts))


def batch(n, B, seed=0):
    probs = [problem(n, 7000 + 100 * n + b) for b in range(B)]
    its = [api.mlpnp_ransac_iterations(n, *RELOC)[0] for _ in probs]
    draws = [api.mlpnp_draws(n, k, seed + b) for b, k in enumerate(its)]
    return probs, [RELOC] * B, draws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--one", type=int, default=0)
    a = ap.parse_args()
    if a.one:
        rs = api.MLPnPsolver.solve_batch(*batch(a.one, 5))
        print("one batch of 5, n = %d: returned %s, inliers %s" % (a.one, [r.returned for r in rs], [r.nInliers for r in rs]))
        return
    for n in (30, 200):
        for B in (1, 5, 20):
            args = batch(n, B)
            rs = api.MLPnPsolver.solve_batch(*args)
            print("solve_batch B = %2d n = %3d: %8.1f us   (%d hypotheses, %d solvers returned)" % (
                B, n, median_us(lambda: api.MLPnPsolver.solve_batch(*args), a.reps), B * api.mlpnp_ransac_iterations(n, *RELOC)[0],
                sum(r.returned for r in rs)))
    rng = np.random.RandomState(21)
    db = helpers.random_database(rng, n_kfs=400, n_words=5000)
    K = 400
    v, keep = views.database_view(db["inv"], db["bows"], db["covis"], db["map_id"], np.zeros(K, np.uint8), np.zeros(K, np.uint8), db["n_words"])
    D = api.KeyFrameDatabase(v, keep)
    score = np.zeros(K, np.float32)
    qw, qv = db["bows"][123]
    got = D.DetectRelocalizationCandidates(qw, qv, int(db["map_id"][123]), score)
    print("DetectRelocalizationCandidates, 400 keyframes, %d query words: %8.1f us   (%d candidates)" % (
        len(qw), median_us(lambda: D.DetectRelocalizationCandidates(qw, qv, int(db["map_id"][123]), score), a.reps), len(got)))


if __name__ == "__main__":
    main()
