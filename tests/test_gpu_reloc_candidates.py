"""KeyFrameDatabase::DetectRelocalizationCandidates on the device-resident database against tests/reloc_db_model.py: candidate lists
equal, mRelocScore bit-equal, over consecutive queries that share the score state; the database at its edges."""
import numpy as np
import pytest

import helpers
import reloc_db_model as rm
from multi_orbslam3_amd import api, views

pytestmark = pytest.mark.gpu


def _database(db):
    K = len(db["bows"])
    v, keep = views.database_view(db["inv"], db["bows"], db["covis"], db["map_id"], np.zeros(K, np.uint8), np.zeros(K, np.uint8), db["n_words"])
    return api.KeyFrameDatabase(v, keep)


def test_thirty_queries_share_the_reloc_scores():
    rng = np.random.RandomState(21)
    db = helpers.random_database(rng, n_kfs=400, n_words=5000)
    db["n_words"] += 1                                           # one word no keyframe contains
    D = _database(db)
    K = 400
    sg, sm = np.zeros(K, np.float32), np.zeros(K, np.float32)
    total = dropped_by_map = 0
    for q in range(30):
        kq = rng.randint(K)
        qw, qv = db["bows"][kq]
        if q % 3 == 1:                                           # a frame between two keyframes: a mix of their words
            w2, v2 = db["bows"][(kq + 1) % K]
            qw = np.union1d(qw[::2], w2[::2]).astype(np.int32)
            qv = rng.rand(len(qw)) + 0.05
            qv /= qv.sum()
        if q == 7:                                               # a query that shares no word with anybody
            qw, qv = np.array([db["n_words"] - 1], np.int32), np.array([1.0])
        qmap = int(db["map_id"][kq]) if q % 5 else 1 - int(db["map_id"][kq])
        got = D.DetectRelocalizationCandidates(qw, qv, qmap, sg)
        want = rm.detect_relocalization_candidates(db, qw, qv, qmap, sm)
        assert got.tolist() == want, (q, got, want)
        assert np.array_equal(sg.view(np.uint32), sm.view(np.uint32)), q
        total += len(want)
        dropped_by_map += int(q % 5 == 0 and not want)
    assert total >= 15 and dropped_by_map >= 3
    D.close()


@pytest.mark.parametrize("case", ["empty", "no_shared_word", "other_map", "one_kf"])
def test_edge_databases(case):
    rng = np.random.RandomState({"empty": 1, "no_shared_word": 2, "other_map": 3, "one_kf": 4}[case])
    if case == "empty":
        db = dict(inv={}, bows=[], covis=[], map_id=np.zeros(0, np.int32), n_words=100)
    elif case == "one_kf":
        db = helpers.random_database(rng, n_kfs=1, n_words=500)
    else:
        db = helpers.random_database(rng, n_kfs=120, n_words=2000)
        db["n_words"] += 3                                        # three words no keyframe contains
    D = _database(db)
    K = len(db["bows"])
    sg, sm = np.zeros(K, np.float32), np.zeros(K, np.float32)
    for q in range(4):
        if K == 0:
            qw, qv = np.array([3, 9], np.int32), np.array([0.5, 0.5])
        else:
            qw, qv = db["bows"][rng.randint(K)]
        if case == "no_shared_word":
            qw, qv = np.array([2000, 2001, 2002], np.int32), np.array([0.3, 0.3, 0.4])
        qmap = 7 if case == "other_map" else 0
        got = D.DetectRelocalizationCandidates(qw, qv, qmap, sg)
        want = rm.detect_relocalization_candidates(db, qw, qv, qmap, sm)
        assert got.tolist() == want, (case, q)
        assert np.array_equal(sg.view(np.uint32), sm.view(np.uint32))
        if case in ("empty", "no_shared_word", "other_map"):
            assert want == []
        if case == "other_map":
            assert sm.any()                                      # scored all the same
        if case == "one_kf":
            assert want == [0]
    D.close()
