"""DetectRelocalizationCandidates without a GPU: the checker (tests/reloc_db_model.py) on a hand-computed database, and the entry point's
argument checks and symbols."""
import ctypes as C
import os
import re

import numpy as np

import reloc_db_model as rm
from multi_orbslam3_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _db():
    # 5 keyframes, 7 words.  The query = words {0, 1, 2} at 1/3 each.
    #   KF0 shares 3 words (map 0); KF1 shares 2 (int(3 * 0.8f) = 2, needs > 2: not scored); KF2 shares 3 and lies in map 1;
    #   KF3 shares 3 (map 0) and is covisible with KF0 and KF1; KF4 shares none.
    third = 1 / 3
    bows = [(np.array([0, 1, 2], np.int32), np.array([third, third, third])), (np.array([0, 1, 5], np.int32), np.array([0.25, 0.25, 0.5])),
            (np.array([0, 1, 2, 4], np.int32), np.array([0.25, 0.25, 0.25, 0.25])), (np.array([0, 1, 2, 6], np.int32), np.array([0.3, 0.3, 0.3, 0.1])),
            (np.array([4, 5], np.int32), np.array([0.5, 0.5]))]
    inv = {}
    for k, (w, _) in enumerate(bows):
        for x in w:
            inv.setdefault(int(x), []).append(k)
    return dict(inv=inv, bows=bows, covis=[[3], [], [], [0, 1], []], map_id=np.array([0, 0, 1, 0, 0], np.int32))


def test_hand_computed_case():
    db = _db()
    qw, qv = np.array([0, 1, 2], np.int32), np.array([1 / 3, 1 / 3, 1 / 3])
    score = np.zeros(5, np.float32)
    score[1] = 0.5                                   # what an earlier query left on KF1
    got = rm.detect_relocalization_candidates(db, qw, qv, 0, score)
    s0, s2, s3 = np.float32(1.0), np.float32(0.75), np.float32(0.9)
    assert np.allclose(score[[0, 2, 3]], [s0, s2, s3], atol=1e-6) and score[1] == 0.5 and score[4] == 0
    # acc: KF0 = 1 + 0.9 (best KF0); KF2 = 0.75 alone, another map -- it is scored and could have set bestAccScore, then is filtered;
    # KF3 = 0.9 + 1 + 0.5 (KF1 shares a word without reaching the threshold: its OLD score counts), best KF0.
    # bestAccScore = 2.4, keep > 1.8: KF0's 1.9 and KF3's 2.4 stay, both name KF0: one candidate.
    assert got == [0]
    # seen from map 1 only KF2 could be returned, and its 0.75 is below 0.75 * 2.4
    assert rm.detect_relocalization_candidates(db, qw, qv, 1, score.copy()) == []
    # a query that shares no word
    assert rm.detect_relocalization_candidates(db, np.array([3], np.int32), np.array([1.0]), 0, score) == []


def test_no_sort_first_encounter_order_decides():
    """Two groups whose representatives both pass the 0.75 bound come back in lKFsSharingWords order, not by score."""
    bows = [(np.array([0, 1], np.int32), np.array([0.4, 0.6])), (np.array([0, 1], np.int32), np.array([0.5, 0.5]))]
    db = dict(inv={0: [0, 1], 1: [0, 1]}, bows=bows, covis=[[], []], map_id=np.zeros(2, np.int32))
    score = np.zeros(2, np.float32)
    got = rm.detect_relocalization_candidates(db, np.array([0, 1], np.int32), np.array([0.5, 0.5]), 0, score)
    assert score[1] > score[0] and got == [0, 1]


def test_entry_point_argument_checks_and_symbol():
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    assert re.search(r"^int\s+orbd_detect_relocalization_candidates\s*\(", hdr, flags=re.M)
    assert "orbd_detect_relocalization_candidates" in capi.EXPORTED_SYMBOLS and hasattr(lib, "orbd_detect_relocalization_candidates")
    n = C.c_int32(0)
    assert lib.orbd_detect_relocalization_candidates(None, None, None, 0, 0, None, None, C.byref(n)) == capi.ORBG_BAD_ARG
