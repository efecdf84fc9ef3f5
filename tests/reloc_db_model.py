"""Checker for KeyFrameDatabase::DetectRelocalizationCandidates (S/KeyFrameDatabase.cc:764-876): a pure-Python restatement on index
arrays with the reference's per-keyframe state (mnRelocQuery as `queried`, mnRelocWords, mRelocScore = reloc_score, which persists from
query to query).  Lists instead of std::list; float32 where the reference has float."""
import numpy as np


def l1_score(qw, qv, w, v):
    """DBoW2::L1Scoring::score: the common words in ascending order, double."""
    a = dict(zip(np.asarray(qw).tolist(), np.asarray(qv).tolist()))
    s = 0.0
    for x, y in zip(np.asarray(w).tolist(), np.asarray(v).tolist()):
        if x in a:
            s += abs(a[x] - y) - abs(a[x]) - abs(y)
    return -s / 2.0


def detect_relocalization_candidates(db, qw, qv, query_map_id, reloc_score):
    """db: dict(inv={word: [kf, ...]}, bows=[(words, values)], covis=[[kf, ...]], map_id).  reloc_score: float32[K], updated in place.
    -> list of keyframe indices (vpRelocCandidates)."""
    K = len(db["bows"])
    queried, words, order = [False] * K, [0] * K, []
    for w in np.asarray(qw).tolist():
        for kf in db["inv"].get(int(w), []):
            if not queried[kf]:                      # no connected-keyframe exclusion, no map filter, no isBad()
                words[kf] = 0
                queried[kf] = True
                order.append(kf)
            words[kf] += 1
    if not order:
        return []
    mx = max(words[k] for k in order)
    mn = int(np.float32(mx) * np.float32(0.8))
    scored = []
    for kf in order:
        if words[kf] > mn:
            si = np.float32(l1_score(qw, qv, *db["bows"][kf]))
            reloc_score[kf] = si
            scored.append((si, kf))
    if not scored:
        return []
    acc, best_acc = [], np.float32(0)
    for si, kf in scored:
        best, bs, a = kf, si, np.float32(si)
        for k2 in list(db["covis"][kf])[:10]:
            if not queried[k2]:
                continue
            a = np.float32(a + reloc_score[k2])      # what an EARLIER query left, if k2 did not reach the word threshold in this one
            if reloc_score[k2] > bs:
                best, bs = k2, reloc_score[k2]
        acc.append((a, best))
        if a > best_acc:
            best_acc = a
    keep = np.float32(0.75) * best_acc
    out, added = [], set()
    for a, kf in acc:                                # lKFsSharingWords order: no sort here
        if a > keep:
            if db["map_id"][kf] != query_map_id:
                continue
            if kf not in added:
                out.append(kf)
                added.add(kf)
    return out
