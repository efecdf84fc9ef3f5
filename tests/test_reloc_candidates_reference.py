"""KeyFrameDatabase::DetectRelocalizationCandidates (S/KeyFrameDatabase.cc:764-876) WHOLE, executed from the reference's own text over
stand-ins for KeyFrame / Frame / Map the way tests/test_reference_formulas.py executes DetectNBestCandidates, against
tests/reloc_db_model.py: a seeded 60-keyframe database with two maps, ten consecutive queries that share the mRelocScore state; lists
equal, scores bit-equal.  CPU only; runs where the reference is present.  Nothing of the reference is copied: the text is read,
translated statement by statement and executed."""
import os
import re

import numpy as np
import pytest

import reloc_db_model as rm
from test_reference_formulas import ENV, REF, CppMap, _body, c_to_python, cpp_prepare

pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "src", "KeyFrameDatabase.cc")), reason="the reference is only present in the build container")

F32, F64 = np.float32, np.float64


def test_detectrelocalizationcandidates_is_the_references_text():
    import helpers
    body = _body(os.path.join(REF, "src", "KeyFrameDatabase.cc"), r"vector<KeyFrame\*>\s+KeyFrameDatabase::DetectRelocalizationCandidates\s*\([^)]*\)\s*\{")
    rep = [("list<KeyFrame*> lKFsSharingWords;", "lKFsSharingWords = [];"), ("unique_lock<mutex> lock(mMutex);", ""),
           ("for(DBoW2::BowVector::const_iterator vit=F->mBowVec.begin(), vend=F->mBowVec.end(); vit != vend; vit++)", "bowitems = F->mBowVec.items(); foreach(vit, bowitems)"),
           ("for(list<KeyFrame*>::iterator lit=lKFs.begin(), lend= lKFs.end(); lit!=lend; lit++) { KeyFrame* pKFi=*lit;", "foreach(pKFi, lKFs) {"),
           ("list<pair<float,KeyFrame*> > lScoreAndMatch;", "lScoreAndMatch = [];"), ("list<pair<float,KeyFrame*> > lAccScoreAndMatch;", "lAccScoreAndMatch = [];"),
           ("for(vector<KeyFrame*>::iterator vit=vpNeighs.begin(), vend=vpNeighs.end(); vit!=vend; vit++) { KeyFrame* pKF2 = *vit;", "foreach(pKF2, vpNeighs) {"),
           ("set<KeyFrame*> spAlreadyAddedKF;", "spAlreadyAddedKF = CppSet();"), ("vector<KeyFrame*> vpRelocCandidates;", "vpRelocCandidates = [];"),
           ("const float &si = it->first;", "float si = it->first;"), ("make_pair(", "Pair(")]
    body = re.sub(r"\s+", " ", body)
    body = re.sub(r"[\w\.]+\.reserve\([^;]*\);", "", body)
    for a, b in rep:
        assert a in body, a
        body = body.replace(a, b)
    loops = "for(list<pair<float,KeyFrame*> >::iterator it=lScoreAndMatch.begin(), itend=lScoreAndMatch.end(); it!=itend; it++)"
    assert body.count(loops) == 1
    body = body.replace(loops, "foreach(it, lScoreAndMatch)")
    loopa = "for(list<pair<float,KeyFrame*> >::iterator it=lAccScoreAndMatch.begin(), itend=lAccScoreAndMatch.end(); it!=itend; it++)"
    assert body.count(loopa) == 1
    body = body.replace(loopa, "foreach(it, lAccScoreAndMatch)")
    lw = "for(list<KeyFrame*>::iterator lit=lKFsSharingWords.begin(), lend= lKFsSharingWords.end(); lit!=lend; lit++)"
    assert body.count(lw) == 2
    body = body.replace(lw + " { if((*lit)->mnRelocWords>maxCommonWords) maxCommonWords=(*lit)->mnRelocWords; }",
                        "foreach(litv, lKFsSharingWords) { if(litv->mnRelocWords>maxCommonWords) maxCommonWords=litv->mnRelocWords; }")
    body = body.replace(lw + " { KeyFrame* pKFi = *lit;", "foreach(pKFi, lKFsSharingWords) {")
    assert "::iterator" not in body and "*lit" not in body
    # the returns: an empty vector early, the candidates at the end
    assert body.count("return vector<KeyFrame*>();") == 2
    body = body.replace("return vector<KeyFrame*>();", "return [];")
    body = body.replace(".push_back(", ".append(")
    # the mutex's bare block
    body = re.sub(r"\s+", " ", body)
    assert "{ bowitems = F->mBowVec.items();" in body
    body = body.replace("{ bowitems = F->mBowVec.items();", "if(True) { bowitems = F->mBowVec.items();")
    src = c_to_python(cpp_prepare(body), typed_ints=True, keep_returns=True)
    assert "minCommonWords = as_int(maxCommonWords*F32(0.8))" in src and "sort" not in src
    assert "F32(0.75)*bestAccScore" in src.replace(" ", "")
    sc_body = _body(os.path.join(REF, "Thirdparty", "DBoW2", "DBoW2", "ScoringObject.cpp"), r"double\s+L1Scoring::score\s*\([^)]*\)\s*const\s*\{")
    sc_body = sc_body.replace("BowVector::const_iterator v1_it, v2_it;", "").replace("const WordValue& vi", "double vi").replace("const WordValue& wi", "double wi")
    sc_body = sc_body.replace("++v1_it;", "v1_it++;").replace("++v2_it;", "v2_it++;").replace("fabs(", "abs(")
    ind = lambda text: "\n".join("    " + ln for ln in text.splitlines())      # noqa: E731
    prog = ("def l1score(v1, v2):\n" + ind(c_to_python(cpp_prepare(sc_body), keep_returns=True)) +
            "\ndef DetectRelocalizationCandidates(mvInvertedFile, mpVoc, F, pMap):\n" + ind(src))

    class Pair:
        def __init__(self, a, b): self.first, self.second = a, b

    class CppSet:
        def __init__(self, it=()): self.s = set(id(x) for x in it)
        def count(self, x): return 1 if id(x) in self.s else 0
        def insert(self, x): self.s.add(id(x))

    class BowMap(CppMap):
        def __init__(self, words, values): self.keys = [int(w) for w in words]; self.vals = [F64(v) for v in values]
        def items(self): return [Pair(k, v) for k, v in zip(self.keys, self.vals)]

    class Obj:
        pass

    rng = np.random.RandomState(202)
    db = helpers.random_database(rng, n_kfs=60, n_words=900, words_per_kf=(40, 120), n_maps=2, bad_frac=0.0)
    K = len(db["bows"])
    maps = {int(m): Obj() for m in np.unique(db["map_id"])}
    assert len(maps) == 2
    kfs = []
    for k in range(K):
        f = Obj(); f.idx = k; f.mnRelocQuery = -1; f.mnRelocWords = 0; f.mRelocScore = F32(0)
        f.mBowVec = BowMap(*db["bows"][k]); f.map = maps[int(db["map_id"][k])]
        f.GetMap = (lambda f=f: f.map)
        kfs.append(f)
    for k in range(K):
        kfs[k].GetBestCovisibilityKeyFrames = (lambda n, k=k: [kfs[j] for j in db["covis"][k]][:n])
    inverted = [[kfs[j] for j in db["inv"].get(w, [])] for w in range(db["n_words"])]
    env = dict(ENV, F32=F32, F64=F64, abs=abs, as_int=lambda x: int(x), Pair=Pair, CppSet=CppSet)
    exec(prog, env)
    voc = type("Voc", (), {"score": staticmethod(lambda a, b: env["l1score"](a, b))})()
    score_m = np.zeros(K, np.float32)
    hits = other_map = 0
    for qn in range(10):
        kq = int(rng.randint(K))
        qw, qv = db["bows"][kq]
        if qn % 2:                                               # a frame between two keyframes: a mix of their words
            w2, _ = db["bows"][(kq + 1) % K]
            qw = np.union1d(qw[::2], w2[::2]).astype(np.int32)
            qv = rng.rand(len(qw)) + 0.05
            qv /= qv.sum()
        qmap = int(db["map_id"][kq]) if qn % 4 else 1 - int(db["map_id"][kq])
        want = rm.detect_relocalization_candidates(db, qw, qv, qmap, score_m)
        q = Obj(); q.mnId = 50000 + qn; q.mBowVec = BowMap(qw, qv)
        got = env["DetectRelocalizationCandidates"](inverted, voc, q, maps[qmap])
        assert [f.idx for f in got] == want, (qn, [f.idx for f in got], want)
        mine = np.array([f.mRelocScore for f in kfs], np.float32)
        assert np.array_equal(mine.view(np.uint32), score_m.view(np.uint32)), qn
        hits += len(want)
        other_map += int(qn % 4 == 0)
    assert hits >= 5 and other_map >= 2
