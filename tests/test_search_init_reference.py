"""ORBmatcher::SearchForInitialization and Frame::GetFeaturesInArea EXECUTED FROM THE REFERENCE'S OWN SOURCE TEXT and held against
tests/search_init_model.py (CPU only; runs where the reference is present -- the GPU box has none).  As in
tests/test_reference_formulas.py the two bodies are cut out of S/ORBmatcher.cc and S/Frame.cc where they lie and translated statement
by statement into Python (braces -> indentation, declarations -> assignments with the declared type's rounding, a literal with an
`f` -> float32, with a decimal point -> double, `?:` -> conditional expressions, `for` -> range) over stand-in Frames whose members are
numpy float32 scalars, so that C's promotion rules hold.  Nothing of the reference is copied into the repository: the text is read,
translated, executed and compared.  ComputeThreeMaxima (S/ORBmatcher.cc:2312-2353, outside the two bodies) is the model's."""
import os
import re

import numpy as np
import pytest

import search_init_model as sm

REF = "/root/reference/src/orb_slam3_ros/orb_slam3"
SRC_M, SRC_F = os.path.join(REF, "src", "ORBmatcher.cc"), os.path.join(REF, "src", "Frame.cc")
pytestmark = pytest.mark.skipif(not (os.path.isfile(SRC_M) and os.path.isfile(SRC_F)), reason="the reference is only present in the build container")

F32, F64 = np.float32, np.float64


def _body(path, signature_regex):
    text = open(path).read()
    m = re.search(signature_regex, text)
    assert m, signature_regex
    i = text.index("{", m.end() - 1)
    j = _match(text, i, "{", "}")
    body = re.sub(r"/\*.*?\*/", " ", text[i + 1:j], flags=re.S)
    return re.sub(r"//[^\n]*", " ", body)


def _match(s, i, a, b):
    depth = 0
    for j in range(i, len(s)):
        depth += s[j] == a
        depth -= s[j] == b
        if depth == 0:
            return j
    raise AssertionError("unbalanced")


# ---- C statements -> a tree

def _parse(s):
    """-> list of ('for', head, body) | ('if', cond, then, else | None) | ('block', [..]) | ('stmt', text)"""
    out, i = [], 0
    while True:
        while i < len(s) and s[i].isspace():
            i += 1
        if i >= len(s):
            return out
        node, i = _parse_one(s, i)
        out.append(node)


def _parse_one(s, i):
    while s[i].isspace():
        i += 1
    if s[i] == "{":
        j = _match(s, i, "{", "}")
        return ("block", _parse(s[i + 1:j])), j + 1
    m = re.match(r"(for|if)\s*\(", s[i:])
    if m:
        p = i + m.end() - 1
        q = _match(s, p, "(", ")")
        body, k = _parse_one(s, q + 1)
        if m.group(1) == "for":
            return ("for", s[p + 1:q], body), k
        k2 = k
        while k2 < len(s) and s[k2].isspace():
            k2 += 1
        if s[k2:k2 + 4] == "else" and not (s[k2 + 4].isalnum() or s[k2 + 4] == "_"):
            els, k3 = _parse_one(s, k2 + 4)
            return ("if", s[p + 1:q], body, els), k3
        return ("if", s[p + 1:q], body, None), k
    j = s.index(";", i)
    return ("stmt", " ".join(s[i:j].split())), j + 1


# ---- expressions

def _ternary(e):
    """a ? b : c (right-associative, top level of e) -> (b if a else c)"""
    depth = 0
    for i, ch in enumerate(e):
        depth += ch in "([{"
        depth -= ch in ")]}"
        if ch == "?" and depth == 0:
            d2, nest = 0, 0
            for j in range(i + 1, len(e)):
                d2 += e[j] in "([{"
                d2 -= e[j] in ")]}"
                if d2 == 0 and e[j] == "?":
                    nest += 1
                if d2 == 0 and e[j] == ":" and e[j - 1] != ":" and e[j + 1:j + 2] != ":":
                    if nest == 0:
                        return "((%s) if (%s) else (%s))" % (_ternary(e[i + 1:j]), e[:i], _ternary(e[j + 1:]))
                    nest -= 1
            raise AssertionError(e)
    return e


def _expr(e):
    e = e.replace("cv::", "")
    e = re.sub(r"vector<\w+>\(([^,]+),([^)]+)\)", r"Vec([\2] * int(\1))", e)
    e = re.sub(r"\(int\)", "", e)
    e = re.sub(r"\(float\)\s*(\w+)", r"F32(\1)", e)
    e = re.sub(r"(?<![\w.])(\d+\.\d*|\.\d+)f(?![\w.])", r"F32(\1)", e)
    e = re.sub(r"(?<![\w.(])(\d+\.\d*|\.\d+)(?![\w.)])", r"F64(\1)", e)
    e = e.replace("&&", " and ").replace("||", " or ")
    e = re.sub(r"!(?!=)", " not ", e)
    e = re.sub(r"\*vit\b", "vit", e)
    e = e.replace("fabs(", "abs(")
    return _ternary(e)


DECL = r"(?:const\s+)?(?:vector<\w+>|float|int|bool|size_t|KeyPoint|Mat)\s*&?\s*"


def _stmt(st):
    st = st.replace("cv::", "")
    if st in ("continue", "break"):
        return st
    if st.startswith("return"):
        return "return " + _expr(st[6:].strip())
    if re.match(r"\w+\.reserve\(", st) or re.match(r"rotHist\[i\]\.reserve", st):
        return "pass"
    m = re.match(r"assert\((.+)\)$", st)
    if m:
        return "assert " + _expr(m.group(1))
    m = re.match(r"ComputeThreeMaxima\(rotHist,HISTO_LENGTH,ind1,ind2,ind3\)$", st.replace(" ", ""))
    if m:
        return "ind1, ind2, ind3 = ComputeThreeMaxima(rotHist, HISTO_LENGTH)"
    m = re.match(r"(\w+)(\+\+|--)$", st)
    if m:
        return "%s %s= 1" % (m.group(1), m.group(2)[0])
    m = re.match(r"vector<\w+>\s+(\w+)\[(\w+)\]$", st)
    if m:
        return "%s = [Vec() for _ in range(%s)]" % (m.group(1), m.group(2))
    m = re.match(r"vector<\w+>\s+(\w+)$", st)
    if m:
        return "%s = Vec()" % m.group(1)
    m = re.match(r"vector<\w+>\s+(\w+)\((.+),(.+)\)$", st)
    if m:
        return "%s = Vec([%s] * int(%s))" % (m.group(1), _expr(m.group(3)), _expr(m.group(2)))
    m = re.match(r"(?:const\s+)?(float|int|size_t)\s+(\w+)\s*=\s*(.+)$", st)
    if m:
        return "%s = %s(%s)" % (m.group(2), "F32" if m.group(1) == "float" else "int", _expr(m.group(3)))
    m = re.match(DECL + r"(\w+)\s*=\s*(.+)$", st)
    if m:
        return "%s = %s" % (m.group(1), _expr(m.group(2)))
    m = re.match(r"(\w+)\s*\+=\s*(.+)$", st)
    if m:
        return "%s = F32(%s + %s)" % (m.group(1), m.group(1), _expr(m.group(2)))
    m = re.match(r"([\w\[\]\.]+)\s*=\s*(.+)$", st)
    if m:
        return "%s = %s" % (_expr(m.group(1)), _expr(m.group(2)))
    return _expr(st)                                        # a call: v.push_back(..)


def _for(head):
    h = head.replace("cv::", "")
    m = re.match(r"vector<size_t>::iterator\s+vit\s*=\s*(\w+)\.begin\(\)\s*;\s*vit\s*!=\s*\1\.end\(\)\s*;\s*vit\+\+$", h.strip())
    if m:
        return "for vit in list(%s):" % m.group(1)
    init, cond, inc = [p.strip() for p in h.split(";")]
    m = re.match(r"(?:int|size_t)\s+(\w+)\s*=\s*([^,]+?)(?:\s*,\s*(\w+)\s*=\s*(.+))?$", init)
    assert m and inc == m.group(1) + "++", head
    var, lo = m.group(1), _expr(m.group(2))
    c = re.match(r"%s\s*(<=|<)\s*(.+)$" % var, cond)
    assert c, head
    hi = c.group(2).strip()
    if m.group(3) and hi == m.group(3):
        hi = m.group(4)
    hi = _expr(hi)
    return "for %s in range(int(%s), int(%s)%s):" % (var, lo, hi, " + 1" if c.group(1) == "<=" else "")


def _emit(nodes, ind, out):
    for n in nodes:
        pad = "    " * ind
        if n[0] == "stmt":
            if n[1]:
                out.append(pad + _stmt(n[1]))
        elif n[0] == "block":
            _emit(n[1], ind, out)
        elif n[0] == "for":
            out.append(pad + _for(n[1]))
            _emit([n[2]], ind + 1, out)
        else:
            out.append(pad + "if %s:" % _expr(" ".join(n[1].split())))
            _emit([n[2]], ind + 1, out)
            if n[3] is not None:
                out.append(pad + "else:")
                _emit([n[3]], ind + 1, out)


def _function(name, args, body):
    out = ["def %s(%s):" % (name, ", ".join(args))]
    _emit(_parse(body), 1, out)
    return "\n".join(out)


# ---- stand-ins

class Vec(list):
    def push_back(self, v):
        self.append(v)

    def size(self):
        return len(self)

    def empty(self):
        return len(self) == 0


class Pt:
    def __init__(self, x, y):
        self.x, self.y = F32(x), F32(y)


class KeyPoint:
    def __init__(self, k):
        self.pt, self.octave, self.angle = Pt(k["x"], k["y"]), int(k["octave"]), F32(k["angle"])


class Desc:
    def __init__(self, d):
        self.d = d

    def row(self, i):
        return self.d[int(i)]


def _sat(v):
    v = float(v)
    return -2 ** 31 if not v > -2.0 ** 31 else (2 ** 31 - 1 if not v < 2.0 ** 31 else int(v))


ENV = {"F32": F32, "F64": F64, "Vec": Vec, "INT_MAX": sm.INT_MAX, "HISTO_LENGTH": 30, "TH_LOW": 50, "FRAME_GRID_COLS": 64, "FRAME_GRID_ROWS": 48,
       "floor": lambda v: _sat(np.floor(v)), "ceil": lambda v: _sat(np.ceil(v)), "round": sm.round_away, "abs": abs, "max": max, "min": min,
       "ComputeThreeMaxima": lambda hist, L: sm.three_maxima([len(h) for h in hist]),
       "DescriptorDistance": lambda a, b: int(sm.POP[np.bitwise_xor(a, b)].sum())}


class RefFrame:
    """The members the two bodies touch, from a model Frame; GetFeaturesInArea is the reference's text."""

    def __init__(self, F, area_code):
        self.mvKeysUn = Vec(KeyPoint(k) for k in F.kps)
        self.mvKeys, self.mvKeysRight = self.mvKeysUn, Vec()
        self.mDescriptors = Desc(F.desc)
        self.N, self.Nleft = F.n, -1
        self.mGrid = [[Vec(F.grid[ix * sm.ROWS + iy]) for iy in range(sm.ROWS)] for ix in range(sm.COLS)]
        self.mGridRight = self.mGrid
        self.mnMinX, self.mnMinY = F.min_x, F.min_y
        self.mfGridElementWidthInv, self.mfGridElementHeightInv = F.w_inv, F.h_inv
        self._area = area_code

    def GetFeaturesInArea(self, x, y, r, minLevel, maxLevel, bRight=False):
        env = dict(ENV, **{k: getattr(self, k) for k in ("mvKeysUn", "mvKeys", "mvKeysRight", "N", "Nleft", "mGrid", "mGridRight", "mnMinX", "mnMinY",
                                                          "mfGridElementWidthInv", "mfGridElementHeightInv")})
        exec(self._area, env)
        with np.errstate(all="ignore"):
            return env["GetFeaturesInArea"](F32(x), F32(y), F32(r), int(minLevel), int(maxLevel), bRight)


@pytest.fixture(scope="module")
def code():
    area = _function("GetFeaturesInArea", ["x", "y", "r", "minLevel", "maxLevel", "bRight"],
                     _body(SRC_F, r"vector<size_t>\s+Frame::GetFeaturesInArea\s*\("))
    search = _function("SearchForInitialization", ["F1", "F2", "vbPrevMatched", "windowSize", "mfNNratio", "mbCheckOrientation"],
                       _body(SRC_M, r"int\s+ORBmatcher::SearchForInitialization\s*\(").replace("return nmatches;", "return nmatches, vnMatches12;"))
    # what the translation must have kept: the skip before the bookkeeping, the strict window, the float product
    flat = search.replace(" ", "")
    assert flat.index("ifvMatchedDistance[i2]<=dist:") < flat.index("ifdist<bestDist:") < flat.index("ifdist<bestDist2:")
    assert "abs(distx)<factorX" in area.replace(" ", "") and "ifbestDist<F32(bestDist2)*mfNNratio:" in flat
    return area, search


def run_text(code, F1, F2, prev, window, nn_ratio=0.9, check=True):
    area, search = code
    R1, R2 = RefFrame(F1, area), RefFrame(F2, area)
    pm = Vec(Pt(p[0], p[1]) for p in np.asarray(prev, F32).reshape(-1, 2))
    env = dict(ENV)
    exec(search, env)
    with np.errstate(all="ignore"):
        n, m12 = env["SearchForInitialization"](R1, R2, pm, int(window), F32(nn_ratio), bool(check))
    return int(n), np.array(list(m12), np.int32), np.array([[p.x, p.y] for p in pm], F32).reshape(-1, 2)


@pytest.mark.parametrize("name", ["small", "ties", "ties_loose", "edges", "levels_f1", "levels_f2", "window10", "no_orientation"])
def test_reference_text_gives_the_models_result(code, name):
    c = sm.cases()[name] if name != "small" else sm.case_small()
    want = sm.run_case(c)
    n, m12, prev = run_text(code, c["F1"], c["F2"], c["prev"], c["window"], c.get("nn_ratio", 0.9), c.get("check_orientation", True))
    assert n == want["nmatches"] and np.array_equal(m12, want["matches12"])
    assert prev.tobytes() == np.ascontiguousarray(want["prev"], F32).tobytes()


def test_reference_text_of_get_features_in_area_gives_the_models_lists(code):
    c = sm.case_edges()
    F2 = RefFrame(c["F2"], code[0])
    for x, y in list(c["prev"]) + [(c["F2"].kps["x"][i], c["F2"].kps["y"][i]) for i in range(0, 400, 37)]:
        for r in (100, 10, 33):
            assert list(F2.GetFeaturesInArea(x, y, r, 0, 0)) == sm.features_in_area(c["F2"], x, y, r), (x, y, r)
