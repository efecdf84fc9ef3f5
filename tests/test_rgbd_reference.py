"""Frame::ComputeStereoFromRGBD, the convertTo condition of Tracking::GrabImageRGBD and the inversion of mDepthMapFactor EXECUTED FROM THE
REFERENCE'S OWN SOURCE TEXT and held against tests/rgbd_model.py (CPU only; runs where the reference is present -- the GPU box has
none).  As in tests/test_reference_formulas.py the bodies are cut out of S/Frame.cc and S/Tracking.cc where they lie and translated
statement by statement into Python (braces -> indentation, declarations -> assignments with the declared type's rounding, a literal
with an `f` -> float32, `for` -> range) over stand-in objects whose members are numpy float32 values, so that C's promotion rules hold.
Nothing of the reference is copied into the repository: the text is read, translated, executed and compared.  cv::Mat::convertTo itself
is OpenCV's, not the reference's: the stand-in's is the pinned arithmetic of the model (one float32 product per pixel)."""
import os
import re

import numpy as np
import pytest

import rgbd_model as rm

REF = "/root/reference/src/orb_slam3_ros/orb_slam3"
SRC_F, SRC_T = os.path.join(REF, "src", "Frame.cc"), os.path.join(REF, "src", "Tracking.cc")
pytestmark = pytest.mark.skipif(not (os.path.isfile(SRC_F) and os.path.isfile(SRC_T)), reason="the reference is only present in the build container")

F32 = np.float32
CV_32F, CV_16U = 5, 2


def _match(s, i, a, b):
    depth = 0
    for j in range(i, len(s)):
        depth += s[j] == a
        depth -= s[j] == b
        if depth == 0:
            return j
    raise AssertionError("unbalanced")


def _body(path, signature_regex):
    text = open(path).read()
    m = re.search(signature_regex, text)
    assert m, signature_regex
    i = text.index("{", m.end() - 1)
    j = _match(text, i, "{", "}")
    body = re.sub(r"/\*.*?\*/", " ", text[i + 1:j], flags=re.S)
    return re.sub(r"//[^\n]*", " ", body)


MEMBERS = ("mvuRight", "mvDepth", "mvKeysUn", "mvKeys", "mbf", "mDepthMapFactor", "N")


def _expr(e):
    e = e.replace("cv::", "")
    e = re.sub(r"vector<float>\(([^,]+),([^)]+)\)", r"np.full(\1, \2, F32)", e)
    e = re.sub(r"(\w+)\.at<float>\(", r"\1.at_float(", e)
    e = re.sub(r"(?<![\w.])(\d+\.\d*|\.\d+)f(?![\w.])", r"F32(\1)", e)
    e = e.replace("&&", " and ").replace("||", " or ").replace("fabs(", "abs(")
    for mname in MEMBERS:
        e = re.sub(r"(?<![\w.])%s\b" % mname, "self." + mname, e)
    return e.strip()


def _translate(body, ind="    "):
    """The statement forms these bodies use: for (int i = a; i < b; i++), if / else, declarations, assignments."""
    out, depth, pending = [], 1, 0
    toks = re.findall(r"for\s*\([^)]*\)|if\s*\((?:[^()]|\([^()]*\))*\)|else\b|\{|\}|[^;{}\s][^;{}]*;", body)
    assert "".join(toks).replace(" ", "").replace("\n", "") == re.sub(r"\s", "", body), "untranslated text"
    for t in toks:
        t = t.strip()
        if t == "{":
            pending = 0
            continue
        if t == "}":
            depth -= 1
            continue
        line = None
        m = re.match(r"for\s*\(\s*int\s+(\w+)\s*=\s*([^;]+);\s*\1\s*<\s*([^;]+);\s*\1\+\+\s*\)$", t)
        if m:
            line = "for %s in range(%s, %s):" % (m.group(1), _expr(m.group(2)), _expr(m.group(3)))
        elif t.startswith("if"):
            line = "if %s:" % _expr(t[t.index("(") + 1:t.rindex(")")])
        elif t == "else":
            line = "else:"
        if line is not None:
            out.append(ind * depth + line)
            depth += 1
            pending += 1
            continue
        st = t[:-1].strip()
        m = re.match(r"(?:const\s+)?(cv::KeyPoint|float|int)\s*&?\s*(\w+)\s*=\s*(.+)$", st)
        if m:
            rhs = _expr(m.group(3))
            st = "%s = %s" % (m.group(2), {"float": "F32(%s)", "int": "int(%s)"}.get(m.group(1), "%s") % rhs)
        else:
            st = _expr(st)
        out.append(ind * depth + st)
        # a statement without braces ends the constructs it hangs from
        depth -= pending
        pending = 0
    return out


class _Pt:
    def __init__(self, x, y):
        self.x, self.y = F32(x), F32(y)


class _Kp:
    def __init__(self, x, y):
        self.pt = _Pt(x, y)


class _Mat:
    """cv::Mat of CV_32F: at<float>(int row, int col) -- float arguments convert as C converts them (towards zero)."""
    def __init__(self, a):
        self.a = a
        self.reads = []

    def at_float(self, row, col):
        r, c = int(row), int(col)
        assert 0 <= r < self.a.shape[0] and 0 <= c < self.a.shape[1], "the reference reads outside the image here"
        self.reads.append((r, c))
        return self.a[r, c]


class _Frame:
    pass


@pytest.fixture(scope="module")
def compute_stereo_from_rgbd():
    body = _body(SRC_F, r"void\s+Frame::ComputeStereoFromRGBD\s*\(\s*const\s+cv::Mat\s*&\s*imDepth\s*\)")
    code = "def ComputeStereoFromRGBD(self, imDepth):\n" + "\n".join(_translate(body))
    ns = dict(np=np, F32=F32)
    exec(code, ns)
    return ns["ComputeStereoFromRGBD"], code


def _grab_body():
    return _body(SRC_T, r"cv::Mat\s+Tracking::GrabImageRGBD\s*\(")


def test_translation_covers_the_whole_body(compute_stereo_from_rgbd):
    fn, code = compute_stereo_from_rgbd
    for needle in ("for i in range(0, self.N):", "at_float(v,u)", "if d>0:", "self.mvDepth[i] = d", "kpU.pt.x-self.mbf/d", "np.full(self.N, -1, F32)"):
        assert needle in code.replace(", ", ", "), (needle, code)


def _run(fn, xy, x_un, img32, bf):
    F = _Frame()
    F.N = len(xy)
    F.mvKeys = [_Kp(x, y) for x, y in xy]
    F.mvKeysUn = [_Kp(x, 0) for x in x_un]
    F.mbf = F32(bf)
    mat = _Mat(img32)
    with np.errstate(over="ignore", divide="ignore"):
        fn(F, mat)
    return F.mvuRight, F.mvDepth, mat


@pytest.mark.parametrize("kind", ["u16", "f32", "f32_factor"])
def test_reference_text_gives_the_models_result(compute_stereo_from_rgbd, kind):
    """GrabImageRGBD's condition decides whether the image is converted (the stand-in's convertTo: the pinned product), then the
    reference's ComputeStereoFromRGBD runs on the converted image; the model converts only the values it reads."""
    fn, _ = compute_stereo_from_rgbd
    rng = np.random.RandomState(4)
    h, w = 23, 31
    if kind == "u16":
        raw = rng.randint(0, 65536, (h, w)).astype(np.uint16)
        raw[rng.rand(h, w) < 0.2] = 0
        factor = rm.depth_map_factor(5000.0)
    else:
        raw = rng.uniform(-1.0, 8.0, (h, w)).astype(F32)
        raw[rng.rand(h, w) < 0.1] = np.nan
        raw[rng.rand(h, w) < 0.05] = np.inf
        raw[rng.rand(h, w) < 0.05] = 0.0
        factor = F32(1.0) if kind == "f32" else F32(0.37)
    xy = rng.uniform([0, 0], [w - 0.001, h - 0.001], (500, 2)).astype(F32)
    xy[:4] = [[w - 1 + 0.999, h - 1 + 0.999], [0.999, 0.999], [0, 0], [3.5, 7.25]]
    xy = np.minimum(xy, np.array([np.nextafter(F32(w), F32(0)), np.nextafter(F32(h), F32(0))], F32))
    x_un = (xy[:, 0] + rng.uniform(-3, 3, len(xy))).astype(F32)
    cond = _convert_condition()
    img = rm.convert_to_f32(raw, factor) if cond(F32(factor), CV_16U if kind == "u16" else CV_32F) else raw
    assert img.dtype == np.float32 and (kind == "f32") == (img is raw)
    ur, dp, mat = _run(fn, xy, x_un, img, 40.0)
    m_ur, m_dp = rm.depth_at_points(xy, x_un, raw, factor, 40.0)
    assert np.asarray(dp, F32).tobytes() == m_dp.tobytes() and np.asarray(ur, F32).tobytes() == m_ur.tobytes()
    assert (m_dp > 0).sum() > 100 and (m_dp == -1).sum() > 30
    # the pixel read is the truncated DISTORTED coordinate, row first
    assert mat.reads == [(int(y), int(x)) for x, y in xy]


def _convert_condition():
    """-> f(mDepthMapFactor, imDepth.type()) from the text of S/Tracking.cc:1107-1108"""
    body = _grab_body()
    m = re.search(r"if\s*\(((?:[^()]|\((?:[^()]|\([^()]*\))*\))*)\)\s*imDepth\.convertTo\(\s*imDepth\s*,\s*CV_32F\s*,\s*mDepthMapFactor\s*\)\s*;", body)
    assert m, "GrabImageRGBD no longer converts the depth image as the model pins it"
    e = _expr(m.group(1)).replace("self.mDepthMapFactor", "mDepthMapFactor").replace("imDepth.type()", "imDepth_type")
    return eval("lambda mDepthMapFactor, imDepth_type: bool(%s)" % e, dict(F32=F32, CV_32F=CV_32F, abs=abs))


def test_convert_condition_text_is_the_models():
    cond = _convert_condition()
    for f in (1.0, 1.000009, 1.00001, 1.00002, 0.99998, 0.999991, 0.0002, 5000.0, 0.0, -1.0, 1.0 + 2e-5, 1.0 - 2e-5):
        for typ, dt in ((CV_32F, np.float32), (CV_16U, np.uint16)):
            assert cond(F32(f), typ) == rm.needs_convert(dt, f), (f, typ)


def test_depth_map_factor_text_is_the_models():
    text = re.sub(r"//[^\n]*", " ", open(SRC_T).read())
    m = re.search(r"if\s*\(\s*sensor\s*==\s*RGBD\s*\)\s*\{\s*if\s*\(([^{};]*)\)\s*mDepthMapFactor\s*=\s*([^;]+);\s*else\s+mDepthMapFactor\s*=\s*([^;]+);", text)
    assert m, "the inversion of mDepthMapFactor is not where the model expects it"
    cond, a, b = [_expr(g).replace("self.mDepthMapFactor", "f") for g in m.groups()]
    fn = eval("lambda f: F32(%s) if (%s) else F32(%s)" % (a, cond, b), dict(F32=F32, abs=abs))
    for y in (5000.0, 1.0, 0.0, 1e-6, 9.9e-6, 1.1e-5, -1e-6, -5000.0, 1000.0, 5208.0, 0.5):
        assert fn(F32(y)).tobytes() == rm.depth_map_factor(y).tobytes(), y


def test_constructor_text_has_the_models_order():
    """ExtractORB(0, imGray, 0, 0) -> return when empty -> UndistortKeyPoints -> ComputeStereoFromRGBD -> Nleft = -1 ->
    AssignFeaturesToGrid: the order rgbd_model.rgbd_frame restates."""
    body = _body(SRC_F, r"Frame::Frame\(\s*uint8_t\s+ClientId\s*,\s*const\s+cv::Mat\s*&\s*imGray\s*,\s*const\s+cv::Mat\s*&\s*imDepth[^)]*\)[^{]*")
    flat = re.sub(r"\s", "", body)
    marks = ["ExtractORB(0,imGray,0,0);", "if(mvKeys.empty())return;", "UndistortKeyPoints();", "ComputeStereoFromRGBD(imDepth);", "Nleft=-1;",
             "AssignFeaturesToGrid();"]
    pos = [flat.find(mk) for mk in marks]
    assert all(p >= 0 for p in pos) and pos == sorted(pos), pos
    # and GrabImageRGBD: colour conversion by channel count and mbRGB, then the depth conversion, then the constructor
    g = re.sub(r"\s", "", _grab_body())
    marks = ["if(mImGray.channels()==3)", "if(mbRGB)cvtColor(mImGray,mImGray,CV_RGB2GRAY);elsecvtColor(mImGray,mImGray,CV_BGR2GRAY);",
             "elseif(mImGray.channels()==4)", "if(mbRGB)cvtColor(mImGray,mImGray,CV_RGBA2GRAY);elsecvtColor(mImGray,mImGray,CV_BGRA2GRAY);",
             "imDepth.convertTo(imDepth,CV_32F,mDepthMapFactor);", "mCurrentFrame=Frame(mnClientId,mImGray,imDepth,"]
    pos = [g.find(mk) for mk in marks]
    assert all(p >= 0 for p in pos) and pos == sorted(pos), pos
