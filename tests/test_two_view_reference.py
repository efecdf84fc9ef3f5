"""CheckHomography, CheckFundamental, Normalize and CheckRT's gate sequence EVALUATED FROM THE REFERENCE'S OWN SOURCE TEXT and held
against tests/two_view_model.py (CPU only; runs where the reference is present -- the GPU box has none).  As in
tests/test_reference_formulas.py the bodies are cut out of S/TwoViewReconstruction.cc where they lie, translated statement by statement
(declared float -> rounding on assignment, a literal with a decimal point -> double, `x += e` -> x = float(x + e), for-loops -> range)
and executed with numpy scalars, whose promotion rules for float32 / float64 operands are C's.  Nothing of the reference is copied
into the repository: the text is read, evaluated and compared."""
import os
import re

import numpy as np
import pytest

import two_view_model as tm

REF = "/root/reference/src/orb_slam3_ros/orb_slam3"
SRC = os.path.join(REF, "src", "TwoViewReconstruction.cc")
pytestmark = pytest.mark.skipif(not os.path.isfile(SRC), reason="the reference is only present in the build container")

F32, F64 = np.float32, np.float64


def _body(signature_regex):
    text = open(SRC).read()
    m = re.search(signature_regex, text)
    assert m, signature_regex
    i = text.index("{", m.end() - 1)
    depth, j = 0, i
    while True:
        depth += text[j] == "{"
        depth -= text[j] == "}"
        if depth == 0:
            break
        j += 1
    body = re.sub(r"/\*.*?\*/", " ", text[i + 1:j], flags=re.S)
    return re.sub(r"//[^\n]*", " ", body)


def _expr(e):
    """A scalar C expression -> Python over numpy scalars: a literal with a decimal point is a double, an integer literal stays one."""
    e = re.sub(r"(?<![\w.])(\d+\.\d*|\.\d+)(?![\w.])", r"F64(\1)", e)
    return e.replace("fabs(", "abs(")


def _float_statements(body):
    """`[const] float name = expr;` statements of a straight-line body, in order -> [(name, python expression)]."""
    out = []
    for st in body.split(";"):
        m = re.match(r"\s*(?:const\s+)?float\s+(\w+)\s*=\s*(.+)$", st.strip(), flags=re.S)
        if m:
            out.append((m.group(1), _expr(" ".join(m.group(2).split()))))
    return out


def _loop_body(body):
    m = re.search(r"for\s*\(\s*int\s+i\s*=\s*0\s*;\s*i\s*<\s*N\s*;\s*i\+\+\s*\)", body)
    assert m
    i = body.index("{", m.end())
    depth, j = 0, i
    while True:
        depth += body[j] == "{"
        depth -= body[j] == "}"
        if depth == 0:
            break
        j += 1
    return body[:m.start()], body[i + 1:j]


def _run_checker(name, mats, consts_expected):
    """Executes the float statements of Check<name> for every (hypothesis, match) of a few hypotheses -> chi1, chi2 (h, n) float32."""
    body = _body(r"float\s+TwoViewReconstruction::%s\s*\(" % name)
    head, loop = _loop_body(body)
    pre = dict(_float_statements(head))
    for k, v in consts_expected.items():
        assert k in pre and F32(eval(pre[k], {"F64": F64, "sigma": F32(1.0)})) == v, (k, pre.get(k))      # `const float th = 5.991;`
    stmts = [(n, e) for n, e in _float_statements(loop) if not re.search(r"kp[12]\.pt", e)]
    assert [n for n, _ in stmts][-1] == "chiSquare2"
    # the gates and the sum, as text: `if(chiSquareK>th) bIn = false; else score += <th> - chiSquareK;`, first 1 then 2
    flat = "".join(loop.split())
    ths = "thScore" if name == "CheckFundamental" else "th"
    i1 = flat.index("if(chiSquare1>th)bIn=false;elsescore+=%s-chiSquare1;" % ths)
    i2 = flat.index("if(chiSquare2>th)bIn=false;elsescore+=%s-chiSquare2;" % ths)
    assert i1 < i2 and "floatscore=0;" in "".join(head.split())
    return stmts, pre


def _eval_pairs(stmts, env0, m, n_pairs):
    chi = np.zeros((2, n_pairs), F32)
    with np.errstate(all="ignore"):
        for i in range(n_pairs):
            env = dict(env0, u1=F32(m[0][i]), v1=F32(m[1][i]), u2=F32(m[2][i]), v2=F32(m[3][i]))
            for name, e in stmts:
                env[name] = F32(eval(e, {"F64": F64, "abs": abs}, env))
            chi[0, i], chi[1, i] = env["chiSquare1"], env["chiSquare2"]
    return chi


@pytest.mark.parametrize("which", ["CheckHomography", "CheckFundamental"])
def test_checker_text_gives_the_models_chi_squares(which):
    sc, d, a, b = tm.case("p65")
    isH = which == "CheckHomography"
    stmts, pre = _run_checker(which, None, {"th": F32(5.991)} if isH else {"th": F32(3.841), "thScore": F32(5.991)})
    inv_sigma = F32(eval(pre["invSigmaSquare"], {"F64": F64, "sigma": F32(1.0)}))
    for h in (0, 7, 32):
        env = {"invSigmaSquare": inv_sigma}
        M = a.H21[h] if isH else a.F21[h]
        for r in range(3):
            for c in range(3):
                env[("h%d%d" if isH else "f%d%d") % (r + 1, c + 1)] = F32(M[r, c])
                if isH:
                    env["h%d%dinv" % (r + 1, c + 1)] = F32(tm.inv3(a.H21[h], F32)[r, c])
        chi = _eval_pairs(stmts, env, a.m, a.N)
        want = a.chi[0 if isH else 1][:, h, :]
        assert np.array_equal(chi.view(np.uint32), want.view(np.uint32)), (which, h)


def test_normalize_text_gives_the_models_bits():
    body = _body(r"void\s+TwoViewReconstruction::Normalize\s*\(")
    # mechanical translation into Python source: loops, float declarations, `+=`, the members the function touches
    lines, indent = [], 0
    src = body.replace("{", ";{;").replace("}", ";};")
    pending_for = False
    for st in (s.strip() for s in src.split(";")):
        if not st:
            continue
        if st == "{":
            continue
        if st == "}":
            indent -= 1
            continue
        if st.startswith("for"):
            pending_for = True
            continue
        if pending_for:                      # the rest of `for(int i=0; i<N; i++)`: "i<N", "i++)" then the block
            if st.startswith("i<N"):
                continue
            if st.startswith("i++)"):
                lines.append("    " * indent + "for i in range(n):")
                indent += 1
                pending_for = False
                rest = st[len("i++)"):].strip()
                if not rest:
                    continue
                st = rest
        st = st.replace("vNormalizedPoints[i].x", "nx[i]").replace("vNormalizedPoints[i].y", "ny[i]")
        st = st.replace("vKeys[i].pt.x", "kx[i]").replace("vKeys[i].pt.y", "ky[i]")
        st = re.sub(r"T\.at<float>\((\d),(\d)\)", r"T[\1,\2]", st)
        if st.startswith("const int N") or st.startswith("vNormalizedPoints.resize"):
            continue
        if st.startswith("T = cv::Mat::eye"):
            lines.append("    " * indent + "T = np.eye(3, dtype=F32)")
            continue
        m = re.match(r"(?:float\s+)?([\w\[\],]+)\s*(\+?=)\s*(.+)$", st)
        assert m, st
        lhs, op, rhs = m.group(1), m.group(2), _expr(m.group(3))
        rhs = "%s + (%s)" % (lhs, rhs) if op == "+=" else rhs
        lines.append("    " * indent + "%s = F32(%s)" % (lhs, rhs))
    code = "\n".join(lines)
    assert code.count("for i in range(n):") == 3 and "meanDevX" in code
    for name in ("p63", "wide"):
        sc = tm.case(name)[0]
        for keys in (sc.keys1, sc.keys2):
            n = len(keys)
            env = {"F32": F32, "F64": F64, "np": np, "abs": abs, "n": n, "N": F32(n), "kx": keys[:, 0].astype(F32), "ky": keys[:, 1].astype(F32),
                   "nx": np.zeros(n, F32), "ny": np.zeros(n, F32)}
            exec(code, env)
            pn, T = tm.normalize(keys, F32)
            assert np.array_equal(env["T"].view(np.uint32), T.view(np.uint32))
            assert np.array_equal(np.stack([env["nx"], env["ny"]], axis=1).view(np.uint32), pn.view(np.uint32))


def test_check_rt_gate_sequence_in_the_text():
    """The order of CheckRT's gates in the reference's text is the order of the model's gate record (1 non-finite, 2 depth in camera 1,
    3 depth in camera 2, 4 / 5 reprojection, 6 counted), and the scalar statements of the two reprojection gates, executed on the
    model's own points, land on the side of th2 the model recorded."""
    body = _body(r"int\s+TwoViewReconstruction::CheckRT\s*\(")
    flat = "".join(body.split())
    marks = ["if(!vbMatchesInliers[i])continue;", "!isfinite(p3dC1.at<float>(0))", "if(p3dC1.at<float>(2)<=0&&cosParallax<0.99998)continue;",
             "if(p3dC2.at<float>(2)<=0&&cosParallax<0.99998)continue;", "if(squareError1>th2)continue;", "if(squareError2>th2)continue;",
             "vCosParallax.push_back(cosParallax);", "nGood++;", "if(cosParallax<0.99998)vbGood[vMatches12[i].first]=true;",
             "sort(vCosParallax.begin(),vCosParallax.end());", "size_tidx=min(50,int(vCosParallax.size()-1));", "parallax=acos(vCosParallax[idx])*180/CV_PI;"]
    pos = [flat.index(m) for m in marks]
    assert pos == sorted(pos)
    assert "floatcosParallax=normal1.dot(normal2)/(dist1*dist2);" in flat and "cv::Matp3dC2=R*p3dC1+t;" in flat
    # the reprojection statements: `float invZ1 = 1.0/p3dC1.at<float>(2);` ... `float squareError1 = ...;`
    seg = body[body.index("float im1x"):body.index("vCosParallax.push_back")]
    seg = re.sub(r"p3dC([12])\.at<float>\((\d)\)", r"p\1[\2]", seg)
    seg = re.sub(r"kp([12])\.pt\.([xy])", r"k\1\2", seg)
    stmts = []
    for st in (" ".join(s.split()) for s in seg.split(";")):
        m = re.match(r"(?:float\s+)?(\w+)\s*=\s*(.+)$", st)
        if m and not st.startswith("if"):
            stmts.append((m.group(1), _expr(m.group(2))))
    assert [n for n, _ in stmts] == ["invZ1", "im1x", "im1y", "squareError1", "invZ2", "im2x", "im2y", "squareError2"]
    sc, d, a, b = tm.case("wide")
    k = a.best_motion
    R, t = a.motion_R[k], a.motion_t[k]
    inl = a.masks[1, a.bestF]
    nG, par, counted, good, p3d, gate = tm.check_rt(R, t, a.m, inl, sc.cam, 1.0, F32)
    assert nG == a.motion_nGood[k] and set(np.unique(gate)) >= {0, 6}
    th2 = F32(4.0 * F64(F32(1.0) * F32(1.0)))
    fx, fy, cx, cy = (F32(v) for v in sc.cam)
    for i in np.nonzero(counted)[0][:50]:
        p1 = p3d[i]
        p2 = tm.mulv3(R[None], p1[None], F32, beta=t[None, :].astype(F64))[0]
        env = dict(p1=p1, p2=p2, fx=fx, fy=fy, cx=cx, cy=cy, k1x=F32(a.m[0][i]), k1y=F32(a.m[1][i]), k2x=F32(a.m[2][i]), k2y=F32(a.m[3][i]))
        for name, e in stmts:
            env[name] = F32(eval(e, {"F64": F64}, env))
        assert env["squareError1"] <= th2 and env["squareError2"] <= th2
