"""cf_draw_faces / cf_op_draw / cf_draw_layout without a GPU: the symbols are exported, declared in the header and bound in _lib.py, the
struct agrees with the header, every CF_EINVAL of the contract comes back before any device is touched with the frame buffer unchanged,
the host-side cf_draw_layout (the code the prep kernel runs) equals the numpy restatement field for field, the restatement gives the
answers worked by hand, and the inputs of the GPU cases (tests/draw_cases.py) are known not to be vacuous."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from draw_cases import (BOX, CASES, GLYPH, GLYPH_BITS, LANDMARKS, OPT, draw_layout_ref, draw_ref, image_layers, opt, permuted, row_layers,
                        standard_rows, yuv_color_ref)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc")
L = cfa._lib


def test_draw_symbols_constants_and_struct_match_the_header():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    for sym in ("cf_draw_faces", "cf_op_draw", "cf_draw_layout"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), sym
        assert sym in L.EXPORTS and hasattr(lib, sym)
        assert getattr(lib, sym).argtypes is not None, sym
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(CF_DRAW_[A-Z0-9_]+)\s+(\d+)", text)}
    assert consts == {"CF_DRAW_BOX": 1, "CF_DRAW_LANDMARKS": 2, "CF_DRAW_LABEL_NONE": 0, "CF_DRAW_LABEL_SCORE": 1, "CF_DRAW_LABEL_ID": 2}
    for k, v in consts.items():
        assert getattr(L, k) == v
    fields = re.search(r"typedef struct cf_draw_opts\s*\{(.*?)\}\s*cf_draw_opts;", code, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*[;,]", fields)
    assert [f for f, _ in L.DrawOpts._fields_] == names, names
    assert C.sizeof(L.DrawOpts) == 44
    o = L.draw_opts()
    assert (o.what, o.thickness, o.radius, o.label, o.label_scale, o.dash_held, o.scale) == (3, 1, 2, 1, 2, 1, 1.0)
    assert bytes(o.box_color) == bytes([2, 255, 0, 0]) and bytes(o.lm_color) == bytes([0, 0, 255, 0])
    # the statement is in the header and beside the code, and the kernel file is built without FMA contraction
    src = open(os.path.join(CSRC, "cf_draw.hip")).read() + open(os.path.join(CSRC, "cf_drawmath.h")).read()
    glyph_rows = [" ".join("%02X" % v for v in g) for g in GLYPH]
    for words in ["dx*dx + dy*dy <= r*r + r", "(x + y) % (8 * t)", "min(max(floor(v * f), -8192.0), 16384.0)"] + ["%d: %s" % (d, r) for d, r in enumerate(glyph_rows)]:
        assert words in text and words in src, words
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bcf_draw\.hip\b", mk, flags=re.M) and re.search(r"EXTRA_cf_draw\s*=\s*-ffp-contract=off", mk)


# ------------------------------------------------------------------------------------------ refusals
def _call(fmt=L.CF_FRAME_BGR, opts=None, B=1, h=8, w=12, pitch0=None, pitch1=None, planes="auto", boxes="auto", scores="auto", lms="auto",
          info="auto", counts="auto", H=8, W=12, null_opts=False):
    """One cf_op_draw call on a fresh noise frame: (return code, frame unchanged?)."""
    bgr, il = fmt == L.CF_FRAME_BGR, fmt in (L.CF_YUV_NV12, L.CF_YUV_NV21)
    buf = np.random.default_rng(1).integers(0, 256, 8192 * 3 + 64, dtype=np.uint8)
    keep = buf.copy()
    tab = (L.PlanesRW * 1)()
    if planes == "auto":
        tab[0].p0, tab[0].p1, tab[0].p2 = buf.ctypes.data, buf.ctypes.data + 4096, buf.ctypes.data + 8192
    elif planes is not None:
        tab[0].p0, tab[0].p1, tab[0].p2 = [(buf.ctypes.data + 4096 * k) if on else None for k, on in enumerate(planes)]
    pitch0 = (3 * w if bgr else w) if pitch0 is None else pitch0
    pitch1 = (0 if bgr else w if il else w // 2) if pitch1 is None else pitch1
    bx = np.float32([[2, 2, 8, 6]]) if isinstance(boxes, str) else boxes
    sc = np.float32([0.5]) if isinstance(scores, str) else scores
    lm = np.float32([[3, 3, 4, 4, 5, 5, 6, 4, 7, 3]]) if isinstance(lms, str) else lms
    nf = np.int32([[1, 1, 0]]) if isinstance(info, str) else info
    cn = np.array([1], np.int32) if isinstance(counts, str) else counts
    o = opts if opts is not None else L.draw_opts()
    r = L.lib().cf_op_draw(0, None if null_opts else C.byref(o), fmt, None if planes is None else tab, B, h, w, pitch0, pitch1,
                           L.ptr(bx), L.ptr(sc), L.ptr(lm), L.ptr(nf), L.ptr(cn), H, W)
    return r, np.array_equal(buf, keep)


def test_op_draw_refuses_bad_arguments_before_any_device_work():
    D = L.draw_opts
    bad = [
        dict(fmt=-1), dict(fmt=5), dict(fmt=99),
        dict(opts=D(what=4)), dict(opts=D(what=-1)), dict(opts=D(what=7)), dict(opts=D(label=3)), dict(opts=D(label=-1)),
        dict(opts=D(what=0, label="none")),
        dict(opts=D(thickness=0)), dict(opts=D(thickness=17)), dict(opts=D(thickness=-1)),
        dict(opts=D(radius=-1)), dict(opts=D(radius=17)),
        dict(opts=D(label_scale=0)), dict(opts=D(label_scale=9)), dict(opts=D(label_scale=-2)),
        dict(opts=D(dash_held=2)), dict(opts=D(dash_held=-1)),
        dict(opts=D(scale=0.2)), dict(opts=D(scale=4.5)), dict(opts=D(scale=float("nan"))), dict(opts=D(scale=float("inf"))), dict(opts=D(scale=-1.0)),
        dict(fmt=L.CF_YUV_NV12, h=7), dict(fmt=L.CF_YUV_I420, w=11), dict(fmt=L.CF_YUV_YV12, h=7, w=11),
        dict(h=0), dict(w=0), dict(h=8193), dict(w=8193), dict(h=-8),
        dict(pitch0=35), dict(fmt=L.CF_YUV_NV12, pitch0=11), dict(fmt=L.CF_YUV_NV21, pitch1=11), dict(fmt=L.CF_YUV_I420, pitch1=5),
        dict(planes=None), dict(planes=(False, True, True)), dict(fmt=L.CF_YUV_NV12, planes=(True, False, True)),
        dict(fmt=L.CF_YUV_I420, planes=(True, True, False)), dict(fmt=L.CF_YUV_YV12, planes=(True, False, True)),
        dict(B=0), dict(null_opts=True), dict(counts=None), dict(boxes=None), dict(scores=None), dict(counts=np.array([-1], np.int32)),
        dict(H=0), dict(W=0),
        dict(lms=None), dict(opts=D(label="id"), info=None),                 # CF_DRAW_LANDMARKS without rows, CF_DRAW_LABEL_ID without info
    ]
    for kw in bad:
        r, same = _call(**kw)
        assert r == -1 and same, kw
        assert b"cf_op_draw" in L.lib().cf_op_last_error(), kw
    # fine arguments get as far as the device (none here: CF_EHIP) or succeed: an odd BGR frame, no landmarks wanted and none given, a
    # 1 x 1 frame, no info with the score label
    for kw in (dict(h=7, w=11), dict(opts=D(landmarks=False), lms=None), dict(h=1, w=1), dict(info=None), dict(opts=D(what=0, label="score"))):
        assert _call(**kw)[0] != -1, kw
    # the context form: nothing without a context
    o = D()
    tab = (L.PlanesRW * 1)()
    assert L.lib().cf_draw_faces(None, C.byref(o), L.CF_FRAME_BGR, tab, 0, 1, 8, 12, 36, 0) == -1
    # cf_draw_layout refuses the same options and sizes
    out = np.zeros(32, np.int32)
    box = np.float32([1, 1, 5, 4])
    for o, hw, HW in ((D(thickness=0), (6, 8), (6, 8)), (D(what=0, label="none"), (6, 8), (6, 8)), (D(), (0, 8), (6, 8)), (D(), (6, 8193), (6, 8)),
                      (D(), (6, 8), (0, 8)), (D(scale=5.0), (6, 8), (6, 8))):
        assert L.lib().cf_draw_layout(C.byref(o), L.ptr(box), 0.5, None, None, hw[0], hw[1], HW[0], HW[1], L.ptr(out)) == -1
        assert b"cf_draw_layout" in L.lib().cf_op_last_error()
    assert L.lib().cf_draw_layout(C.byref(D()), None, 0.5, None, None, 6, 8, 6, 8, L.ptr(out)) == -1
    assert L.lib().cf_draw_layout(C.byref(D()), L.ptr(box), 0.5, None, None, 6, 8, 6, 8, None) == -1


def test_python_wrappers_refuse_what_they_can_see():
    with pytest.raises(ValueError):
        L.draw_opts(label="name")
    with pytest.raises(ValueError):
        L.draw_opts(box_color=(0, 0))
    with pytest.raises(ValueError):
        L.draw_opts(lm_color=(0, 0, 256))
    with pytest.raises(TypeError):
        L.draw_opts(colour=(0, 0, 0))
    img = np.zeros((1, 8, 12, 3), np.uint8)
    box = np.float32([[2, 2, 8, 6]])
    with pytest.raises(ValueError):
        ops.draw_faces(img, box, [0.5], [2], (8, 12), landmarks=False)                      # counts do not sum to the rows
    with pytest.raises(ValueError):
        ops.draw_faces(img, box, [0.5, 0.6], [1], (8, 12), landmarks=False)                 # scores of another length
    with pytest.raises(ValueError):
        ops.draw_faces(img, box, [0.5], [1], (8, 12), lms=np.zeros((2, 10)))
    for kw in (dict(thickness=0), dict(scale=0.1), dict(what=9), dict(label=5), dict()):    # dict(): landmarks wanted, none given
        with pytest.raises(cfa._lib.CenterFaceValueError):
            ops.draw_faces(img, box, [0.5], [1], (8, 12), **kw)
        assert not img.any()


# ------------------------------------------------------------------------------------------ cf_draw_layout == the restatement
def _layout_pair(o, box, score, lms, info, hw, HW):
    kw = dict(o)
    got = ops.draw_layout(box, score, hw, HW, lms=lms, info=info, **kw)
    want = draw_layout_ref(o, box, score, lms, info, hw[0], hw[1], HW[0], HW[1])
    assert got.dtype == want.dtype and np.array_equal(got, want), (o, box, score, lms, info, hw, HW, got.tolist(), want.tolist())
    return got


def test_layout_equals_the_restatement_field_for_field():
    nan, inf = float("nan"), float("inf")
    lm0 = [1, 1, 2.5, 2.5, 3, 3, 4, 4, 5, 5]
    hand = [
        # corners on .0 and .5, negative coordinates, beyond the frame, the clamps
        ([1, 1, 5, 4], (6, 8), (6, 8)), ([1.5, 1.5, 5.5, 4.5], (6, 8), (6, 8)), ([0.5, 0.5, 1.0, 1.0], (6, 8), (6, 8)),
        ([-3.5, -2.0, 4.0, 3.5], (6, 8), (6, 8)), ([-0.5, -0.5, 0.5, 0.5], (6, 8), (6, 8)), ([20, 20, 40, 50], (6, 8), (6, 8)),
        ([-1e6, -1e6, 1e6, 1e6], (6, 8), (6, 8)), ([-20000, 3, -10000, 9], (64, 64), (64, 64)), ([10000, 3, 30000, 9], (64, 64), (32, 32)),
        ([3e38, 0, 3.4e38, 5], (6, 8), (6, 8)), ([-3.4e38, 0, 3.4e38, 5], (6, 8), (6, 8)),
        # skipped rows
        ([nan, 1, 5, 4], (6, 8), (6, 8)), ([1, inf, 5, 4], (6, 8), (6, 8)), ([1, 1, -inf, 4], (6, 8), (6, 8)), ([1, 1, 5, nan], (6, 8), (6, 8)),
        ([3, 1, 3, 4], (6, 8), (6, 8)), ([5, 1, 3, 4], (6, 8), (6, 8)), ([1, 4, 5, 4], (6, 8), (6, 8)),
        # anisotropic and non-dyadic factors
        ([10, 10, 30, 20], (1080, 1920), (480, 640)), ([10.3, 7.7, 31.9, 22.1], (75, 101), (64, 96)), ([3, 3, 9, 9], (37, 51), (32, 48)),
        ([0.1, 0.2, 0.30000001, 0.7], (8192, 8192), (1, 1)),
    ]
    ids = (1, 42, 2147483647, 0, -3)
    scores = (np.float32(0.3), np.float32(0.999), np.float32(1.0), nan, np.float32(-0.0), np.float32(0.0), inf, -inf, np.float32(7.5), np.float32(-2.0),
              np.float32(0.29), np.float32(0.07), np.float32(3.4e38))
    n = 0
    for box, hw, HW in hand:
        for label in ("none", "score", "id"):
            for k, (score, tid) in enumerate(zip(scores, ids * 3)):
                o = opt(label=label, label_scale=1 + k % 8, thickness=1 + (3 * k) % 16, scale=(1.0, 1.3, 0.25, 4.0)[k % 4])
                lms = [lm0, None, [nan, 1, 2, inf, -inf, 3, 1e9, -1e9, 5.5, 5.5]][k % 3]
                _layout_pair(o, box, score, lms, [tid, 1, k % 3], hw, HW)
                _layout_pair(o, box, score, lms, None, hw, HW)
                n += 2
    # the plate above the box and, at Y1 < 9k, inside it
    for y1, k, t, want_y0 in ((9, 1, 1, 0), (8, 1, 1, 9), (8, 1, 5, 13), (40, 4, 2, 4), (35, 4, 2, 37), (0, 8, 16, 16)):
        got = _layout_pair(opt(label="id", label_scale=k, thickness=t), [3, y1, 30, 60], 0.5, None, [42, 1, 0], (64, 64), (64, 64))
        assert got[2] == y1 and got[7] == want_y0 and got[6] == 3 and got[8] == k * 13 and got[9] == 9 * k and got[10] == 2 and list(got[11:13]) == [4, 2]
    # seeded rows
    rng = np.random.default_rng(11)
    for i in range(300):
        hw = (int(rng.integers(1, 200)), int(rng.integers(1, 300)))
        HW = (int(rng.integers(1, 200)), int(rng.integers(1, 300)))
        c = rng.uniform(-20, 320, 2)
        half = rng.uniform(-1, 60, 2) * (0.5 if i % 7 else 1.0)
        box = np.float32([c[0] - half[0], c[1] - half[1], c[0] + half[0], c[1] + half[1]])
        if i % 5 == 0:
            box = np.round(box * 2) / 2                                       # corners on .0 and .5
        lms = np.float32(rng.uniform(-30, 330, 10))
        if i % 11 == 0:
            lms[int(rng.integers(0, 10))] = (nan, inf, -inf)[i % 3]
        o = opt(label=("none", "score", "id")[i % 3], label_scale=int(rng.integers(1, 9)), thickness=int(rng.integers(1, 17)),
                scale=float(np.float32(rng.uniform(0.25, 4.0))))
        info = [int(rng.integers(-2, 2 ** 31 - 1)) if i % 4 else int(rng.integers(1, 100)), 1, int(rng.integers(0, 3))]
        _layout_pair(o, box, np.float32(rng.uniform(-0.1, 1.1)), lms if i % 6 else None, info if i % 9 else None, hw, HW)
        n += 1
    assert n > 1000
    # known fields: a skipped row is all zeros; scores and ids become these digits
    assert not _layout_pair(opt(), [nan, 1, 5, 4], 0.5, lm0, [1, 1, 0], (6, 8), (6, 8)).any()
    for score, digits in ((np.float32(0.3), [3, 0]), (np.float32(0.999), [9, 9]), (np.float32(1.0), [1, 0, 0]), (np.float32(-0.0), [0]), (np.float32(7.5), [1, 0, 0]),
                          (np.float32(0.29), [2, 8]), (nan, [])):
        got = _layout_pair(opt(label="score"), [1, 1, 5, 4], score, None, None, (6, 8), (6, 8))
        assert got[10] == len(digits) and list(got[11:11 + len(digits)]) == digits, (score, got.tolist())     # float32(0.3) * 100 = 30.000001, float32(0.29) * 100 = 28.99999
    for tid, digits in ((1, [1]), (42, [4, 2]), (2147483647, [2, 1, 4, 7, 4, 8, 3, 6, 4, 7]), (0, [])):
        got = _layout_pair(opt(label="id"), [1, 1, 5, 4], 0.5, None, [tid, 1, 1], (6, 8), (6, 8))
        assert got[5] == 1 and got[10] == len(digits) and list(got[11:11 + len(digits)]) == digits
    # the clamps
    got = _layout_pair(opt(), [-1e6, -1e6, 1e6, 1e6], 0.5, [1e9, -1e9] * 5, None, (6, 8), (6, 8))
    assert list(got[1:5]) == [-8192, -8192, 16384, 16384] and list(got[22:24]) == [16384, -8192] and got[21] == 31


# ------------------------------------------------------------------------------------------ known answers of the restatement
def _rec(box, o, hw, score=0.5, lms=None, info=None):
    return draw_layout_ref(o, box, score, lms, info, hw[0], hw[1], hw[0], hw[1])


def test_restatement_outline_of_thickness_one():
    """Box (1,1)-(5,4) on an 8 x 6 frame: the ring cv2.rectangle(img, (1, 1), (5, 4), c, 1) names -- rows 1 and 4 from x = 1 to 5, columns
    1 and 5 between them; 14 pixels."""
    Lm = row_layers(_rec([1, 1, 5.5, 4.2], opt(what=BOX, label="none"), (6, 8)), opt(what=BOX, label="none"), 6, 8)
    want = np.zeros((6, 8), np.uint8)
    want[1, 1:6] = want[4, 1:6] = 2
    want[1:5, 1] = want[1:5, 5] = 2
    assert np.array_equal(Lm, want) and int((Lm > 0).sum()) == 14
    # t = 2 fills it: the box is 5 x 4, thinner than 2t in y
    L2 = row_layers(_rec([1, 1, 5.5, 4.2], opt(what=BOX, label="none", thickness=2), (6, 8)), opt(what=BOX, label="none", thickness=2), 6, 8)
    fill = np.zeros((6, 8), np.uint8)
    fill[1:5, 1:6] = 2
    assert np.array_equal(L2, fill)
    # held and dashed, t = 1: of the ring's pixels those with (x + y) % 8 < 4; layer 1
    o = opt(what=BOX, label="none")
    Ld = row_layers(_rec([1, 1, 5.5, 4.2], o, (6, 8), info=[5, 3, 1]), o, 6, 8)
    y, x = np.mgrid[0:6, 0:8]
    assert np.array_equal(Ld, np.where((want > 0) & ((x + y) % 8 < 4), 1, 0).astype(np.uint8)) and Ld.any()


def test_restatement_dot_of_radius_two_and_zero():
    o = opt(what=LANDMARKS, label="none", radius=2)
    lms = [4, 3] + [1e9, 1e9] * 4
    Lm = row_layers(_rec([0, 0, 2, 2], o, (7, 9), lms=lms), o, 7, 9)
    want = np.zeros((7, 9), np.uint8)
    want[1:6, 2:7] = 4
    for yy, xx in ((1, 2), (1, 6), (5, 2), (5, 6)):
        want[yy, xx] = 0
    assert np.array_equal(Lm, want) and int((Lm == 4).sum()) == 21           # the 5 x 5 square without its corners
    o0 = opt(what=LANDMARKS, label="none", radius=0)
    L0 = row_layers(_rec([0, 0, 2, 2], o0, (7, 9), lms=lms), o0, 7, 9)
    assert int((L0 == 4).sum()) == 1 and L0[3, 4] == 4
    # a held row's landmarks are not drawn
    assert not row_layers(_rec([0, 0, 2, 2], o, (7, 9), lms=lms, info=[1, 1, 2]), o, 7, 9).any()


def test_restatement_ink_of_seven():
    """Id 7 at k = 1 over a box at (2, 12): the plate is [2, 9) x [3, 12), 7 x 9 pixels of layer 2 with the glyph 1F 01 02 04 08 08 08 in
    ink one pixel in from its top left corner."""
    o = opt(what=0, label="id", label_scale=1)
    Lm = row_layers(_rec([2, 12, 10, 18], o, (20, 16), info=[7, 1, 0]), o, 20, 16)
    want = np.zeros((20, 16), np.uint8)
    want[3:12, 2:9] = 2
    seven = ["#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."]
    for r, line in enumerate(seven):
        for c, ch in enumerate(line):
            if ch == "#":
                want[4 + r, 3 + c] = 3
    assert np.array_equal(Lm, want)
    assert np.array_equal(GLYPH_BITS[7], np.array([[ch == "#" for ch in line] for line in seven]))
    # k = 2: every cell is a 2 x 2 block
    o2 = opt(what=0, label="id", label_scale=2)
    L2 = row_layers(_rec([2, 20, 10, 28], o2, (30, 20), info=[7, 1, 0]), o2, 30, 20)
    assert np.array_equal(L2[2:20, 2:16], np.kron(want[3:12, 2:9], np.ones((2, 2), np.uint8)))


def test_colour_conversions():
    for bgr, yuv in (((255, 255, 255), (235, 128, 128)), ((0, 0, 0), (16, 128, 128)), ((2, 255, 0), (145, 55, 34))):
        assert yuv_color_ref(bgr) == yuv and ops.bgr_to_yuv_color(bgr) == yuv
    rng = np.random.default_rng(0)
    for bgr in rng.integers(0, 256, (200, 3)):
        got = ops.bgr_to_yuv_color(bgr)
        assert got == yuv_color_ref(bgr) and 16 <= got[0] <= 235 and 16 <= got[1] <= 240 and 16 <= got[2] <= 240


def test_restatement_highest_layer_wins_and_chroma_takes_it():
    """A dot on an outline on a plate: 4 over 2; the chroma sample under a lone dot pixel takes the dot's colour, its three luma
    neighbours stay."""
    o = opt(radius=0, label="none", what=BOX | LANDMARKS)
    y = np.full((8, 8), 7, np.uint8)
    c = np.full((4, 8), 9, np.uint8)
    draw_ref([(y, c)], "nv12", [[2, 2, 6.5, 6.5]], [0.5], [1], (8, 8), 8, 8, lms=[[2, 2, 5, 5] + [1e9] * 6], info=None, **o)
    assert y[2, 2] == o["lm_color"][0] and y[2, 3] == o["box_color"][0] and y[5, 5] == o["lm_color"][0] and y[3, 3] == 7 and y[4, 5] == 7
    assert tuple(c[1, 2:4]) == tuple(o["lm_color"][1:]) and tuple(c[2, 4:6]) == tuple(o["lm_color"][1:])      # (1,1): dot over outline; (2,2): lone dot
    assert tuple(c[1, 4:6]) == tuple(o["box_color"][1:]) and tuple(c[2, 2:4]) == tuple(o["box_color"][1:]) and tuple(c[0, 0:2]) == (9, 9)
    # NV21 stores V first
    c2 = np.full((4, 8), 9, np.uint8)
    draw_ref([(y.copy(), c2)], "nv21", [[2, 2, 6.5, 6.5]], [0.5], [1], (8, 8), 8, 8, lms=[[2, 2, 5, 5] + [1e9] * 6], info=None, **o)
    assert tuple(c2[1, 2:4]) == tuple(o["lm_color"][:0:-1])


# ------------------------------------------------------------------------------------------ the GPU cases are not vacuous
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gpu_case_inputs_draw_something(case):
    fr = case.frames()
    want, maps = case.expect(fr)
    assert not want.same(fr), case.name                                       # the restatement changed at least one byte
    # padding and guards are not drawn on
    for a, b, (r, c), p in zip(want.bufs, fr.bufs, case_geo(want), case_pitches(want)):
        if not case.dense:
            body = np.zeros(len(a), bool)
            body[:r * p].reshape(r, p)[:, :c] = True
            assert np.array_equal(a[~body], b[~body])
    if case.layers:
        owned = {k: sum(int((m == k).sum()) for m in maps) for k in (1, 2, 3, 4)}
        assert all(v > 0 for v in owned.values()), (case.name, owned)
    # another row order gives the same picture
    other, _ = permuted(case).expect(fr)
    assert other.same(want), case.name


def case_geo(fr):
    return fr.geo * fr.B


def case_pitches(fr):
    return fr.pitches * fr.B


def test_standard_rows_reach_what_they_are_meant_to():
    """The hand-made rows of the 48 x 64 cases: boxes across each frame edge and the tile edges y = 16, 32, one outside, skipped rows, a
    box thinner than 2t at t = 3, plates that cross, a plate clipped by the top and by the right edge."""
    h, w, net = 48, 64, (32, 48)
    b, s, l, i = standard_rows(h, w, *net)
    o = opt(label="id", thickness=3)
    recs = [draw_layout_ref(o, b[k], s[k], l[k], i[k], h, w, *net) for k in range(len(b))]
    ok = [r for r in recs if r[0]]
    assert len(recs) - len(ok) == 2
    assert any(r[1] < 0 <= r[3] for r in ok) and any(r[2] < 0 <= r[4] for r in ok) and any(r[1] < w <= r[3] for r in ok) and any(r[2] < h <= r[4] for r in ok)
    assert any(r[1] >= w and r[2] >= h for r in ok)
    assert any(r[2] < 16 <= r[4] for r in ok) and any(r[2] < 32 <= r[4] for r in ok)
    assert any(r[3] - r[1] + 1 < 2 * 3 for r in ok)
    assert any(r[10] == 10 and r[6] + r[8] > w for r in ok)                   # ten digits, clipped by the right edge
    assert any(r[10] > 0 and r[7] < 0 for r in ok)                            # clipped by the top edge
    plates = [(r[6], r[7], r[6] + r[8], r[7] + r[9], r[5]) for r in ok if r[10]]
    assert any(a[4] != c[4] and a[0] < c[2] and c[0] < a[2] and a[1] < c[3] and c[1] < a[3] for a in plates for c in plates)      # a held plate crosses a live one
    Lm = image_layers(opt(), b, s, l, i, h, w, *net)
    assert Lm[0, 0] == 4 and all((Lm == k).any() for k in (1, 2, 3, 4))
