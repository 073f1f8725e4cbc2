"""Rotated sources (cf_rot_geometry, cf_forward_rot, cf_op_rot, cf_op_unrot): what can be checked without a GPU -- the declarations, the
host-only geometry against the restatement of tests/rot_cases.py, the refusals that come before any device work (each names its value),
the restated row mapping by hand, and the words the documents owe."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
import csrc_text
from fit_cases import WORKED, fit_geometry_ref
from rot_cases import ROTS, rot_geometry_ref, rot_ref, unrot_ref, upright

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = cfa._lib
SYMBOLS = ("cf_rot_geometry", "cf_forward_rot", "cf_op_rot", "cf_op_unrot")
CSRC = os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc")


def test_rot_symbols_and_struct_match_the_header():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), sym
        assert sym in L.EXPORTS and hasattr(lib, sym)
        assert getattr(lib, sym).argtypes is not None, sym
    body = re.search(r"typedef struct cf_rot_opts\s*\{(.*?)\}\s*cf_rot_opts;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("int32_t", "rot"), ("int32_t", "stretch"), ("cf_fit_opts", "fit")]
    assert [n for n, _ in L.RotOpts._fields_] == ["rot", "stretch", "fit"] and L.RotOpts._fields_[2][1] is L.FitOpts
    assert C.sizeof(L.RotOpts) == 20 and C.sizeof(L.FitOpts) == 12 and C.sizeof(L.FitGeom) == 16     # additive: the fit's structs stayed
    assert lib.cf_version() == 100
    o = L.rot_opts(90)
    assert (o.rot, o.stretch) == (90, 1)
    o = L.rot_opts(270, True)
    assert (o.rot, o.stretch, o.fit.anchor, o.fit.upscale, list(o.fit.fill)) == (270, 0, 0, 1, [0, 0, 0, 0])
    o = L.rot_opts(180, dict(anchor="topleft", upscale=False, fill=(1, 2, 3)))
    assert (o.rot, o.stretch, o.fit.anchor, o.fit.upscale, list(o.fit.fill)) == (180, 0, 1, 0, [1, 2, 3, 0])
    assert L.rot_opts(0, {}).stretch == 0                                   # an empty dict is a fit with the defaults, not a stretch
    # the new file shares the one statement of the resize and of the conversion and is built without contraction
    # (through the cutters' shared header: required of the union, refused in every file of it)
    texts = csrc_text.unit("cf_rot.hip")
    src = texts["cf_rot.hip"]
    assert '#include "cf_cutpx.h"' in src
    csrc_text.assert_one_statement(texts, ('#include "cf_cvresize.h"', '#include "cf_yuvmath.h"', "cv_linear_coeffs(", "cv_linear_vpass(", "yuv_px(", "pack_bgr("))
    assert "__builtin_amdgcn_perm" not in src                               # the byte-selecting pack is stated once, in the header
    # rot 0 and rot 180 are the fit's own kernel and launch; the fit's launch hands the quarter turns to this file
    fit = open(os.path.join(CSRC, "cf_fit.hip")).read()
    assert "fit_frames_kernel<SRC, VF, 0>" in fit and "fit_frames_kernel<SRC, VF, 2>" in fit and "launch_rot_quarter(" in fit
    assert "launch_rot_quarter(" in src and "rot_quarter_kernel" in src and "rot_half_kernel" not in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "cf_rot.hip" in srcs and re.search(r"EXTRA_cf_rot\s*=\s*-ffp-contract=off", mk)


# ------------------------------------------------------------------------------------------ the geometry
def _geometry(h, w, H, W, rot=0, stretch=0, anchor=0, upscale=1, null=None):
    o = L.RotOpts(rot, stretch, L.FitOpts(anchor, upscale, (C.c_uint8 * 4)(0, 0, 0, 0)))
    g = L.FitGeom(-7, -7, -7, -7)
    code = L.lib().cf_rot_geometry(None if null == "o" else C.byref(o), h, w, H, W, None if null == "g" else C.byref(g))
    return code, (g.rw, g.rh, g.dx, g.dy)


def test_rot_geometry_equals_the_restatement():
    for (h, w), (H, W), up, want in WORKED:
        for rot in ROTS:
            sh, sw = (w, h) if rot in (90, 270) else (h, w)                 # the STORED frame whose upright view is the worked h x w
            assert rot_geometry_ref(sh, sw, H, W, rot, 0, "center", bool(up)) == want
            assert _geometry(sh, sw, H, W, rot, 0, 0, up) == (0, want), (h, w, rot)
            assert _geometry(sh, sw, H, W, rot, 0, 1, up) == (0, want[:2] + (0, 0))
            assert _geometry(sh, sw, H, W, rot, 1, 0, up) == (0, (W, H, 0, 0))
            assert ops.rot_geometry(sh, sw, H, W, rot, dict(upscale=bool(up))) == want
            assert ops.rot_geometry(sh, sw, H, W, rot) == (W, H, 0, 0)
    for h, w, H, W in [(h, w, H, W) for h in range(2, 30, 3) for w in range(2, 30, 5) for H, W in ((32, 64), (64, 32))] + [(1080, 1920, 640, 640)]:
        for rot in ROTS:
            for anchor in (0, 1):
                for up in (0, 1):
                    want = rot_geometry_ref(h, w, H, W, rot, 0, anchor, bool(up))
                    assert _geometry(h, w, H, W, rot, 0, anchor, up) == (0, want), (h, w, H, W, rot, anchor, up)
                    assert want == (fit_geometry_ref(w, h, H, W, anchor, bool(up)) if rot in (90, 270) else fit_geometry_ref(h, w, H, W, anchor, bool(up)))
    assert rot_geometry_ref(1080, 1920, 640, 640, 90, 0) == (360, 640, 140, 0)          # a corridor camera: the content stands upright


def test_rot_geometry_refuses_bad_values_and_names_them():
    lib = L.lib()
    for kw in (dict(rot=45), dict(rot=-90), dict(rot=360), dict(rot=1), dict(stretch=2), dict(stretch=-1), dict(anchor=2), dict(upscale=2), dict(h=1),
               dict(w=8193), dict(H=0), dict(W=0), dict(null="o"), dict(null="g"), dict(stretch=1, anchor=2)):
        a = dict(h=8, w=12, H=32, W=32)
        a.update(kw)
        code, g = _geometry(**a)
        assert code == -1 and g == (-7, -7, -7, -7), kw
        assert b"cf_rot_geometry" in lib.cf_op_last_error(), kw
    assert _geometry(8, 12, 32, 32, rot=45)[0] == -1 and b"rot=45" in lib.cf_op_last_error()
    assert _geometry(8, 12, 32, 32, stretch=3)[0] == -1 and b"stretch=3" in lib.cf_op_last_error()
    assert _geometry(8, 12, 32, 32, rot=90, anchor=5)[0] == -1 and b"anchor 5" in lib.cf_op_last_error()
    assert _geometry(8, 8193, 32, 32, rot=90)[0] == -1 and b"w=8193" in lib.cf_op_last_error()
    with pytest.raises(ValueError):
        ops.rot_geometry(8, 12, 32, 32, 45)


# ------------------------------------------------------------------------------------------ refusals before any device work
POISON = 0xA5


def _frames():
    buf = np.zeros(3 * 4096, np.uint8)
    tab = (L.YuvPlanes * 1)()
    tab[0].y, tab[0].c0, tab[0].c1 = [buf.ctypes.data + 4096 * k for k in range(3)]
    return tab, buf


def _op_rot(rot=90, stretch=0, fmt=L.CF_FRAME_BGR, B=1, h=8, w=12, pitch0=None, H=4, W=8, anchor=0, upscale=1, opts=True, out=True, forward=False):
    tab, buf = _frames()
    pitch0 = (3 * w if fmt == L.CF_FRAME_BGR else w) if pitch0 is None else pitch0
    pitch1 = 0 if fmt == L.CF_FRAME_BGR else w
    o = L.RotOpts(rot, stretch, L.FitOpts(anchor, upscale, (C.c_uint8 * 4)(0, 0, 0, 0)))
    if forward:
        return L.lib().cf_forward_rot(None, C.byref(o) if opts else None, fmt, tab, 0, B, h, w, pitch0, pitch1), True
    canvas = np.full((max(B, 1), max(H, 1), max(W, 1), 3), POISON, np.uint8)
    code = L.lib().cf_op_rot(0, C.byref(o) if opts else None, fmt, tab, B, h, w, pitch0, pitch1, H, W, L.ptr(canvas) if out else None)
    return code, bool((canvas == POISON).all())


REFUSALS = [dict(rot=45), dict(rot=-90), dict(rot=91), dict(rot=360), dict(stretch=2), dict(stretch=-1), dict(opts=False), dict(anchor=2), dict(upscale=-1),
            dict(stretch=1, anchor=2), dict(fmt=5), dict(B=0), dict(h=1), dict(w=8194), dict(fmt=L.CF_YUV_NV12, h=7), dict(pitch0=35)]


def test_rot_entry_points_refuse_bad_arguments_before_any_device_work():
    lib = L.lib()
    for kw in REFUSALS + [dict(W=6), dict(H=0), dict(out=False)]:
        code, untouched = _op_rot(**kw)
        assert code == -1 and untouched, kw
        assert b"cf_op_rot" in lib.cf_op_last_error(), kw
    for forward in (False, True):
        assert _op_rot(rot=45, forward=forward)[0] == -1 and b"rot=45" in lib.cf_op_last_error()
        assert _op_rot(stretch=7, forward=forward)[0] == -1 and b"stretch=7" in lib.cf_op_last_error()
        assert _op_rot(anchor=7, forward=forward)[0] == -1 and b"anchor 7" in lib.cf_op_last_error()
        assert _op_rot(w=8194, forward=forward)[0] == -1 and b"w=8194" in lib.cf_op_last_error()
        assert _op_rot(pitch0=35, forward=forward)[0] == -1 and b"pitch0=35" in lib.cf_op_last_error()
    # cf_forward_rot without a context: every refusal is reported before "null context"
    for kw in REFUSALS:
        assert _op_rot(forward=True, **kw)[0] == -1, kw
        assert b"cf_forward_rot" in lib.cf_op_last_error() and b"null context" not in lib.cf_op_last_error(), kw
    for rot in ROTS:
        assert _op_rot(rot=rot, forward=True)[0] == -1 and b"cf_forward_rot: null context" in lib.cf_op_last_error()
    # fine arguments get as far as the device (none here) or succeed
    for kw in (dict(), dict(rot=0), dict(rot=180, stretch=1), dict(rot=270, h=7, w=11), dict(fmt=L.CF_YUV_NV12)):
        assert _op_rot(**kw)[0] != -1, kw

    def unrot(rot=90, stretch=0, B=1, h=8, w=12, H=32, W=32, rows=2, max_out=4, null=None, anchor=0):
        a = {k: np.zeros(s, np.float32) for k, s in (("d", (max(B, 1), max(rows, 1), 4)), ("s", (max(B, 1), max(rows, 1))), ("l", (max(B, 1), max(rows, 1), 10)))}
        od, ol = np.full((max(B, 1), max(max_out, 1), 5), 7.5, np.float32), np.full((max(B, 1), max(max_out, 1), 10), 7.5, np.float32)
        cn, oc, fl = np.zeros(max(B, 1), np.int32), np.full(max(B, 1), -9, np.int32), np.full(max(B, 1), -9, np.int32)
        o = L.RotOpts(rot, stretch, L.FitOpts(anchor, 1, (C.c_uint8 * 4)(0, 0, 0, 0)))
        p = {k: (None if k == null else L.ptr(v)) for k, v in dict(a, cn=cn, od=od, ol=ol, oc=oc, fl=fl).items()}
        code = lib.cf_op_unrot(0, None if null == "o" else C.byref(o), B, h, w, H, W, p["d"], p["s"], p["l"], p["cn"], rows, max_out, p["od"], p["ol"],
                               p["oc"], p["fl"])
        return code, bool((od == 7.5).all() and (ol == 7.5).all() and (oc == -9).all() and (fl == -9).all())
    for kw in (dict(rot=45), dict(stretch=2), dict(anchor=2), dict(B=0), dict(rows=0), dict(max_out=0), dict(h=1), dict(W=0), dict(null="o"), dict(null="d"),
               dict(null="s"), dict(null="l"), dict(null="cn"), dict(null="od"), dict(null="ol"), dict(null="oc"), dict(null="fl")):
        code, untouched = unrot(**kw)
        assert code == -1 and untouched, kw
        assert b"cf_op_unrot" in lib.cf_op_last_error(), kw
    assert unrot(rot=45)[0] == -1 and b"rot=45" in lib.cf_op_last_error()
    assert unrot()[0] != -1 and unrot(rot=270, stretch=1, h=7, w=11)[0] != -1


def test_python_wrappers_refuse_what_they_can_see():
    img = np.zeros((1, 8, 12, 3), np.uint8)
    with pytest.raises(ValueError):
        ops.rot_frames(img, (4, 8), rot=45)
    with pytest.raises(ValueError):
        ops.rot_frames(img, (4, 6), rot=90)
    with pytest.raises(ValueError):
        ops.rot_frames(img, (4, 8), rot=90, fit=dict(anchor="middle"))
    with pytest.raises(ValueError):
        ops.unrot_rows((8, 12), (32, 32), np.zeros((1, 2, 3)), np.zeros((1, 2)), np.zeros((1, 2, 10)), [0], 4, rot=90)
    # rotate= together with tiled=True, and a turn outside the four, are refused by every product path before any engine exists
    face = cfa.CenterFace.__new__(cfa.CenterFace)
    assert [face._rotation(r) for r in ROTS] == list(ROTS) and face._rotation(0, True) == 0
    frames, yuv = np.zeros((1, 8, 12, 3), np.uint8), np.zeros((1, 12, 12), np.uint8)
    for rotate, words in ((90, ("rotate", "tiled")), (45, ("rotate", "45"))):
        tiled = rotate == 90
        for call in (lambda: face.anonymize(frames, rotate=rotate, tiled=tiled), lambda: face.anonymize_yuv(yuv, rotate=rotate, tiled=tiled),
                     lambda: face.annotate(frames, rotate=rotate, tiled=tiled), lambda: face.annotate_yuv(yuv, rotate=rotate, tiled=tiled),
                     lambda: face.detect_fit(frames, rotate=rotate) if not tiled else face._plan(frames, "bgr", "given", rotate=rotate, tiled=True)):
            with pytest.raises(ValueError) as e:
                call()
            assert all(wd in str(e.value) for wd in words), (rotate, str(e.value))


# ------------------------------------------------------------------------------------------ the restatements by hand
def test_upright_view_is_the_statements_index_map():
    rng = np.random.default_rng(0)
    F = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    h, w = F.shape[:2]
    U = {rot: upright(F, rot) for rot in ROTS}
    assert U[0].shape == U[180].shape == (5, 7, 3) and U[90].shape == U[270].shape == (7, 5, 3)
    for y in range(7):
        for x in range(5):
            assert (U[90][y, x] == F[h - 1 - x, y]).all() and (U[270][y, x] == F[x, w - 1 - y]).all()
    for y in range(5):
        for x in range(7):
            assert (U[0][y, x] == F[y, x]).all() and (U[180][y, x] == F[h - 1 - y, w - 1 - x]).all()
    # a frame that keeps its size is reproduced turned; the stretch has no padding
    c = rot_ref(F, 90, 16, 12, 0, anchor="topleft", upscale=False, fill=(1, 2, 3))
    assert np.array_equal(c[:7, :5], U[90]) and (c[7:] == np.uint8([1, 2, 3])).all() and (c[:, 5:] == np.uint8([1, 2, 3])).all()
    assert rot_ref(F, 270, 7, 5, 1).tobytes() == U[270].tobytes()


def test_unrot_ref_by_hand():
    # a stored 40 x 120 frame, rot 90: the upright view is 120 x 40; in 64 x 96 it takes rw 21, rh 64, dx 37: scale 40/21, 120/64
    hw, geom = (40, 120), (21, 64, 37, 0)
    assert rot_geometry_ref(40, 120, 64, 96, 90, 0) == geom
    d = np.float32([[(37, 0, 58, 64), (40, 8, 44, 16), (58, 8, 60, 16), (44, 16, 40, 8)]])        # the content; a box; cx = 59 dropped; inverted
    l = np.float32([[np.tile([37.0, 0.0], 5)] * 4])
    out, flags = unrot_ref(geom, hw, 90, d, np.float32([[0.9, 0.8, 0.7, 0.6]]), l, [4])
    dets, lms = out[0]
    assert flags.tolist() == [0] and dets[:, 4].tolist() == [np.float32(0.9), np.float32(0.8), np.float32(0.6)]
    # X = uy(y), Y = (h-1) - ux(x): the content's corners (37, 0) -> (0, 39), (58, 64) -> (120, -1); X1 from y1, Y1 from x2
    assert dets[0, :4].tolist() == [0.0, -1.0, 120.0, 39.0]
    sx, sy = 40.0 / 21.0, 120.0 / 64.0
    assert dets[1, :4].tolist() == [np.float32(8 * sy), np.float32(39 - 7 * sx), np.float32(16 * sy), np.float32(39 - 3 * sx)]
    assert dets[2, 0] > dets[2, 2] and dets[2, 1] > dets[2, 3]                   # an inverted box stays inverted: no min / max
    assert lms[0].tolist() == [0.0, 39.0] * 5                                    # the canvas content's origin is the stored frame's bottom-left
    # rot 180 and 270 of the same point; rot 0 is the fit's map
    for rot, g, want in ((180, (96, 32, 0, 16), (119.0, 39.0)), (270, geom, (119.0, 0.0)), (0, (96, 32, 0, 16), (0.0, 0.0))):
        x0, y0 = g[2], g[3]
        o, _ = unrot_ref(g, hw, rot, np.float32([[(x0, y0, x0 + 2, y0 + 2)]]), np.ones((1, 1), np.float32), np.float32([[np.tile([x0, y0], 5)]]), [1])
        assert o[0][1][0, :2].tolist() == list(want), rot
    # a signed zero survives the assignment
    o, _ = unrot_ref((96, 32, 0, 16), hw, 0, np.float32([[(-0.0, 16, 4, 20)]]), np.ones((1, 1), np.float32), np.zeros((1, 1, 10), np.float32), [1])
    assert np.signbit(o[0][0][0, 0])
    # count > rows sets the flag; a count of 0 gives nothing
    o, flags = unrot_ref(geom, hw, 90, np.concatenate([d, d]), np.ones((2, 4), np.float32), np.zeros((2, 4, 10), np.float32), [9, 0])
    assert flags.tolist() == [1, 0] and [len(x) for x, _ in o] == [3, 0]


# ------------------------------------------------------------------------------------------ the documents
def test_documents_state_the_scope_of_rotated_sources():
    for name in ("README.md", "INTEGRATION.md", os.path.join("include", "centerface_hip.h")):
        text = re.sub(r"\s+", " ", open(os.path.join(REPO, name)).read())
        near = [m.start() for m in re.finditer(r"cf_forward_rot", text)]
        assert near, name
        assert any("no accuracy claim" in text[max(0, p - 2500):p + 2500].lower() for p in near), name
    text = re.sub(r"\s+", " ", open(os.path.join(REPO, "README.md")).read()).lower()
    for word in ("mirrored", "per frame", "tiled", "probing", "labels"):
        assert word in text, word
