"""Aspect-preserving input (cf_fit_geometry, cf_forward_fit, cf_unfit_rows, cf_op_fit, cf_op_unfit): what can be checked without a GPU --
the declarations, the host-only geometry against the Python-integer restatement of tests/fit_cases.py, the refusals that come before
any device work, the restated row mapping by hand, and the words the documents owe.

A refusal that needs a context (B > max_batch, the state rules) is in tests/test_fit.py: a context cannot be created without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
import csrc_text
from fit_cases import WORKED, fit_geometry_ref, fit_ref, unfit_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = cfa._lib
SYMBOLS = ("cf_fit_geometry", "cf_forward_fit", "cf_unfit_rows", "cf_op_fit", "cf_op_unfit")


# ------------------------------------------------------------------------------------------ the declarations
def test_fit_symbols_constants_and_structs_match_the_header():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), sym
        assert sym in L.EXPORTS and hasattr(lib, sym)
        assert getattr(lib, sym).argtypes is not None, sym
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(CF_FIT_[A-Z0-9_]+)\s+(\d+)", text)}
    assert consts == {"CF_FIT_CENTER": 0, "CF_FIT_TOPLEFT": 1}
    assert (L.CF_FIT_CENTER, L.CF_FIT_TOPLEFT) == (0, 1) and L.FIT_ANCHORS["center"] == 0 and L.FIT_ANCHORS["topleft"] == 1
    types = {"int32_t": C.c_int32}
    for name, cls in (("cf_fit_opts", L.FitOpts), ("cf_fit_geom", L.FitGeom)):
        body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), code, flags=re.S).group(1)
        fields = []
        for ty, names in re.findall(r"(\w+)\s+([\w\s,\[\]]+);", body):
            for n in names.split(","):
                n = n.strip()
                fields.append((n[:-3], C.c_uint8 * 4) if n.endswith("[4]") and ty == "uint8_t" else (n, types[ty]))
        assert list(cls._fields_) == fields, (name, fields)
    assert C.sizeof(L.FitOpts) == 12 and C.sizeof(L.FitGeom) == 16
    # the other option structs kept their sizes, the version and the format integers stayed
    sizes = {L.TrackOpts: 20, L.FollowOpts: 8, L.RedactOpts: 20, L.BestShotOpts: 16, L.SceneOpts: 8, L.TileRect: 16, L.MergeOpts: 12}
    assert {k.__name__: C.sizeof(k) for k in sizes} == {k.__name__: v for k, v in sizes.items()}
    assert lib.cf_version() == 100
    assert (L.CF_YUV_NV12, L.CF_YUV_NV21, L.CF_YUV_I420, L.CF_YUV_YV12, L.CF_FRAME_BGR) == (0, 1, 2, 3, 4)
    o = L.fit_opts()
    assert (o.anchor, o.upscale, list(o.fill)) == (0, 1, [0, 0, 0, 0])
    o = L.fit_opts("topleft", False, (1, 2, 3))
    assert (o.anchor, o.upscale, list(o.fill)) == (1, 0, [1, 2, 3, 0])
    for bad in (dict(anchor="middle"), dict(fill=(1, 2)), dict(fill=(1, 2, 256))):
        with pytest.raises(ValueError):
            L.fit_opts(**bad)
    # the fit includes the one statement of the resize and of the conversion, and is built without FMA contraction (so is the map)
    # (the statements are in the shared headers cf_fit.hip includes: required of the union, refused in every file of it)
    texts = csrc_text.unit("cf_fit.hip")
    assert '#include "cf_cutpx.h"' in texts["cf_fit.hip"] and '#include "cf_collect.h"' in texts["cf_fit.hip"]
    csrc_text.assert_one_statement(texts, ('#include "cf_cvresize.h"', '#include "cf_yuvmath.h"', "cv_linear_coeffs(", "cv_linear_vpass(", "yuv_px("))
    mk = open(os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "cf_fit.hip" in srcs and re.search(r"EXTRA_cf_fit\s*=\s*-ffp-contract=off", mk)


# ------------------------------------------------------------------------------------------ the geometry
def _geometry(h, w, H, W, anchor=0, upscale=1, null=None):
    o = L.FitOpts(anchor, upscale, (C.c_uint8 * 4)(0, 0, 0, 0))
    g = L.FitGeom(-7, -7, -7, -7)
    code = L.lib().cf_fit_geometry(None if null == "o" else C.byref(o), h, w, H, W, None if null == "g" else C.byref(g))
    return code, (g.rw, g.rh, g.dx, g.dy)


def test_fit_geometry_equals_the_restatement():
    for (h, w), (H, W), up, want in WORKED:
        assert fit_geometry_ref(h, w, H, W, "center", bool(up)) == want
        assert _geometry(h, w, H, W, 0, up) == (0, want)
        assert ops.fit_geometry(h, w, H, W, "center", bool(up)) == want
        assert _geometry(h, w, H, W, 1, up) == (0, want[:2] + (0, 0))
    cases = [(h, w, H, W) for h in range(2, 41) for w in range(2, 41) for H, W in ((32, 64), (64, 32), (64, 64))]
    cases += [(8192, 2, H, W) for H, W in ((32, 64), (64, 32), (640, 640))] + [(2, 8192, H, W) for H, W in ((32, 64), (64, 32), (640, 640))]
    cases += [(8192, 8192, 640, 640), (8190, 8192, 8192, 8192), (1080, 1920, 640, 640), (2160, 3840, 32, 32)]
    for h, w, H, W in cases:
        for anchor in (0, 1):
            for up in (0, 1):
                want = fit_geometry_ref(h, w, H, W, anchor, bool(up))
                assert _geometry(h, w, H, W, anchor, up) == (0, want), (h, w, H, W, anchor, up)
                rw, rh, dx, dy = want
                assert 1 <= rw <= W and 1 <= rh <= H and 0 <= dx <= W - rw and 0 <= dy <= H - rh
                if up or h > H or w > W:
                    assert rw == W or rh == H, (h, w, H, W, up, want)
                else:
                    assert (rw, rh) == (w, h)
                assert (dx, dy) == (((W - rw) // 2, (H - rh) // 2) if anchor == 0 else (0, 0))
    # the extreme shapes keep at least one pixel
    assert fit_geometry_ref(8192, 2, 64, 64) == (1, 64, 31, 0) and fit_geometry_ref(2, 8192, 64, 64) == (64, 1, 0, 31)


def test_fit_geometry_refuses_bad_values_and_writes_nothing():
    for kw in (dict(anchor=2), dict(anchor=-1), dict(upscale=2), dict(upscale=-1), dict(h=1), dict(w=1), dict(h=8193), dict(w=8193), dict(H=0), dict(W=0),
               dict(null="o"), dict(null="g")):
        a = dict(h=8, w=12, H=32, W=32)
        a.update(kw)
        code, g = _geometry(**a)
        assert code == -1 and g == (-7, -7, -7, -7), kw
        assert b"cf_fit_geometry" in L.lib().cf_op_last_error(), kw
    assert _geometry(8, 12, 32, 32, anchor=5)[0] == -1 and b"anchor 5" in L.lib().cf_op_last_error()           # the value is named
    assert _geometry(8, 12, 32, 32, upscale=3)[0] == -1 and b"upscale=3" in L.lib().cf_op_last_error()
    assert _geometry(8, 8193, 32, 32)[0] == -1 and b"w=8193" in L.lib().cf_op_last_error()
    assert _geometry(33, 99, 32, 32) == (0, (32, 11, 0, 10))                                                   # odd sides are fine
    with pytest.raises(ValueError):
        ops.fit_geometry(8, 12, 32, 32, anchor="middle")
    with pytest.raises(ValueError):
        ops.fit_geometry(1, 12, 32, 32)


# ------------------------------------------------------------------------------------------ refusals before any device work
POISON = 0xA5


def _frames(fmt, planes=(True, True, True)):
    buf = np.zeros(3 * 4096, np.uint8)
    tab = (L.YuvPlanes * 1)()
    tab[0].y, tab[0].c0, tab[0].c1 = [(buf.ctypes.data + 4096 * k) if on else None for k, on in enumerate(planes)]
    return tab, buf


def _pitches(fmt, w, pitch0, pitch1):
    bgr, il = fmt == L.CF_FRAME_BGR, fmt in (L.CF_YUV_NV12, L.CF_YUV_NV21)
    return (3 * w if bgr else w) if pitch0 is None else pitch0, (0 if bgr else w if il else w // 2) if pitch1 is None else pitch1


def _op_fit(fmt=L.CF_FRAME_BGR, B=1, h=8, w=12, pitch0=None, pitch1=None, H=4, W=8, planes=(True, True, True), out=True, anchor=0, upscale=1, opts=True,
            table=True):
    tab, buf = _frames(fmt, planes)
    pitch0, pitch1 = _pitches(fmt, w, pitch0, pitch1)
    o = L.FitOpts(anchor, upscale, (C.c_uint8 * 4)(0, 0, 0, 0))
    canvas = np.full((max(B, 1), max(H, 1), max(W, 1), 3), POISON, np.uint8)
    code = L.lib().cf_op_fit(0, C.byref(o) if opts else None, fmt, tab if table else None, B, h, w, pitch0, pitch1, H, W, L.ptr(canvas) if out else None)
    return code, bool((canvas == POISON).all())


def _forward_fit(fmt=L.CF_FRAME_BGR, B=1, h=8, w=12, pitch0=None, pitch1=None, planes=(True, True, True), anchor=0, upscale=1, opts=True, table=True,
                 on_device=0, shift=0):
    tab, buf = _frames(fmt, planes)
    if shift:
        tab[0].y = tab[0].y + shift
    pitch0, pitch1 = _pitches(fmt, w, pitch0, pitch1)
    o = L.FitOpts(anchor, upscale, (C.c_uint8 * 4)(0, 0, 0, 0))
    return L.lib().cf_forward_fit(None, C.byref(o) if opts else None, fmt, tab if table else None, on_device, B, h, w, pitch0, pitch1)


FRAME_REFUSALS = [
    dict(fmt=-1), dict(fmt=5), dict(B=0), dict(B=-3), dict(h=1), dict(w=1), dict(h=8194), dict(w=8194), dict(h=0),
    dict(fmt=L.CF_YUV_NV12, h=7), dict(fmt=L.CF_YUV_I420, w=11), dict(pitch0=35), dict(fmt=L.CF_YUV_NV12, pitch0=11),
    dict(fmt=L.CF_YUV_NV21, pitch1=11), dict(fmt=L.CF_YUV_I420, pitch1=5), dict(fmt=L.CF_YUV_YV12, pitch1=5),
    dict(planes=(False, True, True)), dict(fmt=L.CF_YUV_NV12, planes=(True, False, True)), dict(fmt=L.CF_YUV_I420, planes=(True, True, False)),
    dict(anchor=2), dict(anchor=-1), dict(upscale=2), dict(upscale=-1), dict(opts=False), dict(table=False),
]


def test_fit_entry_points_refuse_bad_arguments_before_any_device_work():
    lib = L.lib()
    for kw in FRAME_REFUSALS + [dict(W=6), dict(W=0), dict(H=0), dict(out=False)]:
        code, untouched = _op_fit(**kw)
        assert code == -1 and untouched, kw
        assert b"cf_op_fit" in lib.cf_op_last_error() and b"null context" not in lib.cf_op_last_error(), kw
    assert _op_fit(anchor=7)[0] == -1 and b"anchor 7" in lib.cf_op_last_error()                    # the value is named
    assert _op_fit(w=8194)[0] == -1 and b"w=8194" in lib.cf_op_last_error()
    assert _op_fit(pitch0=35)[0] == -1 and b"pitch0=35" in lib.cf_op_last_error()
    # fine arguments get as far as the device (none here: CF_EHIP) or succeed: BGR frames may have odd sides
    for kw in (dict(), dict(h=7, w=11), dict(fmt=L.CF_YUV_YV12), dict(pitch0=50), dict(anchor=1, upscale=0)):
        assert _op_fit(**kw)[0] != -1, kw
    # cf_forward_fit without a context: every refusal is reported before "null context"
    for kw in FRAME_REFUSALS + [dict(on_device=1, shift=2), dict(on_device=1, pitch0=38), dict(fmt=L.CF_YUV_NV12, on_device=1, pitch1=14)]:
        assert _forward_fit(**kw) == -1, kw
        assert b"cf_forward_fit" in lib.cf_op_last_error() and b"null context" not in lib.cf_op_last_error(), kw
    assert _forward_fit() == -1 and b"cf_forward_fit: null context" in lib.cf_op_last_error()
    assert _forward_fit(h=7, w=11) == -1 and b"null context" in lib.cf_op_last_error()
    assert _forward_fit(on_device=1) == -1 and b"null context" in lib.cf_op_last_error()
    # cf_unfit_rows
    d = np.full((1, 4, 5), POISON, np.float32)
    assert lib.cf_unfit_rows(None, 0, L.ptr(d), None, None, None, 0) == -1
    assert b"cf_unfit_rows" in lib.cf_op_last_error() and b"max_out" in lib.cf_op_last_error() and b"null context" not in lib.cf_op_last_error()
    assert lib.cf_unfit_rows(None, 4, L.ptr(d), None, None, None, 0) == -1 and b"cf_unfit_rows: null context" in lib.cf_op_last_error()
    assert (d == np.float32(POISON)).all()

    def unfit(B=1, h=8, w=12, H=32, W=32, rows=2, max_out=4, null=None, anchor=0, upscale=1):
        a = {k: np.zeros(s, np.float32) for k, s in (("d", (max(B, 1), max(rows, 1), 4)), ("s", (max(B, 1), max(rows, 1))), ("l", (max(B, 1), max(rows, 1), 10)))}
        od, ol = np.full((max(B, 1), max(max_out, 1), 5), 7.5, np.float32), np.full((max(B, 1), max(max_out, 1), 10), 7.5, np.float32)
        cn, oc, fl = np.zeros(max(B, 1), np.int32), np.full(max(B, 1), -9, np.int32), np.full(max(B, 1), -9, np.int32)
        o = L.FitOpts(anchor, upscale, (C.c_uint8 * 4)(0, 0, 0, 0))
        p = {k: (None if k == null else L.ptr(v)) for k, v in dict(a, cn=cn, od=od, ol=ol, oc=oc, fl=fl).items()}
        code = lib.cf_op_unfit(0, None if null == "o" else C.byref(o), B, h, w, H, W, p["d"], p["s"], p["l"], p["cn"], rows, max_out, p["od"], p["ol"],
                               p["oc"], p["fl"])
        return code, bool((od == 7.5).all() and (ol == 7.5).all() and (oc == -9).all() and (fl == -9).all())
    for kw in (dict(anchor=2), dict(upscale=-1), dict(B=0), dict(rows=0), dict(max_out=0), dict(h=1), dict(w=8193), dict(H=0), dict(W=0), dict(null="o"),
               dict(null="d"), dict(null="s"), dict(null="l"), dict(null="cn"), dict(null="od"), dict(null="ol"), dict(null="oc"), dict(null="fl")):
        code, untouched = unfit(**kw)
        assert code == -1 and untouched, kw
        assert b"cf_op_unfit" in lib.cf_op_last_error(), kw
    assert unfit()[0] != -1 and unfit(h=7, w=11)[0] != -1


def test_python_wrappers_refuse_what_they_can_see():
    img = np.zeros((1, 8, 12, 3), np.uint8)
    with pytest.raises(ValueError):
        ops.fit_frames(img[:, :, ::2], (4, 8))                           # rows not contiguous
    with pytest.raises(ValueError):
        ops.fit_frames(img, (4, 8), fmt="rgb")
    with pytest.raises(ValueError):
        ops.fit_frames(img, (4, 6))                                      # the library's refusal is a ValueError too
    with pytest.raises(ValueError):
        ops.fit_frames(img, (4, 8), anchor="middle")
    with pytest.raises(ValueError):
        ops.unfit_rows((8, 12), (32, 32), np.zeros((1, 2, 3)), np.zeros((1, 2)), np.zeros((1, 2, 10)), [0], 4)
    # fit= together with tiled=True is refused by every product path before any engine exists
    face = cfa.CenterFace.__new__(cfa.CenterFace)
    assert face._fit_options(None) is None and face._fit_options(False, True) is None
    assert face._fit_options(True) == {} and face._fit_options(dict(anchor="topleft", fill=(1, 2, 3))) == dict(anchor="topleft", fill=(1, 2, 3))
    for bad in (dict(cell=4), dict(anchor="middle"), dict(fill=(1, 2))):
        with pytest.raises(ValueError):
            face._fit_options(bad)
    frames, yuv = np.zeros((1, 8, 12, 3), np.uint8), np.zeros((1, 12, 12), np.uint8)
    for call in (lambda: face.anonymize(frames, fit=True, tiled=True), lambda: face.anonymize_yuv(yuv, fit=True, tiled=True),
                 lambda: face.annotate(frames, fit=True, tiled=True), lambda: face.annotate_yuv(yuv, fit={"anchor": "topleft"}, tiled=True),
                 lambda: face.best_shots(frames, tracker=object(), shots=object(), fit=True, tiled=True),
                 lambda: face.detect_aligned_frames(frames, fit=True, tiled=True)):
        with pytest.raises(ValueError) as e:
            call()
        assert "fit" in str(e.value) and "tiled" in str(e.value)


# ------------------------------------------------------------------------------------------ the restatements by hand
def test_fit_ref_by_hand():
    rng = np.random.default_rng(0)
    # a frame that keeps its size is reproduced byte for byte at (dx, dy), the fill is everywhere else
    img = rng.integers(0, 256, (30, 50, 3), dtype=np.uint8)
    c = fit_ref(img, 64, 96, "center", False, (1, 2, 3))
    assert np.array_equal(c[17:47, 23:73], img)
    mask = np.ones((64, 96), bool)
    mask[17:47, 23:73] = False
    assert (c[mask] == np.uint8([1, 2, 3])).all()
    assert np.array_equal(fit_ref(img, 64, 96, "topleft", False)[:30, :50], img)
    # a flat frame stays flat inside the content whatever the scale
    flat = np.full((120, 40, 3), 77, np.uint8)
    c = fit_ref(flat, 64, 96)
    assert (c[:, 37:58] == 77).all() and (c[:, :37] == 0).all() and (c[:, 58:] == 0).all()


def test_unfit_ref_by_hand():
    geom, hw = (96, 32, 0, 16), (40, 120)                                 # 40 x 120 in 64 x 96: scale 1.25 both ways
    l0 = np.arange(10, dtype=np.float32) + 20
    rows = [
        (10, 20, 30, 30, 0.9),                 # centre (20, 25): kept
        (10, 10, 30, 22, 0.8),                 # cy = 16 = dy: kept
        (10, 30, 30, 66, 0.7),                 # cy = 48 = dy + rh: dropped
        (np.nan, 20, 30, 30, 0.6),             # a NaN corner: dropped
        (10, 20, np.inf, 30, 0.5),             # an infinite corner: dropped
        (10, 0, 30, 31.5, 0.4),                # cy = 15.75 < dy: dropped
        (-20, 20, 20, 30, 0.3),                # cx = 0 = dx: kept, the corner goes negative (no clamping)
    ]
    d = np.float32([[r[:4] for r in rows]])
    s = np.float32([[r[4] for r in rows]])
    l = np.tile(l0, (1, len(rows), 1))
    out, flags = unfit_ref(geom, hw, d, s, l, [len(rows)])
    dets, lms = out[0]
    assert flags.tolist() == [0] and dets[:, 4].tolist() == [np.float32(0.9), np.float32(0.8), np.float32(0.3)]
    assert dets[0, :4].tolist() == [12.5, 5.0, 37.5, 17.5] and dets[1, :4].tolist() == [12.5, -7.5, 37.5, 7.5]
    assert dets[2, :4].tolist() == [-25.0, 5.0, 25.0, 17.5]
    assert lms[0].tolist() == [(v - (16 if k & 1 else 0)) * 1.25 for k, v in enumerate(l0.tolist())]
    # x edges with a horizontal offset: 120 x 40 in 64 x 96 has dx 37, rw 21
    geom, hw = (21, 64, 37, 0), (120, 40)
    d = np.float32([[(36, 10, 38, 20), (57, 10, 59, 20), (56, 10, 59.5, 20), (36, 10, 37.5, 20)]])       # cx = 37 kept, 58 dropped, 57.75 kept, 36.75 dropped
    out, flags = unfit_ref(geom, hw, d, np.ones((1, 4), np.float32), np.zeros((1, 4, 10), np.float32), [4])
    assert len(out[0][0]) == 2 and out[0][0][0, 0] == np.float32((36.0 - 37.0) * (40.0 / 21.0))
    # count > rows sets the flag and only the rows written are seen; a count of 0 gives nothing
    out, flags = unfit_ref(geom, hw, np.concatenate([d, d]), np.ones((2, 4), np.float32), np.zeros((2, 4, 10), np.float32), [9, 0])
    assert flags.tolist() == [1, 0] and [len(x) for x, _ in out] == [2, 0] and out[1][0].shape == (0, 5) and out[1][1].shape == (0, 10)


# ------------------------------------------------------------------------------------------ the documents
def test_documents_make_no_accuracy_claim_for_the_fit():
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("include", "centerface_hip.h")):
        text = re.sub(r"\s+", " ", open(os.path.join(REPO, name)).read())
        near = [m.start() for m in re.finditer(r"cf_forward_fit", text)]
        assert near, name
        assert any("no accuracy claim" in text[max(0, p - 1500):p + 1500].lower() for p in near), name
        assert "dataset/dataset.py:114-134" in text, name
