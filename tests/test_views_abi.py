"""Multi-scale detection (cf_view_layout, cf_forward_views, cf_merge_views, cf_op_views, cf_op_merge_views): what can be checked without
a GPU -- the declarations, the host-only layout against the Python-integer restatement of tests/view_cases.py, the refusals that come
before any device work (with no context at all), the product paths' ValueErrors, the one statement of the resize and the conversion,
and the words the documents owe.

A refusal that needs a context (Bf * V > max_batch, a content outside ITS canvas) is in tests/test_views.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
import csrc_text
from view_cases import WORKED, view_layout_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc")
L = cfa._lib
SYMBOLS = ("cf_view_layout", "cf_forward_views", "cf_merge_views", "cf_op_views", "cf_op_merge_views")


def _header():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


# ------------------------------------------------------------------------------------------ the declarations
def test_view_symbols_and_structs_match_the_header():
    text, code = _header()
    lib = L.lib()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), sym
        assert sym in L.EXPORTS and hasattr(lib, sym)
        assert getattr(lib, sym).argtypes is not None, sym
    for name, cls in (("cf_view", L.View), ("cf_view_opts", L.ViewOpts)):
        body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), code, flags=re.S).group(1)
        fields = []
        for ty, names in re.findall(r"(\w+)\s+([\w\s,\[\]]+);", body):
            assert ty == "int32_t", (name, ty)
            for n in names.split(","):
                m = re.fullmatch(r"(\w+)\[(\d+)\]", n.strip())
                fields.append((m.group(1), C.c_int32 * int(m.group(2))) if m else (n.strip(), C.c_int32))
        assert list(cls._fields_) == fields, (name, fields)
    assert C.sizeof(L.View) == 32 and C.sizeof(L.ViewOpts) == 52
    assert "/* 32 bytes */" in text and "/* 52 bytes */" in text
    # nothing else moved
    assert lib.cf_version() == 100
    assert [C.sizeof(c) for c in (L.TileRect, L.MergeOpts, L.FitOpts, L.FitGeom, L.RotOpts)] == [16, 12, 12, 16, 20]
    o = L.view_opts()
    assert (o.tile_h, o.tile_w, o.overlap, o.anchor, o.n_levels, list(o.scale_pm)) == (0, 0, 0, 0, 1, [1000, 0, 0, 0, 0, 0, 0, 0])
    o = L.view_opts(tile=(64, 32), scales=(1.0, 0.5, 0.2504), anchor="topleft")
    assert (o.tile_h, o.tile_w, o.overlap, o.anchor, o.n_levels, list(o.scale_pm)[:3]) == (64, 32, 6, 1, 3, [1000, 500, 250])
    assert L.view_opts(tile=640, overlap=128).overlap == 128
    for bad in (dict(anchor="middle"), dict(scales=(1.001,)), dict(scales=(0.0004,)), dict(scales=(0.0,)), dict(scales=(-0.5,)), dict(scales=(0.5,) * 9)):
        with pytest.raises(ValueError):
            L.view_opts(**bad)
    with pytest.raises(ValueError):
        L.fill_bytes((1, 2))
    with pytest.raises(ValueError):
        L.fill_bytes((1, 2, 256))


def test_the_cutter_holds_one_statement_of_resize_and_conversion_and_no_atomic():
    # (through the cutters' shared header: required of the union, refused in every file of it)
    texts = csrc_text.unit("cf_views.hip")
    src = texts["cf_views.hip"]
    assert '#include "cf_cutpx.h"' in src
    csrc_text.assert_one_statement(texts, ('#include "cf_cvresize.h"', '#include "cf_yuvmath.h"', "cv_linear_coeffs(", "cv_linear_vpass(", "yuv_px("))
    assert all("2048" not in text for text in texts.values())
    # the views' rows go through the one collect kernel and the one launch of the NMS stages, which live with the tile merge
    merge = csrc_text.unit("cf_tiles.hip")
    csrc_text.assert_one_statement(merge, ("collect_rows_kernel<ViewItems, 0>", "struct ViewItems", "launch_nms_stages("))
    assert "cut_views_kernel" in src and "launch_nms_stages(" not in src
    # the tile cutter and the fit kernel were not edited into it: they still stand where they stood
    assert "cut_tiles_kernel" in open(os.path.join(CSRC, "cf_tiles.hip")).read() and "fit_frames_kernel" in open(os.path.join(CSRC, "cf_fit.hip")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bcf_views\.hip\b", mk, flags=re.M) and re.search(r"EXTRA_cf_views\s*=\s*-ffp-contract=off", mk)


def test_the_documents_state_the_limits():
    header = _header()[0]
    section = header[header.index("multi-scale detection"):header.index("face tracks across video frames")]
    docs = {"header": section, "README.md": open(os.path.join(REPO, "README.md")).read(), "DESIGN.md": open(os.path.join(REPO, "DESIGN.md")).read()}
    for name, text in docs.items():
        flat = re.sub(r"[\s*]+", " ", text.lower())
        assert "cf_forward_views" in text or "detect_views" in text, name
        for word in ("packing", "rotated", "no accuracy claim"):
            assert word in flat, (name, word)
    # the timing file holds the probe's table, or says plainly that there is none
    prof = open(os.path.join(REPO, "profiles", "views.md")).read()
    assert "view_probe.py" in prof and ("not measured" in prof.lower() or re.search(r"^\|.*views cutter.*\|\s*\d", prof, flags=re.M))


# ------------------------------------------------------------------------------------------ the layout
UNTOUCHED = (-101058055,) * 8                            # 0xF9F9F9F9
ROOM = 512


def _layout(h, w, H, W, tile_h=0, tile_w=0, overlap=0, anchor=0, pm=(1000,), cap=None, n_levels=None):
    o = L.ViewOpts(tile_h, tile_w, overlap, anchor, len(pm) if n_levels is None else n_levels, (C.c_int32 * 8)(*(list(pm) + [0] * 8)[:8]))
    n = C.c_int(-1)
    room = ROOM if cap is None else cap
    tab = (L.View * (max(room, 1) + 2))()
    C.memset(tab, 0xF9, C.sizeof(tab))
    code = L.lib().cf_view_layout(C.byref(o), h, w, H, W, tab, room, C.byref(n))
    a = np.frombuffer(tab, np.int32).reshape(-1, 8)
    return code, n.value, [tuple(r) for r in a[:min(max(n.value, 0), room) + 2].tolist()]


SIZES = [(1080, 1920), (1920, 1080), (70, 94), (72, 96), (20, 30), (2, 8192), (8192, 2), (2, 2), (640, 640), (8192, 8192)]
CANVASES = [(640, 640), (32, 64), (64, 32), (4, 8)]
LEVELS = [(), (1000,), (500,), (1000, 500), (1000, 500, 250), (1, 1000), (999, 501, 499, 333, 250, 125, 63, 2)]


def test_view_layout_worked_example_by_hand():
    assert view_layout_ref(1080, 1920, 640, 640, 640, 640, 128, "center", (1000, 500)) == WORKED
    code, n, got = _layout(1080, 1920, 640, 640, 640, 640, 128, 0, (1000, 500))
    assert code == 0 and n == 10 and got[:10] == WORKED and got[10] == UNTOUCHED
    assert ops.view_layout(1080, 1920, 640, 640, tile=640, overlap=128, scales=(1.0, 0.5)).tolist() == [list(v) for v in WORKED]
    # top-left anchoring moves only the levels; a portrait frame is width-limited the other way round
    assert ops.view_layout(1080, 1920, 640, 640, scales=(1.0, 0.5), anchor="topleft").tolist() == [[0, 0, 1920, 1080, 0, 0, 640, 360], [0, 0, 1920, 1080, 0, 0, 320, 180]]
    assert ops.view_layout(1920, 1080, 640, 640, scales=(0.25,)).tolist() == [[0, 0, 1080, 1920, 275, 240, 90, 160]]
    # a 2 x 8192 frame is fitted to one canvas row, and a small level to one pixel
    assert ops.view_layout(2, 8192, 32, 64, scales=(1.0, 0.01)).tolist() == [[0, 0, 8192, 2, 0, 15, 64, 1], [0, 0, 8192, 2, 31, 15, 1, 1]]


def test_view_layout_equals_the_restatement():
    count = 0
    for h, w in SIZES:
        for H, W in CANVASES:
            for anchor in (0, 1):
                for pm in LEVELS:
                    for th, tw, ov in ((0, 0, 0), (0, 0, 7), (32, 64, 8), (640, 640, 128), (16, 16, 0)):
                        if (th, h * w, anchor) == (16, 8192 * 8192, 1) or (th, h * w) == (16, 8192 * 8192) and len(pm) > 1:
                            continue                                          # (262144 tiles: once per level count is enough)
                        want = view_layout_ref(h, w, H, W, th, tw, ov, anchor, pm)
                        code, n, got = _layout(h, w, H, W, th, tw, ov, anchor, pm)
                        if want is None:
                            assert code == -1 and n == -1 and got[0] == UNTOUCHED, (h, w, H, W, anchor, pm, th, tw, ov)
                            assert b"cf_view_layout" in L.lib().cf_op_last_error()
                            continue
                        count += 1
                        m = min(len(want), ROOM)                                  # (16 x 16 tiles of 8192 x 8192: only the first ROOM are written)
                        assert code == 0 and n == len(want) and got[:m] == want[:m], (h, w, H, W, anchor, pm, th, tw, ov, got[:m][:12], want[:12])
                        assert len(want) >= ROOM or got[n] == UNTOUCHED
                        for sx0, sy0, sw, sh, dx, dy, dw, dh in want:              # every view is one cf_forward_views takes in this canvas
                            assert not ((sx0 | sy0 | sw | sh) & 1) and sw >= 2 and sh >= 2 and 0 <= sx0 <= w - sw and 0 <= sy0 <= h - sh
                            assert dw >= 1 and dh >= 1 and 0 <= dx <= W - dw and 0 <= dy <= H - dh
    assert count > 1500
    # the aspect extremes drive dw or dh to 1
    assert view_layout_ref(8192, 2, 32, 64, scales_pm=(1000, 500))[0][6:] == (1, 32)
    assert view_layout_ref(2, 8192, 32, 64, scales_pm=(1,))[0][4:] == (31, 15, 1, 1)


def test_view_layout_writes_only_cap_views_and_refuses_bad_values():
    code, n, got = _layout(1080, 1920, 640, 640, 640, 640, 128, 0, (1000, 500), cap=3)
    assert code == 0 and n == 10 and got[:3] == WORKED[:3] and got[3] == UNTOUCHED
    o = L.view_opts(tile=640, overlap=128, scales=(1.0, 0.5))
    n = C.c_int(-1)
    assert L.lib().cf_view_layout(C.byref(o), 1080, 1920, 640, 640, None, 0, C.byref(n)) == 0 and n.value == 10
    tab = (L.View * 4)()
    assert L.lib().cf_view_layout(C.byref(o), 1080, 1920, 640, 640, tab, 4, None) == -1
    assert L.lib().cf_view_layout(None, 1080, 1920, 640, 640, tab, 4, C.byref(n)) == -1
    assert L.lib().cf_view_layout(C.byref(o), 1080, 1920, 640, 640, None, 4, C.byref(n)) == -1
    bad = [dict(anchor=2), dict(anchor=-1), dict(n_levels=9), dict(n_levels=-1), dict(pm=(0,)), dict(pm=(1001,)), dict(pm=(1000, -5)),
           dict(pm=()),                                                       # no tiles, no levels: empty
           dict(pm=(), tile_h=4096, tile_w=4096),                             # one tile is not a tile view: empty as well
           dict(h=1), dict(w=0), dict(h=8194), dict(H=0), dict(W=0),
           dict(tile_h=640), dict(tile_w=640), dict(tile_h=641, tile_w=640), dict(tile_h=640, tile_w=640, overlap=640), dict(tile_h=640, tile_w=640, overlap=3),
           dict(h=1081, tile_h=640, tile_w=640)]                               # what cf_tile_grid refuses
    for kw in bad:
        a = dict(h=1080, w=1920, H=640, W=640)
        a.update(kw)
        assert _layout(**a)[0] == -1, kw
        assert b"cf_view_layout" in L.lib().cf_op_last_error(), kw
    assert _layout(1081, 1921, 640, 640)[0] == 0                              # odd sides without tiles: as cf_fit_geometry takes them
    for kw in (dict(scales=(1.5,)), dict(scales=(0.0,)), dict(anchor="middle"), dict(tile=641), dict(scales=())):
        with pytest.raises(ValueError):
            ops.view_layout(1080, 1920, 640, 640, **kw)


# ------------------------------------------------------------------------------------------ refusals before any device work
GOOD = (0, 0, 4, 4, 0, 0, 8, 4)


def _frames(fmt, planes=(True, True, True)):
    buf = np.zeros(3 * 4096, np.uint8)
    tab = (L.YuvPlanes * 1)()
    tab[0].y, tab[0].c0, tab[0].c1 = [(buf.ctypes.data + 4096 * k) if on else None for k, on in enumerate(planes)]
    return tab, buf


def _args(fmt=L.CF_FRAME_BGR, Bf=1, h=8, w=12, pitch0=None, pitch1=None, views=(GOOD,), planes=(True, True, True), fill=True, V=None):
    bgr, il = fmt == L.CF_FRAME_BGR, fmt in (L.CF_YUV_NV12, L.CF_YUV_NV21)
    tab, keep = _frames(fmt, planes)
    pitch0 = (3 * w if bgr else w) if pitch0 is None else pitch0
    pitch1 = (0 if bgr else w if il else w // 2) if pitch1 is None else pitch1
    vt, n = L.view_table(views) if views is not None else (None, 1)
    return (fmt, tab, Bf, h, w, pitch0, pitch1, vt, n if V is None else V, L.fill_bytes((1, 2, 3)) if fill else None), keep


def _forward(on_device=0, **kw):
    """cf_forward_views without a context: the arguments are checked all the same."""
    (fmt, tab, Bf, h, w, p0, p1, vt, V, fill), keep = _args(**kw)
    return L.lib().cf_forward_views(None, fmt, tab, on_device, Bf, h, w, p0, p1, vt, V, fill)


def _op(H=4, W=8, out=True, **kw):
    (fmt, tab, Bf, h, w, p0, p1, vt, V, fill), keep = _args(**kw)
    canv = np.zeros((max(Bf, 1), max(V, 1), max(H, 1), max(W, 1), 3), np.uint8)
    return L.lib().cf_op_views(0, fmt, tab, Bf, h, w, p0, p1, vt, V, fill, H, W, L.ptr(canv) if out else None)


BAD_VIEWS = [  # (view, what the message says)
    ((1, 0, 4, 4, 0, 0, 8, 4), b"odd"), ((0, 1, 4, 4, 0, 0, 8, 4), b"odd"), ((0, 0, 3, 4, 0, 0, 8, 4), b"odd"), ((0, 0, 4, 5, 0, 0, 8, 4), b"odd"),
    ((0, 0, 0, 4, 0, 0, 8, 4), b"smaller than 2"), ((0, 0, 4, 0, 0, 0, 8, 4), b"smaller than 2"),
    ((-2, 0, 4, 4, 0, 0, 8, 4), b"inside the frame"), ((0, -2, 4, 4, 0, 0, 8, 4), b"inside the frame"), ((10, 0, 4, 4, 0, 0, 8, 4), b"inside the frame"),
    ((0, 6, 4, 4, 0, 0, 8, 4), b"inside the frame"), ((0, 0, 14, 4, 0, 0, 8, 4), b"inside the frame"), ((0, 0, 4, 10, 0, 0, 8, 4), b"inside the frame"),
    ((0, 0, 4, 4, 0, 0, 0, 4), b"empty content"), ((0, 0, 4, 4, 0, 0, 8, 0), b"empty content"), ((0, 0, 4, 4, 0, 0, -1, 4), b"empty content"),
    ((0, 0, 4, 4, -1, 0, 8, 4), b"inside the canvas"), ((0, 0, 4, 4, 0, -1, 8, 4), b"inside the canvas"),
]
BAD_IN_A_CANVAS = [((0, 0, 4, 4, 1, 0, 8, 4), b"inside the canvas"), ((0, 0, 4, 4, 0, 1, 8, 4), b"inside the canvas"), ((0, 0, 4, 4, 0, 0, 9, 4), b"inside the canvas"),
                   ((0, 0, 4, 4, 0, 0, 8, 5), b"inside the canvas"), ((0, 0, 4, 4, 8, 0, 1, 1), b"inside the canvas"), ((0, 0, 4, 4, 0, 4, 1, 1), b"inside the canvas")]


def test_forward_views_without_a_context_checks_its_arguments_first_and_names_the_view():
    err = L.lib().cf_op_last_error
    for view, what in BAD_VIEWS:
        for at in (0, 2):                                                     # the offending view's index is in the message
            views = [GOOD] * at + [view] + [GOOD]
            assert _forward(views=views) == -1, view
            msg = err()
            assert b"cf_forward_views" in msg and b"view %d " % at in msg and what in msg, (view, at, msg)
            assert _op(views=views) == -1 and b"cf_op_views" in err() and b"view %d " % at in err() and what in err(), (view, at, err())
    for view, what in BAD_IN_A_CANVAS:                                        # these need a canvas: the single-op form has one
        views = [GOOD, GOOD, GOOD, view]
        assert _op(views=views) == -1 and b"view 3 " in err() and what in err(), (view, err())
    others = [dict(views=()), dict(V=0), dict(views=None), dict(fmt=-1), dict(fmt=5), dict(Bf=0), dict(h=7), dict(w=11), dict(h=8194), dict(w=0),
              dict(pitch0=35), dict(fmt=L.CF_YUV_NV12, pitch0=11), dict(fmt=L.CF_YUV_NV21, pitch1=11), dict(fmt=L.CF_YUV_I420, pitch1=5),
              dict(planes=(False, True, True)), dict(fmt=L.CF_YUV_NV12, planes=(True, False, True)), dict(fmt=L.CF_YUV_I420, planes=(True, True, False)),
              dict(fill=False)]
    for kw in others:
        assert _forward(**kw) == -1 and b"cf_forward_views" in err(), kw
        assert b"null context" not in err(), (kw, err())                      # the cause, not the missing context
        assert _op(**kw) == -1 and b"cf_op_views" in err(), kw
    assert _forward(views=()) == -1 and b"V must be at least 1" in err()
    # device planes: addresses and pitches are multiples of 4
    assert _forward(on_device=1, pitch0=38) == -1 and b"cf_forward_views" in err() and b"null context" not in err()
    # good arguments: only the context is missing
    for kw in (dict(), dict(fmt=L.CF_YUV_YV12), dict(pitch0=50), dict(views=[GOOD, (8, 4, 4, 4, 7, 3, 1, 1), (0, 0, 12, 8, 1, 1, 5, 3)])):
        assert _forward(**kw) == -1 and b"null context" in err(), kw
        assert _op(**kw) != -1, kw                                             # ... and the single-op form gets as far as the device
    for kw in (dict(W=6), dict(W=0), dict(H=0), dict(out=False)):
        assert _op(**kw) == -1 and b"cf_op_views" in err(), kw
    o = L.merge_opts()
    assert L.lib().cf_merge_views(None, C.byref(o), 4, None, None, None, None, 0) == -1


def test_op_merge_views_refuses_bad_arguments_before_any_device_work():
    def merge(opts=None, views=(GOOD,), Bf=1, h=8, w=12, H=4, W=8, rows=2, max_out=4, null=None):
        vt, V = L.view_table(views)
        a = {k: np.zeros(s, np.float32) for k, s in (("d", (Bf, V, rows, 4)), ("s", (Bf, V, rows)), ("l", (Bf, V, rows, 10)), ("od", (Bf, max(max_out, 1), 5)),
                                                     ("ol", (Bf, max(max_out, 1), 10)))}
        cn, oc, fl = (np.zeros(max(Bf * V, 1), np.int32) for _ in range(3))
        o = opts or L.merge_opts()
        p = {k: (None if k == null else L.ptr(v)) for k, v in dict(a, cn=cn, oc=oc, fl=fl).items()}
        return L.lib().cf_op_merge_views(0, None if null == "o" else C.byref(o), vt, V, Bf, h, w, H, W, p["d"], p["s"], p["l"], p["cn"], rows, max_out,
                                         p["od"], p["ol"], p["oc"], p["fl"])
    err = L.lib().cf_op_last_error
    for kw in (dict(opts=L.merge_opts(metric=2)), dict(opts=L.merge_opts(thresh=-0.1)), dict(opts=L.merge_opts(edge=-1)), dict(opts=L.merge_opts(thresh=float("nan"))),
               dict(opts=L.merge_opts(edge=float("inf"))), dict(rows=0), dict(max_out=0), dict(H=0), dict(W=0), dict(h=7), dict(Bf=0), dict(views=()),
               dict(null="o"), dict(null="d"), dict(null="s"), dict(null="l"), dict(null="cn"), dict(null="od"), dict(null="ol"), dict(null="oc"), dict(null="fl")):
        assert merge(**kw) == -1, kw
        assert b"cf_op_merge_views" in err(), kw
    for view, what in BAD_VIEWS + BAD_IN_A_CANVAS:
        assert merge(views=[GOOD, view]) == -1 and b"view 1 " in err() and what in err(), (view, err())
    assert merge() != -1
    assert merge(views=(GOOD,) * 64, rows=4096) == L.CF_ENOMEM               # 262144 candidates per frame: 8 GiB of suppression bits


# ------------------------------------------------------------------------------------------ the Python layers
def test_python_wrappers_and_product_paths_refuse_what_they_can_see():
    img = np.zeros((1, 8, 12, 3), np.uint8)
    with pytest.raises(ValueError):
        ops.cut_views(img[:, :, ::2], [GOOD], (4, 8))                      # rows not contiguous
    with pytest.raises(ValueError):
        ops.cut_views(img, [GOOD], (4, 8), fmt="rgb")
    with pytest.raises(ValueError):
        ops.cut_views(img, [(1, 0, 4, 4, 0, 0, 8, 4)], (4, 8))             # the library's refusal is a ValueError too
    with pytest.raises(ValueError):
        ops.cut_views(img, [GOOD], (4, 8), fill=(1, 2))
    with pytest.raises(ValueError):
        ops.merge_views([GOOD], (8, 12), (4, 8), np.zeros((1, 2, 3, 4)), np.zeros((1, 2, 3)), np.zeros((1, 2, 3, 10)), np.zeros((1, 2)), 4)
    # views= is refused together with tiled=True, fit= and rotate= by every product path, before any engine exists
    face = cfa.CenterFace.__new__(cfa.CenterFace)
    assert face._views_options(None) is None and face._views_options(False, True, True, 90) is None
    full = face._views_options(True)
    assert full == dict(scales=(1.0, 0.5), tile=None, overlap=None, anchor="center", fill=(0, 0, 0), metric="ios", thresh=0.5, edge=2.0)
    assert face._views_options(dict(scales=(0.25,), tile=64, edge=0.0)) == dict(full, scales=(0.25,), tile=64, edge=0.0)
    for bad in (dict(cell=4), dict(anchor="middle"), dict(fill=(1, 2)), dict(scales=(1.5,)), dict(scales=(0.5,) * 9), dict(metric="giou")):
        with pytest.raises(ValueError):
            face._views_options(bad)
    frames, yuv = np.zeros((1, 8, 12, 3), np.uint8), np.zeros((1, 12, 12), np.uint8)
    for other, kw in (("tiled", dict(tiled=True)), ("fit", dict(fit=True)), ("rotate", dict(rotate=90))):
        for call in (lambda: face.anonymize(frames, views=True, **kw), lambda: face.anonymize_yuv(yuv, views=True, **kw),
                     lambda: face.annotate(frames, views={"scales": (1.0,)}, **kw), lambda: face.annotate_yuv(yuv, views=True, **kw),
                     lambda: face.best_shots(frames, tracker=object(), shots=object(), views=True, **kw),
                     lambda: face.detect_aligned_frames(frames, views=True, **kw)):
            with pytest.raises(ValueError) as e:
                call()
            assert "views" in str(e.value) and other in str(e.value), (other, str(e.value))
    for call in (lambda: face.detect_views(frames, scales=(2.0,)), lambda: face.detect_views(frames, anchor="middle"), lambda: face.detect_views(frames, metric="giou"),
                 lambda: face.detect_views(frames, lookback=object()), lambda: face.anonymize(frames, views=dict(scales=(0.0,)))):
        with pytest.raises(ValueError):
            call()
    # rotate= with tiled=True keeps raising what it raised
    with pytest.raises(ValueError) as e:
        face.anonymize(frames, rotate=90, tiled=True)
    assert "rotate" in str(e.value) and "tiled" in str(e.value) and "views" not in str(e.value)
