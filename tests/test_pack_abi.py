"""Packed views (cf_pack_views, cf_forward_packed, cf_merge_packed, cf_op_packed, cf_op_merge_packed): what can be checked without a
GPU -- the declarations, the host-only shelf packer against the Python-integer restatement of tests/pack_cases.py (the worked examples
written out, a few hundred random item lists, the geometry of every result), the cap / n_places protocol, every CF_EINVAL with its named
cause, the refusals of cf_forward_packed that come before any device work (with no context at all), the Python layers' ValueErrors and
the words the documents owe.

A refusal that needs a context (N > max_batch, a content outside ITS canvas) is in tests/test_pack.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
import csrc_text
from pack_cases import WORKED_GUTTER_0, WORKED_GUTTER_16, WORKED_VIEWS, pack_views_ref, unpacked_places

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc")
L = cfa._lib
SYMBOLS = ("cf_pack_views", "cf_forward_packed", "cf_merge_packed", "cf_op_packed", "cf_op_merge_packed")


def _header():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


# ------------------------------------------------------------------------------------------ the declarations
def test_pack_symbols_and_struct_match_the_header():
    text, code = _header()
    lib = L.lib()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), sym
        assert sym in L.EXPORTS and hasattr(lib, sym)
        assert getattr(lib, sym).argtypes is not None, sym
    body = re.search(r"typedef struct cf_place\s*\{(.*?)\}\s*cf_place;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s+([\w\s,]+);", body) == [("int32_t", "frame, canvas"), ("cf_view", "view")]
    assert [(n, t) for n, t in L.Place._fields_] == [("frame", C.c_int32), ("canvas", C.c_int32), ("view", L.View)]
    assert C.sizeof(L.Place) == 40 and "/* 40 bytes */" in text
    assert L.Place.view.offset == 8 and C.sizeof(L.View) == 32
    # place_table lays the ten int32 of a row out as the struct
    tab, P = L.place_table([(1, 2, 3, 4, 5, 6, 7, 8, 9, 10), (0, 0, 0, 0, 2, 2, 0, 0, 1, 1)])
    v = tab[0].view
    assert P == 2 and (tab[0].frame, tab[0].canvas, v.sx0, v.sy0, v.sw, v.sh, v.dx, v.dy, v.dw, v.dh) == (1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
    assert (tab[1].frame, tab[1].view.sw, tab[1].view.dh) == (0, 2, 1)
    assert L.place_table(np.zeros((0, 10), np.int32))[1] == 0
    assert lib.cf_version() == 100                                              # nothing else moved


def test_the_packed_kernels_stand_beside_the_old_ones():
    texts = csrc_text.unit("cf_views.hip")
    src = texts["cf_views.hip"]
    assert "cut_packed_kernel" in src and "cut_views_kernel" in src
    # the rows of either go through the one collect kernel (an Items type each) and the one launch of the NMS stages, unchanged
    merge = csrc_text.unit("cf_tiles.hip")
    csrc_text.assert_one_statement(merge, ("collect_rows_kernel<PlacedItems, 0>", "collect_rows_kernel<ViewItems, 0>", "struct PlacedItems", "struct ViewItems"))
    assert merge["cf_tiles.hip"].count("launch_nms_stages(") == 1 and "launch_nms_stages(" not in src
    csrc_text.assert_one_statement(texts, ())                                    # the list and the compactions are prefix sums


def test_the_documents_state_what_is_built_and_its_limits():
    header = _header()[0]
    section = header[header.index("packed views: several levels"):header.index("face tracks across video frames")]
    docs = {"header": section}
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        docs[name] = open(os.path.join(REPO, name)).read()
    for name, text in docs.items():
        flat = re.sub(r"[\s*`]+", " ", text.lower())
        assert "cf_forward_packed" in text and "cf_merge_packed" in text and "cf_pack_views" in text, name
        for word in ("per canvas", "gutter", "share an edge", "not measured" if name == "INTEGRATION.md" else "nobody has measured"):
            assert word in flat, (name, word)
        assert not re.search(r"packing[^.]*into one canvas[^.]*is not built", flat), name
    for name in ("header", "README.md", "DESIGN.md"):
        flat = re.sub(r"[\s*`]+", " ", docs[name].lower())
        assert "cf_align_faces" in flat and "rotated" in flat, name
    # the timing file holds the probe's table, or says plainly that there is none
    prof = open(os.path.join(REPO, "profiles", "pack.md")).read()
    assert "pack_probe.py" in prof and ("not measured" in prof.lower() or re.search(r"^\|.*packed.*\|\s*\d", prof, flags=re.M))


# ------------------------------------------------------------------------------------------ the packer
UNTOUCHED = (-101058055,) * 10                           # 0xF9F9F9F9
ROOM = 8


def _pack(views, Bf, H, W, gutter=0, cap=None, V=None, null=()):
    """The raw call: (code, placements written, n_places, n_canvases, the rows behind the written ones)."""
    vt, n = L.view_table(views)
    V = n if V is None else V
    want = max(V, 0) * max(Bf, 0)
    cap = want if cap is None else cap
    buf = np.full((max(cap, want, 0) + ROOM, 10), UNTOUCHED[0], np.int32)
    tab = (L.Place * len(buf)).from_buffer(buf)
    P, N = C.c_int(-1), C.c_int(-1)
    code = L.lib().cf_pack_views(None if "views" in null else vt, V, Bf, H, W, gutter, None if "places" in null else tab, cap,
                                 None if "n_places" in null else C.byref(P), None if "n_canvases" in null else C.byref(N))
    return code, buf, P.value, N.value


def _check_geometry(places, N, H, W, gutter):
    """Inside the canvas, pairwise at least ``gutter`` apart (so disjoint), canvases 0 .. N - 1 all used."""
    by = {}
    for f, n, _, _, _, _, dx, dy, dw, dh in places:
        assert 0 <= n < N and dx >= 0 and dy >= 0 and dx + dw <= W and dy + dh <= H, (n, dx, dy, dw, dh)
        by.setdefault(n, []).append((dx, dy, dw, dh))
    assert sorted(by) == list(range(N))
    for n, rs in by.items():
        a = np.array(rs, np.int64)
        x0, y0, x1, y1 = a[:, 0], a[:, 1], a[:, 0] + a[:, 2], a[:, 1] + a[:, 3]
        apart_x = (x0[:, None] >= x1[None, :] + gutter) | (x0[None, :] >= x1[:, None] + gutter)
        apart_y = (y0[:, None] >= y1[None, :] + gutter) | (y0[None, :] >= y1[:, None] + gutter)
        ok = apart_x | apart_y | np.eye(len(rs), dtype=bool)
        assert ok.all(), (n, gutter, np.argwhere(~ok)[:2].tolist())


def test_pack_views_worked_examples():
    """1080 x 1920 frames in 640 x 640, levels 1000, 500 and 250, Bf = 2: the tuples of the statement, written out."""
    assert ops.view_layout(1080, 1920, 640, 640, scales=(1.0, 0.5, 0.25)).tolist() == [list(v) for v in WORKED_VIEWS]
    assert WORKED_GUTTER_0 == [(0, 0, 0), (0, 0, 360), (0, 320, 360), (1, 0, 0), (1, 0, 360), (0, 480, 360)]
    assert WORKED_GUTTER_16 == [(0, 0, 0), (0, 0, 376), (0, 336, 376), (1, 0, 0), (1, 0, 376), (1, 336, 376)]
    for gutter, want in ((0, WORKED_GUTTER_0), (16, WORKED_GUTTER_16)):
        places, N = ops.pack_views(WORKED_VIEWS, 2, (640, 640), gutter)
        assert N == 2 and places.dtype == np.int32 and places.shape == (6, 10)
        assert [(p[1], p[6], p[7]) for p in places.tolist()] == want, gutter
        assert places[:, 0].tolist() == [0, 0, 0, 1, 1, 1]                       # frame-major
        assert places[:, 2:6].tolist() == [list(v[:4]) for v in WORKED_VIEWS] * 2 and places[:, 8:].tolist() == [list(v[6:]) for v in WORKED_VIEWS] * 2
        ref, refN = pack_views_ref(WORKED_VIEWS, 2, 640, 640, gutter)
        assert refN == 2 and places.tolist() == [list(p) for p in ref]
        _check_geometry(ref, 2, 640, 640, gutter)
    # the canvas counts of 16 such frames
    count = lambda **kw: ops.pack_views(ops.view_layout(1080, 1920, 640, 640, **kw), 16, (640, 640))[1]      # noqa: E731
    assert count(scales=(1.0, 0.5, 0.25)) == 16 and count(scales=(1.0, 0.5)) == 16 and count(scales=(0.5,)) == 3
    assert count(tile=640, overlap=128, scales=(1.0, 0.5)) == 144               # a tile view fills a canvas: eight of its own per frame
    # the unpacked list is what a packer with nothing to share gives: every view fills the canvas
    full = [(0, 0, 8, 8, 0, 0, 16, 8), (2, 2, 4, 4, 0, 0, 16, 8)]
    places, N = ops.pack_views(full, 3, (8, 16))
    assert N == 6 and places.tolist() == [list(p) for p in unpacked_places(full, 3)]


def test_pack_views_random_item_lists_equal_the_restatement():
    """A few hundred random item lists -- mixed sizes with W x H, 1 x 1 and odd ones among them, gutters 0, 1 and 16: the library's
    placements are the restatement's, and in each the contents lie inside the canvas, disjoint and at least ``gutter`` apart."""
    rng = np.random.default_rng(11)
    seen_canvases = set()
    for case in range(300):
        H, W = [(32, 64), (40, 40), (17, 23), (640, 640)][case % 4]
        gutter = (0, 1, 16)[case % 3]
        V, Bf = int(rng.integers(1, 9)), int(rng.integers(1, 7))
        views = []
        for v in range(V):
            kind = rng.integers(0, 6)
            if kind == 0:
                dw, dh = W, H
            elif kind == 1:
                dw, dh = 1, 1
            elif kind == 2:
                dw, dh = int(rng.integers(1, W + 1)) | 1, int(rng.integers(1, H + 1)) | 1
                dw, dh = min(dw, W), min(dh, H)
            else:
                dw, dh = int(rng.integers(1, W // 2 + 1)), int(rng.integers(1, H // 2 + 1))
            views.append((2 * v, 0, 2 + 2 * v, 4, int(rng.integers(0, 5)), int(rng.integers(0, 5)), dw, dh))      # dx, dy are replaced
        ref, refN = pack_views_ref(views, Bf, H, W, gutter)
        code, buf, P, N = _pack(views, Bf, H, W, gutter)
        assert code == 0 and P == V * Bf == len(ref) and N == refN, (case, P, N, refN)
        assert buf[:P].tolist() == [list(p) for p in ref], case
        assert (buf[P:] == UNTOUCHED[0]).all()
        _check_geometry(ref, N, H, W, gutter)
        got, gN = ops.pack_views(views, Bf, (H, W), gutter)
        assert gN == N and got.tolist() == buf[:P].tolist()
        seen_canvases.add(min(N, 3))
    assert seen_canvases == {1, 2, 3}


def test_pack_views_cap_and_count_protocol():
    views = [v[:4] + (5, 5) + v[6:] for v in WORKED_VIEWS]
    ref, refN = pack_views_ref(views, 4, 640, 640, 0)
    assert refN == 4                                                          # two full levels do not fit one canvas
    for cap in (0, 1, 5, 12, 20):
        code, buf, P, N = _pack(views, 4, 640, 640, 0, cap=cap)
        assert code == 0 and P == 12 and N == 4
        assert buf[:min(cap, 12)].tolist() == [list(p) for p in ref[:cap]] and (buf[min(cap, 12):] == UNTOUCHED[0]).all(), cap
    code, buf, P, N = _pack(views, 4, 640, 640, 0, cap=0, null=("places",))   # the count alone
    assert code == 0 and (P, N) == (12, 4)


def test_pack_views_refusals_name_the_cause():
    err = L.lib().cf_op_last_error
    good = [(0, 0, 4, 4, 0, 0, 8, 4)]
    cases = [(dict(null=("views",)), b"null"), (dict(null=("n_places",)), b"null"), (dict(null=("n_canvases",)), b"null"),
             (dict(null=("places",), cap=1), b"null"), (dict(V=0), b"V must be at least 1"), (dict(V=-1), b"V must be at least 1"),
             (dict(Bf=0), b"Bf must be at least 1"), (dict(Bf=-3), b"Bf must be at least 1"), (dict(gutter=-1), b"gutter"), (dict(cap=-1), b"cap"),
             (dict(H=0), b"H and W"), (dict(W=0), b"H and W"),
             (dict(views=good + [(0, 0, 4, 4, 0, 0, 9, 4)]), b"view 1 "), (dict(views=[(0, 0, 4, 4, 0, 0, 8, 5)] + good), b"view 0 "),
             (dict(views=good * 2 + [(0, 0, 4, 4, 0, 0, 0, 4)]), b"view 2 "), (dict(views=good + [(0, 0, 4, 4, 0, 0, 8, 0)]), b"view 1 "),
             (dict(views=good + [(0, 0, 4, 4, 0, 0, -2, 4)]), b"view 1 ")]
    for kw, what in cases:
        args = dict(views=good, Bf=2, H=4, W=8)
        args.update(kw)
        code, buf, P, N = _pack(**args)
        assert code == -1, kw
        assert b"cf_pack_views" in err() and what in err(), (kw, err())
        assert (buf == UNTOUCHED[0]).all() and (P, N) == (-1, -1), kw            # nothing is written on refusal
    assert _pack(good + [(0, 0, 4, 4, 0, 0, 9, 4)], 1, 4, 8)[0] == -1 and b"larger than the canvas" in err()
    assert _pack([(0, 0, 4, 4, 0, 0, 8, 0)], 1, 4, 8)[0] == -1 and b"empty content" in err()
    assert _pack(good, 2, 4, 8)[0] == 0
    # the source rectangle is none of the packer's business (cf_forward_packed checks it against the frame)
    assert _pack([(1, 3, 5, 7, 0, 0, 8, 4)], 1, 4, 8)[0] == 0
    with pytest.raises(ValueError):
        ops.pack_views(good, 0, (4, 8))
    with pytest.raises(ValueError):
        ops.pack_views(good, 1, (4, 8), gutter=-1)
    with pytest.raises(ValueError):
        ops.pack_views([(0, 0, 4, 4, 0, 0, 9, 4)], 1, (4, 8))


# ------------------------------------------------------------------------------------------ refusals before any device work
GOOD = (0, 0, 0, 0, 4, 4, 0, 0, 8, 4)                    # frame 0, canvas 0, a 4 x 4 source, the whole (4, 8) canvas


def _frames(planes=(True, True, True), Bf=1):
    buf = np.zeros(3 * 4096, np.uint8)
    tab = (L.YuvPlanes * max(Bf, 1))()
    for b in range(max(Bf, 1)):
        tab[b].y, tab[b].c0, tab[b].c1 = [(buf.ctypes.data + 4096 * k) if on else None for k, on in enumerate(planes)]
    return tab, buf


def _args(fmt=L.CF_FRAME_BGR, Bf=1, h=8, w=12, pitch0=None, pitch1=None, places=(GOOD,), planes=(True, True, True), fill=True, P=None, N=1):
    bgr, il = fmt == L.CF_FRAME_BGR, fmt in (L.CF_YUV_NV12, L.CF_YUV_NV21)
    tab, keep = _frames(planes, Bf)
    pitch0 = (3 * w if bgr else w) if pitch0 is None else pitch0
    pitch1 = (0 if bgr else w if il else w // 2) if pitch1 is None else pitch1
    pt, n = L.place_table(places) if places is not None else (None, 1)
    return (fmt, tab, Bf, h, w, pitch0, pitch1, pt, n if P is None else P, N, L.fill_bytes((1, 2, 3)) if fill else None), keep


def _forward(on_device=0, **kw):
    """cf_forward_packed without a context: the arguments are checked all the same."""
    (fmt, tab, Bf, h, w, p0, p1, pt, P, N, fill), keep = _args(**kw)
    return L.lib().cf_forward_packed(None, fmt, tab, on_device, Bf, h, w, p0, p1, pt, P, N, fill)


def _op(H=4, W=8, out=True, **kw):
    (fmt, tab, Bf, h, w, p0, p1, pt, P, N, fill), keep = _args(**kw)
    canv = np.zeros((max(N, 1), max(H, 1), max(W, 1), 3), np.uint8)
    return L.lib().cf_op_packed(0, fmt, tab, Bf, h, w, p0, p1, pt, P, N, fill, H, W, L.ptr(canv) if out else None)


BAD_VIEWS = [  # (view, what the message says)
    ((1, 0, 4, 4, 0, 0, 8, 4), b"odd"), ((0, 0, 3, 4, 0, 0, 8, 4), b"odd"), ((0, 0, 0, 4, 0, 0, 8, 4), b"smaller than 2"),
    ((-2, 0, 4, 4, 0, 0, 8, 4), b"inside the frame"), ((10, 0, 4, 4, 0, 0, 8, 4), b"inside the frame"), ((0, 0, 4, 10, 0, 0, 8, 4), b"inside the frame"),
    ((0, 0, 4, 4, 0, 0, 0, 4), b"empty content"), ((0, 0, 4, 4, 0, 0, 8, -1), b"empty content"),
    ((0, 0, 4, 4, -1, 0, 8, 4), b"inside the canvas"), ((0, 0, 4, 4, 0, -1, 8, 4), b"inside the canvas"),
]
BAD_IN_A_CANVAS = [((0, 0, 4, 4, 1, 0, 8, 4), b"inside the canvas"), ((0, 0, 4, 4, 0, 0, 8, 5), b"inside the canvas"), ((0, 0, 4, 4, 8, 0, 1, 1), b"inside the canvas")]


def test_forward_packed_without_a_context_checks_its_arguments_first():
    err = L.lib().cf_op_last_error
    other = (0, 1, 0, 0, 4, 4, 0, 0, 8, 4)                                    # the same content on another canvas: no overlap
    for view, what in BAD_VIEWS:
        for at in (0, 2):                                                     # the offending placement's index is in the message
            places = [GOOD, other][:at] + [(0, 2) + view]
            assert _forward(places=places, N=3) == -1, view
            msg = err()
            assert b"cf_forward_packed" in msg and b"placement %d" % at in msg and what in msg, (view, at, msg)
            assert _op(places=places, N=3) == -1 and b"cf_op_packed" in err() and b"placement %d" % at in err() and what in err(), (view, at, err())
    for view, what in BAD_IN_A_CANVAS:                                        # these need a canvas: the single-op form has one
        assert _op(places=[GOOD, (0, 1) + view], N=2) == -1 and b"placement 1" in err() and what in err(), (view, err())
    # the ranges of frame and canvas
    for place, what in (((1,) + GOOD[1:], b"frame 1 outside [0, 1)"), ((-1,) + GOOD[1:], b"frame -1 outside"), ((0, 1) + GOOD[2:], b"canvas 1 outside [0, 1)"),
                        ((0, -1) + GOOD[2:], b"canvas -1 outside")):
        for call in (_forward, _op):
            assert call(places=[GOOD, place]) == -1 and b"placement 1 " in err() and what in err(), (place, err())
    assert _forward(places=[GOOD, (1,) + GOOD[1:]], Bf=2, N=1) == -1 and b"overlap" in err()      # (frame 1 exists now: the same content twice)
    # two overlapping contents on one canvas: both indices are named; a shared edge is no overlap; another canvas is none either
    a, b2, c2 = (0, 0, 0, 0, 4, 4, 0, 0, 4, 4), (0, 0, 0, 0, 4, 4, 4, 0, 4, 4), (0, 0, 0, 0, 4, 4, 3, 3, 2, 1)
    for call, name in ((_forward, b"cf_forward_packed"), (_op, b"cf_op_packed")):
        assert call(places=[a, b2, c2]) == -1 and name in err(), err()            # c2 reaches into both a and b2
        m = re.search(rb"placements (\d+) and (\d+) overlap on canvas 0", err())
        assert m and (int(m.group(1)), int(m.group(2))) in ((0, 2), (1, 2)), err()
        assert call(places=[b2, GOOD[:2] + (0, 0, 4, 4, 0, 0, 1, 1), a]) == -1 and b"placements 1 and 2 overlap on canvas 0" in err(), err()
    assert _forward(places=[a, (0, 1) + c2[2:], b2], N=2) == -1 and b"null context" in err(), err()      # c2 on another canvas: no overlap
    assert _op(places=[a, (0, 1) + c2[2:], b2], N=2) != -1
    assert _forward(places=[a, b2]) == -1 and b"null context" in err()       # edge to edge at x = 4: only the context is missing
    assert _forward(places=[a, (0, 0, 0, 0, 4, 4, 0, 3, 8, 1)]) == -1 and b"placements 0 and 1 overlap" in err()      # one row of overlap
    assert _forward(places=[a, (0, 0, 0, 0, 4, 4, 0, 4, 8, 1)]) == -1 and b"null context" in err()                    # edge to edge at y = 4
    others = [dict(places=()), dict(P=0), dict(places=None), dict(N=0), dict(N=-1), dict(fmt=-1), dict(fmt=5), dict(Bf=0), dict(h=7), dict(w=11), dict(h=8194),
              dict(w=0), dict(pitch0=35), dict(fmt=L.CF_YUV_NV12, pitch0=11), dict(fmt=L.CF_YUV_NV21, pitch1=11), dict(fmt=L.CF_YUV_I420, pitch1=5),
              dict(planes=(False, True, True)), dict(fmt=L.CF_YUV_NV12, planes=(True, False, True)), dict(fmt=L.CF_YUV_I420, planes=(True, True, False)),
              dict(fill=False)]
    for kw in others:
        assert _forward(**kw) == -1 and b"cf_forward_packed" in err(), kw
        assert b"null context" not in err(), (kw, err())                      # the cause, not the missing context
        assert _op(**kw) == -1 and b"cf_op_packed" in err(), kw
    assert _forward(places=()) == -1 and b"P must be at least 1" in err()
    assert _forward(N=0) == -1 and b"N must be at least 1" in err()
    assert _forward(on_device=1, pitch0=38) == -1 and b"cf_forward_packed" in err() and b"null context" not in err()
    # good arguments: only the context is missing
    for kw in (dict(), dict(fmt=L.CF_YUV_YV12), dict(pitch0=50), dict(places=[a, b2, (0, 1, 8, 4, 4, 4, 7, 3, 1, 1)], N=3)):
        assert _forward(**kw) == -1 and b"null context" in err(), (kw, err())
        assert _op(**kw) != -1, kw                                             # ... and the single-op form gets as far as the device
    for kw in (dict(W=6), dict(W=0), dict(H=0), dict(out=False)):
        assert _op(**kw) == -1 and b"cf_op_packed" in err(), kw
    o = L.merge_opts()
    assert L.lib().cf_merge_packed(None, C.byref(o), 4, None, None, None, None, 0) == -1


def test_op_merge_packed_refuses_bad_arguments_before_any_device_work():
    def merge(opts=None, places=(GOOD,), N=1, Bf=1, h=8, w=12, H=4, W=8, rows=2, max_out=4, null=None):
        pt, P = L.place_table(places)
        n = max(N, 1)
        a = {k: np.zeros(s, np.float32) for k, s in (("d", (n, rows, 4)), ("s", (n, rows)), ("l", (n, rows, 10)), ("od", (max(Bf, 1), max(max_out, 1), 5)),
                                                     ("ol", (max(Bf, 1), max(max_out, 1), 10)))}
        cn, oc, fl = (np.zeros(max(n, Bf, 1), np.int32) for _ in range(3))
        o = opts or L.merge_opts()
        p = {k: (None if k == null else L.ptr(v)) for k, v in dict(a, cn=cn, oc=oc, fl=fl).items()}
        return L.lib().cf_op_merge_packed(0, None if null == "o" else C.byref(o), pt, P, N, Bf, h, w, H, W, p["d"], p["s"], p["l"], p["cn"], rows, max_out,
                                          p["od"], p["ol"], p["oc"], p["fl"])
    err = L.lib().cf_op_last_error
    for kw in (dict(opts=L.merge_opts(metric=2)), dict(opts=L.merge_opts(thresh=-0.1)), dict(opts=L.merge_opts(edge=-1)), dict(opts=L.merge_opts(thresh=float("nan"))),
               dict(rows=0), dict(max_out=0), dict(H=0), dict(W=0), dict(h=7), dict(Bf=0), dict(places=()), dict(N=0),
               dict(null="o"), dict(null="d"), dict(null="s"), dict(null="l"), dict(null="cn"), dict(null="od"), dict(null="ol"), dict(null="oc"), dict(null="fl")):
        assert merge(**kw) == -1, kw
        assert b"cf_op_merge_packed" in err(), kw
    for view, what in BAD_VIEWS + BAD_IN_A_CANVAS:
        assert merge(places=[GOOD, (0, 1) + view], N=2) == -1 and b"placement 1" in err() and what in err(), (view, err())
    assert merge(places=[GOOD, GOOD]) == -1 and b"placements 0 and 1 overlap" in err()
    assert merge(places=[GOOD, (1,) + GOOD[1:]]) == -1 and b"frame 1 outside" in err()
    assert merge() != -1
    # 64 placements of one frame x 4096 rows: 262144 candidates per frame, 8 GiB of suppression bits
    assert merge(places=[(0, n) + GOOD[2:] for n in range(64)], N=64, rows=4096) == L.CF_ENOMEM


# ------------------------------------------------------------------------------------------ the Python layers
def test_python_layers_refuse_before_any_device_work():
    img = np.zeros((1, 8, 12, 3), np.uint8)
    with pytest.raises(ValueError):
        ops.cut_packed(img, [GOOD], 1, (4, 8), fmt="rgb")
    with pytest.raises(ValueError):
        ops.cut_packed(img, [GOOD, GOOD], 1, (4, 8))                            # the library's refusal is a ValueError too
    with pytest.raises(ValueError):
        ops.cut_packed(img, [GOOD], 1, (4, 8), fill=(1, 2))
    with pytest.raises(ValueError):
        ops.merge_packed([GOOD], 1, (8, 12), (4, 8), np.zeros((1, 2, 3)), np.zeros((1, 2)), np.zeros((1, 2, 10)), np.zeros((1,)), 4)
    # pack and gutter are keys of views=; without them the options are what they were
    face = cfa.CenterFace.__new__(cfa.CenterFace)
    full = face._views_options(True)
    assert "pack" not in full and "gutter" not in full
    assert face._views_options(dict(pack=True)) == dict(full, pack=True)
    assert face._views_options(dict(pack=True, gutter=16, scales=(1.0, 0.5, 0.25))) == dict(full, pack=True, gutter=16, scales=(1.0, 0.5, 0.25))
    for bad in (dict(pack=True, gutter=-1), dict(gutter=4), dict(pack=True, packed=1)):
        with pytest.raises(ValueError):
            face._views_options(bad)
    frames = np.zeros((1, 8, 12, 3), np.uint8)
    for call in (lambda: face.detect_views(frames, pack=True, gutter=-2), lambda: face.detect_views(frames, gutter=3),
                 lambda: face.anonymize(frames, views=dict(pack=True), tiled=True), lambda: face.annotate(frames, views=dict(pack=True), rotate=90)):
        with pytest.raises(ValueError):
            call()
    from centerface_amd import demo
    for bad in (["--pack"], ["--scales", "1,0.5", "--gutter", "4"], ["--scales", "1,0.5", "--pack", "--gutter", "-1"]):
        with pytest.raises(SystemExit):
            demo.main(["nothing.png"] + bad)
