"""Tiled detection (cf_tile_grid, cf_forward_tiles, cf_merge_tiles, cf_op_cut_tiles, cf_op_merge_tiles): what can be checked without a
GPU -- the declarations, the host-only rectangle grid against a pure-Python restatement, the refusals that come before any device
work -- and the numpy restatements of the cutter and the merge that tests/test_tiles.py compares the kernels with.

A refusal that needs a context (Bf * T > max_batch) is in tests/test_tiles.py: a context cannot be created without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
import csrc_text
from oracle import centerface_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = cfa._lib


# ------------------------------------------------------------------------------------------ restatements
def tile_grid_ref(h, w, tile_h, tile_w, overlap, with_full=True):
    """cf_tile_grid in Python integers: [(x0, y0, rw, rh), ...], row-major, the whole frame last."""
    def axis(n, t):
        r = min(t, n)
        if r == n:
            return r, [0]
        k = -(-(n - overlap) // (r - overlap))
        return r, [((i * (n - r)) // (k - 1)) & ~1 for i in range(k)]
    rw, xs = axis(w, tile_w)
    rh, ys = axis(h, tile_h)
    out = [(x0, y0, rw, rh) for y0 in ys for x0 in xs]
    if with_full and len(out) > 1:
        out.append((0, 0, w, h))
    return out


def cut_ref(bgr, rect, size):
    """Tile of one BGR frame [h,w,3]: the crop, resized as the oracle restates cv2.resize (the taps clamp at the crop's edges)."""
    x0, y0, rw, rh = (int(v) for v in rect)
    return O.resize_bilinear_u8(np.ascontiguousarray(bgr[y0:y0 + rh, x0:x0 + rw]), int(size[0]), int(size[1]))


def nms_ref(boxes, scores, thresh, metric="iou"):
    """oracle.nms_greedy with ONE change: metric 'ios' divides the intersection by the smaller of the two areas instead of the union."""
    x1, y1, x2, y2 = (boxes[:, i].astype(np.float32) for i in range(4))
    one = np.float32(1)
    areas = (x2 - x1 + one) * (y2 - y1 + one)
    order = np.argsort(scores, kind="stable")[::-1]
    n = boxes.shape[0]
    suppressed = np.zeros(n, dtype=bool)
    thr = np.float32(thresh)
    keep = []
    with np.errstate(all="ignore"):
        for _i in range(n):
            i = order[_i]
            if suppressed[i]:
                continue
            keep.append(int(i))
            rest = order[_i + 1:]
            xx1 = np.maximum(x1[i], x1[rest])
            yy1 = np.maximum(y1[i], y1[rest])
            xx2 = np.minimum(x2[i], x2[rest])
            yy2 = np.minimum(y2[i], y2[rest])
            w = np.maximum(np.float32(0), xx2 - xx1 + one)
            h = np.maximum(np.float32(0), yy2 - yy1 + one)
            inter = w * h
            ovr = inter / (np.minimum(areas[i], areas[rest]) if metric == "ios" else areas[i] + areas[rest] - inter)
            suppressed[rest[ovr >= thr]] = True
    return keep


def merge_ref(rects, frame_hw, net_hw, dets_net, scores, lms_net, counts, metric="ios", thresh=0.5, edge=2.0):
    """cf_merge_tiles restated: per frame (dets [n,5], lms [n,10]) in frame pixels -- ALL kept rows, in keep order -- and the flags.
    dets_net [Bf,T,rows,4], scores [Bf,T,rows], lms_net [Bf,T,rows,10], counts [Bf,T]."""
    h, w = frame_hw
    H, W = net_hw
    dets_net, scores, lms_net = (np.asarray(a, np.float32) for a in (dets_net, scores, lms_net))
    Bf, T, rows = scores.shape
    e = np.float32(edge)
    fW, fH = np.float32(W), np.float32(H)
    out, flags = [], np.zeros(Bf, np.int32)
    for f in range(Bf):
        cand_b, cand_s, cand_l = [], [], []
        for t, (x0, y0, rw, rh) in enumerate(np.asarray(rects).reshape(-1, 4).tolist()):
            n = int(counts[f][t])
            if n > rows:
                flags[f] |= 1
            sx, sy = np.float64(rw) / np.float64(W), np.float64(rh) / np.float64(H)
            for i in range(min(n, rows)):
                x1, y1, x2, y2 = dets_net[f, t, i]
                if not np.isfinite(dets_net[f, t, i]).all():
                    continue
                if (x0 > 0 and x1 < e) or (x0 + rw < w and x2 > fW - e) or (y0 > 0 and y1 < e) or (y0 + rh < h and y2 > fH - e):
                    continue
                scale = np.array([sx, sy] * 5, np.float64)
                off = np.array([x0, y0] * 5, np.float64)
                cand_b.append((dets_net[f, t, i].astype(np.float64) * scale[:4] + off[:4]).astype(np.float32))
                cand_l.append((lms_net[f, t, i].astype(np.float64) * scale + off).astype(np.float32))
                cand_s.append(scores[f, t, i])
        if not cand_b:
            out.append((np.zeros((0, 5), np.float32), np.zeros((0, 10), np.float32)))
            continue
        b, s, l = np.stack(cand_b), np.array(cand_s, np.float32), np.stack(cand_l)
        keep = nms_ref(b, s, thresh, metric)
        out.append((np.concatenate([b[keep], s[keep][:, None]], 1), l[keep]))
    return out, flags


# ------------------------------------------------------------------------------------------ the declarations
def _header():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_tile_symbols_constants_and_structs_match_the_header():
    text, code = _header()
    lib = L.lib()
    for sym in ("cf_tile_grid", "cf_forward_tiles", "cf_merge_tiles", "cf_op_cut_tiles", "cf_op_merge_tiles"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), sym
        assert sym in L.EXPORTS and hasattr(lib, sym)
        assert getattr(lib, sym).argtypes is not None, sym
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(CF_MERGE_[A-Z0-9_]+)\s+(\d+)", text)}
    assert consts == {"CF_MERGE_IOU": 0, "CF_MERGE_IOS": 1}
    assert (L.CF_MERGE_IOU, L.CF_MERGE_IOS) == (0, 1) and L.MERGE_METRICS == {"iou": 0, "ios": 1}
    for name, cls, types in (("cf_tile_rect", L.TileRect, {"int32_t": C.c_int32}), ("cf_merge_opts", L.MergeOpts, {"int32_t": C.c_int32, "float": C.c_float})):
        body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), code, flags=re.S).group(1)
        fields = []
        for ty, names in re.findall(r"(\w+)\s+([\w\s,]+);", body):
            fields += [(n.strip(), types[ty]) for n in names.split(",")]
        assert list(cls._fields_) == fields, (name, fields)
    assert C.sizeof(L.TileRect) == 16 and C.sizeof(L.MergeOpts) == 12
    o = L.merge_opts()
    assert (o.metric, o.thresh, o.edge) == (1, 0.5, 2.0)
    with pytest.raises(ValueError):
        L.merge_opts(metric="giou")
    # the cutter includes the one statement of the resize and of the conversion, and is built without FMA contraction (so is the map)
    # (the statements are in the shared headers cf_tiles.hip includes: required of the union, refused in every file of it)
    texts = csrc_text.unit("cf_tiles.hip")
    assert '#include "cf_cutpx.h"' in texts["cf_tiles.hip"] and '#include "cf_collect.h"' in texts["cf_tiles.hip"]
    csrc_text.assert_one_statement(texts, ('#include "cf_cvresize.h"', '#include "cf_yuvmath.h"', "cv_linear_coeffs(", "cv_linear_vpass(", "yuv_px("))
    mk = open(os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc", "Makefile")).read()
    assert "cf_tiles.hip" in mk and re.search(r"EXTRA_cf_tiles\s*=\s*-ffp-contract=off", mk)


# ------------------------------------------------------------------------------------------ the grid
def _grid(h, w, th, tw, ov, full=1, cap=None):
    n = C.c_int(-1)
    room = 16384 if cap is None else cap
    tab = (L.TileRect * max(room, 1))()
    C.memset(tab, 0xF9, C.sizeof(tab))
    code = L.lib().cf_tile_grid(h, w, th, tw, ov, full, tab, room, C.byref(n))
    a = np.frombuffer(tab, np.int32).reshape(-1, 4)
    return code, n.value, [tuple(r) for r in a[:max(n.value, 0) + 4].tolist()]


UNTOUCHED = (-101058055,) * 4                            # 0xF9F9F9F9


SWEEP = [(h, w, t, ov) for h in (2, 30, 64, 70, 258) for w in (2, 64, 94, 300, 642) for t in (32, 64, 640)
         for ov in (0, 2, 16, 30, 128) if ov <= t // 2]


def test_tile_grid_equals_the_restatement_and_covers_the_frame():
    assert tile_grid_ref(1080, 1920, 640, 640, 128) == [(0, 0, 640, 640), (426, 0, 640, 640), (852, 0, 640, 640), (1280, 0, 640, 640),
                                                       (0, 440, 640, 640), (426, 440, 640, 640), (852, 440, 640, 640), (1280, 440, 640, 640),
                                                       (0, 0, 1920, 1080)]
    cases = SWEEP + [(1080, 1920, 640, 128), (1080, 1920, 4096, 0), (2160, 3840, 640, 160)]
    for h, w, t, ov in cases:
        for th, tw in ((t, t), (t, 2 * t)):
            for full in (1, 0):
                want = tile_grid_ref(h, w, th, tw, ov, bool(full))
                code, n, got = _grid(h, w, th, tw, ov, full)
                assert code == 0 and n == len(want) and got[:n] == want, (h, w, th, tw, ov, full, got[:n], want)
                assert all(r == UNTOUCHED for r in got[n:n + 4])
                tiles = want[:-1] if (full and len(want) > 1) else want
                if th >= h and tw >= w:
                    assert want == [(0, 0, w, h)]                          # one rectangle, no whole-frame duplicate
                cover = np.zeros((h, w), bool)
                for x0, y0, rw, rh in want:
                    assert not ((x0 | y0 | rw | rh) & 1) and rw >= 2 and rh >= 2
                    assert 0 <= x0 and x0 + rw <= w and 0 <= y0 and y0 + rh <= h
                for x0, y0, rw, rh in tiles:
                    cover[y0:y0 + rh, x0:x0 + rw] = True
                assert cover.all(), (h, w, th, tw, ov)
                xs = sorted({r[0] for r in tiles})
                ys = sorted({r[1] for r in tiles})
                rw, rh = tiles[0][2], tiles[0][3]
                assert xs[-1] + rw == w and ys[-1] + rh == h
                assert all(a + rw - b >= ov for a, b in zip(xs, xs[1:])) and all(a + rh - b >= ov for a, b in zip(ys, ys[1:]))
    assert ops.tile_grid(1080, 1920, 640, 128).tolist() == [list(r) for r in tile_grid_ref(1080, 1920, 640, 640, 128)]
    assert ops.tile_grid(1080, 1920, (640, 640), 128, with_full=False).shape == (8, 4)


def test_tile_grid_writes_only_cap_rectangles_and_refuses_bad_values():
    want = tile_grid_ref(1080, 1920, 640, 640, 128)
    code, n, got = _grid(1080, 1920, 640, 640, 128, cap=5)
    assert code == 0 and n == 9 and got[:5] == want[:5]
    n = C.c_int(-1)
    assert L.lib().cf_tile_grid(1080, 1920, 640, 640, 128, 1, None, 0, C.byref(n)) == 0 and n.value == 9
    tab = (L.TileRect * 12)()
    for r in tab:
        r.x0 = -7
    assert L.lib().cf_tile_grid(1080, 1920, 640, 640, 128, 1, tab, 5, C.byref(n)) == 0
    assert [r.x0 for r in tab[5:]] == [-7] * 7
    for bad in ((1081, 1920, 640, 640, 128), (1080, 1921, 640, 640, 128), (1080, 1920, 641, 640, 128), (1080, 1920, 640, 642 + 1, 128),
                (1080, 1920, 640, 640, 127), (1080, 1920, 640, 640, 640), (1080, 1920, 640, 320, 320), (1080, 1920, 640, 640, -2),
                (0, 1920, 640, 640, 128), (1080, 1920, 0, 640, 0)):
        assert _grid(*bad)[0] == -1, bad
        assert b"cf_tile_grid" in L.lib().cf_op_last_error()
    assert L.lib().cf_tile_grid(1080, 1920, 640, 640, 128, 1, tab, 12, None) == -1
    with pytest.raises(ValueError):
        ops.tile_grid(1080, 1920, 640, 641)


# ------------------------------------------------------------------------------------------ refusals before any device work
def _cut(fmt=L.CF_FRAME_BGR, Bf=1, h=8, w=12, pitch0=None, pitch1=None, rects=((0, 0, 4, 4),), H=4, W=8, planes=(True, True, True), out=True):
    bgr, il = fmt == L.CF_FRAME_BGR, fmt in (L.CF_YUV_NV12, L.CF_YUV_NV21)
    buf = np.zeros(3 * 4096, np.uint8)
    tab = (L.YuvPlanes * 1)()
    tab[0].y, tab[0].c0, tab[0].c1 = [(buf.ctypes.data + 4096 * k) if on else None for k, on in enumerate(planes)]
    pitch0 = (3 * w if bgr else w) if pitch0 is None else pitch0
    pitch1 = (0 if bgr else w if il else w // 2) if pitch1 is None else pitch1
    rt, T = L.tile_rects(rects) if rects is not None else (None, 1)
    tiles = np.zeros((max(Bf, 1), max(T, 1), max(H, 1), max(W, 1), 3), np.uint8)
    return L.lib().cf_op_cut_tiles(0, fmt, tab, Bf, h, w, pitch0, pitch1, rt, T, H, W, L.ptr(tiles) if out else None)


def test_cut_and_merge_refuse_bad_arguments_before_any_device_work():
    bad = [
        dict(fmt=-1), dict(fmt=5), dict(Bf=0), dict(h=7), dict(w=11), dict(h=8194), dict(w=8194), dict(h=0), dict(W=6), dict(W=0), dict(H=0),
        dict(pitch0=35), dict(fmt=L.CF_YUV_NV12, pitch0=11), dict(fmt=L.CF_YUV_NV21, pitch1=11), dict(fmt=L.CF_YUV_I420, pitch1=5),
        dict(rects=None), dict(rects=()),
        dict(rects=((1, 0, 4, 4),)), dict(rects=((0, 1, 4, 4),)), dict(rects=((0, 0, 3, 4),)), dict(rects=((0, 0, 4, 5),)),
        dict(rects=((0, 0, 0, 4),)), dict(rects=((0, 0, 4, 0),)), dict(rects=((-2, 0, 4, 4),)), dict(rects=((0, -2, 4, 4),)),
        dict(rects=((10, 0, 4, 4),)), dict(rects=((0, 6, 4, 4),)), dict(rects=((0, 0, 14, 4),)), dict(rects=((0, 0, 4, 10),)),
        dict(rects=((0, 0, 4, 4), (0, 0, 12, 8), (2, 2, 12, 4))),
        dict(planes=(False, True, True)), dict(fmt=L.CF_YUV_NV12, planes=(True, False, True)), dict(fmt=L.CF_YUV_I420, planes=(True, True, False)),
        dict(out=False),
    ]
    for kw in bad:
        assert _cut(**kw) == -1, kw
        assert b"cf_op_cut_tiles" in L.lib().cf_op_last_error(), kw
    assert _cut(rects=((0, 0, 4, 4), (0, 0, 12, 8), (2, 2, 12, 4))) == -1 and b"rectangle 2" in L.lib().cf_op_last_error()     # named
    # fine arguments get as far as the device (none here: CF_EHIP) or succeed
    for kw in (dict(), dict(rects=((8, 4, 4, 4),)), dict(rects=((0, 0, 12, 8),)), dict(fmt=L.CF_YUV_YV12), dict(pitch0=50)):
        assert _cut(**kw) != -1, kw

    def merge(opts=None, rects=((0, 0, 4, 4),), Bf=1, h=8, w=12, H=32, W=32, rows=2, max_out=4, null=None):
        rt, T = L.tile_rects(rects)
        a = {k: np.zeros(s, np.float32) for k, s in (("d", (Bf, T, rows, 4)), ("s", (Bf, T, rows)), ("l", (Bf, T, rows, 10)), ("od", (Bf, max(max_out, 1), 5)),
                                                     ("ol", (Bf, max(max_out, 1), 10)))}
        cn, oc, fl = (np.zeros(max(Bf * T, 1), np.int32) for _ in range(3))
        o = opts or L.merge_opts()
        p = {k: (None if k == null else L.ptr(v)) for k, v in dict(a, cn=cn, oc=oc, fl=fl).items()}
        return L.lib().cf_op_merge_tiles(0, None if null == "o" else C.byref(o), rt, T, Bf, h, w, H, W, p["d"], p["s"], p["l"], p["cn"], rows, max_out,
                                         p["od"], p["ol"], p["oc"], p["fl"])
    for kw in (dict(opts=L.merge_opts(metric=2)), dict(opts=L.merge_opts(metric=-1)), dict(opts=L.merge_opts(thresh=-0.1)), dict(opts=L.merge_opts(edge=-1)),
               dict(opts=L.merge_opts(thresh=float("nan"))), dict(opts=L.merge_opts(edge=float("inf"))), dict(rows=0), dict(max_out=0), dict(H=0), dict(W=0),
               dict(h=7), dict(rects=((1, 0, 4, 4),)), dict(rects=((0, 0, 14, 4),)), dict(null="o"), dict(null="d"), dict(null="s"), dict(null="l"),
               dict(null="cn"), dict(null="od"), dict(null="ol"), dict(null="oc"), dict(null="fl")):
        assert merge(**kw) == -1, kw
        assert b"cf_op_merge_tiles" in L.lib().cf_op_last_error(), kw
    assert merge() != -1
    # 64 tiles x 4096 rows: 262144 candidates per frame need 8 GiB of suppression bits
    assert merge(rects=((0, 0, 4, 4),) * 64, rows=4096) == L.CF_ENOMEM
    # the context forms: nothing without a context
    o = L.merge_opts()
    rt, T = L.tile_rects(((0, 0, 4, 4),))
    assert L.lib().cf_merge_tiles(None, C.byref(o), 4, None, None, None, None, 0) == -1
    assert L.lib().cf_forward_tiles(None, L.CF_FRAME_BGR, (L.YuvPlanes * 1)(), 0, 1, 8, 12, 36, 0, rt, T) == -1


def test_python_wrappers_refuse_what_they_can_see():
    img = np.zeros((1, 8, 12, 3), np.uint8)
    with pytest.raises(ValueError):
        ops.cut_tiles(img[:, :, ::2], [(0, 0, 4, 4)], (4, 8))            # rows not contiguous
    with pytest.raises(ValueError):
        ops.cut_tiles(img, [(0, 0, 4, 4)], (4, 8), fmt="rgb")
    with pytest.raises(ValueError):
        ops.cut_tiles(img, [(1, 0, 4, 4)], (4, 8))                       # the library's refusal is a ValueError too
    ro = img.copy()
    ro.flags.writeable = False
    try:                                                                 # a read-only frame is fine for the cutter: it gets to the device
        assert ops.cut_tiles(ro, [(0, 0, 4, 4)], (4, 8)).shape == (1, 1, 4, 8, 3)
    except cfa._lib.CenterFaceError as e:
        assert e.code == -3, e                                           # (no device here)
    with pytest.raises(ValueError):
        ops.merge_tiles([(0, 0, 4, 4)], (8, 12), (32, 32), np.zeros((1, 2, 3, 4)), np.zeros((1, 2, 3)), np.zeros((1, 2, 3, 10)), np.zeros((1, 2)), 4)


# ------------------------------------------------------------------------------------------ the IoS variant of the NMS restatement
def test_ios_restatement_is_nms_greedy_with_one_changed_denominator():
    rng = np.random.default_rng(3)
    for n in (1, 7, 70, 300):
        xy = rng.uniform(0, 200, (n, 2)).astype(np.float32)
        wh = rng.uniform(1, 90, (n, 2)).astype(np.float32)
        boxes = np.concatenate([xy, xy + wh], 1)
        scores = rng.choice(np.linspace(0.3, 0.9, 12).astype(np.float32), n)          # many ties
        for thr in (0.3, 0.5):
            assert nms_ref(boxes, scores, thr, "iou") == O.nms_greedy(boxes, scores, thr)
        assert set(nms_ref(boxes, scores, 0.5, "ios")) <= set(nms_ref(boxes, scores, 0.5, "iou"))      # IoS >= IoU for every pair
    # a partial box lying inside a full one: IoU = 101 * 41 / (101 * 101) = 0.406 survives 0.5, IoS = 1 does not
    pair = np.float32([[100, 100, 200, 200], [100, 100, 200, 140]])
    sc = np.float32([0.9, 0.8])
    assert nms_ref(pair, sc, 0.5, "iou") == [0, 1] and O.nms_greedy(pair, sc, 0.5) == [0, 1]
    assert nms_ref(pair, sc, 0.5, "ios") == [0]
    assert nms_ref(pair, sc[::-1].copy(), 0.5, "ios") == [1]              # the higher score survives, whichever box it is
    # the restated merge on the same pair seen by two tiles (identity map: the rectangles are network-sized at the origin... of one tile)
    out, flags = merge_ref([(0, 0, 256, 256)], (256, 256), (256, 256), pair[None, None], sc[None, None], np.zeros((1, 1, 2, 10), np.float32), [[2]], "ios")
    assert len(out[0][0]) == 1 and out[0][0][0].tolist() == [100, 100, 200, 200, np.float32(0.9)] and flags.tolist() == [0]
