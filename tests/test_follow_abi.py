"""The follower's C ABI and Python binding, and the hand-checked cases of its numpy restatement (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from follow_cases import LEARNED, LOST, MOVED, NONE, RefFollower, canvas, luma_of, run_follow, view
from track_cases import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "centerface_hip.h")).read()
SYMBOLS = ("cf_track_follow", "cf_op_follow")


def test_symbols_exported_declared_and_bound():
    L = cfa._lib.lib()
    for s in SYMBOLS:
        assert s in cfa._lib.EXPORTS
        assert re.search(r"\bint %s\(" % s, HEADER), s
        assert hasattr(L, s) and getattr(L, s).argtypes, s
    assert callable(cfa.ops.follow_sequence)
    for name in ("track_follow", "track_follow_device"):
        assert callable(getattr(cfa.Engine, name))


def test_follow_opts_and_codes_agree_with_the_header():
    body = re.search(r"typedef struct cf_follow_opts \{(.*?)\} cf_follow_opts;", HEADER, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t)\s+(\w+);", body, re.M)
    assert [(n, C.c_int32) for _, n in fields] == list(cfa._lib.FollowOpts._fields_)
    assert [n for _, n in fields] == ["search", "max_sad"]
    assert C.sizeof(cfa._lib.FollowOpts) == 8
    assert C.sizeof(cfa._lib.TrackOpts) == 20 and C.sizeof(cfa._lib.RedactOpts) == 20          # the others kept their size
    for name, value in (("NONE", 0), ("LEARNED", 1), ("MOVED", 2), ("LOST", 3)):
        assert re.search(r"^#define CF_FOLLOW_%s\s+%d\s*$" % (name, value), HEADER, re.M), name
        assert getattr(cfa._lib, "CF_FOLLOW_" + name) == value
    assert (NONE, LEARNED, MOVED, LOST) == (0, 1, 2, 3)
    o = cfa._lib.follow_opts()
    assert (o.search, o.max_sad) == (4, 4096)


def test_makefile_builds_the_kernel_without_fma_contraction():
    mk = open(os.path.join(ROOT, "lightweight-face-detection-centernet_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "cf_follow.hip" in srcs
    assert re.search(r"^EXTRA_cf_follow\s*=\s*-ffp-contract=off\s*$", mk, re.M)


# ---------------------------------------------------------------------------------------------- refusals of cf_op_follow
TRACK = dict(iou=0.3, max_age=15, min_hits=2, max_tracks=4, hold_grow=0.1)
ORDER = ("boxes", "scores", "lms_in", "counts_in", "detect", "dets", "lms", "info", "counts", "flags", "moves")


def _op_args(S=2, F=2, rows=3, M=4, h=8, w=12):
    a = dict(boxes=np.zeros((F, S, rows, 4), np.float32), scores=np.zeros((F, S, rows), np.float32), lms_in=np.zeros((F, S, rows, 10), np.float32),
             counts_in=np.zeros((F, S), np.int32), detect=np.ones((F,), np.uint8), dets=np.full((F, S, M, 5), 9.0, np.float32),
             lms=np.full((F, S, M, 10), 9.0, np.float32), info=np.full((F, S, M, 3), 9, np.int32), counts=np.full((F, S), 9, np.int32),
             flags=np.full((F, S), 9, np.int32), moves=np.full((F, S, M, 4), 9, np.int32))
    a["planes"] = [np.full((h * 3 // 2, w), 7, np.uint8) for _ in range(max(F * S, 1))]      # room for every format's planes
    return a


def _op_follow(a, track=None, follow=(4, 4096), S=2, F=2, rows=3, fmt=0, h=8, w=12, pitch0=12, pitch1=12, space=(8, 12), tiled=0,
               null_opts=False, null_fopts=False, null_table=False, null_plane=None):
    P = cfa._lib.ptr
    L = cfa._lib.lib()
    o, fo = cfa._lib.track_opts(**(track or TRACK)), cfa._lib.follow_opts(*follow)
    tab = (cfa._lib.PlanesRW * len(a["planes"]))()
    for k, pl in enumerate(a["planes"]):
        tab[k].p0, tab[k].p1, tab[k].p2 = pl.ctypes.data, pl.ctypes.data + h * w, pl.ctypes.data + h * w + (h // 2) * (w // 2)
    if null_plane is not None:
        setattr(tab[null_plane[0]], "p%d" % null_plane[1], None)
    keep = {k: (None if a[k] is None else a[k].copy()) for k in ORDER}
    r = L.cf_op_follow(0, None if null_opts else C.byref(o), None if null_fopts else C.byref(fo), S, F, rows, *[P(a[k]) for k in ORDER[:5]], fmt,
                       None if null_table else tab, h, w, pitch0, pitch1, space[0], space[1], tiled, *[P(a[k]) for k in ORDER[5:]])
    for k in ORDER:                                                       # refused: nothing was written
        assert a[k] is None or a[k].tobytes() == keep[k].tobytes(), k
    return r, (L.cf_op_last_error() or b"").decode()


@pytest.mark.parametrize("follow, word", [((0, 4096), "search"), ((9, 4096), "search"), ((-1, 4096), "search"), ((4, -1), "max_sad"), ((4, 65281), "max_sad")])
def test_bad_follow_options_are_refused_before_any_device(follow, word):
    r, why = _op_follow(_op_args(), follow=follow)
    assert r == -1 and "cf_op_follow" in why and word in why, why
    # cf_track_follow checks its options and geometry before it looks at the context
    L = cfa._lib.lib()
    fo = cfa._lib.follow_opts(*follow)
    tab = (cfa._lib.PlanesRW * 1)()
    assert L.cf_track_follow(None, None, 0, 1, C.byref(fo), 4, tab, 0, 8, 12, 36, 0, None, None, None, None, None, 0) == -1
    why = L.cf_op_last_error().decode()
    assert "cf_track_follow" in why and word in why and "null context" not in why, why


def test_bad_track_options_counts_pitches_formats_and_null_pointers_are_refused_before_any_device():
    for bad, word in ((dict(iou=0.0), "iou"), (dict(max_age=-1), "max_age"), (dict(min_hits=0), "min_hits"), (dict(max_tracks=1025), "max_tracks"),
                      (dict(hold_grow=2.0), "hold_grow")):
        r, why = _op_follow(_op_args(), track=dict(TRACK, **bad))
        assert r == -1 and word in why, why
    for kw, word in ((dict(S=0), "n_streams"), (dict(S=4097), "n_streams"), (dict(F=0), "n_frames"), (dict(F=-1), "n_frames"), (dict(rows=0), "rows"),
                     (dict(fmt=5), "format"), (dict(fmt=-1), "format"), (dict(pitch0=11), "pitch0"), (dict(fmt=4, pitch0=35), "pitch0"),
                     (dict(pitch1=11), "pitch1"), (dict(fmt=2, pitch1=5), "pitch1"), (dict(h=7), "even"), (dict(h=0), "h and w"), (dict(w=8194, pitch0=8194), "h and w"),
                     (dict(space=(0, 12)), "space"), (dict(tiled=2), "tiled"), (dict(tiled=1, space=(8, 14)), "frame space"),
                     (dict(null_opts=True), "null options"), (dict(null_fopts=True), "null options"), (dict(null_table=True), "null frame table"),
                     (dict(null_plane=(3, 0)), "null plane"), (dict(null_plane=(1, 1)), "null plane"), (dict(fmt=2, null_plane=(2, 2)), "null plane")):
        r, why = _op_follow(_op_args(), **kw)
        assert r == -1 and "cf_op_follow" in why and word in why, (kw, why)
    for k in ORDER:
        a = _op_args()
        a[k] = None
        r, why = _op_follow(a)
        assert r == -1 and "null" in why, (k, why)
    a = _op_args()
    a["counts_in"][1, 0] = -1
    r, why = _op_follow(a)
    assert r == -1 and "negative count" in why
    L = cfa._lib.lib()
    fo = cfa._lib.follow_opts()
    tab = (cfa._lib.PlanesRW * 1)()
    assert L.cf_track_follow(None, None, 0, 1, None, 4, tab, 0, 8, 12, 36, 0, None, None, None, None, None, 0) == -1
    assert "null options" in L.cf_op_last_error().decode()
    assert L.cf_track_follow(None, None, 0, 1, C.byref(fo), 4, tab, 0, 8, 12, 36, 0, None, None, None, None, None, 0) == -1
    assert "null plane" in L.cf_op_last_error().decode()
    tab[0].p0 = 4096
    assert L.cf_track_follow(None, None, 0, 0, C.byref(fo), 4, tab, 0, 8, 12, 36, 0, None, None, None, None, None, 0) == -1
    assert "B must be" in L.cf_op_last_error().decode()
    assert L.cf_track_follow(None, None, 0, 1, C.byref(fo), 4, tab, 0, 8, 12, 36, 0, None, None, None, None, None, 0) == -1
    assert "null context" in L.cf_op_last_error().decode()
    with pytest.raises(ValueError):
        cfa.ops.follow_sequence(np.zeros((2, 2, 3, 5), np.float32), np.zeros((2, 2, 3)), np.zeros((2, 2, 3, 10)), np.zeros((2, 2)), np.zeros((4, 8, 12, 3), np.uint8))
    with pytest.raises(ValueError):                                        # 3 frames for F x S = 2 x 2
        cfa.ops.follow_sequence(np.zeros((2, 2, 3, 4), np.float32), np.zeros((2, 2, 3)), np.zeros((2, 2, 3, 10)), np.zeros((2, 2)), np.zeros((3, 8, 12, 3), np.uint8))


def test_centerface_follow_arguments_need_a_tracker():
    f = cfa.CenterFace._follow
    assert f(None, None, True, None, "frames", "bgr") is None and f(None, False, True, None, "frames", "bgr") is None
    for follow, detect in ((True, True), (None, False), (dict(search=2), True)):
        with pytest.raises(ValueError):
            f(None, follow, detect, None, "frames", "bgr")
    trk = object()
    assert f(None, True, True, trk, "frames", "nv12") == ("frames", "nv12", {})
    assert f(None, None, False, trk, "frames", "nv12") == ("frames", "nv12", {})
    assert f(None, dict(search=2, max_sad=9), True, trk, "frames", "bgr") == ("frames", "bgr", dict(search=2, max_sad=9))
    with pytest.raises(ValueError):
        f(None, dict(radius=2), True, trk, "frames", "bgr")


# ---------------------------------------------------------------------------------------------- the restatement, checked by hand
H, W, MARGIN = 160, 160, 40


def _one_face(side):
    """A face of ``side`` pixels centred at (80, 80) with distinct landmarks, as the update's row tables."""
    x1 = 80.0 - side / 2
    boxes, scores, lms, counts = tables([[[(x1, x1, x1 + side, x1 + side)]]], 1)
    return boxes[0, 0], scores[0, 0], lms[0, 0], 1


@pytest.mark.parametrize("side, c", ((16, 1), (40, 3), (64, 4)))
@pytest.mark.parametrize("fmt", ("nv12", "bgr"))
def test_restatement_translated_patch_is_found_exactly(side, c, fmt):
    """The whole scene moves by (dx*c, dy*c): the window about the old centre holds the template exactly dx, dy cells away, SAD 0, and the
    box and the landmarks move by exactly that many pixels (frame space: fx = fy = 1)."""
    rng = np.random.default_rng(side)
    cv = canvas(rng, fmt, H, W, MARGIN, smooth=1)
    luma = lambda tx, ty: luma_of((view(cv, H, W, MARGIN, tx, ty).reshape(H, -1),), fmt)      # noqa: E731
    for dx, dy in ((0, 0), (4, -4), (-3, 2), (1, 4), (-4, -4)):
        t = RefFollower(1, (H, W), tiled=True, search=4, max_sad=0, min_hits=1, max_tracks=2)
        b, s, l, n = _one_face(side)
        t.update(0, b, s, l, n)
        d0, l0, _, m0 = t.follow(0, luma(0, 0))
        assert m0.tolist() == [[0, 0, 0, LEARNED]] and t.fol[0][0].c == c and d0[0, :4].tolist() == b[0].tolist()
        d1, l1, info, m1 = t.follow(0, luma(dx * c, dy * c))
        assert m1.tolist() == [[dx * c, dy * c, 0, MOVED]], (dx, dy, m1)
        assert d1[0, :4].tolist() == (b[0] + np.float32([dx * c, dy * c] * 2)).tolist()
        assert l1[0].tolist() == (l[0] + np.float32([dx * c, dy * c] * 5)).tolist()
        assert info.tolist() == [[1, 1, 0]]
        # the template is not refreshed: the way back is found from the same template, and the quantisation does not add up
        d2, _, _, m2 = t.follow(0, luma(0, 0))
        assert m2.tolist() == [[-dx * c, -dy * c, 0, MOVED]] and d2[0, :4].tolist() == b[0].tolist()


def test_restatement_uniform_frame_ties_go_to_no_move():
    t = RefFollower(1, (H, W), tiled=True, search=4, max_sad=0, min_hits=1, max_tracks=2)
    t.update(0, *_one_face(40))
    flat = np.full((H, W), 93, np.int64)
    assert t.follow(0, flat)[3].tolist() == [[0, 0, 0, LEARNED]]
    assert t.follow(0, flat)[3].tolist() == [[0, 0, 0, MOVED]]


def test_restatement_vanished_patch_is_lost_and_nothing_moves():
    rng = np.random.default_rng(1)
    t = RefFollower(1, (H, W), tiled=True, search=4, max_sad=0, min_hits=1, max_tracks=2)
    b, s, l, n = _one_face(40)
    t.update(0, b, s, l, n)
    t.follow(0, rng.integers(0, 256, (H, W)).astype(np.int64))
    d, lm, _, m = t.follow(0, rng.integers(0, 256, (H, W)).astype(np.int64))
    assert m[0, 3] == LOST and m[0, 2] > 0
    assert d[0, :4].tobytes() == b[0].tobytes() and lm[0].tobytes() == l[0].tobytes()
    assert t.slots[0][0].box.tobytes() == b[0].tobytes() and t.fol[0][0].box == b[0].tobytes()


def test_restatement_relearns_after_an_update_or_under_a_new_id():
    rng = np.random.default_rng(2)
    frame = rng.integers(0, 256, (H, W)).astype(np.int64)
    t = RefFollower(1, (H, W), tiled=True, search=2, max_sad=65280, min_hits=1, max_age=0, max_tracks=2)
    b, s, l, n = _one_face(40)
    t.update(0, b, s, l, n)
    assert t.follow(0, frame)[3][0, 3] == LEARNED and t.follow(0, frame)[3][0, 3] == MOVED
    t.update(0, b + np.float32(1), s, l, n)                                # matched: the update rewrote the box
    assert t.slots[0][0].id == 1 and t.follow(0, frame)[3][0, 3] == LEARNED
    assert t.follow(0, frame)[3][0, 3] == MOVED
    t.update(0, b, s, l, 0)                                               # max_age = 0: freed
    t.update(0, b + np.float32(1), s, l, n)                                # the same slot, the same box, a new id
    assert t.slots[0][0].id == 2 and t.fol[0][0].box == t.slots[0][0].box.tobytes()
    assert t.follow(0, frame)[3][0, 3] == LEARNED
    # a box without a side, or with a non-finite corner, is skipped
    t2 = RefFollower(1, (H, W), tiled=True, min_hits=1, max_tracks=2)
    t2.slots[0][0].alive, t2.slots[0][0].id = True, 5
    t2.slots[0][0].box, t2.slots[0][0].score, t2.slots[0][0].lms = np.float32([5, 5, 5, 5]), np.float32(1), np.zeros(10, np.float32)
    assert t2.follow(0, frame)[3].tolist() == [[0, 0, 0, NONE]]
    t2.slots[0][0].box = np.float32([5, 5, np.inf, 9])
    assert t2.follow(0, frame)[3].tolist() == [[0, 0, 0, NONE]]


def test_restatement_network_space_moves_by_pixels_over_fx():
    """Rows of a 64 x 64 network, frames of 96 x 128: fx = 2, fy = 1.5; a move of (px, py) frame pixels is (px / 2, py / 1.5) in the rows."""
    rng = np.random.default_rng(3)
    cv = canvas(rng, "nv12", 96, 128, 32, smooth=1)
    t = RefFollower(1, (64, 64), search=4, max_sad=0, min_hits=1, max_tracks=2)
    boxes, scores, lms, _ = tables([[[(20, 24, 36, 40)]]], 1)              # 32 x 24 frame pixels: S = 32, c = 2
    t.update(0, boxes[0, 0], scores[0, 0], lms[0, 0], 1)
    t.follow(0, view(cv, 96, 128, 32, 0, 0).astype(np.int64))
    assert t.fol[0][0].c == 2
    d, _, _, m = t.follow(0, view(cv, 96, 128, 32, 6, -4).astype(np.int64))
    assert m.tolist() == [[6, -4, 0, MOVED]]
    want = [np.float32(20 + 6 / 2.0), np.float32(24.0 + -4 / 1.5), np.float32(36 + 6 / 2.0), np.float32(40.0 + -4 / 1.5)]
    assert d[0, :4].tolist() == want


def test_run_follow_detects_every_other_frame():
    rng = np.random.default_rng(4)
    cv = canvas(rng, "nv12", H, W, MARGIN, smooth=1)
    shifts = [(0, 0), (3, 0), (6, 3), (6, 6)]
    lumas = [view(cv, H, W, MARGIN, *sh).astype(np.int64) for sh in shifts]
    frames = [[[(60 + (tx if f % 2 == 0 else 0), 60 + (ty if f % 2 == 0 else 0), 100 + (tx if f % 2 == 0 else 0), 100 + (ty if f % 2 == 0 else 0))]]
              for f, (tx, ty) in enumerate(shifts)]
    b, s, l, c = tables(frames, 1)
    d, _, info, cnt, fl, mv = run_follow(b, s, l, c, lumas, (H, W), detect=[1, 0, 1, 0], tiled=True, max_sad=0, min_hits=1, max_tracks=2)
    assert cnt[:, 0].tolist() == [1, 1, 1, 1] and not fl.any()
    assert mv[:, 0, 0].tolist() == [[0, 0, 0, LEARNED], [3, 0, 0, MOVED], [0, 0, 0, LEARNED], [0, 3, 0, MOVED]]
    assert d[:, 0, 0, :4].tolist() == [[60, 60, 100, 100], [63, 60, 103, 100], [66, 63, 106, 103], [66, 66, 106, 106]]
    assert info[:, 0, 0].tolist() == [[1, 1, 0], [1, 1, 0], [1, 2, 0], [1, 2, 0]]
