"""The tracker's C ABI and Python binding, and the hand-checked cases of its numpy restatement (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from track_cases import RefTracker, iou32, grown, tables, run_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "centerface_hip.h")).read()
SYMBOLS = ("cf_track_create", "cf_track_destroy", "cf_track_reset", "cf_track_update", "cf_op_track")
CTYPES = {"float": C.c_float, "int32_t": C.c_int32}


def test_symbols_exported_declared_and_bound():
    L = cfa._lib.lib()
    for s in SYMBOLS:
        assert s in cfa._lib.EXPORTS
        assert re.search(r"\bint %s\(" % s, HEADER), s
        assert hasattr(L, s) and getattr(L, s).argtypes, s
    assert "typedef struct cf_tracker cf_tracker;" in HEADER
    assert callable(cfa.ops.track_sequence) and cfa.Tracker is cfa.centerface.Tracker
    for name in ("track_update", "track_update_device"):
        assert callable(getattr(cfa.Engine, name))


def test_track_opts_agree_with_the_header_and_other_structs_kept_their_size():
    body = re.search(r"typedef struct cf_track_opts \{(.*?)\} cf_track_opts;", HEADER, re.S).group(1)
    fields = re.findall(r"^\s*(float|int32_t)\s+(\w+);", body, re.M)
    assert [(n, CTYPES[t]) for t, n in fields] == list(cfa._lib.TrackOpts._fields_)
    assert [n for _, n in fields] == ["iou_thresh", "max_age", "min_hits", "max_tracks", "hold_grow"]
    assert C.sizeof(cfa._lib.TrackOpts) == 20
    assert C.sizeof(cfa._lib.RedactOpts) == 20 and C.sizeof(cfa._lib.BlurOpts) == 12 and C.sizeof(cfa._lib.MergeOpts) == 12
    o = cfa._lib.track_opts()
    assert (round(o.iou_thresh, 6), o.max_age, o.min_hits, o.max_tracks, o.hold_grow) == (0.3, 15, 2, 256, 0.0)


def test_makefile_builds_the_kernel_without_fma_contraction():
    mk = open(os.path.join(ROOT, "lightweight-face-detection-centernet_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "cf_track.hip" in srcs
    assert re.search(r"^EXTRA_cf_track\s*=\s*-ffp-contract=off\s*$", mk, re.M)


GOOD = dict(iou=0.3, max_age=15, min_hits=2, max_tracks=4, hold_grow=0.1)
BAD_OPTS = [dict(iou=0.0), dict(iou=-0.1), dict(iou=1.0001), dict(iou=float("nan")), dict(iou=float("inf")),
            dict(max_age=-1), dict(max_age=1001), dict(min_hits=0), dict(min_hits=1001), dict(max_tracks=0), dict(max_tracks=1025),
            dict(hold_grow=-0.01), dict(hold_grow=1.01), dict(hold_grow=float("nan")), dict(hold_grow=float("inf"))]


def _op_args(S=2, F=2, rows=3, M=4):
    return dict(boxes=np.zeros((F, S, rows, 4), np.float32), scores=np.zeros((F, S, rows), np.float32), lms_in=np.zeros((F, S, rows, 10), np.float32),
                counts_in=np.zeros((F, S), np.int32), dets=np.full((F, S, M, 5), 9.0, np.float32), lms=np.full((F, S, M, 10), 9.0, np.float32),
                info=np.full((F, S, M, 3), 9, np.int32), counts=np.full((F, S), 9, np.int32), flags=np.full((F, S), 9, np.int32))


def _op_track(o, S, F, rows, a):
    P = cfa._lib.ptr
    L = cfa._lib.lib()
    order = ("boxes", "scores", "lms_in", "counts_in", "dets", "lms", "info", "counts", "flags")
    keep = {k: (None if a[k] is None else a[k].copy()) for k in order}
    r = L.cf_op_track(0, C.byref(o) if o is not None else None, S, F, rows, *[P(a[k]) for k in order])
    for k in order:                                                       # refused: nothing was written
        assert a[k] is None or a[k].tobytes() == keep[k].tobytes(), k
    return r, (L.cf_op_last_error() or b"").decode()


@pytest.mark.parametrize("bad", BAD_OPTS, ids=lambda d: "%s=%r" % next(iter(d.items())))
def test_bad_options_are_refused_before_any_device(bad):
    o = cfa._lib.track_opts(**dict(GOOD, **bad))
    r, why = _op_track(o, 2, 2, 3, _op_args())
    assert r == -1 and next(iter(bad)).split("_")[0] in why, why
    out = C.c_void_p(1234)
    assert cfa._lib.lib().cf_track_create(None, 2, C.byref(o), C.byref(out)) == -1 and out.value == 1234
    why = cfa._lib.lib().cf_op_last_error().decode()
    assert "cf_track_create" in why and "null context" not in why and next(iter(bad)).split("_")[0] in why, why
    with pytest.raises(ValueError):
        cfa.Tracker(0, 2, **dict(GOOD, **bad))


def test_bad_counts_ranges_and_null_pointers_are_refused_before_any_device():
    o = cfa._lib.track_opts(**GOOD)
    L = cfa._lib.lib()
    for S, F, rows in ((0, 2, 3), (4097, 2, 3), (2, 0, 3), (2, 2, 0), (-1, 2, 3), (2, -1, 3), (2, 2, -1)):
        r, why = _op_track(o, S, F, rows, _op_args())
        assert r == -1 and "cf_op_track" in why, (S, F, rows, why)
    r, why = _op_track(None, 2, 2, 3, _op_args())
    assert r == -1 and "null options" in why
    for k in ("boxes", "scores", "lms_in", "counts_in", "dets", "lms", "info", "counts", "flags"):
        a = _op_args()
        a[k] = None
        r, why = _op_track(o, 2, 2, 3, a)
        assert r == -1 and "null" in why, (k, why)
    a = _op_args()
    a["counts_in"][1, 0] = -1
    r, why = _op_track(o, 2, 2, 3, a)
    assert r == -1 and "negative count" in why
    # cf_track_create: the stream count, null options, null out; a good set is refused only for the missing context
    out = C.c_void_p(1234)
    for S in (0, -3, 4097):
        assert L.cf_track_create(None, S, C.byref(o), C.byref(out)) == -1 and "n_streams" in L.cf_op_last_error().decode() and out.value == 1234
    assert L.cf_track_create(None, 2, None, C.byref(out)) == -1 and "null options" in L.cf_op_last_error().decode()
    assert L.cf_track_create(None, 2, C.byref(o), None) == -1 and "null out" in L.cf_op_last_error().decode()
    assert L.cf_track_create(None, 2, C.byref(o), C.byref(out)) == -1 and "null context" in L.cf_op_last_error().decode() and out.value == 1234
    assert L.cf_track_destroy(None) == 0
    assert L.cf_track_reset(None, 0) == -1
    assert L.cf_track_update(None, None, 0, None, None, None, None, None, 0) == -1
    t = cfa.Tracker(0, 3, **GOOD)                                         # lazily created: no device is touched here
    t.reset(), t.reset(2)
    with pytest.raises(ValueError):
        t.reset(3)
    t.close()
    with pytest.raises(ValueError):
        cfa.ops.track_sequence(np.zeros((2, 2, 3, 5), np.float32), np.zeros((2, 2, 3)), np.zeros((2, 2, 3, 10)), np.zeros((2, 2)))


# ---------------------------------------------------------------------------------------------- the restatement, checked by hand
def test_restatement_exact_threshold_match():
    """(0,0,9,9) has area 100, (0,0,9,4) area 50 and lies inside it: IoU = 50 / (100 + 50 - 50) = 0.5 exactly, which matches at 0.5 and
    not at the next float32 above it."""
    assert iou32((0, 0, 9, 9), (0, 0, 9, 4)) == np.float32(0.5)
    for thr, same in ((0.5, True), (float(np.nextafter(np.float32(0.5), np.float32(1))), False)):
        t = RefTracker(1, iou=thr, max_age=0, min_hits=1, max_tracks=4)
        _, _, i0, _ = t.update(0, [(0, 0, 9, 9)], [0.9], np.zeros((1, 10)), 1)
        d, _, i1, _ = t.update(0, [(0, 0, 9, 4)], [0.8], np.ones((1, 10)), 1)
        assert i0.tolist() == [[1, 1, 0]]
        assert i1.tolist() == ([[1, 2, 0]] if same else [[2, 1, 0]])
        assert d.tolist() == [[0, 0, 9, 4, np.float32(0.8)]]


def test_restatement_tie_goes_to_the_lowest_slot():
    """Two slots mirror each other about the row: equal IoU; slot 0 takes it, slot 1 ages."""
    t = RefTracker(1, iou=0.3, max_age=5, min_hits=1, max_tracks=4)
    t.update(0, [(0, 0, 9, 9), (20, 0, 29, 9)], [0.9, 0.8], np.zeros((2, 10)), 2)
    row = (10, 0, 19, 9)
    assert iou32((0, 0, 9, 9), row) == iou32((20, 0, 29, 9), row) == 0       # apart: below the threshold, a third track is born
    t2 = RefTracker(1, iou=0.3, max_age=5, min_hits=1, max_tracks=4)
    t2.update(0, [(0, 0, 19, 9), (10, 0, 29, 9)], [0.9, 0.8], np.zeros((2, 10)), 2)
    row = (5, 0, 24, 9)
    a, b = iou32((0, 0, 19, 9), row), iou32((10, 0, 29, 9), row)
    assert a == b and a >= np.float32(0.3)                                   # 150 / 250 = 0.6 from both sides
    d, _, info, _ = t2.update(0, [row], [0.7], np.zeros((1, 10)), 1)
    assert info.tolist() == [[1, 2, 0], [2, 1, 1]]
    assert d[0, :4].tolist() == [5, 0, 24, 9] and d[1, :4].tolist() == [10, 0, 29, 9]


def test_restatement_row_order_decides_between_two_rows():
    """Two rows want the one slot: the earlier row gets it (although the later overlaps more), the later one is born."""
    t = RefTracker(1, iou=0.3, max_age=5, min_hits=1, max_tracks=4)
    t.update(0, [(0, 0, 19, 19)], [0.9], np.zeros((1, 10)), 1)
    rows = [(2, 0, 21, 19), (0, 0, 19, 19)]
    assert iou32((0, 0, 19, 19), rows[0]) < iou32((0, 0, 19, 19), rows[1])
    d, _, info, _ = t.update(0, rows, [0.5, 0.6], np.zeros((2, 10)), 2)
    assert info.tolist() == [[1, 2, 0], [2, 1, 0]]
    assert d[:, :4].tolist() == [[2, 0, 21, 19], [0, 0, 19, 19]]


def test_restatement_hold_age_birth_and_growth():
    """min_hits = 2, max_age = 2: a one-frame face is never held; a confirmed one is held two frames, its box growing by a quarter of
    its half-size per missed frame, then dies; the next face takes the lowest free slot with a new id."""
    assert [float(v) for v in grown((10, 20, 30, 60), 0.25, 2)] == [5.0, 10.0, 35.0, 70.0]
    assert grown((10, 20, 30, 60), 0.25, 0) == [10, 20, 30, 60]
    face, other = (10, 20, 30, 60), (100, 100, 120, 120)
    frames = [[[face, other]], [[face]], [[]], [[]], [[]], [[other]]]
    b, s, l, c = tables(frames, 2)
    d, lm, info, cnt, fl = run_sequence(b, s, l, c, iou=0.3, max_age=2, min_hits=2, max_tracks=3, hold_grow=0.25)
    assert cnt[:, 0].tolist() == [2, 1, 1, 1, 0, 1] and not fl.any()
    assert info[1, 0, 0].tolist() == [1, 2, 0]                               # `other` (id 2, one hit) was freed at once
    assert info[2, 0, 0].tolist() == [1, 2, 1] and d[2, 0, 0, :4].tolist() == [7.5, 15.0, 32.5, 65.0]
    assert info[3, 0, 0].tolist() == [1, 2, 2] and d[3, 0, 0, :4].tolist() == [5.0, 10.0, 35.0, 70.0]
    assert np.array_equal(lm[3, 0, 0], l[1, 0, 0])                           # last-seen landmarks
    assert info[5, 0, 0].tolist() == [3, 1, 0]                               # slot 0 again, ids still rising
    # overflow: max_tracks = 1, two faces -> the first row wins, the flag is set
    _, _, info, cnt, fl = run_sequence(b[:1], s[:1], l[:1], c[:1], min_hits=1, max_tracks=1)
    assert cnt.tolist() == [[1]] and fl.tolist() == [[1]] and info[0, 0, 0].tolist() == [1, 1, 0]
