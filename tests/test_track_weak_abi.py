"""The C ABI and the Python binding of the tracker with two thresholds, and hand-checked cases of its numpy restatement (no GPU needed):
every refusal comes before a device is touched and names its rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from track_cases import iou32, run_sequence, tables
from weak_cases import A, A2, A3, STRONG, WEAK, WeakRefTracker, at, run_weak_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "centerface_hip.h")).read()
SYMBOLS = ("cf_track_create_weak", "cf_op_track_weak")
GOOD = dict(iou=0.3, max_age=15, min_hits=2, max_tracks=4, hold_grow=0.1)
NAN, INF = float("nan"), float("inf")
BAD_WEAK = [(dict(birth_score=v), "birth_score must be finite and in (0, 1]") for v in (0.0, -0.1, 1.0001, NAN, INF, -INF)] + \
           [(dict(weak_iou=v), "weak_iou must be finite and in (0, 1]") for v in (0.0, -0.5, 1.5, NAN, INF)]


def test_symbols_exported_declared_and_bound():
    L = cfa._lib.lib()
    for s in SYMBOLS:
        assert s in cfa._lib.EXPORTS
        assert re.search(r"\bint %s\(" % s, HEADER), s
        assert hasattr(L, s) and getattr(L, s).argtypes, s
    assert len(L.cf_track_create_weak.argtypes) == 5 and len(L.cf_op_track_weak.argtypes) == 15
    body = re.search(r"typedef struct cf_track_weak_opts \{(.*?)\} cf_track_weak_opts;", HEADER, re.S).group(1)
    assert re.findall(r"^\s*float\s+(\w+);", body, re.M) == [n for n, _ in cfa._lib.TrackWeakOpts._fields_] == ["birth_score", "weak_iou"]
    assert C.sizeof(cfa._lib.TrackWeakOpts) == 8 and C.sizeof(cfa._lib.TrackOpts) == 20      # the existing struct kept its layout
    o = cfa._lib.track_weak_opts()
    assert (round(o.birth_score, 6), o.weak_iou) == (0.3, 0.5)


def test_the_statement_is_in_the_header_the_kernel_file_and_the_readme():
    kernel = open(os.path.join(ROOT, "lightweight-face-detection-centernet_amd", "csrc", "cf_track.hip")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for text in (HEADER, kernel):
        for phrase in ("score > birth_score", "hits >= min_hits", "weak_iou", "DISCARDED", "Bit 1 (value 2)"):
            assert phrase in text, phrase
    for phrase in ("LEARNS", "back-fills only strong births", "score term already weighs it down"):
        assert phrase in HEADER, phrase
    assert "weak_score" in readme and "nobody has measured" in readme and "no accuracy claim" in readme


def _op_args(S=2, F=2, rows=3, M=4):
    return dict(boxes=np.zeros((F, S, rows, 4), np.float32), scores=np.zeros((F, S, rows), np.float32), lms_in=np.zeros((F, S, rows, 10), np.float32),
                counts_in=np.zeros((F, S), np.int32), dets=np.full((F, S, M, 5), 9.0, np.float32), lms=np.full((F, S, M, 10), 9.0, np.float32),
                info=np.full((F, S, M, 3), 9, np.int32), counts=np.full((F, S), 9, np.int32), flags=np.full((F, S), 9, np.int32))


ORDER = ("boxes", "scores", "lms_in", "counts_in", "dets", "lms", "info", "counts", "flags")


def _op_track_weak(o, w, S, F, rows, a, device=0):
    """(code, message) of cf_op_track_weak; a refused call has written nothing."""
    P, L = cfa._lib.ptr, cfa._lib.lib()
    keep = {k: (None if a[k] is None else a[k].copy()) for k in ORDER}
    r = L.cf_op_track_weak(device, C.byref(o) if o is not None else None, C.byref(w) if w is not None else None, S, F, rows, *[P(a[k]) for k in ORDER])
    if r != 0:
        for k in ORDER:
            assert a[k] is None or a[k].tobytes() == keep[k].tobytes(), k
    return r, (L.cf_op_last_error() or b"").decode()


@pytest.mark.parametrize("bad, rule", BAD_WEAK, ids=["%s=%r" % next(iter(b.items())) for b, _ in BAD_WEAK])
def test_bad_weak_options_are_refused_before_any_device(bad, rule):
    L = cfa._lib.lib()
    o, w = cfa._lib.track_opts(**GOOD), cfa._lib.track_weak_opts(**bad)
    r, why = _op_track_weak(o, w, 2, 2, 3, _op_args(), device=123456)           # (a device that does not exist: it is never touched)
    assert r == -1 and "cf_op_track_weak" in why and rule in why, why
    out = C.c_void_p(1234)
    assert L.cf_track_create_weak(None, 2, C.byref(o), C.byref(w), C.byref(out)) == -1 and out.value == 1234
    why = L.cf_op_last_error().decode()
    assert "cf_track_create_weak" in why and rule in why and "null context" not in why, why


def test_the_plain_options_are_checked_first_and_a_good_set_stops_at_the_context():
    L = cfa._lib.lib()
    w, out = cfa._lib.track_weak_opts(0.3, 0.5), C.c_void_p(1234)
    for bad, word in ((dict(iou=0.0), "iou_thresh"), (dict(max_age=-1), "max_age"), (dict(min_hits=0), "min_hits"), (dict(max_tracks=1025), "max_tracks"),
                      (dict(hold_grow=NAN), "hold_grow")):
        o = cfa._lib.track_opts(**dict(GOOD, **bad))
        assert L.cf_track_create_weak(None, 2, C.byref(o), C.byref(cfa._lib.track_weak_opts(NAN, NAN)), C.byref(out)) == -1
        why = L.cf_op_last_error().decode()
        assert "cf_track_create_weak" in why and word in why and "birth_score" not in why, why
        r, why = _op_track_weak(o, w, 2, 2, 3, _op_args(), device=123456)
        assert r == -1 and "cf_op_track_weak" in why and word in why, why
    o = cfa._lib.track_opts(**GOOD)
    for S in (0, 4097):
        assert L.cf_track_create_weak(None, S, C.byref(o), C.byref(w), C.byref(out)) == -1 and "n_streams" in L.cf_op_last_error().decode()
    assert L.cf_track_create_weak(None, 2, None, C.byref(w), C.byref(out)) == -1 and "null options" in L.cf_op_last_error().decode()
    assert L.cf_track_create_weak(None, 2, C.byref(o), C.byref(w), None) == -1 and "null out" in L.cf_op_last_error().decode()
    assert L.cf_track_create_weak(None, 2, C.byref(o), C.byref(w), C.byref(out)) == -1
    why = L.cf_op_last_error().decode()
    assert "cf_track_create_weak" in why and "null context" in why and out.value == 1234
    # the limits and the pointers of cf_op_track, under the new name
    for S, F, rows in ((0, 2, 3), (2, 0, 3), (2, 2, 0)):
        r, why = _op_track_weak(o, w, S, F, rows, _op_args(), device=123456)
        assert r == -1 and "cf_op_track_weak" in why, why
    for k in ORDER:
        a = _op_args()
        a[k] = None
        r, why = _op_track_weak(o, w, 2, 2, 3, a, device=123456)
        assert r == -1 and "null" in why, (k, why)
    a = _op_args()
    a["counts_in"][1, 0] = -1
    r, why = _op_track_weak(o, w, 2, 2, 3, a, device=123456)
    assert r == -1 and "negative count" in why


def test_null_weak_options_are_the_plain_calls():
    """weak == NULL gets exactly as far as cf_track_create / cf_op_track get: the same refusals under the plain names."""
    L = cfa._lib.lib()
    o, out = cfa._lib.track_opts(**GOOD), C.c_void_p(1234)
    assert L.cf_track_create_weak(None, 2, C.byref(o), None, C.byref(out)) == -1
    weak_says = L.cf_op_last_error().decode()
    assert L.cf_track_create(None, 2, C.byref(o), C.byref(out)) == -1
    assert weak_says == L.cf_op_last_error().decode() and "null context" in weak_says and out.value == 1234
    bad = cfa._lib.track_opts(**dict(GOOD, iou=2.0))
    assert L.cf_track_create_weak(None, 2, C.byref(bad), None, C.byref(out)) == -1 and "iou_thresh" in L.cf_op_last_error().decode()
    r, why = _op_track_weak(o, None, 2, 0, 3, _op_args())
    assert r == -1 and why.startswith("cf_op_track:") and "n_frames" in why


WRONG = [dict(weak_score=0.0), dict(weak_score=-0.1), dict(weak_score=0.3), dict(weak_score=0.31), dict(weak_score=NAN), dict(weak_score=0.1, birth_score=1.01),
         dict(weak_score=0.1, birth_score=NAN), dict(weak_score=0.1, birth_score=0.05), dict(weak_score=0.1, weak_iou=0.0), dict(weak_score=0.1, weak_iou=1.2),
         dict(weak_score=0.1, weak_iou=NAN)]


@pytest.mark.parametrize("bad", WRONG, ids=lambda d: ",".join("%s=%r" % kv for kv in d.items()))
def test_tracker_refuses_bad_thresholds_before_anything_is_created(bad):
    with pytest.raises(ValueError, match="weak_score < birth_score|weak_iou"):
        cfa.Tracker(0, 2, **dict(GOOD, **bad))


def test_tracker_keeps_its_thresholds_and_a_plain_one_has_none():
    t = cfa.Tracker(0, 3, weak_score=0.1, **GOOD)                           # lazily created: no device is touched here
    assert (t.weak_score, t.birth_score) == (0.1, 0.3) and round(t._wo.weak_iou, 6) == 0.5 and round(t._wo.birth_score, 6) == 0.3
    t.reset(), t.close()
    t = cfa.Tracker(0, 3, weak_score=0.05, birth_score=1.0, weak_iou=1.0, **GOOD)
    assert (t.weak_score, t.birth_score) == (0.05, 1.0)
    t.close()
    p = cfa.Tracker(0, 3, birth_score=0.7, weak_iou=0.9, **GOOD)            # without weak_score the two are not looked at
    assert p.weak_score is None and p.birth_score is None and p._wo is None
    p.close()
    with pytest.raises(ValueError):                                         # the plain options are still the library's to refuse
        cfa.Tracker(0, 2, weak_score=0.1, **dict(GOOD, max_tracks=0))
    with pytest.raises(ValueError, match="weak_iou needs birth_score"):
        cfa.ops.track_sequence(np.zeros((1, 1, 1, 4)), np.zeros((1, 1, 1)), np.zeros((1, 1, 1, 10)), np.zeros((1, 1)), weak_iou=0.5)


# ---------------------------------------------------------------------------------------------- the restatement, checked by hand
def test_restatement_a_weak_row_matches_a_confirmed_track_only():
    assert iou32(A, A2) == iou32(A2, A3) == np.float32(1645.0) / np.float32(2537.0) and iou32(A, A3) < np.float32(0.5)
    t = WeakRefTracker(1, 0.3, 0.5, iou=0.3, max_age=3, min_hits=2, max_tracks=4, hold_grow=0.1)
    z = np.zeros((1, 10))
    assert t.update(0, [A2], [WEAK], z, 1)[3] == 0 and t.next_id == [1]     # an empty tracker: discarded, no id spent
    _, _, info, fl = t.update(0, [A], [STRONG], z, 1)
    assert info.tolist() == [[1, 1, 0]] and fl == 0
    d, _, info, fl = t.update(0, [A2], [WEAK], z, 1)                        # tentative: not matched, freed at once
    assert len(d) == 0 and fl == 0
    t.update(0, [A], [STRONG], z, 1), t.update(0, [A], [STRONG], z, 1)
    d, _, info, fl = t.update(0, [A2], [WEAK], z + 7, 1)
    assert info.tolist() == [[2, 3, 0]] and fl == 2 and d[0].tolist() == list(A2) + [np.float32(WEAK)]
    d, _, info, fl = t.update(0, [A], [np.float32(0.3)], z, 1)              # IoU(A2, A) passes; score == birth_score is weak
    assert info.tolist() == [[2, 4, 0]] and fl == 2
    d, _, info, fl = t.update(0, [A3], [WEAK], z, 1)                        # IoU(A, A3) = 0.425 < weak_iou: discarded, the track is held
    assert info.tolist() == [[2, 4, 1]] and fl == 0 and d[0, 0] < A[0]


def test_restatement_with_only_strong_rows_is_track_cases():
    frames = [[[at(A, STRONG), at(A3, 0.31)]], [[at(A2, 0.5)]], [[]], [[at(A3, 0.9), at(A, 0.4)]]]
    b, s, l, c = tables(frames, 3)
    o = dict(iou=0.3, max_age=1, min_hits=1, max_tracks=2, hold_grow=0.2)
    for got, want in zip(run_weak_sequence(b, s, l, c, birth_score=0.3, weak_iou=0.5, **o), run_sequence(b, s, l, c, **o)):
        assert got.tobytes() == want.tobytes()
