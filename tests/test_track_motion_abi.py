"""The C ABI and the Python binding of the tracker with constant-velocity prediction, and hand-checked cases of its numpy restatement (no
GPU needed): every refusal comes before a device is touched and names its rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from motion_cases import A, MotionRefTracker, learn, run_motion_sequence, shifted
from track_cases import F32, RefTracker, iou32, run_sequence, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "centerface_hip.h")).read()
SYMBOLS = ("cf_track_create_ex", "cf_op_track_ex", "cf_op_follow_ex")
GOOD = dict(iou=0.3, max_age=15, min_hits=2, max_tracks=4, hold_grow=0.1)
NAN, INF = float("nan"), float("inf")
GAIN_RULE, DAMP_RULE = "gain must be finite and in (0, 1]", "damp must be finite and in [0, 1]"
BAD_MOTION = [(dict(gain=v), GAIN_RULE) for v in (0.0, -0.1, 1.0001, NAN, INF, -INF)] + \
             [(dict(damp=v), DAMP_RULE) for v in (-0.1, 1.5, NAN, INF, -INF)]


def test_symbols_exported_declared_and_bound():
    L = cfa._lib.lib()
    for s in SYMBOLS:
        assert s in cfa._lib.EXPORTS
        assert re.search(r"\bint %s\(" % s, HEADER), s
        assert hasattr(L, s) and getattr(L, s).argtypes, s
    assert len(L.cf_track_create_ex.argtypes) == 6 and len(L.cf_op_track_ex.argtypes) == 17 and len(L.cf_op_follow_ex.argtypes) == 28
    body = re.search(r"typedef struct cf_track_motion_opts \{(.*?)\} cf_track_motion_opts;", HEADER, re.S).group(1)
    assert re.findall(r"^\s*float\s+(\w+);", body, re.M) == [n for n, _ in cfa._lib.TrackMotionOpts._fields_] == ["gain", "damp"]
    assert C.sizeof(cfa._lib.TrackMotionOpts) == 8
    assert C.sizeof(cfa._lib.TrackOpts) == 20 and C.sizeof(cfa._lib.TrackWeakOpts) == 8          # the existing structs kept their layouts
    assert [n for n, _ in cfa._lib.TrackOpts._fields_] == ["iou_thresh", "max_age", "min_hits", "max_tracks", "hold_grow"]
    assert [n for n, _ in cfa._lib.TrackWeakOpts._fields_] == ["birth_score", "weak_iou"]
    o = cfa._lib.track_motion_opts()
    assert (o.gain, o.damp) == (0.5, 1.0)
    # the existing entry points kept their signatures
    assert len(L.cf_track_create.argtypes) == 4 and len(L.cf_track_create_weak.argtypes) == 5
    assert len(L.cf_op_track.argtypes) == 14 and len(L.cf_op_track_weak.argtypes) == 15 and len(L.cf_op_follow.argtypes) == 26


def test_the_statement_is_in_the_header_the_kernel_file_and_the_readme():
    kernel = open(os.path.join(ROOT, "lightweight-face-detection-centernet_amd", "csrc", "cf_track.hip")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (HEADER, kernel):
        for phrase in ("16777216 (2^24)", "P = (o.x1 + vx, o.y1 + vy, o.x2 + vx,", "rx = (cdx - cox) - vx", "a = hb == 1 ? 1.0f : gain",
                       "vx' = vx + a * (rx / (float)(g + 1))", "COASTS", "vel = (vx * damp, vy * damp)", "tpl_id == id", "vel = (0, 0)",
                       "cannot bootstrap", "size is not predicted", "max_age * v", "nobody has measured", "no accuracy claim", "88 bytes"):
            assert phrase in text, phrase
    assert "constant velocity" in HEADER and "cf_track_motion_opts" in HEADER
    assert "track_update_kernel<true, true>" in kernel and "track_update_kernel<false, false>" in kernel
    for text in (readme, design):
        assert "motion" in text and "nobody has measured" in text and "no accuracy claim" in text
    assert "cannot bootstrap" in readme and "Tracker(motion=" in readme


def _op_args(S=2, F=2, rows=3, M=4):
    return dict(boxes=np.zeros((F, S, rows, 4), np.float32), scores=np.zeros((F, S, rows), np.float32), lms_in=np.zeros((F, S, rows, 10), np.float32),
                counts_in=np.zeros((F, S), np.int32), dets=np.full((F, S, M, 5), 9.0, np.float32), lms=np.full((F, S, M, 10), 9.0, np.float32),
                info=np.full((F, S, M, 3), 9, np.int32), counts=np.full((F, S), 9, np.int32), flags=np.full((F, S), 9, np.int32),
                vel=np.full((F, S, M, 2), 9.0, np.float32))


ORDER = ("boxes", "scores", "lms_in", "counts_in", "dets", "lms", "info", "counts", "flags", "vel")


def _ref(x):
    return C.byref(x) if x is not None else None


def _op_track_ex(o, w, m, S, F, rows, a, device=0):
    """(code, message) of cf_op_track_ex; a refused call has written nothing."""
    P, L = cfa._lib.ptr, cfa._lib.lib()
    keep = {k: (None if a[k] is None else a[k].copy()) for k in ORDER}
    r = L.cf_op_track_ex(device, _ref(o), _ref(w), _ref(m), S, F, rows, *[None if a[k] is None else P(a[k]) for k in ORDER])
    if r != 0:
        for k in ORDER:
            assert a[k] is None or a[k].tobytes() == keep[k].tobytes(), k
    return r, (L.cf_op_last_error() or b"").decode()


def _op_follow_ex(o, w, m, fo, S=1, F=1, rows=2, M=4, h=32, wd=32, device=0):
    """(code, message) of cf_op_follow_ex on black BGR frames; a refused call has written nothing."""
    P, L = cfa._lib.ptr, cfa._lib.lib()
    a = _op_args(S, F, rows, M)
    moves, detect = np.full((F, S, M, 4), 9, np.int32), np.ones(F, np.uint8)
    frames = np.zeros((F * S, h, wd, 3), np.uint8)
    tab, B, fh, fw, p0, p1, keep_alive = cfa._lib.frame_planes(frames, "bgr", writable=False)
    outs = [a[k] for k in ("dets", "lms", "info", "counts", "flags")] + [moves]
    keep = [x.copy() for x in outs]
    r = L.cf_op_follow_ex(device, _ref(o), _ref(w), _ref(m), _ref(fo), S, F, rows, P(a["boxes"]), P(a["scores"]), P(a["lms_in"]), P(a["counts_in"]), P(detect),
                          cfa._lib.frame_format("bgr"), tab, fh, fw, p0, p1, fh, fw, 0, *[P(x) for x in outs])
    del keep_alive
    if r != 0:
        for x, k in zip(outs, keep):
            assert x.tobytes() == k.tobytes()
    return r, (L.cf_op_last_error() or b"").decode()


@pytest.mark.parametrize("bad, rule", BAD_MOTION, ids=["%s=%r" % next(iter(b.items())) for b, _ in BAD_MOTION])
def test_bad_motion_options_are_refused_before_any_device(bad, rule):
    L = cfa._lib.lib()
    o, w, m = cfa._lib.track_opts(**GOOD), cfa._lib.track_weak_opts(), cfa._lib.track_motion_opts(**bad)
    for weak in (None, w):
        r, why = _op_track_ex(o, weak, m, 2, 2, 3, _op_args(), device=123456)       # (a device that does not exist: it is never touched)
        assert r == -1 and "cf_op_track_ex" in why and rule in why, why
        r, why = _op_follow_ex(o, weak, m, cfa._lib.follow_opts(), device=123456)
        assert r == -1 and "cf_op_follow_ex" in why and rule in why, why
        out = C.c_void_p(1234)
        assert L.cf_track_create_ex(None, 2, C.byref(o), _ref(weak), C.byref(m), C.byref(out)) == -1 and out.value == 1234
        why = L.cf_op_last_error().decode()
        assert "cf_track_create_ex" in why and rule in why and "null context" not in why, why


def test_damp_zero_and_the_ends_of_the_ranges_are_good():
    L = cfa._lib.lib()
    o, out = cfa._lib.track_opts(**GOOD), C.c_void_p(1234)
    for gain, damp in ((0.5, 0.0), (1.0, 1.0), (1e-6, 0.5)):
        m = cfa._lib.track_motion_opts(gain, damp)
        assert L.cf_track_create_ex(None, 2, C.byref(o), None, C.byref(m), C.byref(out)) == -1
        why = L.cf_op_last_error().decode()
        assert "cf_track_create_ex" in why and "null context" in why and out.value == 1234, why


def test_the_plain_and_the_weak_options_are_checked_first():
    L = cfa._lib.lib()
    out, badm = C.c_void_p(1234), cfa._lib.track_motion_opts(NAN, NAN)
    w = cfa._lib.track_weak_opts(0.3, 0.5)
    for bad, word in ((dict(iou=0.0), "iou_thresh"), (dict(max_age=-1), "max_age"), (dict(min_hits=0), "min_hits"), (dict(max_tracks=1025), "max_tracks"),
                      (dict(hold_grow=NAN), "hold_grow")):
        o = cfa._lib.track_opts(**dict(GOOD, **bad))
        assert L.cf_track_create_ex(None, 2, C.byref(o), C.byref(cfa._lib.track_weak_opts(NAN, NAN)), C.byref(badm), C.byref(out)) == -1
        why = L.cf_op_last_error().decode()
        assert "cf_track_create_ex" in why and word in why and "birth_score" not in why and "gain" not in why, why
        r, why = _op_track_ex(o, w, badm, 2, 2, 3, _op_args(), device=123456)
        assert r == -1 and "cf_op_track_ex" in why and word in why and "gain" not in why, why
    o = cfa._lib.track_opts(**GOOD)
    for badw, word in ((cfa._lib.track_weak_opts(NAN, 0.5), "birth_score"), (cfa._lib.track_weak_opts(0.3, 0.0), "weak_iou")):
        assert L.cf_track_create_ex(None, 2, C.byref(o), C.byref(badw), C.byref(badm), C.byref(out)) == -1
        why = L.cf_op_last_error().decode()
        assert "cf_track_create_ex" in why and word in why and "gain" not in why, why
        r, why = _op_track_ex(o, badw, badm, 2, 2, 3, _op_args(), device=123456)
        assert r == -1 and word in why and "gain" not in why, why
        r, why = _op_follow_ex(o, badw, badm, cfa._lib.follow_opts(), device=123456)
        assert r == -1 and "cf_op_follow_ex" in why and word in why and "gain" not in why, why
    # gain before damp, the motion options before the follower's
    r, why = _op_track_ex(o, None, badm, 2, 2, 3, _op_args(), device=123456)
    assert r == -1 and GAIN_RULE in why
    r, why = _op_follow_ex(o, None, cfa._lib.track_motion_opts(0.5, 2.0), cfa._lib.follow_opts(search=0), device=123456)
    assert r == -1 and DAMP_RULE in why and "search" not in why, why
    r, why = _op_follow_ex(o, None, cfa._lib.track_motion_opts(), cfa._lib.follow_opts(search=0), device=123456)
    assert r == -1 and "cf_op_follow_ex" in why and "search" in why, why
    m = cfa._lib.track_motion_opts()
    for S in (0, 4097):
        assert L.cf_track_create_ex(None, S, C.byref(o), None, C.byref(m), C.byref(out)) == -1 and "n_streams" in L.cf_op_last_error().decode()
    assert L.cf_track_create_ex(None, 2, None, None, C.byref(m), C.byref(out)) == -1 and "null options" in L.cf_op_last_error().decode()
    assert L.cf_track_create_ex(None, 2, C.byref(o), None, C.byref(m), None) == -1 and "null out" in L.cf_op_last_error().decode()
    # the limits and the pointers of cf_op_track, under the new name; vel alone may be NULL
    for S, F, rows in ((0, 2, 3), (2, 0, 3), (2, 2, 0)):
        r, why = _op_track_ex(o, None, m, S, F, rows, _op_args(), device=123456)
        assert r == -1 and "cf_op_track_ex" in why, why
    for k in ORDER[:-1]:
        a = _op_args()
        a[k] = None
        r, why = _op_track_ex(o, None, m, 2, 2, 3, a, device=123456)
        assert r == -1 and "null" in why, (k, why)
    a = _op_args()
    a["counts_in"][1, 0] = -1
    r, why = _op_track_ex(o, None, m, 2, 2, 3, a, device=123456)
    assert r == -1 and "negative count" in why


def test_null_motion_options_are_the_calls_without_them():
    """motion == NULL gets exactly as far as cf_track_create_weak / cf_op_track_weak / cf_op_track / cf_op_follow get: their refusals,
    verbatim, under their names."""
    L = cfa._lib.lib()
    o, w, out = cfa._lib.track_opts(**GOOD), cfa._lib.track_weak_opts(), C.c_void_p(1234)
    for weak in (None, w):
        assert L.cf_track_create_ex(None, 2, C.byref(o), _ref(weak), None, C.byref(out)) == -1
        ex_says = L.cf_op_last_error().decode()
        assert L.cf_track_create_weak(None, 2, C.byref(o), _ref(weak), C.byref(out)) == -1
        assert ex_says == L.cf_op_last_error().decode() and "null context" in ex_says and out.value == 1234
        assert ex_says.startswith("cf_track_create_weak:" if weak is not None else "cf_track_create:")
    badw = cfa._lib.track_weak_opts(0.0, 0.5)
    assert L.cf_track_create_ex(None, 2, C.byref(o), C.byref(badw), None, C.byref(out)) == -1
    why = L.cf_op_last_error().decode()
    assert why.startswith("cf_track_create_weak:") and "birth_score must be finite and in (0, 1]" in why
    bad = cfa._lib.track_opts(**dict(GOOD, iou=2.0))
    assert L.cf_track_create_ex(None, 2, C.byref(bad), None, None, C.byref(out)) == -1
    assert L.cf_op_last_error().decode().startswith("cf_track_create:") and "iou_thresh" in L.cf_op_last_error().decode()
    r, why = _op_track_ex(o, None, None, 2, 0, 3, _op_args())
    assert r == -1 and why.startswith("cf_op_track:") and "n_frames" in why
    r, why = _op_track_ex(o, w, None, 2, 0, 3, _op_args())
    assert r == -1 and why.startswith("cf_op_track_weak:") and "n_frames" in why
    r, why = _op_track_ex(o, badw, None, 2, 2, 3, _op_args(), device=123456)
    assert r == -1 and why.startswith("cf_op_track_weak:") and "birth_score" in why
    r, why = _op_follow_ex(o, None, None, cfa._lib.follow_opts(search=0), device=123456)
    assert r == -1 and why.startswith("cf_op_follow:") and "search" in why, why


WRONG = [dict(gain=0.0), dict(gain=-0.5), dict(gain=1.5), dict(gain=NAN), dict(gain=INF), dict(damp=-0.1), dict(damp=1.1), dict(damp=NAN), dict(damp=-INF),
         dict(speed=1.0), dict(gain=0.5, dampen=0.5), "yes", 1.5, (0.5, 1.0)]


@pytest.mark.parametrize("bad", WRONG, ids=repr)
def test_tracker_refuses_bad_motion_before_anything_is_created(bad):
    with pytest.raises(ValueError, match="gain|damp|motion"):
        cfa.Tracker(0, 2, motion=bad, **GOOD)


def test_tracker_keeps_its_motion_and_a_plain_one_has_none():
    t = cfa.Tracker(0, 3, motion=True, **GOOD)                              # lazily created: no device is touched here
    assert t.motion == dict(gain=0.5, damp=1.0) and t._wo is None and (t._mo.gain, t._mo.damp) == (0.5, 1.0)
    t.reset(), t.close()
    t = cfa.Tracker(0, 3, motion=dict(damp=0.0), weak_score=0.1, **GOOD)
    assert t.motion == dict(gain=0.5, damp=0.0) and t.weak_score == 0.1 and t._wo is not None
    t.close()
    t = cfa.Tracker(0, 3, motion=dict(gain=1.0, damp=0.25), **GOOD)
    assert t.motion == dict(gain=1.0, damp=0.25)
    t.close()
    for none in (None, False):
        p = cfa.Tracker(0, 3, motion=none, **GOOD)
        assert p.motion is None and p._mo is None
        p.close()
    with pytest.raises(ValueError):                                         # the plain options are still the library's to refuse
        cfa.Tracker(0, 2, motion=True, **dict(GOOD, max_tracks=0))
    z = (np.zeros((1, 1, 1, 4)), np.zeros((1, 1, 1)), np.zeros((1, 1, 1, 10)), np.zeros((1, 1)))
    with pytest.raises(ValueError, match="unknown keys"):
        cfa.ops.track_sequence(*z, motion=dict(speed=2))
    with pytest.raises(ValueError, match="motion"):
        cfa.ops.follow_sequence(*z, np.zeros((1, 32, 32, 3), np.uint8), motion="on")


def test_a_plain_tracker_calls_what_it_called_before(monkeypatch):
    """``_make`` reaches cf_track_create_ex only when motion is set."""
    calls = []

    class Spy(object):
        def __init__(self, L):
            self._L = L

        def __getattr__(self, name):
            f = getattr(self._L, name)
            if name.startswith("cf_track_create"):
                def g(*a):
                    calls.append(name)
                    return f(*a)
                return g
            return f

    spy = Spy(cfa._lib.lib())
    for kw, want in ((dict(), "cf_track_create"), (dict(weak_score=0.1), "cf_track_create_weak"), (dict(motion=True), "cf_track_create_ex"),
                     (dict(motion=dict(gain=0.25), weak_score=0.1), "cf_track_create_ex")):
        t = cfa.Tracker(0, 2, **dict(GOOD, **kw))
        t._L = spy
        del calls[:]
        assert t._make(None, C.c_void_p()) == -1
        assert calls == [want], (kw, calls)
        t.close()


# ---------------------------------------------------------------------------------------------- the restatement, checked by hand
OPTS = dict(iou=0.3, max_age=15, min_hits=2, max_tracks=4, hold_grow=0.0)


@pytest.mark.parametrize("gain", [0.5, 1.0, 0.125])
def test_restatement_a_dropout_is_held_where_the_face_went(gain):
    assert iou32(A, shifted(A, 20)) == F32(1071.0) / F32(3111.0)
    t = MotionRefTracker(1, gain=gain, damp=1.0, **OPTS)
    z = np.zeros((1, 10))
    _, _, info, fl = t.update(0, [A], [0.9], z, 1)
    assert info.tolist() == [[1, 1, 0]] and fl == 0 and t.out_vel.tolist() == [[0.0, 0.0]]
    d, _, info, _ = t.update(0, [shifted(A, 20)], [0.9], z, 1)
    assert info.tolist() == [[1, 2, 0]] and t.out_vel.tolist() == [[20.0, 0.0]] and d[0, :4].tolist() == list(shifted(A, 20))
    d, l, info, _ = t.update(0, np.zeros((0, 4)), [], np.zeros((0, 10)), 0)
    assert info.tolist() == [[1, 2, 1]] and d[0, :4].tolist() == list(shifted(A, 40)) and t.out_vel.tolist() == [[20.0, 0.0]]
    assert l[0].tolist() == [20.0, 0.0] * 5                                 # the landmarks coast with the box
    d, _, info, _ = t.update(0, [shifted(A, 60)], [0.9], z, 1)
    assert info.tolist() == [[1, 3, 0]] and t.out_vel.tolist() == [[20.0, 0.0]] and t.next_id == [2]
    # the tracker without the model holds A+20 and spends id 2
    p = RefTracker(1, **OPTS)
    p.update(0, [A], [0.9], z, 1), p.update(0, [shifted(A, 20)], [0.9], z, 1)
    d, _, info, _ = p.update(0, np.zeros((0, 4)), [], np.zeros((0, 10)), 0)
    assert info.tolist() == [[1, 2, 1]] and d[0, :4].tolist() == list(shifted(A, 20))
    _, _, info, _ = p.update(0, [shifted(A, 60)], [0.9], z, 1)
    assert sorted(info[:, 0].tolist()) == [1, 2] and p.next_id == [3]


def test_restatement_gain_divides_the_residual_by_the_frames_since():
    assert learn(F32(0), 1020, 1060, 1000, 1040, 0, 1, F32(0.25)) == F32(20)              # the second sighting: taken whole
    assert learn(F32(20), 1050, 1090, 1020, 1060, 0, 2, F32(0.25)) == F32(22.5)           # then a quarter of the residual 10
    third = F32(F32(10) / F32(3))
    assert learn(F32(20), 1050, 1090, 1020, 1060, 2, 5, F32(1.0)) == F32(F32(20) + third)   # g = 2: / 3, rounded before the product
    assert learn(F32(20), 1050, 1090, 1020, 1060, 2, 5, F32(0.3)) == F32(F32(20) + F32(F32(0.3) * third))


def test_restatement_stationary_faces_are_the_plain_tracker():
    frames = [[[A, shifted(A, 100)]], [[A]], [[]], [[shifted(A, 100), A]], [[]], [[]], [[A]]]
    b, s, l, c = tables(frames, 3)
    o = dict(iou=0.3, max_age=1, min_hits=1, max_tracks=3, hold_grow=0.2)
    got = run_motion_sequence(b, s, l, c, motion=dict(gain=0.5, damp=0.5), **o)
    for g, want in zip(got[:5], run_sequence(b, s, l, c, **o)):
        assert g.tobytes() == want.tobytes()
    assert not got[5].any()
