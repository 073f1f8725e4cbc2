"""The lookback's C ABI and Python binding, the hand-checked cases of its numpy restatement, and the delay line of the product paths against
a stand-in engine (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from lookback_cases import CUT, SAME, RefLookback, face_box, grown, run_lookback, tracked_tables
from test_product_paths import BGR, H, MOSAIC, W, YUV, StubEngine, Script, make_face

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "centerface_hip.h")).read()
SYMBOLS = ("cf_lookback_create", "cf_lookback_destroy", "cf_lookback_forget", "cf_lookback_step", "cf_op_lookback")


def test_symbols_exported_declared_and_bound():
    L = cfa._lib.lib()
    for s in SYMBOLS:
        assert s in cfa._lib.EXPORTS
        assert re.search(r"\bint %s\(" % s, HEADER), s
        assert hasattr(L, s) and getattr(L, s).argtypes, s
    assert re.search(r"typedef struct cf_lookback cf_lookback;", HEADER)
    assert len(L.cf_lookback_step.argtypes) == 13 and len(L.cf_op_lookback.argtypes) == 16
    assert callable(cfa.ops.lookback_sequence)
    for name in ("lookback_step", "lookback_step_device"):
        assert callable(getattr(cfa.Engine, name))
    for name in ("forget", "close", "_handle"):
        assert callable(getattr(cfa.Lookback, name))
    assert "Lookback" in cfa.__all__


def test_lookback_opts_agree_with_the_header():
    body = re.search(r"typedef struct cf_lookback_opts \{(.*?)\} cf_lookback_opts;", HEADER, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|float)\s+(\w+);", body, re.M)
    assert [(n, C.c_int32 if t == "int32_t" else C.c_float) for t, n in fields] == list(cfa._lib.LookbackOpts._fields_)
    assert [n for _, n in fields] == ["depth", "rows", "grow", "confirm"]
    assert C.sizeof(cfa._lib.LookbackOpts) == 16
    o = cfa._lib.lookback_opts()
    assert (o.depth, o.rows, o.confirm) == (8, 256, 1) and o.grow == np.float32(0.05)
    sig = inspect.signature(cfa.Lookback.__init__)
    assert [(k, p.default) for k, p in sig.parameters.items()][2:] == [("streams", inspect.Parameter.empty), ("depth", 8), ("rows", 256), ("grow", 0.05),
                                                                         ("confirm", 1)]


def test_makefile_builds_the_kernel_without_contraction():
    mk = open(os.path.join(ROOT, "lightweight-face-detection-centernet_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "cf_lookback.hip" in srcs and re.search(r"EXTRA_cf_lookback\s*=\s*-ffp-contract=off", mk)


def test_the_documents_state_the_limits_and_make_no_accuracy_claim():
    for name in ("README.md", os.path.join("include", "centerface_hip.h")):
        text = open(os.path.join(ROOT, name)).read()
        at = text.find("cf_lookback_step")
        assert at >= 0, name
        near = text[max(0, at - 8000):at + 8000]
        for word in ("no accuracy claim", "NOT COVERED", "not moved"):
            assert word in near, (name, word)
    prof = open(os.path.join(ROOT, "profiles", "lookback.md")).read()
    assert "tools/lookback_probe.py" in prof and "cf_lookback_step" in prof


# ---------------------------------------------------------------------------------------------- refusals
CREATE_REFUSALS = [((0, 4, 0.05, 1), 2, "depth"), ((33, 4, 0.05, 1), 2, "depth"), ((2, 0, 0.05, 1), 2, "rows"), ((2, 1025, 0.05, 1), 2, "rows"),
                   ((2, 4, -0.01, 1), 2, "grow"), ((2, 4, 1.01, 1), 2, "grow"), ((2, 4, float("nan"), 1), 2, "grow"), ((2, 4, float("inf"), 1), 2, "grow"),
                   ((2, 4, 0.05, 0), 2, "confirm"), ((2, 4, 0.05, 4), 2, "confirm"), ((2, 4, 0.05, 1), 0, "n_streams"), ((2, 4, 0.05, 1), 4097, "n_streams")]


@pytest.mark.parametrize("opts, S, word", CREATE_REFUSALS, ids=[w + str(i) for i, (_, _, w) in enumerate(CREATE_REFUSALS)])
def test_create_and_op_refuse_bad_options_before_any_device(opts, S, word):
    L = cfa._lib.lib()
    h = C.c_void_p()
    o = cfa._lib.lookback_opts(*opts)
    assert L.cf_lookback_create(None, S, C.byref(o), C.byref(h)) == -1 and h.value is None
    why = L.cf_op_last_error().decode()
    assert "cf_lookback_create" in why and word in why and "null context" not in why, why
    with pytest.raises(ValueError):
        cfa.Lookback(0, S, *opts)
    r, why = _op(opts=opts, S=S)
    assert r == -1 and "cf_op_lookback" in why and word in why, why


def _op(opts=(2, 4, 0.05, 1), S=2, F=3, rows_in=4, null=None, null_opts=False):
    L = cfa._lib.lib()
    o = cfa._lib.lookback_opts(*opts)
    n, R = min(max(F, 1) * max(S, 1), 8), min(max(opts[1], 1), 8)      # (a refusal touches no table: small ones will do)
    a = dict(push=np.ones(max(F, 1), np.uint8), dets_in=np.zeros((n, max(rows_in, 1), 5), np.float32), lms_in=np.zeros((n, max(rows_in, 1), 10), np.float32),
             info_in=np.zeros((n, max(rows_in, 1), 3), np.int32), counts_in=np.zeros(n, np.int32), cuts=np.zeros(n, np.int32),
             dets=np.full((n, R, 5), 9, np.float32), lms=np.full((n, R, 10), 9, np.float32), info=np.full((n, R, 3), 9, np.int32),
             counts=np.full(n, 9, np.int32), state=np.full((n, 4), 9, np.int32))
    p = {k: (None if k == null else cfa._lib.ptr(v)) for k, v in a.items()}
    r = L.cf_op_lookback(0, None if null_opts else C.byref(o), S, F, rows_in, p["push"], p["dets_in"], p["lms_in"], p["info_in"], p["counts_in"], p["cuts"],
                         p["dets"], p["lms"], p["info"], p["counts"], p["state"])
    for k in ("dets", "lms", "info", "counts", "state"):
        assert (a[k] == 9).all()                                             # refused: nothing was written
    return r, (L.cf_op_last_error() or b"").decode()


def test_cf_op_lookback_refuses_counts_and_null_arguments():
    for kw, word in ((dict(F=0), "n_steps"), (dict(rows_in=0), "rows_in"), (dict(rows_in=5), "rows_in"), (dict(null_opts=True), "null options"),
                     (dict(opts=(2, 1024, 0.05, 1), S=4096, F=5), "2^24")) + tuple(
                         (dict(null=k), "null argument") for k in ("push", "dets_in", "lms_in", "info_in", "counts_in", "dets", "lms", "info", "counts", "state")):
        r, why = _op(**kw)
        assert r == -1 and "cf_op_lookback" in why and word in why, (kw, why)


def test_step_forget_and_destroy_check_their_arguments_before_the_context():
    L = cfa._lib.lib()
    st = np.full((1, 4), 9, np.int32)
    for B, word in ((0, "B must be"), (-3, "B must be"), (1, "null context")):
        assert L.cf_lookback_step(None, None, 0, B, 1, None, 0, None, None, None, None, cfa._lib.ptr(st), 0) == -1
        why = L.cf_op_last_error().decode()
        assert "cf_lookback_step" in why and word in why and (word == "null context" or "null context" not in why), why
        assert (st == 9).all()
    h = C.c_void_p()
    o = cfa._lib.lookback_opts()
    assert L.cf_lookback_create(None, 2, None, C.byref(h)) == -1 and "null options" in L.cf_op_last_error().decode()
    assert L.cf_lookback_create(None, 2, C.byref(o), None) == -1 and "null out" in L.cf_op_last_error().decode()
    assert L.cf_lookback_create(None, 2, C.byref(o), C.byref(h)) == -1 and "null context" in L.cf_op_last_error().decode()
    assert L.cf_lookback_forget(None, 0) == -1 and "cf_lookback_forget" in L.cf_op_last_error().decode() and L.cf_lookback_destroy(None) == 0
    lb = cfa.Lookback(0, 3)                                                 # no engine yet: nothing is created, the range is checked
    lb.forget(2)
    lb.forget()
    with pytest.raises(ValueError):
        lb.forget(3)
    assert [lb.fill(k) for k in range(3)] == [0, 0, 0]
    lb.close()


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_grown_coordinates_by_hand():
    # centre (20, 40), half sides (10, 20); g = 1 + 2 * 0.25 = 1.5 exactly: half sides 15 and 30
    assert grown((10.0, 20.0, 30.0, 60.0), 0.25, 2).tolist() == [5.0, 10.0, 35.0, 70.0]
    assert grown((10.0, 20.0, 30.0, 60.0), 0.25, 0).tolist() == [10.0, 20.0, 30.0, 60.0]
    assert grown((10.0, 20.0, 30.0, 60.0), 0.0, 7).tolist() == [10.0, 20.0, 30.0, 60.0]
    # grow = float32(0.05) = 0.0500000007450580596923828125; j = 3; box (1.5, 2.25, 4.0, 9.75): every step in float64, one rounding at the end
    g = 1.0 + 0.0500000007450580596923828125 * 3.0
    want = [np.float32(2.75 - 1.25 * g), np.float32(6.0 - 3.75 * g), np.float32(2.75 + 1.25 * g), np.float32(6.0 + 3.75 * g)]
    got = grown((1.5, 2.25, 4.0, 9.75), 0.05, 3)
    assert got.dtype == np.float32 and got.tolist() == [float(v) for v in want]
    assert abs(float(got[0]) - 1.3125) < 1e-6 and abs(float(got[3]) - 10.3125) < 1e-6      # 2.75 -+ 1.4375, 6 -+ 4.3125


def test_a_face_born_at_frame_3_is_painted_into_frames_1_and_2_at_depth_2():
    a, b = face_box(0), face_box(5)
    frames = [[[(1, a)]], [[(1, a)]], [[(1, a), (2, b)]], [[(1, a), (2, b)]], [[(1, a)]], [[]], [[]]]      # frames 1..5 (id 2 is born at frame 3), two drains
    d, l, i, c = tracked_tables(frames, 3)
    grow = 0.25
    od, ol, oi, oc, st = run_lookback(d, l, i, c, push=[1, 1, 1, 1, 1, 0, 0], depth=2, rows=4, grow=grow)
    assert st[:, 0, 0].tolist() == [-1, -1, 0, 1, 2, 3, 4] and oc[:, 0].tolist() == [0, 0, 2, 2, 2, 2, 1]
    # step 3 emits frame 1: its own row, then id 2 from two frames ahead, grown by 1 + 2 * grow, info = id, 0, 2
    assert st[2, 0].tolist() == [0, 1, 1, 0]
    assert od[2, 0, 0].tobytes() == d[0, 0, 0].tobytes() and oi[2, 0, 0].tolist() == [1, 1, 0]
    bx = np.asarray(b, np.float32).astype(np.float64)
    cx, cy, hw, hh = (bx[0] + bx[2]) * 0.5, (bx[1] + bx[3]) * 0.5, (bx[2] - bx[0]) * 0.5 * 1.5, (bx[3] - bx[1]) * 0.5 * 1.5
    assert od[2, 0, 1, :4].tolist() == [float(np.float32(v)) for v in (cx - hw, cy - hh, cx + hw, cy + hh)]
    assert od[2, 0, 1, 4] == d[2, 0, 1, 4] and ol[2, 0, 1].tobytes() == l[2, 0, 1].tobytes()      # score and landmarks of the birth frame, as stored
    assert oi[2, 0, 1].tolist() == [2, 0, 2]
    # step 4 emits frame 2: the birth is one frame ahead, grown by 1 + grow
    assert st[3, 0].tolist() == [1, 1, 1, 0] and oi[3, 0, 1].tolist() == [2, 0, 1]
    assert od[3, 0, 1, :4].tolist() == grown(b, grow, 1).tolist()
    # frame 3 holds id 2 itself: nothing is painted back, in it or after it
    assert st[4, 0].tolist() == [2, 2, 0, 0] and st[5, 0].tolist() == [3, 2, 0, 0] and st[6, 0].tolist() == [4, 1, 0, 0]
    assert (od[0] == 0).all() and (od[2, 0, 2:] == 0).all()                  # nothing was written where nothing is due


def _pusher(ref):
    def push(rows, code=None):
        d, l, i, n = tracked_tables([[rows]], 3)
        return ref.step(0, True, d[0, 0], l[0, 0], i[0, 0], n[0, 0], code)
    return push


def test_cuts_forget_confirm_and_capacity_by_hand():
    a, b, c3 = face_box(0), face_box(1), face_box(2)
    ref = RefLookback(1, depth=2, rows=3, grow=0.0, confirm=1)
    push = _pusher(ref)
    push([(1, a)], SAME), push([(1, a)], SAME)
    dets, _, _, state = push([(1, a), (2, b)], CUT)                         # frame 3, the birth frame, starts another scene: frame 1 stays as it is
    assert state.tolist() == [0, 1, 0, 0] and len(dets) == 1
    assert push([(1, a), (2, b), (3, c3)], SAME)[3].tolist() == [1, 1, 0, 0]      # frame 2: stopped by the cut right behind it
    _, _, info, state = push([(3, c3)], SAME)                               # frame 3: the cut on the emitted entry itself stops nothing
    assert state.tolist() == [2, 2, 1, 0] and info.tolist() == [[1, 1, 0], [2, 1, 0], [3, 0, 1]]
    ref.forget(0)
    assert push([(4, a)], SAME)[3].tolist() == [3, 3, 0, 0]                 # frame 6 is pushed behind a forget: it counts as a cut
    assert push([(4, a)], SAME)[3].tolist() == [4, 1, 0, 0]                 # ... so frame 5 does not get id 4 from it
    assert push([], SAME)[3].tolist() == [5, 1, 0, 0]                       # frame 6 itself: id 4 is its own, frame 7 has nothing new
    assert ref.step(0, False)[3].tolist() == [6, 1, 0, 0] and ref.step(0, False)[3].tolist() == [7, 0, 0, 0]      # the drain
    assert ref.step(0, False)[3].tolist() == [-1, 0, 0, 0]
    # capacity: the own rows fill rows = 2, the eligible row is dropped and bit 0 says so
    ref = RefLookback(1, depth=1, rows=2, grow=0.0)
    push = _pusher(ref)
    push([(1, a), (2, b)])
    _, _, info, state = push([(3, c3)])
    assert state.tolist() == [0, 2, 0, 1] and info[:, 0].tolist() == [1, 2]
    # confirm = 2: an id must show in two of the queued frames, and a cut between the two ends the count
    for code, want in ((None, 1), (CUT, 0)):
        ref = RefLookback(1, depth=3, rows=4, grow=0.0, confirm=2)
        push = _pusher(ref)
        push([]), push([(7, a)]), push([])
        assert push([(7, a)], code)[3].tolist() == [0, 0, want, 0]
    ref = RefLookback(1, depth=3, rows=4, grow=0.0, confirm=2)
    push = _pusher(ref)
    push([]), push([(7, a)]), push([])
    assert push([])[3].tolist() == [0, 0, 0, 0]                             # seen once (the flicker of a false alarm): not painted back
    # a non-finite corner is never painted back; a negative count is an empty frame
    ref = RefLookback(1, depth=1, rows=4, grow=0.0)
    push = _pusher(ref)
    push([])
    assert push([(1, (1.0, float("nan"), 5.0, 6.0)), (2, a)])[3].tolist() == [0, 0, 1, 0]
    d, l, i, _ = tracked_tables([[[(3, a)]]], 3)
    assert ref.step(0, True, d[0, 0], l[0, 0], i[0, 0], -4)[3].tolist() == [1, 2, 0, 0] and ref.queue[0][0].n == 0


def test_lookback_and_flush_are_defaults_of_the_four_methods():
    for name in ("anonymize", "anonymize_yuv", "annotate", "annotate_yuv"):
        p = inspect.signature(getattr(cfa.CenterFace, name)).parameters
        assert p["lookback"].default is None and p["flush"].default is False, name
        assert p["lookback"].kind == p["flush"].kind == inspect.Parameter.KEYWORD_ONLY
    face = make_face((H, W), StubEngine(Script()))
    imgs = [np.zeros(BGR, np.uint8)] * 2
    with pytest.raises(ValueError):
        face.anonymize(imgs, lookback=cfa.Lookback(0, 2), **MOSAIC)          # needs tracker=
    with pytest.raises(ValueError):
        face.anonymize(imgs, flush=True, **MOSAIC)                          # needs lookback=
    with pytest.raises(ValueError):
        face.anonymize(imgs * 2, tracker=TRK, lookback=cfa.Lookback(0, 3), **MOSAIC)      # four images, three streams
    assert face.engine.s.log == []


# ---------------------------------------------------------------------------------------------- the delay line against a stand-in engine
TRK = object()


class LookbackStub(StubEngine):
    """The stand-in of test_product_paths plus ``lookback_step``: every stream emits the sequence number of what it was pushed ``depth``
    steps ago, with one row whose first value names (stream, seq)."""

    def __init__(self, script, lb, **kw):
        super().__init__(script, **kw)
        self.pushed, self.lb = {}, lb

    def track_update_device(self, tracker, stream0=0):
        self._log("track_update_device", tracker is TRK, stream0)

    def lookback_step(self, lb, stream0=0, B=None, push=True, scene=None):
        assert lb is self.lb
        self._log("lookback_step", stream0, B, push, scene)
        dets, lms, info = np.zeros((B, lb.rows, 5), np.float32), np.zeros((B, lb.rows, 10), np.float32), np.zeros((B, lb.rows, 3), np.int32)
        counts, state = np.zeros(B, np.int32), np.zeros((B, 4), np.int32)
        for b in range(B):
            q = self.pushed.setdefault(stream0 + b, [0, 0])                  # next seq to push, next seq to emit
            q[0] += 1 if push else 0
            if (q[0] - q[1] == lb.depth + 1) if push else (q[0] > q[1]):
                state[b], counts[b], dets[b, 0, 0] = (q[1], 1, 0, 0), 1, 100 * (stream0 + b) + q[1]
                q[1] += 1
            else:
                state[b, 0] = -1
        self.B = B
        return dets, lms, info, counts, state

    def cover_faces(self, frames, fmt="bgr", **options):
        self._log("cover_faces", frames.shape, fmt, options)
        frames.reshape(len(frames), -1)[:, 0] ^= 0xFF                       # a mark in every frame it is given
        return frames

    def draw_faces(self, frames, fmt="bgr", **options):
        self._log("draw_faces", frames.shape, fmt)
        frames.reshape(len(frames), -1)[:, 1] ^= 0xFF
        return frames


@pytest.mark.parametrize("method, shape", (("anonymize", BGR), ("anonymize_yuv", YUV), ("annotate", BGR), ("annotate_yuv", YUV)))
def test_delay_line_warm_up_steady_state_and_flush(method, shape):
    depth, S = 2, 3                                                          # three streams through max_batch = 2: chunks at 0 and 2
    lb = cfa.Lookback(0, S, depth=depth, rows=4)
    eng = LookbackStub(Script(), lb)
    hw = shape[:2] if len(shape) == 3 else (shape[0] * 2 // 3, shape[1])
    face = make_face(hw, eng)
    call = getattr(face, method)
    kw = dict(MOSAIC) if method.startswith("anonymize") else {}
    rng = np.random.default_rng(4)
    video = rng.integers(0, 256, (5, S) + shape, dtype=np.uint8)             # frame t of stream k
    keep = video.copy()
    mark = 0 if method.startswith("anonymize") else 1
    got = [[] for _ in range(S)]
    for t in range(5):
        eng.s.next, n0 = 0, len(eng.s.log)
        ready = call(list(video[t]), tracker=TRK, lookback=lb, flush=(t == 4), **kw)
        assert len(ready) == S
        for k in range(S):
            assert len(ready[k]) == (0 if t < depth else 1 if t < 4 else depth + 1), (t, k)
            got[k].extend(ready[k])
        names = [e[1] for e in eng.s.log[n0:]]
        assert names.count("lookback_step") == (2 if t < 4 else 2 + 2 * depth)
        assert names.count("cover_faces" if mark == 0 else "draw_faces") == (0 if t < depth else 2 if t < 4 else 2 + 2 * depth)
        steps = [e for e in eng.s.log[n0:] if e[1] == "lookback_step"]
        assert [e[2:5] for e in steps[:2]] == [(0, 2, True), (2, 1, True)] and all(e[4] is False for e in steps[2:])
        # each push stands behind the chunk's update, and a due frame is covered behind the step
        assert names.index("track_update_device") < names.index("lookback_step")
        assert [lb.fill(k) for k in range(S)] == [min(t + 1, depth) if t < 4 else 0] * S
    assert np.array_equal(video, keep)                                       # the caller's arrays are never written
    for k in range(S):
        assert len(got[k]) == 5
        for t, (frame, dets, lms, info) in enumerate(got[k]):
            want = keep[t, k].copy()
            want.reshape(-1)[mark] ^= 0xFF                                   # the retained copy of frame t, covered (drawn) once
            assert frame.shape == shape and np.array_equal(frame, want), (k, t)
            assert not np.shares_memory(frame, video)
            assert dets.shape == (1, 5) and dets[0, 0] == 100 * k + t and lms.shape == (1, 10) and info.shape == (1, 3)
    lb.close()


def test_unequal_fill_is_refused_before_any_engine_call():
    lb = cfa.Lookback(0, 3, depth=2, rows=4)
    eng = LookbackStub(Script(), lb)
    face = make_face((H, W), eng)
    imgs = [np.zeros(BGR, np.uint8)] * 3
    face.anonymize(imgs[:2], tracker=TRK, lookback=lb, **MOSAIC)             # streams 0 and 1 advance, stream 2 does not
    n = len(eng.s.log)
    with pytest.raises(ValueError, match="fill"):
        face.anonymize(imgs, tracker=TRK, lookback=lb, **MOSAIC)
    with pytest.raises(ValueError, match="fill"):
        face.annotate(imgs, tracker=TRK, lookback=lb)
    assert len(eng.s.log) == n and [lb.fill(k) for k in range(3)] == [1, 1, 0]
    eng.s.next = 0
    assert [len(r) for r in face.anonymize(imgs[:2], tracker=TRK, lookback=lb, **MOSAIC)] == [0, 0]      # the two that agree go on
    lb.close()


def test_scene_codes_reach_the_step_on_the_device_or_from_the_host():
    class Eng(LookbackStub):
        def scene_check(self, frames, fmt, scenes, tracker=None, stream0=0, *, codes=True, out_ptr=None):
            self._log("scene_check", stream0, codes, out_ptr)
            return None if out_ptr or not codes else np.full((len(frames), 4), SAME, np.int32)

        def track_follow(self, frames, fmt, tracker, stream0=0, **o):
            self._log("track_follow", stream0)
            B = len(frames)
            return np.zeros((B, 4, 5), np.float32), np.zeros((B, 4, 10), np.float32), None, np.zeros(B, np.int32), None

    lb = cfa.Lookback(0, 2, depth=1, rows=4)
    lb._scene_codes = lambda engine: 4096                                    # (no GPU here: a stand-in address)
    eng = Eng(Script(), lb)
    face = make_face((H, W), eng)
    imgs = [np.zeros(BGR, np.uint8)] * 2
    face.anonymize(imgs, tracker=TRK, scenes="scenes", lookback=lb, **MOSAIC)
    log = [e for e in eng.s.log if e[1] in ("scene_check", "lookback_step")]
    assert log[0][2:] == (0, False, 4096) and log[1][2:] == (0, 2, True, 4096)
    eng.s.next, n = 0, len(eng.s.log)
    face.anonymize(imgs, tracker=TRK, scenes="scenes", lookback=lb, detect=False, **MOSAIC)      # the codes are read: they feed the step from the host
    log = [e for e in eng.s.log[n:] if e[1] in ("scene_check", "lookback_step")]
    assert log[0][2:] == (0, True, None) and isinstance(log[1][5], np.ndarray) and log[1][5].shape == (2, 4)
    assert CUT == cfa._lib.CF_SCENE_CUT and SAME == cfa._lib.CF_SCENE_SAME
    lb.close()
