"""The traced lookback's C ABI and Python binding, the refusals that need no device, a hand-checked case and the planted-move scenes of
its numpy restatement, and the product path against a stand-in engine (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from follow_cases import MOVED, NONE
from lookback_cases import grown
from lookback_trace_cases import HAND_BOX, HAND_MOVE, HW, PLANTED, lumas_of, planted, run_lookback_trace, shifted
from test_lookback_abi import TRK, LookbackStub
from test_product_paths import BGR, H, MOSAIC, W, Script, make_face

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "centerface_hip.h")).read()
SYMBOLS = ("cf_lookback_trace_enable", "cf_lookback_step_frames", "cf_op_lookback_trace")


def test_symbols_exported_declared_and_bound():
    L = cfa._lib.lib()
    for s in SYMBOLS:
        assert s in cfa._lib.EXPORTS
        assert re.search(r"\bint %s\(" % s, HEADER), s
        assert hasattr(L, s) and getattr(L, s).argtypes, s
    assert len(L.cf_lookback_trace_enable.argtypes) == 5 and len(L.cf_lookback_step_frames.argtypes) == 21
    assert len(L.cf_op_lookback_trace.argtypes) == 27
    assert len(L.cf_lookback_step.argtypes) == 13 and len(L.cf_op_lookback.argtypes) == 16      # the untraced calls keep their form
    for s, n in zip(SYMBOLS, (5, 21, 27)):                                  # ... and the header declares as many
        args = re.search(r"\bint %s\((.*?)\);" % s, HEADER, re.S).group(1)
        assert len(args.split(",")) == n, s
    assert callable(cfa.ops.lookback_trace_sequence)
    for name in ("lookback_step_frames", "lookback_step_frames_device"):
        assert callable(getattr(cfa.Engine, name))
    sig = inspect.signature(cfa.Lookback.trace)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [("search", 4), ("max_sad", 4096)]
    sig = inspect.signature(cfa.Engine.lookback_step_frames)
    assert list(sig.parameters)[1:] == ["lb", "frames", "fmt", "stream0", "B", "push", "scene"]


def test_the_header_states_the_ring_and_keeps_the_untraced_sentence():
    assert "298 MB" in HEADER and "(w + 15) & ~15" in HEADER
    at = HEADER.find("cf_lookback_trace_enable")
    assert "no accuracy claim" in HEADER[at - 3000:at + 6000]
    mk = open(os.path.join(ROOT, "lightweight-face-detection-centernet_amd", "csrc", "Makefile")).read()
    assert re.search(r"EXTRA_cf_lookback\s*=\s*-ffp-contract=off", mk) and re.search(r"EXTRA_cf_follow\s*=\s*-ffp-contract=off", mk)


# ---------------------------------------------------------------------------------------------- refusals before any device
ENABLE_REFUSALS = [(None, 64, 96, "null options"), ((0, 4096), 64, 96, "search"), ((9, 4096), 64, 96, "search"), ((4, -1), 64, 96, "max_sad"),
                   ((4, 65281), 64, 96, "max_sad"), ((4, 4096), 63, 96, "h and w"), ((4, 4096), 64, 95, "h and w"), ((4, 4096), 0, 96, "h and w"),
                   ((4, 4096), 64, 0, "h and w"), ((4, 4096), 8194, 96, "h and w"), ((4, 4096), 64, 8194, "h and w")]


@pytest.mark.parametrize("opts, h, w, word", ENABLE_REFUSALS, ids=["%s_%d" % (r[3].split()[0], i) for i, r in enumerate(ENABLE_REFUSALS)])
def test_enable_refuses_bad_arguments_before_any_device(opts, h, w, word):
    L = cfa._lib.lib()
    o = None if opts is None else C.byref(cfa._lib.follow_opts(*opts))
    assert L.cf_lookback_trace_enable(None, None, o, h, w) == -1
    why = L.cf_op_last_error().decode()
    assert "cf_lookback_trace_enable" in why and word in why and "null context" not in why, why
    if opts is not None and h == 64 and w == 96:
        r, why = _op(fopts=opts)
        assert r == -1 and "cf_op_lookback_trace" in why and word in why, why
        with pytest.raises(ValueError):
            cfa.Lookback(0, 2).trace(*opts)
    elif opts is not None:
        r, why = _op(h=h, w=w)
        assert r == -1 and "cf_op_lookback_trace" in why, why


def test_enable_and_step_frames_with_good_arguments_name_the_null_context():
    L = cfa._lib.lib()
    o = cfa._lib.follow_opts()
    assert L.cf_lookback_trace_enable(None, None, C.byref(o), 64, 96) == -1 and "null context" in L.cf_op_last_error().decode()
    st = np.full((1, 4), 9, np.int32)
    frame = np.zeros((64, 96), np.uint8)
    tab = (cfa._lib.PlanesRW * 1)()
    tab[0].p0 = tab[0].p1 = frame.ctypes.data
    step = lambda B, push, fmt=0, t=tab, h=64, w=96: L.cf_lookback_step_frames(None, None, 0, B, push, None, 0, fmt, t, 0, h, w, 96, 96, None, None,      # noqa: E731
                                                                                None, None, cfa._lib.ptr(st), None, 0)
    for B in (0, -2):
        assert step(B, 1) == -1
        why = L.cf_op_last_error().decode()
        assert "cf_lookback_step_frames" in why and "B must be" in why and "null context" not in why, why
    assert step(1, 1) == -1 and "null context" in L.cf_op_last_error().decode()
    assert step(1, 0, t=None, h=0, w=0) == -1 and "null context" in L.cf_op_last_error().decode()      # a drain needs no frame
    assert step(1, 1, fmt=7) == -1 and "format" in L.cf_op_last_error().decode()                       # the follower's geometry rules
    assert step(1, 1, t=None) == -1 and "null context" not in L.cf_op_last_error().decode()
    assert step(1, 1, h=63) == -1 and "null context" not in L.cf_op_last_error().decode()
    assert (st == 9).all()


def _op(fopts=(4, 4096), h=64, w=96, S=2, F=2, rows_in=4, null=None, tiled=0, space=(64, 96)):
    L = cfa._lib.lib()
    o, fo = cfa._lib.lookback_opts(2, 4, 0.05, 1), cfa._lib.follow_opts(*fopts)
    n, R = F * S, 4
    a = dict(push=np.ones(F, np.uint8), dets_in=np.zeros((n, rows_in, 5), np.float32), lms_in=np.zeros((n, rows_in, 10), np.float32),
             info_in=np.zeros((n, rows_in, 3), np.int32), counts_in=np.zeros(n, np.int32), cuts=np.zeros(n, np.int32),
             dets=np.full((n, R, 5), 9, np.float32), lms=np.full((n, R, 10), 9, np.float32), info=np.full((n, R, 3), 9, np.int32),
             counts=np.full(n, 9, np.int32), state=np.full((n, 4), 9, np.int32), moves=np.full((n, R, 4), 9, np.int32))
    p = {k: (None if k == null else cfa._lib.ptr(v)) for k, v in a.items()}
    hh, ww = max(min(h, 128), 2), max(min(w, 128), 2)                       # (a refusal touches no frame: small ones will do)
    frames = np.zeros((n, hh * 3 // 2, ww), np.uint8)
    tab = (cfa._lib.PlanesRW * n)()
    for k in range(n):
        tab[k].p0, tab[k].p1 = frames[k].ctypes.data, frames[k, hh:].ctypes.data
    r = L.cf_op_lookback_trace(0, C.byref(o), C.byref(fo), S, F, rows_in, p["push"], p["dets_in"], p["lms_in"], p["info_in"], p["counts_in"], p["cuts"],
                               0, tab, h, w, max(w, 4), max(w, 4), space[0], space[1], tiled, p["dets"], p["lms"], p["info"], p["counts"], p["state"], p["moves"])
    for k in ("dets", "lms", "info", "counts", "state", "moves"):
        assert (a[k] == 9).all()                                             # refused: nothing was written
    return r, (L.cf_op_last_error() or b"").decode()


def test_cf_op_lookback_trace_refuses_before_any_device():
    for kw, word in ((dict(F=0), "n_steps"), (dict(rows_in=5), "rows_in"), (dict(null="moves"), "null argument"), (dict(null="dets"), "null argument"),
                     (dict(space=(0, 96)), "space_h"), (dict(tiled=1, space=(64, 64)), "frame space"), (dict(tiled=2), "tiled")):
        r, why = _op(**kw)
        assert r == -1 and "cf_op_lookback_trace" in why and word in why, (kw, why)


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_one_birth_traced_two_frames_back_by_hand():
    """depth 2, one track born at frame 3.  The canvas moves by (+4, -2) per frame and the face is 32 pixels wide (c = 2), so the face of
    frame 3 stood 4 pixels further left and 2 further down in frame 2, 8 and 4 in frame 1.  grow = 1/16: g = 1.0625 and 1.125 exactly."""
    tabs, frames, _ = planted(11, "nv12", HW, 6, HAND_MOVE, [(3, HAND_BOX)], 2)
    d, l, i, c, push = tabs
    dets, lms, info, cnt, st, mv = run_lookback_trace(d, l, i, c, lumas_of(frames, "nv12"), HW, push, depth=2, rows=4, grow=0.0625)
    assert st[:, 0, 0].tolist() == [-1, -1, 0, 1, 2, 3, 4, 5] and cnt[:, 0].tolist() == [0, 0, 0, 1, 1, 1, 1, 1]
    # step 3 emits frame 1 (distance 2), step 4 frame 2 (distance 1), step 5 frame 3 with its own row
    assert mv[3, 0, 0].tolist() == [-8, 4, 0, MOVED] and mv[4, 0, 0].tolist() == [-4, 2, 0, MOVED] and mv[5, 0, 0].tolist() == [0, 0, 0, NONE]
    assert info[3, 0, 0].tolist() == [1, 0, 2] and info[4, 0, 0].tolist() == [1, 0, 1] and info[5, 0, 0].tolist() == [1, 1, 0]
    # (30.5, 16.25, 62.5, 48.25) - (4, -2): (26.5, 18.25, 58.5, 50.25), centre (42.5, 34.25), half side 16 * 1.0625 = 17
    assert dets[4, 0, 0, :4].tolist() == [25.5, 17.25, 59.5, 51.25]
    # - (8, -4): (22.5, 20.25, 54.5, 52.25), centre (38.5, 36.25), half side 16 * 1.125 = 18
    assert dets[3, 0, 0, :4].tolist() == [20.5, 18.25, 56.5, 54.25]
    assert dets[5, 0, 0, :4].tolist() == list(HAND_BOX)
    # the landmarks move with the box and are not grown: arange(10) * 1.5 + id + 0.125 * 3 of the birth frame
    birth = np.arange(10, dtype=np.float32) * 1.5 + 1 + 0.375
    assert lms[4, 0, 0].tolist() == (birth + np.tile(np.float32([-4, 2]), 5)).tolist()
    assert lms[3, 0, 0].tolist() == (birth + np.tile(np.float32([-8, 4]), 5)).tolist()
    assert dets[3, 0, 0, 4] == d[3, 0, 0, 4]


@pytest.mark.parametrize("seed, fmt, move, box", PLANTED, ids=[p[1] for p in PLANTED])
def test_the_restatement_recovers_every_planted_move(seed, fmt, move, box):
    """depth 3, a birth at frame 3: the back-filled box at distance j is the birth box moved by -j times the move, then grown, SAD 0."""
    depth = 3
    tabs, frames, _ = planted(seed, fmt, HW, 7, move, [(3, box)], depth)
    d, l, i, c, push = tabs
    dets, _, info, cnt, st, mv = run_lookback_trace(d, l, i, c, lumas_of(frames, fmt), HW, push, depth=depth, rows=4, grow=0.05)
    for j in (1, 2, 3):
        f = 3 - j + depth                                                    # the step that emits frame 3 - j
        assert st[f, 0].tolist() == [3 - j, 0, 1, 0] and info[f, 0, 0].tolist() == [1, 0, j]
        assert mv[f, 0, 0].tolist() == [-j * move[0], -j * move[1], 0, MOVED], (j, mv[f, 0, 0])
        assert dets[f, 0, 0, :4].tolist() == grown(np.float32(shifted(box, -j * move[0], -j * move[1])), 0.05, j).tolist()


# ---------------------------------------------------------------------------------------------- the product path against a stand-in engine
class TraceStub(LookbackStub):
    def lookback_step_frames(self, lb, frames, fmt, stream0=0, B=None, push=True, scene=None):
        self._log("lookback_step_frames", np.asarray(frames).shape, fmt, stream0, B, push)
        self.frames_seen.append(np.array(frames))
        n = len(self.s.log)
        out = self.lookback_step(lb, stream0, B, push, scene)
        del self.s.log[n:]                                                   # (one entry per call)
        return out + (np.zeros((B, lb.rows, 4), np.int32),)


@pytest.mark.parametrize("traced", (True, False))
def test_the_chunks_frames_reach_the_step_only_with_trace(traced):
    depth, S = 1, 3
    lb = cfa.Lookback(0, S, depth=depth, rows=4)
    if traced:
        assert lb.trace() is lb
    eng = TraceStub(Script(), lb)
    eng.frames_seen = []
    face = make_face((H, W), eng)
    rng = np.random.default_rng(2)
    video = rng.integers(0, 256, (3, S) + BGR, dtype=np.uint8)
    for t in range(3):
        eng.s.next, n0 = 0, len(eng.s.log)
        ready = face.anonymize(list(video[t]), tracker=TRK, lookback=lb, flush=(t == 2), **MOSAIC)
        assert [len(r) for r in ready] == [0 if t == 0 else 1 if t < 2 else 2] * S
        log = [e for e in eng.s.log[n0:] if e[1].startswith("lookback_step")]
        pushes = [e for e in log if e[1] == ("lookback_step_frames" if traced else "lookback_step")][:2]
        if traced:
            assert [e[2:] for e in pushes] == [((2,) + BGR, "bgr", 0, 2, True), ((1,) + BGR, "bgr", 2, 1, True)]
            assert np.array_equal(np.concatenate(eng.frames_seen[-2:]), video[t])       # the chunk's own frames, unmarked
            assert all(e[1] == "lookback_step" and e[4] is False for e in log[2:])      # the drains stay lookback_step(push=False)
        else:
            assert [e[2:5] for e in pushes] == [(0, 2, True), (2, 1, True)] and not eng.frames_seen
            assert all(e[1] == "lookback_step" for e in log)
    lb.close()


def test_trace_comes_before_the_first_use():
    lb = cfa.Lookback(0, 2, depth=1, rows=4)
    eng = LookbackStub(Script(), lb)
    face = make_face((H, W), eng)
    face.anonymize([np.zeros(BGR, np.uint8)] * 2, tracker=TRK, lookback=lb, **MOSAIC)
    with pytest.raises(ValueError, match="first use"):
        lb.trace()
    lb.close()
