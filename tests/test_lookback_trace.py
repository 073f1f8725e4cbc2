"""The traced lookback on the GPU: cf_op_lookback_trace against the numpy restatement (tests/lookback_trace_cases.py) bit for bit, then the
enabled object behind an engine -- the state rules, the redaction of the delayed frame with the moved rows, the product path."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from follow_cases import FORMATS, LOST, MOVED, NONE, luma_of, planes_of
from lookback_cases import grown, random_tracked, run_lookback, tracked_tables
from lookback_trace_cases import HW, PLANTED, RefLookbackTrace, lumas_of, moving_frames, planted, run_lookback_trace, shifted
from test_lookback import _decode, _rows_of, drained, one_birth_per_frame
from test_redact import redact_ref, source_frames
from test_track import _outcome, OK, STATE, VALUE

pytestmark = pytest.mark.gpu

NAMES = ("dets", "lms", "info", "counts", "state", "moves")


def check(tabs, frames, fmt, space_hw, cuts=None, **opts):
    """ops.lookback_trace_sequence == the restatement on dets, lms, info, counts, state and moves; what is not written keeps the prefill.
    tabs = dets_in, lms_in, info_in, counts_in, push; frames[f * S + s] = the plane tuple of step f of stream s."""
    d, l, i, c, push = tabs
    F, S = c.shape
    R = opts.get("rows", 256)
    rng = np.random.default_rng(7)
    pre = dict(dets=rng.standard_normal((F, S, R, 5)).astype(np.float32), lms_out=rng.standard_normal((F, S, R, 10)).astype(np.float32),
               info=rng.integers(-9, 9, (F, S, R, 3)).astype(np.int32), moves=rng.integers(-9, 9, (F, S, R, 4)).astype(np.int32))
    want = run_lookback_trace(d, l, i, c, lumas_of(frames, fmt), space_hw, push, cuts, **{k: v.copy() for k, v in pre.items()}, **opts)
    got = ops.lookback_trace_sequence(d, l, i, c, frames, fmt, space_hw, push, cuts, **{k: v.copy() for k, v in pre.items()}, **opts)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
            raise AssertionError("%s differs at %s: got %s, want %s (%s)" % (name, bad[:4].tolist(), g[tuple(bad[0][:3])], w[tuple(bad[0][:3])], opts))
    return want


def walking(F, n):
    """shifts of F pushed frames that wander by a pixel or two per frame, and n more for the drains."""
    return [((f * 3) % 7 - 3 + f, (f * 2) % 5 - 2) for f in range(F)] + [(0, 0)] * n


# boxes of a 64 x 96 space in 64 x 96 frames: a 1-pixel box (c = 1), the 32-pixel face (c = 2), side 33 (c = 3), a box bigger than the frame
# (side 120: c = 8, every window crosses all four borders), and one half outside it (its runs clamp at the right and the lower border)
GEOMETRY = ((50.0, 30.0, 51.0, 31.0), (30.5, 16.25, 62.5, 48.25), (8.0, 20.0, 41.0, 50.5), (-10.0, -12.0, 110.0, 80.0), (80.0, 44.0, 112.0, 76.0))


def geometry_scene(seed, fmt, pads, depth=3, F=7, hw=HW):
    """Frames 0 .. 2 hold an older track; the five GEOMETRY boxes are born in frame 3, while the picture moves by (2, -1) per frame."""
    shifts = [(2 * f, -f) for f in range(F)] + [(0, 0)] * depth
    frames = moving_frames(seed, fmt, hw[0], hw[1], shifts, pads=pads)
    old = (1, (5.0, 5.0, 21.0, 21.0))
    rows = [[[old] + ([(2 + k, shifted(b, 2 * (f - 3), -(f - 3))) for k, b in enumerate(GEOMETRY)] if f >= 3 else [])] for f in range(F)]
    return drained(tracked_tables(rows, 6), depth), frames


@pytest.mark.parametrize("pads", ((0, 0), (5, 3), (4, 8)), ids=lambda p: "pad%d_%d" % p)
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_and_pitch(fmt, pads):
    tabs, frames = geometry_scene(1, fmt, pads)
    want = check(tabs, frames, fmt, HW, depth=3, rows=12, grow=0.05, max_sad=65280)
    st, mv = want[4], want[5]
    assert st[3, 0].tolist() == [0, 1, 5, 0] and st[5, 0].tolist() == [2, 1, 5, 0] and st[6, 0].tolist() == [3, 6, 0, 0]
    assert (mv[3:6, 0, 1:6, 3] == MOVED).all() and mv[5, 0, 1].tolist() == [-2, 1, 0, MOVED] and mv[3, 0, 1].tolist() == [-6, 3, 0, MOVED]
    assert not mv[6, 0, :6].any()                                            # own rows


@pytest.mark.parametrize("search", (1, 8))
def test_search_radius(search):
    tabs, frames = geometry_scene(2, "nv12", (0, 0))
    want = check(tabs, frames, "nv12", HW, depth=3, rows=12, grow=0.05, search=search, max_sad=3000)
    codes = set(want[5][3:6, 0, 1:6, 3].ravel().tolist())
    assert codes <= {MOVED, LOST} and (search == 8) == (want[5][5, 0, 1].tolist() == [-2, 1, 0, MOVED])      # the 1-pixel box: (-2, 1) cells lie outside R = 1


@pytest.mark.parametrize("depth", (1, 3, 32))
def test_births_at_every_distance_and_while_warming_up(depth):
    """One birth per frame from the first on: the chains of the first ``depth`` births are shorter than depth."""
    F = depth + 3
    lattice = lambda k: (4.0 + (k % 5) * 18.5, 3.0 + (k // 5 % 3) * 19.0, 20.0 + (k % 5) * 18.5, 21.5 + (k // 5 % 3) * 19.0)      # noqa: E731
    rows = [[[(k + 1, lattice(k)) for k in range(f + 1)]] for f in range(F)]
    tabs = drained(tracked_tables(rows, F), depth + 1)
    frames = moving_frames(3, "i420", *HW, walking(F, depth + 1), smooth=2)
    want = check(tabs, frames, "i420", HW, depth=depth, rows=F + depth, grow=0.03, max_sad=65280)
    st, info = want[4], want[2]
    assert st[depth, 0].tolist() == [0, 1, depth, 0] and info[depth, 0, 1:depth + 1, 2].tolist() == list(range(1, depth + 1))
    assert st[:, 0, 0].tolist() == [-1] * depth + list(range(F)) + [-1] and (want[5][depth, 0, 1:depth + 1, 3] == MOVED).all()


def test_pushes_between_drains():
    push = np.array([1, 1, 1, 0, 1, 1, 0, 0, 0, 0], np.uint8)
    d, l, i, c = tracked_tables(one_birth_per_frame(10), 11)
    d[..., :4] *= np.float32(0.1)                                            # the lattice of lookback_cases, brought into the frame
    frames = moving_frames(4, "bgr", *HW, walking(10, 0), smooth=2)
    st = check((d, l, i, c, push), frames, "bgr", HW, depth=3, rows=16, grow=0.05, max_sad=65280)[4]
    assert st[:, 0, 0].tolist() == [-1, -1, -1, 0, -1, 1, 2, 3, 4, -1]


def test_a_cut_at_every_queue_position_and_forget():
    """Stream s has its cut (forget) on frame s: it lies on E, on the entry in front of E, in the middle of a chain, and outside it."""
    depth, F = 3, 8
    d, l, i, c, push = drained(tracked_tables(one_birth_per_frame(F, S=F), F + 1, S=F), depth + 1)
    d[..., :4] *= np.float32(0.1)
    frames = moving_frames(5, "nv21", *HW, walking(F, depth + 1), S=F, smooth=2)
    for bit in (1, 2, 3):
        cuts = np.zeros((F + depth + 1, F), np.int32)
        cuts[np.arange(F), np.arange(F)] = bit
        st = check((d, l, i, c, push), frames, "nv21", HW, cuts=cuts, depth=depth, rows=16, grow=0.1, max_sad=65280)[4]
        for s in range(F):
            for t in range(F):
                want = min(depth, F - 1 - t) if not t < s <= t + depth else s - t - 1
                assert st[t + depth, s].tolist() == [t, t + 1, want, 0], (bit, s, t)


def test_an_older_frame_of_noise_ends_the_chain():
    """depth 3, a birth at frame 4, frame 2 replaced by noise: distance 1 is found, distance 2 is LOST, distance 3 repeats its words."""
    seed, fmt, move, box = PLANTED[0]
    tabs, frames, _ = planted(seed, fmt, HW, 8, move, [(4, box)], 3)
    rng = np.random.default_rng(9)
    frames[2] = planes_of(rng, fmt, rng.integers(0, 256, HW, dtype=np.uint8))
    want = check(tabs, frames, fmt, HW, depth=3, rows=4, grow=0.05)
    mv, dets = want[5], want[0]
    assert mv[6, 0, 0].tolist() == [-move[0], -move[1], 0, MOVED]            # frame 3, emitted by step 6
    lost = mv[5, 0, 0].tolist()
    assert lost[:2] == [-move[0], -move[1]] and lost[2] > 4096 and lost[3] == LOST and mv[4, 0, 0].tolist() == lost
    for f, j in ((5, 2), (4, 3)):                                            # the box stays where the walk last had the face
        assert dets[f, 0, 0, :4].tolist() == grown(np.float32(shifted(box, -move[0], -move[1])), 0.05, j).tolist()


def test_born_rows_at_the_wave_edges_and_seventy_births():
    """An entry of 257 rows whose rows 0, 63, 64, 255 and 256 are born (the others are older tracks); then 70 births in one frame."""
    n, new = 257, (0, 63, 64, 255, 256)
    box = lambda k: (2.0 + (k % 20) * 4.5, 1.5 + (k // 20) * 4.5, 6.0 + (k % 20) * 4.5 + k % 3, 6.5 + (k // 20) * 4.5)      # noqa: E731
    olds = [(k + 1, box(k)) for k in range(n) if k not in new]
    full = [(1000 + k if k in new else k + 1, box(k)) for k in range(n)]
    tabs = drained(tracked_tables([[olds], [full], [full]], n), 2)
    frames = moving_frames(6, "nv12", *HW, walking(3, 2), smooth=2)
    want = check(tabs, frames, "nv12", HW, depth=2, rows=270, grow=0.05, max_sad=65280)
    assert want[4][2, 0].tolist() == [0, n - 5, 5, 0] and want[2][2, 0, n - 5:n, 0].tolist() == [1000 + k for k in new]
    assert (want[5][2, 0, n - 5:n, 3] == MOVED).all()
    seventy = [(k + 1, (1.0 + (k % 10) * 9.0, 1.0 + (k // 10) * 8.5, 9.5 + (k % 10) * 9.0, 9.0 + (k // 10) * 8.5)) for k in range(70)]
    tabs = drained(tracked_tables([[[]], [[]], [seventy]], 70), 2)
    want = check(tabs, frames, "nv12", HW, depth=2, rows=70, grow=0.05, max_sad=65280)
    assert want[4][2, 0].tolist() == [0, 0, 70, 0] and want[4][3, 0].tolist() == [1, 0, 70, 0] and (want[5][2:4, 0, :70, 3] == MOVED).all()


def _random(seed, scale=0.1):
    d, l, i, c, cuts = random_tracked(seed)
    d[..., :4] *= np.float32(scale)                                          # the lattice of lookback_cases, brought into the frame (NaN and inf stay)
    d, l, i, c, push = drained((d, l, i, c), 9)
    return (d, l, i, c, push), np.concatenate([cuts, np.zeros((9, cuts.shape[1]), np.int32)])


def test_confirm_and_a_rows_surplus_in_stretched_rows():
    """Random sequences with cuts, forgets, vanishing ids and non-finite corners: rows of a 64 x 96 network in frames of 76 x 102.  The
    flag bit and the dropped rows are those of the untraced restatement."""
    tabs, cuts = _random(0)
    F, S = tabs[3].shape
    frames = moving_frames(7, "yv12", 76, 102, walking(F - 9, 9), S=S, pads=(2, 1), smooth=2)
    flagged = 0
    for opts in (dict(depth=8, rows=16, grow=0.05, confirm=1), dict(depth=3, rows=17, grow=0.3, confirm=2), dict(depth=2, rows=64, grow=0.0, confirm=3)):
        want = check(tabs, frames, "yv12", (64, 96), cuts=cuts, max_sad=65280, **opts)
        plain = run_lookback(*tabs[:4], tabs[4], cuts, **opts)
        assert want[3].tobytes() == plain[3].tobytes() and want[4].tobytes() == plain[4].tobytes()
        flagged += int(want[4][:, :, 3].sum())
        assert (want[4][:, :, 2].sum() > 0) == (opts["confirm"] <= opts["depth"])
    assert flagged > 0


def test_rows_in_frame_space():
    tabs, cuts = _random(1, scale=0.12)
    F, S = tabs[3].shape
    frames = moving_frames(8, "bgr", *HW, walking(F - 9, 9), S=S, pads=(3, 0), smooth=2)
    want = check(tabs, frames, "bgr", HW, cuts=cuts, tiled=True, depth=4, rows=24, grow=0.05, search=3, max_sad=2500)
    assert {MOVED, LOST} <= set(want[5][..., 3].ravel().tolist())


@pytest.mark.parametrize("seed, fmt, move, box", PLANTED, ids=[p[1] for p in PLANTED])
def test_the_back_filled_box_follows_the_planted_move(seed, fmt, move, box):
    """The back-filled box at distance j is the birth box moved by -j times the move, then grown; the same tables through
    ops.lookback_sequence give the unmoved boxes."""
    depth = 3
    tabs, frames, _ = planted(seed, fmt, HW, 7, move, [(3, box)], depth, pads=(4, 4))
    want = check(tabs, frames, fmt, HW, depth=depth, rows=4, grow=0.05)
    d, l, i, c, push = tabs
    plain = ops.lookback_sequence(d, l, i, c, push, depth=depth, rows=4, grow=0.05)
    for j in (1, 2, 3):
        f = 3 - j + depth
        assert want[5][f, 0, 0].tolist() == [-j * move[0], -j * move[1], 0, MOVED]
        assert want[0][f, 0, 0, :4].tolist() == grown(np.float32(shifted(box, -j * move[0], -j * move[1])), 0.05, j).tolist()
        assert plain[0][f, 0, 0, :4].tolist() == grown(np.float32(box), 0.05, j).tolist()
    assert plain[3].tobytes() == want[3].tobytes() and plain[4].tobytes() == want[4].tobytes()


def test_identical_frames_equal_the_untraced_step():
    tabs, cuts = _random(2)
    d, l, i, c, push = tabs
    F, S = c.shape
    rng = np.random.default_rng(10)
    one = [planes_of(rng, "nv12", rng.integers(0, 256, HW, dtype=np.uint8)) for _ in range(S)]
    frames = [one[s] for _ in range(F) for s in range(S)]
    opts = dict(depth=5, rows=20, grow=0.07, confirm=1)
    got = ops.lookback_trace_sequence(d, l, i, c, frames, "nv12", HW, push, cuts, max_sad=65280, **opts)
    plain = ops.lookback_sequence(d, l, i, c, push, cuts, **opts)
    for name, g, w in zip(NAMES, got, plain):
        assert g.tobytes() == w.tobytes(), name
    assert got[4][:, :, 2].sum() > 0 and not got[5][..., :3].any() and (got[5][..., 3] == MOVED).any()


# ---------------------------------------------------------------------------------------------- behind an engine
EVEN = (("noise", (76, 102)), ("binary", (76, 102)), ("blocks", (76, 102)), ("binary", (96, 128)), ("noise", (192, 256)), ("binary", (192, 256)),
        ("blocks", (150, 200)))


def _even_faces(eng, rng, need=2, B=2):
    """The first of EVEN whose forward_resized + threshold decode keeps ``need`` faces (frames of even sides): (frames, result)."""
    tried = []
    for kind, hw in EVEN:
        src = source_frames(rng, kind, (B,) + hw + (3,))
        eng.forward_resized_enqueue(src)
        base = _decode(eng)
        tried.append((kind, hw, [len(d) for d, _ in base]))
        if sum(len(d) for d, _ in base) >= need:
            return src, base
    raise AssertionError("no source kept %d faces with the default weights: %s" % (need, tried))


def _blank(eng, hw, B=2):
    for v in (128, 0, 255):
        blank = np.full((B,) + hw + (3,), v, np.uint8)
        eng.forward_resized_enqueue(blank)
        if sum(len(d) for d, _ in _decode(eng)) == 0:
            return blank
    raise AssertionError("every constant batch keeps faces with the default weights")


def test_state_rules_of_an_enabled_object():
    rng = np.random.default_rng(5)
    eng = cfa.Engine(64, 96, max_batch=2, dtype="bf16")
    frames = rng.integers(0, 256, (2, 76, 102, 3), dtype=np.uint8)
    trk = cfa.Tracker(eng, 2, max_tracks=8)
    plain, late, lb = cfa.Lookback(eng, 2, depth=2, rows=8), cfa.Lookback(eng, 2, depth=2, rows=8).trace(), cfa.Lookback(eng, 2, depth=2, rows=8).trace(3, 500)
    rows = lambda: (eng.forward_resized_enqueue(frames), _decode(eng), eng.track_update(trk))      # noqa: E731
    rows()
    assert _outcome(lambda: eng.lookback_step_frames(plain, frames, "bgr")) == STATE      # a plain object has no ring
    assert _outcome(lambda: eng.lookback_step(plain, 0, 2)) == OK
    # enable after a push -> STATE (the Python object enables at its first step_frames: here the library call itself)
    o = cfa._lib.follow_opts()
    import ctypes as C
    assert eng._L.cf_lookback_trace_enable(eng._h, plain._handle(eng), C.byref(o), 76, 102) == cfa._lib.CF_ESTATE
    rows()
    assert _outcome(lambda: eng.lookback_step(lb, 0, 2, push=False)) == STATE             # a drain before the first push
    assert _outcome(lambda: eng.lookback_step_frames(lb, frames, "bgr")) == OK            # enables for 76 x 102, pushes
    assert eng._L.cf_lookback_trace_enable(eng._h, lb._handle(eng), C.byref(o), 76, 102) == cfa._lib.CF_ESTATE      # twice
    assert _outcome(lambda: eng.lookback_step_frames(lb, frames, "bgr")) == STATE         # the same rows again
    rows()
    assert _outcome(lambda: eng.lookback_step(lb, 0, 2, push=True)) == STATE              # the frame is missing
    assert _outcome(lambda: eng.lookback_step_frames(lb, frames[:, :64, :96].copy(), "bgr")) == VALUE      # another frame size
    assert _outcome(lambda: eng.lookback_step_frames(lb, frames[:1], "bgr", 0, 2)) == VALUE
    assert _outcome(lambda: eng.lookback_step_frames(lb, frames, "bgr", 1)) == VALUE      # streams 1, 2 of an object with 2
    assert _outcome(lambda: eng.lookback_step_frames(lb, frames, "bgr")) == OK
    a = eng.lookback_step(lb, 0, 2, push=False)                              # a drain through either call
    b = eng.lookback_step_frames(lb, None, "bgr", push=False)
    assert a[4][:, 0].tolist() == [0, 0] and b[4][:, 0].tolist() == [1, 1] and len(b) == 6 and b[5].shape == (2, 8, 4)
    assert eng.lookback_step_frames(lb, None, "bgr", 0, 2, push=False)[4][:, 0].tolist() == [-1, -1]
    assert _outcome(lambda: eng.redact_faces(frames.copy(), "bgr")) == OK    # the lookback rows are the newest
    # trace() set, but the rows come in frame space of another size than the frames -> VALUE is the library's, not a crash
    rows()
    assert _outcome(lambda: eng.lookback_step_frames(late, frames, "bgr")) == OK
    for o_ in (trk, plain, late, lb):
        o_.close()
    eng.close()


def test_the_delayed_frame_is_covered_with_the_moved_rows():
    """depth 1.  The stream shows a picture and then the same picture moved by (4, 2) pixels; the detector is given a blank batch in place
    of the first, so that the faces are born in the second.  The emitted first frame has their boxes where the walk found them, the
    rows equal the restatement's, and the redaction of that frame is redact_ref's with those rows."""
    rng = np.random.default_rng(3)
    eng = cfa.Engine(64, 96, max_batch=2, dtype="bf16")
    src, _ = _even_faces(eng, rng, need=2, B=2)
    h, w = src.shape[1:3]
    before = np.roll(src, (-2, -4), axis=(1, 2))                             # what src shows, 4 pixels further left and 2 further up
    trk = cfa.Tracker(eng, 2, min_hits=1, max_age=3, max_tracks=70)
    lb = cfa.Lookback(eng, 2, depth=1, rows=70, grow=0.25).trace(search=4, max_sad=65280)
    ref = RefLookbackTrace(2, (64, 96), False, 4, 65280, depth=1, rows=70, grow=0.25)
    _blank(eng, (h, w))
    eng.track_update(trk)
    first = eng.lookback_step_frames(lb, before, "bgr")
    assert first[4][:, 0].tolist() == [-1, -1] and not first[3].any()
    eng.forward_resized_enqueue(src)
    _decode(eng)
    tracked, _ = eng.track_update(trk)
    got = eng.lookback_step_frames(lb, src, "bgr")
    moved = 0
    for b in range(2):
        ref.step(b, True, np.zeros((70, 5)), np.zeros((70, 10)), np.zeros((70, 3), np.int32), 0, None, luma_of((before[b].reshape(h, 3 * w),), "bgr"))
        d, l, ids, hits, misses = tracked[b]
        n = len(d)
        pad = lambda a, k: np.concatenate([a, np.zeros((70 - n, k), a.dtype)])      # noqa: E731
        wd, wl, wi, ws, wm = ref.step(b, True, pad(d, 5), pad(l, 10), pad(np.stack([ids, hits, misses], 1).astype(np.int32), 3), n, None,
                                      luma_of((src[b].reshape(h, 3 * w),), "bgr"))
        gd, gl, gi = _rows_of(got[:5], b)
        assert gd.tobytes() == wd.tobytes() and gl.tobytes() == wl.tobytes() and gi.tobytes() == wi.tobytes() and got[4][b].tolist() == ws.tolist()
        assert got[5][b, :len(wm)].tobytes() == wm.tobytes() and ws.tolist() == [0, 0, n, 0]
        moved += int((wm[:, :2] != 0).any(axis=1).sum())
    assert moved >= 1
    counts = got[3]
    boxes = np.concatenate([got[0][b, :counts[b], :4] for b in range(2)])
    opt = dict(mode="mosaic", shape="ellipse", cell=6)
    a, want = before.copy(), before.copy()
    eng.redact_faces(a, "bgr", **opt)
    redact_ref([(f.reshape(h, 3 * w),) for f in want], "bgr", boxes, counts, (64, 96), h, w, **opt)
    assert np.array_equal(a, want) and not np.array_equal(a, before)
    trk.close(), lb.close(), eng.close()


def test_anonymize_with_a_traced_lookback_equals_the_chain_by_hand():
    rng = np.random.default_rng(31)
    hw = (76, 102)
    face, face2 = (cfa.CenterFace(*hw, dtype="bf16", max_batch=2) for _ in range(2))
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        imgs = list(source_frames(rng, kind, (2,) + hw + (3,)))
        if sum(len(d) for d, _ in face.detect_batch(imgs)) >= 1:
            break
    blank = [np.full(hw + (3,), 128, np.uint8)] * 2
    near = [np.roll(f, (2, -4), axis=(0, 1)) for f in imgs]                  # the picture of imgs, moved
    video = [blank, near, imgs, blank, imgs]
    opt = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    topt = dict(min_hits=2, max_age=2)
    trk, trk2 = cfa.Tracker(face.engine, 2, **topt), cfa.Tracker(face2.engine, 2, **topt)
    lb = cfa.Lookback(face.engine, 2, depth=1, rows=256).trace(max_sad=65280)
    lb2 = cfa.Lookback(face2.engine, 2, depth=1, rows=256).trace(max_sad=65280)
    got = [[], []]
    for t, frame in enumerate(video):
        keep = [f.copy() for f in frame]
        ready = face.anonymize(frame, tracker=trk, lookback=lb, flush=(t == len(video) - 1), **opt)
        assert all(np.array_equal(a, b) for a, b in zip(frame, keep))
        for k in range(2):
            got[k].extend(ready[k])
    eng, want, held, moves = face2.engine, [[], []], [], 0
    eng.set_rescale(face2.scale_h, face2.scale_w)
    for t, frame in enumerate(video):
        eng.forward_resized_enqueue(np.stack(frame))
        eng.decode_threshold(0.3, face2.nms_thresh, face2.max_dets)
        eng.track_update_device(trk2, 0)
        held.append(np.stack(frame))
        for push in ([True] if t < len(video) - 1 else [True, False]):
            step = eng.lookback_step_frames(lb2, np.stack(frame), "bgr", 0, 2, push=push) if push else eng.lookback_step(lb2, 0, 2, push=False) + (None,)
            d, l, i, c, s, m = step
            moves += 0 if m is None else int(np.abs(m[..., :2]).sum())
            if s[0, 0] >= 0:
                out = held.pop(0)
                eng.cover_faces(out, "bgr", **opt)
                for k in range(2):
                    want[k].append((out[k], d[k, :c[k]], l[k, :c[k]], i[k, :c[k]]))
    eng.set_rescale(0.0, 0.0)
    for k in range(2):
        assert len(got[k]) == len(want[k]) == len(video)
        for g, w_ in zip(got[k], want[k]):
            assert all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(g, w_))
    assert sum(len(got[k][t][1]) for k in range(2) for t in range(len(video))) >= 1
    for o in (trk, trk2, lb, lb2):
        o.close()
    face.close(), face2.close()


COMBOS = {"tiled": dict(tiled=True), "fit": dict(fit=True), "scenes": dict(scenes=True), "follow": dict(follow=True),
          "follow_only": dict(follow=True, detect=False), "tiled_scenes_follow": dict(tiled=True, scenes=True, follow=True)}


@pytest.mark.parametrize("name", sorted(COMBOS))
def test_every_product_path_takes_a_traced_lookback(name):
    """tiled=, fit=, scenes=, follow= and detect=False with a traced object, whatever space the rows are latched in.  On a video that
    stands still no displacement beats (0, 0), so the delayed frames and their rows equal those of the untraced object bit for bit;
    on one that moves the call runs through and returns every frame once."""
    rng = np.random.default_rng(17)
    hw = (150, 200)
    face = cfa.CenterFace(64, 96, dtype="bf16", max_batch=24)
    for kind in ("blocks", "binary", "noise", "blocks", "binary", "noise"):  # the default weights answer to one of them
        imgs = list(source_frames(rng, kind, (2,) + hw + (3,)))
        if sum(len(d) for d, _ in face.detect_batch(imgs)) >= 2:
            break
    blank = [np.full(hw + (3,), 128, np.uint8)] * 2
    near = [np.roll(f, (2, -4), axis=(0, 1)) for f in imgs]
    kw = COMBOS[name]

    def run(traced, video):
        trk, lb = cfa.Tracker(face.engine, 2, min_hits=1, max_age=2), cfa.Lookback(face.engine, 2, depth=2, rows=256)
        scn = cfa.SceneCuts(face.engine, 2) if kw.get("scenes") else None
        if traced:
            lb.trace(max_sad=65280)
        out = [[], []]
        for t, frame in enumerate(video):
            k = dict(kw)
            if scn is not None:
                k["scenes"] = scn
            if "detect" in k:
                k["detect"] = t < 2                                          # then the faces are only followed
            ready = face.anonymize(list(frame), tracker=trk, lookback=lb, flush=(t == len(video) - 1), mode="solid", shape="rect", fill=(1, 2, 3), **k)
            for s in range(2):
                out[s].extend(ready[s])
        for o in (trk, lb) + ((scn,) if scn is not None else ()):
            o.close()
        return out

    still = [blank, imgs, imgs, imgs]
    plain, traced = run(False, still), run(True, still)
    for s in range(2):
        assert len(plain[s]) == len(traced[s]) == len(still)
        for g, w_ in zip(traced[s], plain[s]):
            assert all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(g, w_))
    rows = np.concatenate([i for s in range(2) for _, _, _, i in traced[s]])
    assert len(rows) >= 2 and (name == "scenes" or ((rows[:, 1] == 0) & (rows[:, 2] > 0)).any())      # faces, and some painted back into the blank frame
    moving = run(True, [blank, near, imgs, blank])
    assert [len(moving[s]) for s in range(2)] == [4, 4] and all(f.shape == hw + (3,) for s in range(2) for f, _, _, _ in moving[s])
    face.close()
