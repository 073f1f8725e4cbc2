"""The lookback on the GPU: cf_op_lookback against the numpy restatement (tests/lookback_cases.py) bit for bit, then the object behind an
engine's update -- the state rules, the redaction and the annotation of the delayed frame, a ring of two engines, the product path."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from lookback_cases import RefLookback, face_box, grown, random_tracked, run_lookback, tracked_tables
from test_redact import redact_ref, source_frames
from test_track import _blank_batch, _feed_until_faces, _outcome, OK, STATE, VALUE
from track_cases import tables

pytestmark = pytest.mark.gpu


def check_sequence(d, l, i, c, push=None, cuts=None, **opts):
    """ops.lookback_sequence == the restatement on dets, lms, info, counts and state; what is not written keeps the prefill."""
    F, S = c.shape
    R = opts.get("rows", 256)
    rng = np.random.default_rng(7)
    d0 = rng.standard_normal((F, S, R, 5)).astype(np.float32)
    l0 = rng.standard_normal((F, S, R, 10)).astype(np.float32)
    i0 = rng.integers(-9, 9, (F, S, R, 3)).astype(np.int32)
    want = run_lookback(d, l, i, c, push, cuts, d0, l0, i0, **opts)
    got = ops.lookback_sequence(d, l, i, c, push, cuts, d0.copy(), l0.copy(), i0.copy(), **opts)
    for name, g, w in zip(("dets", "lms", "info", "counts", "state"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
            raise AssertionError("%s differs at %s: got %s, want %s (%s)" % (name, bad[:4].tolist(), g[tuple(bad[0][:2])][:3], w[tuple(bad[0][:2])][:3], opts))
    return want


def one_birth_per_frame(F, S=1, first=0):
    """Frame f of every stream holds the ids 1 .. first + f + 1: one track is born in every frame."""
    return [[[(k + 1, face_box(k)) for k in range(first + f + 1)] for _ in range(S)] for f in range(F)]


def drained(tabs, extra):
    """The tables with ``extra`` steps behind them that push nothing, and the push column."""
    d, l, i, c = tabs
    pad = lambda a: np.concatenate([a, np.zeros((extra,) + a.shape[1:], a.dtype)])      # noqa: E731
    return pad(d), pad(l), pad(i), pad(c), np.array([1] * len(c) + [0] * extra, np.uint8)


@pytest.mark.parametrize("R", (1, 3, 64, 65, 256, 257, 1024))
def test_rows_at_the_wave_and_workgroup_edges(R):
    """depth 2; a frame with half the rows, one that fills them, one whose count exceeds the stride, one of R tracks that are all new:
    the compaction crosses 64 and 256, the own rows alone fill ``rows``, a surplus sets bit 0 and the first rows win."""
    a = R // 2
    n1 = a + (R - a) // 2 + 1
    ids = [list(range(1, a + 1)), list(range(1, n1 + 1)), list(range(R + 1, 2 * R + 4)), list(range(R, 0, -1)),
           list(range(2 * R + 10, 3 * R + 10)), list(range(1, R + 1))]
    frames = [[[(k, face_box(k % 997, 10.0 + k % 7)) for k in row]] for row in ids]
    d, l, i, c, push = drained(tracked_tables(frames, R), 3)
    assert c[2, 0] == R + 3                                                  # a count above the stride
    _, _, info, cnt, st = check_sequence(d, l, i, c, push, depth=2, rows=R, grow=0.05)
    assert st[:, 0, 0].tolist() == [-1, -1, 0, 1, 2, 3, 4, 5, -1]
    # frame 0: a own rows, n1 - a births one frame ahead and R two frames ahead: topped up to rows, the surplus dropped, the first win
    assert cnt[2, 0] == R and st[2, 0].tolist() == [0, a, R - a, 1]
    assert info[2, 0, a].tolist() == [a + 1, 0, 1] and info[2, 0, R - 1].tolist() == ([n1, 0, 1] if n1 == R else [R + (R - n1), 0, 2])
    assert st[3, 0].tolist() == [1, n1, R - n1, 1]
    assert st[4, 0].tolist() == [2, R, 0, 1]                                 # frame 2: its own rows fill the image, all R new ones are dropped


@pytest.mark.parametrize("depth", (1, 2, 32))
def test_births_at_every_distance(depth):
    F = depth + 4
    d, l, i, c, push = drained(tracked_tables(one_birth_per_frame(F), F + 1), depth + 2)
    dets, _, info, cnt, st = check_sequence(d, l, i, c, push, depth=depth, rows=F + depth + 2, grow=0.03)
    f = depth                                                                # the step that emits frame 0
    assert st[f, 0].tolist() == [0, 1, depth, 0] and info[f, 0, 1:depth + 1, 2].tolist() == list(range(1, depth + 1))
    assert dets[f, 0, depth, :4].tolist() == grown(face_box(depth), 0.03, depth).tolist()
    assert st[:, 0, 0].tolist() == [-1] * depth + list(range(F)) + [-1] * 2 and st[-3, 0].tolist() == [F - 1, F, 0, 0]


def test_a_cut_at_every_queue_position_and_forget():
    """Stream s has its cut (forget) on frame s: seen from an emitted frame it lies on every entry e_1 .. e_depth, on the emitted entry
    itself (which stops nothing) and outside the queue."""
    depth, F = 3, 8
    tabs = drained(tracked_tables(one_birth_per_frame(F, S=F), F + 1, S=F), depth + 1)
    for bit in (1, 2, 3):
        cuts = np.zeros((F + depth + 1, F), np.int32)
        cuts[np.arange(F), np.arange(F)] = bit
        _, _, _, _, st = check_sequence(*tabs, cuts=cuts, depth=depth, rows=16, grow=0.1)
        for s in range(F):
            for t in range(F):                                               # frame t, emitted by step t + depth: painted from the frames before the cut
                want = min(depth, F - 1 - t) if not t < s <= t + depth else s - t - 1
                assert st[t + depth, s].tolist() == [t, t + 1, want, 0], (bit, s, t)


@pytest.mark.parametrize("confirm", (1, 2, 4))
def test_confirm_with_ids_that_vanish_and_recur_across_a_cut(confirm):
    a, b, c3 = face_box(0), face_box(1), face_box(2)
    seq = [[], [(1, a)], [(2, b)], [(1, a), (2, b), (3, c3)], [(3, c3)], [(2, b), (3, c3), (4, a)], [(4, a)], [(3, c3), (4, a)], [(4, a)]]
    frames = [[rows, rows] for rows in seq]
    cuts = np.zeros((len(seq) + 4, 2), np.int32)
    cuts[3, 1] = cuts[7, 1] = 1                                              # stream 1: ids 1 and 2 recur behind a cut, where they do not count
    d, l, i, c, push = drained(tracked_tables(frames, 4, S=2), 4)
    _, _, _, _, st = check_sequence(d, l, i, c, push, cuts, depth=3, rows=8, grow=0.05, confirm=confirm)
    want = {1: [3, 2], 2: [2, 0], 4: [0, 0]}[confirm]                        # what frame 0 gains: every birth up to the cut | ids 1, 2, seen twice | nothing:
    #                                                                          at most depth entries are counted, depth + 1 sightings never happen
    assert st[3, :, 2].tolist() == want


def test_the_flickering_onset_is_covered_in_the_middle_frame():
    """hit, miss, hit under min_hits = 2: the tracker frees the tentative track at once and the middle frame has no row; the lookback
    paints the second track's first box into it.  The ids are the tracker's own."""
    face = face_box(3)
    b, s, l, c = tables([[[face]], [[]], [[face]], [[face]], [[face]]], 2)
    d, lm, info, cnt, _ = ops.track_sequence(b, s, l, c, iou=0.3, max_age=5, min_hits=2, max_tracks=4, hold_grow=0.0)
    assert cnt[:, 0].tolist() == [1, 0, 1, 1, 1] and info[:, 0, 0, 0].tolist() == [1, 0, 2, 2, 2]
    dets, _, oi, oc, st = check_sequence(d, lm, info, cnt, depth=2, rows=4, grow=0.05)
    assert st[3, 0].tolist() == [1, 0, 1, 0] and oi[3, 0, 0].tolist() == [2, 0, 1]      # the bare middle frame, covered from one frame ahead
    assert dets[3, 0, 0, :4].tolist() == grown(face, 0.05, 1).tolist()
    assert st[2, 0].tolist() == [0, 1, 1, 0] and oi[2, 0, :2, 0].tolist() == [1, 2]     # frame 0: its own tentative row and the second track


def test_non_finite_corners_and_odd_counts():
    nan, inf = float("nan"), float("inf")
    a, b = face_box(0), face_box(1)
    frames = [[[]], [[(1, (nan, 0, 5, 5)), (2, a), (3, (0, 0, inf, 5)), (4, (0, -inf, 5, 5)), (5, b)]], [[(6, a)]], [[(7, b)]], [[(8, a)]]]
    d, l, i, c = tracked_tables(frames, 5)
    c[2, 0], c[3, 0] = -3, 9                                                 # a negative count is an empty frame; 9 > stride 5 pushes the five rows there are
    i[3, 0, 1:, 0] = (9, 10, 11, 12)                                         # (whatever lies in them: here four more new ids)
    d[3, 0, 1:, :4] = face_box(7)
    _, _, info, _, st = check_sequence(d, l, i, c, depth=1, rows=6, grow=0.05)
    assert st[1, 0].tolist() == [0, 0, 2, 0] and info[1, 0, :2, 0].tolist() == [2, 5]      # the three non-finite rows are never painted back
    assert st[2, 0].tolist() == [1, 5, 0, 0] and st[3, 0].tolist() == [2, 0, 5, 0] and st[4, 0].tolist() == [3, 5, 0, 0]


def test_warm_up_and_a_full_drain_emit_every_frame_once():
    depth, F, S = 5, 9, 2
    d, l, i, c, push = drained(tracked_tables(one_birth_per_frame(F, S), F + 1, S), F + 2)
    _, _, _, _, st = check_sequence(d, l, i, c, push, depth=depth, rows=24, grow=0.05)
    for s in range(S):
        seq = st[:, s, 0]
        assert seq[seq >= 0].tolist() == list(range(F)) and seq[:depth].tolist() == [-1] * depth and seq[F + depth:].tolist() == [-1] * (F + 2 - depth)
    # pushes between drains: the queue refills from where it stands
    push2 = np.array([1, 1, 1, 0, 1, 1, 0, 0, 0, 0], np.uint8)
    tabs = tracked_tables(one_birth_per_frame(10), 11)
    _, _, _, _, st = check_sequence(*tabs, push=push2, depth=3, rows=16, grow=0.05)
    assert st[:, 0, 0].tolist() == [-1, -1, -1, 0, -1, 1, 2, 3, 4, -1]


@pytest.mark.parametrize("seed", (0, 1))
def test_random_sequences(seed):
    d, l, i, c, cuts = random_tracked(seed)
    assert d.shape[2] == 16 and c.max() > 10 and (cuts & 1).any() and (cuts & 2).any()
    d, l, i, c, push = drained((d, l, i, c), 9)
    cuts = np.concatenate([cuts, np.zeros((9, cuts.shape[1]), np.int32)])
    flagged = 0
    for opts in (dict(depth=8, rows=16, grow=0.05, confirm=1), dict(depth=3, rows=17, grow=0.3, confirm=2), dict(depth=2, rows=64, grow=0.0, confirm=3)):
        st = check_sequence(d, l, i, c, push, cuts, **opts)[4]
        assert (st[:, :, 2].sum() > 0) == (opts["confirm"] <= opts["depth"])      # depth + 1 sightings never happen: nothing is painted back
        flagged += int(st[:, :, 3].sum())
    assert flagged > 0
    assert check_sequence(d, l, i, c, push, None, depth=8, rows=40, grow=1.0)[4][:, :, 2].sum() > 0


# ---------------------------------------------------------------------------------------------- behind an engine
def _decode(eng):
    return eng.decode_threshold(0.3, 0.3, 64)


def _rows_of(step, b):
    dets, lms, info, counts, state = step
    n = int(counts[b])
    return dets[b, :n], lms[b, :n], info[b, :n]


def test_state_rules_of_the_step():
    rng = np.random.default_rng(5)
    eng = cfa.Engine(64, 96, max_batch=3, dtype="bf16")
    frames = rng.integers(0, 256, (2, 76, 102, 3), dtype=np.uint8)
    trk = cfa.Tracker(eng, 2, max_tracks=8)
    lb = cfa.Lookback(eng, 3, depth=2, rows=8)
    push = lambda **kw: eng.lookback_step(lb, 0, 2, **kw)                    # noqa: E731
    assert _outcome(lambda: eng.lookback_step(lb, 0, 2, push=False)) == STATE      # a drain before the first push: no row space yet
    assert _outcome(push) == STATE                                          # no forward
    eng.forward_resized_enqueue(frames)
    assert _outcome(push) == STATE                                          # no decode
    _decode(eng)
    assert _outcome(push) == STATE                                          # decoded rows, but no update behind them
    eng.track_update(trk)
    assert _outcome(lambda: eng.lookback_step(lb, 0, 3)) == STATE           # the tracked rows are those of two images
    assert _outcome(lambda: eng.lookback_step(lb, 2, 2)) == VALUE           # streams 2, 3 of an object with 3
    assert _outcome(lambda: eng.lookback_step(lb, -1, 2)) == VALUE
    assert _outcome(lambda: eng.lookback_step(lb, 0, 4)) == VALUE           # B above max_batch
    assert _outcome(push) == OK
    assert _outcome(push) == STATE                                          # the same rows again: time would advance twice
    assert _outcome(lambda: eng.lookback_step(lb, 0, 2, push=False)) == OK  # a drain needs no forward ...
    assert _outcome(push) == STATE                                          # ... and frees nothing for a second push
    assert _outcome(lambda: eng.track_update(trk)) == STATE                 # the refusal of a second update is what it was
    assert _outcome(lambda: eng.align_faces(size=16)) == OK                 # and the decode's own rows are still named by those who name them
    _decode(eng)
    assert _outcome(push) == STATE                                          # a new decode: its rows are not tracked yet
    eng.track_update(trk)
    assert _outcome(push) == OK
    eng.track_follow(frames, "bgr", trk)                                    # followed rows are tracked rows no step has consumed
    assert _outcome(push) == OK and _outcome(push) == STATE
    eng.upload_images(list(frames))
    assert _outcome(lambda: eng.redact_faces(frames.copy(), "bgr")) == OK   # (the followed rows survive an upload, as before)
    # another stride, another space
    other_trk = cfa.Tracker(eng, 2, max_tracks=7)
    eng.forward_resized_enqueue(frames)
    _decode(eng), eng.track_update(other_trk)
    assert _outcome(push) == VALUE                                          # 7 rows per image, the object was first given 8
    big = cfa.Tracker(eng, 2, max_tracks=9)
    lb2 = cfa.Lookback(eng, 2, depth=1, rows=8)
    _decode(eng), eng.track_update(big)
    assert _outcome(lambda: eng.lookback_step(lb2, 0, 2)) == VALUE          # 9 rows per image do not fit an entry of 8
    small = cfa.Engine(64, 64, max_batch=2, dtype="bf16")
    t64 = cfa.Tracker(small, 2, max_tracks=8)
    small.forward_resized_enqueue(frames)
    _decode(small), small.track_update(t64)
    assert _outcome(lambda: small.lookback_step(lb, 0, 2)) == VALUE         # rows of a 64 x 64 network in an object latched to 64 x 96
    for o in (t64, big, other_trk, trk, lb, lb2):
        o.close()
    small.close(), eng.close()


def test_the_delayed_frame_is_covered_and_drawn_with_the_lookback_rows():
    """depth 1: a blank batch, then a batch with faces.  The second step emits the blank frame with the faces' first boxes, grown; the
    redaction of that frame is the restatement's with those rows, the annotation draws them as held rows, stream 0 of the three-stream
    object is untouched, and the next forward makes the decode's rows current again."""
    rng = np.random.default_rng(3)
    eng = cfa.Engine(64, 96, max_batch=3, dtype="bf16")
    trk = cfa.Tracker(eng, 2, min_hits=1, max_age=3, max_tracks=70)
    lb, ref = cfa.Lookback(eng, 3, depth=1, rows=70, grow=0.25), RefLookback(3, depth=1, rows=70, grow=0.25)
    blank = _blank_batch(eng, B=2)
    assert sum(len(d) for d, _ in blank) == 0
    eng.track_update(trk)
    first = eng.lookback_step(lb, 1, 2)                                     # streams 1 and 2; stream 0 stays empty
    assert first[4][:, 0].tolist() == [-1, -1] and not first[3].any()
    src, base = _feed_until_faces(eng, rng, need=2, B=2)
    tracked, _ = eng.track_update(trk)
    got = eng.lookback_step(lb, 1, 2)
    h, w = src.shape[1:3]
    delayed = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)            # the frame that was held back (any bytes)
    for b in range(2):
        ref.step(1 + b, True, np.zeros((70, 5)), np.zeros((70, 10)), np.zeros((70, 3), np.int32), 0)
        d, l, ids, hits, misses = tracked[b]
        n = len(d)
        pad = lambda a, k: np.concatenate([a, np.zeros((70 - n, k), a.dtype)])      # noqa: E731
        wd, wl, wi, ws = ref.step(1 + b, True, pad(d, 5), pad(l, 10), pad(np.stack([ids, hits, misses], 1).astype(np.int32), 3), n)
        gd, gl, gi = _rows_of(got, b)
        assert gd.tobytes() == wd.tobytes() and gl.tobytes() == wl.tobytes() and gi.tobytes() == wi.tobytes() and got[4][b].tolist() == ws.tolist()
        assert ws.tolist() == [0, 0, n, 0] and (gi[:, 1] == 0).all() and (gi[:, 2] == 1).all()
    counts = got[3]
    assert counts.sum() >= 2
    boxes = np.concatenate([got[0][b, :counts[b], :4] for b in range(2)])
    opt = dict(mode="mosaic", shape="ellipse", cell=6)
    a, want = delayed.copy(), delayed.copy()
    eng.redact_faces(a, "bgr", **opt)
    redact_ref([(f.reshape(h, 3 * w),) for f in want], "bgr", boxes, counts, (64, 96), h, w, **opt)
    assert np.array_equal(a, want) and not np.array_equal(a, delayed)
    # the annotation: a back-filled row is a held one (hits 0, misses 1), with its id
    info = np.concatenate([got[2][b, :counts[b]] for b in range(2)])
    scores = np.concatenate([got[0][b, :counts[b], 4] for b in range(2)])
    lms = np.concatenate([got[1][b, :counts[b]] for b in range(2)])
    dopt = dict(label="id", held_color=(0, 255, 255), box_color=(2, 255, 0), dash_held=True)
    a, want, live = delayed.copy(), delayed.copy(), delayed.copy()
    eng.draw_faces(a, "bgr", **dopt)
    ops.draw_faces(want, boxes, scores, counts, (64, 96), "bgr", lms=lms, info=info, **dopt)
    live_info = info.copy()
    live_info[:, 1:] = (1, 0)
    ops.draw_faces(live, boxes, scores, counts, (64, 96), "bgr", lms=lms, info=live_info, **dopt)
    assert np.array_equal(a, want) and not np.array_equal(a, live) and not np.array_equal(a, delayed)
    # stream 0 was never pushed: a drain of it emits nothing; a drain of streams 1, 2 emits the frame with the faces, as it was tracked
    rest = eng.lookback_step(lb, 0, 3, push=False)
    assert rest[4][:, 0].tolist() == [-1, 1, 1] and rest[3][0] == 0
    for b in range(2):
        gd, gl, gi = _rows_of(rest, 1 + b)
        assert gd.tobytes() == tracked[b][0].tobytes() and gi[:, 0].tolist() == tracked[b][2].tolist() and rest[4][1 + b].tolist() == [1, len(gd), 0, 0]
    # three frames for the three images of the drain; then a forward and a decode: the decode's rows again
    with pytest.raises(ValueError):
        eng.redact_faces(delayed.copy(), "bgr", **opt)
    eng.forward_resized_enqueue(src)
    base = _decode(eng)
    a, want = src.copy(), src.copy()
    eng.redact_faces(a, "bgr", **opt)
    redact_ref([(f.reshape(h, 3 * w),) for f in want], "bgr", np.concatenate([d[:, :4] for d, _ in base]), [len(d) for d, _ in base], (64, 96), h, w, **opt)
    assert np.array_equal(a, want)
    trk.close(), lb.close(), eng.close()


def test_two_engines_share_one_object():
    """A ring: two engines alternate five batches through one tracker and one lookback object, in the device forms with nothing waited
    for in between; the emitted rows equal the restatement run over the tracked rows in call order."""
    rng = np.random.default_rng(11)
    engs = [cfa.Engine(64, 96, max_batch=2, dtype="bf16") for _ in range(2)]
    src, _ = _feed_until_faces(engs[0], rng, need=2, B=2)
    blank = np.full(src.shape, 128, np.uint8)
    batches = [blank, src, source_frames(rng, "noise", src.shape), src, blank]
    M = 65
    trk = cfa.Tracker(engs[1], 2, iou=0.3, max_age=1, min_hits=2, max_tracks=M, hold_grow=0.05)
    lb, ref = cfa.Lookback(engs[0], 2, depth=2, rows=M, grow=0.1), RefLookback(2, depth=2, rows=M, grow=0.1)
    shapes = ((2, M, 5), (2, M, 10), (2, M, 3), (2,), (2, M, 5), (2, M, 10), (2, M, 3), (2,), (2, 4))
    dtypes = (np.float32, np.float32, np.int32, np.int32, np.float32, np.float32, np.int32, np.int32, np.int32)
    dev = [[e.device_alloc(int(np.prod(s)) * 4) for s in shapes] for _ in batches for e in engs[:1]]
    for i, batch in enumerate(batches):
        e, p = engs[i % 2], dev[i]
        e.forward_resized_enqueue(batch)
        e.decode_threshold_enqueue(0.3, 0.3, 64)
        e.track_update_device(trk, 0, p[0], p[1], p[2], p[3])
        e.lookback_step_device(lb, 0, 2, True, None, p[4], p[5], p[6], p[7], p[8])
    for e in engs:
        e.synchronize()
    emitted = 0
    for i in range(len(batches)):
        host = [np.zeros(s, t) for s, t in zip(shapes, dtypes)]
        for a, p in zip(host, dev[i]):
            engs[0].memcpy_d2h(a, p)
        td, tl, ti, tc, gd, gl, gi, gc, gs = host
        for b in range(2):
            wd, wl, wi, ws = ref.step(b, True, td[b], tl[b], ti[b], tc[b])
            k = len(wd)
            assert gc[b] == k and gs[b].tolist() == ws.tolist(), (i, b)
            assert gd[b, :k].tobytes() == wd.tobytes() and gl[b, :k].tobytes() == wl.tobytes() and gi[b, :k].tobytes() == wi.tobytes()
            emitted += int(ws[2])
    assert emitted >= 2                                                      # the blank first frame gained the faces of the second
    for row in dev:
        for p in row:
            engs[0].device_free(p)
    trk.close(), lb.close()
    for e in engs:
        e.close()


def test_anonymize_with_a_lookback_equals_the_chain_by_hand():
    rng = np.random.default_rng(31)
    hw = (76, 102)
    face, face2 = (cfa.CenterFace(*hw, dtype="bf16", max_batch=2) for _ in range(2))
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        imgs = list(source_frames(rng, kind, (2,) + hw + (3,)))
        if sum(len(d) for d, _ in face.detect_batch(imgs)) >= 1:
            break
    blank = [np.full(hw + (3,), 128, np.uint8)] * 2
    video = [blank, imgs, blank, imgs]
    opt = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    topt = dict(min_hits=2, max_age=2)
    trk, trk2 = cfa.Tracker(face.engine, 2, **topt), cfa.Tracker(face2.engine, 2, **topt)
    lb, lb2 = cfa.Lookback(face.engine, 2, depth=1, rows=256), cfa.Lookback(face2.engine, 2, depth=1, rows=256)
    got = [[], []]
    for t, frame in enumerate(video):
        keep = [f.copy() for f in frame]
        ready = face.anonymize(frame, tracker=trk, lookback=lb, flush=(t == len(video) - 1), **opt)
        assert all(np.array_equal(a, b) for a, b in zip(frame, keep))
        assert [len(r) for r in ready] == [0 if t == 0 else 2 if t == len(video) - 1 else 1] * 2
        for k in range(2):
            got[k].extend(ready[k])
    # by hand, on a second engine, tracker and object
    eng, want, held = face2.engine, [[], []], []
    eng.set_rescale(face2.scale_h, face2.scale_w)
    for t, frame in enumerate(video):
        eng.forward_resized_enqueue(np.stack(frame))
        eng.decode_threshold(0.3, face2.nms_thresh, face2.max_dets)
        eng.track_update_device(trk2, 0)
        held.append(np.stack(frame))
        for push in ([True] if t < len(video) - 1 else [True, False]):
            d, l, i, c, s = eng.lookback_step(lb2, 0, 2, push=push)
            if s[0, 0] >= 0:
                out = held.pop(0)
                eng.cover_faces(out, "bgr", **opt)
                for k in range(2):
                    want[k].append((out[k], d[k, :c[k]], l[k, :c[k]], i[k, :c[k]]))
    eng.set_rescale(0.0, 0.0)
    for k in range(2):
        assert len(got[k]) == len(want[k]) == len(video)
        for g, w in zip(got[k], want[k]):
            assert all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(g, w))
    # the blank frames before a frame with faces are covered where the faces will be detected
    assert any((got[k][0][0] != blank[k]).any() for k in range(2)) and sum(len(got[k][0][1]) for k in range(2)) >= 1
    for o in (trk, trk2, lb, lb2):
        o.close()
    face.close(), face2.close()
