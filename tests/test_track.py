"""Face tracks across frames on the GPU: cf_op_track against the numpy restatement (tests/track_cases.py) bit for bit, then the tracker
behind an engine's decode -- the update, the redaction of held tracks, the state rules, tiled frames, a ring of two engines."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from test_redact import SOURCES, source_frames
from track_cases import RefTracker, grid_faces, random_sequence, run_sequence, tables

pytestmark = pytest.mark.gpu


def check_sequence(boxes, scores, lms, counts, **opts):
    """ops.track_sequence == the restatement on dets, lms, info, counts and flags, rows past the count unchanged (outputs prefilled)."""
    F, S = counts.shape
    M = opts.get("max_tracks", 256)
    rng = np.random.default_rng(7)
    d0 = rng.standard_normal((F, S, M, 5)).astype(np.float32)
    l0 = rng.standard_normal((F, S, M, 10)).astype(np.float32)
    i0 = rng.integers(-9, 9, (F, S, M, 3)).astype(np.int32)
    want = run_sequence(boxes, scores, lms, counts, d0, l0, i0, **opts)
    got = ops.track_sequence(boxes, scores, lms, counts, d0.copy(), l0.copy(), i0.copy(), **opts)
    for name, g, w in zip(("dets", "lms", "info", "counts", "flags"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
            raise AssertionError("%s differs at %s: got %s, want %s (%s)" % (name, bad[:4].tolist(), g[tuple(bad[0][:2])][:3], w[tuple(bad[0][:2])][:3], opts))
    return want


FACE = (10.5, 20.25, 30.75, 61.5)


def test_empty_frames():
    b, s, l, c = tables([[[], []], [[], []], [[], []]], 4, S=2)
    _, _, _, cnt, fl = check_sequence(b, s, l, c, max_tracks=5)
    assert not cnt.any() and not fl.any()


@pytest.mark.parametrize("gap", (3, 4))
def test_one_face_through_a_dropout(gap):
    """max_age = 3: a dropout of 3 frames keeps the id (misses counting 1, 2, 3, the box growing), one of 4 frames ends it (new id)."""
    frames = [[[FACE]], [[FACE]]] + [[[]]] * gap + [[[FACE]]]
    b, s, l, c = tables(frames, 2)
    _, _, info, cnt, _ = check_sequence(b, s, l, c, iou=0.3, max_age=3, min_hits=2, max_tracks=3, hold_grow=0.07)
    assert info[2:2 + min(gap, 3), 0, 0, 2].tolist() == [1, 2, 3][:min(gap, 3)]
    assert cnt[:, 0].tolist() == [1, 1] + [1, 1, 1, 0][:gap] + [1]
    assert info[-1, 0, 0].tolist() == ([1, 3, 0] if gap == 3 else [2, 1, 0])


def test_max_age_zero_and_min_hits():
    """max_age = 0: nothing is ever held.  min_hits = 2: a one-frame face is never held, a two-frame face is."""
    frames = [[[FACE]], [[FACE]], [[]], [[FACE]], [[]], [[]]]
    b, s, l, c = tables(frames, 1)
    _, _, _, cnt, _ = check_sequence(b, s, l, c, max_age=0, min_hits=1, max_tracks=2)
    assert cnt[:, 0].tolist() == [1, 1, 0, 1, 0, 0]
    _, _, info, cnt, _ = check_sequence(b, s, l, c, max_age=5, min_hits=2, max_tracks=2)
    assert cnt[:, 0].tolist() == [1, 1, 1, 1, 1, 1] and info[3, 0, 0].tolist() == [1, 3, 0]
    _, _, info, cnt, _ = check_sequence(b[3:], s[3:], l[3:], c[3:], max_age=5, min_hits=2, max_tracks=2)
    assert cnt[:, 0].tolist() == [1, 0, 0]


def test_slot_reuse_after_death_takes_the_lowest_free_slot():
    a, bb, cc, dd = grid_faces(4)
    frames = [[[a, bb, cc]], [[bb, cc]], [[bb, cc, dd, a]], [[cc]], [[a, bb, cc, dd]]]
    b, s, l, c = tables(frames, 4)
    _, _, info, cnt, fl = check_sequence(b, s, l, c, max_age=0, min_hits=1, max_tracks=4)
    assert info[2, 0, :4, 0].tolist() == [4, 2, 3, 5]                       # slot 0 was free: dd takes it, a takes slot 3; ids rise
    assert info[4, 0, :4, 0].tolist() == [6, 7, 3, 8] and not fl.any()


def test_non_finite_rows_and_counts_above_the_rows():
    nan, inf = float("nan"), float("inf")
    a, bb, cc = grid_faces(3)
    frames = [[[a, (nan, 0, 5, 5), bb, (0, 0, inf, 5), (0, -inf, 5, 5)]],
              [[(0, 0, 5, nan), a, bb, cc, cc, cc]],                       # six faces, four rows: count > rows
              [[a, bb]]]
    b, s, l, c = tables(frames, 4)
    assert c[1, 0] == 6
    _, _, info, cnt, _ = check_sequence(b, s, l, c, max_age=2, min_hits=1, max_tracks=8)
    assert cnt[:, 0].tolist() == [2, 3, 3] and info[1, 0, :3, 0].tolist() == [1, 2, 3]
    # extreme but finite corners: areas overflow, measures are inf / NaN and never win
    big = 3.0e38
    frames = [[[(-big, -big, big, big), a]], [[(-big, -big, big, big), a, (0, 0, big, 5)]]]
    b, s, l, c = tables(frames, 3)
    check_sequence(b, s, l, c, max_age=2, min_hits=1, max_tracks=8)


def test_overflow_sets_the_flag_and_the_first_rows_win():
    faces = grid_faces(5)
    b, s, l, c = tables([[faces], [faces[::-1]], [faces]], 5)
    d, _, info, cnt, fl = check_sequence(b, s, l, c, max_age=4, min_hits=1, max_tracks=3)
    assert cnt[:, 0].tolist() == [3, 3, 3] and fl[:, 0].tolist() == [1, 1, 1]
    assert d[0, 0, :3, :4].tolist() == [list(f) for f in faces[:3]] and info[1, 0, :3, 0].tolist() == [1, 2, 3]


@pytest.mark.parametrize("M", (1, 3, 64, 65, 1024))
def test_lane_ownership(M):
    """Lanes own 1 slot, some none (M < 64), 1 and 2 (65), 16 (1024); 100 faces fill slots beyond the first 64, then most leave, come
    back shifted (ties between neighbours on the lattice), and new ones arrive."""
    faces = grid_faces(100, size=20.0, gap=4.0)
    moved = grid_faces(100, size=20.0, gap=4.0, dx=12.0)                    # half-way to the right neighbour: equal IoU with both
    frames = [[faces], [faces], [faces[::3]], [moved[::2] + faces[1::2]], [[]], [moved]]
    b, s, l, c = tables(frames, 104)
    _, _, _, cnt, fl = check_sequence(b, s, l, c, iou=0.2, max_age=2, min_hits=2, max_tracks=M, hold_grow=0.05)
    assert cnt[0, 0] == min(M, 100) and bool(fl[0, 0]) == (M < 100)


@pytest.mark.parametrize("seed", (0, 1))
def test_random_sequences(seed):
    b, s, l, c = random_sequence(seed)
    assert b.shape[:3] == (12, 3, 48) and c.max() > 20
    check_sequence(b, s, l, c, iou=0.3, max_age=2, min_hits=2, max_tracks=64, hold_grow=0.1)
    check_sequence(b, s, l, c, iou=0.6, max_age=1, min_hits=1, max_tracks=33)


# ---------------------------------------------------------------------------------------------- behind an engine
def _feed_until_faces(eng, rng, need=2, B=3):
    """The first of SOURCES whose forward_resized + threshold decode in network coordinates keeps ``need`` faces: (frames, result)."""
    tried = []
    for kind, hw in SOURCES:
        src = source_frames(rng, kind, (B,) + hw + (3,))
        eng.forward_resized_enqueue(src)
        base = eng.decode_threshold(0.3, 0.3, 64)
        tried.append((kind, hw, [len(d) for d, _ in base]))
        if sum(len(d) for d, _ in base) >= need:
            return src, base
    raise AssertionError("no source kept %d faces with the default weights: %s" % (need, tried))


def _blank_batch(eng, B=3):
    """A constant batch on which the decode keeps nothing."""
    for v in (128, 0, 255):
        eng.forward_resized_enqueue(np.full((B, 75, 101, 3), v, np.uint8))
        base = eng.decode_threshold(0.3, 0.3, 64)
        if sum(len(d) for d, _ in base) == 0:
            return base
    raise AssertionError("every constant batch keeps faces with the default weights")


def _same_update(got, want):
    for g, w in zip(got, want):
        for a, b in zip(g, (w[0], w[1], w[2][:, 0], w[2][:, 1], w[2][:, 2])):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (g, w)


def _state_error(call):
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        call()
    assert e.value.code == cfa._lib.CF_ESTATE


OK, STATE, VALUE = "ok", "CF_ESTATE", "ValueError"


def _outcome(call):
    try:
        call()
    except ValueError:
        return VALUE
    except cfa._lib.CenterFaceError as e:
        assert e.code == cfa._lib.CF_ESTATE, e
        return STATE
    return OK


def _expect(state, eng, trk, frames, **want):
    """Calls the named consumers of the current face rows, in the order given, and compares the outcome class of each; a refused call
    must leave its host frames as they were.  (A merge or an update that succeeds moves the context on: name it last.)"""
    keep = frames.copy()
    calls = dict(align=lambda: eng.align_faces(size=16),
                 align_frame=lambda: eng.align_faces_frame(keep, "bgr", size=16),
                 redact=lambda: eng.redact_faces(keep, "bgr", mode="solid", fill=(1, 2, 3)),
                 blur=lambda: eng.blur_faces(keep, "bgr", radius=2),
                 merge=lambda: eng.merge_tiles(max_out=64),
                 update=lambda: eng.track_update(trk))
    for name, outcome in want.items():
        keep[...] = frames
        assert _outcome(calls[name]) == outcome, (state, name)
        if outcome != OK:
            assert np.array_equal(keep, frames), (state, name)


def test_row_sources_state_table():
    """Which consumer accepts the context in which state: the decode's, the merge's and the tracker's rows, walked through a plain and a
    tiled forward.  Only the outcome class is asserted (random frames: every call is legal with any number of rows)."""
    rng = np.random.default_rng(5)
    eng = cfa.Engine(64, 96, max_batch=4, dtype="bf16")
    frames = rng.integers(0, 256, (2, 76, 102, 3), dtype=np.uint8)
    four = rng.integers(0, 256, (4, 76, 102, 3), dtype=np.uint8)
    decode = lambda: eng.decode_threshold(0.3, 0.3, 64)                     # noqa: E731
    everything = lambda o: dict(align=o, align_frame=o, redact=o, blur=o, merge=o, update=o)      # noqa: E731
    chips = lambda o: dict(align=OK, align_frame=o, redact=o, blur=o)       # noqa: E731
    # ---- a plain forward
    trk = cfa.Tracker(eng, 2, max_tracks=8)
    _expect("fresh", eng, trk, frames, **everything(STATE))
    eng.forward_resized_enqueue(frames)
    _expect("forward", eng, trk, frames, **everything(STATE))
    decode()
    _expect("decode", eng, trk, frames, **chips(OK), merge=STATE, update=OK)
    _expect("update", eng, trk, frames, **chips(OK), merge=STATE, update=STATE)
    decode()
    _expect("decode again", eng, trk, frames, **chips(OK), merge=STATE, update=OK)
    _expect("update again", eng, trk, frames, **chips(OK), merge=STATE, update=STATE)
    eng.upload_images(list(frames))
    _expect("upload", eng, trk, frames, **everything(STATE))
    eng.forward_enqueue(rng.standard_normal((2, 3, 64, 96)).astype(np.float32))
    _expect("float forward", eng, trk, frames, **everything(STATE))
    decode()
    _expect("float decode", eng, trk, frames, align=STATE, align_frame=OK, redact=OK, blur=OK, merge=STATE, update=OK)
    _expect("float update", eng, trk, frames, align=STATE, align_frame=OK, redact=OK, blur=OK, merge=STATE, update=STATE)
    trk.close()
    # ---- a tiled forward: 2 frames x 2 rectangles, rows in frame pixels (another coordinate space: another tracker)
    trk = cfa.Tracker(eng, 2, max_tracks=8)
    eng.forward_tiles_enqueue(frames, [(0, 0, 64, 48), (38, 28, 64, 48)], "bgr")
    _expect("tiles", eng, trk, frames, **everything(STATE))
    decode()
    _expect("tiles decode", eng, trk, frames, **chips(STATE), update=STATE, merge=OK)
    _expect("merge", eng, trk, frames, **chips(OK))
    _expect("merge, B = Bf * T", eng, trk, four, align_frame=VALUE, redact=VALUE, blur=VALUE)
    _expect("merge", eng, trk, frames, update=OK)
    _expect("tiles update", eng, trk, frames, **chips(OK), update=STATE, merge=OK)
    _expect("merge again", eng, trk, frames, **chips(OK), update=OK)
    _expect("tiles update again", eng, trk, frames, **chips(OK), update=STATE)
    decode()
    _expect("tiles decode again", eng, trk, frames, **chips(STATE), update=STATE, merge=OK)
    trk.close(), eng.close()


def test_engine_update_holds_tracks_and_the_redaction_covers_them():
    rng = np.random.default_rng(3)
    eng = cfa.Engine(64, 96, max_batch=3, dtype="bf16")
    opts = dict(iou=0.3, max_age=3, min_hits=1, max_tracks=70, hold_grow=0.1)
    trk = cfa.Tracker(eng, 3, **opts)
    ref = RefTracker(3, **opts)
    eng.forward_resized_enqueue(source_frames(rng, "noise", (3, 75, 101, 3)))
    _state_error(lambda: eng.track_update(trk))                             # a forward, but no decode
    src, base = _feed_until_faces(eng, rng)
    got, flags = eng.track_update(trk)
    want = [ref.update(b, d[:, :4], d[:, 4], l, len(d)) for b, (d, l) in enumerate(base)]
    _same_update(got, want)
    assert not flags.any() and sum(len(g[0]) for g in got) >= 2
    _state_error(lambda: eng.track_update(trk))                             # the same decode again: time would advance twice
    # a blank batch: without an update nothing is covered (today's behaviour); with it, the held tracks are
    blank = _blank_batch(eng)
    assert sum(len(d) for d, _ in blank) == 0
    frames = rng.integers(0, 256, (3, 76, 102, 3), dtype=np.uint8)
    yuv = rng.integers(0, 256, (3, 76 * 3 // 2, 102), dtype=np.uint8)
    for call in (lambda f, fmt: eng.redact_faces(f, fmt, mode="mosaic", shape="ellipse", cell=6), lambda f, fmt: eng.blur_faces(f, fmt, radius=2)):
        for src_frames, fmt in ((frames, "bgr"), (yuv, "nv12")):
            keep = src_frames.copy()
            call(keep, fmt)
            assert np.array_equal(keep, src_frames)
    got, flags = eng.track_update(trk)
    want = [ref.update(b, np.zeros((0, 4)), np.zeros(0), np.zeros((0, 10)), 0) for b in range(3)]
    _same_update(got, want)
    assert all((g[4] == 1).all() for g in got) and sum(len(g[0]) for g in got) >= 2
    boxes = np.concatenate([g[0][:, :4] for g in got])
    counts = np.array([len(g[0]) for g in got], np.int32)
    for src_frames, fmt in ((frames, "bgr"), (yuv, "nv12")):
        for kind in ("redact", "blur"):
            a, b = src_frames.copy(), src_frames.copy()
            if kind == "redact":
                eng.redact_faces(a, fmt, mode="mosaic", shape="ellipse", cell=6)
                ops.redact_faces(b, boxes, counts, (64, 96), fmt, mode="mosaic", shape="ellipse", cell=6)
            else:
                eng.blur_faces(a, fmt, radius=2)
                ops.blur_faces(b, boxes, counts, (64, 96), fmt, radius=2)
            assert np.array_equal(a, b) and not np.array_equal(a, src_frames), (fmt, kind)
    # chips of the held tracks come from their last-seen landmarks
    chips, offs, _ = eng.align_faces_frame(frames, "bgr", size=16)
    assert offs.tolist() == [0] + np.cumsum(counts).tolist()
    # a new decode of the same forward: the decode's rows again (none), and the tracker may advance again
    eng.decode_threshold(0.3, 0.3, 64)
    keep = frames.copy()
    eng.redact_faces(keep, "bgr", mode="solid", fill=(1, 2, 3))
    assert np.array_equal(keep, frames)
    # state and argument errors
    x = source_frames(rng, "binary", (3, 64, 96, 3))
    eng.forward_enqueue(x)
    eng.decode_threshold(0.3, 0.3, 64)
    eng.upload_images(list(x))
    _state_error(lambda: eng.track_update(trk))                             # an upload was started
    eng.forward_enqueue(x[:2])
    eng.decode_threshold(0.3, 0.3, 64)
    with pytest.raises(ValueError):
        eng.track_update(trk, stream0=2)                                    # streams 2, 3 of a tracker with 3
    with pytest.raises(ValueError):
        eng.track_update(trk, stream0=-1)
    other = cfa.Engine(64, 64, max_batch=1, dtype="bf16")
    other.forward_enqueue(x[:1, :, :64].copy())
    other.decode_threshold(0.3, 0.3, 64)
    with pytest.raises(ValueError):
        other.track_update(trk)                                             # rows of a 64 x 64 network in a tracker latched to 64 x 96
    other.close()
    # reset: the same frame again is all new tracks with new ids
    ref = RefTracker(3, **opts)
    trk2 = cfa.Tracker(eng.device, 3, **opts)                               # created by its first update
    eng.forward_resized_enqueue(src)
    base = eng.decode_threshold(0.3, 0.3, 64)
    for step in range(3):
        if step:
            eng.decode_threshold(0.3, 0.3, 64)                              # a new decode of the same forward: the same rows
        if step == 2:
            trk2.reset(), ref.reset()
        before = None if step == 0 else got
        got, _ = eng.track_update(trk2)
        _same_update(got, [ref.update(b, d[:, :4], d[:, 4], l, len(d)) for b, (d, l) in enumerate(base)])
        if step == 1:
            assert any((g[3] == 2).any() for g in got)                      # the same rows again: tracks were matched
    # after the reset every track is new (one hit) and its id above every id given before: ids are not reused
    assert sum(len(g[2]) for g in got) >= 2 and all((g[3] == 1).all() for g in got)
    assert all(len(g[2]) == 0 or len(p[2]) == 0 or g[2].min() > p[2].max() for g, p in zip(got, before))
    trk.close(), trk2.close(), eng.close()


def test_anonymize_without_a_tracker_is_unchanged_and_with_one_covers_the_dropout():
    rng = np.random.default_rng(31)
    hw = (76, 102)
    face = cfa.CenterFace(*hw, dtype="bf16", max_batch=3)
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        imgs = list(source_frames(rng, kind, (3,) + hw + (3,)))
        if sum(len(d) for d, _ in face.detect_batch(imgs)) >= 1:
            break
    opt = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    out0, dets0 = face.anonymize(imgs, **opt)
    out1, dets1 = face.anonymize(imgs, tracker=None, **opt)
    assert np.array_equal(out0, out1) and not np.array_equal(out0, np.stack(imgs))
    assert all(a.tobytes() == c.tobytes() and b.tobytes() == d.tobytes() for (a, b), (c, d) in zip(dets0, dets1))
    yuv = source_frames(rng, kind, (3, hw[0] * 3 // 2, hw[1]))
    oy0, _ = face.anonymize_yuv(yuv, "nv12", **opt)
    oy1, _ = face.anonymize_yuv(yuv, "nv12", tracker=None, **opt)
    assert np.array_equal(oy0, oy1)
    # with a tracker: the frame with faces is covered as before; the blank frame after it is covered where the faces were
    trk = cfa.Tracker(face.engine, 3, min_hits=1, max_age=2)
    out2, dets2 = face.anonymize(imgs, tracker=trk, **opt)
    assert np.array_equal(out2, out0)
    for v in (128, 0, 255):                                                 # a constant frame on which nothing is detected
        blank = [np.full(hw + (3,), v, np.uint8)] * 3
        if sum(len(d) for d, _ in face.detect_batch(blank)) == 0:
            break
    outn, detsn = face.anonymize(blank, **opt)
    assert sum(len(d) for d, _ in detsn) == 0 and np.array_equal(outn, np.stack(blank))
    outb, detsb = face.anonymize(blank, tracker=trk, **opt)
    assert sum(len(d) for d, _ in detsb) == 0
    # hold_grow = 0: the held boxes are the first frame's, so the covered samples are the same set -- there the first output holds the
    # fill, and nothing outside it was changed in either
    held = (outb != np.stack(blank)).any(axis=3)
    assert held.any() and (out0[held] == np.array([1, 2, 3], np.uint8)).all()
    assert not ((out0 != np.stack(imgs)).any(axis=3) & ~held).any()
    trk.close(), face.close()


def test_detect_tiled_with_a_tracker_holds_frame_pixel_tracks():
    from test_tiles import ENG_HW, FRAME_HW
    rng = np.random.default_rng(2)
    h, w = FRAME_HW
    face = cfa.CenterFace(ENG_HW[0], ENG_HW[1], dtype="bf16", max_batch=12)
    for kind in ("blocks", "binary", "noise", "blocks", "binary", "noise"):
        img = source_frames(rng, kind, (1, h, w, 3))
        got = face.detect_tiled(img)
        if len(got[0][0]) >= 2:
            break
    assert len(got[0][0]) >= 2
    opts = dict(iou=0.3, max_age=2, min_hits=1, max_tracks=1024, hold_grow=0.2)     # (the ten tiles of noise keep some two hundred rows)
    opt = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    trk, ref = cfa.Tracker(face.engine, 1, **opts), RefTracker(1, **opts)
    plain, f1 = img.copy(), img.copy()
    face.detect_tiled(plain, redact=opt)
    got1 = face.detect_tiled(f1, redact=opt, tracker=trk)
    assert np.array_equal(f1, plain) and got1[0][0].tobytes() == got[0][0].tobytes()
    ref.update(0, got[0][0][:, :4], got[0][0][:, 4], got[0][1], len(got[0][0]))
    # the second frame has its faces painted out: nothing is detected, the tracks are held in frame pixels and covered
    for v in (128, 0, 255):
        blank = np.full((1, h, w, 3), v, np.uint8)
        if len(face.detect_tiled(blank)[0][0]) == 0:
            break
    f2 = blank.copy()
    got2 = face.detect_tiled(f2, redact=opt, tracker=trk)
    assert len(got2[0][0]) == 0
    d, l, info, _ = ref.update(0, np.zeros((0, 4)), np.zeros(0), np.zeros((0, 10)), 0)
    assert (info[:, 2] == 1).all()
    want = ops.redact_faces(blank.copy(), d[:, :4], np.array([len(d)], np.int32), (h, w), "bgr", **opt)
    assert np.array_equal(f2, want) and not np.array_equal(f2, blank)
    # a third frame through the engine itself: the ids of the first frame, two frames missed
    rects = ops.tile_grid(h, w, ENG_HW, 16)
    face.engine.forward_tiles_enqueue(blank, rects, "bgr")
    face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets)
    _state_error(lambda: face.engine.track_update(trk))                     # tiled, but no merge yet
    face.engine.merge_tiles(max_out=face.max_dets)
    res, flags = face.engine.track_update(trk)
    _same_update(res, [ref.update(0, np.zeros((0, 4)), np.zeros(0), np.zeros((0, 10)), 0)])
    assert res[0][2].tolist() == list(range(1, len(got[0][0]) + 1)) and (res[0][4] == 2).all()
    trk.close(), face.close()


def test_two_engines_share_one_tracker():
    """A ring: two engines alternate six batches through one tracker, updates in the device form with nothing waited for in between;
    the tracked rows equal the restatement run over the batches in call order."""
    rng = np.random.default_rng(11)
    engs = [cfa.Engine(64, 96, max_batch=2, dtype="bf16") for _ in range(2)]
    src, _ = _feed_until_faces(engs[0], rng, need=2, B=2)
    again = source_frames(rng, "noise", src.shape)
    blank = np.full(src.shape, 128, np.uint8)
    batches = [src, src, again, blank, src, again]
    opts = dict(iou=0.3, max_age=1, min_hits=2, max_tracks=65, hold_grow=0.05)
    M = opts["max_tracks"]
    trk, ref = cfa.Tracker(engs[1], 2, **opts), RefTracker(2, **opts)
    sizes = (2 * M * 5 * 4, 2 * M * 10 * 4, 2 * M * 3 * 4, 8, 8)
    dev = [[e.device_alloc(n) for n in sizes] for e in engs]
    decoded, tracked = [], []

    def collect(e, bufs):
        decoded.append(e.decode_threshold(0.3, 0.3, 64))                    # waits for the enqueued decode; launches nothing
        host = [np.empty((2, M, 5), np.float32), np.empty((2, M, 10), np.float32), np.empty((2, M, 3), np.int32), np.empty(2, np.int32), np.empty(2, np.int32)]
        e.synchronize()
        for a, p in zip(host, bufs):
            e.memcpy_d2h(a, p)
        tracked.append(host)

    for i, batch in enumerate(batches):
        e, bufs = engs[i % 2], dev[i % 2]
        if i >= 2:
            collect(e, bufs)
        e.forward_resized_enqueue(batch)
        e.decode_threshold_enqueue(0.3, 0.3, 64)
        e.track_update_device(trk, 0, *bufs)
    for i in (4, 5):
        collect(engs[i % 2], dev[i % 2])
    assert sum(len(d) for base in decoded for d, _ in base) >= 6
    for base, (d, l, info, cnt, fl) in zip(decoded, tracked):
        for b, (bd, bl) in enumerate(base):
            wd, wl, wi, wf = ref.update(b, bd[:, :4], bd[:, 4], bl, len(bd))
            k = len(wd)
            assert cnt[b] == k and fl[b] == wf
            assert d[b, :k].tobytes() == wd.tobytes() and l[b, :k].tobytes() == wl.tobytes() and info[b, :k].tobytes() == wi.tobytes()
    for e, bufs in zip(engs, dev):
        for p in bufs:
            e.device_free(p)
    trk.close()
    for e in engs:
        e.close()


def _chunked_by_hand(face, trk, frames, fmt, opt):
    """anonymize / anonymize_yuv of five frames at max_batch = 2, restated from public Engine calls: image b of the chunk that starts at
    frame i continues tracker stream i + b."""
    eng, out, dets = face.engine, np.stack(list(frames)), []
    eng.set_rescale(face.scale_h, face.scale_w)
    for i in range(0, len(out), 2):
        if fmt == "bgr":
            eng.forward_resized_enqueue(np.stack(list(frames[i:i + 2])))
        else:
            eng.forward_yuv_enqueue(frames[i:i + 2], fmt)
        dets.extend(eng.decode_threshold(0.3, face.nms_thresh, face.max_dets))
        eng.track_update_device(trk, i)
        eng.cover_faces(out[i:i + 2], fmt, **opt)
    eng.set_rescale(0.0, 0.0)
    return out, dets


def test_chunked_anonymize_continues_tracker_stream_i_plus_b():
    """Five frames through max_batch = 2 (chunks at 0, 2, 4) with a tracker, twice: byte for byte the hand-written chunk loop on a second
    CenterFace and a second Tracker.  min_hits = 1 holds every face at once, so a chunk fed to the wrong streams would cover other boxes.
    BGR frames through anonymize, then NV12 frames of 76 x 102 through anonymize_yuv."""
    for fmt in ("bgr", "nv12"):
        _check_chunked_anonymize(fmt)


def _check_chunked_anonymize(fmt):
    rng = np.random.default_rng(17)
    face, face2 = (cfa.CenterFace(75, 101, dtype="bf16", max_batch=2) if fmt == "bgr" else cfa.CenterFace(76, 102, dtype="bf16", max_batch=2) for _ in range(2))
    tried = []
    for kind, hw in SOURCES:
        if fmt == "bgr":
            frames = list(source_frames(rng, kind, (5,) + hw + (3,)))
            n = [len(d) for d, _ in face.detect_batch(frames)]
        else:
            frames = source_frames(rng, kind, (5, 76 * 3 // 2, 102))
            n = [len(d) for d, _ in face.detect_yuv(frames, fmt)]
        tried.append((kind, hw, n))
        if sum(n) >= 2 and sum(n[2:]) >= 1:
            break
    else:
        raise AssertionError("no source holds two faces, one of them behind the first chunk, with the default weights: %s" % tried)
    before = np.stack(list(frames))
    opts = dict(min_hits=1, max_age=3, hold_grow=0.1)
    trk, trk2 = cfa.Tracker(face.engine, 5, **opts), cfa.Tracker(face2.engine, 5, **opts)
    opt = dict(mode="solid", shape="rect")
    for call in range(2):
        out, dets = face.anonymize(frames, tracker=trk, **opt) if fmt == "bgr" else face.anonymize_yuv(frames, fmt, tracker=trk, **opt)
        want, want_dets = _chunked_by_hand(face2, trk2, frames, fmt, opt)
        assert np.array_equal(out, want), call
        assert len(dets) == len(want_dets) == 5
        for (d, l), (wd, wl) in zip(dets, want_dets):
            assert d.shape == wd.shape and l.shape == wl.shape and d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes(), call
        assert np.array_equal(np.stack(list(frames)), before)
    assert (out[2:] != before[2:]).any()                                     # the second call covered a box behind the first chunk
    trk.close(), trk2.close(), face.close(), face2.close()
