"""The follower on the GPU: cf_op_follow against the numpy restatement (tests/follow_cases.py) bit for bit, then cf_track_follow behind an
engine -- key frames, a context that ran no forward, the consumers of the followed rows, the state rules, CenterFace.anonymize."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from follow_cases import FORMATS, LEARNED, LOST, MOVED, NONE, RefFollower, canvas, luma_of, planes_of, run_follow, view
from test_redact import redact_ref, source_frames
from test_track import _blank_batch, _feed_until_faces, _state_error
from track_cases import grid_faces, tables

pytestmark = pytest.mark.gpu


def check(faces, frames, fmt, space_hw, rows=None, S=1, **opts):
    """ops.follow_sequence == the restatement on dets, lms, info, counts, flags and moves, rows past the count unchanged (outputs
    prefilled).  faces[f][s] = the rows of frame f of stream s, frames[f * S + s] its plane tuple."""
    rows = rows or max(1, max(len(x) for per in faces for x in per))
    b, s, l, c = tables(faces, rows, S)
    F, M = len(faces), opts.get("max_tracks", 256)
    rng = np.random.default_rng(7)
    pre = dict(dets0=rng.standard_normal((F, S, M, 5)).astype(np.float32), lms0=rng.standard_normal((F, S, M, 10)).astype(np.float32),
               info0=rng.integers(-9, 9, (F, S, M, 3)).astype(np.int32), moves0=rng.integers(-9, 9, (F, S, M, 4)).astype(np.int32))
    want = run_follow(b, s, l, c, [luma_of(pl, fmt) for pl in frames], space_hw, **pre, **opts)
    got = ops.follow_sequence(b, s, l, c, frames, fmt, space_hw, opts.pop("detect", None), tiled=opts.pop("tiled", False), search=opts.pop("search", 4),
                              max_sad=opts.pop("max_sad", 4096), dets=pre["dets0"].copy(), lms_out=pre["lms0"].copy(), info=pre["info0"].copy(),
                              moves=pre["moves0"].copy(), **opts)
    for name, g, w in zip(("dets", "lms", "info", "counts", "flags", "moves"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
            raise AssertionError("%s differs at %s: got %s, want %s (%s)" % (name, bad[:4].tolist(), g[tuple(bad[0][:3])], w[tuple(bad[0][:3])], opts))
    return want


def moving(seed, fmt, h, w, shifts, S=1, pads=(0, 0), smooth=4):
    """frames[f * S + s]: stream s sees its own texture moved by shifts[f] (every stream by the same amount)."""
    rng = np.random.default_rng(seed)
    margin = 8 + max(max(abs(tx), abs(ty)) for tx, ty in shifts)
    cvs = [canvas(rng, fmt, h, w, margin, smooth) for _ in range(S)]
    return [planes_of(rng, fmt, view(cvs[s], h, w, margin, tx, ty), *pads) for tx, ty in shifts for s in range(S)]


def shifted(face, tx, ty):
    return (face[0] + tx, face[1] + ty, face[2] + tx, face[3] + ty)


# rows of a 64 x 64 network in frames of 96 x 128: fx = 2, fy = 1.5.  Sides in frame pixels: 16 (c = 1), 41 x 36 (c = 3, which does not
# divide it), 110 x 81 (c = 7: the window of 24 cells about the frame's middle crosses all four borders)
SPACE, FRAME = (64, 64), (96, 128)
SMALL, MID, LARGE = (8.0, 6.0, 16.0, 15.0), (38.25, 30.5, 58.75, 54.5), (4.5, 5.0, 59.5, 59.0)
SHIFTS = [(0, 0), (2, -1), (3, 3), (-4, 2)]


@pytest.mark.parametrize("pads", ((0, 0), (5, 3), (4, 8)), ids=lambda p: "pad%d_%d" % p)
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_and_pitch(fmt, pads):
    """Detect on the first frame, then follow three moved frames: three faces of three cell sizes, network space with fx != fy != 1."""
    frames = moving(1, fmt, *FRAME, SHIFTS, pads=pads)
    faces = [[[SMALL, MID, LARGE]]] + [[[]]] * 3
    want = check(faces, frames, fmt, SPACE, detect=[1, 0, 0, 0], min_hits=1, max_tracks=5, max_sad=65280)
    codes = want[5][:, 0, :3, 3]
    assert (codes[0] == LEARNED).all() and (codes[1:] == MOVED).all() and want[5][1:, 0, :3, :2].any()


@pytest.mark.parametrize("search", (1, 8))
def test_search_radius(search):
    frames = moving(2, "nv12", *FRAME, SHIFTS, smooth=2)
    want = check([[[SMALL, MID, LARGE]]] + [[[]]] * 3, frames, "nv12", SPACE, detect=[1, 0, 0, 0], search=search, min_hits=1, max_tracks=4, max_sad=2000)
    assert set(want[5][1:, 0, :3, 3].ravel().tolist()) <= {MOVED, LOST}


def test_frame_space_three_streams_and_skipped_rows():
    """Rows in frame pixels (a tiled path's), odd BGR frames, three streams with their own faces; a box without a side is skipped."""
    h, w = 75, 101
    frames = moving(3, "bgr", h, w, SHIFTS[:3], S=3, pads=(3, 0))
    per = [[(10, 12, 40, 44)], [(50.5, 20.25, 90.0, 60.0), (5, 5, 5, 5)], []]
    faces = [per, [[], [], []], [[], [(20, 20, 36, 36)], [(1, 2, 30, 33)]]]
    want = check(faces, frames, "bgr", (h, w), S=3, tiled=True, detect=[1, 0, 1], min_hits=1, max_age=2, max_tracks=4, hold_grow=0.1, max_sad=65280)
    assert want[5][0, 1, 1].tolist() == [0, 0, 0, NONE] and want[3].tolist() == [[1, 2, 0], [1, 2, 0], [1, 3, 1]]


def test_slot_64_and_dead_slots_between_live_ones():
    """max_tracks = 65: 65 faces are born, then only those of slots 0, 5 and 64 are seen again (max_age = 0 frees the others), and the
    three are followed: slots 0 and 64 share a lane of the emit."""
    h = w = 160
    frames = moving(4, "i420", h, w, [(0, 0), (0, 0), (1, 2), (-2, 1)], smooth=1)
    all65 = grid_faces(65, size=10.0, gap=4.0, per_row=9, dx=16.0, dy=16.0)        # (every window stays inside the frame)
    some = [all65[0], all65[5], all65[64]]
    want = check([[all65], [some], [[]], [[]]], frames, "i420", (h, w), rows=65, tiled=True, detect=[1, 1, 0, 0], min_hits=1, max_age=0, max_tracks=65, max_sad=0)
    assert want[3][:, 0].tolist() == [65, 3, 3, 3] and want[2][3, 0, :3, 0].tolist() == [1, 6, 65]
    assert want[5][2, 0, :3].tolist() == [[1, 2, 0, MOVED]] * 3 and want[5][3, 0, :3].tolist() == [[-3, -1, 0, MOVED]] * 3


def test_dropout_the_held_box_moves_with_the_face_and_grows_on_top():
    """detect, detect, miss, miss while the face moves 3 pixels a frame: the held box follows it, and hold_grow grows it about the new centre."""
    h = w = 128
    face = (40.0, 44.0, 80.0, 84.0)                                         # side 40: c = 3
    shifts = [(0, 0), (3, 0), (6, 3), (9, 6)]
    frames = moving(5, "nv21", h, w, shifts, pads=(4, 4), smooth=1)
    faces = [[[face]], [[shifted(face, 3, 0)]], [[]], [[]]]
    want = check(faces, frames, "nv21", (h, w), tiled=True, min_hits=2, max_age=5, max_tracks=3, hold_grow=0.25, max_sad=0)
    assert want[2][:, 0, 0].tolist() == [[1, 1, 0], [1, 2, 0], [1, 2, 1], [1, 2, 2]]
    assert want[5][:, 0, 0].tolist() == [[0, 0, 0, LEARNED], [0, 0, 0, LEARNED], [3, 3, 0, MOVED], [3, 3, 0, MOVED]]
    assert want[0][2, 0, 0, :4].tolist() == [46 - 5.0, 47 - 5.0, 86 + 5.0, 87 + 5.0]       # moved by (6, 3), half-size 20 grown by a quarter
    assert want[0][3, 0, 0, :4].tolist() == [49 - 10.0, 50 - 10.0, 89 + 10.0, 90 + 10.0]


def test_detect_every_fourth_frame():
    h, w = 96, 128
    shifts = [(f, (f * 2) % 5 - 2) for f in range(8)]
    frames = moving(6, "yv12", h, w, shifts, S=2, pads=(0, 2), smooth=2)
    a, b = (30.0, 20.0, 62.0, 50.0), (70.5, 40.5, 99.5, 80.0)
    faces = [[[shifted(a, *sh), shifted(b, *sh)], [shifted(b, *sh)]] if f % 4 == 0 else [[], []] for f, sh in enumerate(shifts)]
    want = check(faces, frames, "yv12", (h, w), S=2, tiled=True, detect=[f % 4 == 0 for f in range(8)], min_hits=1, max_tracks=4, max_sad=65280)
    codes = want[5][:, 0, :2, 3]
    assert (codes[::4] == LEARNED).all() and (np.delete(codes, [0, 4], axis=0) == MOVED).all()
    assert want[2][7, 0, :2].tolist() == [[1, 2, 0], [2, 2, 0]]               # hits count detections only


# ---------------------------------------------------------------------------------------------- behind an engine
OPTS = dict(iou=0.3, max_age=3, min_hits=1, max_tracks=70, hold_grow=0.1)


def _views(frames):
    return [(f.reshape(f.shape[0], -1),) for f in frames]


def _same_follow(got, want):
    dets, lms, info, counts, moves = got
    for b, (wd, wl, wi, wm) in enumerate(want):
        k = len(wd)
        assert counts[b] == k
        for name, g, w in (("dets", dets, wd), ("lms", lms, wl), ("info", info, wi), ("moves", moves, wm)):
            assert g[b, :k].tobytes() == w.tobytes(), (name, b, g[b, :k], w)


def _rows(got):
    dets, _, _, counts, _ = got
    return np.concatenate([dets[b, :counts[b], :4] for b in range(len(counts))]), counts


def test_engine_follow_feeds_the_consumers_of_the_newest_rows():
    rng = np.random.default_rng(3)
    eng = cfa.Engine(64, 96, max_batch=3, dtype="bf16")
    eng2 = cfa.Engine(64, 96, max_batch=3, dtype="bf16")                     # never runs a forward
    trk, ref = cfa.Tracker(eng, 5, **OPTS), RefFollower(5, (64, 96), search=3, max_sad=30000, **OPTS)
    fo = dict(search=3, max_sad=30000)
    src, base = _feed_until_faces(eng, rng)
    h, w = src.shape[1:3]
    frames = np.stack([canvas(rng, "bgr", 76, 102, 0, 4) for _ in range(3)])
    later = np.roll(frames, (2, 4), axis=(1, 2))                            # everything moves down 2, right 4 (the border wraps)
    # a tracker that was never updated has no space to follow in
    _state_error(lambda: eng.track_follow(frames, "bgr", trk, 1))
    chips0 = eng.align_faces(size=16)
    # ---- key frame: forward -> decode -> update -> follow (every slot learns) -> redact
    eng.track_update(trk, stream0=1)
    for b, (d, l) in enumerate(base):
        ref.update(1 + b, d[:, :4], d[:, 4], l, len(d))
    got = eng.track_follow(frames, "bgr", trk, 1, **fo)
    _same_follow(got, [ref.follow(1 + b, luma_of(v, "bgr")) for b, v in enumerate(_views(frames))])
    assert got[3].sum() >= 2 and (got[4][0, :got[3][0], 3] == LEARNED).all()
    _state_error(lambda: eng.track_update(trk, stream0=1))                  # the decode's rows went through an update already
    chips1 = eng.align_faces(size=16)                                       # names the decode's own rows: as before the follow
    assert all(np.array_equal(a, b) for a, b in zip(chips0, chips1))
    boxes, counts = _rows(got)
    a, want = frames.copy(), frames.copy()
    eng.redact_faces(a, "bgr", mode="mosaic", shape="ellipse", cell=6)
    redact_ref(_views(want), "bgr", boxes, counts, (64, 96), 76, 102, mode="mosaic", shape="ellipse", cell=6)
    assert np.array_equal(a, want) and not np.array_equal(a, frames)
    # ---- a dropout on eng (blank batch -> update: every track is held), then the follow of the moved frames on eng2
    _blank_batch(eng)
    eng.track_update(trk, stream0=1)
    for b in range(3):
        ref.update(1 + b, np.zeros((0, 4)), np.zeros(0), np.zeros((0, 10)), 0)
    _state_error(lambda: eng2.redact_faces(later.copy(), "bgr"))            # eng2 has no rows yet
    got = eng2.track_follow(later, "bgr", trk, 1, **fo)
    _same_follow(got, [ref.follow(1 + b, luma_of(v, "bgr")) for b, v in enumerate(_views(later))])
    codes = np.concatenate([got[4][b, :got[3][b], 3] for b in range(3)])
    assert (got[2][0, :got[3][0], 2] == 1).all() and LEARNED not in codes and (codes == MOVED).any()      # (a decoded box without a side is NONE)
    boxes, counts = _rows(got)
    a, want = later.copy(), later.copy()
    eng2.redact_faces(a, "bgr", mode="solid", shape="rect", fill=(1, 2, 3))
    redact_ref(_views(want), "bgr", boxes, counts, (64, 96), 76, 102, mode="solid", shape="rect", fill=(1, 2, 3))
    assert np.array_equal(a, want) and not np.array_equal(a, later)
    a, want = later.copy(), later.copy()
    eng2.blur_faces(a, "bgr", radius=2)
    ops.blur_faces(want, boxes, counts, (64, 96), "bgr", radius=2)
    assert np.array_equal(a, want)
    n = int(counts.sum())
    flat = lambda x, k: np.concatenate([x[b, :counts[b]] for b in range(3)]).reshape(n, k)      # noqa: E731
    a, want = later.copy(), later.copy()
    eng2.draw_faces(a, "bgr", label="id")
    ops.draw_faces(want, boxes, flat(got[0], 5)[:, 4], counts, (64, 96), "bgr", lms=flat(got[1], 10), info=flat(got[2], 3), label="id")
    assert np.array_equal(a, want) and not np.array_equal(a, later)
    _, offs, _ = eng2.align_faces_frame(later, "bgr", size=16)
    assert offs.tolist() == [0] + np.cumsum(counts).tolist()
    _state_error(lambda: eng2.align_faces(size=16))                         # the decode's own rows: eng2 has none
    _state_error(lambda: eng2.track_update(trk, stream0=1))
    # eng still holds its update's rows (held where they were); its own follow replaces them, a new forward ends that
    got1 = eng.track_follow(later, "bgr", trk, 1, **fo)
    _same_follow(got1, [ref.follow(1 + b, luma_of(v, "bgr")) for b, v in enumerate(_views(later))])
    eng.forward_resized_enqueue(src)
    _state_error(lambda: eng.redact_faces(later.copy(), "bgr"))
    eng.decode_threshold(0.3, 0.3, 64)
    eng.track_update(trk, stream0=1)                                        # and the tracker may advance again
    # ---- argument errors: before any GPU work
    for call in (lambda: eng.track_follow(frames, "bgr", trk, 3), lambda: eng.track_follow(frames, "bgr", trk, -1),
                 lambda: eng.track_follow(frames, "bgr", trk, 1, search=0), lambda: eng.track_follow(frames, "bgr", trk, 1, max_sad=65281),
                 lambda: eng.track_follow(np.concatenate([frames, frames[:1]]), "bgr", trk, 0)):      # B = 4 > max_batch
        with pytest.raises(ValueError):
            call()
    trk.close(), eng.close(), eng2.close()


def test_tiled_tracker_refuses_frames_of_another_size():
    rng = np.random.default_rng(5)
    eng = cfa.Engine(64, 96, max_batch=4, dtype="bf16")
    frames = rng.integers(0, 256, (2, 76, 102, 3), dtype=np.uint8)
    trk = cfa.Tracker(eng, 2, max_tracks=8)
    eng.forward_tiles_enqueue(frames, [(0, 0, 64, 48), (38, 28, 64, 48)], "bgr")
    eng.decode_threshold(0.3, 0.3, 64)
    eng.merge_tiles(max_out=64)
    eng.track_update(trk)
    with pytest.raises(ValueError):
        eng.track_follow(np.zeros((2, 64, 96, 3), np.uint8), "bgr", trk)
    keep = frames.copy()
    dets, _, _, counts, moves = eng.track_follow(keep, "bgr", trk)
    assert np.array_equal(keep, frames) and all((moves[b, :counts[b], 3] == LEARNED).all() for b in range(2))
    with pytest.raises(ValueError):                                        # the followed rows are in frame pixels: the frames must be the tiled size
        eng.redact_faces(np.zeros((2, 64, 96, 3), np.uint8), "bgr")
    eng.redact_faces(keep, "bgr", mode="solid")
    trk.close(), eng.close()


def _by_hand(face, trk, frames, opt, detect, fo):
    """anonymize(..., follow=fo, detect=detect) of three frames at max_batch = 2, restated from public Engine calls."""
    eng, out, res, moves = face.engine, np.stack(list(frames)), [], []
    if detect:
        eng.set_rescale(face.scale_h, face.scale_w)
    for i in range(0, len(out), 2):
        if detect:
            eng.forward_resized_enqueue(np.stack(list(frames[i:i + 2])))
            res.extend(eng.decode_threshold(0.3, face.nms_thresh, face.max_dets))
            eng.track_update_device(trk, i)
        d, l, _, n, m = eng.track_follow(out[i:i + 2], "bgr", trk, i, **fo)
        moves.extend(m[b, :n[b]] for b in range(len(n)))
        if not detect:
            fx, fy = out.shape[2] / float(face.img_w_new), out.shape[1] / float(face.img_h_new)
            for b in range(len(n)):
                dd, ll = d[b, :n[b]].astype(np.float64), l[b, :n[b]].astype(np.float64)
                dd[:, 0:4:2] *= fx; dd[:, 1:4:2] *= fy; ll[:, 0::2] *= fx; ll[:, 1::2] *= fy      # noqa: E702
                res.append((dd, ll))
        eng.cover_faces(out[i:i + 2], "bgr", **opt)
    eng.set_rescale(0.0, 0.0)
    return out, res, moves


def test_anonymize_detects_once_then_follows_the_moved_faces_in_two_chunks():
    rng = np.random.default_rng(31)
    hw = (75, 101)
    face, face2 = (cfa.CenterFace(*hw, dtype="bf16", max_batch=2) for _ in range(2))
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        imgs = list(source_frames(rng, kind, (3,) + hw + (3,)))
        n = [len(d) for d, _ in face.detect_batch(imgs)]
        if sum(n) >= 2 and n[2] >= 1:                                       # a face behind the first chunk
            break
    else:
        raise AssertionError("no source holds a face in the third frame with the default weights")
    nxt = [np.roll(im, (2, 4), axis=(0, 1)) for im in imgs]                # everything moves down 2, right 4
    opt = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    fo = dict(search=4, max_sad=65280)
    with pytest.raises(ValueError):
        face.anonymize(imgs, follow=True, **opt)                            # follow needs a tracker
    trk, trk2 = (cfa.Tracker(f.engine, 3, min_hits=1, max_age=3) for f in (face, face2))
    plain, dets_plain = face.anonymize(imgs, **opt)
    out, dets = face.anonymize(imgs, tracker=trk, follow=fo, **opt)
    want, want_dets, _ = _by_hand(face2, trk2, imgs, opt, True, fo)
    assert np.array_equal(out, want) and np.array_equal(out, plain)         # a key frame: the detections, where they are
    for (d, l), (wd, wl) in zip(dets, want_dets):
        assert d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes()
    out2, dets2 = face.anonymize(nxt, tracker=trk, detect=False, follow=fo, **opt)
    want2, want_dets2, moves = _by_hand(face2, trk2, nxt, opt, False, fo)
    assert np.array_equal(out2, want2)
    for (d, l), (wd, wl) in zip(dets2, want_dets2):
        assert d.dtype == np.float64 and d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes()
    assert [len(d) for d, _ in dets2] == n
    codes = np.concatenate([m[:, 3] for m in moves])                       # (a decoded box without a side is NONE)
    assert set(codes.tolist()) <= {NONE, MOVED} and any(m[:, :2].any() for m in moves)
    covered, before = (out2 != np.stack(nxt)).any(axis=3), (out != np.stack(imgs)).any(axis=3)
    assert covered[2].any() and not np.array_equal(covered, before)         # the third frame (second chunk) too, and not where the faces were
    trk.close(), trk2.close(), face.close(), face2.close()
