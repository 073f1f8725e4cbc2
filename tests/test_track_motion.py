"""The tracker with constant-velocity prediction on the GPU: cf_op_track_ex / cf_op_follow_ex against the numpy restatement
(tests/motion_cases.py) on every byte of every table -- the velocities included --, the scenarios of the statement one by one, the equality
with the trackers without the model where nothing moves or no model is asked for, and one engine-level run on the normal route."""
import ctypes as C

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from follow_cases import LEARNED, LOST, MOVED, canvas, luma_of, planes_of, run_follow, view
from motion_cases import A, crowded, drifting_sequence, run_motion_follow, run_motion_sequence, shifted
from track_cases import F32, grid_faces, iou32, random_sequence, run_sequence, tables
from weak_cases import mixed_random_sequence, run_weak_sequence

pytestmark = pytest.mark.gpu

NAMES = ("dets", "lms", "info", "counts", "flags", "vel")
OPTS = dict(iou=0.3, max_age=3, min_hits=2, hold_grow=0.1)
TWO24 = 16777216.0


def _same(got, want, what, names=NAMES):
    assert len(got) == len(want) == len(names), what
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
            raise AssertionError("%s: %s differs at %s: got %s, want %s" % (what, name, bad[:4].tolist(), g[tuple(bad[0][:3])], w[tuple(bad[0][:3])]))


def check_motion(boxes, scores, lms, counts, motion=True, birth_score=None, weak_iou=None, **opts):
    """ops.track_sequence(motion=, vel=True) == the restatement on dets, lms, info, counts, flags and vel, the bytes past the counts that
    the caller filled included.  Returns the restatement's tables."""
    F, S = counts.shape
    M = opts.get("max_tracks", 256)
    rng = np.random.default_rng(7)
    d0 = rng.standard_normal((F, S, M, 5)).astype(np.float32)
    l0 = rng.standard_normal((F, S, M, 10)).astype(np.float32)
    i0 = rng.integers(-9, 9, (F, S, M, 3)).astype(np.int32)
    v0 = rng.standard_normal((F, S, M, 2)).astype(np.float32)
    weak = {} if birth_score is None else dict(birth_score=birth_score, weak_iou=0.5 if weak_iou is None else weak_iou)
    want = run_motion_sequence(boxes, scores, lms, counts, motion, dets0=d0, lms0=l0, info0=i0, vel0=v0, **weak, **opts)
    got = ops.track_sequence(boxes, scores, lms, counts, d0.copy(), l0.copy(), i0.copy(), motion=motion, vel=v0.copy(), **weak, **opts)
    _same(got, want, (motion, weak, opts))
    return want


def box_of(dets, f, k, s=0):
    return tuple(dets[f, s, k, :4].tolist())


def pad_for(M, faces=1):
    """The static crowd in front of a scenario with ``faces`` faces in a tracker of M slots: its faces take the last slots."""
    return min(M - faces, 70 - faces)


# ---------------------------------------------------------------------------------------------- the scenarios of the statement
@pytest.mark.parametrize("M", (1, 65, 130))
def test_a_dropout_is_held_where_the_face_went_and_the_face_keeps_its_id(M):
    k = pad_for(M)
    frames = crowded([[A], [shifted(A, 20)], [], [shifted(A, 60)]], k)
    b, s, l, c = tables(frames, k + 1)
    o = dict(OPTS, hold_grow=0.0, max_tracks=M)
    d, lm, info, cnt, fl, vel = check_motion(b, s, l, c, **o)
    assert cnt[:, 0].tolist() == [k + 1] * 4 and not fl.any()
    assert info[:, 0, k].tolist() == [[k + 1, 1, 0], [k + 1, 2, 0], [k + 1, 2, 1], [k + 1, 3, 0]]
    assert box_of(d, 2, k) == shifted(A, 40) and vel[:, 0, k].tolist() == [[0, 0], [20, 0], [20, 0], [20, 0]]
    assert (lm[2, 0, k] - lm[1, 0, k]).tolist() == [20, 0] * 5                 # the landmarks coast with the box
    assert not vel[:, 0, :k].any()                                            # the crowd stands still
    # the tracker without the model holds A+20 and spends a new id
    plain = ops.track_sequence(b, s, l, c, **o)
    _same(plain, run_sequence(b, s, l, c, **o), "plain", NAMES[:5])
    assert box_of(plain[0], 2, k) == shifted(A, 20) and plain[2][2, 0, k].tolist() == [k + 1, 2, 1]
    if M > k + 1:
        assert plain[2][3, 0, k + 1].tolist() == [k + 2, 1, 0]
    else:
        assert plain[4][3, 0] == 1                                            # no slot for it: dropped


@pytest.mark.parametrize("M", (1, 65, 130))
def test_two_missed_frames_divide_the_residual_by_three(M):
    """Rematched at A+87 where A+80 was expected: the residual 7 over g + 1 = 3 is inexact, which pins the order of the operations."""
    k = pad_for(M)
    frames = crowded([[A], [shifted(A, 20)], [], [], [shifted(A, 87)], []], k)
    b, s, l, c = tables(frames, k + 1)
    for gain in (0.5, 0.3):
        d, _, info, _, _, vel = check_motion(b, s, l, c, dict(gain=gain), max_tracks=M, **OPTS)
        assert info[3, 0, k].tolist() == [k + 1, 2, 2] and info[4, 0, k].tolist() == [k + 1, 3, 0] and box_of(d, 4, k) == shifted(A, 87)
        third = F32(F32(7) / F32(3))
        assert vel[4, 0, k, 0] == F32(F32(20) + F32(F32(gain) * third)) and vel[4, 0, k, 1] == 0
        assert d[5, 0, k, 0] > 1087 + 15                                      # and coasts on by the new velocity (grown by hold_grow)


@pytest.mark.parametrize("damp", (0.5, 0.0, 1.0))
def test_three_coasts_with_a_fractional_velocity(damp):
    step = (2.3, -1.7)
    frames = crowded([[A], [shifted(A, *step)], [], [], [], [shifted(A, 6.0, -4.0)]], 66)
    b, s, l, c = tables(frames, 67)
    d, _, info, _, _, vel = check_motion(b, s, l, c, dict(damp=damp), max_tracks=67, **dict(OPTS, hold_grow=0.0))
    v0 = vel[1, 0, 66].copy()
    assert abs(float(v0[0]) - 2.3) < 1e-3 and abs(float(v0[1]) + 1.7) < 1e-3
    assert info[2:5, 0, 66, 2].tolist() == [1, 2, 3] and info[5, 0, 66].tolist() == [67, 3, 0]
    assert vel[2, 0, 66].tobytes() == (v0 * F32(damp)).astype(np.float32).tobytes()
    if damp == 0.0:
        assert not vel[2:5, 0, 66].any() and box_of(d, 2, 66) == box_of(d, 3, 66) == box_of(d, 4, 66)      # one coast, then it stands


def test_the_second_sighting_is_taken_whole_and_the_third_by_gain():
    frames = crowded([[A], [shifted(A, 20)], [shifted(A, 50)], [], [shifted(A, 100, 3)]], 64)
    b, s, l, c = tables(frames, 65)
    seen = {}
    for gain in (1.0, 0.25):
        _, _, info, _, _, vel = check_motion(b, s, l, c, dict(gain=gain), max_tracks=65, **OPTS)
        assert info[2, 0, 64].tolist() == [65, 3, 0]
        seen[gain] = vel[:, 0, 64, 0].tolist()
    assert seen[1.0][:3] == [0, 20, 30] and seen[0.25][:3] == [0, 20, 22.5]


@pytest.mark.parametrize("M", (3, 65, 130))
def test_prediction_decides_the_arg_max(M):
    """Slot k moves +20 per frame and is stored at A, slot k + 1 stands at A+24; the rows are A+20, then A+24.  Measured against the stored
    boxes the first row goes to slot k + 1 (0.822 against 0.344) and the second is new; against the predicted ones both keep their ids."""
    assert iou32(A, shifted(A, 20)) == F32(1071.0) / F32(3111.0) and iou32(shifted(A, 24), shifted(A, 20)) == F32(1887.0) / F32(2295.0)
    assert iou32(A, shifted(A, 24)) < F32(0.3)
    k = pad_for(M, 2)
    frames = crowded([[shifted(A, -20), shifted(A, 24)], [A, shifted(A, 24)], [shifted(A, 20), shifted(A, 24)]], k)
    b, s, l, c = tables(frames, k + 2)
    want = run_motion_sequence(b, s, l, c, max_tracks=M, **OPTS)                # the numbers in the restatement first
    assert want[2][2, 0, k:k + 2].tolist() == [[k + 1, 3, 0], [k + 2, 3, 0]] and not want[4].any()
    d, _, info, cnt, fl, vel = check_motion(b, s, l, c, max_tracks=M, **OPTS)
    assert box_of(d, 2, k) == shifted(A, 20) and box_of(d, 2, k + 1) == shifted(A, 24) and cnt[2, 0] == k + 2
    assert vel[2, 0, k:k + 2].tolist() == [[20, 0], [0, 0]]
    plain = ops.track_sequence(b, s, l, c, max_tracks=M, **OPTS)
    _same(plain, run_sequence(b, s, l, c, max_tracks=M, **OPTS), "plain", NAMES[:5])
    assert plain[2][2, 0, k].tolist() == [k + 1, 2, 1]                        # the mover is held where it was
    assert plain[2][2, 0, k + 1].tolist() == [k + 2, 3, 0] and box_of(plain[0], 2, k + 1) == shifted(A, 20)      # its row went to the other
    assert (plain[2][2, 0, k + 2].tolist() == [k + 3, 1, 0]) if M > k + 2 else (plain[4][2, 0] == 1)


@pytest.mark.parametrize("M", (3, 65, 130))
def test_a_tie_between_two_predicted_boxes_goes_to_the_lowest_slot(M):
    """Slot k comes from the left at +8, slot k + 1 from the right at -8: both are expected at A+8, where the one row of the frame lies."""
    k = pad_for(M, 2)
    frames = crowded([[shifted(A, -8), shifted(A, 24)], [A, shifted(A, 16)], [shifted(A, 8)]], k)
    b, s, l, c = tables(frames, k + 2)
    d, _, info, cnt, fl, vel = check_motion(b, s, l, c, max_tracks=M, **dict(OPTS, hold_grow=0.0))
    assert vel[1, 0, k:k + 2].tolist() == [[8, 0], [-8, 0]]
    assert info[2, 0, k:k + 2].tolist() == [[k + 1, 3, 0], [k + 2, 2, 1]] and cnt[2, 0] == k + 2
    assert box_of(d, 2, k) == box_of(d, 2, k + 1) == shifted(A, 8)             # one took the row, the other coasted onto it


@pytest.mark.parametrize("M", (1, 65, 130))
def test_a_weak_row_matches_the_predicted_box_of_a_confirmed_held_track(M):
    k = pad_for(M)
    S, W = 0.8, 0.2
    at = lambda box, sc: tuple(box) + (sc,)      # noqa: E731
    frames = crowded([[at(A, S)], [at(shifted(A, 20), S)], [], [at(shifted(A, 60), W)], [at(shifted(A, 80), W)]], k)
    b, s, l, c = tables(frames, k + 1)
    assert iou32(shifted(A, 40), shifted(A, 60)) < F32(0.5)                    # the stored box would miss weak_iou
    d, _, info, cnt, fl, vel = check_motion(b, s, l, c, birth_score=0.3, weak_iou=0.5, max_tracks=M, **OPTS)
    assert info[2:, 0, k].tolist() == [[k + 1, 2, 1], [k + 1, 3, 0], [k + 1, 4, 0]] and fl[:, 0].tolist() == [0, 0, 0, 2, 2]
    assert box_of(d, 3, k) == shifted(A, 60) and vel[3, 0, k].tolist() == [20, 0]
    # the same tracker without the model discards the weak row and goes on holding
    weak = ops.track_sequence(b, s, l, c, birth_score=0.3, weak_iou=0.5, max_tracks=M, **OPTS)
    _same(weak, run_weak_sequence(b, s, l, c, birth_score=0.3, weak_iou=0.5, max_tracks=M, **OPTS), "weak", NAMES[:5])
    assert weak[2][3, 0, k].tolist() == [k + 1, 2, 2] and weak[4][3, 0] == 0
    # a tentative track refuses the weak row that lies on it
    frames = crowded([[at(A, S)], [at(A, W)], [at(A, S)]], k)
    b, s, l, c = tables(frames, k + 1)
    _, _, info, cnt, fl, _ = check_motion(b, s, l, c, birth_score=0.3, weak_iou=0.5, max_tracks=M, **OPTS)
    assert cnt[:, 0].tolist() == [k + 1, k, k + 1] and not fl.any() and info[2, 0, k].tolist() == [k + 2, 1, 0]


def test_a_corner_beyond_two_to_the_24_is_skipped_and_one_on_it_is_not():
    on, beyond = (TWO24 - 40, 1000, TWO24, 1050), (TWO24 - 38, 2000, TWO24 + 2, 2050)
    low = (-TWO24 - 2, 3000, -TWO24 + 40, 3050)
    assert F32(TWO24 + 2) > F32(TWO24)
    frames = [[[beyond, on, low, (0, -TWO24, 40, 50 - TWO24)]], [[on, beyond]], [[beyond]]]
    b, s, l, c = tables(frames, 4)
    for M in (3, 65):
        d, _, info, cnt, fl, _ = check_motion(b, s, l, c, max_tracks=M, **dict(OPTS, min_hits=1))
        assert cnt[:, 0].tolist() == [2, 2, 2] and not fl.any()
        assert box_of(d, 0, 0) == on and info[1, 0, 0].tolist() == [1, 2, 0] and info[2, 0, :2, 2].tolist() == [1, 2]
    # without the model such rows are rows like any other
    assert ops.track_sequence(b, s, l, c, max_tracks=3, **dict(OPTS, min_hits=1))[3][0, 0] == 3


@pytest.mark.parametrize("M", (1, 65))
def test_a_coast_across_two_to_the_24_frees_the_slot(M):
    k = pad_for(M)
    B1 = (TWO24 - 60, 1000, TWO24 - 20, 1050)
    frames = crowded([[shifted(B1, -16)], [B1], [], [], [(5000, 5000, 5040, 5050)], []], k)
    b, s, l, c = tables(frames, k + 1)
    d, _, info, cnt, fl, vel = check_motion(b, s, l, c, max_tracks=M, **dict(OPTS, max_age=5, hold_grow=0.0, min_hits=1))
    assert vel[1, 0, k].tolist() == [16, 0] and box_of(d, 2, k) == shifted(B1, 16) and d[2, 0, k, 2] == TWO24 - 4
    assert cnt[:, 0].tolist() == [k + 1, k + 1, k + 1, k, k + 1, k + 1]        # the second coast would reach 2^24 + 12: freed
    # ... and the slot, born again, coasts by zero: a reused slot never inherits a velocity
    assert info[4:, 0, k].tolist() == [[k + 2, 1, 0], [k + 2, 1, 1]] and not vel[4:, 0, k].any()
    assert box_of(d, 5, k) == (5000, 5000, 5040, 5050)


def test_a_slot_freed_by_age_and_born_again_coasts_by_zero():
    far_away = (3000, 3000, 3040, 3050)
    frames = crowded([[A], [shifted(A, 20)], [], [], [far_away], [], [shifted(far_away, 5)]], 64)
    b, s, l, c = tables(frames, 65)
    d, _, info, cnt, _, vel = check_motion(b, s, l, c, max_tracks=65, **dict(OPTS, max_age=1, min_hits=1, hold_grow=0.0))
    assert cnt[:, 0].tolist() == [65, 65, 65, 64, 65, 65, 65] and vel[2, 0, 64].tolist() == [20, 0]
    assert info[4:, 0, 64].tolist() == [[66, 1, 0], [66, 1, 1], [66, 2, 0]] and box_of(d, 5, 64) == far_away
    assert not vel[4:6, 0, 64].any() and vel[6, 0, 64].tolist() == [2.5, 0]   # g = 1: the displacement 5 over two frames


def test_stationary_faces_give_the_plain_trackers_tables_and_no_velocity():
    rng = np.random.default_rng(11)
    faces = grid_faces(90, size=20.0, gap=6.0)
    frames = []
    for f in range(10):
        per = []
        for s in range(2):
            here = [fc for i, fc in enumerate(faces) if i < 40 + 5 * f and rng.random() > (0.3 if f % 4 else 0.8)]
            per.append([here[i] for i in rng.permutation(len(here))])
        frames.append(per)
    b, s, l, c = tables(frames, 90, S=2)
    for M, o in ((65, dict(iou=0.3, max_age=2, min_hits=2, hold_grow=0.1)), (130, dict(iou=0.5, max_age=1, min_hits=1, hold_grow=0.0))):
        got = check_motion(b, s, l, c, dict(gain=0.7, damp=0.5), max_tracks=M, **o)
        rng7 = np.random.default_rng(7)                                       # (check_motion's prefill of dets, lms and info)
        F, S = c.shape
        pre = (rng7.standard_normal((F, S, M, 5)).astype(np.float32), rng7.standard_normal((F, S, M, 10)).astype(np.float32),
               rng7.integers(-9, 9, (F, S, M, 3)).astype(np.int32))
        plain = ops.track_sequence(b, s, l, c, *[p.copy() for p in pre], max_tracks=M, **o)
        _same(got[:5], plain, "stationary", NAMES[:5])
        live = np.arange(M)[None, None, :] < got[3][:, :, None]
        assert not got[5][live].any() and got[5][live].tobytes() == bytes(got[5][live].nbytes)
        assert (got[2][..., 2][live] > 0).any() and got[3].max() > 40 and got[3].min() < got[3].max()      # held rows, births, deaths


def _track_ex_raw(b, s, l, c, o, wo, mo, M, vel=None):
    F, S, rows, _ = b.shape
    P = cfa._lib.ptr
    out = (np.zeros((F, S, M, 5), np.float32), np.zeros((F, S, M, 10), np.float32), np.zeros((F, S, M, 3), np.int32), np.zeros((F, S), np.int32),
           np.zeros((F, S), np.int32))
    rc = cfa._lib.lib().cf_op_track_ex(0, C.byref(o), None if wo is None else C.byref(wo), None if mo is None else C.byref(mo), S, F, rows,
                                       P(np.ascontiguousarray(b, np.float32)), P(np.ascontiguousarray(s, np.float32)), P(np.ascontiguousarray(l, np.float32)),
                                       P(np.ascontiguousarray(c, np.int32)), *[P(x) for x in out], None if vel is None else P(vel))
    assert rc == 0, cfa._lib.lib().cf_op_last_error()
    return out


def test_without_motion_options_the_new_entry_point_is_the_old_ones():
    o = dict(iou=0.3, max_age=2, min_hits=2, max_tracks=64, hold_grow=0.1)
    b, s, l, c = random_sequence(0)
    vel = np.full((12, 3, 64, 2), 5.0, np.float32)
    got = _track_ex_raw(b, s, l, c, cfa._lib.track_opts(**o), None, None, 64, vel)
    _same(got, ops.track_sequence(b, s, l, c, **o), "plain", NAMES[:5])
    assert (vel == 5.0).all()                                                 # left alone
    b, s, l, c = mixed_random_sequence(0)
    o["max_tracks"] = 65
    got = _track_ex_raw(b, s, l, c, cfa._lib.track_opts(**o), cfa._lib.track_weak_opts(0.3, 0.5), None, 65)
    want = ops.track_sequence(b, s, l, c, birth_score=0.3, weak_iou=0.5, **o)
    _same(got, want, "weak", NAMES[:5])
    assert (want[4] & 2).any()
    # with them and no velocity table the other tables are the same as with one
    mo = cfa._lib.track_motion_opts()
    _same(_track_ex_raw(b, s, l, c, cfa._lib.track_opts(**o), None, mo, 65), ops.track_sequence(b, s, l, c, motion=True, vel=True, **o)[:5],
          "no vel", NAMES[:5])


@pytest.mark.parametrize("seed", (0, 1))
def test_random_sequences_of_drifting_faces(seed):
    b, s, l, c = drifting_sequence(seed)
    assert b.shape[:3] == (12, 3, 48) and c.max() > 20 and (s[..., 0] < 0.3).any() and (s[..., 0] > 0.3).any()
    got = check_motion(b, s, l, c, iou=0.3, max_age=2, min_hits=2, max_tracks=64, hold_grow=0.1)
    live = np.arange(64)[None, None, :] < got[3][:, :, None]
    assert got[5][live].any() and (got[2][..., 2][live] > 0).any()            # velocities were learnt, tracks were held
    plain = ops.track_sequence(b, s, l, c, iou=0.3, max_age=2, min_hits=2, max_tracks=64, hold_grow=0.1)
    assert plain[3].tobytes() != got[3].tobytes()                             # and the model made a difference: other tracks are alive
    check_motion(b, s, l, c, dict(gain=0.9, damp=0.75), iou=0.5, max_age=1, min_hits=1, max_tracks=33)
    got = check_motion(b, s, l, c, dict(gain=0.25, damp=1.0), birth_score=0.3, weak_iou=0.4, iou=0.3, max_age=3, min_hits=2, max_tracks=65, hold_grow=0.05)
    assert (got[4] & 2).any()


# ---------------------------------------------------------------------------------------------- with the follower
FACE, STEP, FH, FW = (8.0, 20.0, 31.0, 43.0), 12, 64, 96


def _moving_scene(fmt, F=5, dropout=(2,)):
    """A texture that moves STEP pixels to the right per frame and the box of a face on it, detected in every frame but ``dropout``."""
    rng = np.random.default_rng(21)
    margin = 8 + STEP * F
    cv = canvas(rng, fmt, FH, FW, margin, 4)
    frames = [planes_of(rng, fmt, view(cv, FH, FW, margin, STEP * f, 0), 4, 2) for f in range(F)]
    rows = [[[] if f in dropout else [shifted(FACE, STEP * f)]] for f in range(F)]
    return frames, tables(rows, 2)


@pytest.mark.parametrize("fmt", ("bgr", "nv12"))
def test_behind_a_coast_the_follower_follows_from_the_predicted_place(fmt):
    frames, (b, s, l, c) = _moving_scene(fmt)
    lumas = [luma_of(pl, fmt) for pl in frames]
    o = dict(iou=0.3, max_age=3, min_hits=2, max_tracks=3, hold_grow=0.0)
    fo = dict(search=4, max_sad=2000)
    want = run_motion_follow(b, s, l, c, lumas, (FH, FW), True, **fo, **o)
    got = ops.follow_sequence(b, s, l, c, frames, fmt, (FH, FW), motion=True, **fo, **o)
    _same(got, want, fmt, NAMES[:5] + ("moves",))
    d, _, info, cnt, _, moves = got
    assert cnt[:, 0].tolist() == [1] * 5 and info[:, 0, 0].tolist() == [[1, 1, 0], [1, 2, 0], [1, 2, 1], [1, 3, 0], [1, 4, 0]]
    assert moves[[0, 1, 3, 4], 0, 0, 3].tolist() == [LEARNED] * 4
    assert moves[2, 0, 0].tolist() == [0, 0, 0, MOVED]                         # at the dropout: found where it was expected, never LEARNED
    assert box_of(d, 2, 0) == shifted(FACE, 2 * STEP)
    # the follower alone looks about the stale centre, STEP = 12 pixels away and beyond its 4 cells of 2 pixels: it loses the face
    plain_want = run_follow(b, s, l, c, lumas, (FH, FW), **fo, **o)
    plain = ops.follow_sequence(b, s, l, c, frames, fmt, (FH, FW), motion=None, **fo, **o)
    _same(plain, plain_want, "no motion", NAMES[:5] + ("moves",))
    assert plain[5][2, 0, 0, 3] in (LOST, MOVED) and box_of(plain[0], 2, 0) != shifted(FACE, 2 * STEP)


def test_two_dropouts_with_the_follower_between_updates():
    """Updates only on every second frame: the follower carries the box in between, so the velocity per update is what it left over."""
    frames, (b, s, l, c) = _moving_scene("bgr", F=6, dropout=(4,))
    lumas = [luma_of(pl, "bgr") for pl in frames]
    detect = [1, 0, 1, 0, 1, 0]
    o = dict(iou=0.2, max_age=3, min_hits=1, max_tracks=2, hold_grow=0.1)
    fo = dict(search=8, max_sad=3000)
    want = run_motion_follow(b, s, l, c, lumas, (FH, FW), dict(gain=1.0, damp=0.5), detect=detect, **fo, **o)
    got = ops.follow_sequence(b, s, l, c, frames, "bgr", (FH, FW), detect, motion=dict(gain=1.0, damp=0.5), **fo, **o)
    _same(got, want, "every second", NAMES[:5] + ("moves",))
    assert got[5][4, 0, 0, 3] != LEARNED and got[2][4, 0, 0].tolist() == [1, 2, 1]


# ---------------------------------------------------------------------------------------------- behind an engine
def test_an_engine_with_a_motion_tracker_gives_the_rows_of_the_op():
    """forward, decode, update on the normal route, frame after frame -- a source with faces, the same moved by two pixels, a blank
    frame, the source moved on --, against cf_op_track_ex on the rows the decodes kept."""
    from test_track import _blank_batch, _feed_until_faces
    rng = np.random.default_rng(3)
    eng = cfa.Engine(64, 96, max_batch=3, dtype="bf16")
    opts = dict(iou=0.3, max_age=3, min_hits=1, max_tracks=70, hold_grow=0.1)
    for motion, weak in ((True, {}), (dict(gain=1.0, damp=0.5), dict(weak_score=0.1, birth_score=0.3, weak_iou=0.5))):
        trk = cfa.Tracker(eng, 3, motion=motion, **weak, **opts)
        src, _ = _feed_until_faces(eng, rng)
        thr = 0.1 if weak else 0.3
        bases, gots = [], []
        for step in (0, 2, None, 4, None):
            if step is None:
                _blank_batch(eng)
            else:
                eng.forward_resized_enqueue(np.roll(src, step, axis=2))
            bases.append(eng.decode_threshold(thr, 0.3, 64))
            gots.append(eng.track_update(trk))
        F, rows = len(bases), 64
        b, s, l, c = np.zeros((F, 3, rows, 4), np.float32), np.zeros((F, 3, rows), np.float32), np.zeros((F, 3, rows, 10), np.float32), np.zeros((F, 3), np.int32)
        for f, base in enumerate(bases):
            for k, (d, lm) in enumerate(base):
                n = len(d)
                b[f, k, :n], s[f, k, :n], l[f, k, :n], c[f, k] = d[:, :4], d[:, 4], lm, n
        wk = dict(birth_score=0.3, weak_iou=0.5) if weak else {}
        od, ol, oi, oc, fl, vel = ops.track_sequence(b, s, l, c, motion=motion, vel=True, **wk, **opts)
        for f, (got, flags) in enumerate(gots):
            assert flags.tolist() == fl[f].tolist()
            for k, g in enumerate(got):
                n = int(oc[f, k])
                want = (od[f, k, :n], ol[f, k, :n], oi[f, k, :n, 0], oi[f, k, :n, 1], oi[f, k, :n, 2])
                for x, y in zip(g, want):
                    assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (f, k)
        assert oc[0].sum() >= 2 and (oi[2, :, :, 2] > 0).any()                 # faces, and held ones at the blank frame
        trk.close()
    eng.close()
