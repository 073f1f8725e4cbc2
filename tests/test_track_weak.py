"""The tracker with two thresholds on the GPU: cf_op_track_weak against the numpy restatement (tests/weak_cases.py) bit for bit on every
table, the scenarios of the statement one by one, the equality with the plain tracker where every row is strong -- and the property the
product paths rest on: the rows with score > 0.3 of a decode (a merge) at 0.1 are a prefix of it and equal the decode (the merge) at 0.3."""
import ctypes as C

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from oracle import centerface_oracle as O
from track_cases import random_sequence, run_sequence, tables
from weak_cases import A, A2, A3, FAR, STRONG, WEAK, at, crowd, mixed_random_sequence, pad_for, run_weak_sequence

pytestmark = pytest.mark.gpu

SLOTS = (1, 3, 64, 65, 130)               # lanes own one slot (some none), one and two, three: the 64-lane ballot boundaries
NAMES = ("dets", "lms", "info", "counts", "flags")


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
            raise AssertionError("%s: %s differs at %s: got %s, want %s" % (what, name, bad[:4].tolist(), g[tuple(bad[0][:2])][:3], w[tuple(bad[0][:2])][:3]))


def check_weak(boxes, scores, lms, counts, birth_score=0.3, weak_iou=0.5, **opts):
    """ops.track_sequence(birth_score=, weak_iou=) == the restatement on dets, lms, info, counts and flags, the bytes past the counts
    that the caller filled included.  Returns the restatement's tables."""
    F, S = counts.shape
    M = opts.get("max_tracks", 256)
    rng = np.random.default_rng(7)
    d0 = rng.standard_normal((F, S, M, 5)).astype(np.float32)
    l0 = rng.standard_normal((F, S, M, 10)).astype(np.float32)
    i0 = rng.integers(-9, 9, (F, S, M, 3)).astype(np.int32)
    want = run_weak_sequence(boxes, scores, lms, counts, d0, l0, i0, birth_score=birth_score, weak_iou=weak_iou, **opts)
    got = ops.track_sequence(boxes, scores, lms, counts, d0.copy(), l0.copy(), i0.copy(), birth_score=birth_score, weak_iou=weak_iou, **opts)
    _same(got, want, opts)
    return want


OPTS = dict(iou=0.3, max_age=3, min_hits=2, hold_grow=0.1)


def box_of(dets, f, k, s=0):
    return tuple(dets[f, s, k, :4].tolist())


# ---------------------------------------------------------------------------------------------- the scenarios of the statement
@pytest.mark.parametrize("M", SLOTS)
def test_a_weak_row_moves_the_track_where_the_plain_tracker_holds_a_stale_box(M):
    """strong, strong, weak with the box moved, strong: the third frame's row is the weak row's box, ungrown, hits advanced, misses 0,
    flag bit 1.  The plain tracker, the weak row dropped from its input, holds the box of the second frame, grown."""
    k = pad_for(M)
    frames = [[crowd(k) + [at(A, STRONG)]], [crowd(k) + [at(A, STRONG)]], [crowd(k) + [at(A2, WEAK)]], [crowd(k) + [at(A3, STRONG)]]]
    b, s, l, c = tables(frames, k + 1)
    d, lm, info, cnt, fl = check_weak(b, s, l, c, max_tracks=M, **OPTS)
    assert cnt[:, 0].tolist() == [k + 1] * 4 and fl[:, 0].tolist() == [0, 0, 2, 0]
    assert box_of(d, 2, k) == A2 and d[2, 0, k, 4] == np.float32(WEAK) and info[2, 0, k].tolist() == [k + 1, 3, 0]
    assert lm[2, 0, k].tobytes() == l[2, 0, k].tobytes()                      # the landmarks of THAT frame
    assert box_of(d, 3, k) == A3 and info[3, 0, k].tolist() == [k + 1, 4, 0]
    # the same sequence on a plain tracker without the weak row
    frames[2] = [crowd(k)]
    pb, ps, pl, pc = tables(frames, k + 1)
    plain = ops.track_sequence(pb, ps, pl, pc, max_tracks=M, **OPTS)
    _same(plain, run_sequence(pb, ps, pl, pc, max_tracks=M, **OPTS), "plain")
    assert plain[2][2, 0, k].tolist() == [k + 1, 2, 1] and not plain[4].any()
    assert box_of(plain[0], 2, k) != A2 and plain[0][2, 0, k, 0] < A[0]       # held where it was, grown by hold_grow
    assert plain[0][2, 0, k].tobytes() != d[2, 0, k].tobytes()


def test_three_streams_with_different_histories():
    """Stream 0 gets the weak row, stream 1 nothing in that frame (a held box), stream 2 the weak row without a track to match."""
    frames = [[[at(A, STRONG)], [at(A, STRONG)], []], [[at(A, STRONG)], [at(A, STRONG)], []],
              [[at(A2, WEAK)], [], [at(A2, WEAK)]], [[at(A3, STRONG)], [at(A3, STRONG)], [at(A3, STRONG)]]]
    b, s, l, c = tables(frames, 2, S=3)
    d, _, info, cnt, fl = check_weak(b, s, l, c, max_tracks=65, **OPTS)
    assert fl[2].tolist() == [2, 0, 0] and cnt[2].tolist() == [1, 1, 0]
    assert info[2, :2, 0].tolist() == [[1, 3, 0], [1, 2, 1]] and info[3, :, 0].tolist() == [[1, 4, 0], [1, 3, 0], [1, 1, 0]]


@pytest.mark.parametrize("M", (3, 65, 130))
def test_a_tentative_best_slot_is_passed_over_for_a_confirmed_second_best(M):
    """T was born in the frame before (one hit: tentative), C is confirmed.  The weak row lies on T (IoU 1) and overlaps C at 0.648: it
    matches C; T, unmatched and tentative, is freed."""
    k = min(M - 2, 68)
    frames = [[crowd(k) + [at(A, STRONG)]], [crowd(k) + [at(A, STRONG), at(A2, STRONG)]], [crowd(k) + [at(A2, WEAK)]]]
    b, s, l, c = tables(frames, k + 2)
    d, _, info, cnt, fl = check_weak(b, s, l, c, max_tracks=M, **OPTS)
    assert cnt[:, 0].tolist() == [k + 1, k + 2, k + 1] and fl[2, 0] == 2
    assert info[1, 0, k + 1].tolist() == [k + 2, 1, 0]                        # T
    assert info[2, 0, k].tolist() == [k + 1, 3, 0] and box_of(d, 2, k) == A2  # C took the row


@pytest.mark.parametrize("M", (3, 65, 130))
def test_a_strong_row_later_in_row_order_takes_the_weak_rows_best_slot(M):
    """Tracks P = A and Q = A3; the frame's rows are a weak row W, closest to P, and then a strong row on P.  The strong pass runs first
    and takes P; W goes to Q, which it still overlaps at weak_iou."""
    k = min(M - 2, 68)
    W = (1005, 1004, 1045, 1054)
    two = [at(A, STRONG), at(A3, STRONG)]
    frames = [[crowd(k) + two], [crowd(k) + two], [[at(W, WEAK)] + crowd(k) + [at(A, STRONG)]]]
    b, s, l, c = tables(frames, k + 2)
    d, _, info, cnt, fl = check_weak(b, s, l, c, max_tracks=M, **OPTS)
    assert fl[2, 0] == 2 and cnt[2, 0] == k + 2
    assert box_of(d, 2, k) == A and info[2, 0, k].tolist() == [k + 1, 3, 0]
    assert box_of(d, 2, k + 1) == W and info[2, 0, k + 1].tolist() == [k + 2, 3, 0]
    # without Q in reach the weak row is discarded: nothing is born, no flag
    frames = [[crowd(k) + [at(A, STRONG)]], [crowd(k) + [at(A, STRONG)]], [[at(W, WEAK)] + crowd(k) + [at(A, STRONG)]], [crowd(k) + [at(FAR, STRONG)]]]
    b, s, l, c = tables(frames, k + 2)
    d, _, info, cnt, fl = check_weak(b, s, l, c, max_tracks=M, **OPTS)
    assert fl[2, 0] == 0 and cnt[2, 0] == k + 1 and box_of(d, 2, k) == A
    assert info[3, 0, k + 1].tolist() == [k + 2, 1, 0]                        # next_id did not move for the discarded row


@pytest.mark.parametrize("M", (1, 64, 130))
def test_two_weak_rows_on_one_slot_the_first_wins(M):
    k = pad_for(M)
    frames = [[crowd(k) + [at(A, STRONG)]], [crowd(k) + [at(A, STRONG)]], [crowd(k) + [at(A2, WEAK), at(A, 0.25)]]]
    b, s, l, c = tables(frames, k + 2)
    d, _, info, cnt, fl = check_weak(b, s, l, c, max_tracks=M, **OPTS)
    assert cnt[2, 0] == k + 1 and fl[2, 0] == 2
    assert box_of(d, 2, k) == A2 and d[2, 0, k, 4] == np.float32(WEAK) and info[2, 0, k].tolist() == [k + 1, 3, 0]


@pytest.mark.parametrize("M", (3, 65, 130))
def test_a_weak_row_tying_between_two_slots_goes_to_the_lowest(M):
    """The two slots mirror each other about the row (IoU 0.6 from both sides, tests/test_track_abi.py): the lower slot takes it."""
    k = min(M - 2, 68)
    left, right, row = (2000, 1000, 2019, 1009), (2010, 1000, 2029, 1009), (2005, 1000, 2024, 1009)
    two = [at(left, STRONG), at(right, STRONG)]
    frames = [[crowd(k) + two], [crowd(k) + two], [crowd(k) + [at(row, WEAK)]]]
    b, s, l, c = tables(frames, k + 2)
    d, _, info, cnt, fl = check_weak(b, s, l, c, max_tracks=M, **OPTS)
    assert fl[2, 0] == 2 and box_of(d, 2, k) == row and info[2, 0, k:k + 2].tolist() == [[k + 1, 3, 0], [k + 2, 2, 1]]


@pytest.mark.parametrize("M", (1, 65))
def test_weak_rows_alone_on_an_empty_tracker_do_nothing(M):
    frames = [[[at(A, WEAK), at(FAR, 0.25)]], [[at(A, WEAK)]], [[at(A, STRONG)]]]
    b, s, l, c = tables(frames, 2)
    _, _, info, cnt, fl = check_weak(b, s, l, c, max_tracks=M, **OPTS)
    assert cnt[:, 0].tolist() == [0, 0, 1] and not fl.any() and info[2, 0, 0].tolist() == [1, 1, 0]      # next_id unmoved


@pytest.mark.parametrize("M", (3, 65))
def test_unmatched_weak_rows_on_a_full_tracker_leave_bit_0_clear(M):
    full = crowd(M)
    frames = [[full], [full], [full + [at(A, WEAK), at(FAR, WEAK)]], [full + [at(A, STRONG)]]]
    b, s, l, c = tables(frames, M + 2)
    _, _, _, cnt, fl = check_weak(b, s, l, c, max_tracks=M, **OPTS)
    assert cnt[:, 0].tolist() == [M] * 4 and fl[:, 0].tolist() == [0, 0, 0, 1]      # the same row, strong, is dropped and says so


@pytest.mark.parametrize("M", (1, 65, 130))
def test_a_held_track_is_recovered_ungrown_after_several_misses(M):
    k = pad_for(M)
    frames = [[crowd(k) + [at(A, STRONG)]], [crowd(k) + [at(A, STRONG)]], [crowd(k)], [crowd(k)], [crowd(k) + [at(A2, WEAK)]]]
    b, s, l, c = tables(frames, k + 1)
    d, _, info, _, fl = check_weak(b, s, l, c, max_tracks=M, **OPTS)
    assert info[3, 0, k].tolist() == [k + 1, 2, 2] and d[3, 0, k, 0] < A[0]    # held and grown (hold_grow = 0.1)
    assert info[4, 0, k].tolist() == [k + 1, 3, 0] and box_of(d, 4, k) == A2 and fl[4, 0] == 2


def test_weak_matches_alone_keep_a_track_alive_past_max_age():
    frames = [[[at(A, STRONG)]], [[at(A, STRONG)]]] + [[[at(A, WEAK)]]] * 4
    b, s, l, c = tables(frames, 1)
    o = dict(OPTS, max_age=1, max_tracks=3)
    _, _, info, cnt, fl = check_weak(b, s, l, c, **o)
    assert cnt[:, 0].tolist() == [1] * 6 and info[5, 0, 0].tolist() == [1, 6, 0] and fl[2:, 0].tolist() == [2] * 4
    frames[2:] = [[[]]] * 4
    pb, ps, pl, pc = tables(frames, 1)
    assert ops.track_sequence(pb, ps, pl, pc, **o)[3][:, 0].tolist() == [1, 1, 1, 0, 0, 0]      # the plain tracker loses it


def test_a_score_equal_to_birth_score_and_a_nan_score_are_weak():
    t = np.float32(0.3)
    above = float(np.nextafter(t, np.float32(1)))
    for score, born in ((float(t), False), (float("nan"), False), (above, True)):
        b, s, l, c = tables([[[at(A, score)]]], 1)
        _, _, _, cnt, fl = check_weak(b, s, l, c, max_tracks=3, **OPTS)
        assert cnt[0, 0] == int(born) and not fl.any(), score
    # ... and both match a confirmed track; the score goes into the slot as it is
    for score in (float(t), float("nan")):
        b, s, l, c = tables([[[at(A, STRONG)]], [[at(A, STRONG)]], [[at(A2, score)]]], 1)
        d, _, info, _, fl = check_weak(b, s, l, c, max_tracks=3, **OPTS)
        assert fl[2, 0] == 2 and info[2, 0, 0].tolist() == [1, 3, 0] and d[2, 0, 0, 4].tobytes() == np.float32(score).tobytes()


def test_a_weak_row_with_a_non_finite_corner_is_skipped():
    nan, inf = float("nan"), float("inf")
    for bad in ((nan, 1004, 1046, 1054), (1006, 1004, inf, 1054), (1006, -inf, 1046, 1054)):
        b, s, l, c = tables([[[at(A, STRONG)]], [[at(A, STRONG)]], [[at(bad, WEAK), at(A2, WEAK)]]], 2)
        d, _, info, _, fl = check_weak(b, s, l, c, max_tracks=3, **OPTS)
        assert fl[2, 0] == 2 and box_of(d, 2, 0) == A2 and info[2, 0, 0].tolist() == [1, 3, 0]
    b, s, l, c = tables([[[at(A, STRONG)]], [[at(A, STRONG)]], [[at((nan, 1004, 1046, 1054), WEAK)]]], 1)
    _, _, info, _, fl = check_weak(b, s, l, c, max_tracks=3, **OPTS)
    assert fl[2, 0] == 0 and info[2, 0, 0].tolist() == [1, 2, 1]


def test_min_hits_1_makes_every_track_eligible():
    b, s, l, c = tables([[[at(A, STRONG)]], [[at(A2, WEAK)]]], 1)
    d, _, info, _, fl = check_weak(b, s, l, c, max_tracks=3, **dict(OPTS, min_hits=1))
    assert fl[1, 0] == 2 and info[1, 0, 0].tolist() == [1, 2, 0] and box_of(d, 1, 0) == A2
    _, _, _, cnt, fl = check_weak(b, s, l, c, max_tracks=3, **OPTS)              # min_hits = 2: tentative, never matched, freed
    assert cnt[1, 0] == 0 and fl[1, 0] == 0


def test_weak_iou_is_a_threshold_of_its_own():
    """IoU(A, A2) = 0.648: a weak match at 0.5 and at 0.648's own float32, none at 0.7 -- although iou_thresh = 0.3 would take it."""
    b, s, l, c = tables([[[at(A, STRONG)]], [[at(A, STRONG)]], [[at(A2, WEAK)]]], 1)
    for weak_iou, hit in ((0.5, True), (0.7, False), (1.0, False)):
        _, _, info, _, fl = check_weak(b, s, l, c, weak_iou=weak_iou, max_tracks=3, **OPTS)
        assert fl[2, 0] == (2 if hit else 0) and info[2, 0, 0].tolist() == ([1, 3, 0] if hit else [1, 2, 1])


@pytest.mark.parametrize("M", (64, 65, 130))
def test_a_crowd_across_the_ballot_boundaries(M):
    """70 faces are confirmed, 60 others join them (slots 70 .. 129 where there are that many), then weak rows -- shifted half-way to
    the right neighbour, so that the two neighbours tie at IoU 189 / 693 -- meet held, live, tentative and matched slots in all three
    slots of a lane, in three streams with different histories; some frames have more faces than the table has rows."""
    from track_cases import grid_faces
    a, sh = grid_faces(70, size=20.0, gap=4.0), grid_faces(70, size=20.0, gap=4.0, dx=12.0)
    o = [(x1, y1 + 500, x2, y2 + 500) for x1, y1, x2, y2 in grid_faces(60, size=20.0, gap=4.0)]
    st, wk = lambda fs: [at(f, STRONG) for f in fs], lambda fs: [at(f, WEAK) for f in fs]      # noqa: E731
    frames = [[st(a), st(a[:30]), []],
              [st(a), st(a[:30]), st(o)],
              [st(o) + wk(sh[:10]), wk(sh[:30]) + st(o), st(o) + wk(a)],
              [wk(sh[5:40]) + st(o[::2]), st(a[::2]) + wk(o), wk(o) + st(a[:10])],
              [wk(a[::3]) + st(sh[1::3]) + wk(o[1::2]), wk(a), st(a)],
              [st(a[:35]) + wk(o[:35]), [], wk(sh)]]
    b, s, l, c = tables(frames, 70, S=3)
    _, _, _, cnt, fl = check_weak(b, s, l, c, weak_iou=0.25, iou=0.2, max_age=2, min_hits=2, max_tracks=M, hold_grow=0.05)
    assert cnt[1, 0] == min(M, 70) and (fl & 2).any()


# ---------------------------------------------------------------------------------------------- the two equalities
def test_with_every_score_above_birth_score_the_tables_are_the_plain_trackers():
    b, s, l, c = random_sequence(3, S=2, F=8, max_faces=60, rows=70)
    assert float(s[s > 0].min()) > 0.3 and c.max() > 40
    o = dict(iou=0.3, max_age=2, min_hits=2, max_tracks=65, hold_grow=0.1)
    plain = ops.track_sequence(b, s, l, c, **o)
    _same(ops.track_sequence(b, s, l, c, birth_score=0.3, weak_iou=0.5, **o), plain, "all strong")
    _same(plain, run_sequence(b, s, l, c, **o), "plain")
    assert plain[3].max() == 65 and plain[4].any()                             # the tracker was full, rows were dropped
    # a scenario's tables too: the weak pass has no row to look at
    frames = [[[at(A, STRONG), at(FAR, 0.31)]], [[at(A2, 0.5)]], [[]], [[at(A3, 0.9), at(FAR, 0.4)]]]
    b, s, l, c = tables(frames, 3)
    for M in SLOTS:
        _same(ops.track_sequence(b, s, l, c, birth_score=0.3, weak_iou=0.5, max_tracks=M, **OPTS), ops.track_sequence(b, s, l, c, max_tracks=M, **OPTS), M)


@pytest.mark.parametrize("seed", (0, 1))
def test_random_sequences_with_scores_on_both_sides(seed):
    b, s, l, c = mixed_random_sequence(seed)
    assert b.shape[:3] == (8, 2, 70) and np.isnan(s).any() and (s == np.float32(0.3)).any()
    _, _, _, _, fl = check_weak(b, s, l, c, iou=0.3, max_age=2, min_hits=2, max_tracks=65, hold_grow=0.1)
    assert (fl & 2).any()
    check_weak(b, s, l, c, birth_score=0.6, weak_iou=0.3, iou=0.5, max_age=1, min_hits=1, max_tracks=33)


# ---------------------------------------------------------------------------------------------- the prefix property
MAP_HW, MAX_OUT = (24, 24), 96


def cluster_map():
    """A 24 x 24 head map with 12 clusters of 4 neighbouring candidate cells: boxes of 12 to 16 px on a 4 px lattice, so the cells of a
    cluster suppress one another; scores from 0.11 to 0.95 on both sides of 0.3, the background below 0.1."""
    rng = np.random.default_rng(42)
    h, w = MAP_HW
    hm = rng.uniform(0.01, 0.09, (1, 1, h, w)).astype(np.float32)
    centres = [(2 + 6 * (i // 4) + int(rng.integers(0, 2)), 2 + 6 * (i % 4) + int(rng.integers(0, 2))) for i in range(12)]
    weak, strong = np.linspace(0.11, 0.29, 30).astype(np.float32), np.linspace(0.31, 0.95, 30).astype(np.float32)
    for i, (y, x) in enumerate(centres):                                       # four clusters all weak, four mixed, four all strong
        values = rng.choice(weak if i < 4 else strong if i >= 8 else np.concatenate([weak, strong]), 5, replace=False)
        for v, (dy, dx) in zip(values, ((0, 0), (0, 1), (1, 0), (1, 1), (3, 0))):      # a 2 x 2 block and a cell 12 px below it
            hm[0, 0, y + dy, x + dx] = v
    wh = rng.uniform(3.0, 4.0, (1, 2, h, w)).astype(np.float32)
    reg = rng.uniform(0, 1, (1, 2, h, w)).astype(np.float32)
    lm = rng.normal(0, 1, (1, 10, h, w)).astype(np.float32)
    return hm, wh, reg, lm, (4 * h, 4 * w)


def _decode(mode, m, thr):
    hm, wh, reg, lm, (ih, iw) = m
    h, w = MAP_HW
    dets, lms, cnt = np.zeros((1, MAX_OUT, 5), np.float32), np.zeros((1, MAX_OUT, 10), np.float32), np.full(1, -1, np.int32)
    P = cfa._lib.ptr
    rc = cfa._lib.lib().cf_op_decode_threshold_ex(0, mode, P(hm), P(wh), P(reg), P(lm), 1, h, w, ih, iw, C.c_float(thr), C.c_float(0.3), MAX_OUT,
                                                  P(dets), P(lms), P(cnt))
    assert rc == 0, cfa._lib.lib().cf_op_last_error()
    return dets[0], lms[0], int(cnt[0])


@pytest.mark.parametrize("mode", (0, 1))
def test_the_strong_rows_of_a_decode_at_the_weak_threshold_are_the_decode_at_birth_score(mode):
    m = cluster_map()
    hm, wh, reg, lm, size = m
    assert 30 <= int((hm > np.float32(0.1)).sum()) <= 60 and 8 <= int((hm > np.float32(0.3)).sum())
    for thr in (0.1, 0.3):                                                     # neither decode reaches max_out: the plain statement, on the CPU
        if mode == 0:
            kept = len(O.decode_d1(hm, wh, reg, lm, size, nms_thresh=0.3, fixed_threshold=np.float32(thr))[0])
        else:
            kept = len(O.decode_d2(hm[0], wh[0], reg[0], size, threshold=np.float32(thr), nms_thresh=0.3))
        assert 0 < kept < MAX_OUT, (thr, kept)
    d1, l1, n1 = _decode(mode, m, 0.1)
    d3, l3, n3 = _decode(mode, m, 0.3)
    assert 0 < n3 < n1 < MAX_OUT
    strong = d1[:n1, 4] > np.float32(0.3)
    assert strong[:n3].all() and not strong[n3:].any()                         # a prefix
    assert d1[:n3].tobytes() == d3[:n3].tobytes() and l1[:n3].tobytes() == l3[:n3].tobytes()
    assert (d1[n3:n1, 4] > np.float32(0.1)).all()


def two_tile_table():
    """Two tiles that share a band of the frame, per tile a decode's rows in descending score order: clusters of near-duplicates within a
    tile and across the two.  (rects, frame_hw, net_hw, boxes, scores, lms, the number of rows above 0.3 per tile)."""
    rng = np.random.default_rng(9)
    rects, frame_hw, net_hw, rows = [(0, 0, 64, 48), (38, 28, 64, 48)], (76, 102), (48, 64), 40
    boxes, scores, lms = np.zeros((1, 2, rows, 4), np.float32), np.zeros((1, 2, rows), np.float32), np.zeros((1, 2, rows, 10), np.float32)
    centres = rng.uniform((44, 32), (60, 44), (10, 2))                         # frame pixels, in the band both tiles see
    for t, (x0, y0, _, _) in enumerate(rects):
        own = rng.uniform((8, 8), (56, 40), (10, 2)) + (x0, y0)
        c = np.concatenate([centres + rng.normal(0, 0.6, centres.shape), own, own + rng.normal(0, 1.0, own.shape), centres + rng.normal(0, 1.5, centres.shape)])
        half = rng.uniform(3, 5, (rows, 1))
        fb = np.concatenate([c - half, c + half], 1) - (x0, y0, x0, y0)          # the tile's own coordinates (scale 1)
        boxes[0, t] = np.clip(fb, (3, 3, 3, 3), (60, 44, 60, 44))              # clear of the interior sides by more than `edge`
        cluster = np.concatenate([np.arange(10), np.arange(10), np.arange(10), np.arange(10)])
        sc = np.where(cluster < 3, rng.uniform(0.11, 0.29, rows), rng.uniform(0.11, 0.95, rows)).astype(np.float32)      # three in ten: all weak
        order = np.argsort(-sc, kind="stable")
        boxes[0, t], scores[0, t] = boxes[0, t][order], sc[order]
        lms[0, t] = rng.normal(30, 10, (rows, 10))
    n_strong = (scores > np.float32(0.3)).sum(axis=2).astype(np.int32)         # per tile: the strong rows are its first rows
    assert (n_strong > 5).all() and (n_strong < rows - 5).all()
    return rects, frame_hw, net_hw, boxes, scores, lms, n_strong


def test_the_strong_rows_of_a_merge_of_weak_decodes_are_the_merge_of_the_strong_decodes():
    """The merge of the rows above 0.1 of both tiles begins with, bit for bit, the merge of their rows above 0.3: cf_merge_tiles removes
    duplicates greedily in descending score order, so the product paths may run tiled with a weak tracker."""
    rects, frame_hw, net_hw, boxes, scores, lms, n_strong = two_tile_table()
    rows = boxes.shape[2]
    full = np.full((1, 2), rows, np.int32)
    for metric, thresh in (("ios", 0.5), ("iou", 0.3)):
        d1, l1, c1, f1 = ops.merge_tiles(rects, frame_hw, net_hw, boxes, scores, lms, full, 2 * rows, metric=metric, thresh=thresh)
        d3, l3, c3, f3 = ops.merge_tiles(rects, frame_hw, net_hw, boxes, scores, lms, n_strong, 2 * rows, metric=metric, thresh=thresh)
        n1, n3 = int(c1[0]), int(c3[0])
        assert 0 < n3 < n1 < 2 * rows and n1 < int(full.sum()) and n3 < int(n_strong.sum()) and not f1.any() and not f3.any()      # duplicates went
        strong = d1[0, :n1, 4] > np.float32(0.3)
        assert strong[:n3].all() and not strong[n3:].any()
        assert d1[0, :n3].tobytes() == d3[0, :n3].tobytes() and l1[0, :n3].tobytes() == l3[0, :n3].tobytes()
