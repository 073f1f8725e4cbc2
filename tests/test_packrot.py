"""Rotated sources through packed views on the GPU: the rotated packed cutter (cf_op_packed_rot, cf_forward_packed_rot), the merge into
the STORED frame (cf_op_merge_packed_rot, cf_merge_packed behind a rotated packed forward), the state rules, the consumers and the
product paths behind them, every byte and bit against the restatements of tests/packrot_cases.py (np.rot90 of the stored frame's BGR,
then the packed canvases; the statement's row formulas in float64, the corner assignment per rot, the restated NMS)."""
import ctypes as C

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from packrot_cases import ROTS, merge_packed_rot_ref, packed_rot_canvases_ref, upright_hw
from pack_cases import unpacked_places
from rot_cases import upright
from test_redact import redact_ref, source_frames
from test_tiles import FILL, bgr_of, pitched_frames, same_results

pytestmark = pytest.mark.gpu

FORMATS = ("bgr", "nv12", "nv21", "i420", "yv12")
NET = (64, 96)                  # (H, W) of every context here
RAGGED = (70, 100)              # canvases of the ops form: tiles are cut in both directions (128 x 32 and 32 x 64 tiles)
STORED = ((40, 120), (120, 40), (72, 96))
FILL_BGR = (1, 2, 3)
CF_ESTATE = cfa._lib.CF_ESTATE
L = cfa._lib


def _diff(got, want, *what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and len(bad) == 0, what + (got.shape, want.shape, len(bad), bad[:4].tolist())


def dense_frames(rng, fmt, B, hw):
    h, w = hw
    return rng.integers(0, 256, (B, h, w, 3) if fmt == "bgr" else (B, h * 3 // 2, w), dtype=np.uint8)


# ------------------------------------------------------------------------------------------ the cutter
def hand_table(hu, wu):
    """A hand-made table for Bf = 2 in two (70, 100) canvases; sources in pixels of the upright view (hu, wu >= 40).  The comments say
    what each placement is there for (seams of the quarter-turn tiles: x = 32, 64, 96, y = 64; of the half-turn tiles: y = 32, 64)."""
    whole = (0, 0, wu, hu)
    p = [(0, 0) + whole + (1, 3, 33, 29),                      # odd dx, dy, dw, dh; crosses the seam x = 32
         (1, 0, wu - 30, hu - 22, 30, 22, 34, 3, 31, 29),      # shares the edge x = 34 with it; a source ending at the far corner, enlarged; crosses x = 64
         (1, 0, 0, 0, 20, 4, 1, 32, 20, 4),                    # shares the edge y = 32 with the first; identity
         (0, 0) + whole + (99, 69, 1, 1),                      # a 1 x 1 content in the last column and row
         (1, 0, 4, 6, 20, 16, 60, 40, 39, 30),                 # an enlarging view that crosses the seams x = 64, x = 96 and y = 64
         (0, 0, 10, 8, 24, 16, 2, 40, 24, 16),                 # a source of exactly the content's size
         (1, 0) + whole + (30, 36, 25, 21),                    # a reducing view
         (0, 1) + whole + (0, 0, 100, 31)]                     # canvas 1: the top rows only -- every tile below y = 32 is touched by nobody
    return [tuple(int(v) for v in x) for x in p], 2


@pytest.mark.parametrize("fmt", FORMATS)
def test_op_packed_rot_hand_made_table(fmt):
    """The table over the three stored sizes and the three turns, rows with padding that holds 0xFF (and 0x00): every byte of the
    canvases is the restatement's; the identity view is the np.rot90 crop."""
    rng = np.random.default_rng(40 + FORMATS.index(fmt))
    for hw in STORED:
        dense = dense_frames(rng, fmt, 2, hw)
        bgr = bgr_of(dense, fmt)
        for rot in ROTS:
            hu, wu = upright_hw(hw, rot)
            places, N = hand_table(hu, wu)
            want = packed_rot_canvases_ref(bgr, rot, places, N, RAGGED, FILL_BGR)
            for pad in (0xFF, 0x00) if hw == STORED[0] else (0xFF,):
                frames, _, _, _ = pitched_frames(dense, fmt, pad)
                _diff(ops.cut_packed(frames, places, N, RAGGED, fmt, fill=FILL_BGR, rot=rot), want, fmt, hw, rot, pad)
            # what the restatement says of the table
            assert np.array_equal(want[0, 40:56, 2:26], upright(bgr[0], rot)[8:24, 10:34]) and np.array_equal(want[0, 32:36, 1:21], upright(bgr[1], rot)[0:4, 0:20])
            assert (want[1, 31:] == FILL_BGR).all() and (want[0, 64:, :32] == FILL_BGR).all() and (want[0, :3] == FILL_BGR).all()
            if rot == 90:                                # another fill reaches every fill byte and no content byte
                _diff(ops.cut_packed(dense, places, N, RAGGED, fmt, rot=rot), packed_rot_canvases_ref(bgr, rot, places, N, RAGGED), fmt, hw, "black")


def _raw_cut_rot(dense, places, N, size, fmt, rot, fill=FILL_BGR):
    """cf_op_packed_rot itself, whatever rot is (ops.cut_packed sends rot = 0 to cf_op_packed)."""
    tab, B, h, w, pitch0, pitch1, keep = L.frame_planes(dense, fmt, writable=False)
    pt, P = L.place_table(places)
    out = np.empty((N, size[0], size[1], 3), np.uint8)
    L.check(L.lib().cf_op_packed_rot(0, rot, L.frame_format(fmt), tab, B, h, w, pitch0, pitch1, pt, P, N, L.fill_bytes(fill), size[0], size[1], L.ptr(out)), op=True)
    return out


@pytest.mark.parametrize("fmt", ("bgr", "nv12"))
def test_op_packed_rot_0_is_the_packed_cutter(fmt):
    hw = (72, 96)
    dense = dense_frames(np.random.default_rng(7), fmt, 2, hw)
    places, N = hand_table(*hw)
    want = ops.cut_packed(dense, places, N, RAGGED, fmt, fill=FILL_BGR)
    assert ops.cut_packed(dense, places, N, RAGGED, fmt, fill=FILL_BGR, rot=0).tobytes() == want.tobytes()
    assert _raw_cut_rot(dense, places, N, RAGGED, fmt, 0).tobytes() == want.tobytes()


@pytest.mark.parametrize("rot", ROTS)
def test_op_packed_rot_more_placements_than_one_list_round(rot):
    """One (16, 32) canvas -- one tile of either kernel -- tiled by 300 contents of 1 x 1 (a list round holds 256) from two frames, and
    a second canvas with 212 more: NV12 and BGR."""
    hw = (40, 120)
    hu, wu = upright_hw(hw, rot)
    places = []
    for k in range(512):
        src = (2 * (k % (wu // 2 - 1)), 2 * (k % (hu // 2 - 1)), 2, 2) if k % 5 else (2 * (k % 11), 2 * (k % 13), 6, 4)
        places.append(((k // 3) & 1, 0 if k < 300 else 1) + src + (k % 32, k // 32, 1, 1))
    for fmt in ("nv12", "bgr"):
        dense = dense_frames(np.random.default_rng(50 + rot), fmt, 2, hw)
        want = packed_rot_canvases_ref(bgr_of(dense, fmt), rot, places, 2, (16, 32), FILL_BGR)
        frames, _, _, _ = pitched_frames(dense, fmt, 0xFF)
        _diff(ops.cut_packed(frames, places, 2, (16, 32), fmt, fill=FILL_BGR, rot=rot), want, fmt, rot)
        assert (want[0].reshape(-1, 3)[300:] == FILL_BGR).all() and (want[1].reshape(-1, 3)[:300] == FILL_BGR).all()


@pytest.mark.parametrize("rot", ROTS)
def test_op_packed_rot_frames_0_and_64_on_one_canvas(rot):
    """Bf = 65 frames of 8 x 12 into 33 canvases of (4, 8): canvas n holds frame n on the left and frame 64 - n on the right, so frame 0
    and frame 64 share canvas 0 (YV12: the planes swapped; BGR)."""
    hw = (8, 12)
    hu, wu = upright_hw(hw, rot)
    places = []
    for n in range(33):
        places += [(n, n, 0, 2, wu, 4, 0, 0, 4, 4), (64 - n, n, 2, 0, 6, hu, 4, 1, 4, 3)]
    for fmt in ("yv12", "bgr"):
        dense = dense_frames(np.random.default_rng(90 + rot), fmt, 65, hw)
        want = packed_rot_canvases_ref(bgr_of(dense, fmt), rot, places, 33, (4, 8), FILL_BGR)
        frames, _, _, _ = pitched_frames(dense, fmt, 0xFF)
        _diff(ops.cut_packed(frames, places, 33, (4, 8), fmt, fill=FILL_BGR, rot=rot), want, fmt, rot)


@pytest.mark.parametrize("fmt", ("bgr", "nv21", "i420"))
def test_op_packed_rot_one_whole_frame_placement_is_the_rotated_fit(fmt):
    """A single placement per frame with the rectangle of ops.rot_geometry equals ops.rot_frames byte for byte: fitted and stretched,
    every rot, the three stored sizes."""
    rng = np.random.default_rng(60 + FORMATS.index(fmt))
    for hw in STORED:
        dense = dense_frames(rng, fmt, 2, hw)
        for rot in ROTS:
            hu, wu = upright_hw(hw, rot)
            for fit in (None, dict(fill=FILL_BGR)):
                rw, rh, dx, dy = ops.rot_geometry(hw[0], hw[1], RAGGED[0], RAGGED[1], rot, fit)
                places = [(f, f, 0, 0, wu, hu, dx, dy, rw, rh) for f in range(2)]
                got = ops.cut_packed(dense, places, 2, RAGGED, fmt, fill=FILL_BGR, rot=rot)
                _diff(got, ops.rot_frames(dense, RAGGED, fmt, rot, fit), fmt, hw, rot, fit)


# ------------------------------------------------------------------------------------------ the merge on hand-built tables
def check_merge(places, Bf, frame_hw, net_hw, rot, d, s, l, counts, max_out, **opt):
    """ops.merge_packed(rot=) against merge_packed_rot_ref, bit for bit: counts, flags, the rows below min(count, max_out), and the
    caller's bytes in every row behind them."""
    d, s, l = (np.asarray(a, np.float32) for a in (d, s, l))
    od, ol = np.full((Bf, max_out, 5), FILL), np.full((Bf, max_out, 10), FILL)
    gd, gl, gc, gf = ops.merge_packed(places, Bf, frame_hw, net_hw, d, s, l, counts, max_out, dets=od, lms=ol, rot=rot, **opt)
    want, wflags = merge_packed_rot_ref(places, Bf, frame_hw, rot, d, s, l, counts, **opt)
    assert gc.tolist() == [len(w[0]) for w in want], (rot, gc, [len(w[0]) for w in want])
    assert gf.tolist() == wflags.tolist()
    for f, (wd, wl) in enumerate(want):
        m = min(len(wd), max_out)
        assert gd[f, :m].tobytes() == wd[:m].tobytes(), (rot, f, gd[f, :m], wd[:m])
        assert gl[f, :m].tobytes() == wl[:m].tobytes(), (rot, f)
        assert (gd[f, m:] == FILL).all() and (gl[f, m:] == FILL).all(), (rot, f)
    return want, gc, gf


def canvas_table(N, rows, entries):
    """dets_net / scores / lms_net / counts [N ...] from {canvas: [(x1, y1, x2, y2, score), ...]}; landmark k of row i is 3 + i + 4 (k % 8)."""
    d, s, l = np.zeros((N, rows, 4), np.float32), np.zeros((N, rows), np.float32), np.zeros((N, rows, 10), np.float32)
    c = np.zeros((N,), np.int32)
    for n, rws in entries.items():
        c[n] = len(rws)
        for i, r in enumerate(rws):
            d[n, i], s[n, i] = r[:4], r[4]
            l[n, i] = (np.arange(10) % 8) * 4 + 3 + i
    return d, s, l, c


FRAME = (40, 120)               # the stored frame of the merge tables: not square, so (h, w) and (hu, wu) differ at a quarter turn


def shared(hu, wu):
    """One 64 x 64 canvas: frame 0 at x in [0, 32), y in [0, 22); frame 1 beside it (shared edge x = 32) and below it (y = 22)."""
    return [(0, 0, 0, 0, wu, hu, 0, 0, 32, 22), (1, 0, 0, 0, wu, hu, 32, 0, 32, 22), (1, 0, 0, 0, wu, hu, 0, 22, 32, 22)]


@pytest.mark.parametrize("rot", ROTS)
def test_merge_packed_rot_rows_in_the_neighbour_in_the_fill_and_on_a_shared_edge(rot):
    net = (64, 64)
    hu, wu = upright_hw(FRAME, rot)
    places = shared(hu, wu)
    rows = [(4, 4, 12, 12, 0.9),          # in frame 0's content
            (40, 5, 50, 15, 0.8),         # in the neighbour's content: frame 1's, mapped by ITS view
            (40, 30, 50, 40, 0.95),       # in the fill: nobody's
            (28, 5, 36, 15, 0.7),         # cx = 32 exactly: the half-open rule gives it to the content that starts there (frame 1)
            (5, 18, 15, 26, 0.6),         # cy = 22 exactly: the content below (frame 1)
            (40, 50, 50, 60, 0.99)]       # far down in the fill
    d, s, l, c = canvas_table(1, 8, {0: rows})
    want, gc, gf = check_merge(places, 2, FRAME, net, rot, d, s, l, c, 8)
    assert gc.tolist() == [1, 3] and gf.tolist() == [0, 0]
    # the first row by hand: ux = x * (wu / 32), uy = y * (hu / 22), then the table and the corner assignment of the statement
    h, w = FRAME
    ux, uy = (lambda x: np.float64(x) * (np.float64(wu) / 32)), (lambda y: np.float64(y) * (np.float64(hu) / 22))
    by_hand = {90: (uy(4), (h - 1) - ux(12), uy(12), (h - 1) - ux(4)), 180: ((w - 1) - ux(12), (h - 1) - uy(12), (w - 1) - ux(4), (h - 1) - uy(4)),
               270: ((w - 1) - uy(12), ux(4), (w - 1) - uy(4), ux(12))}[rot]
    assert want[0][0][0, :4].tolist() == [np.float32(v) for v in by_hand]
    assert (want[0][0][0, 2] >= want[0][0][0, 0]) and (want[0][0][0, 3] >= want[0][0][0, 1])      # an upright box stays one
    # one float32 step of the centre to the left, a quarter pixel up, and the rows are frame 0's
    d2 = d.copy()
    d2[0, 3, 2] = np.nextafter(np.float32(36), np.float32(0))
    d2[0, 4, 1] = 17.75
    assert check_merge(places, 2, FRAME, net, rot, d2, s, l, c, 8)[1].tolist() == [3, 1]
    # a frame without any placement has no rows
    assert check_merge(places[:1], 2, FRAME, net, rot, d, s, l, c, 8)[1].tolist() == [1, 0]


@pytest.mark.parametrize("rot", ROTS)
def test_merge_packed_rot_the_edge_rule_tests_against_the_upright_view(rot):
    """Rows within `edge` of a content side.  A source that ends at the upright view's right or bottom border has no interior side
    there, whatever the stored (h, w) say; one that ends where the STORED frame would end, but inside the upright view, has."""
    net = (64, 64)
    h, w = FRAME
    hu, wu = upright_hw(FRAME, rot)
    lo, hi = min(hu, wu), max(hu, wu)                   # 40, 120
    # canvas 0: the source ends at the upright view's far corner (x = wu, y = hu); canvas 1: it ends at (lo, lo) -- for the longer side
    # of the upright view that is interior, though it is where the shorter STORED side ends
    places = [(0, 0, wu - 20, hu - 20, 20, 20, 8, 8, 40, 40), (0, 1, lo - 20, lo - 20, 20, 20, 8, 8, 40, 40)]
    rows = [(20, 20, 47.5, 30, 0.9),      # within 2 of the content's right side (x = 48)
            (20, 32, 30, 47.5, 0.8),      # within 2 of its bottom side (y = 48)
            (9, 20, 19, 30, 0.7),         # within 2 of its left side: the source's left side is interior everywhere here
            (20, 9, 30, 19, 0.6),         # within 2 of its top side: likewise
            (32, 32, 40, 40, 0.5)]        # clear of every side (and of every other row: the NMS has nothing to do, thresh 1.0 besides)
    d, s, l, c = canvas_table(2, 8, {0: rows, 1: rows})
    want, gc, gf = check_merge(places[:1], 1, FRAME, net, rot, d, s, l, c, 8, edge=2.0, thresh=1.0)
    assert sorted(float(v) for v in want[0][0][:, 4]) == [float(np.float32(v)) for v in (0.5, 0.8, 0.9)]      # right and bottom are the view's border
    want, gc, gf = check_merge([(0, 0) + places[1][2:]], 1, FRAME, net, rot, d, s, l, c, 8, edge=2.0, thresh=1.0)
    kept = sorted(float(v) for v in want[0][0][:, 4])
    if rot == 180:                                       # upright (40, 120): y = 40 is its bottom border, x = 40 is interior
        assert kept == [float(np.float32(v)) for v in (0.5, 0.8)]
    else:                                                # upright (120, 40): x = 40 is its right border, y = 40 is interior
        assert kept == [float(np.float32(v)) for v in (0.5, 0.9)]
    assert (hu, wu) == ((h, w) if rot == 180 else (w, h)) and lo == 40 and hi == 120
    # edge 0: all five
    assert check_merge(places, 1, FRAME, net, rot, d, s, l, c, 8, edge=0.0, thresh=1.0)[1].tolist() == [10]


@pytest.mark.parametrize("rot", ROTS)
def test_merge_packed_rot_non_finite_inverted_and_signed_zero(rot):
    """A non-finite corner is dropped; an inverted box and a -0.0 coordinate come back as the statement's ASSIGNMENT of mapped corners
    gives them (a min / max would order the first and could pick either zero)."""
    net = (64, 64)
    hu, wu = upright_hw(FRAME, rot)
    places = [(0, 0, 0, 0, wu, hu, 0, 0, 32, 22)]
    rows = [(4, 4, np.inf, 12, 0.9), (np.nan, 4, 12, 12, 0.85), (20, 15, 10, 5, 0.8),        # non-finite twice; inverted in x and y
            (-0.0, -0.0, 8, 6, 0.7), (24, 2, 30, 8, 0.6)]
    d, s, l, c = canvas_table(1, 8, {0: rows})
    l[0, 3, :2] = -0.0
    want, gc, gf = check_merge(places, 1, FRAME, net, rot, d, s, l, c, 8, thresh=1.0)
    assert gc.tolist() == [3]
    inv = want[0][0][0]
    assert float(inv[4]) == float(np.float32(0.8))
    assert (inv[2] < inv[0]) and (inv[3] < inv[1])       # the inverted box stays inverted in both directions: corners are assigned
    zero = want[0][0][1]
    # ux(-0.0) = -0.0 * sx + 0.0 = +0.0: the coordinate that is ux or uy itself comes back as +0.0, bit for bit
    at = {90: 0, 180: None, 270: 1}[rot]                 # rot 90: X1 = uy(y1); rot 270: Y1 = ux(x1); rot 180: both are differences
    if at is not None:
        assert zero[at].tobytes() == np.float32(0.0).tobytes()


@pytest.mark.parametrize("rot", ROTS)
def test_merge_packed_rot_ties_more_than_1024_items_and_a_truncated_canvas(rot):
    """Bf = 3 frames with five placements each in the 16 quarter slots of four 64 x 64 canvases, 256 rows per canvas: 1280 (placement,
    row) items a frame, so the collect's 1024-wide round runs twice; whole-view and interior sources (the edge rule); scores from 40
    values (ties); an empty, a truncated canvas (it flags every frame on it), a NaN."""
    rng = np.random.default_rng(12)
    net, rows = (64, 64), 256
    c0 = rng.uniform(-2, 66, (4, rows, 2))
    half = rng.uniform(0.5, 7, (4, rows, 2))
    d = np.concatenate([c0 - half, c0 + half], -1).astype(np.float32)
    s = rng.choice(np.linspace(0.3, 0.95, 40).astype(np.float32), (4, rows))
    l = rng.uniform(-4, 68, (4, rows, 10)).astype(np.float32)
    d[1, 5, 2] = np.nan
    slots = [(n, x, y, 32, 32 if y == 0 or x == 0 else 20) for n in range(4) for y in (0, 32) for x in (0, 32)]
    hu, wu = upright_hw(FRAME, rot)
    places = []
    for i, (n, x, y, dw, dh) in enumerate(slots[:15]):
        src = (0, 0, wu, hu) if i % 2 else (8, 8, 24, 24)
        places.append((i % 3, n) + src + (x, y, dw, dh))
    counts = np.array([rows, rows + 9, rows - 7, rows], np.int32)
    want, gc, gf = check_merge(places, 3, FRAME, net, rot, d, s, l, counts, 5 * rows)
    assert gf.tolist() == [1, 1, 1] and gc.min() > 8, (gc, gf)
    counts[:] = [rows, rows, 0, 31]
    want, gc, gf = check_merge(places, 3, FRAME, net, rot, d, s, l, counts, 7, metric="iou", thresh=0.3, edge=0.0)      # truncated outputs
    assert gf.tolist() == [0, 0, 0]
    counts[:] = [rows, rows, 3, rows + 1]                                      # canvas 3 holds placements 12, 13, 14: frames 0, 1, 2
    assert check_merge(places, 3, FRAME, net, rot, d, s, l, counts, 5 * rows)[2].tolist() == [1, 1, 1]
    counts[:] = [2, 2, rows + 1, 2]                                            # canvas 2 holds placements 8 .. 11, of which 8 stays: frame 2
    assert check_merge(places[:9] + places[12:], 3, FRAME, net, rot, d, s, l, counts, 5 * rows)[2].tolist() == [0, 0, 1]


def test_merge_packed_rot_0_is_the_packed_merge():
    rng = np.random.default_rng(3)
    net, rows = (64, 64), 64
    places = shared(FRAME[0], FRAME[1]) + [(0, 1, 8, 8, 24, 24, 3, 5, 40, 30)]
    c0 = rng.uniform(-2, 66, (2, rows, 2))
    half = rng.uniform(0.5, 7, (2, rows, 2))
    d = np.concatenate([c0 - half, c0 + half], -1).astype(np.float32)
    s = rng.uniform(0.3, 0.95, (2, rows)).astype(np.float32)
    l = rng.uniform(-4, 68, (2, rows, 10)).astype(np.float32)
    c = np.array([rows, rows - 3], np.int32)
    want = ops.merge_packed(places, 2, FRAME, net, d, s, l, c, 128)
    assert want[2].min() >= 4
    got = ops.merge_packed(places, 2, FRAME, net, d, s, l, c, 128, rot=0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    # cf_op_merge_packed_rot itself at rot 0 (ops.merge_packed sends rot = 0 to cf_op_merge_packed)
    pt, P = L.place_table(places)
    od, ol, oc, fl = np.zeros((2, 128, 5), np.float32), np.zeros((2, 128, 10), np.float32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    o = L.merge_opts("ios", 0.5, 2.0)
    L.check(L.lib().cf_op_merge_packed_rot(0, 0, C.byref(o), pt, P, 2, 2, FRAME[0], FRAME[1], net[0], net[1], L.ptr(d), L.ptr(s), L.ptr(l), L.ptr(c), rows, 128,
                                           L.ptr(od), L.ptr(ol), L.ptr(oc), L.ptr(fl)), op=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((od, ol, oc, fl), want))


@pytest.mark.parametrize("rot", ROTS)
def test_merge_packed_rot_one_whole_frame_placement_equals_unrot_rows_by_value(rot):
    """Non-overlapping boxes with descending scores, so the NMS keeps all of them in the decode's order: np.array_equal to
    ops.unrot_rows (by value: the `+ sx0` turns a -0.0 into +0.0), fitted and stretched."""
    for frame in STORED:
        hu, wu = upright_hw(frame, rot)
        for fit in (None, True):
            rw, rh, dx, dy = ops.rot_geometry(frame[0], frame[1], NET[0], NET[1], rot, fit)
            assert rw >= 10 and rh >= 12
            boxes = [(dx + 1 + 5 * (k % 2), dy + 1 + 4 * (k // 2), dx + 4 + 5 * (k % 2), dy + 3 + 4 * (k // 2)) for k in range(6)]      # a 2 x 3 grid, disjoint
            d = np.zeros((2, 8, 4), np.float32)
            d[:, :6] = boxes
            d[1, 0, :2] = (-0.0 if dx == 0 else dx, -0.0 if dy == 0 else dy)      # (stretched: ux(-0.0) is -0.0 behind the unfit, +0.0 here)
            s = np.tile(np.linspace(0.9, 0.4, 8, dtype=np.float32), (2, 1))
            l = (np.arange(160, dtype=np.float32).reshape(2, 8, 10) % 9) + np.float32(min(dx, dy))
            c = np.array([6, 5], np.int32)
            places = [(f, f, 0, 0, wu, hu, dx, dy, rw, rh) for f in range(2)]
            a = ops.merge_packed(places, 2, frame, NET, d, s, l, c, 8, thresh=1.0, rot=rot)
            b = ops.unrot_rows(frame, NET, d, s, l, c, 8, rot=rot, fit=fit)
            assert a[2].tolist() == b[2].tolist() == [6, 5] and a[3].tolist() == b[3].tolist()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (frame, rot, fit)


# ------------------------------------------------------------------------------------------ the context
FRAME_HW = (72, 96)             # the stored frames of the engine tests
LAYOUT = dict(tile=(64, 48), overlap=8, scales=(1.0, 0.5))


def engine_layout(rot, gutter=0, Bf=2):
    """The packer's output for the views of the UPRIGHT view: tiles (each a canvas of its own) and two levels (sharing canvases)."""
    hu, wu = upright_hw(FRAME_HW, rot)
    views = ops.view_layout(hu, wu, *NET, **LAYOUT)
    assert len(views) >= 4 and (views[-1][6] < NET[1] and views[-1][7] < NET[0])
    places, N = ops.pack_views(views, Bf, NET, gutter)
    assert N < Bf * len(views)                                                   # something shares a canvas
    return views, [tuple(p) for p in places.tolist()], N


def net_rows(per):
    """The per-canvas decode results (network coordinates) as the merge's tables."""
    rows = max(1, max(len(d) for d, _ in per))
    N = len(per)
    d, s, l, c = np.zeros((N, rows, 4), np.float32), np.zeros((N, rows), np.float32), np.zeros((N, rows, 10), np.float32), np.zeros((N,), np.int32)
    for n, (dd, ll) in enumerate(per):
        c[n] = len(dd)
        d[n, :len(dd)], s[n, :len(dd)], l[n, :len(dd)] = dd[:, :4], dd[:, 4], ll
    return d, s, l, c


def packrot_engine(rot, fmt="bgr", gutter=0, seed=0, **engine):
    """A 64 x 96 context with the default (synthetic) weights and two stored 72 x 96 frames whose rotated packed forward keeps rows in
    both frames after the merge -- and no more than a tracker holds --, at the highest score of a ladder that does: (engine, dense frames,
    placements, N, score).  The default weights answer to one of the source kinds."""
    h, w = FRAME_HW
    _, places, N = engine_layout(rot, gutter)
    eng = cfa.Engine(NET[0], NET[1], max_batch=N, dtype="bf16", **engine)
    tried = []
    for score in (0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05):
        for k, kind in enumerate(("blocks", "binary", "noise") * 2):
            dense = source_frames(np.random.default_rng(seed + 10 * k), kind, (2, h, w, 3) if fmt == "bgr" else (2, h * 3 // 2, w))
            eng.forward_packed_enqueue(dense, places, N, fmt, rot=rot)
            eng.decode_threshold(score, 0.3, 256)
            n = [len(d) for d, _ in eng.merge_packed(max_out=1024)[0]]
            tried.append((score, kind, n))
            if min(n) >= 1 and sum(n) >= 3 and max(n) <= 120:
                print("packrot_engine:", tried[-1])
                return eng, dense, places, N, score
    raise AssertionError(tried)


@pytest.mark.parametrize("rot,fmt,gutter", [(90, "bgr", 0), (270, "nv12", 3), (90, "nv12", 3), (270, "bgr", 0)])
def test_engine_forward_packed_rot_writes_the_restated_canvases(rot, fmt, gutter):
    """cf_forward_packed_rot with the packer's output for the upright view, host-staged (padded rows, and one dense block) and in
    place on device planes: cf_get_resized_input returns the restated canvases; the planes are untouched; the refusals."""
    h, w = FRAME_HW
    hu, wu = upright_hw(FRAME_HW, rot)
    _, places, N = engine_layout(rot, gutter)
    dense = dense_frames(np.random.default_rng(rot + gutter), fmt, 2, FRAME_HW)
    want = packed_rot_canvases_ref(bgr_of(dense, fmt), rot, places, N, NET, FILL_BGR)
    eng = cfa.Engine(NET[0], NET[1], max_batch=N, dtype="bf16")
    frames, bufs, p0, p1 = pitched_frames(dense, fmt, 0xFF)
    for src in (frames, dense):
        eng.forward_packed_enqueue(src, places, N, fmt, fill=FILL_BGR, rot=rot)
        assert eng.last_B == N
        _diff(eng.resized_input(), want, fmt, rot, "host")
    frames, bufs, p0, p1 = pitched_frames(dense, fmt, 0x00, aligned=True)
    dev = [eng.device_alloc(b.nbytes) for b in bufs]
    for dv, b in zip(dev, bufs):
        eng.memcpy_h2d(dv, b)
    n = len(frames[0])
    planes = [tuple(dev[b * n:(b + 1) * n]) for b in range(2)]
    eng.forward_packed_enqueue(planes, places, N, fmt, fill=FILL_BGR, on_device=True, h=h, w=w, pitch0=p0, pitch1=p1, rot=rot)
    _diff(eng.resized_input(), want, fmt, rot, "device")
    for dv, b in zip(dev, bufs):                                                 # read in place: the planes are untouched
        back = np.empty_like(b)
        eng.memcpy_d2h(back, dv)
        assert np.array_equal(back, b)
        eng.device_free(dv)
    # refusals name their value and leave the engine working
    with pytest.raises(ValueError) as e:
        eng.forward_packed_enqueue(dense, places, N, fmt, rot=45)
    assert "rot=45" in str(e.value)
    with pytest.raises(ValueError) as e:                                         # a source inside the stored (h, w), outside the upright view
        eng.forward_packed_enqueue(dense, [(0, 0, 0, 0, w, h, 0, 0, 8, 8)], N, fmt, rot=rot)
    assert "placement 0" in str(e.value) and "inside the frame" in str(e.value) and "UPRIGHT" in str(e.value)
    with pytest.raises(ValueError) as e:
        eng.forward_packed_enqueue(dense, places, N + 1, fmt, rot=rot)
    assert "max_batch" in str(e.value)
    eng.forward_packed_enqueue(dense, places, N, fmt, fill=FILL_BGR, rot=rot)
    _diff(eng.resized_input(), want, fmt, rot, "again")
    assert (hu, wu) == (w, h)                                                    # (a quarter turn: the layout above was made for the swapped sides)
    eng.close()


@pytest.mark.parametrize("rot", (90, 270))
def test_engine_packed_rot_decode_and_merge_equal_the_restatement(rot):
    eng, dense, places, N, score = packrot_engine(rot)
    canv = packed_rot_canvases_ref(dense, rot, places, N, NET)
    _diff(eng.resized_input(), canv, "engine")
    per = eng.decode_threshold(score, 0.3, 256)
    assert len(per) == N
    d, s, l, c = net_rows(per)
    for opt in (dict(metric="ios", thresh=0.5, edge=2.0), dict(metric="iou", thresh=0.3, edge=0.0)):
        want, wflags = merge_packed_rot_ref(places, 2, FRAME_HW, rot, d, s, l, c, **opt)
        eng.forward_packed_enqueue(dense, places, N, "bgr", rot=rot)
        with pytest.raises(cfa._lib.CenterFaceError) as e:                 # before a decode
            eng.merge_packed(**opt)
        assert e.value.code == CF_ESTATE
        assert same_results(eng.decode_threshold(score, 0.3, 256), per)
        got, flags = eng.merge_packed(max_out=256, **opt)
        print("merged per frame:", [len(x) for x, _ in got], "of", int(c.sum()))
        assert same_results(got, want) and flags.tolist() == wflags.tolist() == [0, 0]
        assert min(len(x) for x, _ in got) >= 1
        # the rows are in the STORED frame, not in the upright view: the unturned restatement of the same tables differs
        assert not same_results(got, merge_packed_rot_ref(places, 2, upright_hw(FRAME_HW, rot), 0, d, s, l, c, **opt)[0])
        mo = 64                                                            # the device form, read back
        bufs = [eng.device_alloc(2 * mo * 5 * 4), eng.device_alloc(2 * mo * 10 * 4), eng.device_alloc(8), eng.device_alloc(8)]
        eng.merge_packed_device(mo, *bufs, **opt)
        eng.synchronize()
        hd, hl, hc, hf = np.empty((2, mo, 5), np.float32), np.empty((2, mo, 10), np.float32), np.empty(2, np.int32), np.empty(2, np.int32)
        for a, b in zip((hd, hl, hc, hf), bufs):
            eng.memcpy_d2h(a, b)
            eng.device_free(b)
        assert hc.tolist() == [len(x) for x, _ in want] and hf.tolist() == [0, 0]
        assert same_results([(hd[f, :min(hc[f], mo)], hl[f, :min(hc[f], mo)]) for f in range(2)], [(x[:mo], y[:mo]) for x, y in want])
    eng.close()


def test_engine_packed_rot_under_the_flip_test():
    """With the flip test on, the N canvases are as restated, their mirrors sit behind them (whole canvases), N must fit half the
    context, and the merge runs on the rows of the merged heads."""
    rot = 90
    eng, dense, places, N, score = packrot_engine(rot, "nv12", gutter=3, seed=2, flip_test=True)      # (the engine doubles the context for the mirrors)
    want = packed_rot_canvases_ref(bgr_of(dense, "nv12"), rot, places, N, NET)
    eng.forward_packed_enqueue(dense, places, N, "nv12", rot=rot)
    assert eng.last_B == N
    both = np.empty((2 * N,) + NET + (3,), np.uint8)
    eng._chk(eng._L.cf_get_resized_input(eng._h, cfa._lib.ptr(both), 2 * N))
    _diff(both[:N], want, "flip")
    assert np.array_equal(both[N:], both[:N, :, ::-1])                      # the second half is the mirror
    per = eng.decode_threshold(score, 0.3, 256)
    assert len(per) == N
    d, s, l, c = net_rows(per)
    got, flags = eng.merge_packed(max_out=256)
    assert same_results(got, merge_packed_rot_ref(places, 2, FRAME_HW, rot, d, s, l, c)[0]) and min(len(x) for x, _ in got) >= 1
    with pytest.raises(ValueError) as e:
        eng.forward_packed_enqueue(dense, places, N + 1, "nv12", rot=rot)
    assert "flip test" in str(e.value)
    eng.close()


@pytest.mark.parametrize("rot,fmt", [(90, "bgr"), (270, "nv12")])
def test_state_rules_and_the_consumers_behind_a_rotated_packed_merge(rot, fmt):
    eng, dense, places, N, score = packrot_engine(rot, fmt, seed=1)
    h, w = FRAME_HW
    opt = dict(mode="solid", shape="rect", fill=(1, 2, 3))

    def estate(call):
        with pytest.raises(cfa._lib.CenterFaceError) as e:
            call()
        assert e.value.code == CF_ESTATE, e.value

    frames, bufs, _, _ = pitched_frames(dense, fmt, 0xFF)
    eng.forward_packed_enqueue(dense, places, N, fmt, rot=rot)
    estate(eng.merge_packed)                                               # without a threshold decode
    per = eng.decode_threshold(score, 0.3, 256)
    estate(eng.merge_views)                                                # it is not a views forward ...
    estate(eng.merge_tiles)                                                # ... nor a tiled ...
    estate(eng.unfit_rows)                                                 # ... nor a fitted or a rotated single-view one
    estate(lambda: eng.redact_faces(frames, fmt, **opt))                   # a forward and a decode, but no merge
    trk = cfa.Tracker(eng, 2, min_hits=1)
    estate(lambda: eng.track_update_device(trk, 0))
    merged, flags = eng.merge_packed(max_out=256)
    counts = np.array([len(d) for d, _ in merged], np.int32)
    assert counts.min() >= 1 and flags.tolist() == [0, 0]
    assert same_results(merged, merge_packed_rot_ref(places, 2, FRAME_HW, rot, *net_rows(per))[0])
    estate(eng.merge_views)
    estate(eng.merge_tiles)
    estate(eng.unfit_rows)
    # the redaction of the STORED frames with the merged boxes, which are in their pixels: (H, W) = (h, w)
    boxes = np.concatenate([d[:, :4] for d, _ in merged])
    wframes, wbufs, _, _ = pitched_frames(dense, fmt, 0xFF)
    redact_ref(wframes, fmt, boxes, counts, (h, w), h, w, **opt)
    assert eng.redact_faces(frames, fmt, **opt) is frames
    assert all(np.array_equal(a, b) for a, b in zip(bufs, wbufs))
    assert not all(np.array_equal(a, b) for a, b in zip(bufs, pitched_frames(dense, fmt, 0xFF)[1]))      # something was redacted
    chips, offs, _ = eng.align_faces_frame(dense, fmt, 32)                 # one chip per merged row, cut from the stored frames
    assert np.diff(offs).tolist() == counts.tolist() and len(chips) == int(counts.sum())
    # the tracker takes the merged rows of Bf frames of (h, w) STORED; a second update behind one merge is refused
    dev = eng.device_alloc(8)
    eng.track_update_device(trk, 0, counts_ptr=dev)
    eng.synchronize()
    tc = np.empty(2, np.int32)
    eng.memcpy_d2h(tc, dev)
    assert tc.tolist() == counts.tolist()
    estate(lambda: eng.track_update_device(trk, 0))
    # ... and, latched in (tiled, h, w) stored, it continues the stream over a second call: the same frames confirm every track
    eng.forward_packed_enqueue(dense, places, N, fmt, rot=rot)
    eng.decode_threshold(score, 0.3, 256)
    eng.merge_packed(max_out=256)
    eng.track_update_device(trk, 0, counts_ptr=dev)
    eng.synchronize()
    eng.memcpy_d2h(tc, dev)
    eng.device_free(dev)
    assert (tc >= counts).all() and (tc <= np.minimum(2 * counts, trk.max_tracks)).all()      # (a box that does not match itself -- inverted -- is born anew)
    trk.close()
    # any other forward forgets the turn and the placements
    views0 = ops.view_layout(h, w, *NET, scales=(1.0,))
    for forward in (lambda: eng.forward_views_enqueue(dense, views0, fmt), lambda: eng.forward_fit_enqueue(dense, fmt),
                    lambda: eng.forward_rot_enqueue(dense, fmt, rot, fit=True)):
        forward()
        eng.decode_threshold(score, 0.3, 256)
        estate(eng.merge_packed)
    # an unturned packed forward behind a turned one is merged unturned
    places0 = unpacked_places(views0, 2)
    eng.forward_packed_enqueue(dense, places0, 2, fmt)
    per0 = eng.decode_threshold(score, 0.3, 256)
    assert same_results(eng.merge_packed(max_out=256)[0], merge_packed_rot_ref(places0, 2, FRAME_HW, 0, *net_rows(per0))[0])
    # ... and an upload forgets the turn
    eng.forward_packed_enqueue(dense, places, N, fmt, rot=rot)
    eng.decode_threshold(score, 0.3, 256)
    eng.upload_images(list(packed_rot_canvases_ref(bgr_of(dense, fmt), rot, places, N, NET)[:2]))
    estate(eng.merge_packed)
    eng.close()


# ------------------------------------------------------------------------------------------ the product paths
def engine_sequence(face, frames, fmt, rot, per, pack, gutter=0):
    """view_layout(hu, wu) + (pack_views | the unpacked list) + forward_packed(rot) + decode + merge_packed, chunk by chunk: as
    detect_views(rotate=) is to run them."""
    hu, wu = upright_hw(FRAME_HW, rot)
    views = ops.view_layout(hu, wu, *NET, **LAYOUT)
    out = []
    for i in range(0, len(frames), per):
        chunk = frames[i:i + per]
        places, N = ops.pack_views(views, len(chunk), NET, gutter) if pack else (unpacked_places(views, len(chunk)), len(chunk) * len(views))
        face.engine.forward_packed_enqueue(chunk, places, N, fmt, rot=rot)
        face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets)
        out += face.engine.merge_packed(max_out=face.max_dets)[0]
    return out


def test_centerface_detect_views_rotated_and_anonymize():
    """detect_views(rotate=90, tile=, scales=, pack=False / True) = the same calls made by hand on the engine;
    anonymize(views=dict(rotate=270, pack=True)) and anonymize_yuv change exactly the bytes redact_ref changes for the merged boxes;
    rotate=0 and views=dict(rotate=0) are the calls without the key."""
    h, w = FRAME_HW
    face = cfa.CenterFace(NET[0], NET[1], dtype="bf16", max_batch=16)
    V = len(ops.view_layout(w, h, *NET, **LAYOUT))
    per_unpacked = 16 // V
    counts = [ops.pack_views(ops.view_layout(w, h, *NET, **LAYOUT), n, NET)[1] for n in (1, 2, 3, 4)]
    per_packed = max(n for n, c in zip((1, 2, 3, 4), counts) if c <= 16)
    assert per_unpacked >= 1 and 1 <= per_packed <= 3
    rng = np.random.default_rng(2)
    tried = []
    for kind in ("blocks", "binary", "noise", "blocks", "binary", "noise"):  # the default weights answer to one of them
        imgs = source_frames(rng, kind, (3, h, w, 3))
        got = face.detect_views(imgs, pack=True, rotate=90, **LAYOUT)
        n270 = sum(len(d) for d, _ in face.detect_views(imgs, pack=True, rotate=270, **LAYOUT))
        tried.append((kind, [len(d) for d, _ in got], n270))
        if sum(len(d) for d, _ in got) >= 2 and n270 >= 2:
            break
    print("detect_views(pack=True, rotate=90 | 270):", tried)
    assert sum(len(d) for d, _ in got) >= 2 and n270 >= 2, tried
    assert all(d.shape[1:] == (5,) and l.shape == (len(d), 10) and d.dtype == np.float32 for d, l in got)
    assert same_results(got, engine_sequence(face, imgs, "bgr", 90, per_packed, True))
    assert same_results(face.detect_views(imgs, rotate=90, **LAYOUT), engine_sequence(face, imgs, "bgr", 90, per_unpacked, False))
    assert same_results(face.detect_views(imgs, pack=True, gutter=2, rotate=180, **LAYOUT), engine_sequence_180(face, imgs, 2))
    opts = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    want = engine_sequence(face, imgs, "bgr", 270, per_packed, True)
    keep = imgs.copy()
    out, dets = face.anonymize(list(imgs), views=dict(LAYOUT, rotate=270, pack=True), **opts)
    assert np.array_equal(imgs, keep) and same_results(dets, want)
    ref = keep.copy()
    redact_ref([(f.reshape(h, -1),) for f in ref], "bgr", np.concatenate([d[:, :4] for d, _ in want]), [len(d) for d, _ in want], (h, w), h, w, **opts)
    assert np.array_equal(out, ref)
    # NV12 frames of the same size
    yuv = source_frames(np.random.default_rng(3), tried[-1][0], (3, h * 3 // 2, w))
    ywant = engine_sequence(face, yuv, "nv12", 270, per_packed, True)
    yout, ydets = face.anonymize_yuv(yuv, "nv12", views=dict(LAYOUT, rotate=270, pack=True), **opts)
    assert same_results(ydets, ywant)
    yref = yuv.copy()
    redact_ref([(f[:h], f[h:]) for f in yref], "nv12", np.concatenate([d[:, :4] for d, _ in ywant]), [len(d) for d, _ in ywant], (h, w), h, w, **opts)
    assert np.array_equal(yout, yref)
    assert sum(len(d) for d, _ in want) >= 2 and not np.array_equal(out, keep)                  # something was redacted
    # annotate and the chips take the same path
    _, adets = face.annotate(list(imgs), views=dict(LAYOUT, rotate=270, pack=True))
    assert same_results(adets, want)
    rows = face.detect_aligned_frames(imgs, "bgr", 32, views=dict(LAYOUT, rotate=270, pack=True))
    assert same_results([(d, l) for d, l, _ in rows], want) and [len(c) for _, _, c in rows] == [len(d) for d, _ in want]
    # rotate=0 and views=dict(rotate=0): every call does what it did
    for pack in (False, True):
        plain = face.detect_views(imgs, pack=pack, **LAYOUT)
        assert same_results(face.detect_views(imgs, pack=pack, rotate=0, **LAYOUT), plain)
        a = face.anonymize(list(imgs), views=dict(LAYOUT, pack=pack, rotate=0), **opts)
        b = face.anonymize(list(imgs), views=dict(LAYOUT, pack=pack), **opts)
        assert a[0].tobytes() == b[0].tobytes() and same_results(a[1], b[1]) and same_results(b[1], plain)
    face.close()


def engine_sequence_180(face, frames, gutter):
    """The hand-made sequence of detect_views(pack=True, gutter=, rotate=180): the upright view has the stored frame's size."""
    views = ops.view_layout(FRAME_HW[0], FRAME_HW[1], *NET, **LAYOUT)
    per, out = 1, []
    while per < len(frames) and ops.pack_views(views, per + 1, NET, gutter)[1] <= face.engine.max_batch:
        per += 1
    for i in range(0, len(frames), per):
        chunk = frames[i:i + per]
        places, N = ops.pack_views(views, len(chunk), NET, gutter)
        face.engine.forward_packed_enqueue(chunk, places, N, "bgr", rot=180)
        face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets)
        out += face.engine.merge_packed(max_out=face.max_dets)[0]
    return out
