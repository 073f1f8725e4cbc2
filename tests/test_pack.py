"""Packed views on the GPU: the packed cutter (cf_op_packed, cf_forward_packed), the merge by placement (cf_op_merge_packed,
cf_merge_packed), the state rules and the product paths behind them, every byte against the restatements of tests/pack_cases.py (canvas =
fill, then per placement the restated cut of its source rectangle pasted at its content; merge = merge_views_ref over placements).  The
anchor: the placement list {f, f * V + v, views[v]} gives cf_forward_views' bytes and cf_merge_views' bits."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from pack_cases import merge_packed_ref, pack_views_ref, packed_canvases_ref, unpacked_places
from test_redact import redact_ref, source_frames
from test_tiles import FILL, bgr_of, pitched_frames, same_results
from test_views import FORMATS, LEVELS, TILES, cut_case, random_table, views_for
from view_cases import view_layout_ref

pytestmark = pytest.mark.gpu

NET = (32, 64)                  # (H, W) of every context and canvas here
FILL_BGR = (1, 2, 3)
CF_ESTATE = cfa._lib.CF_ESTATE


def _diff(got, want, *what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and len(bad) == 0, what + (got.shape, want.shape, len(bad), bad[:4].tolist())


# ------------------------------------------------------------------------------------------ the cutter
@pytest.mark.parametrize("fmt", FORMATS)
def test_op_packed_of_the_unpacked_list_is_the_views_cutter(fmt):
    """The placement list {f, f * V + v, views[v]} of the fifteen views of tests/test_views.py, Bf = 2 frames of 70 x 94 and 72 x 96, rows
    with padding that holds 0xFF or 0x00: every byte is ops.cut_views' and the restatement's."""
    for hw in ((70, 94), (72, 96)):
        dense, bgr, views, want = cut_case(fmt, hw)
        places, N = unpacked_places(views, 2), 2 * len(views)
        want = want.reshape((N,) + NET + (3,))
        assert np.array_equal(packed_canvases_ref(bgr, places, N, NET, FILL_BGR), want)      # the two restatements agree
        for pad in (0xFF, 0x00):
            frames, _, _, _ = pitched_frames(dense, fmt, pad)
            _diff(ops.cut_packed(frames, places, N, NET, fmt, fill=FILL_BGR), want, fmt, hw, pad)
        got = ops.cut_packed(dense, places, N, NET, fmt, fill=FILL_BGR)
        _diff(got, ops.cut_views(dense, views, NET, fmt, fill=FILL_BGR).reshape(want.shape), fmt, hw, "cut_views")
        # the order of the list is free: reversed, the canvases are the same
        _diff(ops.cut_packed(dense, places[::-1], N, NET, fmt, fill=FILL_BGR), want, fmt, hw, "reversed")


def hand_table(h, w):
    """A hand-made packed table for Bf = 2 in (32, 64) canvases, (placements, N = 6); the comments say what each canvas is there for."""
    whole = (0, 0, w, h)
    p = [(0, 0) + whole + (0, 0, 21, 13),                      # canvas 0: two frames in one canvas;
         (1, 0) + whole + (21, 0, 30, 13),                     #   a shared vertical edge at x = 21 (not a multiple of 4),
         (0, 0, 10, 20, 24, 16, 0, 13, 21, 10),                #   a shared horizontal edge at y = 13 (not a multiple of 4),
         (1, 0, w - 30, h - 22, 30, 22, 21, 13, 43, 19),       #   a content that ends in the canvas's far corner; fill at x >= 51, y < 13
         (1, 1) + whole + (63, 31, 1, 1),                      # canvas 1: a 1 x 1 content in the last lane and row,
         (0, 1, 6, 8, 18, 20, 5, 30, 2, 2)]                    #   a 2 x 2 content inside one lane, in the last rows; canvas 2: empty
    for k in range(32):                                        # canvas 3: tiled completely by 32 contents of 8 x 8, frames alternating
        src = (2 * (k % 7), 2 * (k % 5), 8 + 4 * (k % 6), 8 + 2 * (k % 9)) if k % 3 else (4 * (k % 8), 2 * k, 8, 8)      # (k % 3 == 0: identity)
        p.append((k & 1, 3) + src + (8 * (k % 8), 8 * (k // 8), 8, 8))
    for k in range(512):                                       # canvas 4: tiled completely by 512 contents of 2 x 2: the tile's list takes two rounds
        src = (2 * (k % 40), 2 * (k % 31), 2, 2) if k % 5 else (2 * (k % 11), 2 * (k % 13), 6, 4)
        p.append(((k // 3) & 1, 4) + src + (2 * (k % 32), 2 * (k // 32), 2, 2))
    p.append((0, 5) + whole + (0, 0, 64, 32))                  # canvas 5: one content that is the whole canvas
    return [tuple(int(v) for v in x) for x in p], 6


_hand_cache = {}


def hand_case(fmt, hw):
    if (fmt, hw) not in _hand_cache:
        dense, bgr, _, _ = cut_case(fmt, hw)
        places, N = hand_table(*hw)
        _hand_cache[(fmt, hw)] = (dense, bgr, places, N, packed_canvases_ref(bgr, places, N, NET, FILL_BGR))
    return _hand_cache[(fmt, hw)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_op_packed_hand_made_table(fmt):
    for hw in ((70, 94), (72, 96)):
        dense, bgr, places, N, want = hand_case(fmt, hw)
        for pad in (0xFF, 0x00):
            frames, _, _, _ = pitched_frames(dense, fmt, pad)
            _diff(ops.cut_packed(frames, places, N, NET, fmt, fill=FILL_BGR), want, fmt, hw, pad)
        # what the restatement says of the table: the empty canvas is all fill, the fill beside the contents of canvas 0 and 1 stands
        assert (want[2] == FILL_BGR).all() and (want[0, :13, 51:] == FILL_BGR).all() and (want[1, :30] == FILL_BGR).all() and (want[1, 31, 7:63] == FILL_BGR).all()
        assert np.array_equal(want[3, 0:8, 0:8], bgr[0, 0:8, 0:8]) and np.array_equal(want[3, 8:16, 8:16], bgr[1, 18:26, 4:12])      # identities, k = 0 and 9
        assert np.array_equal(want[4, 0:2, 2:4], bgr[0, 2:4, 2:4])                                                                      # k = 1 of the 2 x 2 ones
        # another fill reaches every fill byte and no content byte
        _diff(ops.cut_packed(dense, places, N, NET, fmt), packed_canvases_ref(bgr, places, N, NET), fmt, hw, "black")


@pytest.mark.parametrize("gutter", (0, 1, 3))
def test_op_packed_of_the_packers_output(gutter):
    """ops.pack_views on the half and the quarter level (and a third of odd size) of Bf = 5 frames of 70 x 94, NV12 and BGR."""
    h, w = 70, 94
    views = view_layout_ref(h, w, *NET, scales_pm=(500, 250, 330))
    places, N = ops.pack_views(views, 5, NET, gutter)
    ref, refN = pack_views_ref(views, 5, NET[0], NET[1], gutter)
    assert N == refN < 5 and places.tolist() == [list(p) for p in ref]
    assert len({(p[0], p[1]) for p in ref}) > N                                # some canvas holds more than one frame
    for fmt in ("nv12", "bgr"):
        dense = np.random.default_rng(21 + gutter).integers(0, 256, (5, h, w, 3) if fmt == "bgr" else (5, h * 3 // 2, w), dtype=np.uint8)
        frames, _, _, _ = pitched_frames(dense, fmt, 0xFF)
        _diff(ops.cut_packed(frames, places, N, NET, fmt, fill=FILL_BGR), packed_canvases_ref(bgr_of(dense, fmt), places, N, NET, FILL_BGR), fmt, gutter)


@pytest.mark.parametrize("fmt", ("yv12", "bgr"))
def test_op_packed_frames_0_and_64_on_one_canvas(fmt):
    """Bf = 65 frames of 8 x 8 into 33 canvases of (4, 8): canvas n holds frame n on the left and frame 64 - n on the right, so frame 0 and
    frame 64 share canvas 0 -- no table of 64 frames serves that (YV12: the planes swapped)."""
    rng = np.random.default_rng(90 + FORMATS.index(fmt))
    dense = rng.integers(0, 256, (65, 8, 8, 3) if fmt == "bgr" else (65, 12, 8), dtype=np.uint8)
    places = []
    for n in range(33):
        places += [(n, n, 0, 2, 8, 4, 0, 0, 4, 4), (64 - n, n, 2, 0, 6, 8, 4, 1, 4, 3)]
    want = packed_canvases_ref(bgr_of(dense, fmt), places, 33, (4, 8), FILL_BGR)
    frames, _, _, _ = pitched_frames(dense, fmt, 0xFF)
    _diff(ops.cut_packed(frames, places, 33, (4, 8), fmt, fill=FILL_BGR), want, fmt)


# ------------------------------------------------------------------------------------------ the context's forward
@pytest.mark.parametrize("fmt", FORMATS)
def test_engine_forward_packed_writes_the_restated_canvases(fmt):
    """cf_forward_packed, host-staged (padded rows, and one dense block) and in place on device planes: cf_get_resized_input returns the
    restated canvases; the planes are untouched; the refusals that need a context."""
    hw = (72, 96)
    dense, bgr, places, N, want = hand_case(fmt, hw)
    eng = cfa.Engine(NET[0], NET[1], max_batch=N, dtype="bf16")
    frames, bufs, p0, p1 = pitched_frames(dense, fmt, 0xFF)
    for src in (frames, dense):
        eng.forward_packed_enqueue(src, places, N, fmt, fill=FILL_BGR)
        assert eng.last_B == N
        _diff(eng.resized_input(), want, fmt, "host")
    for pad in (0xFF, 0x00):
        frames, bufs, p0, p1 = pitched_frames(dense, fmt, pad, aligned=True)
        dev = [eng.device_alloc(b.nbytes) for b in bufs]
        for d, b in zip(dev, bufs):
            eng.memcpy_h2d(d, b)
        n = len(frames[0])
        planes = [tuple(dev[b * n:(b + 1) * n]) for b in range(2)]
        eng.forward_packed_enqueue(planes, places, N, fmt, fill=FILL_BGR, on_device=True, h=hw[0], w=hw[1], pitch0=p0, pitch1=p1)
        _diff(eng.resized_input(), want, fmt, pad)
        for d, b in zip(dev, bufs):                                                  # read in place: the planes are untouched
            back = np.empty_like(b)
            eng.memcpy_d2h(back, d)
            assert np.array_equal(back, b)
        with pytest.raises(ValueError):                                              # a misaligned device plane
            eng.forward_packed_enqueue([(planes[0][0] + 2,) + planes[0][1:]] + planes[1:], places, N, fmt, on_device=True, h=hw[0], w=hw[1], pitch0=p0, pitch1=p1)
        for d in dev:
            eng.device_free(d)
    # another table behind the first one: the device table is replaced (here: the unpacked list of three views)
    _, _, views, vwant = cut_case(fmt, hw)
    eng.forward_packed_enqueue(dense, unpacked_places(views[:3], 2), 6, fmt, fill=FILL_BGR)
    _diff(eng.resized_input(), vwant[:, :3].reshape((6,) + NET + (3,)), fmt, "second table")
    # refusals name the placement and leave the engine working; the content must lie inside THIS canvas; N must fit max_batch
    with pytest.raises(ValueError) as e:
        eng.forward_packed_enqueue(dense, places[:3] + [(0, 1, 0, 0, 96, 72, 1, 0, 64, 32)], N, fmt)
    assert "placement 3" in str(e.value) and "canvas" in str(e.value)
    with pytest.raises(ValueError) as e:
        eng.forward_packed_enqueue(dense, places[:4] + [(1, 0, 0, 0, 96, 72, 52, 14, 2, 2)], N, fmt)
    assert "placements 3 and 4 overlap" in str(e.value)
    with pytest.raises(ValueError) as e:
        eng.forward_packed_enqueue(dense, places, N + 1, fmt)
    assert "max_batch" in str(e.value)
    eng.forward_packed_enqueue(dense, places, N, fmt, fill=FILL_BGR)
    _diff(eng.resized_input(), want, fmt, "again")
    eng.close()


def test_engine_forward_packed_under_the_flip_test():
    """With the flip test on the N canvases are followed by their mirrors (whole canvases, whole pixels reversed per row), and N must fit
    half the context: as the views forward behaves."""
    dense, bgr, places, N, want = hand_case("nv12", (72, 96))
    eng = cfa.Engine(NET[0], NET[1], max_batch=N, dtype="bf16", flip_test=True)      # (the engine doubles the context for the mirrors)
    eng.forward_packed_enqueue(dense, places, N, "nv12", fill=FILL_BGR)
    assert eng.last_B == N
    both = np.empty((2 * N,) + NET + (3,), np.uint8)
    eng._chk(eng._L.cf_get_resized_input(eng._h, cfa._lib.ptr(both), 2 * N))
    _diff(both[:N], want, "flip")
    assert np.array_equal(both[N:], both[:N, :, ::-1])                      # the second half is the mirror
    with pytest.raises(ValueError) as e:
        eng.forward_packed_enqueue(dense, places, N + 1, "nv12")
    assert "flip test" in str(e.value)
    eng.close()


# ------------------------------------------------------------------------------------------ the merge on hand-built tables
def check_merge(places, Bf, frame_hw, net_hw, d, s, l, counts, max_out, **opt):
    """ops.merge_packed against merge_packed_ref, bit for bit: counts, flags, the rows below min(count, max_out), and the caller's bytes
    in every row behind them."""
    d, s, l = (np.asarray(a, np.float32) for a in (d, s, l))
    od, ol = np.full((Bf, max_out, 5), FILL), np.full((Bf, max_out, 10), FILL)
    gd, gl, gc, gf = ops.merge_packed(places, Bf, frame_hw, net_hw, d, s, l, counts, max_out, dets=od, lms=ol, **opt)
    want, wflags = merge_packed_ref(places, Bf, frame_hw, d, s, l, counts, **opt)
    assert gc.tolist() == [len(w[0]) for w in want], (gc, [len(w[0]) for w in want])
    assert gf.tolist() == wflags.tolist()
    for f, (wd, wl) in enumerate(want):
        m = min(len(wd), max_out)
        assert gd[f, :m].tobytes() == wd[:m].tobytes(), (f, gd[f, :m], wd[:m])
        assert gl[f, :m].tobytes() == wl[:m].tobytes(), f
        assert (gd[f, m:] == FILL).all() and (gl[f, m:] == FILL).all(), f
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


def test_merge_packed_of_the_unpacked_list_is_the_views_merge():
    """Random tables of test_views.py's kind (V = 5 views x 256 rows: the 1024-wide round runs twice; ties; an empty, a truncated view; a
    NaN; a frame without rows): the unpacked list gives ops.merge_views' dets, landmarks, counts and flags, bit for bit."""
    rng = np.random.default_rng(5)
    frame, net, rows = (64, 96), (64, 64), 256
    views = TILES + LEVELS + [(30, 20, 40, 30, 7, 5, 51, 39)]
    d, s, l = random_table(rng, views, 3, rows, net)
    c = np.zeros((3, 5), np.int32)
    c[0] = [rows, 0, rows - 7, 31, rows]
    c[1] = [rows + 9, rows, 1, rows, 64]
    d[1, 1, 5, 2] = np.nan
    places = unpacked_places(views, 3)
    pd, ps, pl, pc = d.reshape(15, rows, 4), s.reshape(15, rows), l.reshape(15, rows, 10), c.reshape(15)
    for opt in (dict(metric="ios", thresh=0.5, edge=2.0), dict(metric="iou", thresh=0.3, edge=0.0)):
        a = ops.merge_packed(places, 3, frame, net, pd, ps, pl, pc, 5 * rows, **opt)
        b = ops.merge_views(views, frame, net, d, s, l, c, 5 * rows, **opt)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), opt
        assert a[2][2] == 0 and a[3].tolist() == [0, 1, 0] and a[2][0] > 8 and a[2][1] > 8
    check_merge(places, 3, frame, net, pd, ps, pl, pc, 5 * rows)
    check_merge(places, 3, frame, net, pd, ps, pl, pc, 7, metric="iou", thresh=0.3, edge=0.0)      # truncated outputs


# one 64 x 64 canvas, 64 x 96 frames: frame 0 at x in [0, 32), y in [0, 22); frame 1 beside it (shared edge x = 32) and below it (y = 22)
SHARED = [(0, 0, 0, 0, 96, 64, 0, 0, 32, 22), (1, 0, 0, 0, 96, 64, 32, 0, 32, 22), (1, 0, 0, 0, 96, 64, 0, 22, 32, 22)]


def test_merge_packed_rows_in_the_neighbour_in_the_fill_and_on_a_shared_edge():
    frame, net = (64, 96), (64, 64)
    rows = [(4, 4, 12, 12, 0.9),          # in frame 0's content
            (40, 5, 50, 15, 0.8),         # in the neighbour's content: frame 1's, mapped by ITS view
            (40, 30, 50, 40, 0.95),       # in the fill: nobody's
            (28, 5, 36, 15, 0.7),         # cx = 32 exactly: the half-open rule gives it to the content that starts there (frame 1)
            (5, 18, 15, 26, 0.6),         # cy = 22 exactly: the content below (frame 1)
            (40, 50, 50, 60, 0.99)]       # far down in the fill
    d, s, l, c = canvas_table(1, 8, {0: rows})
    want, gc, gf = check_merge(SHARED, 2, frame, net, d, s, l, c, 8)
    assert gc.tolist() == [1, 3] and gf.tolist() == [0, 0]
    assert want[0][0][0].tolist() == [12, np.float32(4 * (64 / 22)), 36, np.float32(12 * (64 / 22)), np.float32(0.9)]
    by_score = {float(r[4]): r[:4].tolist() for r in want[1][0]}
    sy = 64 / 22
    assert by_score[float(np.float32(0.8))] == [24, np.float32(5 * sy), 54, np.float32(15 * sy)]               # (x - 32) * 3
    assert by_score[float(np.float32(0.7))] == [-12, np.float32(5 * sy), 12, np.float32(15 * sy)]
    assert by_score[float(np.float32(0.6))] == [15, np.float32((18 - 22) * sy), 45, np.float32((26 - 22) * sy)]      # (y - 22) * 64 / 22
    # one float32 step of the centre to the left (cx = 32 - 2^-19), a quarter pixel up (cy = 21.875), and the row is frame 0's
    d2 = d.copy()
    d2[0, 3, 2] = np.nextafter(np.float32(36), np.float32(0))
    d2[0, 4, 1] = 17.75
    assert (d2[0, 3, 0] + d2[0, 3, 2]) * np.float32(0.5) == np.nextafter(np.float32(32), np.float32(0))
    assert check_merge(SHARED, 2, frame, net, d2, s, l, c, 8)[1].tolist() == [3, 1]
    # the order of the walk is the placement index: the same placements listed frame 1 first give the same rows per frame
    want2, gc2, _ = check_merge([SHARED[2], SHARED[1], SHARED[0]], 2, frame, net, d, s, l, c, 8)
    assert gc2.tolist() == [1, 3] and want2[0][0].tobytes() == want[0][0].tobytes()
    # a gutter between the contents: the row on the old edge is in the fill now
    apart = [SHARED[0], (1, 0, 0, 0, 96, 64, 34, 0, 30, 22)]
    assert check_merge(apart, 2, frame, net, d, s, l, c, 8)[1].tolist() == [1, 1]
    # a frame without any placement has no rows
    assert check_merge(SHARED[:1], 2, frame, net, d, s, l, c, 8)[1].tolist() == [1, 0]


def test_merge_packed_negative_zero_unturned():
    """rot 0: a -0.0 corner and a -0.0 landmark in a content at the canvas's origin map as float32((float64(-0.0) - 0) * sx + sx0) = +0.0,
    bit for bit (the turned merges have this case in tests/test_packrot.py)."""
    d, s, l, c = canvas_table(1, 4, {0: [(-0.0, -0.0, 8, 6, 0.7)]})
    l[0, 0, :2] = -0.0
    want, gc, _ = check_merge(SHARED, 2, (64, 96), (64, 64), d, s, l, c, 4)
    assert gc.tolist() == [1, 0] and want[0][0][0].tolist() == [0, 0, 24, np.float32(6 * (64 / 22)), np.float32(0.7)]
    assert not np.signbit(want[0][0][0, :2]).any() and not np.signbit(want[0][1][0, :2]).any()


def test_merge_packed_truncated_canvas_flags_every_frame_on_it():
    frame, net = (64, 96), (64, 64)
    places = SHARED + [(2, 1, 0, 0, 96, 64, 0, 0, 32, 22), (3, 1, 0, 0, 96, 64, 32, 22, 32, 22), (3, 2, 0, 0, 96, 64, 0, 0, 64, 43)]
    rows3 = [(4, 4, 12, 12, 0.9), (40, 5, 50, 15, 0.8), (20, 30, 30, 40, 0.7)]
    d, s, l, c = canvas_table(3, 3, {0: rows3, 1: rows3, 2: rows3})
    assert check_merge(places, 4, frame, net, d, s, l, c, 8)[2].tolist() == [0, 0, 0, 0]
    c[0] = 5                                                                   # canvas 0 had more rows than the decode's max_out: frames 0 and 1
    want, gc, gf = check_merge(places, 4, frame, net, d, s, l, c, 8)
    assert gf.tolist() == [1, 1, 0, 0] and gc.tolist() == [1, 2, 1, 3]         # ... and its rows below `rows` are merged all the same
    c[0], c[2] = 3, 4                                                          # canvas 2: frame 3 alone, through its second placement
    assert check_merge(places, 4, frame, net, d, s, l, c, 8)[2].tolist() == [0, 0, 0, 1]
    c[1], c[2] = 9, 3                                                          # canvas 1: frames 2 and 3
    assert check_merge(places, 4, frame, net, d, s, l, c, 8)[2].tolist() == [0, 0, 1, 1]


def test_merge_packed_ties_and_more_than_1024_items_per_frame():
    """Bf = 3 frames with five placements each in the 16 quarter slots of four 64 x 64 canvases, 256 rows per canvas: 1280 (placement,
    row) items a frame, so the collect's 1024-wide round runs twice; whole-frame and interior sources (the edge rule); scores from 40
    values (ties); an empty, a truncated canvas, a NaN."""
    rng = np.random.default_rng(12)
    frame, net, rows = (64, 96), (64, 64), 256
    slots = [(n, x, y, 32, 32 if y == 0 or x == 0 else 20) for n in range(4) for y in (0, 32) for x in (0, 32)]
    places = []
    for i, (n, x, y, dw, dh) in enumerate(slots[:15]):
        src = (0, 0, 96, 64) if i % 2 else (32, 16, 32, 32)
        places.append((i % 3, n) + src + (x, y, dw, dh))
    assert sorted(p[0] for p in places) == [0] * 5 + [1] * 5 + [2] * 5
    c = rng.uniform(-2, 66, (4, rows, 2))
    half = rng.uniform(0.5, 7, (4, rows, 2))
    d = np.concatenate([c - half, c + half], -1).astype(np.float32)
    s = rng.choice(np.linspace(0.3, 0.95, 40).astype(np.float32), (4, rows))
    l = rng.uniform(-4, 68, (4, rows, 10)).astype(np.float32)
    counts = np.array([rows, rows + 9, rows - 7, rows], np.int32)
    d[1, 5, 2] = np.nan
    for opt in (dict(metric="ios", thresh=0.5, edge=2.0), dict(metric="iou", thresh=0.3, edge=0.0)):
        want, gc, gf = check_merge(places, 3, frame, net, d, s, l, counts, 5 * rows, **opt)
        assert gf.tolist() == [1, 1, 1] and gc.min() > 8, (gc, gf)
    counts[:] = [rows, rows, 0, 31]
    want, gc, gf = check_merge(places, 3, frame, net, d, s, l, counts, 5 * rows)
    assert gf.tolist() == [0, 0, 0]
    check_merge(places, 3, frame, net, d, s, l, counts, 7)                     # truncated outputs


# ------------------------------------------------------------------------------------------ the context's merge and the state rules
FRAME_HW = (72, 96)
LAYOUT = dict(tile=(32, 64), overlap=8, scales=(1.0, 0.5))


def engine_places():
    """Two 72 x 96 frames in fourteen (32, 64) canvases: the six tiles of each frame on canvases of their own, then the full level of
    frame 0 beside the half level of frame 1 on canvas 12 and the other way round on canvas 13."""
    h, w = FRAME_HW
    views = [tuple(v) for v in ops.view_layout(h, w, *NET, **LAYOUT).tolist()]
    assert len(views) == 8 and views[6][6:] == (43, 32)                        # (the half level is cut to 21 x 16 here: it stands beside the full one)
    places = [(f, 6 * f + t) + views[t] for f in range(2) for t in range(6)]
    for f in range(2):
        places.append((f, 12 + f) + views[6][:4] + (0, 0, 43, 32))
        places.append((1 - f, 12 + f) + views[7][:4] + (43, 3, 21, 16))
    return places, 14


def net_rows(per):
    """The per-canvas decode results (network coordinates) as the merge's tables."""
    rows = max(1, max(len(d) for d, _ in per))
    N = len(per)
    d, s, l, c = np.zeros((N, rows, 4), np.float32), np.zeros((N, rows), np.float32), np.zeros((N, rows, 10), np.float32), np.zeros((N,), np.int32)
    for n, (dd, ll) in enumerate(per):
        c[n] = len(dd)
        d[n, :len(dd)], s[n, :len(dd)], l[n, :len(dd)] = dd[:, :4], dd[:, 4], ll
    return d, s, l, c


def packed_engine(fmt="bgr", seed=0):
    """A 32 x 64 context with the default (synthetic) weights and two 72 x 96 frames whose packed forward keeps, at 0.3, rows in both
    frames after the merge: (engine, dense frames, placements, N).  The default weights answer to one of the source kinds."""
    h, w = FRAME_HW
    places, N = engine_places()
    eng = cfa.Engine(NET[0], NET[1], max_batch=N, dtype="bf16")
    tried = []
    for k, kind in enumerate(("blocks", "binary", "noise") * 3):
        dense = source_frames(np.random.default_rng(seed + 10 * k), kind, (2, h, w, 3) if fmt == "bgr" else (2, h * 3 // 2, w))
        eng.forward_packed_enqueue(dense, places, N, fmt)
        eng.decode_threshold(0.3, 0.3, 256)
        n = [len(d) for d, _ in eng.merge_packed(max_out=1024)[0]]
        tried.append((kind, n))
        if min(n) >= 1 and sum(n) >= 3:
            print("packed_engine:", tried)
            return eng, dense, places, N
    raise AssertionError(tried)


def test_engine_packed_decode_and_merge_equal_the_restatement():
    eng, dense, places, N = packed_engine()
    canv = packed_canvases_ref(dense, places, N, NET)
    _diff(eng.resized_input(), canv, "engine")
    per = eng.decode_threshold(0.3, 0.3, 256)
    assert len(per) == N
    # the per-canvas results are those of the restated canvases fed as an ordinary uint8 batch
    eng.forward_enqueue(canv)
    assert same_results(eng.decode_threshold(0.3, 0.3, 256), per)
    with pytest.raises(cfa._lib.CenterFaceError) as e:                     # ... behind which there is nothing to merge
        eng.merge_packed()
    assert e.value.code == CF_ESTATE
    d, s, l, c = net_rows(per)
    for opt in (dict(metric="ios", thresh=0.5, edge=2.0), dict(metric="iou", thresh=0.3, edge=0.0)):
        want, wflags = merge_packed_ref(places, 2, FRAME_HW, d, s, l, c, **opt)
        eng.forward_packed_enqueue(dense, places, N, "bgr")
        with pytest.raises(cfa._lib.CenterFaceError) as e:                 # before a decode
            eng.merge_packed(**opt)
        assert e.value.code == CF_ESTATE
        assert same_results(eng.decode_threshold(0.3, 0.3, 256), per)
        got, flags = eng.merge_packed(max_out=256, **opt)
        print("merged per frame:", [len(x) for x, _ in got], "of", int(c.sum()))
        assert same_results(got, want) and flags.tolist() == wflags.tolist() == [0, 0]
        assert same_results(eng.merge_packed(max_out=1, **opt)[0], want)   # truncated host form: the wrapper comes back for all of them
        mo = 64                                                            # the device form, read back; every output may be NULL
        bufs = [eng.device_alloc(2 * mo * 5 * 4), eng.device_alloc(2 * mo * 10 * 4), eng.device_alloc(8), eng.device_alloc(8)]
        eng.merge_packed_device(mo, *bufs, **opt)
        eng.synchronize()
        hd, hl, hc, hf = np.empty((2, mo, 5), np.float32), np.empty((2, mo, 10), np.float32), np.empty(2, np.int32), np.empty(2, np.int32)
        for a, b in zip((hd, hl, hc, hf), bufs):
            eng.memcpy_d2h(a, b)
            eng.device_free(b)
        assert hc.tolist() == [len(x) for x, _ in want] and hf.tolist() == [0, 0]
        assert same_results([(hd[f, :min(hc[f], mo)], hl[f, :min(hc[f], mo)]) for f in range(2)], [(x[:mo], y[:mo]) for x, y in want])
        eng.merge_packed_device(mo, **opt)
        eng.set_rescale(1.37, 1.21)                                        # cf_set_rescale changes the decode's own rows, not the merge
        assert not same_results(eng.decode_threshold(0.3, 0.3, 256), per)
        assert same_results(eng.merge_packed(max_out=256, **opt)[0], want)
        eng.set_rescale(0.0, 0.0)
    eng.close()


@pytest.mark.parametrize("fmt", ("bgr", "nv12"))
def test_state_rules_and_the_consumers_behind_a_packed_merge(fmt):
    eng, dense, places, N = packed_engine(fmt, seed=1)
    h, w = FRAME_HW
    opt = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    views = ops.view_layout(h, w, *NET, scales=(1.0,))

    def estate(call):
        with pytest.raises(cfa._lib.CenterFaceError) as e:
            call()
        assert e.value.code == CF_ESTATE, e.value

    frames, bufs, _, _ = pitched_frames(dense, fmt, 0xFF)
    eng.forward_packed_enqueue(dense, places, N, fmt)
    estate(eng.merge_packed)                                               # without a threshold decode
    eng.decode_threshold(0.3, 0.3, 256)
    estate(eng.merge_views)                                                # it is not a views forward ...
    estate(eng.merge_tiles)                                                # ... nor a tiled ...
    estate(eng.unfit_rows)                                                 # ... nor a fitted one
    estate(lambda: eng.redact_faces(frames, fmt, **opt))                   # a packed forward and a decode, but no merge
    trk = cfa.Tracker(eng, 2, min_hits=1)
    estate(lambda: eng.track_update_device(trk, 0))
    merged, flags = eng.merge_packed(max_out=256)
    counts = np.array([len(d) for d, _ in merged], np.int32)
    assert counts.min() >= 1 and flags.tolist() == [0, 0]
    estate(eng.merge_views)
    estate(eng.merge_tiles)
    estate(eng.unfit_rows)
    # the redaction of the source frames with the merged boxes, which are in frame pixels: (H, W) = (h, w)
    boxes = np.concatenate([d[:, :4] for d, _ in merged])
    wframes, wbufs, _, _ = pitched_frames(dense, fmt, 0xFF)
    redact_ref(wframes, fmt, boxes, counts, (h, w), h, w, **opt)
    assert eng.redact_faces(frames, fmt, **opt) is frames
    assert all(np.array_equal(a, b) for a, b in zip(bufs, wbufs))
    assert not all(np.array_equal(a, b) for a, b in zip(bufs, pitched_frames(dense, fmt, 0xFF)[1]))      # something was redacted
    # the tracker takes the merged rows of Bf frames of (h, w); a second update behind one merge is refused
    dev = eng.device_alloc(8)
    eng.track_update_device(trk, 0, counts_ptr=dev)
    eng.synchronize()
    tc = np.empty(2, np.int32)
    eng.memcpy_d2h(tc, dev)
    eng.device_free(dev)
    assert tc.tolist() == counts.tolist()
    estate(lambda: eng.track_update_device(trk, 0))
    trk.close()
    # any other forward forgets the placements: cf_merge_packed behind a views, a tiled, a fitted and a plain forward
    for forward in (lambda: eng.forward_views_enqueue(dense, views, fmt), lambda: eng.forward_tiles_enqueue(dense, [p[2:6] for p in places[:6]], fmt),
                    lambda: eng.forward_fit_enqueue(dense, fmt), lambda: eng.forward_enqueue(packed_canvases_ref(bgr_of(dense, fmt), places, N, NET)[:2])):
        forward()
        eng.decode_threshold(0.3, 0.3, 256)
        estate(eng.merge_packed)
    # ... and so does an upload
    eng.forward_packed_enqueue(dense, places, N, fmt)
    eng.decode_threshold(0.3, 0.3, 256)
    eng.upload_images(list(packed_canvases_ref(bgr_of(dense, fmt), places, N, NET)[:2]))
    estate(eng.merge_packed)
    eng.close()


# ------------------------------------------------------------------------------------------ the product paths
def engine_sequence(face, frames, fmt, views, per, gutter=0, merge=()):
    """pack_views + forward_packed + decode + merge_packed, chunk by chunk, every chunk packed for its own length: as
    detect_views(pack=True) is to run them."""
    out = []
    for i in range(0, len(frames), per):
        chunk = frames[i:i + per]
        places, N = ops.pack_views(views, len(chunk), NET, gutter)
        face.engine.forward_packed_enqueue(chunk, places, N, fmt)
        face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets)
        out += face.engine.merge_packed(*merge, max_out=face.max_dets)[0]
    return out


def test_centerface_detect_views_packed_and_anonymize():
    """CenterFace.detect_views(pack=True) = pack_views + forward_packed + decode + merge_packed per chunk, the chunk as long as max_batch
    allows and the last one shorter; anonymize(views=dict(pack=True)) changes exactly the bytes redact_ref changes for the merged boxes,
    in BGR and NV12; pack=False is the views path."""
    h, w = FRAME_HW
    face = cfa.CenterFace(NET[0], NET[1], dtype="bf16", max_batch=20)
    views = ops.view_layout(h, w, *NET, **LAYOUT)
    # six tiles and the full level (43 x 32) on canvases of their own per frame, the half levels (22 x 16) share one: two frames per
    # chunk (15 <= 20 < 22) and the third alone
    assert [ops.pack_views(views, n, NET)[1] for n in (1, 2, 3)] == [8, 15, 22]
    rng = np.random.default_rng(2)
    tried = []
    for kind in ("blocks", "binary", "noise", "blocks", "binary", "noise"):  # the default weights answer to one of them
        imgs = source_frames(rng, kind, (3, h, w, 3))
        got = face.detect_views(imgs, pack=True, **LAYOUT)
        tried.append((kind, [len(d) for d, _ in got]))
        if sum(len(d) for d, _ in got) >= 2:
            break
    print("detect_views(pack=True):", tried)
    assert sum(len(d) for d, _ in got) >= 2, tried
    assert all(d.shape[1:] == (5,) and l.shape == (len(d), 10) and d.dtype == np.float32 for d, l in got)
    want = engine_sequence(face, imgs, "bgr", views, 2)
    assert same_results(got, want)
    # levels alone: frames share a canvas, with a gutter; the merge options travel
    small = ops.view_layout(h, w, *NET, scales=(0.5, 0.25))
    assert ops.pack_views(small, 3, NET, 1)[1] == pack_views_ref(small, 3, NET[0], NET[1], 1)[1] < 3
    assert same_results(face.detect_views(imgs, scales=(0.5, 0.25), pack=True, gutter=1), engine_sequence(face, imgs, "bgr", small, 3, 1))
    assert same_results(face.detect_views(imgs, pack=True, metric="iou", thresh=0.3, edge=0.0, **LAYOUT), engine_sequence(face, imgs, "bgr", views, 2, 0, ("iou", 0.3, 0.0)))
    opts = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    keep = imgs.copy()
    out, dets = face.anonymize(list(imgs), views=dict(LAYOUT, pack=True), **opts)
    assert np.array_equal(imgs, keep) and same_results(dets, want)
    ref = keep.copy()
    redact_ref([(f.reshape(h, -1),) for f in ref], "bgr", np.concatenate([d[:, :4] for d, _ in want]), [len(d) for d, _ in want], (h, w), h, w, **opts)
    assert np.array_equal(out, ref) and not np.array_equal(out, keep)
    # NV12 frames of the same size
    yuv = source_frames(np.random.default_rng(3), tried[-1][0], (3, h * 3 // 2, w))
    ywant = engine_sequence(face, yuv, "nv12", views, 2)
    yout, ydets = face.anonymize_yuv(yuv, "nv12", views=dict(LAYOUT, pack=True), **opts)
    assert same_results(ydets, ywant)
    yref = yuv.copy()
    redact_ref([(f[:h], f[h:]) for f in yref], "nv12", np.concatenate([d[:, :4] for d, _ in ywant]), [len(d) for d, _ in ywant], (h, w), h, w, **opts)
    assert np.array_equal(yout, yref)
    # annotate and the chips take the same path
    _, adets = face.annotate(list(imgs), views=dict(LAYOUT, pack=True))
    assert same_results(adets, want)
    rows = face.detect_aligned_frames(imgs, "bgr", 32, views=dict(LAYOUT, pack=True))
    assert same_results([(d, l) for d, l, _ in rows], want) and [len(c) for _, _, c in rows] == [len(d) for d, _ in want]
    # pack=False: every call does what it did
    plain = face.detect_views(imgs, **LAYOUT)
    assert same_results(face.detect_views(imgs, pack=False, **LAYOUT), plain)
    a, b = face.anonymize(list(imgs), views=dict(LAYOUT, pack=False), **opts), face.anonymize(list(imgs), views=LAYOUT, **opts)
    assert a[0].tobytes() == b[0].tobytes() and same_results(a[1], b[1]) and same_results(b[1], plain)
    print("packed vs unpacked rows per frame:", [len(d) for d, _ in want], [len(d) for d, _ in plain])
    # more canvases per frame than max_batch holds
    with pytest.raises(ValueError) as e:
        cfa.CenterFace(NET[0], NET[1], dtype="bf16", max_batch=4).detect_views(imgs, pack=True, **LAYOUT)
    assert "max_batch" in str(e.value)
    face.close()


def test_a_tracker_continues_one_stream_over_two_packed_calls():
    """With a tracker two packed calls continue one stream: the tracks of the first call's merged rows are confirmed by the second's,
    and the redaction of the second call covers the tracked rows."""
    h, w = FRAME_HW
    face = cfa.CenterFace(NET[0], NET[1], dtype="bf16", max_batch=16)
    rng = np.random.default_rng(4)
    upright = lambda res: [int(((d[:, 2] >= d[:, 0]) & (d[:, 3] >= d[:, 1])).sum()) for d, _ in res]      # noqa: E731  (boxes whose IoU with themselves is 1)
    for kind in ("blocks", "binary", "noise", "blocks", "binary", "noise"):
        imgs = source_frames(rng, kind, (2, h, w, 3))
        plain = face.detect_views(imgs, pack=True, **LAYOUT)
        if min(len(d) for d, _ in plain) >= 1 and min(upright(plain)) >= 1:
            break
    assert min(len(d) for d, _ in plain) >= 1
    trk = cfa.Tracker(face.engine, 2, min_hits=2)
    opts = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    ref = imgs.copy()
    redact_ref([(f.reshape(h, -1),) for f in ref], "bgr", np.concatenate([d[:, :4] for d, _ in plain]), [len(d) for d, _ in plain], (h, w), h, w, **opts)
    for call in range(2):
        frames = imgs.copy()
        got = face.detect_views(frames, tracker=trk, redact=opts, pack=True, **LAYOUT)
        assert same_results(got, plain)                                    # the detections returned stay the frame's own
        assert np.array_equal(frames, ref) and not np.array_equal(frames, imgs)      # every track is matched: the tracked rows are the detections
    info = np.zeros((2, trk.max_tracks, 3), np.int32)
    dev = [face.engine.device_alloc(info.nbytes), face.engine.device_alloc(8)]
    places, N = ops.pack_views(ops.view_layout(h, w, *NET, **LAYOUT), 2, NET)
    face.engine.forward_packed_enqueue(imgs, places, N, "bgr")
    face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets)
    face.engine.merge_packed(max_out=face.max_dets)
    face.engine.track_update_device(trk, 0, info_ptr=dev[0], counts_ptr=dev[1])
    face.engine.synchronize()
    tc = np.empty(2, np.int32)
    face.engine.memcpy_d2h(info, dev[0])
    face.engine.memcpy_d2h(tc, dev[1])
    for p in dev:
        face.engine.device_free(p)
    # the same frames three times: a row whose box matches itself (x2 >= x1 and y2 >= y1: IoU 1) is the third hit of the track the first
    # call started; the synthetic weights also give turned boxes, which are born anew each time (tests/test_views.py explains) and whose
    # tentative track of the call before is freed, so the counts stay those of the detections and no row stands at two hits
    hits = [info[b, :tc[b], 1] for b in range(2)]
    print("hits per tracked row:", [np.bincount(x, minlength=4).tolist() for x in hits], "boxes that match themselves:", upright(plain))
    assert tc.tolist() == [len(d) for d, _ in plain] and all(set(x.tolist()) <= {1, 3} for x in hits)
    assert all(int((x == 3).sum()) >= n for x, n in zip(hits, upright(plain))) and sum(int((x == 3).sum()) for x in hits) >= 1
    trk.close()
    face.close()


def test_demo_pack(tmp_path, capsys):
    """``demo --scales 1,0.5,0.25 --tiled 64 --pack --gutter 2 --anonymize OUT`` writes its file: the bytes of
    ``CenterFace.anonymize(views=dict(pack=True, gutter=2))`` on the decoded file, through a context of as many canvases as the packer
    says."""
    from PIL import Image
    from centerface_amd import demo
    frame = source_frames(np.random.default_rng(8), "blocks", (1, 72, 96, 3))[0]
    path, out = str(tmp_path / "in.png"), str(tmp_path / "out.png")
    Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(path)
    views = dict(scales=(1.0, 0.5, 0.25), tile=64, pack=True, gutter=2)
    table = ops.view_layout(72, 96, 64, 64, scales=views["scales"], tile=64)
    N = ops.pack_views(table, 1, (64, 64), 2)[1]
    assert N < len(table)
    face = cfa.CenterFace(64, 64, dtype="bf16", max_batch=N)
    black, res = face.anonymize([demo.imread(path)], views=views, mode="solid", shape="rect")      # the command line has no --fill
    plain, _ = face.detect_views(demo.imread(path)[None], **views)[0]
    face.close()
    capsys.readouterr()
    demo.main([path, "--scales", "1,0.5,0.25", "--tiled", "64", "--pack", "--gutter", "2", "--anonymize", out, "--mode", "solid", "--shape", "rect"])
    assert capsys.readouterr().out == demo.format_wider_result(path, res[0][0])
    assert np.array_equal(demo.imread(out), black[0])
    demo.main([path, "--scales", "1,0.5,0.25", "--tiled", "64", "--pack", "--gutter", "2"])      # the detections alone
    assert capsys.readouterr().out == demo.format_wider_result(path, plain)
    dets, _ = demo.anonymize_file(path, str(tmp_path / "third.png"), scales=(1.0, 0.5, 0.25), tiled=64, pack=True, gutter=2, mode="solid", shape="rect")
    assert dets.tobytes() == res[0][0].tobytes() and np.array_equal(demo.imread(str(tmp_path / "third.png")), black[0])
