"""Multi-scale detection on the GPU: the views cutter (cf_op_views, cf_forward_views), the merge (cf_op_merge_views, cf_merge_views), the
state rules and the product paths behind them, every byte against the restatements of tests/view_cases.py (canvas = the restated tile
cut of each view's source rectangle pasted into a filled canvas; merge = three drop rules + float64 map + the NMS restatement),
tests/test_yuv_input.py and tests/test_redact.py."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from fit_cases import fit_geometry_ref
from test_redact import redact_ref, source_frames
from test_tiles import FILL, bgr_of, net_tables, pitched_frames, same_results, table
from view_cases import canvases_ref, merge_views_ref, view_layout_ref

pytestmark = pytest.mark.gpu

FORMATS = ("bgr", "nv12", "nv21", "i420", "yv12")
NET = (32, 64)                  # (H, W) of every context and canvas here
FILL_BGR = (1, 2, 3)
CF_ESTATE = cfa._lib.CF_ESTATE


# ------------------------------------------------------------------------------------------ the cutter
def views_for(h, w):
    """The views of one frame size in a (32, 64) canvas; the comments say what each is there for."""
    H, W = NET
    rw, rh, dx, dy = fit_geometry_ref(h, w, H, W)
    half, quarter = view_layout_ref(h, w, H, W, scales_pm=(500, 250))
    v = [(0, 0, 40, 30, 0, 0, W, H),                     # 0: a tile view
         (w - 36, h - 26, 36, 26, 0, 0, W, H),           # 1: a tile view whose source ends at the far corner
         (10, 20, 24, 16, 5, 7, 24, 16),                 # 2: identity: the source of exactly the content's size
         (0, 0, w, h, dx, dy, rw, rh),                   # 3: the fit view
         half, quarter,                                  # 4, 5: the half and the quarter level
         (0, 0, w, h, W - 1, H - 1, 1, 1),               # 6: a content of 1 x 1, in the canvas's last lane and row
         (0, 0, w, h, 17, 0, 1, H),                      # 7: 1 column x full height
         (44, 36, 2, 2, 8, 4, 40, 20),                   # 8: a 2 x 2 source enlarged
         (w - 30, h - 22, 30, 22, 33, 9, 21, 13),        # 9: a source ending at the far corner, content odd everywhere
         (6, 8, 18, 20, 5, 30, 2, 2)]                    # 10: a content inside one lane, in the last rows (upscale taps, then fill)
    for a in range(4):                                   # 11 .. 14: dx and dx + dw at every residue mod 4
        v.append((2 * a, 4, 50, 40, 4 + a, 3 + a, 20 + (a + 1) % 4 - a, 9))
    assert sorted((x[4] % 4, (x[4] + x[6]) % 4) for x in v[11:]) == [(0, 1), (1, 2), (2, 3), (3, 0)]
    return [tuple(int(k) for k in x) for x in v]


_cut_cache = {}


def cut_case(fmt, hw):
    """(dense frames, their BGR restatement, the views, the reference canvases) of one format and frame size, Bf = 2, computed once."""
    if (fmt, hw) not in _cut_cache:
        rng = np.random.default_rng(FORMATS.index(fmt) * 13 + hw[0])
        h, w = hw
        dense = rng.integers(0, 256, (2, h, w, 3) if fmt == "bgr" else (2, h * 3 // 2, w), dtype=np.uint8)
        bgr = bgr_of(dense, fmt)
        _cut_cache[(fmt, hw)] = (dense, bgr, views_for(h, w), canvases_ref(bgr, views_for(h, w), NET, FILL_BGR))
    return _cut_cache[(fmt, hw)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_op_views_bit_exact(fmt):
    """Bf = 2 frames of 70 x 94 and 72 x 96, fifteen views, (H, W) = (32, 64), fill (1, 2, 3), rows with padding: every byte equals the
    restatement, whether the padding and the bytes behind every plane hold 0xFF or 0x00; a dense block too."""
    for hw in ((70, 94), (72, 96)):
        dense, bgr, views, want = cut_case(fmt, hw)
        for pad in (0xFF, 0x00):
            frames, bufs, _, _ = pitched_frames(dense, fmt, pad)
            got = ops.cut_views(frames, views, NET, fmt, fill=FILL_BGR)
            assert got.shape == want.shape == (2, len(views)) + NET + (3,)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (fmt, hw, pad, len(bad), bad[:4].tolist())
        assert np.array_equal(ops.cut_views(dense, views, NET, fmt, fill=FILL_BGR), want)         # dense frames
        # the identity view reproduces the source bytes; the padding is the fill, to the byte beside the content
        assert np.array_equal(want[:, 2, 7:23, 5:29], bgr[:, 20:36, 10:34])
        assert (want[:, 2, :7] == FILL_BGR).all() and (want[:, 2, 7:23, 29:] == FILL_BGR).all() and (want[:, 2, 7:23, :5] == FILL_BGR).all()
        assert (want[:, 6, :31] == FILL_BGR).all() and (want[:, 6, 31, :63] == FILL_BGR).all()
        # the tile views are the tile cutter's images, the fit view is the fit's canvas
        got = ops.cut_views(dense, views, NET, fmt, fill=FILL_BGR)
        tiles = ops.cut_tiles(dense, [v[:4] for v in views[:2]], NET, fmt)
        assert np.array_equal(got[:, :2], tiles), (fmt, hw)
        assert np.array_equal(got[:, 3], ops.fit_frames(dense, NET, fmt, fill=FILL_BGR)), (fmt, hw)
        # another fill reaches every padding byte and no content byte
        black = ops.cut_views(dense, views, NET, fmt)
        assert np.array_equal(black, canvases_ref(bgr, views, NET))


def test_op_views_odd_sized_content_of_bgr_frames():
    """BGR frames of 70 x 94: the levels of a top-left layout and one of every anchor, whose contents have odd sides and odd origins."""
    dense, bgr, _, _ = cut_case("bgr", (70, 94))
    for anchor in ("center", "topleft"):
        views = ops.view_layout(70, 94, *NET, scales=(1.0, 0.77, 0.5, 0.33, 0.03), anchor=anchor)
        assert views.tolist() == [list(v) for v in view_layout_ref(70, 94, *NET, anchor=anchor, scales_pm=(1000, 770, 500, 330, 30))]
        frames, _, _, _ = pitched_frames(dense, "bgr", 0xFF)
        got, want = ops.cut_views(frames, views, NET, "bgr", fill=FILL_BGR), canvases_ref(bgr, views, NET, FILL_BGR)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (anchor, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("fmt", ("yv12", "bgr"))
def test_op_views_more_frames_than_one_launch(fmt):
    """Bf = 65 frames of 8 x 8 (one launch takes 64), two views, (H, W) = (4, 8), rows with padding: frame 64 is the second launch's only
    frame -- its planes (YV12: swapped) at table entry 0, its canvases behind those of the 64 before it."""
    rng = np.random.default_rng(90 + FORMATS.index(fmt))
    dense = rng.integers(0, 256, (65, 8, 8, 3) if fmt == "bgr" else (65, 12, 8), dtype=np.uint8)
    views = [(0, 2, 8, 4, 0, 0, 8, 4), (2, 0, 6, 8, 3, 1, 4, 3)]
    want = canvases_ref(bgr_of(dense, fmt), views, (4, 8), FILL_BGR)
    frames, _, _, _ = pitched_frames(dense, fmt, 0xFF)
    got = ops.cut_views(frames, views, (4, 8), fmt, fill=FILL_BGR)
    assert got.shape == want.shape == (65, 2, 4, 8, 3)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (fmt, len(bad), bad[:4].tolist())


# ------------------------------------------------------------------------------------------ the context's forward
@pytest.mark.parametrize("fmt", FORMATS)
def test_engine_forward_views_writes_the_restated_canvases(fmt):
    """cf_forward_views, host-staged (padded rows, and one dense block) and in place on device planes: cf_get_resized_input returns the
    restated canvases, image f * V + v = view v of frame f; the planes are untouched; the refusals that need a context."""
    hw = (72, 96)
    dense, bgr, views, want = cut_case(fmt, hw)
    V = len(views)
    eng = cfa.Engine(NET[0], NET[1], max_batch=2 * V, dtype="bf16")
    frames, bufs, p0, p1 = pitched_frames(dense, fmt, 0xFF)
    for src in (frames, dense):
        eng.forward_views_enqueue(src, views, fmt, fill=FILL_BGR)
        got = eng.resized_input()
        assert eng.last_B == 2 * V and got.shape == (2 * V,) + NET + (3,) and np.array_equal(got.reshape(want.shape), want), fmt
    for pad in (0xFF, 0x00):
        frames, bufs, p0, p1 = pitched_frames(dense, fmt, pad, aligned=True)
        dev = [eng.device_alloc(b.nbytes) for b in bufs]
        for d, b in zip(dev, bufs):
            eng.memcpy_h2d(d, b)
        n = len(frames[0])
        planes = [tuple(dev[b * n:(b + 1) * n]) for b in range(2)]
        eng.forward_views_enqueue(planes, views, fmt, fill=FILL_BGR, on_device=True, h=hw[0], w=hw[1], pitch0=p0, pitch1=p1)
        assert np.array_equal(eng.resized_input().reshape(want.shape), want), (fmt, pad)
        for d, b in zip(dev, bufs):                                                  # read in place: the planes are untouched
            back = np.empty_like(b)
            eng.memcpy_d2h(back, d)
            assert np.array_equal(back, b)
        with pytest.raises(ValueError):                                              # a misaligned device plane
            eng.forward_views_enqueue([(planes[0][0] + 2,) + planes[0][1:]] + planes[1:], views, fmt, on_device=True, h=hw[0], w=hw[1], pitch0=p0, pitch1=p1)
        for d in dev:
            eng.device_free(d)
    # refusals name the view and leave the engine working; the content must lie inside THIS canvas; Bf * V must fit max_batch
    with pytest.raises(ValueError) as e:
        eng.forward_views_enqueue(dense, views[:3] + [(0, 0, 96, 72, 1, 0, 64, 32)], fmt)
    assert "view 3 " in str(e.value) and "canvas" in str(e.value)
    with pytest.raises(ValueError) as e:
        eng.forward_views_enqueue(dense, views[:2] + [(2, 2, 96, 8, 0, 0, 64, 32)], fmt)
    assert "view 2 " in str(e.value) and "frame" in str(e.value)
    with pytest.raises(ValueError) as e:
        eng.forward_views_enqueue(dense, views + views[:1], fmt)
    assert "max_batch" in str(e.value) and "%d x %d" % (2, V + 1) in str(e.value)
    eng.forward_views_enqueue(dense, views, fmt, fill=FILL_BGR)
    assert np.array_equal(eng.resized_input().reshape(want.shape), want)
    eng.close()


def test_engine_forward_views_under_the_flip_test():
    """With the flip test on the views batch is followed by its mirror (whole pixels reversed per row), and Bf * V must fit half the
    context: as the tiled forward behaves."""
    dense, bgr, views, want = cut_case("nv12", (72, 96))
    views, want = views[:5], want[:, :5]
    eng = cfa.Engine(NET[0], NET[1], max_batch=10, dtype="bf16", flip_test=True)
    eng.forward_views_enqueue(dense, views, "nv12", fill=FILL_BGR)
    assert eng.last_B == 10
    both = np.empty((20,) + NET + (3,), np.uint8)
    eng._chk(eng._L.cf_get_resized_input(eng._h, cfa._lib.ptr(both), 20))
    assert np.array_equal(both[:10].reshape(want.shape), want)
    assert np.array_equal(both[10:], both[:10, :, ::-1])                    # the second half is the mirror
    with pytest.raises(ValueError) as e:
        eng.forward_views_enqueue(dense, views + views[:1], "nv12")
    assert "flip test" in str(e.value)
    eng.close()


# ------------------------------------------------------------------------------------------ the merge on hand-built tables
def check_merge(views, frame_hw, net_hw, d, s, l, counts, max_out, **opt):
    """ops.merge_views against merge_views_ref, bit for bit: counts, flags, the rows below min(count, max_out), and the caller's bytes in
    every row behind them."""
    d, s, l = (np.asarray(a, np.float32) for a in (d, s, l))
    Bf = d.shape[0]
    od, ol = np.full((Bf, max_out, 5), FILL), np.full((Bf, max_out, 10), FILL)
    gd, gl, gc, gf = ops.merge_views(views, frame_hw, net_hw, d, s, l, counts, max_out, dets=od, lms=ol, **opt)
    want, wflags = merge_views_ref(views, frame_hw, d, s, l, counts, **opt)
    assert gc.tolist() == [len(w[0]) for w in want], (gc, [len(w[0]) for w in want])
    assert gf.tolist() == wflags.tolist()
    for f, (wd, wl) in enumerate(want):
        m = min(len(wd), max_out)
        assert gd[f, :m].tobytes() == wd[:m].tobytes(), (f, gd[f, :m], wd[:m])
        assert gl[f, :m].tobytes() == wl[:m].tobytes(), f
        assert (gd[f, m:] == FILL).all() and (gl[f, m:] == FILL).all(), f
    return want, gc, gf


CONTENT = (4, 6, 40, 30)                                 # dx, dy, dw, dh: x in [4, 44), y in [6, 36) of a 64 x 64 canvas
INNER = [(32, 32, 64, 64) + CONTENT]                     # every source side interior in a 128 x 128 frame
LOW = [(0, 0, 64, 64) + CONTENT]                         # its left and top sides on the frame border
HIGH = [(64, 64, 64, 64) + CONTENT]                      # its right and bottom sides on the frame border
# a 64 x 96 frame in a 64 x 64 canvas: two tiles (the right side of 0 and the left side of 1 are interior), the fitted frame, its half
TILES = [(0, 0, 64, 64, 0, 0, 64, 64), (32, 0, 64, 64, 0, 0, 64, 64)]
LEVELS = [(0, 0, 96, 64, 0, 10, 64, 43), (0, 0, 96, 64, 16, 21, 32, 22)]


def test_merge_views_edge_rule_per_side():
    """Each of the four edge compares, against the CONTENT's sides (dx = 4, dy = 6: not the canvas's), on an interior source side and on
    a frame-border one; the value exactly on the limit is kept."""
    assert [list(v) for v in LEVELS] == ops.view_layout(64, 96, 64, 64, scales=(1.0, 0.5)).tolist()
    frame, net = (128, 128), (64, 64)
    sides = [((5.5, 12, 20, 30, 0.7), LOW), ((10, 7.5, 20, 30, 0.7), LOW), ((10, 12, 42.5, 30, 0.7), HIGH), ((10, 12, 20, 34.5, 0.7), HIGH)]
    for bx, border in sides:
        d, s, l, c = table(1, 1, 2, {(0, 0): [bx]})
        assert check_merge(INNER, frame, net, d, s, l, c, 2, edge=2.0)[1].tolist() == [0], bx       # within 2 of an interior side
        assert check_merge(INNER, frame, net, d, s, l, c, 2, edge=1.0)[1].tolist() == [1], bx       # ... but not within 1
        assert check_merge(INNER, frame, net, d, s, l, c, 2, edge=0.0)[1].tolist() == [1], bx
        assert check_merge(border, frame, net, d, s, l, c, 2, edge=2.0)[1].tolist() == [1], bx      # that side is the frame's: no rule
    for bx, border in sides[:2]:                                               # ... and the opposite pair of sides still has it
        d, s, l, c = table(1, 1, 2, {(0, 0): [bx]})
        assert check_merge(HIGH, frame, net, d, s, l, c, 2, edge=2.0)[1].tolist() == [0], bx
    # exactly on the limits: x1 = dx + edge, y1 = dy + edge, x2 = dx + dw - edge, y2 = dy + dh - edge are kept, one float32 step past is not
    d, s, l, c = table(1, 1, 2, {(0, 0): [(6, 8, 42, 34, 0.7)]})
    want, gc, _ = check_merge(INNER, frame, net, d, s, l, c, 2, edge=2.0)
    assert gc.tolist() == [1]
    sx, sy = 64 / 40, 64 / 30
    assert want[0][0][0].tolist() == [np.float32(2 * sx + 32), np.float32(2 * sy + 32), np.float32(38 * sx + 32), np.float32(28 * sy + 32), np.float32(0.7)]
    for k, step in ((0, -1), (1, -1), (2, 1), (3, 1)):
        d2 = d.copy()
        d2[0, 0, 0, k] = np.nextafter(d[0, 0, 0, k], np.float32(step * 1e9))
        assert check_merge(INNER, frame, net, d2, s, l, c, 2, edge=2.0)[1].tolist() == [0], k
    # a whole-frame level has no interior side: a box that touches its content's sides stays
    d, s, l, c = table(1, 2, 2, {(0, 1): [(16, 21, 48, 43, 0.7)]})
    assert check_merge(LEVELS, (64, 96), net, d, s, l, c, 2, edge=5.0)[1].tolist() == [1]


def test_merge_views_centre_rule_non_finite_corners_and_flags():
    frame, net = (64, 96), (64, 64)
    half = LEVELS[1:]                                                         # content x in [16, 48), y in [21, 43)
    kept = [(14, 25, 18, 27, 0.9), (20, 19, 24, 23, 0.8), (45, 40, 50, 45.5, 0.7)]      # cx = 16; cy = 21; just inside the far corner
    gone = [(46, 25, 50, 27, 0.9), (20, 41, 24, 45, 0.9), (10, 25, 14, 27, 0.9), (50, 25, 54, 27, 0.9), (20, 15, 24, 19, 0.9), (20, 45, 24, 49, 0.9)]
    for bx in kept + gone:                                                    # cx = 48; cy = 43; left, right, above, below
        d, s, l, c = table(1, 1, 2, {(0, 0): [bx]})
        assert check_merge(half, frame, net, d, s, l, c, 2)[1].tolist() == [1 if bx in kept else 0], bx
    # mapped with the content's origin and the level's scale: (x - 16) * 3, (y - 21) * (64 / 22)
    d, s, l, c = table(1, 1, 2, {(0, 0): [(20, 25, 30, 32, 0.6)]})
    want, _, _ = check_merge(half, frame, net, d, s, l, c, 2)
    assert want[0][0][0].tolist() == [12, np.float32(4 * (64 / 22)), 42, np.float32(11 * (64 / 22)), np.float32(0.6)]
    assert want[0][1][0, 0] == np.float32((3 - 16) * 3.0) and want[0][1][0, 1] == np.float32((7 - 21) * (64 / 22))
    # a centre in the padding of a level is no face, whatever its score; the same box in a tile is one
    d, s, l, c = table(1, 3, 2, {(0, 0): [(2, 2, 12, 12, 0.5)], (0, 2): [(2, 2, 12, 12, 0.99)]})
    want, gc, _ = check_merge(TILES[:1] + LEVELS, frame, net, d, s, l, c, 4)
    assert gc.tolist() == [1] and want[0][0][0].tolist() == [2, 2, 12, 12, 0.5]
    # a non-finite corner is dropped
    d, s, l, c = table(1, 2, 4, {(0, 0): [(np.nan, 10, 30, 30, 0.9), (10, 10, 30, 30, 0.5), (10, 10, np.inf, 30, 0.95)], (0, 1): [(30, 40, 50, -np.inf, 0.9)]})
    assert check_merge(TILES, frame, net, d, s, l, c, 4)[1].tolist() == [1]
    # a view image with counts > rows sets bit 0 of its frame's flag, only there; its rows below `rows` are merged
    d, s, l, c = table(2, 2, 3, {(0, 0): [(10, 10, 30, 30, 0.9)], (1, 1): [(20, 25, 24, 29, 0.5), (26, 25, 30, 29, 0.6), (32, 25, 36, 29, 0.7)]})
    c[1, 1] = 5
    _, gc, gf = check_merge(TILES[:1] + LEVELS[1:], frame, net, d, s, l, c, 4)
    assert gc.tolist() == [1, 3] and gf.tolist() == [0, 1]


def test_merge_views_negative_zero_and_a_centre_outside_the_canvas():
    """Unturned: a -0.0 corner and a -0.0 landmark of a view whose content starts at the canvas's origin map as
    float32((float64(-0.0) - 0) * sx + sx0) = +0.0, bit for bit; a row whose centre lies left of the canvas is dropped by the centre
    rule (the tile merge, which has none, keeps that row)."""
    frame, net = (64, 96), (64, 64)
    d, s, l, c = table(1, 2, 4, {(0, 0): [(-0.0, -0.0, 8, 6, 0.7), (-40, 10, 10, 30, 0.9)]})
    l[0, 0, 0, :2] = -0.0
    want, gc, _ = check_merge(TILES, frame, net, d, s, l, c, 4)
    assert gc.tolist() == [1] and want[0][0][0].tolist() == [0, 0, 8, 6, np.float32(0.7)]
    assert not np.signbit(want[0][0][0, :2]).any() and not np.signbit(want[0][1][0, :2]).any()


def test_merge_views_across_scales_ties_and_truncation():
    frame, net = (64, 96), (64, 64)
    views = TILES[:1] + LEVELS[1:]
    # a small box from the tile inside a large one from the half level: frame (10, 10, 30, 30) inside (6, 2.9, 60, 59.6)
    d, s, l, c = table(1, 2, 3, {(0, 0): [(10, 10, 30, 30, 0.8)], (0, 1): [(18, 22, 36, 41.5, 0.9)]})
    want, gc, _ = check_merge(views, frame, net, d, s, l, c, 4, metric="iou", thresh=0.5)
    assert gc.tolist() == [2] and want[0][0][0, :4].tolist() == [6, np.float32(64 / 22), 60, np.float32(20.5 * (64 / 22))]      # IoU 0.14: both stay
    want, gc, _ = check_merge(views, frame, net, d, s, l, c, 4, metric="ios", thresh=0.5)
    assert gc.tolist() == [1] and want[0][0][0, 4] == np.float32(0.9)            # IoS 1: the part goes
    s[0, 0, 0] = 0.95                                                            # the higher score survives, whichever view it is from
    want, gc, _ = check_merge(views, frame, net, d, s, l, c, 4, metric="ios", thresh=0.5)
    assert gc.tolist() == [1] and want[0][0][0].tolist() == [10, 10, 30, 30, np.float32(0.95)]
    # the same face seen by both tiles with equal scores: the higher candidate index (the later view) first
    d, s, l, c = table(1, 2, 4, {(0, 0): [(40, 10, 60, 30, 0.9)], (0, 1): [(8, 10, 28, 30, 0.9)]})
    want, gc, _ = check_merge(TILES, frame, net, d, s, l, c, 4)
    assert gc.tolist() == [1] and want[0][1][0, 0] == l[0, 1, 0, 0] + 32
    # more survivors than max_out: only max_out rows are written, the count tells; the rows of the next (empty) frame stay as they were
    five = [(4 + 11 * k, 10, 12 + 11 * k, 20, 0.5 + 0.05 * k) for k in range(5)]
    d, s, l, c = table(2, 2, 5, {(0, 0): five})
    want, gc, _ = check_merge(TILES, frame, net, d, s, l, c, 2)
    assert gc.tolist() == [5, 0] and want[0][0][0, 4] == np.float32(0.7)


def random_table(rng, views, Bf, rows, net):
    """Boxes around every view's content (most centres inside, some in the padding), many score ties."""
    V = len(views)
    d = np.zeros((Bf, V, rows, 4), np.float32)
    for v, (_, _, _, _, dx, dy, dw, dh) in enumerate(views):
        c = np.stack([rng.uniform(dx - 3, dx + dw + 3, (Bf, rows)), rng.uniform(dy - 3, dy + dh + 3, (Bf, rows))], -1)
        half = rng.uniform(0.5, 0.2 * max(dw, dh) + 1, (Bf, rows, 2))
        d[:, v] = np.concatenate([c - half, c + half], -1)
    s = rng.choice(np.linspace(0.3, 0.95, 40).astype(np.float32), (Bf, V, rows))
    l = rng.uniform(-4, max(net) + 4, (Bf, V, rows, 10)).astype(np.float32)
    return d, s, l


def test_merge_views_random_tables_cross_the_1024_wide_round():
    """V = 5 views x 256 rows = 1280 (view, row) items a frame: the collect's 1024-wide round runs twice, and the candidates pass the 64-
    and 256-candidate boundaries of the rank / mask / sweep kernels.  Bf = 3 with different counts per view, an empty view, a truncated
    view, a NaN; a third frame without any row."""
    rng = np.random.default_rng(5)
    frame, net, rows = (64, 96), (64, 64), 256
    views = TILES + LEVELS + [(30, 20, 40, 30, 7, 5, 51, 39)]
    d, s, l = random_table(rng, views, 3, rows, net)
    c = np.zeros((3, 5), np.int32)
    c[0] = [rows, 0, rows - 7, 31, rows]
    c[1] = [rows + 9, rows, 1, rows, 64]
    d[1, 1, 5, 2] = np.nan
    for metric, thr, edge in (("ios", 0.5, 2.0), ("iou", 0.3, 0.0), ("ios", 0.9, 5.0)):
        want, gc, gf = check_merge(views, frame, net, d, s, l, c, 5 * rows, metric=metric, thresh=thr, edge=edge)
        assert gc[2] == 0 and gf.tolist() == [0, 1, 0] and gc[0] > 8 and gc[1] > 8
    check_merge(views, frame, net, d, s, l, c, 7, metric="iou", thresh=0.3, edge=0.0)             # truncated outputs


def test_merge_views_of_a_pure_tile_layout_is_the_tile_merge():
    """Tile views and rows whose centres lie in the canvas: dets, landmarks, counts and flags of ops.merge_views are those of
    ops.merge_tiles, bit for bit."""
    rng = np.random.default_rng(6)
    frame, net, rows = (128, 160), (64, 64), 60
    rects = [(0, 0, 64, 64), (48, 0, 64, 64), (96, 0, 64, 64), (0, 64, 64, 64), (0, 0, 160, 128)]
    views = [r + (0, 0, 64, 64) for r in rects]
    xy = rng.uniform(0, 56, (2, 5, rows, 2)).astype(np.float32)
    wh = rng.uniform(2, 24, (2, 5, rows, 2)).astype(np.float32)
    d = np.minimum(np.concatenate([xy, xy + wh], -1), np.float32(64))
    s = rng.choice(np.linspace(0.3, 0.95, 40).astype(np.float32), (2, 5, rows))
    l = rng.uniform(0, 64, (2, 5, rows, 10)).astype(np.float32)
    c = np.array([[rows, 0, rows - 7, 31, rows], [rows + 9, rows, 1, rows, 40]], np.int32)
    cx, cy = (d[..., 0] + d[..., 2]) * np.float32(0.5), (d[..., 1] + d[..., 3]) * np.float32(0.5)
    assert (cx >= 0).all() and (cx < 64).all() and (cy >= 0).all() and (cy < 64).all()
    for opt in (dict(metric="ios", thresh=0.5, edge=2.0), dict(metric="iou", thresh=0.3, edge=0.0)):
        a = ops.merge_views(views, frame, net, d, s, l, c, 5 * rows, **opt)
        b = ops.merge_tiles(rects, frame, net, d, s, l, c, 5 * rows, **opt)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), opt
        assert a[2].min() > 8 and a[3].tolist() == [0, 1]


# ------------------------------------------------------------------------------------------ the context's merge and the state rules
FRAME_HW = (72, 96)
LAYOUT = dict(tile=(32, 64), overlap=8, scales=(1.0, 0.5))


def views_engine(fmt="bgr", seed=0, need=3):
    """A 32 x 64 context with the default (synthetic) weights and two 72 x 96 frames whose views forward (3 x 2 tiles + two levels, V = 8)
    keeps, at 0.3, rows in both frames after the merge and more at 0.1: (engine, dense frames, the views).  The default weights answer
    to one of the source kinds."""
    h, w = FRAME_HW
    views = ops.view_layout(h, w, *NET, **LAYOUT)
    assert len(views) == 8 and views.tolist() == [list(v) for v in view_layout_ref(h, w, *NET, 32, 64, 8, "center", (1000, 500))]
    eng = cfa.Engine(NET[0], NET[1], max_batch=2 * len(views), dtype="bf16")
    tried = []
    for k, kind in enumerate(("blocks", "binary", "noise") * 3):
        dense = source_frames(np.random.default_rng(seed + 10 * k), kind, (2, h, w, 3) if fmt == "bgr" else (2, h * 3 // 2, w))
        eng.forward_views_enqueue(dense, views, fmt)
        n = []
        for thr in (0.3, 0.1):
            eng.decode_threshold(thr, 0.3, 256)
            n.append([len(d) for d, _ in eng.merge_views(max_out=1024)[0]])
        tried.append((kind, n))
        if min(n[0]) >= 1 and sum(n[0]) >= need and sum(n[1]) > sum(n[0]):
            print("views_engine:", tried)
            return eng, dense, views
    raise AssertionError(tried)


def test_engine_views_decode_and_merge_equal_the_restatement():
    eng, dense, views = views_engine()
    V = len(views)
    canv = canvases_ref(dense, views, NET).reshape((2 * V,) + NET + (3,))
    assert np.array_equal(eng.resized_input(), canv)
    per = eng.decode_threshold(0.3, 0.3, 256)
    # the per-view results are those of the restated canvases fed as an ordinary uint8 batch
    eng.forward_enqueue(canv)
    assert same_results(eng.decode_threshold(0.3, 0.3, 256), per)
    with pytest.raises(cfa._lib.CenterFaceError) as e:                     # ... behind which there is nothing to merge
        eng.merge_views()
    assert e.value.code == CF_ESTATE
    d, s, l, c = net_tables(per, 2, V)
    for opt in (dict(metric="ios", thresh=0.5, edge=2.0), dict(metric="iou", thresh=0.3, edge=0.0)):
        want, wflags = merge_views_ref(views, FRAME_HW, d, s, l, c, **opt)
        eng.forward_views_enqueue(dense, views, "bgr")
        with pytest.raises(cfa._lib.CenterFaceError) as e:                 # before a decode
            eng.merge_views(**opt)
        assert e.value.code == CF_ESTATE
        assert same_results(eng.decode_threshold(0.3, 0.3, 256), per)
        got, flags = eng.merge_views(max_out=256, **opt)
        print("merged per frame:", [len(x) for x, _ in got], "of", c.sum(1).tolist())
        assert same_results(got, want) and flags.tolist() == wflags.tolist() == [0, 0]
        assert same_results(eng.merge_views(max_out=1, **opt)[0], want)    # truncated host form: the wrapper comes back for all of them
        mo = 64                                                            # the device form, read back; every output may be NULL
        bufs = [eng.device_alloc(2 * mo * 5 * 4), eng.device_alloc(2 * mo * 10 * 4), eng.device_alloc(8), eng.device_alloc(8)]
        eng.merge_views_device(mo, *bufs, **opt)
        eng.synchronize()
        hd, hl, hc, hf = np.empty((2, mo, 5), np.float32), np.empty((2, mo, 10), np.float32), np.empty(2, np.int32), np.empty(2, np.int32)
        for a, b in zip((hd, hl, hc, hf), bufs):
            eng.memcpy_d2h(a, b)
            eng.device_free(b)
        assert hc.tolist() == [len(x) for x, _ in want] and hf.tolist() == [0, 0]
        assert same_results([(hd[f, :min(hc[f], mo)], hl[f, :min(hc[f], mo)]) for f in range(2)], [(x[:mo], y[:mo]) for x, y in want])
        eng.merge_views_device(mo, **opt)
        eng.set_rescale(1.37, 1.21)                                        # cf_set_rescale changes the decode's own rows, not the merge
        assert not same_results(eng.decode_threshold(0.3, 0.3, 256), per)
        assert same_results(eng.merge_views(max_out=256, **opt)[0], want)
        eng.set_rescale(0.0, 0.0)
    # rows decoded at 0.1 and filtered at > 0.3 equal the merge of a decode at 0.3: no stage is cut (counts below every max_out, flags 0)
    eng.forward_views_enqueue(dense, views, "bgr")
    assert max(len(x) for x, _ in eng.decode_threshold(0.3, 0.3, 256)) < 256
    strong, f3 = eng.merge_views(max_out=1024)
    weak_per = eng.decode_threshold(0.1, 0.3, 256)
    assert max(len(x) for x, _ in weak_per) < 256
    weak, f1 = eng.merge_views(max_out=1024)
    assert not f3.any() and not f1.any() and sum(len(x) for x, _ in weak) > sum(len(x) for x, _ in strong)
    assert same_results([(x[x[:, 4] > np.float32(0.3)], y[x[:, 4] > np.float32(0.3)]) for x, y in weak], strong)
    eng.close()


@pytest.mark.parametrize("fmt", ("bgr", "nv12"))
def test_state_rules_and_the_consumers_behind_a_views_merge(fmt):
    eng, dense, views = views_engine(fmt, seed=1)
    h, w = FRAME_HW
    opt = dict(mode="solid", shape="rect", fill=(1, 2, 3))

    def estate(call):
        with pytest.raises(cfa._lib.CenterFaceError) as e:
            call()
        assert e.value.code == CF_ESTATE, e.value

    frames, bufs, _, _ = pitched_frames(dense, fmt, 0xFF)
    eng.forward_views_enqueue(dense, views, fmt)
    estate(eng.merge_views)                                                # without a threshold decode
    eng.decode_threshold(0.3, 0.3, 256)
    estate(eng.merge_tiles)                                                # it is not a tiled forward ...
    estate(eng.unfit_rows)                                                 # ... nor a fitted one
    estate(lambda: eng.redact_faces(frames, fmt, **opt))                   # a views forward and a decode, but no merge
    trk = cfa.Tracker(eng, 2, min_hits=1)
    estate(lambda: eng.track_update_device(trk, 0))
    merged, flags = eng.merge_views(max_out=256)
    counts = np.array([len(d) for d, _ in merged], np.int32)
    assert counts.min() >= 1 and flags.tolist() == [0, 0]
    estate(eng.merge_tiles)
    estate(eng.unfit_rows)
    # the redaction of the source frames with the merged boxes, which are in frame pixels: (H, W) = (h, w)
    boxes = np.concatenate([d[:, :4] for d, _ in merged])
    wframes, wbufs, _, _ = pitched_frames(dense, fmt, 0xFF)
    redact_ref(wframes, fmt, boxes, counts, (h, w), h, w, **opt)
    assert eng.redact_faces(frames, fmt, **opt) is frames
    assert all(np.array_equal(a, b) for a, b in zip(bufs, wbufs))
    assert not all(np.array_equal(a, b) for a, b in zip(bufs, pitched_frames(dense, fmt, 0xFF)[1]))      # something was redacted
    with pytest.raises(ValueError):                                        # the wrong B is refused
        eng.redact_faces([frames[0]], fmt, **opt)
    chips, offs, _ = eng.align_faces_frame(dense, fmt, 32)                 # one chip per merged row, cut from the frames
    assert np.diff(offs).tolist() == counts.tolist()
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
    # any other forward forgets the views: cf_merge_views behind a tiled, a fitted and a plain forward
    for forward in (lambda: eng.forward_tiles_enqueue(dense, [v[:4] for v in views[:6]], fmt), lambda: eng.forward_fit_enqueue(dense, fmt),
                    lambda: eng.forward_enqueue(canvases_ref(bgr_of(dense, fmt), views, NET)[0])):
        forward()
        eng.decode_threshold(0.3, 0.3, 256)
        estate(eng.merge_views)
    # ... and so does an upload
    eng.forward_views_enqueue(dense, views, fmt)
    eng.decode_threshold(0.3, 0.3, 256)
    eng.upload_images(list(canvases_ref(bgr_of(dense, fmt), views, NET)[0, :2]))
    estate(eng.merge_views)
    # more views than the context holds
    with pytest.raises(ValueError) as e:
        eng.forward_views_enqueue(np.concatenate([dense, dense[:1]]), views, fmt)
    assert "max_batch" in str(e.value)
    eng.close()


# ------------------------------------------------------------------------------------------ the product paths
def engine_sequence(face, frames, fmt, views, merge=()):
    """forward_views + decode + merge_views, chunk by chunk, as detect_views is to run them."""
    per = face.engine.max_batch // len(views)
    out = []
    for i in range(0, len(frames), per):
        face.engine.forward_views_enqueue(frames[i:i + per], views, fmt)
        face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets)
        out += face.engine.merge_views(*merge, max_out=face.max_dets)[0]
    return out


def test_centerface_detect_views_and_anonymize():
    """CenterFace.detect_views = forward_views + decode + merge_views over the layout of the frames' size; anonymize(views=) changes
    exactly the bytes redact_ref changes for the merged boxes, in BGR and NV12; the inputs stay untouched."""
    h, w = FRAME_HW
    face = cfa.CenterFace(NET[0], NET[1], dtype="bf16", max_batch=20)
    views = ops.view_layout(h, w, *NET, **LAYOUT)
    assert 2 * len(views) <= 20 < 3 * len(views)                           # two frames per chunk: the third goes alone
    rng = np.random.default_rng(2)
    tried = []
    for kind in ("blocks", "binary", "noise", "blocks", "binary", "noise"):  # the default weights answer to one of them
        imgs = source_frames(rng, kind, (3, h, w, 3))
        got = face.detect_views(imgs, **LAYOUT)
        tried.append((kind, [len(d) for d, _ in got]))
        if sum(len(d) for d, _ in got) >= 2:
            break
    print("detect_views:", tried)
    assert sum(len(d) for d, _ in got) >= 2, tried
    assert all(d.shape[1:] == (5,) and l.shape == (len(d), 10) and d.dtype == np.float32 for d, l in got)
    want = engine_sequence(face, imgs, "bgr", views)
    assert same_results(got, want)
    # the defaults: no tiles, levels 1.0 and 0.5; the merge options travel
    two = ops.view_layout(h, w, *NET, scales=(1.0, 0.5))
    assert len(two) == 2 and same_results(face.detect_views(imgs), engine_sequence(face, imgs, "bgr", two))
    assert same_results(face.detect_views(imgs, metric="iou", thresh=0.3, edge=0.0, **LAYOUT), engine_sequence(face, imgs, "bgr", views, ("iou", 0.3, 0.0)))
    opts = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    keep = imgs.copy()
    out, dets = face.anonymize(list(imgs), views=LAYOUT, **opts)
    assert np.array_equal(imgs, keep) and same_results(dets, want)
    ref = keep.copy()
    redact_ref([(f.reshape(h, -1),) for f in ref], "bgr", np.concatenate([d[:, :4] for d, _ in want]), [len(d) for d, _ in want], (h, w), h, w, **opts)
    assert np.array_equal(out, ref) and not np.array_equal(out, keep)
    # NV12 frames of the same size
    yuv = source_frames(np.random.default_rng(3), tried[-1][0], (3, h * 3 // 2, w))
    ywant = engine_sequence(face, yuv, "nv12", views)
    yout, ydets = face.anonymize_yuv(yuv, "nv12", views=LAYOUT, **opts)
    assert same_results(ydets, ywant)
    yref = yuv.copy()
    redact_ref([(f[:h], f[h:]) for f in yref], "nv12", np.concatenate([d[:, :4] for d, _ in ywant]), [len(d) for d, _ in ywant], (h, w), h, w, **opts)
    assert np.array_equal(yout, yref)
    # annotate, the chips and views=True take the same path
    _, adets = face.annotate(list(imgs), views=LAYOUT)
    assert same_results(adets, want)
    assert same_results(face.anonymize(list(imgs), views=True, **opts)[1], engine_sequence(face, imgs, "bgr", two))
    rows = face.detect_aligned_frames(imgs, "bgr", 32, views=LAYOUT)
    assert same_results([(d, l) for d, l, _ in rows], want) and [len(c) for _, _, c in rows] == [len(d) for d, _ in want]
    # more views than max_batch holds
    with pytest.raises(ValueError) as e:
        cfa.CenterFace(NET[0], NET[1], dtype="bf16", max_batch=4).detect_views(imgs, **LAYOUT)
    assert "max_batch" in str(e.value)
    face.close()


def test_a_tracker_continues_one_stream_over_two_views_calls():
    """With a tracker two calls continue one stream: the tracks of the first call's merged rows are confirmed by the second's, and the
    redaction of the second call covers the tracked rows; a tracker with weak_score decodes at it and returns the strong rows."""
    h, w = FRAME_HW
    face = cfa.CenterFace(NET[0], NET[1], dtype="bf16", max_batch=16)
    views = ops.view_layout(h, w, *NET, **LAYOUT)
    rng = np.random.default_rng(4)
    for kind in ("blocks", "binary", "noise", "blocks", "binary", "noise"):
        imgs = source_frames(rng, kind, (2, h, w, 3))
        plain = face.detect_views(imgs, **LAYOUT)
        if min(len(d) for d, _ in plain) >= 1:
            break
    assert min(len(d) for d, _ in plain) >= 1
    trk = cfa.Tracker(face.engine, 2, min_hits=2)
    opts = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    ref = imgs.copy()
    redact_ref([(f.reshape(h, -1),) for f in ref], "bgr", np.concatenate([d[:, :4] for d, _ in plain]), [len(d) for d, _ in plain], (h, w), h, w, **opts)
    for call in range(2):
        frames = imgs.copy()
        got = face.detect_views(frames, tracker=trk, redact=opts, **LAYOUT)
        assert same_results(got, plain)                                    # the detections returned stay the frame's own
        assert np.array_equal(frames, ref) and not np.array_equal(frames, imgs)      # every track is matched: the tracked rows are the detections
    info = np.zeros((2, trk.max_tracks, 3), np.int32)
    dev = [face.engine.device_alloc(info.nbytes), face.engine.device_alloc(8)]
    face.engine.forward_views_enqueue(imgs, views, "bgr")
    face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets)
    face.engine.merge_views(max_out=face.max_dets)
    face.engine.track_update_device(trk, 0, info_ptr=dev[0], counts_ptr=dev[1])
    face.engine.synchronize()
    tc = np.empty(2, np.int32)
    face.engine.memcpy_d2h(info, dev[0])
    face.engine.memcpy_d2h(tc, dev[1])
    for p in dev:
        face.engine.device_free(p)
    # The same frames three times: a row whose box matches itself (IoU 1) is the third hit of the track the first call started.  The
    # synthetic weights also give boxes with x2 < x1, whose "+1" IoU with themselves is below the threshold: those are born anew each
    # time (hits 1) and their tentative track of the call before is freed, so the counts stay those of the detections.
    hits = [info[b, :tc[b], 1] for b in range(2)]
    print("hits per tracked row:", [np.bincount(x, minlength=4).tolist() for x in hits])
    assert tc.tolist() == [len(d) for d, _ in plain] and all(x.min() >= 1 and x.max() == 3 for x in hits)
    trk.close()
    weak = cfa.Tracker(face.engine, 2, min_hits=1, weak_score=0.1)
    assert same_results(face.detect_views(imgs, tracker=weak, **LAYOUT), plain)
    weak.close()
    face.close()


def test_without_views_the_product_paths_do_what_they_did():
    """views=None / False is the call without the keyword, byte for byte: anonymize, annotate and detect_tiled on the same inputs (what
    those compute is pinned by the tests of their own files, which this change leaves alone)."""
    h, w = FRAME_HW
    rng = np.random.default_rng(7)
    imgs = source_frames(rng, "blocks", (2, NET[0], NET[1], 3))
    big = source_frames(rng, "blocks", (2, h, w, 3))
    face = cfa.CenterFace(NET[0], NET[1], dtype="bf16", max_batch=16)

    def same(a, b):
        return a[0].tobytes() == b[0].tobytes() and same_results(a[1], b[1])

    base = face.anonymize(list(imgs), mode="solid", shape="rect")
    assert same(face.anonymize(list(imgs), views=None, mode="solid", shape="rect"), base)
    assert same(face.anonymize(list(imgs), views=False, mode="solid", shape="rect"), base)
    assert same(face.annotate(list(imgs), views=None), face.annotate(list(imgs)))
    tiled = face.detect_tiled(big, (32, 64), 8)
    assert same(face.anonymize(list(big), tiled=True, tile=(32, 64), overlap=8, views=False), face.anonymize(list(big), tiled=True, tile=(32, 64), overlap=8))
    assert same_results(face.anonymize(list(big), tiled=True, tile=(32, 64), overlap=8)[1], tiled)
    for call in (lambda: face.anonymize(list(big), views=True, tiled=True), lambda: face.annotate(list(big), views=True, fit=True),
                 lambda: face.anonymize(list(big), views=True, rotate=90), lambda: face.anonymize(list(big), rotate=90, tiled=True)):
        with pytest.raises(ValueError):
            call()
    face.close()


def test_demo_scales(tmp_path, capsys):
    """``demo --scales 1,0.5 --tiled 64`` on an image file: a 64 x 64 context, tiles and two levels in one batch, the faces redacted in
    the file it writes -- the bytes of ``CenterFace.anonymize(views=)`` on the decoded file."""
    from PIL import Image
    from centerface_amd import demo
    frame = source_frames(np.random.default_rng(8), "blocks", (1, 72, 96, 3))[0]
    path, out = str(tmp_path / "in.png"), str(tmp_path / "out.png")
    Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(path)
    opts = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    dets, _ = demo.anonymize_file(path, out, scales=(1.0, 0.5), tiled=64, **opts)
    views = dict(scales=(1.0, 0.5), tile=64)
    V = len(ops.view_layout(72, 96, 64, 64, **views))
    face = cfa.CenterFace(64, 64, dtype="bf16", max_batch=V)
    want, res = face.anonymize([demo.imread(path)], views=views, **opts)
    plain, _ = face.detect_views(demo.imread(path)[None], **views)[0]
    black, _ = face.anonymize([demo.imread(path)], views=views, mode="solid", shape="rect")      # the command line has no --fill
    face.close()
    assert dets.tobytes() == res[0][0].tobytes() and np.array_equal(demo.imread(out), want[0])
    capsys.readouterr()
    demo.main([path, "--scales", "1,0.5", "--tiled", "64"])                 # the detections alone: path line, count line, rows
    assert capsys.readouterr().out == demo.format_wider_result(path, plain)
    second = str(tmp_path / "second.png")
    demo.main([path, "--scales", "1,0.5", "--tiled", "64", "--anonymize", second, "--mode", "solid", "--shape", "rect"])
    assert np.array_equal(demo.imread(second), black[0]) and not np.array_equal(black[0], demo.imread(path))
    for bad in (["--fit"], ["--rotate", "90"]):
        with pytest.raises(SystemExit):
            demo.main([path, "--scales", "1,0.5"] + bad)

