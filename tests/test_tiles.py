"""Tiled detection on the GPU: the tile cutter (cf_op_cut_tiles, cf_forward_tiles), the merge (cf_op_merge_tiles, cf_merge_tiles) and the
redaction with merged boxes, every byte against the numpy restatements of tests/test_tiles_abi.py (cut = crop + the oracle's resize of
the restated conversion; merge = edge rule + float64 map + the NMS restatement), tests/test_yuv_input.py and tests/test_redact.py."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from test_redact import redact_ref, source_frames
from test_tiles_abi import cut_ref, merge_ref
from test_yuv_input import yuv_to_bgr_ref

pytestmark = pytest.mark.gpu

FORMATS = ("bgr", "nv12", "nv21", "i420", "yv12")
NET = (32, 64)                  # (H, W) of the cutter tests


# ------------------------------------------------------------------------------------------ frames with padded rows
def pitched_frames(dense, fmt, pad, aligned=False, guard=64):
    """Per frame a tuple of row views [rows, row bytes] on buffers of rows x pitch + guard bytes, padding and guard filled with ``pad``;
    ``dense``: [B,h,w,3] BGR or [B, h*3//2, w] 4:2:0.  Returns (views, buffers, pitch0, pitch1)."""
    B = dense.shape[0]
    if fmt == "bgr":
        h, w = dense.shape[1:3]
        geo = [(0, h, 3 * w)]
    else:
        h, w = dense.shape[1] * 2 // 3, dense.shape[2]
        offs, cp = cfa._lib.yuv_dense_geometry(cfa._lib.yuv_format(fmt), h, w)
        geo = [(0, h, w)] + [(o, h // 2, cp) for o in offs[1:] if o is not None]
    pitch = [3 * w + 6 if fmt == "bgr" else w + 4] + [c + 4 for _, _, c in geo[1:]]
    if aligned:
        pitch = [(p + 3) // 4 * 4 for p in pitch]
    views, bufs = [], []
    for b in range(B):
        flat = dense[b].reshape(-1)
        v = []
        for (o, r, c), p in zip(geo, pitch):
            buf = np.full(r * p + guard, pad, np.uint8)
            buf[:r * p].reshape(r, p)[:, :c] = flat[o:o + r * c].reshape(r, c)
            bufs.append(buf)
            v.append(buf[:r * p].reshape(r, p)[:, :c])
        views.append(tuple(v))
    return views, bufs, pitch[0], (pitch[1] if len(pitch) > 1 else 0)


def bgr_of(dense, fmt):
    return dense if fmt == "bgr" else np.stack([yuv_to_bgr_ref(f, fmt) for f in dense])


def rects_for(h, w):
    """One at the origin, one ending at the far corner, one of exactly (W, H), one 2 x 2, one that upscales (18 x 20), the whole frame
    (downscale), two that overlap."""
    H, W = NET
    return [(0, 0, 40, 30), (w - 36, h - 26, 36, 26), (10, 20, W, H), (44, 36, 2, 2), (6, 8, 18, 20), (0, 0, w, h), (20, 10, 50, 40), (40, 30, 50, 40)]


def tiles_ref(bgr, rects, size):
    return np.stack([np.stack([cut_ref(f, r, size) for r in rects]) for f in bgr])


_cut_cache = {}


def cut_case(fmt, hw):
    """(dense frames, reference tiles) of one format and frame size, computed once."""
    if (fmt, hw) not in _cut_cache:
        rng = np.random.default_rng(FORMATS.index(fmt) * 7 + hw[0])
        h, w = hw
        dense = rng.integers(0, 256, (2, h, w, 3) if fmt == "bgr" else (2, h * 3 // 2, w), dtype=np.uint8)
        _cut_cache[(fmt, hw)] = (dense, tiles_ref(bgr_of(dense, fmt), rects_for(h, w), NET))
    return _cut_cache[(fmt, hw)]


# ------------------------------------------------------------------------------------------ the cutter
@pytest.mark.parametrize("fmt", FORMATS)
def test_op_cut_tiles_bit_exact(fmt):
    """Bf = 2 frames of 70 x 94 and 72 x 96, eight rectangles, (H, W) = (32, 64), rows with padding: every byte equals the restatement,
    whether the padding and the bytes behind every plane hold 0xFF or 0x00."""
    for hw in ((70, 94), (72, 96)):
        dense, want = cut_case(fmt, hw)
        rects = rects_for(*hw)
        for pad in (0xFF, 0x00):
            views, bufs, _, _ = pitched_frames(dense, fmt, pad)
            got = ops.cut_tiles(views, rects, NET, fmt)
            assert got.shape == want.shape
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (fmt, hw, pad, len(bad), bad[:4].tolist())
        assert np.array_equal(ops.cut_tiles(dense, rects, NET, fmt), want)           # dense frames
    # the identity rectangle reproduces the source bytes
    dense, want = cut_case(fmt, (70, 94))
    assert np.array_equal(want[:, 2], bgr_of(dense, fmt)[:, 20:52, 10:74])


@pytest.mark.parametrize("fmt", ("yv12", "bgr"))
def test_op_cut_tiles_more_frames_than_one_launch(fmt):
    """Bf = 65 frames of 8 x 8 (one launch takes 64), two rectangles, (H, W) = (4, 8), rows with padding: frame 64 is the second launch's
    only frame -- its planes (YV12: swapped) at table entry 0, its tiles behind those of the 64 before it."""
    rng = np.random.default_rng(90 + FORMATS.index(fmt))
    dense = rng.integers(0, 256, (65, 8, 8, 3) if fmt == "bgr" else (65, 12, 8), dtype=np.uint8)
    rects = [(0, 2, 8, 4), (2, 0, 6, 8)]
    want = tiles_ref(bgr_of(dense, fmt), rects, (4, 8))
    views, _, _, _ = pitched_frames(dense, fmt, 0xFF)
    got = ops.cut_tiles(views, rects, (4, 8), fmt)
    assert got.shape == want.shape == (65, 2, 4, 8, 3)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (fmt, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("fmt", FORMATS)
def test_engine_forward_tiles_writes_the_restated_tiles(fmt):
    """cf_forward_tiles, host-staged (padded rows, and one dense block) and in place on device planes: cf_get_resized_input returns the
    restated tiles, image f * T + t = tile t of frame f."""
    hw = (72, 96)
    dense, want = cut_case(fmt, hw)
    rects = rects_for(*hw)
    T = len(rects)
    eng = cfa.Engine(NET[0], NET[1], max_batch=2 * T, dtype="bf16")
    views, bufs, p0, p1 = pitched_frames(dense, fmt, 0xFF)
    for frames in (views, dense):
        eng.forward_tiles_enqueue(frames, rects, fmt)
        got = eng.resized_input()
        assert got.shape == (2 * T,) + NET + (3,) and np.array_equal(got.reshape(want.shape), want), fmt
    got = None
    for pad in (0xFF, 0x00):
        views, bufs, p0, p1 = pitched_frames(dense, fmt, pad, aligned=True)
        dev = [eng.device_alloc(b.nbytes) for b in bufs]
        for d, b in zip(dev, bufs):
            eng.memcpy_h2d(d, b)
        n = len(views[0])
        eng.forward_tiles_enqueue([tuple(dev[b * n:(b + 1) * n]) for b in range(2)], rects, fmt, on_device=True, h=hw[0], w=hw[1], pitch0=p0, pitch1=p1)
        got = eng.resized_input()
        assert np.array_equal(got.reshape(want.shape), want), (fmt, pad)
        for d, b in zip(dev, bufs):                                                  # read in place: the planes are untouched
            back = np.empty_like(b)
            eng.memcpy_d2h(back, d)
            assert np.array_equal(back, b)
        with pytest.raises(ValueError):                                              # a misaligned device plane
            eng.forward_tiles_enqueue([(dev[b * n] + 2,) + tuple(dev[b * n + 1:(b + 1) * n]) for b in range(2)], rects, fmt, on_device=True, h=hw[0], w=hw[1],
                                      pitch0=p0, pitch1=p1)
        for d in dev:
            eng.device_free(d)
    # refusals name the rectangle and leave the engine working; Bf * T must fit max_batch
    with pytest.raises(ValueError) as e:
        eng.forward_tiles_enqueue(dense, rects[:3] + [(2, 2, 96, 8)], fmt)
    assert "rectangle 3" in str(e.value)
    with pytest.raises(ValueError):
        eng.forward_tiles_enqueue(dense, [(0, 0, 5, 4)], fmt)
    with pytest.raises(ValueError) as e:
        eng.forward_tiles_enqueue(dense, rects + rects[:1], fmt)
    assert "max_batch" in str(e.value)
    eng.forward_tiles_enqueue(dense, rects, fmt)
    assert np.array_equal(eng.resized_input().reshape(want.shape), want)
    eng.close()


# ------------------------------------------------------------------------------------------ the merge on hand-built tables
FILL = np.float32(-7.25)


def check_merge(rects, frame_hw, net_hw, d, s, l, counts, max_out, **opt):
    """ops.merge_tiles against merge_ref, bit for bit: counts, flags, the rows below min(count, max_out), and the caller's bytes in
    every row behind them."""
    d, s, l = (np.asarray(a, np.float32) for a in (d, s, l))
    Bf = d.shape[0]
    od, ol = np.full((Bf, max_out, 5), FILL), np.full((Bf, max_out, 10), FILL)
    gd, gl, gc, gf = ops.merge_tiles(rects, frame_hw, net_hw, d, s, l, counts, max_out, dets=od, lms=ol, **opt)
    want, wflags = merge_ref(rects, frame_hw, net_hw, d, s, l, counts, **opt)
    assert gc.tolist() == [len(w[0]) for w in want], (gc, [len(w[0]) for w in want])
    assert gf.tolist() == wflags.tolist()
    for f, (wd, wl) in enumerate(want):
        m = min(len(wd), max_out)
        assert gd[f, :m].tobytes() == wd[:m].tobytes(), (f, gd[f, :m], wd[:m])
        assert gl[f, :m].tobytes() == wl[:m].tobytes(), f
        assert (gd[f, m:] == FILL).all() and (gl[f, m:] == FILL).all(), f
    return want, gc, gf


def table(Bf, T, rows, entries):
    """dets_net / scores / lms_net / counts from {(f, t): [(x1, y1, x2, y2, score), ...]}; the landmark values of row i are 3 + i + 4 (k % 8)."""
    d, s, l = np.zeros((Bf, T, rows, 4), np.float32), np.zeros((Bf, T, rows), np.float32), np.zeros((Bf, T, rows, 10), np.float32)
    c = np.zeros((Bf, T), np.int32)
    for (f, t), rws in entries.items():
        c[f, t] = len(rws)
        for i, r in enumerate(rws):
            d[f, t, i], s[f, t, i] = r[:4], r[4]
            l[f, t, i] = (np.arange(10) % 8) * 4 + 3 + i
    return d, s, l, c


TWO = [(0, 0, 64, 64), (32, 0, 64, 64)]       # a 64 x 96 frame: the right side of tile 0 and the left side of tile 1 are interior


def test_merge_duplicates_ties_and_the_edge_rule():
    frame, net = (64, 96), (64, 64)
    # the same face (frame 40..60 x 10..30) seen by both tiles: the higher score survives, landmarks mapped with its tile's origin
    d, s, l, c = table(1, 2, 4, {(0, 0): [(40, 10, 60, 30, 0.8)], (0, 1): [(8, 10, 28, 30, 0.9)]})
    want, gc, _ = check_merge(TWO, frame, net, d, s, l, c, 4)
    assert gc.tolist() == [1] and want[0][0][0].tolist() == [40, 10, 60, 30, np.float32(0.9)]
    assert want[0][1][0].tolist() == (l[0, 1, 0] + np.float32([32, 0] * 5)).tolist()
    # equal scores: the higher candidate index (the later tile) first
    s[0, 0, 0] = s[0, 1, 0]
    want, gc, _ = check_merge(TWO, frame, net, d, s, l, c, 4)
    assert gc.tolist() == [1] and want[0][1][0, 0] == l[0, 1, 0, 0] + 32
    # tiles that scale: a 2x tile and the whole frame
    scaled = [(0, 0, 32, 32), (0, 0, 96, 64)]
    check_merge(scaled, frame, net, d, s, l, c, 4, edge=0.0)
    # within `edge` of an interior side: dropped; the same box against a frame-border side: kept
    box = (40, 10, 63.5, 30, 0.7)
    d, s, l, c = table(1, 2, 4, {(0, 0): [box], (0, 1): [box]})
    want, gc, _ = check_merge(TWO, frame, net, d, s, l, c, 4, edge=2.0)
    assert gc.tolist() == [1] and want[0][0][0, 0] == 72                  # tile 1's copy: its right side is the frame's
    want, gc, _ = check_merge(TWO, frame, net, d, s, l, c, 4, edge=0.0)
    assert gc.tolist() == [2]
    for bx in [(1.5, 10, 20, 30, 0.7), (10, 1.5, 20, 30, 0.7), (10, 10, 20, 62.5, 0.7), (10, 10, 62.5, 30, 0.7)]:
        grid = [(32, 32, 64, 64)]                                         # every side interior in a 128 x 128 frame
        d, s, l, c = table(1, 1, 2, {(0, 0): [bx]})
        assert check_merge(grid, (128, 128), net, d, s, l, c, 2, edge=2.0)[1].tolist() == [0], bx
        assert check_merge(grid, (128, 128), net, d, s, l, c, 2, edge=1.0)[1].tolist() == [1], bx
    # exactly on the limit: x1 = edge is kept (x1 < edge is the test), x2 = W - edge is kept
    d, s, l, c = table(1, 1, 2, {(0, 0): [(2, 2, 62, 62, 0.7)]})
    assert check_merge([(32, 32, 64, 64)], (128, 128), net, d, s, l, c, 2, edge=2.0)[1].tolist() == [1]
    # a non-finite corner is dropped
    d, s, l, c = table(1, 2, 4, {(0, 0): [(np.nan, 10, 30, 30, 0.9), (10, 10, 30, 30, 0.5), (10, 10, np.inf, 30, 0.95)], (0, 1): [(30, 40, 50, -np.inf, 0.9)]})
    assert check_merge(TWO, frame, net, d, s, l, c, 4)[1].tolist() == [1]


def test_merge_has_no_centre_rule_and_maps_a_negative_zero():
    """The tile merge drops by the edge rule alone: a row of tile 0 whose centre lies left of the canvas (x1 = -40, x2 = 10) has the
    frame's left side beside it and stays, where the views merge would drop it.  A -0.0 corner and a -0.0 landmark map as
    float32(float64(-0.0) * sx + x0): +0.0 in tile 0 (x0 = 0), bit for bit."""
    frame, net = (64, 96), (64, 64)
    d, s, l, c = table(1, 2, 4, {(0, 0): [(-40, 10, 10, 30, 0.9), (-0.0, 40, 20, 60, 0.8)]})
    l[0, 0, 1, :2] = -0.0
    assert np.signbit(d[0, 0, 1, 0]) and np.signbit(l[0, 0, 1, 0])
    want, gc, _ = check_merge(TWO, frame, net, d, s, l, c, 4)
    assert gc.tolist() == [2] and want[0][0][0].tolist() == [-40, 10, 10, 30, np.float32(0.9)]
    assert want[0][0][1, 0] == 0 and not np.signbit(want[0][0][1, 0]) and not np.signbit(want[0][1][1, :2]).any()


def test_merge_ios_against_iou_flags_and_truncation():
    frame, net = (256, 384), (256, 256)
    rects = [(0, 0, 256, 256), (128, 0, 256, 256)]
    # a partial box (tile 1 sees the upper part only) inside the full one tile 0 sees: IoU 0.406 keeps both at 0.5, IoS removes it
    d, s, l, c = table(1, 2, 3, {(0, 0): [(140, 100, 240, 200, 0.9)], (0, 1): [(12, 100, 112, 140, 0.8)]})
    assert check_merge(rects, frame, net, d, s, l, c, 4, metric="iou", thresh=0.5)[1].tolist() == [2]
    want, gc, _ = check_merge(rects, frame, net, d, s, l, c, 4, metric="ios", thresh=0.5)
    assert gc.tolist() == [1] and want[0][0][0].tolist() == [140, 100, 240, 200, np.float32(0.9)]
    # a tile with counts > rows sets bit 0 of its frame's flag, only there; its rows below `rows` are merged
    d, s, l, c = table(2, 2, 3, {(0, 0): [(140, 100, 240, 200, 0.9)], (1, 1): [(10, 10, 40, 40, 0.5), (60, 60, 90, 90, 0.6), (100, 100, 130, 130, 0.7)]})
    c[1, 1] = 5
    _, gc, gf = check_merge(rects, frame, net, d, s, l, c, 4)
    assert gc.tolist() == [1, 3] and gf.tolist() == [0, 1]
    # more survivors than max_out: only max_out rows are written, the count tells; the rows of the next (empty) frame stay as they were
    five = [(10 + 40 * k, 10, 40 + 40 * k, 40, 0.5 + 0.05 * k) for k in range(5)]
    d, s, l, c = table(2, 2, 5, {(0, 0): five})
    want, gc, _ = check_merge(rects, frame, net, d, s, l, c, 2)
    assert gc.tolist() == [5, 0] and want[0][0][0, 4] == np.float32(0.7)


@pytest.mark.parametrize("T,rows", ((5, 60), (3, 100)))
def test_merge_random_tables(T, rows):
    """300 candidates per frame (past the 64- and 256-candidate boundaries of the rank / mask / sweep kernels), Bf = 2 with different
    counts per tile, an empty tile, a truncated tile, many score ties; a third frame without any row."""
    rng = np.random.default_rng(T)
    frame, net = (128, 160), (64, 64)
    rects = [(0, 0, 64, 64), (48, 0, 64, 64), (96, 0, 64, 64), (0, 64, 64, 64), (0, 0, 160, 128)][:T]
    Bf = 3
    xy = rng.uniform(0, 56, (Bf, T, rows, 2)).astype(np.float32)
    wh = rng.uniform(2, 24, (Bf, T, rows, 2)).astype(np.float32)
    d = np.minimum(np.concatenate([xy, xy + wh], -1), np.float32(64))
    s = rng.choice(np.linspace(0.3, 0.95, 40).astype(np.float32), (Bf, T, rows))
    l = rng.uniform(0, 64, (Bf, T, rows, 10)).astype(np.float32)
    c = np.zeros((Bf, T), np.int32)
    c[0] = [rows, 0, rows - 7, 31, rows][:T]
    c[1] = [rows + 9, rows, 1, rows, 64][:T]
    d[1, 1, 5, 2] = np.nan
    for metric, thr, edge in (("ios", 0.5, 2.0), ("iou", 0.3, 0.0), ("ios", 0.9, 5.0)):
        want, gc, gf = check_merge(rects, frame, net, d, s, l, c, T * rows, metric=metric, thresh=thr, edge=edge)
        assert gc[2] == 0 and gf.tolist() == [0, 1, 0] and gc[0] > 8 and gc[1] > 8
    check_merge(rects, frame, net, d, s, l, c, 7, metric="iou", thresh=0.3, edge=0.0)            # truncated outputs


# ------------------------------------------------------------------------------------------ the engine
ENG_HW = (64, 96)
FRAME_HW = (150, 200)


def tiled_engine(fmt="bgr", seed=0):
    """A 64 x 96 context with the default (synthetic) weights, two 150 x 200 frames, the 3 x 3 + 1 grid, and a score threshold read off
    the heat maps so that EVERY tile has at least 6 cells above it: (engine, dense frames, rects, threshold)."""
    rng = np.random.default_rng(seed)
    h, w = FRAME_HW
    dense = source_frames(rng, "blocks", (2, h, w, 3) if fmt == "bgr" else (2, h * 3 // 2, w))
    rects = ops.tile_grid(h, w, ENG_HW, 16)
    assert len(rects) == 10
    eng = cfa.Engine(ENG_HW[0], ENG_HW[1], max_batch=2 * len(rects), dtype="bf16")
    eng.forward_tiles_enqueue(dense, rects, fmt)
    hm = eng.heads(sigmoid_hm=True)["hm_sigmoid"].reshape(2 * len(rects), -1)
    sixth = np.sort(hm, 1)[:, -6]
    thr = float(np.nextafter(np.float32(sixth.min()), np.float32(0)))
    above = (hm > np.float32(thr)).sum(1)
    print("threshold %.6f, cells above it per tile: %s" % (thr, above.tolist()))
    assert above.min() >= 6, above                                         # a handful of candidates in every tile
    return eng, dense, rects, thr


def net_tables(per, Bf, T):
    """The per-tile decode results (network coordinates) as the merge's tables."""
    rows = max(1, max(len(d) for d, _ in per))
    d, s, l = np.zeros((Bf, T, rows, 4), np.float32), np.zeros((Bf, T, rows), np.float32), np.zeros((Bf, T, rows, 10), np.float32)
    c = np.zeros((Bf, T), np.int32)
    for k, (dd, ll) in enumerate(per):
        f, t = divmod(k, T)
        c[f, t] = len(dd)
        d[f, t, :len(dd)], s[f, t, :len(dd)], l[f, t, :len(dd)] = dd[:, :4], dd[:, 4], ll
    return d, s, l, c


def same_results(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() and u.tobytes() == v.tobytes() for (x, u), (y, v) in zip(a, b))


def test_engine_tiled_decode_and_merge_equal_the_restatement():
    eng, dense, rects, thr = tiled_engine()
    T = len(rects)
    tiles = tiles_ref(dense, rects, ENG_HW).reshape((2 * T,) + ENG_HW + (3,))
    assert np.array_equal(eng.resized_input(), tiles)
    per = eng.decode_threshold(thr, 0.5, 256)
    print("kept per tile:", [len(d) for d, _ in per])
    assert min(len(d) for d, _ in per) >= 1 and sum(len(d) for d, _ in per) >= 2 * T
    # the per-tile results are those of the restated tiles fed as an ordinary uint8 batch
    eng.forward_enqueue(tiles)
    assert same_results(eng.decode_threshold(thr, 0.5, 256), per)
    with pytest.raises(cfa._lib.CenterFaceError) as e:                     # ... behind which there is nothing to merge
        eng.merge_tiles()
    assert e.value.code == cfa._lib.CF_ESTATE
    d, s, l, c = net_tables(per, 2, T)
    outs = {}
    for opt in (dict(metric="ios", thresh=0.5, edge=2.0), dict(metric="iou", thresh=0.3, edge=0.0)):
        want, wflags = merge_ref(rects, FRAME_HW, ENG_HW, d, s, l, c, **opt)
        eng.forward_tiles_enqueue(dense, rects, "bgr")
        with pytest.raises(cfa._lib.CenterFaceError) as e:                 # before a decode
            eng.merge_tiles(**opt)
        assert e.value.code == cfa._lib.CF_ESTATE
        assert same_results(eng.decode_threshold(thr, 0.5, 256), per)
        got, flags = eng.merge_tiles(max_out=256, **opt)
        print("merged per frame:", [len(x) for x, _ in got], "of", c.sum(1).tolist())
        assert same_results(got, want) and flags.tolist() == wflags.tolist() == [0, 0]
        assert all(1 <= len(x) <= n for (x, _), n in zip(got, c.sum(1)))
        outs[opt["metric"]] = got
        # truncated host form: counts beyond max_out make the wrapper come back for all of them
        assert same_results(eng.merge_tiles(max_out=1, **opt)[0], want)
        # the device form, read back
        mo = 64
        bufs = [eng.device_alloc(2 * mo * 5 * 4), eng.device_alloc(2 * mo * 10 * 4), eng.device_alloc(8), eng.device_alloc(8)]
        eng.merge_tiles_device(mo, *bufs, **opt)
        eng.synchronize()
        hd, hl, hc, hf = np.empty((2, mo, 5), np.float32), np.empty((2, mo, 10), np.float32), np.empty(2, np.int32), np.empty(2, np.int32)
        for a, b in zip((hd, hl, hc, hf), bufs):
            eng.memcpy_d2h(a, b)
            eng.device_free(b)
        assert hc.tolist() == [len(x) for x, _ in want] and hf.tolist() == [0, 0]
        assert same_results([(hd[f, :min(hc[f], mo)], hl[f, :min(hc[f], mo)]) for f in range(2)], [(x[:mo], y[:mo]) for x, y in want])
        eng.merge_tiles_device(mo, **opt)                                  # every output may be NULL
        # cf_set_rescale changes the decode's own rows, not the merge
        eng.set_rescale(1.37, 1.21)
        scaled = eng.decode_threshold(thr, 0.5, 256)
        assert [len(x) for x, _ in scaled] == [len(x) for x, _ in per] and not same_results(scaled, per)
        assert same_results(eng.merge_tiles(max_out=256, **opt)[0], want)
        eng.set_rescale(0.0, 0.0)
    # a decode with fewer rows than a tile kept: the merge sees the first rows only and says so
    eng.forward_tiles_enqueue(dense, rects, "bgr")
    L, P = cfa._lib.lib(), cfa._lib.ptr
    d5, l10, cn = np.empty((2 * T, 1, 5), np.float32), np.empty((2 * T, 1, 10), np.float32), np.empty(2 * T, np.int32)
    assert L.cf_decode_threshold(eng._h, thr, 0.5, 1, P(d5), P(l10), P(cn)) == 0
    first = [(x[:1], y[:1]) for x, y in per]
    d1, s1, l1, c1 = net_tables(first, 2, T)
    want, wflags = merge_ref(rects, FRAME_HW, ENG_HW, d1, s1, l1, cn.reshape(2, T))
    got, flags = eng.merge_tiles(max_out=32)
    assert same_results(got, want) and flags.tolist() == wflags.tolist() and (flags == 1).any() == bool((cn > 1).any())
    # a new upload forgets the decode
    eng.upload_images(list(tiles[:2]))
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        eng.merge_tiles()
    assert e.value.code == cfa._lib.CF_ESTATE
    eng.close()


@pytest.mark.parametrize("fmt", ("bgr", "nv12"))
def test_redact_after_a_merge_uses_the_merged_boxes(fmt):
    eng, dense, rects, thr = tiled_engine(fmt, seed=1)
    h, w = FRAME_HW
    per = eng.decode_threshold(thr, 0.5, 256)
    opt = dict(mode="mosaic", shape="ellipse", cell=6)

    def frames(pad=0xFF):
        return pitched_frames(dense, fmt, pad)

    views, bufs, _, _ = frames()
    with pytest.raises(cfa._lib.CenterFaceError) as e:                     # a tiled forward and a decode, but no merge
        eng.redact_faces(views, fmt, **opt)
    assert e.value.code == cfa._lib.CF_ESTATE
    merged, _ = eng.merge_tiles(max_out=256)
    assert sum(len(d) for d, _ in merged) >= 2
    boxes = np.concatenate([d[:, :4] for d, _ in merged])
    counts = np.array([len(d) for d, _ in merged], np.int32)
    wviews, wbufs, _, _ = frames()
    redact_ref(wviews, fmt, boxes, counts, (h, w), h, w, **opt)             # the merged corners, in frame pixels: (H, W) = (h, w)
    assert eng.redact_faces(views, fmt, **opt) is views
    assert all(np.array_equal(a, b) for a, b in zip(bufs, wbufs))
    orig = frames()[1]
    assert not all(np.array_equal(a, b) for a, b in zip(bufs, orig))       # something was redacted
    # the wrong B or frame size is refused, nothing is written
    for bad in ([views[0]], [tuple(p[:h - 2] if k == 0 else p[:(h - 2) // 2] for k, p in enumerate(v)) for v in views]):
        keep = [b.copy() for b in bufs]
        with pytest.raises(ValueError):
            eng.redact_faces(bad, fmt, **opt)
        assert all(np.array_equal(a, b) for a, b in zip(bufs, keep))
    # a new decode forgets the merge
    eng.decode_threshold(thr, 0.5, 256)
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        eng.redact_faces(views, fmt, **opt)
    assert e.value.code == cfa._lib.CF_ESTATE
    # after a following non-tiled forward the redaction is the usual one: the decode's network boxes of B = last batch, scaled by w / W
    T = len(rects)
    tiles = tiles_ref(bgr_of(dense, fmt), rects, ENG_HW).reshape((2 * T,) + ENG_HW + (3,))
    eng.forward_enqueue(tiles[:2])
    base = eng.decode_threshold(thr, 0.5, 256)
    nb, nc = np.concatenate([d[:, :4] for d, _ in base]), np.array([len(d) for d, _ in base], np.int32)
    assert int(nc.sum()) >= 1
    views, bufs, _, _ = frames()
    wviews, wbufs, _, _ = frames()
    redact_ref(wviews, fmt, nb, nc, ENG_HW, h, w, **opt)
    eng.redact_faces(views, fmt, **opt)
    assert all(np.array_equal(a, b) for a, b in zip(bufs, wbufs))
    eng.close()


def test_centerface_detect_tiled_and_anonymize():
    """CenterFace.detect_tiled = forward_tiles + decode + merge with the defaults (tile = the context's size, overlap = a quarter of it,
    the whole frame added); anonymize(tiled=True) redacts a copy with the merged boxes."""
    rng = np.random.default_rng(2)
    h, w = FRAME_HW
    face = cfa.CenterFace(ENG_HW[0], ENG_HW[1], dtype="bf16", max_batch=24)
    rects = ops.tile_grid(h, w, ENG_HW, 16)                                 # min(64, 96) // 4 = 16
    assert 2 * len(rects) <= 24 < 3 * len(rects)                           # two frames per chunk: the third goes alone
    tried = []
    for kind in ("blocks", "binary", "noise", "blocks", "binary", "noise"):  # the default weights answer to one of them
        imgs = source_frames(rng, kind, (3, h, w, 3))
        got = face.detect_tiled(imgs)
        tried.append((kind, [len(d) for d, _ in got]))
        if sum(len(d) for d, _ in got) >= 2:
            break
    print("detect_tiled:", tried)
    assert sum(len(d) for d, _ in got) >= 2, tried
    assert all(d.shape[1:] == (5,) and l.shape == (len(d), 10) and d.dtype == np.float32 for d, l in got)
    want = []
    for chunk in (imgs[:2], imgs[2:]):
        face.engine.forward_tiles_enqueue(chunk, rects, "bgr")
        per = face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets)
        d, s, l, c = net_tables(per, len(chunk), len(rects))
        want += merge_ref(rects, (h, w), ENG_HW, d, s, l, c)[0]
    assert same_results(got, want)
    keep = imgs.copy()
    out, dets = face.anonymize(list(imgs), tiled=True, mode="solid", shape="rect", fill=(1, 2, 3))
    assert np.array_equal(imgs, keep) and same_results(dets, want)
    ref = keep.copy()
    redact_ref([(f.reshape(h, -1),) for f in ref], "bgr", np.concatenate([d[:, :4] for d, _ in want]), [len(d) for d, _ in want], (h, w), h, w,
               mode="solid", shape="rect", fill=(1, 2, 3))
    assert np.array_equal(out, ref)
    with pytest.raises(ValueError):
        cfa.CenterFace(ENG_HW[0], ENG_HW[1], dtype="bf16", max_batch=4).detect_tiled(imgs)       # ten tiles do not fit
    face.close()
