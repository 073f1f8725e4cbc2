"""Face redaction in the source frame (cf_redact_faces / cf_op_redact, csrc/cf_redact.hip): the arithmetic restated in numpy, known
answers of the restatement worked by hand, and the device against the restatement bit for bit -- on every byte of every buffer, pitch
padding and a guard band behind each plane included.

The statement (include/centerface_hip.h has it in full): the float32 box in network coordinates is grown about its centre by `scale`
and mapped to the frame in float64 (fixed order, no FMA), floor / ceil, clamped to [-8192, 16384], snapped outwards to even; a sample
is covered by its own point test in half-pixel units (RECT, or the int64 ELLIPSE test); a covered sample becomes fill[channel] (SOLID) or
the round-half-up mean of its cell of a grid anchored at the FRAME origin, taken from the untouched frame (MOSAIC)."""
import ctypes as C

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops

GUARD = 64                      # bytes behind every plane buffer, pre-filled with PAD like the pitch padding
PAD = 0xA5
FORMATS = ("bgr", "nv12", "nv21", "i420", "yv12")


# ------------------------------------------------------------------------------------------ the restatement
def face_box(box, scale, h, w, H, W):
    """(X1, Y1, X2, Y2) of one face in frame pixels, or None when the face is skipped."""
    x1, y1, x2, y2 = (np.float64(np.float32(v)) for v in box)
    s = np.float64(np.float32(scale))
    if not (np.isfinite(x1) and np.isfinite(y1) and np.isfinite(x2) and np.isfinite(y2)):
        return None
    cx, cy = (x1 + x2) * 0.5, (y1 + y2) * 0.5
    hw, hh = (x2 - x1) * 0.5 * s, (y2 - y1) * 0.5 * s
    if not (hw > 0 and hh > 0):
        return None
    fx, fy = np.float64(w) / np.float64(W), np.float64(h) / np.float64(H)

    def snap(v):
        return int(min(max(v, -8192.0), 16384.0))
    X1, Y1 = snap(np.floor((cx - hw) * fx)), snap(np.floor((cy - hh) * fy))
    X2, Y2 = snap(np.ceil((cx + hw) * fx)), snap(np.ceil((cy + hh) * fy))
    return X1 - X1 % 2, Y1 - Y1 % 2, X2 + X2 % 2, Y2 + Y2 % 2          # python's % is non-negative: down / up to even


def coverage(fboxes, shape, rows, cols, chroma):
    """bool [rows, cols]: the samples of a plane (luma / BGR pixels, or chroma samples) that some box of ``fboxes`` covers."""
    U = (4 * np.arange(cols, dtype=np.int64) + 2) if chroma else (2 * np.arange(cols, dtype=np.int64) + 1)
    V = (4 * np.arange(rows, dtype=np.int64) + 2) if chroma else (2 * np.arange(rows, dtype=np.int64) + 1)
    cov = np.zeros((rows, cols), bool)
    for fb in fboxes:
        if fb is None:
            continue
        X1, Y1, X2, Y2 = fb
        if shape == "rect":
            cov |= ((2 * Y1 <= V) & (V < 2 * Y2))[:, None] & ((2 * X1 <= U) & (U < 2 * X2))[None, :]
        else:
            A, Bv = X2 - X1, Y2 - Y1
            du, dv = U - (X1 + X2), V - (Y1 + Y2)
            assert abs(du).max() <= 49152 and max(A, Bv) <= 24576
            cov |= ((du * Bv) ** 2)[None, :] + ((dv * A) ** 2)[:, None] <= (A * Bv) ** 2
    return cov


def cell_values(plane, m):
    """[rows, cols] -> every sample's mosaic value: (sum + n // 2) // n over its m x m cell of the grid anchored at (0, 0), edge cells
    over the samples they really have."""
    rows, cols = plane.shape
    ys, xs = np.arange(0, rows, m), np.arange(0, cols, m)
    sums = np.add.reduceat(np.add.reduceat(plane.astype(np.int64), ys, axis=0), xs, axis=1)
    n = np.diff(np.append(ys, rows))[:, None] * np.diff(np.append(xs, cols))[None, :]
    mean = (sums + n // 2) // n
    return mean[(np.arange(rows) // m)[:, None], (np.arange(cols) // m)[None, :]]


def plane_passes(fmt):
    """[(plane index, bytes per sample position, chroma?, fill index of each byte of a position)] of a format."""
    return {"bgr": [(0, 3, False, (0, 1, 2))],
            "nv12": [(0, 1, False, (0,)), (1, 2, True, (1, 2))], "nv21": [(0, 1, False, (0,)), (1, 2, True, (2, 1))],
            "i420": [(0, 1, False, (0,)), (1, 1, True, (1,)), (2, 1, True, (2,))],
            "yv12": [(0, 1, False, (0,)), (1, 1, True, (2,)), (2, 1, True, (1,))]}[fmt]


def redact_ref(frames, fmt, boxes, counts, net_hw, h, w, mode="mosaic", shape="ellipse", cell=20, scale=1.3, fill=(0, 0, 0)):
    """The restatement, in place on ``frames`` = per frame a tuple of 2-D uint8 row views [rows, row bytes] (a BGR row = 3w bytes, an
    interleaved chroma row = w bytes).  boxes [N,4] in network coordinates, image after image."""
    H, W = net_hw
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    at = 0
    for b, planes in enumerate(frames):
        fboxes = [face_box(bx, scale, h, w, H, W) for bx in boxes[at:at + int(counts[b])]]
        at += int(counts[b])
        for k, bps, chroma, chans in plane_passes(fmt):
            view = planes[k]
            rows, cols = (h // 2, w // 2) if chroma else (h, w)
            assert view.shape == (rows, cols * bps)
            cov = coverage(fboxes, shape, rows, cols, chroma)
            for c in range(bps):
                ch = view[:, c::bps]                                    # a view: one channel of the plane, [rows, cols]
                val = cell_values(ch, cell // 2 if chroma else cell) if mode == "mosaic" else fill[chans[c]]
                ch[cov] = val[cov] if mode == "mosaic" else val
    return frames


# ------------------------------------------------------------------------------------------ frames with padding and guard bands
class Frames(object):
    """B noise frames of one format in flat uint8 buffers: ``dense`` = one [B, h*3//2, w] (or [B,h,w,3]) block + guard, otherwise one
    buffer per plane with a row pitch and a guard band, padding and guard pre-filled with PAD.  ``views`` are the restatement's row
    views, ``arg`` what ops.redact_faces / Engine.redact_faces take."""

    def __init__(self, rng, fmt, B, h, w, pitch0=None, pitch1=None, dense=False, bufs=None):
        self.fmt, self.B, self.h, self.w, self.dense = fmt, B, h, w, dense
        geo = [(h, 3 * w)] if fmt == "bgr" else [(h, w), (h // 2, w)] if fmt in ("nv12", "nv21") else [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
        self.geo = geo
        if dense:
            one = sum(r * c for r, c in geo)
            self.pitches = [c for _, c in geo]
            self.bufs = bufs or [np.full(B * one + GUARD, PAD, np.uint8)]
            if bufs is None:
                self.bufs[0][:B * one] = rng.integers(0, 256, B * one, dtype=np.uint8)
            flat = self.bufs[0]
            self.views, o = [], 0
            for b in range(B):
                v = []
                for r, c in geo:
                    v.append(flat[o:o + r * c].reshape(r, c))
                    o += r * c
                self.views.append(tuple(v))
            body = flat[:B * one]
            self.arg = body.reshape(B, h, w, 3) if fmt == "bgr" else body.reshape(B, h * 3 // 2, w)
        else:
            self.pitches = [pitch0] + [pitch1] * (len(geo) - 1)
            self.bufs = bufs or []
            self.views = []
            for b in range(B):
                v = []
                for k, (r, c) in enumerate(geo):
                    p = self.pitches[k]
                    if bufs is None:
                        buf = np.full(r * p + GUARD, PAD, np.uint8)
                        buf[:r * p].reshape(r, p)[:, :c] = rng.integers(0, 256, (r, c), dtype=np.uint8)
                        self.bufs.append(buf)
                    buf = self.bufs[b * len(geo) + k]
                    v.append(buf[:r * p].reshape(r, p)[:, :c])
                self.views.append(tuple(v))
            self.arg = self.views

    def clone(self):
        return Frames(None, self.fmt, self.B, self.h, self.w, self.pitches[0], self.pitches[-1], self.dense, [b.copy() for b in self.bufs])

    def same(self, other):
        return all(np.array_equal(a, b) for a, b in zip(self.bufs, other.bufs))

    def diff(self, other):
        for k, (a, b) in enumerate(zip(self.bufs, other.bufs)):
            if not np.array_equal(a, b):
                return "buffer %d of %d: %d bytes differ, first at %s" % (k, len(self.bufs), int((a != b).sum()), np.flatnonzero(a != b)[:6])
        return "equal"


def pitches_for(fmt, w, aligned=False):
    """The issue's pitches 3w+6 / w+4 / w/2+4 (``aligned``: rounded up to 4 for device planes)."""
    p0 = 3 * w + 6 if fmt == "bgr" else w + 4
    p1 = 0 if fmt == "bgr" else w + 4 if fmt in ("nv12", "nv21") else w // 2 + 4
    if aligned:
        p0, p1 = (p0 + 3) // 4 * 4, (p1 + 3) // 4 * 4
    return p0, p1


# ------------------------------------------------------------------------------------------ known answers of the restatement
def _bgr(h, w, value=None, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, 3 * w), dtype=np.uint8) if value is None else np.full((h, 3 * w), value, np.uint8)
    return a


def test_restatement_rect_solid_is_the_even_snapped_rectangle():
    # frame 12 x 16 = network size, scale 1: box (3.2, 2.5)-(8.9, 7.1): centre (6.05, 4.8), half sizes (2.85, 2.3) -> floor 3.2 = 3,
    # ceil 8.9 = 9, floor 2.5 = 2, ceil 7.1 = 8 -> snapped to X [2, 10), Y [2, 8)
    assert face_box((3.2, 2.5, 8.9, 7.1), 1.0, 12, 16, 12, 16) == (2, 2, 10, 8)
    f = _bgr(12, 16, 7)
    redact_ref([(f,)], "bgr", [(3.2, 2.5, 8.9, 7.1)], [1], (12, 16), 12, 16, mode="solid", shape="rect", scale=1.0, fill=(10, 20, 30))
    px = f.reshape(12, 16, 3)
    want = np.full((12, 16, 3), 7, np.uint8)
    want[2:8, 2:10] = (10, 20, 30)
    assert np.array_equal(px, want)
    # scale and a non-integer frame / network ratio: box (8, 4)-(16, 12) in a 32 x 64 network, frame 38 x 50, scale 1.5:
    # cx = 12, hw = 6 -> (6, 18) * 0.78125 = 4.6875, 14.0625 -> 4, 15 -> X [4, 16); cy = 8, hh = 6 -> (2, 14) * 1.1875 = 2.375, 16.625 -> Y [2, 18)
    assert face_box((8, 4, 16, 12), 1.5, 38, 50, 32, 64) == (4, 2, 16, 18)
    # negative odd values snap outwards too: floor(-2.4) = -3 -> -4;  ceil(2.2) = 3 -> 4
    assert face_box((-2.4, -2.4, 2.2, 2.2), 1.0, 12, 16, 12, 16) == (-4, -4, 4, 4)


def test_restatement_ellipse_of_radius_four_pixels():
    # A = Bv = 8: radius 8 half-pixels about the box centre; pixel centres sit at odd offsets, covered iff du^2 + dv^2 <= 64:
    # |dv| = 1 or 3: |du| <= 7 (8 pixels), |dv| = 5: |du| <= 5 (6 pixels; 25 + 49 = 74 > 64), |dv| = 7: |du| <= 3 (4 pixels; 49 + 25 > 64)
    f = _bgr(12, 16, 0)
    redact_ref([(f,)], "bgr", [(4, 2, 12, 10)], [1], (12, 16), 12, 16, mode="solid", shape="ellipse", scale=1.0, fill=(1, 1, 1))
    got = f.reshape(12, 16, 3)[:, :, 0]
    want = np.zeros((12, 16), np.uint8)
    for row, (x0, x1) in zip(range(2, 10), [(6, 10), (5, 11), (4, 12), (4, 12), (4, 12), (4, 12), (5, 11), (6, 10)]):
        want[row, x0:x1] = 1
    assert np.array_equal(got, want) and int(got.sum()) == 52
    assert np.array_equal(got, got[::-1]) and np.array_equal(got[:, 4:12], got[:, 4:12][:, ::-1])       # all four quadrants


def test_restatement_chroma_sample_has_its_own_point_test():
    # the same circle in I420: chroma sample (i, j) is the point (4i+2, 4j+2); about the centre (16, 12) in half-pixels its offsets are
    # +-2 and +-6: (2, 2) -> 8, (2, 6) -> 40, (6, 6) -> 72 > 64, so the four corner samples of the 4 x 4 chroma block stay.  Luma pixel
    # (x, y) = (5, 3) has du = dv = -5 -> 50: covered, while the chroma sample of its quad, (i, j) = (2, 1), du = dv = -6, is not
    y, u, v = np.zeros((12, 16), np.uint8), np.zeros((6, 8), np.uint8), np.zeros((6, 8), np.uint8)
    redact_ref([(y, u, v)], "i420", [(4, 2, 12, 10)], [1], (12, 16), 12, 16, mode="solid", shape="ellipse", scale=1.0, fill=(9, 8, 7))
    want_c = np.zeros((6, 8), bool)
    want_c[2:4, 2:6] = True          # |dv| = 2
    want_c[1, 3:5] = want_c[4, 3:5] = True      # |dv| = 6: |du| = 2 only
    assert np.array_equal(u == 8, want_c) and np.array_equal(v == 7, want_c) and set(np.unique(u)) == {0, 8}
    assert y[3, 5] == 9 and not want_c[1, 2]       # a covered luma pixel whose quad's chroma sample is not covered
    # YV12 holds V first: the first chroma plane takes fill[2]
    y2, c0, c1 = np.zeros((12, 16), np.uint8), np.zeros((6, 8), np.uint8), np.zeros((6, 8), np.uint8)
    redact_ref([(y2, c0, c1)], "yv12", [(4, 2, 12, 10)], [1], (12, 16), 12, 16, mode="solid", shape="ellipse", scale=1.0, fill=(9, 8, 7))
    assert np.array_equal(c0 == 7, want_c) and np.array_equal(c1 == 8, want_c) and np.array_equal(y2, y)
    # and an interleaved plane holds both: NV21 = V, U
    y3, vu = np.zeros((12, 16), np.uint8), np.zeros((6, 16), np.uint8)
    redact_ref([(y3, vu)], "nv21", [(4, 2, 12, 10)], [1], (12, 16), 12, 16, mode="solid", shape="ellipse", scale=1.0, fill=(9, 8, 7))
    assert np.array_equal(vu[:, 0::2] == 7, want_c) and np.array_equal(vu[:, 1::2] == 8, want_c)


def test_restatement_mosaic_edge_cells_average_their_real_samples():
    # frame 10 x 14, m = 4: columns 12..13 and rows 8..9 are edge cells of 2; the grid starts at the frame origin, not at the box
    h, w = 10, 14
    ch = np.arange(h * w, dtype=np.int64).reshape(h, w) % 251
    vals = cell_values(ch, 4)
    assert vals[9, 13] == (ch[8:10, 12:14].sum() + 2) // 4
    assert vals[0, 13] == (ch[0:4, 12:14].sum() + 4) // 8 and vals[9, 0] == (ch[8:10, 0:4].sum() + 4) // 8
    assert vals[5, 6] == (ch[4:8, 4:8].sum() + 8) // 16
    # round half up: a cell of 0, 0, 0, 2 has mean 0.5 -> 1; of 1, 0, 0, 0 has mean 0.25 -> 0
    assert cell_values(np.array([[0, 0], [0, 2]]), 2)[0, 0] == 1 and cell_values(np.array([[1, 0], [0, 0]]), 2)[0, 0] == 0
    f = _bgr(h, w, seed=3)
    before = f.copy()
    # the whole frame, RECT: every pixel takes its cell's value, per channel
    redact_ref([(f,)], "bgr", [(0, 0, 14, 10)], [1], (h, w), h, w, mode="mosaic", shape="rect", cell=4, scale=1.0)
    for c in range(3):
        assert np.array_equal(f[:, c::3], cell_values(before[:, c::3], 4))
    assert len(np.unique(f[8:10, 36:42:3])) == 1
    # a box inside: covered pixels take the FRAME cell's value, pixels of the same cell outside the box stay
    g = before.copy()
    redact_ref([(g,)], "bgr", [(2, 2, 6, 6)], [1], (h, w), h, w, mode="mosaic", shape="rect", cell=4, scale=1.0)
    gp, bp = g.reshape(h, w, 3), before.reshape(h, w, 3)
    assert np.array_equal(gp[2:6, 2:6, 0], cell_values(before[:, 0::3], 4)[2:6, 2:6])
    keep = np.ones((h, w), bool)
    keep[2:6, 2:6] = False
    assert np.array_equal(gp[keep], bp[keep])


def test_restatement_overlap_and_order_do_not_matter():
    boxes = np.float32([(2, 1, 9, 8), (6, 4, 13, 9)])
    for mode, shape in (("mosaic", "ellipse"), ("mosaic", "rect"), ("solid", "ellipse")):
        a, b = _bgr(10, 14, seed=5), _bgr(10, 14, seed=5)
        redact_ref([(a,)], "bgr", boxes, [2], (10, 14), 10, 14, mode=mode, shape=shape, cell=4, scale=1.0, fill=(1, 2, 3))
        redact_ref([(b,)], "bgr", boxes[::-1], [2], (10, 14), 10, 14, mode=mode, shape=shape, cell=4, scale=1.0, fill=(1, 2, 3))
        assert np.array_equal(a, b) and not np.array_equal(a, _bgr(10, 14, seed=5))


def test_restatement_skipped_and_clamped_boxes():
    f = _bgr(10, 14, seed=6)
    before = f.copy()
    nothing = np.float32([(20, 3, 30, 8), (np.nan, 1, 5, 5), (1, 1, np.inf, 5), (4, 2, 4, 9), (9, 2, 3, 9), (-30, -30, -20, -20)])
    assert face_box(nothing[1], 1.3, 10, 14, 10, 14) is None and face_box(nothing[2], 1.3, 10, 14, 10, 14) is None
    assert face_box(nothing[3], 1.3, 10, 14, 10, 14) is None and face_box(nothing[4], 1.3, 10, 14, 10, 14) is None      # x2 == x1, x2 < x1
    redact_ref([(f,)], "bgr", nothing, [6], (10, 14), 10, 14, mode="solid", shape="ellipse", fill=(1, 2, 3))
    assert np.array_equal(f, before)
    # a box so large that the clamp acts: finite, and it covers the frame
    big = face_box((-3e38, -3e38, 3e38, 3e38), 4.0, 8192, 8192, 32, 32)
    assert big == (-8192, -8192, 16384, 16384)
    redact_ref([(f,)], "bgr", [(-1e30, -1e30, 1e30, 1e30)], [1], (10, 14), 10, 14, mode="solid", shape="ellipse", fill=(1, 2, 3))
    assert np.array_equal(f.reshape(10, 14, 3), np.broadcast_to(np.uint8([1, 2, 3]), (10, 14, 3)))


# ------------------------------------------------------------------------------------------ on the GPU: the kernels alone
NET = (32, 64)
# image 0: an interior box, one that overlaps it and shares mosaic cells with it, one cut by the left and top edges, one cut by the
# right and bottom edges; image 1: none; image 2: a one-network-pixel box, a NaN box, a box outside the frame
BOXES = np.float32([(20, 10, 34, 20), (30, 14, 44, 24), (-3, -2, 9, 7), (52, 24, 70, 40),
                    (12, 25, 13, 26), (np.nan, 3, 8, 9), (80, 40, 95, 50)])
COUNTS = np.array([4, 0, 3], np.int32)


def _reversed_rows(boxes, counts):
    out, at = [], 0
    for n in counts:
        out.append(boxes[at:at + n][::-1])
        at += n
    return np.concatenate(out)


def _op_case(fmt, h, w, dense, boxes, counts, net, **opt):
    rng = np.random.default_rng(7)
    p0, p1 = pitches_for(fmt, w)
    fr = Frames(rng, fmt, len(counts), h, w, p0, p1, dense)
    want = fr.clone()
    before = fr.clone()
    redact_ref(want.views, fmt, boxes, counts, net, h, w, **opt)
    out = ops.redact_faces(fr.arg, boxes, counts, net, fmt=fmt, **opt)
    assert out is fr.arg
    assert fr.same(want), (fmt, dense, opt, fr.diff(want))
    return fr, before


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_op_redact_bit_exact(fmt):
    """cf_op_redact against the restatement on every byte (padding and guard included): SOLID / MOSAIC x RECT / ELLIPSE, m = 2 and 6,
    pitched planes and the dense form, B = 3 with counts [4, 0, 3]; the boxes in reversed order give identical bytes."""
    h, w = 38, 50
    changed = 0
    for dense in (False, True):
        for shape in ("rect", "ellipse"):
            cases = [dict(mode="solid", shape=shape, fill=(17, 130, 251))] + [dict(mode="mosaic", shape=shape, cell=m) for m in (2, 6)]
            for opt in cases:
                fr, before = _op_case(fmt, h, w, dense, BOXES, COUNTS, NET, **opt)
                rev, _ = _op_case(fmt, h, w, dense, _reversed_rows(BOXES, COUNTS), COUNTS, NET, **opt)
                assert rev.same(fr), (fmt, dense, opt, rev.diff(fr))
                assert not fr.same(before)
                changed += 1
                # image 1 has no faces, and of image 2 only the one-pixel box writes
                n = len(fr.geo)
                if not dense:
                    assert all(np.array_equal(a, b) for a, b in zip(fr.bufs[n:2 * n], before.bufs[n:2 * n]))
                    if opt["mode"] == "solid":
                        assert not np.array_equal(fr.bufs[2 * n], before.bufs[2 * n])
    assert changed == 12
    # no faces at all: nothing happens
    fr, before = _op_case(fmt, h, w, False, np.zeros((0, 4), np.float32), np.zeros(3, np.int32), NET)
    assert fr.same(before)


@pytest.mark.gpu
def test_op_redact_small_then_large_grid():
    """The smallest frame with m = 2, then a 128 x 256 frame with m = 2 (a cell grid hundreds of times larger) in one process; also the
    default options, a scale at each end of its range and a box that the clamp cuts."""
    tiny = np.float32([(0, 0, 2, 2), (0.5, 0.5, 1.5, 1.5)])
    for fmt in ("bgr", "nv12", "i420"):
        _op_case(fmt, 2, 2, False, tiny, np.array([2], np.int32), (2, 2), mode="mosaic", shape="rect", cell=2, scale=1.0)
    rng = np.random.default_rng(11)
    n = 9
    ctr = rng.uniform((0, 0), (64, 32), (n, 2))
    half = rng.uniform(1.0, 9.0, (n, 2))
    boxes = np.concatenate([ctr - half, ctr + half], 1).astype(np.float32)
    boxes[0] = (-1e30, 5, 1e30, 9)                       # clamped: a band over the full width
    counts = np.array([5, 4], np.int32)
    for fmt in FORMATS:
        _op_case(fmt, 128, 256, fmt == "nv12", boxes, counts, NET, mode="mosaic", shape="ellipse", cell=2)
    _op_case("bgr", 128, 256, True, boxes, counts, NET)                                  # the defaults: mosaic, ellipse, 20, 1.3
    _op_case("nv12", 128, 256, False, boxes, counts, NET, mode="mosaic", shape="rect", cell=256, scale=4.0)
    _op_case("yv12", 128, 256, False, boxes, counts, NET, mode="solid", shape="ellipse", scale=0.25, fill=(1, 2, 3))
    _op_case("bgr", 37, 51, False, BOXES, COUNTS, NET, mode="mosaic", shape="ellipse", cell=6)        # BGR frames may be odd


# More frames than one launch takes (32): a face in frame 0 and in frame 31 (the first launch's last), two in frame 32 (the second
# launch's only frame: its boxes, counts and mosaic cells sit at the launch's offsets), one of them overhanging the right and bottom
# edges; frames 1..30 have none.  Frame = network = 16 x 16.
CHUNK_COUNTS = np.array([1] + [0] * 30 + [1, 2], np.int32)
CHUNK_BOXES = np.float32([(2, 3, 9, 11), (5, 1, 13, 8), (1, 2, 7, 9), (10, 9, 19, 18)])


def chunk_case(case, fmt, **opt):
    """``case`` = this module's or test_blur's _op_case on the 33 frames: every byte equals the restatement, and exactly the frames
    0, 31 and 32 change."""
    fr, before = case(fmt, 16, 16, False, CHUNK_BOXES, CHUNK_COUNTS, (16, 16), **opt)
    n = len(fr.geo)
    changed = [b for b in range(33) if not all(np.array_equal(x, y) for x, y in zip(fr.bufs[b * n:(b + 1) * n], before.bufs[b * n:(b + 1) * n]))]
    assert changed == [0, 31, 32], changed


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ("nv12", "bgr"))
def test_op_redact_more_frames_than_one_launch(fmt):
    chunk_case(_op_case, fmt, mode="mosaic", shape="ellipse", cell=4, scale=1.0)


# ------------------------------------------------------------------------------------------ on the GPU: the engine
def source_frames(rng, kind, shape):
    """uint8 frames: uniform noise, noise of the two extreme levels, or 4-pixel runs of one noise value along axes 1 and 2 (coarse noise
    that survives a resize) -- the default weights answer to fine detail, so one of them keeps faces."""
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "binary":
        return rng.choice(np.array([0, 255], np.uint8), shape)
    small = tuple((n + 3) // 4 if a in (1, 2) else n for a, n in enumerate(shape))
    a = rng.integers(0, 256, small, dtype=np.uint8)
    for k in (1, 2):
        a = np.repeat(a, 4, axis=k)
    return np.ascontiguousarray(a[tuple(slice(0, n) for n in shape)])


SOURCES = (("noise", (75, 101)), ("binary", (75, 101)), ("blocks", (75, 101)), ("binary", (96, 127)), ("noise", (192, 256)),
           ("binary", (192, 256)), ("blocks", (150, 200)))


def _feed_until_faces(eng, how, rng, need=2):
    """The first of SOURCES whose forward (``how``: 'resized' BGR sources of any size, 'yuv' NV12 frames of the even size, 'float' a
    normalised NCHW tensor) + threshold decode in network coordinates keeps ``need`` faces: (source frames, decode result)."""
    tried = []
    for kind, hw in SOURCES:
        if how == "resized":
            src = source_frames(rng, kind, (3,) + hw + (3,))
            eng.forward_resized_enqueue(src)
        elif how == "yuv":
            h, w = (hw[0] + 1) // 2 * 2, (hw[1] + 1) // 2 * 2
            src = source_frames(rng, kind, (3, h * 3 // 2, w))
            eng.forward_yuv_enqueue(src, "nv12")
        else:
            src = source_frames(rng, kind, (3, eng.H, eng.W, 3))
            x = (src.astype(np.float32) / 255.0 - cfa.CenterFace.mean) / cfa.CenterFace.std
            eng.forward_enqueue(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))
        base = eng.decode_threshold(0.3, 0.3, 64)
        tried.append((kind, hw, [len(d) for d, _ in base]))
        if sum(len(d) for d, _ in base) >= need:
            return src, base
    raise AssertionError("no source kept %d faces with the default weights: %s" % (need, tried))


def _net_boxes(base):
    return np.concatenate([d[:, :4] for d, _ in base]), np.array([len(d) for d, _ in base], np.int32)


def _engine_case(eng, fmt, h, w, boxes, counts, dense, **opt):
    rng = np.random.default_rng(13)
    p0, p1 = pitches_for(fmt, w)
    fr = Frames(rng, fmt, len(counts), h, w, p0, p1, dense)
    want = fr.clone()
    redact_ref(want.views, fmt, boxes, counts, (eng.H, eng.W), h, w, **opt)
    assert eng.redact_faces(fr.arg, fmt, **opt) is fr.arg
    assert fr.same(want), (fmt, opt, fr.diff(want))
    return fr


@pytest.mark.gpu
@pytest.mark.parametrize("how", ("resized", "yuv"))
def test_engine_redact_equals_restatement(how):
    """Engine.redact_faces behind forward_resized_enqueue / forward_yuv_enqueue + decode_threshold, default weights, context 64 x 96:
    bit for bit the restatement on the decode's NETWORK-coordinate boxes, with set_rescale off and on; only the first kept row with
    max_out = 1; the decode's outputs are those of a decode taken before any redaction."""
    rng = np.random.default_rng(("resized", "yuv").index(how))
    eng = cfa.Engine(64, 96, max_batch=3, dtype="bf16")
    L, P = cfa._lib.lib(), cfa._lib.ptr
    src, base = _feed_until_faces(eng, how, rng)
    boxes, counts = _net_boxes(base)
    assert int(counts.sum()) >= 2
    fmt = "bgr" if how == "resized" else "nv12"
    h, w = (76, 102) if how == "resized" else (src.shape[1] * 2 // 3, src.shape[2])
    opts = (dict(mode="mosaic", shape="ellipse", cell=2), dict(mode="mosaic", shape="rect", cell=6), dict(mode="solid", shape="ellipse", fill=(3, 99, 201)),
            dict())
    outs = []
    for opt in opts:                                        # m = 2 first: the next grids are smaller, the 128 x 256 one below grows it
        outs.append(_engine_case(eng, fmt, h, w, boxes, counts, False, **opt))
    _engine_case(eng, fmt, 128, 256, boxes, counts, True, mode="mosaic", shape="ellipse", cell=2)
    if how == "resized":
        _engine_case(eng, "bgr", 75, 101, boxes, counts, True, mode="mosaic", shape="ellipse", cell=6)     # the odd source size itself
        _engine_case(eng, "i420", 76, 102, boxes, counts, False, mode="mosaic", shape="ellipse", cell=6)   # any format behind any feed
    # the decode's outputs are unchanged by the calls
    again = eng.decode_threshold(0.3, 0.3, 64)
    for (d, l), (d0, l0) in zip(again, base):
        assert d.tobytes() == d0.tobytes() and l.tobytes() == l0.tobytes()
    # set_rescale on: the decode's boxes change, the redaction does not
    eng.set_rescale(1.37, 1.21)
    scaled = eng.decode_threshold(0.3, 0.3, 64)
    assert [len(d) for d, _ in scaled] == list(counts)
    assert np.array_equal(np.concatenate([d[:, 0] for d, _ in scaled]), np.floor(boxes[:, 0].astype(np.float64) / np.float64(np.float32(1.21))).astype(np.float32))
    for opt, first in zip(opts, outs):
        assert _engine_case(eng, fmt, h, w, boxes, counts, False, **opt).same(first)
    eng.set_rescale(0.0, 0.0)
    # a decode that wrote one row per image: only the first kept row of each image is redacted
    d5, l10, cn = np.empty((3, 1, 5), np.float32), np.empty((3, 1, 10), np.float32), np.empty(3, np.int32)
    assert L.cf_decode_threshold(eng._h, 0.3, 0.3, 1, P(d5), P(l10), P(cn)) == 0
    assert np.array_equal(cn, counts)
    c1 = np.minimum(counts, 1)
    firsts = np.concatenate([d[:1, :4] for d, _ in base])
    _engine_case(eng, fmt, h, w, firsts, c1, False, mode="solid", shape="rect", fill=(1, 2, 3))
    eng.close()


@pytest.mark.gpu
def test_engine_redact_state_errors_float_forward_and_device_form():
    rng = np.random.default_rng(5)
    eng = cfa.Engine(64, 96, max_batch=3, dtype="bf16")
    frames = rng.integers(0, 256, (3, 76, 102, 3), dtype=np.uint8)

    def refused():
        keep = frames.copy()
        with pytest.raises(cfa._lib.CenterFaceError) as e:
            eng.redact_faces(keep, "bgr")
        assert e.value.code == cfa._lib.CF_ESTATE and np.array_equal(keep, frames)
    refused()                                                              # before any forward
    x = source_frames(rng, "binary", (3, 64, 96, 3))
    eng.forward_enqueue(x)
    refused()                                                              # before any threshold decode
    eng.decode_topk(10)
    refused()
    eng.decode_threshold(0.3, 0.3, 64)
    eng.redact_faces(frames.copy(), "bgr")
    eng.forward_enqueue(x)
    refused()                                                              # a new forward was enqueued: the decode is gone
    eng.decode_threshold(0.3, 0.3, 64)
    eng.upload_images(list(x))
    refused()                                                              # an upload was started
    with pytest.raises(ValueError):
        eng.forward_enqueue(x), eng.decode_threshold(0.3, 0.3, 64), eng.redact_faces(frames[:2].copy(), "bgr")      # B is not the forward's
    with pytest.raises(ValueError):
        eng.redact_faces(frames.copy(), "bgr", cell=7)
    # behind a float NCHW forward: the input batch is not read, so it works
    src, base = _feed_until_faces(eng, "float", rng)
    boxes, counts = _net_boxes(base)
    host = _engine_case(eng, "bgr", 76, 102, boxes, counts, False, mode="mosaic", shape="ellipse", cell=6)
    # the device form on planes from device_alloc equals the host form, padding included
    for fmt in ("bgr", "nv12", "yv12"):
        p0, p1 = pitches_for(fmt, 102, aligned=True)
        fr = Frames(np.random.default_rng(13), fmt, 3, 76, 102, p0, p1, False)
        want = fr.clone()
        eng.redact_faces(want.arg, fmt, mode="mosaic", shape="ellipse", cell=6)
        ref = fr.clone()
        redact_ref(ref.views, fmt, boxes, counts, (64, 96), 76, 102, mode="mosaic", shape="ellipse", cell=6)
        assert want.same(ref), (fmt, want.diff(ref))
        dev = [eng.device_alloc(b.nbytes) for b in fr.bufs]
        for d, b in zip(dev, fr.bufs):
            eng.memcpy_h2d(d, b)
        n = len(fr.geo)
        eng.redact_faces_device([tuple(dev[b * n:(b + 1) * n]) for b in range(3)], fmt, 3, 76, 102, p0, p1, mode="mosaic", shape="ellipse", cell=6)
        eng.synchronize()
        for d, b in zip(dev, fr.bufs):
            eng.memcpy_d2h(b, d)
        assert fr.same(want), (fmt, fr.diff(want))
        with pytest.raises(ValueError):                                    # a misaligned device plane, a pitch that is no multiple of 4
            eng.redact_faces_device([(dev[b * n] + 2,) + tuple(dev[b * n + 1:(b + 1) * n]) for b in range(3)], fmt, 3, 76, 102, p0, p1)
        with pytest.raises(ValueError):
            eng.redact_faces_device([tuple(dev[b * n:(b + 1) * n]) for b in range(3)], fmt, 3, 76, 102, p0 + 2, p1)
        for d in dev:
            eng.device_free(d)
    del host
    eng.close()


@pytest.mark.gpu
def test_centerface_anonymize():
    """anonymize / anonymize_yuv: inputs untouched, detections those of detect_batch / detect_yuv, outputs = the restatement on the
    network boxes of the same forward; an image without detections comes back byte for byte."""
    rng = np.random.default_rng(31)
    sd = cfa.weights.synthetic_state_dict(0)
    hw = (76, 102)
    face = cfa.CenterFace(*hw, dtype="bf16", max_batch=3)
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        imgs = list(source_frames(rng, kind, (3,) + hw + (3,)))
        want = face.detect_batch(imgs)
        if sum(len(d) for d, _ in want) >= 1:
            break
    keep = [im.copy() for im in imgs]
    out, dets = face.anonymize(imgs, mode="mosaic", shape="ellipse", cell=6)
    assert all(np.array_equal(a, b) for a, b in zip(imgs, keep))
    assert out.shape == (3,) + hw + (3,) and out.dtype == np.uint8
    n = 0
    for (d, l), (wd, wl) in zip(dets, want):
        assert d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes()
        n += len(d)
    assert n >= 1
    base = face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets)     # the same forward, network coordinates
    boxes, counts = _net_boxes(base)
    assert list(counts) == [len(d) for d, _ in dets]
    ref = np.stack(keep)
    redact_ref([(f.reshape(hw[0], -1),) for f in ref], "bgr", boxes, counts, (face.img_h_new, face.img_w_new), hw[0], hw[1], mode="mosaic", shape="ellipse", cell=6)
    assert np.array_equal(out, ref) and not np.array_equal(out, np.stack(keep))
    # 4:2:0
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        yuv = source_frames(rng, kind, (3, hw[0] * 3 // 2, hw[1]))
        wanty = face.detect_yuv(yuv, "nv12")
        if sum(len(d) for d, _ in wanty) >= 1:
            break
    keepy = yuv.copy()
    outy, detsy = face.anonymize_yuv(yuv, "nv12", mode="solid", shape="rect", fill=(16, 128, 128))
    assert np.array_equal(yuv, keepy) and outy.shape == yuv.shape
    for (d, l), (wd, wl) in zip(detsy, wanty):
        assert d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes()
    boxes, counts = _net_boxes(face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets))
    assert int(counts.sum()) >= 1
    refy = keepy.copy()
    redact_ref([(f[:hw[0]], f[hw[0]:]) for f in refy], "nv12", boxes, counts, (face.img_h_new, face.img_w_new), hw[0], hw[1], mode="solid", shape="rect", fill=(16, 128, 128))
    assert np.array_equal(outy, refy) and not np.array_equal(outy, keepy)
    face.close()
    # no detections: a heat-map bias far below the threshold
    quiet = dict(sd)
    quiet["hm.1.bias"] = sd["hm.1.bias"] - np.float32(100.0)
    face = cfa.CenterFace(*hw, dtype="bf16", max_batch=3, weights=quiet)
    out, dets = face.anonymize(imgs)
    assert np.array_equal(out, np.stack(keep)) and all(d.shape == (0, 5) for d, _ in dets)
    outy, _ = face.anonymize_yuv(yuv, "nv12")
    assert np.array_equal(outy, keepy)
    face.close()
