"""Blur redaction in the source frame (cf_blur_faces / cf_op_blur, csrc/cf_blur.hip): the arithmetic restated in numpy, known answers of
the restatement, and the device against the restatement bit for bit -- on every byte of every buffer, pitch padding and a guard band
behind each plane included.

The statement (include/centerface_hip.h has it in full): faces, boxes and coverage are those of the redaction (tests/test_redact.py:
face_box, coverage).  A covered sample becomes (S + D/2) / D with S the sum over the (6r+1)^2 neighbourhood of the UNTOUCHED plane,
border samples replicated, weighted by the outer product of the taps box_b * box_b * box_b, b = 2r+1, D = b^6; per channel; chroma
planes use (r+1)/2.  radius = 0: r_f = clamp(min(A, Bv) / 8, 1, 24) per face, and a sample takes the largest r_f among the faces that
cover it."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from test_redact import (FORMATS, Frames, face_box, coverage, plane_passes, pitches_for, source_frames, BOXES, COUNTS, NET, _reversed_rows,
                         _feed_until_faces, _net_boxes, chunk_case)


# ------------------------------------------------------------------------------------------ the restatement
def taps(r):
    """box_b * box_b * box_b, b = 2r+1, by integer convolution: 6r+1 taps."""
    box = np.ones(2 * r + 1, np.int64)
    return np.convolve(np.convolve(box, box), box)


def blur_plane(ch, r):
    """[rows, cols] uint8 -> int64 [rows, cols]: every sample's blurred value at strength r, borders replicated, one rounding."""
    t, R, D = taps(r), 3 * r, (2 * r + 1) ** 6
    rows, cols = ch.shape
    p = np.pad(ch.astype(np.int64), R, mode="edge")
    hs = sum(t[i] * p[:, i:i + cols] for i in range(2 * R + 1))
    S = sum(t[j] * hs[j:j + rows] for j in range(2 * R + 1))
    return (S + D // 2) // D


def face_r(fb, radius):
    if radius:
        return int(radius)
    return min(max(min(fb[2] - fb[0], fb[3] - fb[1]) // 8, 1), 24)


def blur_ref(frames, fmt, boxes, counts, net_hw, h, w, shape="ellipse", radius=0, scale=1.3):
    """The restatement, in place on ``frames`` = per frame a tuple of 2-D uint8 row views, as test_redact.redact_ref takes them."""
    H, W = net_hw
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    at = 0
    for b, planes in enumerate(frames):
        fboxes = [face_box(bx, scale, h, w, H, W) for bx in boxes[at:at + int(counts[b])]]
        fboxes = [fb for fb in fboxes if fb is not None]
        at += int(counts[b])
        for k, bps, chroma, _ in plane_passes(fmt):
            view = planes[k]
            rows, cols = (h // 2, w // 2) if chroma else (h, w)
            assert view.shape == (rows, cols * bps)
            rstar = np.zeros((rows, cols), np.int64)                    # the largest r among the faces that cover the sample; 0 = none
            for fb in fboxes:
                cov = coverage([fb], shape, rows, cols, chroma)
                rstar[cov] = np.maximum(rstar[cov], face_r(fb, radius))
            for c in range(bps):
                ch = view[:, c::bps]                                    # a view: one channel of the plane
                src = ch.copy()                                         # the plane as it was before the call
                for r in np.unique(rstar[rstar > 0]):
                    val = blur_plane(src, (int(r) + 1) // 2 if chroma else int(r))
                    m = rstar == r
                    ch[m] = val[m]
    return frames


# ------------------------------------------------------------------------------------------ known answers of the restatement
def test_restatement_taps():
    assert taps(1).tolist() == [1, 3, 6, 7, 6, 3, 1]
    for r in (1, 2, 5, 24):
        t, b = taps(r), 2 * r + 1
        assert len(t) == 6 * r + 1 and int(t.sum()) == b ** 3 and np.array_equal(t, t[::-1])
        k = np.arange(-3 * r, 3 * r + 1)
        assert int((t * k * k).sum()) == b ** 3 * r * (r + 1)          # variance r(r+1): sigma is about r
    assert 255 * 49 ** 3 < 2 ** 31 and 255 * 49 ** 6 < 2 ** 63


def test_restatement_constant_frame_and_impulse():
    for fmt, shp in (("bgr", (24, 96)), ("nv12", (24, 32))):
        planes = (np.full(shp, 77, np.uint8),) if fmt == "bgr" else (np.full(shp, 77, np.uint8), np.full((12, 32), 200, np.uint8))
        keep = [p.copy() for p in planes]
        blur_ref([planes], fmt, [(4, 3, 28, 21)], [1], (24, 32), 24, 32, shape="ellipse", radius=5)
        assert all(np.array_equal(a, b) for a, b in zip(planes, keep))
    # a single 255 in a large RECT: the taps' outer product, rounded once
    for r in (1, 2, 5):
        h = w = 64
        f = np.zeros((h, 3 * w), np.uint8)
        f[30, 3 * 33 + 1] = 255                                        # green of pixel (33, 30)
        blur_ref([(f,)], "bgr", [(0, 0, w, h)], [1], (h, w), h, w, shape="rect", radius=r, scale=1.0)
        t, D, R = taps(r), (2 * r + 1) ** 6, 3 * r
        want = (255 * np.outer(t, t) + D // 2) // D
        g = f[:, 1::3].astype(np.int64)
        assert np.array_equal(g[30 - R:30 + R + 1, 33 - R:33 + R + 1], want)
        assert int(g.sum()) == int(want.sum()) and not f[:, 0::3].any() and not f[:, 2::3].any()
    # the border replicates: a frame whose rows are constant stays as it is along x, and a left edge step keeps its outer level
    f = np.repeat(np.arange(0, 240, 10, dtype=np.uint8)[:, None], 3 * 32, 1)
    g = f.copy()
    blur_ref([(g,)], "bgr", [(0, 0, 32, 24)], [1], (24, 32), 24, 32, shape="rect", radius=2, scale=1.0)
    assert (g == g[:, :1]).all() and g[0, 0] == blur_plane(f[:, 0::3], 2)[0, 0] and 0 < g[0, 0] < 30


def test_restatement_overlap_order_and_duplicates_do_not_matter():
    rng = np.random.default_rng(5)
    boxes = np.float32([(2, 1, 22, 17), (12, 8, 30, 23), (20, 2, 31, 9)])
    for radius, shape in ((0, "ellipse"), (0, "rect"), (3, "ellipse")):
        src = rng.integers(0, 256, (24, 96), dtype=np.uint8)
        a, b, c = src.copy(), src.copy(), src.copy()
        blur_ref([(a,)], "bgr", boxes, [3], (24, 32), 24, 32, shape=shape, radius=radius, scale=1.0)
        blur_ref([(b,)], "bgr", boxes[::-1], [3], (24, 32), 24, 32, shape=shape, radius=radius, scale=1.0)
        blur_ref([(c,)], "bgr", np.concatenate([boxes, boxes[:1]]), [4], (24, 32), 24, 32, shape=shape, radius=radius, scale=1.0)
        assert np.array_equal(a, b) and np.array_equal(a, c) and not np.array_equal(a, src)


def test_restatement_auto_radius_takes_the_largest_covering_face():
    # 64 x 64 frame = network: a 16 x 16 box (r_f = 2) inside a 48 x 40 one (r_f = 5): the intersection carries r = 5
    small, large = (8, 8, 24, 24), (4, 4, 52, 44)
    assert face_r(face_box(small, 1.0, 64, 64, 64, 64), 0) == 2 and face_r(face_box(large, 1.0, 64, 64, 64, 64), 0) == 5
    assert face_r((0, 0, 6, 400), 0) == 1 and face_r((0, 0, 400, 300), 0) == 24 and face_r((0, 0, 400, 300), 7) == 7
    src = np.random.default_rng(3).integers(0, 256, (64, 64), dtype=np.uint8)
    y, uv = src.copy(), np.random.default_rng(4).integers(0, 256, (32, 64), dtype=np.uint8)
    uv0 = uv.copy()
    blur_ref([(y, uv)], "nv12", [small, large], [2], (64, 64), 64, 64, shape="rect", radius=0, scale=1.0)
    assert np.array_equal(y[4:44, 4:52], blur_plane(src, 5)[4:44, 4:52])            # the small face's pixels too
    only_small = src.copy()
    blur_ref([(only_small, uv0.copy())], "nv12", [small], [1], (64, 64), 64, 64, shape="rect", radius=0, scale=1.0)
    assert np.array_equal(only_small[8:24, 8:24], blur_plane(src, 2)[8:24, 8:24]) and not np.array_equal(only_small[8:24, 8:24], y[8:24, 8:24])
    # chroma: r_c = (5+1)/2 = 3 on the 32 x 32 grid, each interleaved channel by itself
    for c in (0, 1):
        assert np.array_equal(uv[2:22, 2 * 2 + c:2 * 26:2], blur_plane(uv0[:, c::2], 3)[2:22, 2:26])
    assert np.array_equal(uv[22:], uv0[22:]) and np.array_equal(uv[:2], uv0[:2])


def test_restatement_chroma_sample_has_its_own_point_test_and_radius():
    # the circle of test_redact's chroma test: A = Bv = 8 about (16, 12) half-pixels: chroma samples at +-2, +-6: the corners of the
    # 4 x 4 block (72 > 64) stay; luma (5, 3) is covered while its quad's chroma sample (2, 1) is not.  r = 4 -> r_c = 2; r = 3 -> 2 too
    rng = np.random.default_rng(8)
    y0, u0, v0 = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((12, 16), (6, 8), (6, 8)))
    want_c = np.zeros((6, 8), bool)
    want_c[2:4, 2:6] = True
    want_c[1, 3:5] = want_c[4, 3:5] = True
    for r in (4, 3):
        y, u, v = y0.copy(), u0.copy(), v0.copy()
        blur_ref([(y, u, v)], "i420", [(4, 2, 12, 10)], [1], (12, 16), 12, 16, shape="ellipse", radius=r, scale=1.0)
        for got, src in ((u, u0), (v, v0)):
            assert np.array_equal(got[want_c], blur_plane(src, 2)[want_c]) and np.array_equal(got[~want_c], src[~want_c])
        assert y[3, 5] == blur_plane(y0, r)[3, 5] and u[1, 2] == u0[1, 2]
        assert (y != y0).sum() <= 52


# ------------------------------------------------------------------------------------------ on the GPU: the kernels alone
def _op_case(fmt, h, w, dense, boxes, counts, net, **opt):
    rng = np.random.default_rng(7)
    p0, p1 = pitches_for(fmt, w)
    fr = Frames(rng, fmt, len(counts), h, w, p0, p1, dense)
    want = fr.clone()
    before = fr.clone()
    blur_ref(want.views, fmt, boxes, counts, net, h, w, **opt)
    out = ops.blur_faces(fr.arg, boxes, counts, net, fmt=fmt, **opt)
    assert out is fr.arg
    assert fr.same(want), (fmt, dense, opt, fr.diff(want))
    return fr, before


# image 0: test_redact's four boxes (an interior one, one that overlaps it, one cut by the left and top edges, one cut by the right and
# bottom edges); image 1: none; image 2: a one-network-pixel box, a NaN row, an empty row (x2 == x1)
BLUR_BOXES = np.concatenate([BOXES[:6], np.float32([(40, 10, 40, 20)])])
BLUR_COUNTS = COUNTS
assert BLUR_COUNTS.tolist() == [4, 0, 3] and np.isnan(BLUR_BOXES[5, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_op_blur_bit_exact(fmt):
    """cf_op_blur against the restatement on every byte (padding and guard included): RECT / ELLIPSE x r = 1, 2, 5, 24 and the per-face
    radius, pitched unaligned planes, B = 3 with faces in images 0 and 2 only; the rows reversed give identical bytes.  At r = 24 the
    halo (72) exceeds the tile and clamps on both sides of the 75 / 74-row frame at once."""
    h, w = (75, 101) if fmt == "bgr" else (74, 100)
    boxes = BLUR_BOXES
    n = 0
    for shape in ("rect", "ellipse"):
        for radius in (1, 2, 5, 24, 0):
            opt = dict(shape=shape, radius=radius)
            fr, before = _op_case(fmt, h, w, False, boxes, BLUR_COUNTS, NET, **opt)
            rev, _ = _op_case(fmt, h, w, False, _reversed_rows(boxes, BLUR_COUNTS), BLUR_COUNTS, NET, **opt)
            assert rev.same(fr), (fmt, opt, rev.diff(fr))
            assert not fr.same(before)
            k = len(fr.geo)                                            # image 1 has no faces: its buffers are untouched
            assert all(np.array_equal(a, b) for a, b in zip(fr.bufs[k:2 * k], before.bufs[k:2 * k]))
            n += 1
    assert n == 10
    _op_case(fmt, h, w, True, boxes, BLUR_COUNTS, NET, shape="ellipse", radius=5)                   # the dense form
    fr, before = _op_case(fmt, h, w, False, np.zeros((0, 4), np.float32), np.zeros(3, np.int32), NET)     # no faces at all
    assert fr.same(before)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ("bgr", "nv12", "yv12"))
def test_op_blur_auto_radius_overlaps(fmt):
    """radius = 0 on a 192 x 256 frame (network 48 x 64, factor 4, scale 1): boxes with min(A, Bv) / 8 = 1, 3 and 30 (capped at 24)
    that overlap pairwise, a second face of r = 3 over the first (equal r: both store the same value), and a face of r = 1 wholly
    inside the large one (every one of its samples is skipped)."""
    h, w = 192, 256
    boxes = np.float32([(10, 8, 13, 30),        # 12 x 88 pixels: r = 1, crosses the next two
                        (6, 10, 14, 16),        # 32 x 24: r = 3
                        (8, 12, 15, 19),        # 28 x 28: r = 3, overlaps the previous
                        (11, 2, 75, 62),        # 256 x 240, cut by the right edge: 240 / 8 = 30 -> 24
                        (30, 30, 33, 33),       # 12 x 12: r = 1, inside the large one
                        (2, 40, 12.5, 47)])     # 42 x 28: r = 3, meets the large one and the first
    rs = [face_r(face_box(bx, 1.0, h, w, 48, 64), 0) for bx in boxes]
    assert rs == [1, 3, 3, 24, 1, 3], rs
    counts = np.array([6], np.int32)
    for shape in ("ellipse", "rect"):
        fr, before = _op_case(fmt, h, w, False, boxes, counts, (48, 64), shape=shape, radius=0, scale=1.0)
        rev, _ = _op_case(fmt, h, w, False, boxes[::-1], counts, (48, 64), shape=shape, radius=0, scale=1.0)
        assert rev.same(fr) and not fr.same(before)


@pytest.mark.gpu
def test_op_blur_small_then_large_frame():
    """The smallest frames first, then 128 x 256 ones in the same process; the default options, a scale at each end of its range and a
    box that the clamp cuts."""
    tiny = np.float32([(0, 0, 2, 2), (0.5, 0.5, 1.5, 1.5)])
    for fmt in ("bgr", "nv12", "i420"):
        _op_case(fmt, 2, 2, False, tiny, np.array([2], np.int32), (2, 2), shape="rect", radius=24, scale=1.0)
    _op_case("bgr", 1, 1, False, tiny, np.array([2], np.int32), (2, 2), shape="rect", radius=0, scale=1.0)
    rng = np.random.default_rng(11)
    n = 9
    ctr = rng.uniform((0, 0), (64, 32), (n, 2))
    half = rng.uniform(1.0, 9.0, (n, 2))
    boxes = np.concatenate([ctr - half, ctr + half], 1).astype(np.float32)
    boxes[0] = (-1e30, 5, 1e30, 9)                       # clamped: a band over the full width
    counts = np.array([5, 4], np.int32)
    for fmt in FORMATS:
        _op_case(fmt, 128, 256, fmt == "nv12", boxes, counts, NET)                       # the defaults: ellipse, per-face radius, 1.3
    _op_case("nv12", 128, 256, False, boxes, counts, NET, shape="rect", radius=8, scale=4.0)
    _op_case("yv12", 128, 256, False, boxes, counts, NET, shape="ellipse", radius=2, scale=0.25)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ("nv12", "bgr"))
def test_op_blur_more_frames_than_one_launch(fmt):
    """test_redact's 33 frames with the per-face radius: frame 32 is the second launch's, which reads its face list (the skip rule
    walks it) and its scratch at the launch's offsets."""
    chunk_case(_op_case, fmt, shape="ellipse", radius=0, scale=1.0)


# ------------------------------------------------------------------------------------------ on the GPU: the engine
def _engine_case(eng, fmt, h, w, boxes, counts, dense, net=None, **opt):
    rng = np.random.default_rng(13)
    p0, p1 = pitches_for(fmt, w)
    fr = Frames(rng, fmt, len(counts), h, w, p0, p1, dense)
    want = fr.clone()
    blur_ref(want.views, fmt, boxes, counts, net or (eng.H, eng.W), h, w, **opt)
    assert eng.blur_faces(fr.arg, fmt, **opt) is fr.arg
    assert fr.same(want), (fmt, opt, fr.diff(want))
    return fr


@pytest.mark.gpu
@pytest.mark.parametrize("how", ("resized", "yuv"))
def test_engine_blur_equals_restatement(how):
    """Engine.blur_faces behind forward_resized_enqueue / forward_yuv_enqueue + decode_threshold, default weights, context 64 x 96: bit
    for bit the restatement on the decode's NETWORK-coordinate boxes.  One context blurs a small frame first and a large one second:
    the scratch grows."""
    rng = np.random.default_rng(("resized", "yuv").index(how))
    eng = cfa.Engine(64, 96, max_batch=3, dtype="bf16")
    src, base = _feed_until_faces(eng, how, rng)
    boxes, counts = _net_boxes(base)
    assert int(counts.sum()) >= 2
    fmt = "bgr" if how == "resized" else "nv12"
    _engine_case(eng, fmt, 38, 50, boxes, counts, False, shape="rect", radius=2)                  # the smallest scratch first
    h, w = (76, 102) if how == "resized" else (src.shape[1] * 2 // 3, src.shape[2])
    first = _engine_case(eng, fmt, h, w, boxes, counts, False)
    for opt in (dict(shape="rect", radius=5), dict(shape="ellipse", radius=24, scale=2.0)):
        _engine_case(eng, fmt, h, w, boxes, counts, False, **opt)
    _engine_case(eng, fmt, 128, 256, boxes, counts, True, shape="ellipse", radius=0)              # the scratch grows again
    if how == "resized":
        _engine_case(eng, "bgr", 75, 101, boxes, counts, True, radius=3)                          # the odd source size itself
        _engine_case(eng, "i420", 76, 102, boxes, counts, False, radius=3)                        # any format behind any feed
    again = eng.decode_threshold(0.3, 0.3, 64)                                                    # the decode's outputs are unchanged
    for (d, l), (d0, l0) in zip(again, base):
        assert d.tobytes() == d0.tobytes() and l.tobytes() == l0.tobytes()
    eng.set_rescale(1.37, 1.21)                                                                   # the decode's boxes change, the blur does not
    eng.decode_threshold(0.3, 0.3, 64)
    assert _engine_case(eng, fmt, h, w, boxes, counts, False).same(first)
    eng.set_rescale(0.0, 0.0)
    eng.close()


@pytest.mark.gpu
def test_engine_blur_state_errors_and_device_form():
    rng = np.random.default_rng(5)
    eng = cfa.Engine(64, 96, max_batch=3, dtype="bf16")
    frames = rng.integers(0, 256, (3, 76, 102, 3), dtype=np.uint8)

    def refused():
        keep = frames.copy()
        with pytest.raises(cfa._lib.CenterFaceError) as e:
            eng.blur_faces(keep, "bgr")
        assert e.value.code == cfa._lib.CF_ESTATE and np.array_equal(keep, frames)
        assert b"cf_blur_faces" in cfa._lib.lib().cf_last_error(eng._h)
    refused()                                                              # before any forward
    x = source_frames(rng, "binary", (3, 64, 96, 3))
    eng.forward_enqueue(x)
    refused()                                                              # before any threshold decode
    eng.decode_topk(10)
    refused()
    eng.decode_threshold(0.3, 0.3, 64)
    eng.blur_faces(frames.copy(), "bgr")
    eng.forward_enqueue(x)
    refused()                                                              # a new forward was enqueued: the decode is gone
    eng.decode_threshold(0.3, 0.3, 64)
    eng.upload_images(list(x))
    refused()                                                              # an upload was started
    with pytest.raises(ValueError):
        eng.forward_enqueue(x), eng.decode_threshold(0.3, 0.3, 64), eng.blur_faces(frames[:2].copy(), "bgr")      # B is not the forward's
    with pytest.raises(ValueError):
        eng.blur_faces(frames.copy(), "bgr", radius=25)
    src, base = _feed_until_faces(eng, "float", rng)
    boxes, counts = _net_boxes(base)
    # the device form on planes from device_alloc equals the host form and the restatement, padding included
    for fmt in ("bgr", "nv12", "yv12"):
        p0, p1 = pitches_for(fmt, 102, aligned=True)
        fr = Frames(np.random.default_rng(13), fmt, 3, 76, 102, p0, p1, False)
        want = fr.clone()
        eng.blur_faces(want.arg, fmt, shape="ellipse", radius=0)
        ref = fr.clone()
        blur_ref(ref.views, fmt, boxes, counts, (64, 96), 76, 102, shape="ellipse", radius=0)
        assert want.same(ref), (fmt, want.diff(ref))
        dev = [eng.device_alloc(b.nbytes) for b in fr.bufs]
        for d, b in zip(dev, fr.bufs):
            eng.memcpy_h2d(d, b)
        n = len(fr.geo)
        eng.blur_faces_device([tuple(dev[b * n:(b + 1) * n]) for b in range(3)], fmt, 3, 76, 102, p0, p1, shape="ellipse", radius=0)
        eng.synchronize()
        for d, b in zip(dev, fr.bufs):
            eng.memcpy_d2h(b, d)
        assert fr.same(want), (fmt, fr.diff(want))
        with pytest.raises(ValueError):                                    # a misaligned device plane, a pitch that is no multiple of 4
            eng.blur_faces_device([(dev[b * n] + 2,) + tuple(dev[b * n + 1:(b + 1) * n]) for b in range(3)], fmt, 3, 76, 102, p0, p1)
        with pytest.raises(ValueError):
            eng.blur_faces_device([tuple(dev[b * n:(b + 1) * n]) for b in range(3)], fmt, 3, 76, 102, p0 + 2, p1)
        for d in dev:
            eng.device_free(d)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ("bgr", "nv12"))
def test_blur_after_a_merge_uses_the_merged_boxes(fmt):
    from test_tiles import tiled_engine, pitched_frames, FRAME_HW
    eng, dense, rects, thr = tiled_engine(fmt, seed=1)
    h, w = FRAME_HW
    eng.decode_threshold(thr, 0.5, 256)
    views, bufs, _, _ = pitched_frames(dense, fmt, 0xA5)
    with pytest.raises(cfa._lib.CenterFaceError) as e:                     # a tiled forward and a decode, but no merge
        eng.blur_faces(views, fmt)
    assert e.value.code == cfa._lib.CF_ESTATE
    merged, _ = eng.merge_tiles(max_out=256)
    assert sum(len(d) for d, _ in merged) >= 2
    boxes = np.concatenate([d[:, :4] for d, _ in merged])
    counts = np.array([len(d) for d, _ in merged], np.int32)
    for opt in (dict(), dict(shape="rect", radius=4)):
        views, bufs, _, _ = pitched_frames(dense, fmt, 0xA5)
        wviews, wbufs, _, _ = pitched_frames(dense, fmt, 0xA5)
        blur_ref(wviews, fmt, boxes, counts, (h, w), h, w, **opt)          # the merged corners, in frame pixels: (H, W) = (h, w)
        assert eng.blur_faces(views, fmt, **opt) is views
        assert all(np.array_equal(a, b) for a, b in zip(bufs, wbufs))
        orig = pitched_frames(dense, fmt, 0xA5)[1]
        assert not all(np.array_equal(a, b) for a, b in zip(bufs, orig))   # something was blurred
    keep = [b.copy() for b in bufs]
    with pytest.raises(ValueError):                                        # the wrong B is refused, nothing is written
        eng.blur_faces([views[0]], fmt)
    assert all(np.array_equal(a, b) for a, b in zip(bufs, keep))
    eng.decode_threshold(thr, 0.5, 256)                                    # a new decode forgets the merge
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        eng.blur_faces(views, fmt)
    assert e.value.code == cfa._lib.CF_ESTATE
    eng.close()


@pytest.mark.gpu
def test_centerface_anonymize_blur():
    """anonymize / anonymize_yuv with mode='blur': copies come back, the inputs stay, the detections are detect_batch's / detect_yuv's,
    and the outputs are the restatement on the network boxes of the same forward."""
    rng = np.random.default_rng(31)
    hw = (76, 102)
    face = cfa.CenterFace(*hw, dtype="bf16", max_batch=3)
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        imgs = list(source_frames(rng, kind, (3,) + hw + (3,)))
        want = face.detect_batch(imgs)
        if sum(len(d) for d, _ in want) >= 1:
            break
    keep = [im.copy() for im in imgs]
    out, dets = face.anonymize(imgs, mode="blur", shape="ellipse", radius=3)
    assert all(np.array_equal(a, b) for a, b in zip(imgs, keep))
    assert out.shape == (3,) + hw + (3,) and out.dtype == np.uint8
    for (d, l), (wd, wl) in zip(dets, want):
        assert d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes()
    boxes, counts = _net_boxes(face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets))     # the same forward, network coordinates
    assert list(counts) == [len(d) for d, _ in dets] and int(counts.sum()) >= 1
    ref = np.stack(keep)
    blur_ref([(f.reshape(hw[0], -1),) for f in ref], "bgr", boxes, counts, (face.img_h_new, face.img_w_new), hw[0], hw[1], shape="ellipse", radius=3)
    assert np.array_equal(out, ref) and not np.array_equal(out, np.stack(keep))
    with pytest.raises(ValueError):
        face.anonymize(imgs, mode="blur", cell=6)
    # 4:2:0, the per-face radius
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        yuv = source_frames(rng, kind, (3, hw[0] * 3 // 2, hw[1]))
        wanty = face.detect_yuv(yuv, "nv12")
        if sum(len(d) for d, _ in wanty) >= 1:
            break
    keepy = yuv.copy()
    outy, detsy = face.anonymize_yuv(yuv, "nv12", mode="blur", shape="rect")
    assert np.array_equal(yuv, keepy) and outy.shape == yuv.shape
    for (d, l), (wd, wl) in zip(detsy, wanty):
        assert d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes()
    boxes, counts = _net_boxes(face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets))
    assert int(counts.sum()) >= 1
    refy = keepy.copy()
    blur_ref([(f[:hw[0]], f[hw[0]:]) for f in refy], "nv12", boxes, counts, (face.img_h_new, face.img_w_new), hw[0], hw[1], shape="rect", radius=0)
    assert np.array_equal(outy, refy) and not np.array_equal(outy, keepy)
    face.close()


@pytest.mark.gpu
def test_centerface_anonymize_blur_tiled():
    """anonymize(tiled=True, mode='blur'): a copy blurred with the merged boxes, which are the returned detections' (frame pixels)."""
    from test_tiles import ENG_HW, FRAME_HW
    rng = np.random.default_rng(2)
    h, w = FRAME_HW
    face = cfa.CenterFace(ENG_HW[0], ENG_HW[1], dtype="bf16", max_batch=24)
    for kind in ("blocks", "binary", "noise", "blocks", "binary", "noise"):
        imgs = source_frames(rng, kind, (3, h, w, 3))
        if sum(len(d) for d, _ in face.detect_tiled(imgs)) >= 2:
            break
    keep = imgs.copy()
    out, dets = face.anonymize(list(imgs), tiled=True, mode="blur", shape="ellipse", radius=0)
    assert np.array_equal(imgs, keep) and sum(len(d) for d, _ in dets) >= 2
    ref = keep.copy()
    blur_ref([(f.reshape(h, -1),) for f in ref], "bgr", np.concatenate([d[:, :4] for d, _ in dets]), [len(d) for d, _ in dets], (h, w), h, w,
             shape="ellipse", radius=0)
    assert np.array_equal(out, ref) and not np.array_equal(out, keep)
    face.close()
