"""Aspect-preserving input on the GPU: the fit kernel (cf_op_fit, cf_forward_fit), the mapping of the decode's rows back into frame
pixels (cf_op_unfit, cf_unfit_rows) and the consumers behind it, every byte against the restatements of tests/fit_cases.py (fit = the
oracle's resize of the restated conversion, pasted into a filled canvas; unfit = centre rule + float64 map), tests/test_yuv_input.py
and tests/test_redact.py."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from fit_cases import WORKED, fit_geometry_ref, fit_ref, unfit_ref
from test_redact import redact_ref, source_frames
from test_tiles import bgr_of, pitched_frames

pytestmark = pytest.mark.gpu

FORMATS = ("bgr", "nv12", "nv21", "i420", "yv12")
NET = (64, 96)                  # (H, W) of every context here
CF_ESTATE = cfa._lib.CF_ESTATE


def dense_frames(rng, fmt, B, hw):
    h, w = hw
    return rng.integers(0, 256, (B, h, w, 3) if fmt == "bgr" else (B, h * 3 // 2, w), dtype=np.uint8)


def canvases_ref(bgr, size=NET, **opts):
    return np.stack([fit_ref(f, size[0], size[1], **opts) for f in bgr])


_fit_cache = {}


def fit_case(fmt, hw):
    """(dense frames, their BGR restatement) of one format and frame size, B = 3, computed once."""
    if (fmt, hw) not in _fit_cache:
        dense = dense_frames(np.random.default_rng(FORMATS.index(fmt) * 11 + hw[0]), fmt, 3, hw)
        _fit_cache[(fmt, hw)] = (dense, bgr_of(dense, fmt))
    return _fit_cache[(fmt, hw)]


def same_results(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() and u.tobytes() == v.tobytes() for (x, u), (y, v) in zip(a, b))


# ------------------------------------------------------------------------------------------ the fit kernel
@pytest.mark.parametrize("fmt", FORMATS)
def test_op_fit_bit_exact(fmt):
    """B = 3 frames of 40 x 120 (padding above and below), 120 x 40 (rw = 21, dx = 37: the content edges fall inside a lane's four
    columns) and 128 x 192 (no padding) into (64, 96), both anchors, fill (1, 2, 3), rows with padding: every byte equals the
    restatement, whether the padding and the bytes behind every plane hold 0xFF or 0x00.  30 x 50 with upscale off keeps its bytes."""
    for hw in ((40, 120), (120, 40), (128, 192)):
        dense, bgr = fit_case(fmt, hw)
        for anchor in ("center", "topleft"):
            opts = dict(anchor=anchor, fill=(1, 2, 3))
            want = canvases_ref(bgr, **opts)
            for pad in (0xFF, 0x00):
                views, bufs, _, _ = pitched_frames(dense, fmt, pad)
                got = ops.fit_frames(views, NET, fmt, **opts)
                assert got.shape == want.shape
                bad = np.argwhere(got != want)
                assert len(bad) == 0, (fmt, hw, anchor, pad, len(bad), bad[:4].tolist())
            assert np.array_equal(ops.fit_frames(dense, NET, fmt, **opts), want)         # dense frames
    dense, bgr = fit_case(fmt, (30, 50))
    for anchor, (y0, x0) in (("center", (17, 23)), ("topleft", (0, 0))):
        opts = dict(anchor=anchor, upscale=False, fill=(1, 2, 3))
        want = canvases_ref(bgr, **opts)
        assert np.array_equal(want[:, y0:y0 + 30, x0:x0 + 50], bgr)                      # the source bytes reproduced
        for pad in (0xFF, 0x00):
            views, _, _, _ = pitched_frames(dense, fmt, pad)
            got = ops.fit_frames(views, NET, fmt, **opts)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (fmt, anchor, pad, len(bad), bad[:4].tolist())
    # a small frame enlarged (upscale on): 30 x 50 -> rw 96, rh 58
    want = canvases_ref(bgr, fill=(9, 8, 7))
    assert np.array_equal(ops.fit_frames(dense, NET, fmt, fill=(9, 8, 7)), want)


def test_op_fit_odd_sides_bgr():
    """33 x 100 BGR frames (odd height; rh = 32) and 41 x 27 (both odd; rw = 42), rows with padding."""
    for hw in ((33, 100), (41, 27)):
        dense, bgr = fit_case("bgr", hw)
        for anchor in ("center", "topleft"):
            want = canvases_ref(bgr, anchor=anchor, fill=(1, 2, 3))
            for pad in (0xFF, 0x00):
                views, _, _, _ = pitched_frames(dense, "bgr", pad)
                got = ops.fit_frames(views, NET, "bgr", anchor=anchor, fill=(1, 2, 3))
                bad = np.argwhere(got != want)
                assert len(bad) == 0, (hw, anchor, pad, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("fmt", ("yv12", "bgr"))
def test_op_fit_more_frames_than_one_launch(fmt):
    """B = 65 frames of 8 x 8 (one launch takes 64) into (4, 8), rows with padding: frame 64 is the second launch's only frame -- its
    planes (YV12: swapped) at table entry 0, its canvas behind those of the 64 before it."""
    dense = dense_frames(np.random.default_rng(90 + FORMATS.index(fmt)), fmt, 65, (8, 8))
    want = canvases_ref(bgr_of(dense, fmt), (4, 8), fill=(1, 2, 3))
    views, _, _, _ = pitched_frames(dense, fmt, 0xFF)
    got = ops.fit_frames(views, (4, 8), fmt, fill=(1, 2, 3))
    assert got.shape == want.shape == (65, 4, 8, 3)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (fmt, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("fmt", FORMATS)
def test_engine_forward_fit_writes_the_restated_canvases(fmt):
    """cf_forward_fit, host-staged (padded rows, and one dense block) and in place on device planes: cf_get_resized_input returns the
    restated canvases; the planes are untouched; a misaligned device plane is refused."""
    hw = (40, 120)
    dense, bgr = fit_case(fmt, hw)
    opts = dict(anchor="center", fill=(1, 2, 3))
    want = canvases_ref(bgr, **opts)
    eng = cfa.Engine(NET[0], NET[1], max_batch=4, dtype="bf16")
    views, bufs, p0, p1 = pitched_frames(dense, fmt, 0xFF)
    for frames in (views, dense):
        eng.forward_fit_enqueue(frames, fmt, **opts)
        got = eng.resized_input()
        assert got.shape == want.shape and np.array_equal(got, want), fmt
    for pad in (0xFF, 0x00):
        views, bufs, p0, p1 = pitched_frames(dense, fmt, pad, aligned=True)
        dev = [eng.device_alloc(b.nbytes) for b in bufs]
        for d, b in zip(dev, bufs):
            eng.memcpy_h2d(d, b)
        n = len(views[0])
        planes = [tuple(dev[b * n:(b + 1) * n]) for b in range(3)]
        eng.forward_fit_enqueue(planes, fmt, on_device=True, h=hw[0], w=hw[1], pitch0=p0, pitch1=p1, **opts)
        assert np.array_equal(eng.resized_input(), want), (fmt, pad)
        for d, b in zip(dev, bufs):                                                  # read in place: the planes are untouched
            back = np.empty_like(b)
            eng.memcpy_d2h(back, d)
            assert np.array_equal(back, b)
        with pytest.raises(ValueError):                                              # a misaligned device plane
            eng.forward_fit_enqueue([(planes[0][0] + 2,) + planes[0][1:]] + planes[1:], fmt, on_device=True, h=hw[0], w=hw[1], pitch0=p0, pitch1=p1)
        for d in dev:
            eng.device_free(d)
    # refusals name the value and leave the engine working; B must fit max_batch
    with pytest.raises(ValueError) as e:
        eng.forward_fit_enqueue(np.concatenate([dense, dense]), fmt)
    assert "max_batch" in str(e.value) and "B=6" in str(e.value)
    with pytest.raises(ValueError) as e:
        eng.forward_fit_enqueue(dense, fmt, anchor=3)
    assert "anchor 3" in str(e.value)
    eng.forward_fit_enqueue(dense, fmt, anchor="topleft", fill=(1, 2, 3))
    assert np.array_equal(eng.resized_input(), canvases_ref(bgr, anchor="topleft", fill=(1, 2, 3)))
    eng.close()


# ------------------------------------------------------------------------------------------ the mapper on hand-built tables
FILL = np.float32(-7.25)


def check_unfit(frame_hw, net_hw, d, s, l, counts, max_out, **opt):
    """ops.unfit_rows against unfit_ref, bit for bit: counts, flags, the rows below min(count, max_out), and the caller's bytes in every
    row behind them."""
    d, s, l = (np.asarray(a, np.float32) for a in (d, s, l))
    B = d.shape[0]
    od, ol = np.full((B, max_out, 5), FILL), np.full((B, max_out, 10), FILL)
    gd, gl, gc, gf = ops.unfit_rows(frame_hw, net_hw, d, s, l, counts, max_out, dets=od, lms=ol, **opt)
    geom = fit_geometry_ref(frame_hw[0], frame_hw[1], net_hw[0], net_hw[1], opt.get("anchor", "center"), opt.get("upscale", True))
    assert ops.fit_geometry(frame_hw[0], frame_hw[1], net_hw[0], net_hw[1], **opt) == geom
    want, wflags = unfit_ref(geom, frame_hw, d, s, l, counts)
    assert gc.tolist() == [len(w[0]) for w in want], (gc, [len(w[0]) for w in want])
    assert gf.tolist() == wflags.tolist()
    for b, (wd, wl) in enumerate(want):
        m = min(len(wd), max_out)
        assert gd[b, :m].tobytes() == wd[:m].tobytes(), (b, gd[b, :m], wd[:m])
        assert gl[b, :m].tobytes() == wl[:m].tobytes(), b
        assert (gd[b, m:] == FILL).all() and (gl[b, m:] == FILL).all(), b
    return want, gc, gf


def unfit_table(rng, geom, net_hw, B, rows):
    """Random boxes around the canvas, most centres in the content, some in the padding or outside the canvas; every image then gets rows
    whose centre sits exactly on each of the four content edges, a NaN and two infinite corners."""
    rw, rh, dx, dy = geom
    H, W = net_hw
    c = np.stack([rng.uniform(dx - 6, dx + rw + 6, (B, rows)), rng.uniform(dy - 6, dy + rh + 6, (B, rows))], -1)
    half = rng.uniform(0.5, 12, (B, rows, 2))
    d = np.concatenate([c - half, c + half], -1).astype(np.float32)
    for b in range(B):
        d[b, 0] = (dx - 2, dy + 1, dx + 2, dy + 3)                          # cx = dx: kept
        d[b, 1] = (dx + rw - 2, dy + 1, dx + rw + 2, dy + 3)                # cx = dx + rw: dropped
        d[b, 2] = (dx + 1, dy - 3, dx + 3, dy + 3)                          # cy = dy: kept
        d[b, 3] = (dx + 1, dy + rh - 3, dx + 3, dy + rh + 3)                # cy = dy + rh: dropped
        d[b, 4, 0] = np.nan
        d[b, 5, 3] = np.inf
        d[b, 6, 1] = -np.inf
    s = rng.choice(np.linspace(0.3, 0.95, 40).astype(np.float32), (B, rows))
    l = rng.uniform(-4, max(H, W) + 4, (B, rows, 10)).astype(np.float32)
    return d, s, l


def test_op_unfit_bit_exact_on_constructed_tables():
    """Every geometry of the statement's worked values, both anchors: NaN and infinite corners, centres on both content edges, counts of
    0, a count above the rows written, landmarks, more kept rows than max_out; one table of 1100 rows crosses the 1024 rows a workgroup
    takes per round."""
    rng = np.random.default_rng(5)
    for (h, w), net, up, _ in WORKED:
        for anchor in ("center", "topleft"):
            geom = fit_geometry_ref(h, w, net[0], net[1], anchor, bool(up))
            d, s, l = unfit_table(rng, geom, net, 4, 40)
            counts = [40, 0, 49, 17]
            want, gc, gf = check_unfit((h, w), net, d, s, l, counts, 64, anchor=anchor, upscale=bool(up))
            assert gf.tolist() == [0, 0, 1, 0] and gc[1] == 0 and gc[0] >= 4 and gc[2] >= 4, (h, w, anchor, gc)
            check_unfit((h, w), net, d, s, l, counts, 3, anchor=anchor, upscale=bool(up))            # truncated outputs
    geom = fit_geometry_ref(40, 120, 64, 96)
    d, s, l = unfit_table(rng, geom, NET, 2, 1100)
    want, gc, _ = check_unfit((40, 120), NET, d, s, l, [1100, 1030], 1100)
    assert gc[0] > 300 and gc[1] > 300
    # by hand: the identity scale of a 32 x 96 frame subtracts dy = 16 from every y and nothing else
    d = np.float32([[(10, 20, 30, 40), (50, 2, 60, 10)]])
    want, gc, _ = check_unfit((32, 96), NET, d, np.float32([[0.5, 0.6]]), np.zeros((1, 2, 10), np.float32), [2], 4)
    assert gc.tolist() == [1] and want[0][0][0].tolist() == [10, 4, 30, 24, 0.5]


def test_op_unfit_keeps_the_sign_of_a_negative_zero():
    """Top-left anchor, dx = dy = 0: X = float32((float64(x) - 0) * sx) and nothing is added, so a -0.0 corner and a -0.0 landmark come
    back as -0.0, bit for bit (a map that added a source offset of 0.0 would return +0.0)."""
    d = np.float32([[(-0.0, -0.0, 8, 6)]])
    l = np.zeros((1, 1, 10), np.float32)
    l[0, 0, :2] = -0.0
    want, gc, _ = check_unfit((32, 96), NET, d, np.float32([[0.5]]), l, [1], 2, anchor="topleft")
    assert gc.tolist() == [1] and np.signbit(want[0][0][0, :2]).all() and np.signbit(want[0][1][0, :2]).all()


# ------------------------------------------------------------------------------------------ the engine
def fitted_engine(hw, fmt="bgr", seed=0, need=2, **opts):
    """A 64 x 96 context with the default (synthetic) weights and two frames of ``hw`` whose fitted forward, decoded at a score threshold
    read off the heat maps (at least 6 cells of the content above it in every image), keeps ``need`` rows with their centre in the
    content whose mapped box has an area inside the frame (so that a redaction has something to cover): (engine, dense frames,
    threshold, the decode's rows).  The default weights answer to one of the source kinds."""
    h, w = hw
    rw, rh, dx, dy = fit_geometry_ref(h, w, NET[0], NET[1], opts.get("anchor", "center"), opts.get("upscale", True))
    eng = cfa.Engine(NET[0], NET[1], max_batch=4, dtype="bf16")
    tried = []
    for k, kind in enumerate(("blocks", "binary", "noise") * 4):
        rng = np.random.default_rng(seed + 10 * k)
        dense = source_frames(rng, kind, (2, h, w, 3) if fmt == "bgr" else (2, h * 3 // 2, w))
        eng.forward_fit_enqueue(dense, fmt, **opts)
        hm = eng.heads(sigmoid_hm=True)["hm_sigmoid"].reshape(2, NET[0] // 4, NET[1] // 4)
        inside = hm[:, (dy + 3) // 4:(dy + rh) // 4, (dx + 3) // 4:(dx + rw) // 4].reshape(2, -1)
        sixth = np.sort(inside, 1)[:, -6]
        thr = float(np.nextafter(np.float32(sixth.min()), np.float32(0)))
        per = eng.decode_threshold(thr, 0.5, 256)
        d, s, l, c = net_tables(per)
        mapped = unfit_ref((rw, rh, dx, dy), hw, d, s, l, c)[0]
        kept = [len(x) for x, _ in mapped]
        solid = sum(int(((x[:, 2] - x[:, 0] >= 2) & (x[:, 3] - x[:, 1] >= 2) & (x[:, 2] > 0) & (x[:, 3] > 0) & (x[:, 0] < w) & (x[:, 1] < h)).sum())
                    for x, _ in mapped)
        tried.append((kind, thr, [len(x) for x, _ in per], kept, solid))
        if min(kept) >= 1 and sum(kept) >= need and solid >= need:
            print("fitted_engine:", tried)
            return eng, dense, thr, per
    raise AssertionError(tried)


def net_tables(per):
    """The decode's results (network coordinates) as the mapper's tables."""
    B = len(per)
    rows = max(1, max(len(d) for d, _ in per))
    d, s, l = np.zeros((B, rows, 4), np.float32), np.zeros((B, rows), np.float32), np.zeros((B, rows, 10), np.float32)
    c = np.zeros(B, np.int32)
    for b, (dd, ll) in enumerate(per):
        c[b] = len(dd)
        d[b, :len(dd)], s[b, :len(dd)], l[b, :len(dd)] = dd[:, :4], dd[:, 4], ll
    return d, s, l, c


def heads_equal(a, b):
    return sorted(a) == sorted(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def test_identity_fit_equals_the_hand_pasted_canvas():
    """A 32 x 96 frame gives rw 96, rh 32, dy 16: the fitted forward and the plain forward of the hand-pasted canvas give bit-identical
    heads and decoded rows, and unfit_rows is those rows with 16 subtracted from every y, for the rows whose centre lies in the content."""
    hw = (32, 96)
    assert ops.fit_geometry(32, 96, *NET) == (96, 32, 0, 16)
    eng, dense, thr, per = fitted_engine(hw)
    heads = eng.heads()
    canvas = np.zeros((2,) + NET + (3,), np.uint8)
    canvas[:, 16:48] = dense
    assert np.array_equal(eng.resized_input(), canvas)
    got, flags = eng.unfit_rows(256)
    eng.forward_enqueue(canvas)
    assert heads_equal(eng.heads(), heads)
    assert same_results(eng.decode_threshold(thr, 0.5, 256), per)
    want = []
    sixteen = np.float32(16)
    for d, l in per:
        cy = (d[:, 1] + d[:, 3]) * np.float32(0.5)
        cx = (d[:, 0] + d[:, 2]) * np.float32(0.5)
        m = (cy >= 16) & (cy < 48) & (cx >= 0) & (cx < 96)
        d, l = d[m].copy(), l[m].copy()
        d[:, 1] -= sixteen
        d[:, 3] -= sixteen
        l[:, 1::2] -= sixteen
        want.append((d, l))
    assert same_results(got, want) and flags.tolist() == [0, 0] and sum(len(d) for d, _ in got) >= 2
    eng.close()


@pytest.mark.parametrize("fmt", ("bgr", "nv12"))
def test_engine_fit_decode_unfit_and_the_consumers(fmt):
    """forward_fit -> decode_threshold -> unfit_rows equals the restated map of the decode's own rows; the redaction of the source frames
    uses those frame-space boxes on every byte; the tracker, the chips cut from the frame and the state rules."""
    hw = (40, 120)
    h, w = hw
    geom = fit_geometry_ref(h, w, *NET)
    eng, dense, thr, per = fitted_engine(hw, fmt, seed=1)
    opt = dict(mode="mosaic", shape="ellipse", cell=6)

    def frames(pad=0xFF):
        return pitched_frames(dense, fmt, pad)

    views, bufs, _, _ = frames()
    with pytest.raises(cfa._lib.CenterFaceError) as e:                     # a fitted forward and a decode, but no unfit_rows
        eng.redact_faces(views, fmt, **opt)
    assert e.value.code == CF_ESTATE
    with pytest.raises(cfa._lib.CenterFaceError) as e:                     # ... and it is not a tiled forward
        eng.merge_tiles()
    assert e.value.code == CF_ESTATE
    trk = cfa.Tracker(eng, 2, min_hits=1)
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        eng.track_update_device(trk, 0)
    assert e.value.code == CF_ESTATE
    d, s, l, c = net_tables(per)
    want, wflags = unfit_ref(geom, hw, d, s, l, c)
    got, flags = eng.unfit_rows(256)
    print("kept per image:", [len(x) for x, _ in per], "in the content:", [len(x) for x, _ in got])
    assert same_results(got, want) and flags.tolist() == wflags.tolist() == [0, 0]
    assert same_results(eng.unfit_rows(max_out=1)[0], want)                # truncated host form: the wrapper comes back for all of them
    # cf_set_rescale changes the decode's own rows, not the mapped ones
    eng.set_rescale(1.37, 1.21)
    scaled = eng.decode_threshold(thr, 0.5, 256)
    assert [len(x) for x, _ in scaled] == [len(x) for x, _ in per] and not same_results(scaled, per)
    assert same_results(eng.unfit_rows(256)[0], want)
    eng.set_rescale(0.0, 0.0)
    assert same_results(eng.decode_threshold(thr, 0.5, 256), per)
    # the device form, read back; every output may be NULL
    mo = 64
    dev = [eng.device_alloc(2 * mo * 5 * 4), eng.device_alloc(2 * mo * 10 * 4), eng.device_alloc(8), eng.device_alloc(8)]
    eng.unfit_rows_device(mo, *dev)
    eng.synchronize()
    hd, hl, hc, hf = np.empty((2, mo, 5), np.float32), np.empty((2, mo, 10), np.float32), np.empty(2, np.int32), np.empty(2, np.int32)
    for a, b in zip((hd, hl, hc, hf), dev):
        eng.memcpy_d2h(a, b)
        eng.device_free(b)
    assert hc.tolist() == [len(x) for x, _ in want] and hf.tolist() == [0, 0]
    assert same_results([(hd[b, :hc[b]], hl[b, :hc[b]]) for b in range(2)], want)
    eng.unfit_rows_device(mo)
    # the redaction of the source frames with the mapped boxes, which are in frame pixels: (H, W) = (h, w)
    boxes = np.concatenate([x[:, :4] for x, _ in want])
    counts = np.array([len(x) for x, _ in want], np.int32)
    solid = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    sviews, sbufs, _, _ = frames()
    wviews, wbufs, _, _ = frames()
    redact_ref(wviews, fmt, boxes, counts, (h, w), h, w, **solid)
    eng.redact_faces(sviews, fmt, **solid)
    assert all(np.array_equal(a, b) for a, b in zip(sbufs, wbufs))
    assert not all(np.array_equal(a, b) for a, b in zip(sbufs, frames()[1]))                 # something was redacted
    wviews, wbufs, _, _ = frames()
    redact_ref(wviews, fmt, boxes, counts, (h, w), h, w, **opt)
    assert eng.redact_faces(views, fmt, **opt) is views
    assert all(np.array_equal(a, b) for a, b in zip(bufs, wbufs))
    # the wrong B or frame size is refused, nothing is written
    for bad in ([views[0]], [tuple(p[:h - 2] if k == 0 else p[:(h - 2) // 2] for k, p in enumerate(v)) for v in views]):
        keep = [b.copy() for b in bufs]
        with pytest.raises(ValueError):
            eng.redact_faces(bad, fmt, **opt)
        assert all(np.array_equal(a, b) for a, b in zip(bufs, keep))
    # one chip per mapped row, cut from the frames
    chips, offs, _ = eng.align_faces_frame(dense, fmt, 32)
    assert np.diff(offs).tolist() == counts.tolist() and len(chips) == int(counts.sum())
    # cf_align_faces works per image on the padded batch, with the decode's own rows
    chips, offs, _ = eng.align_faces(32)
    assert np.diff(offs).tolist() == [len(x) for x, _ in per]
    # the tracker takes the mapped rows of B frames of (h, w): every row starts a track with an id
    M = trk.max_tracks
    dev = [eng.device_alloc(2 * M * 3 * 4), eng.device_alloc(8)]
    eng.track_update_device(trk, 0, info_ptr=dev[0], counts_ptr=dev[1])
    eng.synchronize()
    info, tc = np.empty((2, M, 3), np.int32), np.empty(2, np.int32)
    eng.memcpy_d2h(info, dev[0])
    eng.memcpy_d2h(tc, dev[1])
    for p in dev:
        eng.device_free(p)
    assert tc.tolist() == counts.tolist()
    for b in range(2):
        ids = info[b, :tc[b], 0].tolist()
        assert min(ids) >= 1 and len(set(ids)) == len(ids) and (info[b, :tc[b], 1:] == [1, 0]).all(), info[b, :tc[b]]      # hits 1, misses 0
    views2, bufs2, _, _ = frames()
    eng.redact_faces(views2, fmt, **opt)                                   # the tracked rows: the same boxes (min_hits = 1)
    assert all(np.array_equal(a, b) for a, b in zip(bufs2, wbufs))
    trk.close()
    # a new decode forgets the mapped rows
    eng.decode_threshold(thr, 0.5, 256)
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        eng.redact_faces(views, fmt, **opt)
    assert e.value.code == CF_ESTATE
    # a later plain forward forgets the geometry
    eng.forward_enqueue(canvases_ref(bgr_of(dense, fmt)))
    assert same_results(eng.decode_threshold(thr, 0.5, 256), per)
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        eng.unfit_rows()
    assert e.value.code == CF_ESTATE
    # ... and so does an upload
    eng.forward_fit_enqueue(dense, fmt)
    with pytest.raises(cfa._lib.CenterFaceError) as e:                     # before a decode
        eng.unfit_rows()
    assert e.value.code == CF_ESTATE
    eng.decode_threshold(thr, 0.5, 256)
    eng.upload_images(list(canvases_ref(bgr_of(dense, fmt))))
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        eng.unfit_rows()
    assert e.value.code == CF_ESTATE
    eng.close()


def test_centerface_detect_fit_and_anonymize():
    """CenterFace.detect_fit = forward_fit + decode + unfit_rows with the defaults; anonymize(fit=True) redacts a copy with the mapped
    boxes; the inputs stay untouched."""
    rng = np.random.default_rng(2)
    h, w = 40, 120
    geom = fit_geometry_ref(h, w, *NET)
    face = cfa.CenterFace(NET[0], NET[1], dtype="bf16", max_batch=4)
    tried = []
    for kind in ("blocks", "binary", "noise", "blocks", "binary", "noise"):  # the default weights answer to one of them
        imgs = source_frames(rng, kind, (2, h, w, 3))
        got = face.detect_fit(imgs)
        tried.append((kind, [len(d) for d, _ in got]))
        if sum(len(d) for d, _ in got) >= 2:
            break
    print("detect_fit:", tried)
    assert sum(len(d) for d, _ in got) >= 2, tried
    assert all(d.shape[1:] == (5,) and l.shape == (len(d), 10) and d.dtype == np.float32 for d, l in got)
    face.engine.forward_fit_enqueue(imgs, "bgr")
    per = face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets)
    want = unfit_ref(geom, (h, w), *net_tables(per))[0]
    assert same_results(got, want)
    assert same_results(face.engine.unfit_rows(face.max_dets)[0], want)
    keep = imgs.copy()
    out, dets = face.anonymize(list(imgs), fit=True, mode="solid", shape="rect", fill=(1, 2, 3))
    assert np.array_equal(imgs, keep) and same_results(dets, want)
    ref = keep.copy()
    redact_ref([(f.reshape(h, -1),) for f in ref], "bgr", np.concatenate([d[:, :4] for d, _ in want]), [len(d) for d, _ in want], (h, w), h, w,
               mode="solid", shape="rect", fill=(1, 2, 3))
    assert np.array_equal(out, ref) and not np.array_equal(out, keep)
    # the options travel: the top-left anchor gives the restated canvases, and its rows map back with dy = 0
    got = face.detect_fit(imgs, anchor="topleft", fill=(1, 2, 3))
    assert np.array_equal(face.engine.resized_input(), canvases_ref(imgs, anchor="topleft", fill=(1, 2, 3)))
    per = face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets)
    assert same_results(got, unfit_ref(fit_geometry_ref(h, w, *NET, "topleft"), (h, w), *net_tables(per))[0])
    with pytest.raises(ValueError):
        face.anonymize(list(imgs), fit=True, tiled=True)
    face.close()
