"""Rotated sources on the GPU: the kernel behind cf_forward_rot (cf_op_rot), the mapping of the decode's rows back into the pixels of
the stored frame (cf_op_unrot, cf_unfit_rows behind a rotated forward) and the consumers behind it, every byte against the
restatements of tests/rot_cases.py (numpy's rot90, then tests/fit_cases.py or the oracle's resize; the statement's table in float64),
tests/test_redact.py and tests/flip_cases.py."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from fit_cases import fit_geometry_ref
from flip_cases import flip_heads_ref
from rot_cases import ROTS, rot_geometry_ref, rot_ref, unrot_ref, upright
from test_fit import FILL, FORMATS, NET, dense_frames, fit_case, heads_equal, net_tables, same_results
from test_flip import assert_heads, plain_records
from test_redact import redact_ref, source_frames
from test_tiles import bgr_of, pitched_frames

pytestmark = pytest.mark.gpu

CF_ESTATE = cfa._lib.CF_ESTATE
# (64, 96): the canvas of the fit's tests; (36, 100): a height that is no multiple of a tile or of the rows a lane takes, a width that is
# no multiple of the quarter turns' 32-column tile, content edges inside a lane's four columns
SIZES = (NET, (36, 100))
_ref_cache = {}


def canvases_ref(fmt, hw, rot, size, stretch, **fit):
    """The restated canvases of fit_case(fmt, hw), computed once per case and left unchanged."""
    key = (fmt, hw, rot, size, stretch, tuple(sorted(fit.items())))
    if key not in _ref_cache:
        bgr = fit_case(fmt, hw)[1]
        ref = np.stack([rot_ref(f, rot, size[0], size[1], stretch, **fit) for f in bgr])
        ref.setflags(write=False)
        _ref_cache[key] = ref
    return _ref_cache[key]


def assert_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("rot", ROTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_op_rot_bit_exact(fmt, rot):
    """B = 3 stored frames of 40 x 120, 120 x 40 and 128 x 192 into (64, 96) and (36, 100), fitted (both anchors, fill (1, 2, 3)) and
    stretched, rows with padding that holds 0xFF or 0x00, and dense: every byte equals the restatement.  30 x 50 with upscale off
    reproduces the turned source bytes."""
    for hw in ((40, 120), (120, 40), (128, 192)):
        dense = fit_case(fmt, hw)[0]
        padded = [pitched_frames(dense, fmt, pad)[0] for pad in (0xFF, 0x00)]
        for size in SIZES:
            for fit in (dict(anchor="center", fill=(1, 2, 3)), dict(anchor="topleft", fill=(1, 2, 3)), None):
                want = canvases_ref(fmt, hw, rot, size, fit is None, **(fit or {}))
                for pad, views in zip((0xFF, 0x00), padded):
                    assert_bytes(ops.rot_frames(views, size, fmt, rot, fit), want, (fmt, rot, hw, size, fit, pad))
                assert_bytes(ops.rot_frames(dense, size, fmt, rot, fit), want, (fmt, rot, hw, size, fit, "dense"))
    hw = (30, 50)
    dense, bgr = fit_case(fmt, hw)
    hu, wu = (50, 30) if rot in (90, 270) else (30, 50)
    for anchor in ("center", "topleft"):
        fit = dict(anchor=anchor, upscale=False, fill=(1, 2, 3))
        want = canvases_ref(fmt, hw, rot, NET, False, **fit)
        rw, rh, dx, dy = rot_geometry_ref(30, 50, NET[0], NET[1], rot, 0, anchor, False)
        assert (rw, rh) == (wu, hu)
        assert np.array_equal(want[:, dy:dy + hu, dx:dx + wu], np.stack([upright(f, rot) for f in bgr]))      # the turned source bytes
        for pad in (0xFF, 0x00):
            assert_bytes(ops.rot_frames(pitched_frames(dense, fmt, pad)[0], NET, fmt, rot, fit), want, (fmt, rot, anchor, pad))


@pytest.mark.parametrize("rot", ROTS)
def test_op_rot_odd_sides_bgr(rot):
    """33 x 100 and 41 x 27 BGR frames, rows with padding, fitted and stretched."""
    for hw in ((33, 100), (41, 27)):
        dense = fit_case("bgr", hw)[0]
        for size in SIZES:
            for fit in (dict(anchor="center", fill=(1, 2, 3)), dict(anchor="topleft", fill=(1, 2, 3)), None):
                want = canvases_ref("bgr", hw, rot, size, fit is None, **(fit or {}))
                for pad in (0xFF, 0x00):
                    assert_bytes(ops.rot_frames(pitched_frames(dense, "bgr", pad)[0], size, "bgr", rot, fit), want, (rot, hw, size, fit, pad))


@pytest.mark.parametrize("rot", (90, 180, 270))
@pytest.mark.parametrize("fmt", ("yv12", "bgr"))
def test_op_rot_more_frames_than_one_launch(fmt, rot):
    """B = 65 frames of 8 x 8 (one launch takes 64) into (4, 8): frame 64 is the second launch's only frame -- its planes (YV12:
    swapped) at table entry 0, its canvas behind those of the 64 before it."""
    dense = dense_frames(np.random.default_rng(90 + FORMATS.index(fmt)), fmt, 65, (8, 8))
    bgr = bgr_of(dense, fmt)
    views = pitched_frames(dense, fmt, 0xFF)[0]
    for fit in (dict(fill=(1, 2, 3)), None):
        want = np.stack([rot_ref(f, rot, 4, 8, fit is None, **(fit or {})) for f in bgr])
        got = ops.rot_frames(views, (4, 8), fmt, rot, fit)
        assert got.shape == (65, 4, 8, 3)
        assert_bytes(got, want, (fmt, rot, fit))


@pytest.mark.parametrize("fmt", FORMATS)
def test_rot_0_is_the_fit(fmt):
    """rot = 0 without stretch launches the fit kernel: the bytes of ops.fit_frames, whatever the options."""
    for hw in ((40, 120), (120, 40)):
        views = pitched_frames(fit_case(fmt, hw)[0], fmt, 0xFF)[0]
        for size in SIZES:
            for opts in (dict(anchor="center", fill=(1, 2, 3)), dict(anchor="topleft", upscale=False, fill=(9, 8, 7))):
                assert ops.rot_frames(views, size, fmt, 0, opts).tobytes() == ops.fit_frames(views, size, fmt, **opts).tobytes(), (fmt, hw, size, opts)


# ------------------------------------------------------------------------------------------ the mapper on hand-built tables
def unrot_table(rng, geom, net_hw, B, rows):
    """Rows 0..13 of every image: a centre on each content edge (left and top kept, right and bottom dropped), half a pixel beside each
    (the other way round), a NaN and two infinite corners (dropped), an inverted box, an x corner and a y corner of -0.0 (kept); from
    row 14 on, centres inside the content (even rows) and in the padding or off the canvas (odd rows) in turn."""
    rw, rh, dx, dy = geom
    H, W = net_hw
    assert rows >= 16 and rw >= 8 and rh >= 8
    inside = np.stack([rng.uniform(dx + 0.5, dx + rw - 0.5, (B, rows)), rng.uniform(dy + 0.5, dy + rh - 0.5, (B, rows))], -1)
    side = rng.integers(0, 4, (B, rows))
    far = rng.uniform(0.75, 9, (B, rows))
    outside = inside.copy()
    outside[..., 0] = np.where(side == 0, dx - far, np.where(side == 1, dx + rw + far, outside[..., 0]))
    outside[..., 1] = np.where(side == 2, dy - far, np.where(side == 3, dy + rh + far, outside[..., 1]))
    c = np.where((np.arange(rows) % 2 == 0)[None, :, None], inside, outside)
    half = rng.uniform(0.5, 12, (B, rows, 2))
    d = np.concatenate([c - half, c + half], -1).astype(np.float32)
    mx, my = dx + rw // 2, dy + rh // 2
    for b in range(B):
        d[b, 0] = (dx - 2, my - 1, dx + 2, my + 1)                          # cx = dx: kept
        d[b, 1] = (dx + rw - 2, my - 1, dx + rw + 2, my + 1)                # cx = dx + rw: dropped
        d[b, 2] = (mx - 1, dy - 3, mx + 1, dy + 3)                          # cy = dy: kept
        d[b, 3] = (mx - 1, dy + rh - 3, mx + 1, dy + rh + 3)                # cy = dy + rh: dropped
        d[b, 4] = (dx - 2, my - 1, dx + 1, my + 1)                          # cx = dx - 0.5: dropped
        d[b, 5] = (dx + rw - 2, my - 1, dx + rw + 1, my + 1)                # cx = dx + rw - 0.5: kept
        d[b, 6] = (mx - 1, dy - 3, mx + 1, dy + 2)                          # cy = dy - 0.5: dropped
        d[b, 7] = (mx - 1, dy + rh - 3, mx + 1, dy + rh + 2)                # cy = dy + rh - 0.5: kept
        d[b, 8] = (np.nan, my - 1, mx + 1, my + 1)
        d[b, 9] = (mx - 1, my - 1, mx + 1, np.inf)
        d[b, 10] = (mx - 1, -np.inf, mx + 1, my + 1)
        d[b, 11] = (mx + 3, my + 2, mx - 3, my - 2)                         # inverted both ways, its centre in the content: kept
        d[b, 12] = (-0.0, my - 1, 2 * dx + 2, my + 1)                       # cx = dx + 1
        d[b, 13] = (mx - 1, -0.0, mx + 1, 2 * dy + 2)                       # cy = dy + 1
    s = rng.choice(np.linspace(0.3, 0.95, 40).astype(np.float32), (B, rows))
    l = rng.uniform(-4, max(H, W) + 4, (B, rows, 10)).astype(np.float32)
    l[:, 12, 0] = -0.0
    return d, s, l


def check_unrot(frame_hw, net_hw, rot, fit, d, s, l, counts, max_out):
    """ops.unrot_rows against unrot_ref, bit for bit: counts, flags, the rows below min(count, max_out), and the caller's bytes in every
    row behind them.  Before the comparison, on the restatement alone: a third of every image's rows is kept and a third dropped."""
    B, rows = d.shape[:2]
    geom = rot_geometry_ref(frame_hw[0], frame_hw[1], net_hw[0], net_hw[1], rot, fit is None, **(fit or {}))
    want, wflags = unrot_ref(geom, frame_hw, rot, d, s, l, counts)
    for b, (wd, _) in enumerate(want):
        seen = min(int(counts[b]), rows)
        assert 3 * len(wd) >= seen and 3 * (seen - len(wd)) >= seen and seen >= 14, (b, seen, len(wd))
    assert ops.rot_geometry(frame_hw[0], frame_hw[1], net_hw[0], net_hw[1], rot, fit) == geom
    od, ol = np.full((B, max_out, 5), FILL), np.full((B, max_out, 10), FILL)
    gd, gl, gc, gf = ops.unrot_rows(frame_hw, net_hw, d, s, l, counts, max_out, rot=rot, fit=fit, dets=od, lms=ol)
    assert gc.tolist() == [len(w[0]) for w in want], (gc, [len(w[0]) for w in want])
    assert gf.tolist() == wflags.tolist()
    for b, (wd, wl) in enumerate(want):
        m = min(len(wd), max_out)
        assert gd[b, :m].tobytes() == wd[:m].tobytes(), (rot, fit, b, gd[b, :m], wd[:m])
        assert gl[b, :m].tobytes() == wl[:m].tobytes(), (rot, fit, b)
        assert (gd[b, m:] == FILL).all() and (gl[b, m:] == FILL).all(), b
    return want, gc, gf


@pytest.mark.parametrize("rot", ROTS)
def test_op_unrot_bit_exact_on_constructed_tables(rot):
    """Stored frames of 40 x 120 and 120 x 40 behind a (64, 96) canvas, fitted (both anchors) and stretched: rows on and beside every
    content edge, non-finite corners, an inverted box, corners of -0.0, a count above the rows written (flag bit 0), max_out below the
    kept count; one table of 1100 rows crosses the 1024 rows a workgroup takes per round."""
    rng = np.random.default_rng(50 + rot)
    for hw in ((40, 120), (120, 40)):
        for fit in (dict(anchor="center"), dict(anchor="topleft"), None):
            geom = rot_geometry_ref(hw[0], hw[1], NET[0], NET[1], rot, fit is None, **(fit or {}))
            d, s, l = unrot_table(rng, geom, NET, 4, 40)
            counts = [40, 49, 17, 31]
            want, gc, gf = check_unrot(hw, NET, rot, fit, d, s, l, counts, 64)
            assert gf.tolist() == [0, 1, 0, 0]
            kept = want[0][0]
            assert any(r[0] > r[2] and r[1] > r[3] for r in kept), "the inverted box stays inverted"
            if rot == 0:
                assert any(np.signbit(r[0]) and r[0] == 0 for r in kept) == (geom[2] == 0)      # -0.0 - dx keeps its sign only for dx = 0
            check_unrot(hw, NET, rot, fit, d, s, l, counts, 3)                                  # max_out below the kept count
    geom = rot_geometry_ref(40, 120, NET[0], NET[1], rot, 0)
    d, s, l = unrot_table(rng, geom, NET, 2, 1100)
    want, gc, _ = check_unrot((40, 120), NET, rot, {}, d, s, l, [1100, 1030], 1100)
    assert gc[0] > 400 and gc[1] > 400


# ------------------------------------------------------------------------------------------ the engine
def rot_engine(hw, fmt, rot, fit, seed=0, need=2, **engine):
    """A 64 x 96 context with the default (synthetic) weights and two STORED frames of ``hw`` whose rotated forward, decoded at a score
    threshold read off the heat maps (at least 6 cells of the content above it in every image), keeps ``need`` rows with their centre in
    the content whose mapped box has an area inside the stored frame: (engine, dense frames, threshold, the decode's rows)."""
    h, w = hw
    rw, rh, dx, dy = geom = rot_geometry_ref(h, w, NET[0], NET[1], rot, fit is None, **(fit or {}))
    eng = cfa.Engine(NET[0], NET[1], max_batch=4, dtype="bf16", **engine)
    tried = []
    for k, kind in enumerate(("blocks", "binary", "noise") * 4):
        rng = np.random.default_rng(seed + 10 * k)
        dense = source_frames(rng, kind, (2, h, w, 3) if fmt == "bgr" else (2, h * 3 // 2, w))
        eng.forward_rot_enqueue(dense, fmt, rot, fit=fit)
        hm = eng.heads(sigmoid_hm=True)["hm_sigmoid"].reshape(2, NET[0] // 4, NET[1] // 4)
        inside = hm[:, (dy + 3) // 4:(dy + rh) // 4, (dx + 3) // 4:(dx + rw) // 4].reshape(2, -1)
        thr = float(np.nextafter(np.float32(np.sort(inside, 1)[:, -6].min()), np.float32(0)))
        per = eng.decode_threshold(thr, 0.5, 256)
        mapped = unrot_ref(geom, hw, rot, *net_tables(per))[0]
        kept = [len(x) for x, _ in mapped]
        solid = sum(int(((x[:, 2] - x[:, 0] >= 2) & (x[:, 3] - x[:, 1] >= 2) & (x[:, 2] > 0) & (x[:, 3] > 0) & (x[:, 0] < w) & (x[:, 1] < h)).sum())
                    for x, _ in mapped)
        tried.append((kind, thr, [len(x) for x, _ in per], kept, solid))
        if min(kept) >= 1 and sum(kept) >= need and solid >= need:
            print("rot_engine:", tried)
            return eng, dense, thr, per
    raise AssertionError(tried)


@pytest.mark.parametrize("fmt,rot,fit", (("bgr", 90, {}), ("nv12", 270, {}), ("bgr", 270, None), ("nv12", 90, None)))
def test_engine_rot_decode_unfit_and_the_consumers(fmt, rot, fit):
    """forward_rot on stored frames F = the fitted (stretched) forward of their upright view: the network input and the decode's rows are
    byte-identical; unfit_rows is the restated map of those rows into F's pixels; the redaction of F uses them on every byte; the state
    rules are the fit's."""
    hw = (40, 120)
    h, w = hw
    geom = rot_geometry_ref(h, w, NET[0], NET[1], rot, fit is None, **(fit or {}))
    eng, dense, thr, per = rot_engine(hw, fmt, rot, fit, seed=3)
    staged, heads = eng.resized_input(), eng.heads()
    turned = np.stack([upright(f, rot) for f in bgr_of(dense, fmt)])                      # the BGR restatement, turned
    assert np.array_equal(staged, np.stack([rot_ref(f, rot, NET[0], NET[1], fit is None, **(fit or {})) for f in bgr_of(dense, fmt)]))
    solid = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    views, bufs, _, _ = pitched_frames(dense, fmt, 0xFF)
    for call in (lambda: eng.redact_faces(views, fmt, **solid), eng.merge_tiles):          # no unfit_rows yet; and it is not a tiled forward
        with pytest.raises(cfa._lib.CenterFaceError) as e:
            call()
        assert e.value.code == CF_ESTATE
    want, wflags = unrot_ref(geom, hw, rot, *net_tables(per))
    got, flags = eng.unfit_rows(256)
    print("kept per image:", [len(x) for x, _ in per], "in the content:", [len(x) for x, _ in got])
    assert same_results(got, want) and flags.tolist() == wflags.tolist() == [0, 0]
    assert same_results(eng.unfit_rows(max_out=1)[0], want)                              # the wrapper comes back for all of them
    with pytest.raises(cfa._lib.CenterFaceError) as e:                                   # still no tiled forward
        eng.merge_tiles()
    assert e.value.code == CF_ESTATE
    # the redaction of the STORED frames with the mapped boxes, which are in their pixels: (H, W) = (h, w)
    boxes = np.concatenate([x[:, :4] for x, _ in want])
    counts = np.array([len(x) for x, _ in want], np.int32)
    wviews, wbufs, _, _ = pitched_frames(dense, fmt, 0xFF)
    redact_ref(wviews, fmt, boxes, counts, (h, w), h, w, **solid)
    eng.redact_faces(views, fmt, **solid)
    assert all(np.array_equal(a, b) for a, b in zip(bufs, wbufs))
    assert not all(np.array_equal(a, b) for a, b in zip(bufs, pitched_frames(dense, fmt, 0xFF)[1]))      # something was redacted
    # one upright-fitted chip per mapped row, cut from the stored frames
    chips, offs, _ = eng.align_faces_frame(dense, fmt, 32)
    assert np.diff(offs).tolist() == counts.tolist() and len(chips) == int(counts.sum())
    # the tracker accepts the rows as B frames of (h, w): every row starts a track
    trk = cfa.Tracker(eng, 2, min_hits=1)
    M = trk.max_tracks
    dev = [eng.device_alloc(2 * M * 3 * 4), eng.device_alloc(8)]
    eng.track_update_device(trk, 0, info_ptr=dev[0], counts_ptr=dev[1])
    eng.synchronize()
    tc = np.empty(2, np.int32)
    eng.memcpy_d2h(tc, dev[1])
    for p in dev:
        eng.device_free(p)
    assert tc.tolist() == counts.tolist()
    trk.close()
    # the same network input and rows as the upright view through the paths of before
    if fit is None:
        eng.forward_resized_enqueue(turned)
    else:
        eng.forward_fit_enqueue(turned, "bgr", **fit)
    assert np.array_equal(eng.resized_input(), staged) and heads_equal(eng.heads(), heads)
    assert same_results(eng.decode_threshold(thr, 0.5, 256), per)
    # ... which forget the turn: the fit's own rows, or none
    if fit is None:
        with pytest.raises(cfa._lib.CenterFaceError) as e:
            eng.unfit_rows()
        assert e.value.code == CF_ESTATE
    else:
        ug = fit_geometry_ref(w, h, NET[0], NET[1])
        assert same_results(eng.unfit_rows(256)[0], unrot_ref(ug, (w, h), 0, *net_tables(per))[0])
    # a rotated forward without a decode, and an upload behind one
    eng.forward_rot_enqueue(dense, fmt, rot, fit=fit)
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        eng.unfit_rows()
    assert e.value.code == CF_ESTATE
    eng.decode_threshold(thr, 0.5, 256)
    eng.upload_images(list(staged))
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        eng.unfit_rows()
    assert e.value.code == CF_ESTATE
    # refusals name the value and leave the engine working
    with pytest.raises(ValueError) as e:
        eng.forward_rot_enqueue(dense, fmt, 45)
    assert "rot=45" in str(e.value)
    with pytest.raises(ValueError) as e:
        eng.forward_rot_enqueue(np.concatenate([dense, dense, dense]), fmt, rot)
    assert "max_batch" in str(e.value) and "B=6" in str(e.value)
    eng.forward_rot_enqueue(dense, fmt, rot, fit=fit)
    assert np.array_equal(eng.resized_input(), staged)
    eng.close()


def test_engine_rot_180_and_device_planes():
    """rot 180 through the engine, host-staged and in place on device planes (which stay untouched): the restated canvases."""
    hw, fmt = (40, 120), "nv12"
    dense, bgr = fit_case(fmt, hw)
    fit = dict(anchor="center", fill=(1, 2, 3))
    eng = cfa.Engine(NET[0], NET[1], max_batch=4, dtype="bf16")
    for rot in (180, 90):
        want = canvases_ref(fmt, hw, rot, NET, False, **fit)
        eng.forward_rot_enqueue(pitched_frames(dense, fmt, 0xFF)[0], fmt, rot, fit=fit)
        assert np.array_equal(eng.resized_input(), want)
        views, bufs, p0, p1 = pitched_frames(dense, fmt, 0x00, aligned=True)
        dev = [eng.device_alloc(b.nbytes) for b in bufs]
        for d, b in zip(dev, bufs):
            eng.memcpy_h2d(d, b)
        n = len(views[0])
        planes = [tuple(dev[b * n:(b + 1) * n]) for b in range(3)]
        eng.forward_rot_enqueue(planes, fmt, rot, fit=fit, on_device=True, h=hw[0], w=hw[1], pitch0=p0, pitch1=p1)
        assert np.array_equal(eng.resized_input(), want), rot
        for d, b in zip(dev, bufs):
            back = np.empty_like(b)
            eng.memcpy_d2h(back, d)
            assert np.array_equal(back, b)
            eng.device_free(d)
    eng.close()


def test_flip_engine_behind_a_rotated_forward():
    """A context in flip test: the heads behind forward_rot are the restated merge of a plain engine's records of the turned canvases
    with their mirror appended."""
    sd = cfa.weights.synthetic_state_dict(0)
    dense = fit_case("bgr", (40, 120))[0][:2]
    canvases = canvases_ref("bgr", (40, 120), 90, NET, False)[:2]
    plain = cfa.Engine(NET[0], NET[1], max_batch=4, dtype="bf16", weights=sd)
    want, _ = flip_heads_ref(plain_records(plain, canvases), 2)
    plain.close()
    eng = cfa.Engine(NET[0], NET[1], max_batch=2, dtype="bf16", weights=sd, flip_test=True)
    eng.forward_rot_enqueue(dense, "bgr", 90, fit=True)
    assert np.array_equal(eng.resized_input()[:2], canvases)
    assert_heads(eng.heads(sigmoid_hm=True), want, "flip behind rot 90")
    eng.close()


# ------------------------------------------------------------------------------------------ the product path
def test_centerface_rotate_keyword():
    """anonymize(rotate=90, fit=True) and anonymize_yuv(rotate=270) equal the same calls made by hand on the engine; rotate=0 is the call
    without the keyword; rotate with tiled=True raises."""
    h, w = 40, 120
    face = cfa.CenterFace(NET[0], NET[1], dtype="bf16", max_batch=4)
    eng = face.engine
    opts = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    for fmt, rot, fit in (("bgr", 90, True), ("nv12", 270, None)):
        rng, tried = np.random.default_rng(4), []
        for kind in ("blocks", "binary", "noise") * 2:                     # the default weights answer to one of them
            frames = source_frames(rng, kind, (2, h, w, 3) if fmt == "bgr" else (2, h * 3 // 2, w))
            keep = frames.copy()
            if fmt == "bgr":
                out, dets = face.anonymize(list(frames), rotate=rot, fit=fit, **opts)
            else:
                out, dets = face.anonymize_yuv(frames, fmt, rotate=rot, fit=fit, **opts)
            tried.append((kind, [len(d) for d, _ in dets]))
            if sum(len(d) for d, _ in dets) >= 2:
                break
        print("rotate:", fmt, rot, tried)
        assert sum(len(d) for d, _ in dets) >= 2, tried
        assert np.array_equal(frames, keep)                                # the inputs stay untouched
        eng.forward_rot_enqueue(frames, fmt, rot, fit={} if fit else None)
        eng.decode_threshold(0.3, face.nms_thresh, face.max_dets)
        rows = eng.unfit_rows(face.max_dets)[0]
        assert same_results(dets, rows)
        hand = frames.copy()
        eng.cover_faces(hand, fmt, **opts)
        assert np.array_equal(out, hand) and not np.array_equal(out, keep)
        if fmt == "bgr":
            assert same_results(face.detect_fit(frames, rotate=rot), rows)
            got = face.detect_aligned_frames(frames, "bgr", 32, rotate=rot, fit=True)
            assert same_results([r[:2] for r in got], rows) and [len(r[2]) for r in got] == [len(d) for d, _ in rows]
    # rotate=0: the call without the keyword, bytewise (frames of the instance's size: the plain path; and a fitted one)
    imgs = source_frames(np.random.default_rng(5), "blocks", (2,) + NET + (3,))
    a, b = face.anonymize(list(imgs), **opts), face.anonymize(list(imgs), rotate=0, **opts)
    assert a[0].tobytes() == b[0].tobytes() and same_results(a[1], b[1])
    other = source_frames(np.random.default_rng(7), "blocks", (2, h, w, 3))
    a, b = face.anonymize(list(other), fit=True, **opts), face.anonymize(list(other), fit=True, rotate=0, **opts)
    assert a[0].tobytes() == b[0].tobytes() and same_results(a[1], b[1])
    yuv = source_frames(np.random.default_rng(6), "blocks", (2, NET[0] * 3 // 2, NET[1]))
    a, b = face.anonymize_yuv(yuv, "nv12", **opts), face.anonymize_yuv(yuv, "nv12", rotate=0, **opts)
    assert a[0].tobytes() == b[0].tobytes() and same_results(a[1], b[1])
    for call in (lambda: face.anonymize(list(imgs), rotate=90, tiled=True), lambda: face.anonymize_yuv(yuv, "nv12", rotate=90, tiled=True),
                 lambda: face.annotate(list(imgs), rotate=90, tiled=True), lambda: face.detect_aligned_frames(imgs, rotate=90, tiled=True)):
        with pytest.raises(ValueError):
            call()
    face.close()


def test_demo_rotate(tmp_path, capsys):
    """``demo --rotate 90`` on an image file stored turned: a context of the upright view's size, the faces redacted in the image as
    stored -- the bytes of ``CenterFace.anonymize(rotate=90)`` on the decoded file."""
    from PIL import Image
    from centerface_amd import demo
    frame = source_frames(np.random.default_rng(8), "blocks", (1, 64, 96, 3))[0]
    path, out = str(tmp_path / "turned.png"), str(tmp_path / "out.png")
    Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(path)
    opts = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    dets, _ = demo.anonymize_file(path, out, rotate=90, **opts)
    face = cfa.CenterFace(96, 64, dtype="bf16")                             # (height, width) of the upright view
    want, res = face.anonymize([demo.imread(path)], rotate=90, **opts)
    fitted, _ = face.detect_fit(demo.imread(path)[None], rotate=90)[0]
    face.close()
    assert dets.tobytes() == res[0][0].tobytes()
    assert np.array_equal(demo.imread(out), want[0])
    capsys.readouterr()
    demo.main([path, "--rotate", "90"])                                     # the detections alone: path line, count line, rows
    assert capsys.readouterr().out == demo.format_wider_result(path, fitted)
    with pytest.raises(SystemExit):
        demo.main([path, "--rotate", "90", "--tiled", "64", "--anonymize", out])
    with pytest.raises(SystemExit):
        demo.main([path, "--rotate", "45"])
