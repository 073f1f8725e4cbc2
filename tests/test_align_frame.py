"""Aligned chips cut from the source frame on the GPU (cf_op_align_frame, cf_align_faces_frame, Engine.align_faces_frame[_device],
CenterFace.detect_aligned_frames): chips and float64 matrices BIT FOR BIT against the restatement of tests/test_align_frame_abi.py --
tests/test_align.py's estimate and warp applied to the frame (converted by tests/test_yuv_input.py's restatement for 4:2:0), the
landmarks in frame pixels: as given (the kernel alone, merged rows) or the decode's network-coordinate rows mapped in float64."""
import ctypes as C

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from test_align import align_ref, bits_equal, hard_landmarks, pose_landmarks
from test_align_frame_abi import FORMATS, bgr_of, frame_align_ref, net_to_frame, pitched_planes
from test_redact import redact_ref, source_frames
from test_tiles import FRAME_HW, tiled_engine

pytestmark = pytest.mark.gpu
L = cfa._lib
F32 = dict(out="f32", rgb=True, mean=127.5, scale=1 / 128.0)

# name -> (formats, B, h, w, (pitch0, pitch1) per format kind or None = dense, [(S, chip options)], pose scale)
OP_CASES = {
    "a": (("bgr",), 3, 151, 203, {"bgr": (612, 0)}, [(112, dict(out="u8"))], (0.15, 4.0)),
    "b": (FORMATS[1:], 3, 150, 202, {"il": (208, 208), "planar": (208, 104)}, [(16, dict(out="u8")), (128, F32)], (0.15, 4.0)),
    "c": (FORMATS, 1, 64, 80, None, [(512, dict(out="u8"))], (0.15, 1.2)),
    "d": (FORMATS, 64, 48, 64, None, [(112, dict(out="u8"))], (0.15, 4.0)),
}


def _kind(fmt):
    return "bgr" if fmt == "bgr" else "il" if fmt in ("nv12", "nv21") else "planar"


def _dense_pitches(fmt, w):
    return {"bgr": (3 * w, 0), "il": (w, w), "planar": (w, w // 2)}[_kind(fmt)]


def op_inputs(name, fmt, S):
    """(dense frames, landmark rows, counts) of one case: random poses reaching 20 % over every edge, the 12 hard rows, two poses far
    outside; B = 64: random counts 0..4 with zeros, the hard rows all in image 1."""
    _, B, h, w, _, _, scale = OP_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name + fmt)) * 1000 + S)
    dense = rng.integers(0, 256, (B, h, w, 3) if fmt == "bgr" else (B, h * 3 // 2, w), dtype=np.uint8)
    if B == 64:
        counts = rng.integers(0, 5, B).astype(np.int32)
        counts[[0, 7, 63]] = 0
        counts[1] = 14
        first = int(counts[:1].sum())
    else:
        counts = np.array([19, 0, 5][:B] if B == 3 else [20], np.int32)
        first = 0
    lms = pose_landmarks(rng, int(counts.sum()), h, w, S, scale=scale, margin=-0.2)
    lms[first:first + 12] = hard_landmarks(rng, h, w, S)
    lms[first + 12] += np.float32(3000.0)                           # alignable, wholly outside
    lms[first + 13] -= np.float32(2500.0)
    return dense, lms, counts


_ref_cache = {}


def op_reference(name, fmt, S, opt):
    key = (name, fmt, S, opt["out"])
    if key not in _ref_cache:
        dense, lms, counts = op_inputs(name, fmt, S)
        stats = {}
        want_c, want_m = frame_align_ref(bgr_of(dense, fmt), lms.astype(np.float64), counts, S, stats=stats, **opt)
        _ref_cache[key] = (dense, lms, counts, want_c, want_m, stats)
    return _ref_cache[key]


@pytest.mark.parametrize("fmt", FORMATS)
def test_op_align_frame_bit_exact(fmt):
    """The kernel alone, every format: pitched BGR rows with 3w % 4 != 0, pitched 4:2:0 planes of both chroma layouts, a dense frame
    with S = 512, 64 small frames with counts 0..4.  The padding bytes hold 0x00 in one run and 0xFF in the other: both runs equal each
    other and the restatement.  Every plane is uploaded as exactly rows x pitch bytes."""
    ran = 0
    for name, (fmts, B, h, w, pitches, variants, _) in OP_CASES.items():
        if fmt not in fmts:
            continue
        p0, p1 = pitches[_kind(fmt)] if pitches else _dense_pitches(fmt, w)
        for S, opt in variants:
            dense, lms, counts, want_c, want_m, stats = op_reference(name, fmt, S, opt)
            print("case %s %s S=%d %s: %d faces, %s" % (name, fmt, S, opt["out"], len(want_m), stats))
            assert stats["zero"] >= 6 and stats["partial"] >= 3 and stats["outside"] >= 3, (name, fmt, S, stats)
            got = []
            for pad in (0x00, 0xFF):
                views, bufs = pitched_planes(dense, fmt, p0, p1, pad)
                assert all(b.shape[1] in (p0, p1) for b in bufs)
                got.append(ops.align_frame(views, lms, counts, fmt, size=S, **opt))
                gc, gm = got[-1]
                assert gc.dtype == want_c.dtype and gc.shape == want_c.shape
                assert bits_equal(gm, want_m), (name, fmt, S, pad, np.argwhere(gm != want_m)[:5])
                assert bits_equal(gc, want_c), (name, fmt, S, pad, np.argwhere(gc != want_c)[:5])
            assert bits_equal(got[0][0], got[1][0]) and bits_equal(got[0][1], got[1][1])
            ran += 1
    assert ran >= 3
    # a per-image limit, dense arrays whose pitch the wrapper has to pad (3 * 203 = 609), and no faces at all
    if fmt == "bgr":
        dense, lms, counts, want_c, want_m, _ = op_reference("a", "bgr", 112, dict(out="u8"))
        gc, gm = ops.align_frame(dense, lms, counts, "bgr", size=112, max_per_image=2)
        first = np.concatenate([[0], np.cumsum(counts)])[:-1]
        rows = np.concatenate([np.arange(f, f + min(c, 2)) for f, c in zip(first, counts)])
        assert bits_equal(gc, want_c[rows]) and bits_equal(gm, want_m[rows])
    c0, m0 = ops.align_frame(op_inputs("c", fmt, 512)[0], np.zeros((0, 10), np.float32), np.zeros(1, np.int32), fmt, size=16)
    assert c0.shape == (0, 16, 16, 3) and m0.shape == (0, 6)


@pytest.mark.parametrize("fmt", ("i420", "bgr"))
def test_op_align_frame_more_frames_than_one_launch(fmt):
    """65 frames of 32 x 32 (one launch takes 64): two faces in frame 0, one in frame 63 (the first launch's last) and two in frame 64
    (the second launch's only frame, at table entry 0).  The face numbering runs over all 65 counts in both launches: chips and
    matrices equal the restatement bit for bit, so they come in frame order -- every frame holds other noise."""
    B, h, w, S = 65, 32, 32, 16
    rng = np.random.default_rng(80 + FORMATS.index(fmt))
    dense = rng.integers(0, 256, (B, h, w, 3) if fmt == "bgr" else (B, h * 3 // 2, w), dtype=np.uint8)
    counts = np.zeros(B, np.int32)
    counts[[0, 63, 64]] = 2, 1, 2
    lms = pose_landmarks(rng, 5, h, w, S, scale=(0.1, 0.2), margin=0.2)   # faces of 11..22 pixels, centred inside the frame
    want_c, want_m = frame_align_ref(bgr_of(dense, fmt), lms.astype(np.float64), counts, S)
    assert len(want_m) == 5 and want_m.any(1).all() and all(c.any() for c in want_c)
    assert len({c.tobytes() for c in want_c}) == 5
    gc, gm = ops.align_frame(dense, lms, counts, fmt, size=S)
    assert bits_equal(gm, want_m), np.argwhere(gm != want_m)[:5]
    assert bits_equal(gc, want_c), np.argwhere(gc != want_c)[:5]


# ------------------------------------------------------------------------------------------ the engine, not tiled
ENG_HW, SRC_HW = (96, 128), (150, 202)


def _custom_template(S):
    return (np.float32([[0.30, 0.35], [0.70, 0.36], [0.5, 0.55], [0.35, 0.74], [0.66, 0.75]]) * np.float32(S)).astype(np.float32)


def feed_frames(eng, fmt, rng, need=2, hw=SRC_HW):
    """Frames of ``hw`` the default weights keep ``need`` faces in behind forward_resized (BGR) / forward_yuv: (dense frames, decode)."""
    tried = []
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        src = source_frames(rng, kind, (3,) + hw + (3,) if fmt == "bgr" else (3, hw[0] * 3 // 2, hw[1]))
        eng.forward_resized_enqueue(src) if fmt == "bgr" else eng.forward_yuv_enqueue(src, fmt)
        base = eng.decode_threshold(0.3, 0.3, 64)
        tried.append((kind, [len(d) for d, _ in base]))
        if sum(len(d) for d, _ in base) >= need:
            print("feed %s: %s" % (fmt, tried[-1],))
            return src, base
    raise AssertionError("no source kept %d faces with the default weights: %s" % (need, tried))


@pytest.mark.parametrize("fmt", ("bgr", "nv12"))
def test_engine_align_faces_frame_equals_restatement(fmt):
    """Behind forward_resized (BGR 150 x 202) / forward_yuv (NV12 150 x 202) + decode_threshold on a 96 x 128 context: the chips of the
    frames with the decode's UNRESCALED landmarks mapped by 202 / 128, 150 / 96 in float64 (an anisotropic map), rescale off and on,
    with a per-image limit; the decode, align_faces and redact_faces are not disturbed by the call."""
    rng = np.random.default_rng(40 + FORMATS.index(fmt))
    eng = cfa.Engine(ENG_HW[0], ENG_HW[1], max_batch=3, dtype="bf16")
    src, base = feed_frames(eng, fmt, rng)
    counts = np.array([len(d) for d, _ in base], np.int32)
    pts = net_to_frame(np.concatenate([l for _, l in base]), SRC_HW, ENG_HW)
    bgr = bgr_of(src, fmt)
    net_chips = eng.align_faces(112)
    red_opt = dict(mode="mosaic", shape="ellipse", cell=6)
    redacted = eng.redact_faces(src.copy(), fmt, **red_opt)
    assert not np.array_equal(redacted, src)
    pitch = (612, 0) if fmt == "bgr" else (208, 208)
    for rescale, opt in ((False, dict(size=112)), (True, dict(size=128, template=_custom_template(128), **F32))):
        eng.set_rescale(1.37, 1.21) if rescale else eng.set_rescale(0.0, 0.0)
        dec = eng.decode_threshold(0.3, 0.3, 64)
        views, _ = pitched_planes(src, fmt, pitch[0], pitch[1], 0xFF)      # host frames with padded rows: only the row bytes go up
        chips, offs, mats = eng.align_faces_frame(views if rescale else src, fmt, **opt)
        again = eng.decode_threshold(0.3, 0.3, 64)
        for (d, l), (d2, l2), (d0, l0) in zip(dec, again, base):
            assert bits_equal(d, d2) and bits_equal(l, l2)
            assert rescale or (bits_equal(l, l0) and bits_equal(d, d0))
        assert np.array_equal(offs, np.concatenate([[0], np.cumsum(counts)]))
        want_c, want_m = frame_align_ref(bgr, pts, counts, **opt)
        assert len(chips) == len(want_c) == int(counts.sum())
        assert bits_equal(mats, want_m) and bits_equal(chips, want_c), (fmt, rescale)
        assert int(want_m.any(1).sum()) >= 1, "no alignable face in this case: nothing was compared"
    eng.set_rescale(0.0, 0.0)
    eng.decode_threshold(0.3, 0.3, 64)
    chips1, offs1, mats1 = eng.align_faces_frame(src, fmt, 112, max_per_image=1)
    want_c, want_m = frame_align_ref(bgr, pts, counts, 112, max_per_image=1)
    assert np.array_equal(offs1, np.concatenate([[0], np.cumsum(np.minimum(counts, 1))]))
    assert bits_equal(chips1, want_c) and bits_equal(mats1, want_m)
    # the network-batch chips and the redaction behind the call are what they were before it
    after = eng.align_faces(112)
    assert all(bits_equal(a, b) for a, b in zip(after, net_chips))
    assert np.array_equal(eng.redact_faces(src.copy(), fmt, **red_opt), redacted)
    # the wrong B is refused
    with pytest.raises(ValueError):
        eng.align_faces_frame(src[:2], fmt)
    eng.close()


def test_engine_align_faces_frame_of_the_network_batch_equals_align_faces():
    """Frames of exactly (H, W) through forward_enqueue: the map is the identity, the two entry points agree bit for bit."""
    rng = np.random.default_rng(50)
    eng = cfa.Engine(ENG_HW[0], ENG_HW[1], max_batch=3, dtype="bf16")
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        x = source_frames(rng, kind, (3,) + ENG_HW + (3,))
        eng.forward_enqueue(x)
        if sum(len(d) for d, _ in eng.decode_threshold(0.3, 0.3, 64)) >= 2:
            break
    for opt in (dict(size=112), dict(size=64, **F32)):
        want = eng.align_faces(**opt)
        got = eng.align_faces_frame(x, "bgr", **opt)
        assert len(want[0]) >= 2 and all(bits_equal(a, b) for a, b in zip(got, want))
    # behind a float NCHW forward the network batch is not read: fine
    xf = (x.astype(np.float32) / 255.0 - cfa.CenterFace.mean) / cfa.CenterFace.std
    eng.forward_enqueue(np.ascontiguousarray(xf.transpose(0, 3, 1, 2)))
    base = eng.decode_threshold(0.3, 0.3, 64)
    counts = np.array([len(d) for d, _ in base], np.int32)
    chips, offs, mats = eng.align_faces_frame(x, "bgr", 112)
    want_c, want_m = align_ref(x, np.concatenate([l for _, l in base]), counts, 112)
    assert bits_equal(chips, want_c) and bits_equal(mats, want_m) and offs[-1] == counts.sum()
    eng.close()


# ------------------------------------------------------------------------------------------ the engine, tiled
@pytest.mark.parametrize("fmt", ("bgr", "nv12"))
def test_engine_align_faces_frame_after_a_merge_uses_the_merged_rows(fmt):
    eng, dense, rects, thr = tiled_engine(fmt, seed=1)
    h, w = FRAME_HW
    eng.decode_threshold(thr, 0.5, 256)
    with pytest.raises(cfa._lib.CenterFaceError) as e:                     # a tiled forward and a decode, but no merge
        eng.align_faces_frame(dense, fmt)
    assert e.value.code == L.CF_ESTATE
    merged, _ = eng.merge_tiles(max_out=256)
    counts = np.array([len(d) for d, _ in merged], np.int32)
    lms = np.concatenate([l for _, l in merged])
    assert counts.sum() >= 2
    bgr = bgr_of(dense, fmt)
    for opt in (dict(size=112), dict(size=32, **F32)):
        chips, offs, mats = eng.align_faces_frame(dense, fmt, **opt)
        want_c, want_m = align_ref(bgr, lms, counts, **opt)
        assert offs.shape == (3,) and np.array_equal(offs, np.concatenate([[0], np.cumsum(counts)]))      # [Bf + 1], not [Bf * T + 1]
        assert bits_equal(mats, want_m) and bits_equal(chips, want_c), (fmt, opt)
        assert int(want_m.any(1).sum()) >= 1
    full_c, _, full_m = eng.align_faces_frame(dense, fmt, 112)
    # the wrong B or frame size is refused
    crop = dense[:, :h - 2, :w - 2] if fmt == "bgr" else np.ascontiguousarray(dense[:, :(h - 2) * 3 // 2, :w - 2])
    for bad in (dense[:1], np.ascontiguousarray(crop)):
        with pytest.raises(ValueError):
            eng.align_faces_frame(bad, fmt)
    # the redaction behind it still takes the merged boxes
    boxes = np.concatenate([d[:, :4] for d, _ in merged])
    red_opt = dict(mode="mosaic", shape="ellipse", cell=6)
    views, bufs = pitched_planes(dense, fmt, *((3 * w + 6, 0) if fmt == "bgr" else (w + 4, w + 4)), 0xFF)
    wviews, wbufs = pitched_planes(dense, fmt, *((3 * w + 6, 0) if fmt == "bgr" else (w + 4, w + 4)), 0xFF)
    redact_ref(wviews, fmt, boxes, counts, (h, w), h, w, **red_opt)
    eng.redact_faces(views, fmt, **red_opt)
    assert all(np.array_equal(a, b) for a, b in zip(bufs, wbufs))
    # a merge that wrote fewer rows than it kept (device form, max_out = 1): the counts are clamped, the first row of every frame is a face
    eng.merge_tiles_device(1)
    c1, o1, m1 = eng.align_faces_frame(dense, fmt, 112)
    firsts = np.concatenate([[0], np.cumsum(counts)])[:-1][counts > 0]
    assert np.array_equal(o1, np.concatenate([[0], np.cumsum(np.minimum(counts, 1))]))
    assert bits_equal(c1, full_c[firsts]) and bits_equal(m1, full_m[firsts])
    # a new decode forgets the merge
    eng.decode_threshold(thr, 0.5, 256)
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        eng.align_faces_frame(dense, fmt)
    assert e.value.code == L.CF_ESTATE
    eng.close()


# ------------------------------------------------------------------------------------------ device form, truncation, state
def test_engine_align_faces_frame_device_form_truncation_and_state():
    rng = np.random.default_rng(60)
    eng = cfa.Engine(ENG_HW[0], ENG_HW[1], max_batch=3, dtype="bf16")
    lib, P = L.lib(), L.ptr
    h, w = SRC_HW
    frames = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)

    def refused():
        with pytest.raises(cfa._lib.CenterFaceError) as e:
            eng.align_faces_frame(frames, "bgr")
        assert e.value.code == L.CF_ESTATE
    refused()                                                              # before any forward
    src, base = feed_frames(eng, "bgr", rng)
    eng.forward_resized_enqueue(src)
    refused()                                                              # before any threshold decode
    eng.decode_topk(10)
    refused()
    eng.decode_threshold(0.3, 0.3, 64)
    eng.upload_images(list(src))
    refused()                                                              # an upload was started
    for fmt in ("bgr", "nv12", "yv12"):
        src, base = feed_frames(eng, fmt, rng) if fmt != "yv12" else (src, base)
        if fmt == "yv12":                                                  # the NV12 forward's faces, cut from other frames
            src = rng.integers(0, 256, src.shape, dtype=np.uint8)
        total = sum(len(d) for d, _ in base)
        opt = dict(size=64, **F32) if fmt == "nv12" else dict(size=112)
        want_c, want_o, want_m = eng.align_faces_frame(src, fmt, **opt)
        assert len(want_c) == total == want_o[-1] and total >= 2
        # device planes of EXACTLY rows x pitch bytes each (pitches rounded up to 4, the padding 0xFF), device outputs
        p0, p1 = {"bgr": (608, 0), "nv12": (208, 208), "yv12": (204, 104)}[fmt]
        views, bufs = pitched_planes(src, fmt, p0, p1, 0xFF)
        dev = [eng.device_alloc(b.nbytes) for b in bufs]
        for d, b in zip(dev, bufs):
            eng.memcpy_h2d(d, b)
        n = len(bufs) // 3
        planes = [tuple(dev[b * n:(b + 1) * n]) for b in range(3)]
        one = want_c[0].nbytes
        dc, dm, do = eng.device_alloc(total * one), eng.device_alloc(total * 48), eng.device_alloc(16)
        eng.align_faces_frame_device(planes, fmt, 3, h, w, p0, p1, dc, do, total, dm, **opt)
        eng.synchronize()
        gc, gm, go = np.empty_like(want_c), np.empty((total, 6)), np.empty(4, np.int32)
        for a, d in ((gc, dc), (gm, dm), (go, do)):
            eng.memcpy_d2h(a, d)
        assert bits_equal(gc, want_c) and bits_equal(gm, want_m) and np.array_equal(go, want_o), fmt
        # truncation: the later rows stay untouched, offsets[-1] tells the number wanted; cap_faces = 0 still writes the offsets
        cap = total - 1
        fill_c, fill_m = np.full_like(want_c, 7), np.full((total, 6), -7.0)
        for capn in (cap, 0):
            eng.memcpy_h2d(dc, fill_c), eng.memcpy_h2d(dm, fill_m), eng.memcpy_h2d(do, np.full(4, -1, np.int32))
            eng.align_faces_frame_device(planes, fmt, 3, h, w, p0, p1, dc, do, capn, dm, **opt)
            eng.synchronize()
            for a, d in ((gc, dc), (gm, dm), (go, do)):
                eng.memcpy_d2h(a, d)
            assert np.array_equal(go, want_o) and go[-1] == total
            assert bits_equal(gc[:capn], want_c[:capn]) and bits_equal(gm[:capn], want_m[:capn])
            assert bits_equal(gc[capn:], fill_c[capn:]) and bits_equal(gm[capn:], fill_m[capn:])
        c2, o2, m2 = eng.align_faces_frame(src, fmt, max_faces=cap, **opt)
        assert len(c2) == cap and o2[-1] == total and bits_equal(c2, want_c[:cap]) and bits_equal(m2, want_m[:cap])
        c3, o3, _ = eng.align_faces_frame(src, fmt, max_faces=0, **opt)
        assert len(c3) == 0 and np.array_equal(o3, want_o)
        # a misaligned device plane, a pitch that is no multiple of 4, misaligned chips
        with pytest.raises(ValueError):
            eng.align_faces_frame_device([(planes[0][0] + 2,) + planes[0][1:]] + planes[1:], fmt, 3, h, w, p0, p1, dc, do, total, dm, **opt)
        with pytest.raises(ValueError):
            eng.align_faces_frame_device(planes, fmt, 3, h, w, p0 + 2, p1, dc, do, total, dm, **opt)
        with pytest.raises(ValueError):
            eng.align_faces_frame_device(planes, fmt, 3, h, w, p0, p1, dc + 4, do, total, dm, **opt)
        with pytest.raises(ValueError):
            eng.align_faces_frame_device(planes[:2], fmt, 2, h, w, p0, p1, dc, do, total, dm, **opt)
        # the host form on the device planes' bytes: host frames + device outputs, device frames + host outputs
        o = L.align_opts(**opt)[0]
        tab = L.device_planes(planes)
        hc, hm, ho = np.empty_like(want_c), np.empty((total, 6)), np.empty(4, np.int32)
        assert lib.cf_align_faces_frame(eng._h, C.byref(o), L.frame_format(fmt), tab, 1, 3, h, w, p0, p1, P(hc), P(hm), P(ho), total, 0) == 0
        assert bits_equal(hc, want_c) and bits_equal(hm, want_m) and np.array_equal(ho, want_o)
        for d in dev + [dc, dm, do]:
            eng.device_free(d)
    eng.close()


# ------------------------------------------------------------------------------------------ CenterFace
def test_centerface_detect_aligned_frames():
    """Plain: dets / lms those of detect_batch / detect_yuv (frame pixels), chips = the restatement on the frames with the network-space
    landmarks mapped in float64.  Tiled: dets / lms those of detect_tiled, chips = the restatement with the merged landmarks."""
    rng = np.random.default_rng(70)
    h, w = SRC_HW
    face = cfa.CenterFace(h, w, dtype="bf16", max_batch=2)
    net = (face.img_h_new, face.img_w_new)
    for fmt in ("bgr", "nv12"):
        for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
            frames = source_frames(rng, kind, (3, h, w, 3) if fmt == "bgr" else (3, h * 3 // 2, w))
            want = face.detect_batch(list(frames)) if fmt == "bgr" else face.detect_yuv(frames, fmt)
            if sum(len(d) for d, _ in want) >= 1:
                break
        got = face.detect_aligned_frames(frames, fmt, 112)
        assert len(got) == 3 and sum(len(d) for d, _, _ in got) >= 1
        bgr = bgr_of(frames, fmt)
        for i in (0, 2):                                                   # chunk by chunk (max_batch = 2)
            chunk = frames[i:i + 2]
            face.engine.forward_resized_enqueue(chunk) if fmt == "bgr" else face.engine.forward_yuv_enqueue(chunk, fmt)
            base = face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets)
            counts = [len(d) for d, _ in base]
            want_c, _ = frame_align_ref(bgr[i:i + 2], net_to_frame(np.concatenate([l for _, l in base]), (h, w), net), counts, 112)
            assert bits_equal(np.concatenate([c for _, _, c in got[i:i + 2]]), want_c)
        for (d, l, c), (wd, wl) in zip(got, want):
            assert bits_equal(d, wd) and bits_equal(l, wl)
            assert c.shape == (len(d), 112, 112, 3) and c.dtype == np.uint8
        f32 = face.detect_aligned_frames(frames, fmt, 64, **F32)
        assert all(c.shape == (len(d), 3, 64, 64) and c.dtype == np.float32 for d, _, c in f32)
    with pytest.raises(ValueError):
        face.detect_aligned_frames(frames[:, :100], "nv12")                 # not this instance's frame size
    face.close()
    # tiled
    fh, fw = FRAME_HW
    face = cfa.CenterFace(64, 96, dtype="bf16", max_batch=24)
    for kind in ("blocks", "binary", "noise", "blocks", "binary", "noise"):
        imgs = source_frames(rng, kind, (3, fh, fw, 3))
        want = face.detect_tiled(imgs)
        if sum(len(d) for d, _ in want) >= 2:
            break
    got = face.detect_aligned_frames(imgs, "bgr", 112, tiled=True)
    assert len(got) == 3 and sum(len(d) for d, _, _ in got) >= 2
    for (d, l, c), (wd, wl), img in zip(got, want, imgs):
        assert bits_equal(d, wd) and bits_equal(l, wl)
        want_c, _ = align_ref(img[None], wl, [len(wl)], 112)
        assert bits_equal(c, want_c)
    face.close()
    plain = cfa.CenterFace(96, 128, landmarks=False, dtype="bf16")
    with pytest.raises(ValueError):
        plain.detect_aligned_frames(np.zeros((1, 96, 128, 3), np.uint8))
    plain.close()
