"""4:2:0 video input: NV12 / NV21 / I420 / YV12 frames converted to BGR on the device (cf_forward_yuv, cf_op_yuv_to_bgr,
Engine.forward_yuv_enqueue, CenterFace.detect_yuv / detect_stream(fmt=...)).

The contract: every result for a frame f of format F is BIT-IDENTICAL to feeding cv2.cvtColor(f, cv2.COLOR_YUV2BGR_<F>) through the
uint8 BGR path of the same engine.  cv2 is not installable here, so -- as for the resize -- the conversion is pinned to OpenCV's
published fixed-point BT.601 limited-range statement (modules/imgproc/src/color_yuv.simd.hpp, scalar path; restated in numpy below)
and to known answers computed by hand from it, not to a cv2 binary."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from oracle import centerface_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("nv12", "nv21", "i420", "yv12")


# ------------------------------------------------------------------------------------------ numpy restatement
def bgr_from_yuv(Y, U, V):
    """OpenCV's YUV420 -> BGR arithmetic per pixel (int64 here; every intermediate fits int32)."""
    Y, U, V = (np.asarray(a, np.int64) for a in (Y, U, V))
    uu, vv = U - 128, V - 128
    y = np.maximum(Y - 16, 0) * 1220542
    b = (y + (1 << 19) + 2116026 * uu) >> 20
    g = (y + (1 << 19) - 852492 * vv - 409993 * uu) >> 20
    r = (y + (1 << 19) + 1673527 * vv) >> 20
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def yuv_planes(frame, fmt):
    """Y [h, w], U and V [h/2, w/2] of one frame in OpenCV's single-buffer [h*3/2, w] layout."""
    rows, w = frame.shape
    h = rows * 2 // 3
    Y, rest = frame[:h], frame[h:].reshape(-1)
    if fmt in ("nv12", "nv21"):
        c = rest.reshape(h // 2, w)
        a, b = c[:, 0::2], c[:, 1::2]
    else:
        q = (h // 2) * (w // 2)
        a, b = rest[:q].reshape(h // 2, w // 2), rest[q:].reshape(h // 2, w // 2)
    return (Y, a, b) if fmt in ("nv12", "i420") else (Y, b, a)


def yuv_to_bgr_ref(frame, fmt, size=None):
    """cv2.cvtColor(frame, COLOR_YUV2BGR_<fmt>) restated (each 2x2 luma block shares the chroma sample at (y/2, x/2)), then
    cv2.resize to ``size`` as the oracle restates it."""
    Y, U, V = yuv_planes(frame, fmt)
    up = lambda c: np.repeat(np.repeat(c, 2, 0), 2, 1)      # noqa: E731
    bgr = bgr_from_yuv(Y, up(U), up(V))
    if size is not None and tuple(size) != bgr.shape[:2]:
        bgr = O.resize_bilinear_u8(bgr, size[0], size[1])
    return bgr


def random_frames(rng, B, h, w):
    return rng.integers(0, 256, (B, h * 3 // 2, w), dtype=np.uint8)


def extreme_frames(rng, B, h, w):
    """Luma from {0, 15, 16, 235, 255} (the clamp below 16, the nominal range ends, overshoot), chroma bytes from {0, 255}."""
    f = np.empty((B, h * 3 // 2, w), np.uint8)
    f[:, :h] = rng.choice(np.array([0, 15, 16, 235, 255], np.uint8), (B, h, w))
    f[:, h:] = rng.choice(np.array([0, 255], np.uint8), (B, h // 2, w))
    return f


KNOWN = [((16, 128, 128), (0, 0, 0)), ((126, 128, 128), (128, 128, 128)), ((235, 128, 128), (255, 255, 255)),
         ((0, 128, 128), (0, 0, 0)), ((81, 90, 240), (0, 0, 254)), ((145, 54, 34), (1, 255, 0)),
         ((41, 240, 110), (255, 0, 0)), ((255, 255, 255), (255, 125, 255)), ((0, 0, 0), (0, 154, 0)),
         ((0, 255, 255), (255, 0, 203))]


def test_yuv_oracle_known_answers():
    for (y, u, v), bgr in KNOWN:
        assert tuple(bgr_from_yuv(y, u, v).tolist()) == bgr, ((y, u, v), bgr)
    # the four plane orders on hand-built frames: 2x2 (one chroma sample) and 2x4 (two, to tell interleaved from planar apart)
    Y = np.array([[16, 126], [235, 0]], np.uint8)
    u, v = 90, 240
    hand = {"nv12": [u, v], "nv21": [v, u], "i420": [u, v], "yv12": [v, u]}
    for fmt, chroma in hand.items():
        frame = np.concatenate([Y, np.array([chroma], np.uint8)])
        got = yuv_to_bgr_ref(frame, fmt)
        assert np.array_equal(got, bgr_from_yuv(Y, np.full((2, 2), u), np.full((2, 2), v))), fmt
    Y = np.arange(8, dtype=np.uint8).reshape(2, 4) * 30 + 10
    u0, u1, v0, v1 = 54, 240, 34, 110
    hand = {"nv12": [u0, v0, u1, v1], "nv21": [v0, u0, v1, u1], "i420": [u0, u1, v0, v1], "yv12": [v0, v1, u0, u1]}
    U = np.array([[u0, u0, u1, u1]] * 2)
    V = np.array([[v0, v0, v1, v1]] * 2)
    for fmt, chroma in hand.items():
        frame = np.concatenate([Y, np.array([chroma], np.uint8)])
        assert np.array_equal(yuv_to_bgr_ref(frame, fmt), bgr_from_yuv(Y, U, V)), fmt


def test_yuv_abi_declared_and_exported():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(CF_YUV_[A-Z0-9]+)\s+(\d+)", text)}
    assert consts == {"CF_YUV_NV12": 0, "CF_YUV_NV21": 1, "CF_YUV_I420": 2, "CF_YUV_YV12": 3}
    for k, v in consts.items():
        assert getattr(cfa._lib, k) == v
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"typedef struct cf_yuv_planes\s*\{\s*const void\* y;\s*const void\* c0;\s*const void\* c1;\s*\} cf_yuv_planes;", code)
    for sym in ("cf_forward_yuv", "cf_op_yuv_to_bgr"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), sym
        assert sym in cfa._lib.EXPORTS
        assert hasattr(cfa._lib.lib(), sym), sym
    assert [f for f, _ in cfa._lib.YuvPlanes._fields_] == ["y", "c0", "c1"]
    assert {cfa._lib.yuv_format(f) for f in FORMATS} == {0, 1, 2, 3} and cfa._lib.yuv_format("YUV420P") == 2
    with pytest.raises(ValueError):
        cfa._lib.yuv_format("yuyv")


# ------------------------------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_op_yuv_to_bgr_bit_exact(fmt):
    """The conversion kernels alone: identity (2 x 8 lanes at w % 8 == 0, 2 x 2 lanes otherwise) and convert + resize (4 and 2 output
    pixels per lane), up- and down-scaling, random frames and the extremes of the arithmetic."""
    rng = np.random.default_rng(FORMATS.index(fmt))
    cases = [((2, 2), None), ((6, 10), None), ((64, 96), None), ((480, 640), None),
             ((70, 98), (96, 128)), ((150, 224), (64, 96)), ((30, 42), (20, 50))]
    for (h, w), size in cases:
        frames = np.concatenate([random_frames(rng, 2, h, w), extreme_frames(rng, 1, h, w)])
        got = ops.yuv_to_bgr(frames, fmt, size=size)
        want = np.stack([yuv_to_bgr_ref(f, fmt, size) for f in frames])
        assert got.shape == want.shape and np.array_equal(got, want), (fmt, h, w, size)
    assert np.array_equal(ops.yuv_to_bgr(frames[0], fmt, size=size), want[0])            # one [h*3/2, w] frame
    for frames in (random_frames(rng, 1, 1080, 1920), extreme_frames(rng, 1, 1080, 1920)):
        got = ops.yuv_to_bgr(frames, fmt, size=(1088, 1920))
        assert np.array_equal(got[0], yuv_to_bgr_ref(frames[0], fmt, (1088, 1920))), fmt


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ("fp32", "fp32_split", "bf16"))
def test_engine_forward_yuv_equals_bgr_path(dtype):
    """forward_yuv_enqueue at the network size and at a resize size: the converted input equals the restatement (+ the oracle's resize),
    and heads and the top-100 decode are bit-identical to the same engine fed the restated BGR through its uint8 path."""
    rng = np.random.default_rng(3)
    eng = cfa.Engine(64, 96, max_batch=2, dtype=dtype, weights=cfa.weights.synthetic_state_dict(0))
    for fmt in FORMATS:
        for h, w in ((64, 96), (50, 70)):
            frames = random_frames(rng, 2, h, w)
            bgr = np.stack([yuv_to_bgr_ref(f, fmt) for f in frames])
            eng.forward_yuv_enqueue(frames, fmt)
            got_in = eng.resized_input()
            hy, dy = eng.heads(), eng.decode_topk(100)
            want_in = bgr if (h, w) == (64, 96) else np.stack([O.resize_bilinear_u8(b, 64, 96) for b in bgr])
            assert np.array_equal(got_in, want_in), (dtype, fmt, h, w)
            if (h, w) == (64, 96):
                eng.forward_enqueue(bgr)
            else:
                eng.forward_resized_enqueue(bgr)
            hb, db = eng.heads(), eng.decode_topk(100)
            for k in hb:
                assert np.array_equal(hy[k], hb[k]), (dtype, fmt, h, w, k)
            for a, b in zip(dy, db):
                assert np.array_equal(a, b), (dtype, fmt, h, w)
    eng.close()


@pytest.mark.gpu
def test_device_pitched_planes_and_host_frame_lists():
    """Device-resident frames with pitched rows (pitch = w rounded up to 256) and every plane in an allocation of its own, B = 3; host
    frames as a list of non-adjacent arrays (one 2-D copy per plane) and as page-locked arrays: the same heads as the dense host block."""
    rng = np.random.default_rng(5)
    h, w, B, P = 64, 96, 3, 256
    eng = cfa.Engine(h, w, max_batch=B, dtype="bf16")
    for fmt in FORMATS:
        il = fmt in ("nv12", "nv21")
        frames = random_frames(rng, B, h, w)
        eng.forward_yuv_enqueue(frames, fmt)
        want = eng.heads()
        allocs, ptrs = [], []

        def upload(plane):
            padded = np.zeros((plane.shape[0], P), np.uint8)
            padded[:, :plane.shape[1]] = plane
            d = eng.device_alloc(padded.nbytes)
            eng.memcpy_h2d(d, padded)
            allocs.append(d)
            return d
        cw = w if il else w // 2
        for f in frames:
            rest = f[h:].reshape(-1)
            c0 = rest[:(h // 2) * cw].reshape(h // 2, cw)
            c1 = None if il else rest[(h // 2) * cw:].reshape(h // 2, cw)
            ptrs.append((upload(f[:h]), upload(c0), None if il else upload(c1)))
        eng.forward_yuv_enqueue(ptrs, fmt, on_device=True, h=h, w=w, y_pitch=P, c_pitch=P)
        got = eng.heads()
        for k in want:
            assert np.array_equal(got[k], want[k]), (fmt, "device", k)
        pool = np.zeros((B, 2) + frames.shape[1:], np.uint8)           # frames with gaps between them: not one block
        pool[:, 0] = frames
        for lst in ([pool[b, 0] for b in range(B)], [cfa.pinned_copy(f) for f in frames]):
            eng.forward_yuv_enqueue(lst, fmt)
            got = eng.heads()
            for k in want:
                assert np.array_equal(got[k], want[k]), (fmt, "host list", k)
        for d in allocs:
            eng.device_free(d)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(480, 640), (720, 1280)])
def test_centerface_detect_yuv_equals_detect_batch(hw):
    """CenterFace.detect_yuv for every format = detect_batch on the restated BGR frames (identity size, and 720x1280 resized to
    736x1280), chunked by max_batch; detect_stream(fmt="nv12") yields the same results in order; frames of another size are refused."""
    rng = np.random.default_rng(hw[0])
    face = cfa.CenterFace(*hw, dtype="bf16", max_batch=2)
    frames = random_frames(rng, 3, *hw)
    for fmt in FORMATS:
        got = face.detect_yuv(frames, fmt)
        want = face.detect_batch([yuv_to_bgr_ref(f, fmt) for f in frames])
        assert len(got) == len(want) == 3
        for (d, l), (wd, wl) in zip(got, want):
            assert d.shape == wd.shape and np.array_equal(d, wd) and np.array_equal(l, wl), (hw, fmt)
        if fmt == "nv12":
            want_nv12 = want
    got = list(face.detect_stream(iter(list(frames) * 2), fmt="nv12"))
    assert len(got) == 6
    for (d, l), (wd, wl) in zip(got, want_nv12 * 2):
        assert np.array_equal(d, wd) and np.array_equal(l, wl)
    assert face.detect_yuv(list(frames[:1]), "nv12")[0][0].shape == want_nv12[0][0].shape
    with pytest.raises(ValueError):
        face.detect_yuv(random_frames(rng, 1, hw[0] + 2, hw[1]), "nv12")
    face.close()


@pytest.mark.gpu
def test_bad_arguments_raise_and_the_engine_keeps_working():
    rng = np.random.default_rng(9)
    h, w = 64, 96
    eng = cfa.Engine(h, w, max_batch=2, dtype="bf16")
    frames = random_frames(rng, 2, h, w)
    eng.forward_yuv_enqueue(frames, "i420")
    want = eng.heads()
    d = eng.device_alloc(h * w * 2)
    y, c0, c1 = d, d + h * w, d + h * w + (h // 2) * (w // 2)
    dev = dict(on_device=True, h=h, w=w)
    bad = [
        lambda: eng.forward_yuv_enqueue([(y, c0, c1)], "i420", on_device=True, h=63, w=w),         # odd h
        lambda: eng.forward_yuv_enqueue([(y, c0, c1)], "i420", on_device=True, h=h, w=94 + 1),     # odd w
        lambda: eng.forward_yuv_enqueue([(y, c0, c1)], "i420", on_device=True, h=0, w=w),          # too small
        lambda: eng.forward_yuv_enqueue([], "i420", **dev),                                           # B = 0
        lambda: eng.forward_yuv_enqueue([(y, c0, c1)] * 3, "i420", **dev),                            # B > max_batch
        lambda: eng.forward_yuv_enqueue([(y, c0, c1)], 7, **dev),                                     # unknown format
        lambda: eng.forward_yuv_enqueue([(y, c0, c1)], "yuyv", **dev),
        lambda: eng.forward_yuv_enqueue([(0, c0, c1)], "i420", **dev),                                # NULL planes
        lambda: eng.forward_yuv_enqueue([(y, c0, None)], "i420", **dev),
        lambda: eng.forward_yuv_enqueue([(y, None)], "nv12", **dev),
        lambda: eng.forward_yuv_enqueue([(y, c0, c1)], "i420", y_pitch=w - 16, **dev),                # pitch below the row
        lambda: eng.forward_yuv_enqueue([(y, c0, c1)], "i420", c_pitch=w // 2 - 4, **dev),
        lambda: eng.forward_yuv_enqueue([(y, c0)], "nv12", c_pitch=w - 4, **dev),
        lambda: eng.forward_yuv_enqueue([(y + 2, c0, c1)], "i420", **dev),                            # misaligned device planes
        lambda: eng.forward_yuv_enqueue([(y, c0, c1 + 1)], "i420", **dev),
        lambda: eng.forward_yuv_enqueue([(y, c0, c1)], "i420", y_pitch=w + 2, **dev),                 # misaligned device pitch
        lambda: eng.forward_yuv_enqueue(np.zeros((2, 95, w), np.uint8), "nv12"),                      # not a 4:2:0 frame
        lambda: eng.forward_yuv_enqueue(frames.astype(np.int16), "nv12"),
        lambda: eng.forward_yuv_enqueue(frames, "nv12", y_pitch=w + 4),                               # host frames are dense
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    L = cfa._lib.lib()
    descs = (cfa._lib.YuvPlanes * 1)()
    descs[0].y, descs[0].c0, descs[0].c1 = y, c0, c1
    assert L.cf_forward_yuv(eng._h, 2, descs, 1, 1, h, w - 1, w, w // 2) == -1
    assert b"even" in L.cf_last_error(eng._h)
    assert L.cf_forward_yuv(eng._h, 2, None, 1, 1, h, w, w, w // 2) == -1
    assert L.cf_op_yuv_to_bgr(0, 2, None, None, 1, h, w, h, w) == -1
    with pytest.raises(ValueError):
        ops.yuv_to_bgr(frames, "i420", size=(h, w - 1))
    eng.forward_yuv_enqueue(frames, "i420")                                                          # still correct afterwards
    got = eng.heads()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    eng.device_free(d)
    eng.close()


@pytest.mark.gpu
@pytest.mark.isolated
def test_host_nv12_batches_back_to_back_on_the_copy_stream():
    """Two host-fed NV12 batches over 8 MB each (the copy-stream path: the second batch's copy may only wait for the conversion of the
    first to have read the staging buffer), a BGR forward between them, one engine, no synchronisation until the end -- twice (eager,
    then replayed graphs): every device-output decode equals its synchronous run."""
    rng = np.random.default_rng(11)
    S, B, K = 640, 16, 100
    eng = cfa.Engine(S, S, max_batch=B, dtype="bf16")
    a, c = cfa.pinned_empty((B, S * 3 // 2, S)), cfa.pinned_empty((B, S * 3 // 2, S))
    bgr = cfa.pinned_empty((B, S, S, 3))
    for arr in (a, c, bgr):
        arr[...] = rng.integers(0, 256, arr.shape, dtype=np.uint8)
    assert a.nbytes > (8 << 20)
    steps = [lambda: eng.forward_yuv_enqueue(a, "nv12"), lambda: eng.forward_enqueue(bgr), lambda: eng.forward_yuv_enqueue(c, "nv12")]
    want = []
    for step in steps:
        step()
        want.append(eng.decode_topk(K))
    outs = [(eng.device_alloc(B * K * 24), eng.device_alloc(B * K * 40), eng.device_alloc(B * K * 8)) for _ in steps]
    for _ in range(2):
        for step, o in zip(steps, outs):
            step()
            eng.decode_topk_device(K, *o)
        eng.synchronize()
        for o, (wd, wl, wi) in zip(outs, want):
            dets, lms, inds = np.empty((B, K, 6), np.float32), np.empty((B, K, 10), np.float32), np.empty((B, K), np.int64)
            eng.memcpy_d2h(dets, o[0])
            eng.memcpy_d2h(lms, o[1])
            eng.memcpy_d2h(inds, o[2])
            assert np.array_equal(dets, wd) and np.array_equal(lms, wl) and np.array_equal(inds, wi)
    for o in outs:
        for p in o:
            eng.device_free(p)
    eng.close()
