"""Aligned chips cut from the source frame (cf_align_faces_frame, cf_op_align_frame, ops.align_frame): what can be checked without a
GPU -- the declarations, the refusals that come before any device work -- and the numpy restatement tests/test_align_frame.py compares
the kernel with.

The restatement adds nothing to tests/test_align.py's: a frame's chips are ``align_ref(bgr(frame), landmarks in frame pixels)`` with
``bgr`` the identity or tests/test_yuv_input.py's conversion.  Only the engine's non-tiled path needs more: its landmarks are the
decode's float32 network-coordinate values mapped to the frame in float64 and NOT rounded back, so the estimate takes float64 points
(``estimate64`` below, equal to ``estimate`` bit for bit on float32-representable points)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from test_align import align_ref, bits_equal, estimate, finish, hard_landmarks, pose_landmarks, template_points, warp
from test_yuv_input import yuv_to_bgr_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = cfa._lib
FORMATS = ("bgr", "nv12", "nv21", "i420", "yv12")


# ------------------------------------------------------------------------------------------ restatement
def estimate64(p64, q, S):
    """tests/test_align.py's ``estimate`` with ONE change: the ten landmark values arrive as float64 (no float32 round trip)."""
    f = np.float64
    with np.errstate(all="ignore"):
        p = np.asarray(p64, np.float64).reshape(5, 2)
        pm = ((((p[0] + p[1]) + p[2]) + p[3]) + p[4]) / 5.0
        qm = ((((q[0] + q[1]) + q[2]) + q[3]) + q[4]) / 5.0
        pc, qc = p - pm, q - qm
        den, na, nb = f(0.0), f(0.0), f(0.0)
        for i in range(5):
            den = den + (pc[i, 0] * pc[i, 0] + pc[i, 1] * pc[i, 1])
            na = na + (pc[i, 0] * qc[i, 0] + pc[i, 1] * qc[i, 1])
            nb = nb + (pc[i, 0] * qc[i, 1] - pc[i, 1] * qc[i, 0])
        a, b = na / den, nb / den
        tx = qm[0] - (a * pm[0] - b * pm[1])
        ty = qm[1] - (b * pm[0] + a * pm[1])
        D = a * a + b * b
        ia, ib = a / D, b / D
        M = np.array([ia, ib, -(ia * tx + ib * ty), -ib, ia, -((-ib) * tx + ia * ty)], np.float64)
        ok = bool(np.all(np.isfinite(p)) and den > 0.0 and D > 0.0 and np.all(np.isfinite(M)))
        if ok:
            ok = bool(max(abs(M[0]), abs(M[1]), abs(M[3]), abs(M[4])) * f(S) + max(abs(M[2]), abs(M[5])) < 1048576.0)
    return M if ok else np.zeros(6, np.float64)


def net_to_frame(lms_net, frame_hw, net_hw):
    """The decode's float32 network-coordinate landmark rows [n,10] -> float64 frame pixels: X = (double)x * ((double)w / (double)W),
    Y = (double)y * ((double)h / (double)H)."""
    (h, w), (H, W) = frame_hw, net_hw
    out = np.asarray(lms_net, np.float32).astype(np.float64).reshape(-1, 10)
    with np.errstate(all="ignore"):
        out[:, 0::2] = out[:, 0::2] * (np.float64(w) / np.float64(W))
        out[:, 1::2] = out[:, 1::2] * (np.float64(h) / np.float64(H))
    return out


def bgr_of(dense, fmt):
    """Dense frames ([B,h,w,3] BGR, or [B, h*3//2, w] 4:2:0) as BGR [B,h,w,3]."""
    return dense if fmt == "bgr" else np.stack([yuv_to_bgr_ref(f, fmt) for f in dense])


def frame_align_ref(bgr, pts64, counts, size=112, template=None, out="u8", rgb=False, mean=0.0, scale=1.0, max_per_image=0, stats=None):
    """cf_align_faces_frame restated on BGR frames [B,h,w,3] and float64 landmark rows in frame pixels, image after image: (chips,
    matrices) of the first ``max_per_image`` rows of every image (0 = all).  ``stats`` (a dict) collects how many chips had a zero
    matrix, hung over an edge, or missed the frame altogether."""
    q = template_points(size, template)
    chips, mats, n = [], [], 0
    for b, c in enumerate(counts):
        for i in range(int(c)):
            if max_per_image <= 0 or i < max_per_image:
                M = estimate64(pts64[n], q, size)
                chip, inside = warp(bgr[b], M, size, want_inside=True)
                if stats is not None:
                    stats["zero"] = stats.get("zero", 0) + (not M.any())
                    stats["partial"] = stats.get("partial", 0) + bool(M.any() and inside.sum() > 50 and (~inside).sum() > 50 and chip.any())
                    stats["outside"] = stats.get("outside", 0) + bool(M.any() and not chip.any())
                chips.append(finish(chip, out, rgb, mean, scale))
                mats.append(M)
            n += 1
    shape = (0, 3, size, size) if out == "f32" else (0, size, size, 3)
    return (np.stack(chips) if chips else np.zeros(shape, np.float32 if out == "f32" else np.uint8),
            np.stack(mats) if mats else np.zeros((0, 6)))


def pitched_planes(dense, fmt, pitch0, pitch1, pad):
    """Per frame a tuple of row views [rows, row bytes] on buffers of EXACTLY rows x pitch bytes whose padding holds ``pad``; ``dense``:
    [B,h,w,3] BGR or [B, h*3//2, w] 4:2:0.  Returns (views, buffers)."""
    if fmt == "bgr":
        h, w = dense.shape[1:3]
        geo = [(0, h, 3 * w, pitch0)]
    else:
        h, w = dense.shape[1] * 2 // 3, dense.shape[2]
        offs, cp = L.yuv_dense_geometry(L.yuv_format(fmt), h, w)
        geo = [(0, h, w, pitch0)] + [(o, h // 2, cp, pitch1) for o in offs[1:] if o is not None]
    views, bufs = [], []
    for b in range(dense.shape[0]):
        flat, v = dense[b].reshape(-1), []
        for o, r, c, p in geo:
            buf = np.full((r, p), pad, np.uint8)
            buf[:, :c] = flat[o:o + r * c].reshape(r, c)
            bufs.append(buf)
            v.append(buf[:, :c])
        views.append(tuple(v))
    return views, bufs


# ------------------------------------------------------------------------------------------ CPU: the restatement
def test_estimate64_equals_estimate_on_float32_points():
    rng = np.random.default_rng(0)
    rows = np.concatenate([pose_landmarks(rng, 40, 480, 640, 112, margin=-0.2), hard_landmarks(rng, 480, 640, 112)])
    zero = 0
    for S, tmpl in ((112, None), (16, None), (512, np.float32([[150, 180], [360, 183], [256, 280], [180, 380], [338, 384]]))):
        q = template_points(S, tmpl)
        for r in rows:
            a, b = estimate(r, q, S), estimate64(r.astype(np.float64), q, S)
            assert bits_equal(a, b), (r, a, b)
            zero += not a.any()
    assert zero >= 18                                        # the degenerate rows were among them


def test_frame_restatement_is_align_ref_of_the_converted_frame():
    """For float32 landmarks in frame pixels the frame restatement IS ``align_ref(bgr(frame), lms)``, in every format; and for
    (h, w) == (H, W) the network -> frame map is the identity on float32 values (so cf_align_faces_frame must equal cf_align_faces)."""
    rng = np.random.default_rng(1)
    h, w, S = 48, 64, 32
    counts = np.array([3, 0, 14], np.int32)
    lms = pose_landmarks(rng, 17, h, w, S, margin=-0.2)
    lms[5:17] = hard_landmarks(rng, h, w, S)
    for fmt in FORMATS:
        dense = rng.integers(0, 256, (3, h, w, 3) if fmt == "bgr" else (3, h * 3 // 2, w), dtype=np.uint8)
        bgr = bgr_of(dense, fmt)
        assert bgr.shape == (3, h, w, 3) and bgr.dtype == np.uint8
        for opt in (dict(out="u8"), dict(out="f32", rgb=True, mean=127.5, scale=1 / 128.0)):
            wc, wm = align_ref(bgr, lms, counts, S, None, **opt)
            gc, gm = frame_align_ref(bgr, lms.astype(np.float64), counts, S, None, **opt)
            assert bits_equal(gc, wc) and bits_equal(gm, wm)
        one_c, one_m = frame_align_ref(bgr, lms.astype(np.float64), counts, S, max_per_image=1)
        all_c, all_m = align_ref(bgr, lms, counts, S)
        assert bits_equal(one_c, all_c[[0, 3]]) and bits_equal(one_m, all_m[[0, 3]])      # the first row of images 0 and 2
    ident = net_to_frame(lms, (96, 128), (96, 128))
    assert bits_equal(ident, lms.astype(np.float64))
    aniso = net_to_frame(lms[:5], (150, 202), (96, 128))
    assert np.array_equal(aniso[:, 0::2], lms[:5, 0::2].astype(np.float64) * (202.0 / 128.0))
    assert np.array_equal(aniso[:, 1::2], lms[:5, 1::2].astype(np.float64) * (150.0 / 96.0))
    assert not np.array_equal(aniso.astype(np.float32).astype(np.float64), aniso)        # the mapped values are not float32 values


def test_pitched_planes_hold_exactly_rows_times_pitch():
    rng = np.random.default_rng(2)
    dense = rng.integers(0, 256, (2, 6 * 3 // 2, 10), dtype=np.uint8)
    for fmt, p1, n in (("nv12", 12, 2), ("i420", 8, 3)):
        views, bufs = pitched_planes(dense, fmt, 12, p1, 0xFF)
        assert len(bufs) == 2 * n and bufs[0].shape == (6, 12) and bufs[1].shape == (3, p1)
        assert (bufs[0][:, 10:] == 0xFF).all() and np.array_equal(views[1][0], dense[1, :6])
        tab, B, h, w, pitch0, pitch1, _ = L.frame_planes(views, fmt, writable=False)
        assert (B, h, w, pitch0, pitch1) == (2, 6, 10, 12, p1)


# ------------------------------------------------------------------------------------------ CPU: the ABI
def _opts(**kw):
    return L.align_opts(**kw)[0]


def test_align_frame_symbols_are_declared_exported_and_built():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    for sym in ("cf_align_faces_frame", "cf_op_align_frame"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), sym
        assert sym in L.EXPORTS and hasattr(lib, sym)
        assert getattr(lib, sym).argtypes is not None, sym
    assert callable(ops.align_frame) and callable(cfa.Engine.align_faces_frame) and callable(cfa.Engine.align_faces_frame_device)
    assert callable(cfa.CenterFace.detect_aligned_frames)
    # the new kernel shares the one statement of the estimate and of the conversion, and is built without FMA contraction
    csrc = os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc")
    new, old = open(os.path.join(csrc, "cf_align_frame.hip")).read(), open(os.path.join(csrc, "cf_align.hip")).read()
    for src in (new, old):
        assert '#include "cf_alignmath.h"' in src and "estimate_inverse(" in src and "Similarity estimate_inverse" not in src
    assert '#include "cf_yuvmath.h"' in new and "yuv_px(" in new
    assert "Similarity estimate_inverse" in open(os.path.join(csrc, "cf_alignmath.h")).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "cf_align_frame.hip" in mk and re.search(r"EXTRA_cf_align_frame\s*=\s*-ffp-contract=off", mk)
    assert re.search(r"EXTRA_cf_align\s*=\s*-ffp-contract=off", mk)


def test_align_frame_refuses_bad_arguments_before_any_device_work():
    lib, P = L.lib(), L.ptr
    buf = np.zeros(64 * 64 * 3, np.uint8)
    lms = np.zeros((1, 10), np.float32)
    chips = np.zeros((1, 512, 512, 3), np.float32)
    offs = np.zeros(4, np.int32)
    a = buf.ctypes.data
    NV12, NV21, I420, YV12, BGR = L.CF_YUV_NV12, L.CF_YUV_NV21, L.CF_YUV_I420, L.CF_YUV_YV12, L.CF_FRAME_BGR

    def table(planes, B=1):
        tab = (L.YuvPlanes * B)()
        for b in range(B):
            tab[b].y, tab[b].c0, tab[b].c1 = planes
        return tab

    def op(fmt=BGR, planes=(a, a, a), B=1, h=32, w=32, p0=96, p1=32, lm=lms, c=(1,), o="default", out=chips):
        o = _opts() if o == "default" else o
        c = np.array(c, np.int32) if c is not None else None
        return lib.cf_op_align_frame(0, fmt, table(planes, max(B, 1)) if planes is not None else None, B, h, w, p0, p1, P(lm), P(c),
                                     C.byref(o) if o is not None else None, P(out), None)

    def eng(fmt=BGR, planes=(a, a, a), B=1, h=32, w=32, p0=96, p1=32, o="default", out=chips, of=offs, cap=1, dev_in=0, dev_out=0):
        o = _opts() if o == "default" else o
        return lib.cf_align_faces_frame(None, C.byref(o) if o is not None else None, fmt, table(planes, max(B, 1)) if planes is not None else None,
                                        dev_in, B, h, w, p0, p1, P(out), None, P(of), cap, dev_out)

    cases = [
        (dict(fmt=-1), b"format"), (dict(fmt=5), b"format"), (dict(fmt=99), b"format"),
        (dict(fmt=NV12, h=31), b"even"), (dict(fmt=I420, w=31, p0=32), b"even"), (dict(fmt=YV12, h=33, w=33, p0=36), b"even"),
        (dict(h=0), b"[2, 8192]"), (dict(w=0), b"[2, 8192]"), (dict(h=8194), b"[2, 8192]"), (dict(w=8194, p0=3 * 8194), b"[2, 8192]"),
        (dict(fmt=NV12, h=8194, p0=32), b"[2, 8192]"), (dict(h=1), b"[2, 8192]"), (dict(w=1), b"[2, 8192]"),
        (dict(p0=95), b"pitch0"), (dict(fmt=NV12, p0=31), b"pitch0"), (dict(fmt=NV21, p0=32, p1=31), b"pitch1"),
        (dict(fmt=I420, p0=32, p1=15), b"pitch1"), (dict(fmt=YV12, p0=32, p1=0), b"pitch1"),
        (dict(planes=(None, a, a)), b"null plane"), (dict(fmt=NV12, p0=32, planes=(a, None, None)), b"null plane"),
        (dict(fmt=I420, p0=32, p1=16, planes=(a, a, None)), b"null plane"), (dict(planes=None), b"null frame table"),
        (dict(B=0), b"B must"), (dict(B=-3), b"B must"),
        (dict(o=_opts(size=0)), b"size"), (dict(o=_opts(size=12)), b"size"), (dict(o=_opts(size=15)), b"size"), (dict(o=_opts(size=18)), b"size"),
        (dict(o=_opts(size=113)), b"size"), (dict(o=_opts(size=516)), b"size"), (dict(o=_opts(size=1024)), b"size"), (dict(o=_opts(size=-112)), b"size"),
        (dict(o=_opts(out=-1)), b"chip format"), (dict(o=_opts(out=2)), b"chip format"), (dict(o=_opts(out=7)), b"chip format"),
        (dict(o=_opts(max_per_image=-1)), b"max_per_image"), (dict(o=None), b"null"), (dict(out=None), b"null"),
    ]
    for kw, word in cases:
        for name, fn in (("cf_op_align_frame", op), ("cf_align_faces_frame", eng)):
            assert fn(**kw) == -1, (name, kw)
            msg = lib.cf_op_last_error()
            assert msg.startswith(name.encode()) and word in msg, (name, kw, msg)
    # the op alone: counts and landmarks, and pitches the device cannot read as dwords
    for kw, word in ((dict(c=(-1,)), b"negative count"), (dict(c=None), b"null"), (dict(lm=None), b"null landmarks"),
                     (dict(p0=98), b"multiples of 4"), (dict(fmt=NV12, p0=32, p1=34), b"multiples of 4")):
        assert op(**kw) == -1, kw
        assert word in lib.cf_op_last_error(), (kw, lib.cf_op_last_error())
    assert op(c=(0,), lm=None) == 0                          # no faces: nothing to do, no device touched
    # the engine entry alone: offsets, cap_faces, device alignment rules -- and, everything else being right, the missing context
    for kw, word in ((dict(of=None), b"null"), (dict(cap=-1), b"cap_faces"), (dict(dev_in=1, planes=(a + 2, a, a)), b"4-byte aligned"),
                     (dict(dev_in=1, p0=98), b"multiples of 4"), (dict(dev_in=1, fmt=NV12, p0=32, p1=34), b"multiples of 4"),
                     (dict(dev_out=1, out=chips.reshape(-1)[2:]), b"16-byte aligned"), (dict(), b"null context")):
        assert eng(**kw) == -1, kw
        assert word in lib.cf_op_last_error(), (kw, lib.cf_op_last_error())
    # odd sides are fine for BGR (the missing context is all that is wrong)
    assert eng(h=31, w=31, p0=93) == -1 and b"null context" in lib.cf_op_last_error()


def test_python_wrappers_refuse_wrong_shapes():
    img = np.zeros((2, 32, 32, 3), np.uint8)
    lms = np.zeros((2, 10), np.float32)
    ok = np.array([1, 1], np.int32)
    for frames, lm, cnt, fmt in ((img, lms, [1, 2], "bgr"), (img, lms, [2], "bgr"), (img, lms, [3, -1], "bgr"), (img, np.zeros((2, 8), np.float32), ok, "bgr"),
                                 (img, np.zeros(20, np.float32), ok, "bgr"), (img[..., :2], lms, ok, "bgr"), (img[0], lms, ok, "bgr"), (img, lms, ok, "nv12"),
                                 (np.zeros((2, 47, 32), np.uint8), lms, ok, "nv12"), (np.zeros((2, 48, 32), np.float32), lms, ok, "i420"),
                                 ([(np.zeros((32, 32), np.uint8),)] * 2, lms, ok, "nv12"), (img, lms, ok, "rgb")):
        with pytest.raises(ValueError):
            ops.align_frame(frames, lm, cnt, fmt)
    with pytest.raises(ValueError):
        ops.align_frame(img, lms, ok, size=102)              # the library's refusal, as a ValueError
    with pytest.raises(ValueError):
        ops.align_frame(img, lms, ok, out="yuv")
    with pytest.raises(ValueError):
        ops.align_frame(img, lms, ok, template=np.zeros((4, 2)))
    # a pitch that is no multiple of 4 is repacked on the host, not refused
    tab, B, h, w, p0, p1, _ = L.frame_planes(np.zeros((1, 5, 7, 3), np.uint8), "bgr", writable=False)
    t2, q0, q1, keep = L.frames_pitch4(tab, "bgr", B, h, w, p0, p1)
    assert (p0, q0, q1) == (21, 24, 0) and keep[0].shape == (5, 24)
    dense = np.arange(2 * 9 * 6, dtype=np.uint8).reshape(2, 9, 6)
    tab, B, h, w, p0, p1, _ = L.frame_planes(dense, "i420", writable=False)
    t2, q0, q1, keep = L.frames_pitch4(tab, "i420", B, h, w, p0, p1)
    assert (h, w, p0, p1, q0, q1) == (6, 6, 6, 3, 8, 4) and len(keep) == 6
    assert np.array_equal(keep[3][:, :6], dense[1, :6]) and np.array_equal(keep[4][:, :3], dense[1, 6:].reshape(-1)[:9].reshape(3, 3))
    assert np.array_equal(keep[5][:, :3], dense[1, 6:].reshape(-1)[9:].reshape(3, 3)) and not keep[3][:, 6:].any()
