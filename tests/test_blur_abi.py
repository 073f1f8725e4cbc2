"""cf_blur_faces / cf_op_blur without a GPU: the symbols are exported, declared in the header and bound in _lib.py, the options struct
agrees with the header (and cf_redact_opts is untouched), and every CF_EINVAL of the contract comes back before any device is touched,
with the frame buffer unchanged."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = cfa._lib
CSRC = os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc")


def test_blur_symbols_and_structs_match_the_header():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    for sym in ("cf_blur_faces", "cf_op_blur"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), sym
        assert sym in L.EXPORTS and hasattr(lib, sym)
        assert getattr(lib, sym).argtypes is not None, sym
    fields = re.search(r"typedef struct cf_blur_opts\s*\{(.*?)\}\s*cf_blur_opts;", code, flags=re.S).group(1)
    assert [f for f, _ in L.BlurOpts._fields_] == re.findall(r"(\w+)\s*;", fields) == ["shape", "radius", "scale"]
    assert C.sizeof(L.BlurOpts) == 12
    assert C.sizeof(L.RedactOpts) == 20 and sorted(L.REDACT_MODES) == ["mosaic", "solid"]       # the redaction's struct and modes stay
    o = L.blur_opts("rect", 7, 2.0)
    assert (o.shape, o.radius, o.scale) == (L.CF_REDACT_RECT, 7, 2.0)
    d = L.blur_opts()
    assert (d.shape, d.radius) == (L.CF_REDACT_ELLIPSE, 0) and abs(d.scale - 1.3) < 1e-6
    # the arithmetic is stated in the header and in the kernel file; the kernel file is built without FMA contraction and shares the
    # box mapping with cf_redact.hip through one header
    src = open(os.path.join(CSRC, "cf_blur.hip")).read()
    for words in ("box_b * box_b * box_b", "value = (S + D/2) / D", "clamp(min(A, Bv) / 8, 1, 24)", "1 3 6 7 6 3 1"):
        assert words in text and words in src, words
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "cf_blur.hip" in mk and re.search(r"EXTRA_cf_blur\s*=\s*-ffp-contract=off", mk)
    shared = open(os.path.join(CSRC, "cf_redactmath.h")).read()
    assert "face_box(" in shared and "floor((cx - hw) * fx)" in shared
    for name in ("cf_redact.hip", "cf_blur.hip"):
        body = open(os.path.join(CSRC, name)).read()
        assert '#include "cf_redactmath.h"' in body and "FaceBox face_box(" not in body, name


def _call(fmt=L.CF_FRAME_BGR, opts=None, B=1, h=8, w=12, pitch0=None, pitch1=None, planes="auto", boxes="auto", counts="auto", H=8, W=12,
          null_opts=False):
    """One cf_op_blur call on a fresh noise frame: (return code, frame unchanged?)."""
    bgr, il = fmt == L.CF_FRAME_BGR, fmt in (L.CF_YUV_NV12, L.CF_YUV_NV21)
    buf = np.random.default_rng(1).integers(0, 256, 8192 * 3 + 64, dtype=np.uint8)         # room for every row size tried below
    keep = buf.copy()
    tab = (L.PlanesRW * 1)()
    if planes == "auto":
        tab[0].p0, tab[0].p1, tab[0].p2 = buf.ctypes.data, buf.ctypes.data + 4096, buf.ctypes.data + 8192
    elif planes is not None:
        tab[0].p0, tab[0].p1, tab[0].p2 = [(buf.ctypes.data + 4096 * k) if on else None for k, on in enumerate(planes)]
    pitch0 = (3 * w if bgr else w) if pitch0 is None else pitch0
    pitch1 = (0 if bgr else w if il else w // 2) if pitch1 is None else pitch1
    bx = np.float32([[2, 2, 8, 6]]) if isinstance(boxes, str) else boxes
    cn = np.array([1], np.int32) if isinstance(counts, str) else counts
    o = opts if opts is not None else L.blur_opts()
    r = L.lib().cf_op_blur(0, None if null_opts else C.byref(o), fmt, None if planes is None else tab, B, h, w, pitch0, pitch1,
                           L.ptr(bx), L.ptr(cn), H, W)
    return r, np.array_equal(buf, keep)


def test_op_blur_refuses_bad_arguments_before_any_device_work():
    bad = [
        dict(fmt=-1), dict(fmt=5), dict(fmt=99),
        dict(opts=L.blur_opts(radius=-1)), dict(opts=L.blur_opts(radius=25)), dict(opts=L.blur_opts(radius=1 << 20)),
        dict(opts=L.blur_opts(shape=2)), dict(opts=L.blur_opts(shape=-1)),
        dict(opts=L.blur_opts(scale=0.2)), dict(opts=L.blur_opts(scale=4.5)), dict(opts=L.blur_opts(scale=float("nan"))),
        dict(opts=L.blur_opts(scale=float("inf"))), dict(opts=L.blur_opts(scale=-1.3)),
        # the geometry list of tests/test_redact_abi.py
        dict(fmt=L.CF_YUV_NV12, h=7), dict(fmt=L.CF_YUV_I420, w=11), dict(fmt=L.CF_YUV_YV12, h=7, w=11),
        dict(h=0), dict(w=0), dict(h=8193), dict(w=8193), dict(h=-8),
        dict(pitch0=35), dict(fmt=L.CF_YUV_NV12, pitch0=11), dict(fmt=L.CF_YUV_NV21, pitch1=11), dict(fmt=L.CF_YUV_I420, pitch1=5),
        dict(planes=None), dict(planes=(False, True, True)), dict(fmt=L.CF_YUV_NV12, planes=(True, False, True)),
        dict(fmt=L.CF_YUV_I420, planes=(True, True, False)), dict(fmt=L.CF_YUV_YV12, planes=(True, False, True)),
        dict(B=0), dict(null_opts=True), dict(counts=None), dict(boxes=None), dict(counts=np.array([-1], np.int32)), dict(H=0), dict(W=0),
    ]
    for kw in bad:
        r, same = _call(**kw)
        assert r == -1 and same, kw
        assert b"cf_op_blur" in L.lib().cf_op_last_error(), kw
    # every radius of the range, both ends of the scale and an odd BGR frame are fine arguments: they get as far as the device (none
    # here: CF_EHIP) or succeed
    for kw in (dict(h=7, w=11), dict(opts=L.blur_opts(radius=0)), dict(opts=L.blur_opts(radius=1)), dict(opts=L.blur_opts(radius=24)),
               dict(opts=L.blur_opts(scale=0.25)), dict(opts=L.blur_opts(scale=4.0))):
        assert _call(**kw)[0] != -1, kw
    # the context form: nothing without a context; a NULL context cannot hold an error text
    o = L.blur_opts()
    tab = (L.PlanesRW * 1)()
    assert L.lib().cf_blur_faces(None, C.byref(o), L.CF_FRAME_BGR, tab, 0, 1, 8, 12, 36, 0) == -1
    # blur is no third mode of the redaction
    frame = np.zeros(8 * 36, np.uint8)
    tab[0].p0 = frame.ctypes.data
    for mode in (2, 3):
        ro = L.redact_opts(mode=mode)
        assert L.lib().cf_op_redact(0, C.byref(ro), L.CF_FRAME_BGR, tab, 1, 8, 12, 36, 0, L.ptr(np.float32([[2, 2, 8, 6]])),
                                    L.ptr(np.array([1], np.int32)), 8, 12) == -1


def test_python_wrappers_refuse_what_they_can_see():
    with pytest.raises(ValueError):
        L.blur_opts(shape="circle")
    with pytest.raises(ValueError):
        L.redact_opts(mode="blur")                                     # still no mode of cf_redact_opts
    img = np.zeros((1, 8, 12, 3), np.uint8)
    box = np.float32([[2, 2, 8, 6]])
    with pytest.raises(ValueError):
        ops.blur_faces(img, box, [2], (8, 12))                         # counts do not sum to the rows
    with pytest.raises(ValueError):
        ops.blur_faces(img[:, :, ::2], box, [1], (8, 12))              # not contiguous: cannot be written in place
    with pytest.raises(ValueError):
        ops.blur_faces([(np.zeros((8, 12), np.uint8),)], box, [1], (8, 12), fmt="nv12")     # a plane is missing
    ro = np.zeros((1, 8, 12, 3), np.uint8)
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        ops.blur_faces(ro, box, [1], (8, 12))
    for kw in (dict(radius=25), dict(radius=-1), dict(scale=0.1), dict(shape=5)):           # the library's own refusals are ValueErrors too
        with pytest.raises(cfa._lib.CenterFaceValueError):
            ops.blur_faces(img, box, [1], (8, 12), **kw)
        assert not img.any()
    # mode='blur' is routed before RedactOpts is built, and takes none of the other modes' options
    assert L.split_redact_options(dict(mode="blur", radius=5, shape="rect")) == ("blur", dict(radius=5, shape="rect"))
    assert L.split_redact_options(dict(mode="Blur")) == ("blur", {})
    assert L.split_redact_options(dict(mode="mosaic", cell=6)) == ("redact", dict(mode="mosaic", cell=6))
    assert L.split_redact_options({}) == ("redact", {})
    for kw in (dict(mode="blur", cell=6), dict(mode="blur", fill=(1, 2, 3)), dict(mode="blur", radius=3, cell=20), dict(mode="mosaic", radius=3),
               dict(radius=3)):
        with pytest.raises(ValueError):
            L.split_redact_options(kw)


class _NoEngine(object):
    """Stands where CenterFace.engine is: any use of the device fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the engine was used (%s) before the options were refused" % name)


def test_centerface_refuses_blur_with_cell_or_fill_before_any_work():
    face = cfa.CenterFace.__new__(cfa.CenterFace)                      # no context: the refusal must come before any engine call
    face.engine = _NoEngine()
    imgs = [np.zeros((8, 12, 3), np.uint8)]
    yuv = np.zeros((1, 12, 12), np.uint8)
    for kw in (dict(cell=6), dict(fill=(1, 2, 3))):
        with pytest.raises(ValueError):
            face.anonymize(imgs, mode="blur", **kw)
        with pytest.raises(ValueError):
            face.anonymize(imgs, tiled=True, mode="blur", **kw)
        with pytest.raises(ValueError):
            face.anonymize_yuv(yuv, "nv12", mode="blur", **kw)
        with pytest.raises(ValueError):
            face.anonymize_yuv(yuv, "nv12", tiled=True, mode="blur", **kw)
        with pytest.raises(ValueError):
            face.detect_tiled(np.zeros((1, 8, 12, 3), np.uint8), redact=dict(mode="blur", **kw))
