"""cf_redact_faces / cf_op_redact without a GPU: the symbols are exported, declared in the header and bound in _lib.py, the structs agree
with the header, and every CF_EINVAL of the contract comes back before any device is touched, with the frame buffer unchanged."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = cfa._lib


def _header():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_redact_symbols_constants_and_structs_match_the_header():
    text, code = _header()
    lib = L.lib()
    for sym in ("cf_redact_faces", "cf_op_redact"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), sym
        assert sym in L.EXPORTS and hasattr(lib, sym)
        assert getattr(lib, sym).argtypes is not None, sym
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(CF_FRAME_[A-Z0-9_]+|CF_REDACT_[A-Z0-9_]+|CF_YUV_[A-Z0-9_]+)\s+(\d+)", text)}
    assert consts == {"CF_YUV_NV12": 0, "CF_YUV_NV21": 1, "CF_YUV_I420": 2, "CF_YUV_YV12": 3, "CF_FRAME_BGR": 4,
                      "CF_REDACT_SOLID": 0, "CF_REDACT_MOSAIC": 1, "CF_REDACT_RECT": 0, "CF_REDACT_ELLIPSE": 1}
    for k, v in consts.items():
        assert getattr(L, k) == v
    for name, cls in (("cf_redact_opts", L.RedactOpts), ("cf_planes_rw", L.PlanesRW)):
        fields = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), code, flags=re.S).group(1)
        names = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*;", fields)
        assert [f for f, _ in cls._fields_] == names, (name, names)
    assert C.sizeof(L.RedactOpts) == 20 and C.sizeof(L.PlanesRW) == 3 * C.sizeof(C.c_void_p)
    assert len(L.redact_opts().fill) == 4
    # the arithmetic is stated in the header and in the kernel file, and the kernel file is built without FMA contraction
    src = open(os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc", "cf_redact.hip")).read()
    for words in ("floor((cx - hw) * fx)", "(du*Bv)^2 + (dv*A)^2 <= (A*Bv)^2", "(sum + n/2) / n"):
        assert words in text and words in src, words
    mk = open(os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc", "Makefile")).read()
    assert "cf_redact.hip" in mk and re.search(r"EXTRA_cf_redact\s*=\s*-ffp-contract=off", mk)


def _call(fmt=L.CF_FRAME_BGR, opts=None, B=1, h=8, w=12, pitch0=None, pitch1=None, planes="auto", boxes="auto", counts="auto", H=8, W=12,
          null_opts=False):
    """One cf_op_redact call on a fresh noise frame: (return code, frame unchanged?)."""
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
    o = opts if opts is not None else L.redact_opts()
    r = L.lib().cf_op_redact(0, None if null_opts else C.byref(o), fmt, None if planes is None else tab, B, h, w, pitch0, pitch1,
                             L.ptr(bx), L.ptr(cn), H, W)
    return r, np.array_equal(buf, keep)


def test_op_redact_refuses_bad_arguments_before_any_device_work():
    bad = [
        dict(fmt=-1), dict(fmt=5), dict(fmt=99),
        dict(opts=L.redact_opts(mode=2)), dict(opts=L.redact_opts(mode=-1)), dict(opts=L.redact_opts(shape=2)), dict(opts=L.redact_opts(shape=-1)),
        dict(opts=L.redact_opts(cell=7)), dict(opts=L.redact_opts(cell=0)), dict(opts=L.redact_opts(cell=258)), dict(opts=L.redact_opts(cell=-4)),
        dict(opts=L.redact_opts(scale=0.2)), dict(opts=L.redact_opts(scale=4.5)), dict(opts=L.redact_opts(scale=float("nan"))),
        dict(opts=L.redact_opts(scale=float("inf"))), dict(opts=L.redact_opts(scale=-1.3)),
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
        assert b"cf_op_redact" in L.lib().cf_op_last_error(), kw
    # an odd BGR frame and an odd cell under SOLID are fine arguments: they get as far as the device (none here: CF_EHIP) or succeed
    for kw in (dict(h=7, w=11), dict(opts=L.redact_opts(mode="solid", cell=7))):
        assert _call(**kw)[0] != -1, kw
    # the context form: nothing without a context; a NULL context cannot hold an error text
    o = L.redact_opts()
    tab = (L.PlanesRW * 1)()
    assert L.lib().cf_redact_faces(None, C.byref(o), L.CF_FRAME_BGR, tab, 0, 1, 8, 12, 36, 0) == -1


def test_python_wrappers_refuse_what_they_can_see():
    with pytest.raises(ValueError):
        L.redact_opts(mode="blur")
    with pytest.raises(ValueError):
        L.redact_opts(shape="circle")
    with pytest.raises(ValueError):
        L.redact_opts(fill=(0, 0))
    with pytest.raises(ValueError):
        L.redact_opts(fill=(0, 0, 256))
    with pytest.raises(ValueError):
        L.frame_format("rgb")
    assert L.frame_format("bgr") == 4 and L.frame_format("NV12") == 0 and L.frame_format("yuv420p") == 2
    img = np.zeros((1, 8, 12, 3), np.uint8)
    box = np.float32([[2, 2, 8, 6]])
    with pytest.raises(ValueError):
        ops.redact_faces(img, box, [2], (8, 12))                       # counts do not sum to the rows
    with pytest.raises(ValueError):
        ops.redact_faces(img[:, :, ::2], box, [1], (8, 12))            # not contiguous: cannot be written in place
    with pytest.raises(ValueError):
        ops.redact_faces(np.zeros((1, 10, 12), np.uint8), box, [1], (8, 12), fmt="nv12")    # 10 rows is no h*3/2
    with pytest.raises(ValueError):
        ops.redact_faces([(np.zeros((8, 12), np.uint8),)], box, [1], (8, 12), fmt="nv12")   # a plane is missing
    ro = np.zeros((1, 8, 12, 3), np.uint8)
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        ops.redact_faces(ro, box, [1], (8, 12))
    for kw in (dict(cell=7), dict(scale=0.1), dict(mode=3), dict(shape=5)):                 # the library's own refusals are ValueErrors too
        with pytest.raises(cfa._lib.CenterFaceValueError):
            ops.redact_faces(img, box, [1], (8, 12), **kw)
        assert not img.any()
    # plane tuples with pitches: geometry is read from the arrays
    y = np.zeros((8, 16), np.uint8)[:, :12]
    c = np.zeros((4, 16), np.uint8)[:, :12]
    tab, B, h, w, p0, p1, _ = L.frame_planes([(y, c)], "nv12")
    assert (B, h, w, p0, p1) == (1, 8, 12, 16, 16) and tab[0].p0 == y.ctypes.data and tab[0].p1 == c.ctypes.data and not tab[0].p2
    fl = [np.zeros((12, 12), np.uint8), np.zeros((12, 12), np.uint8)]                       # a list of dense frames
    tab, B, h, w, p0, p1, _ = L.frame_planes(fl, "yv12")
    assert (B, h, w, p0, p1) == (2, 8, 12, 12, 6) and tab[1].p0 == fl[1].ctypes.data and tab[1].p1 - tab[1].p0 == 96 and tab[1].p2 - tab[1].p1 == 24
    tab, B, h, w, p0, p1, _ = L.frame_planes(np.zeros((2, 12, 12), np.uint8), "i420")
    assert (B, h, w, p0, p1) == (2, 8, 12, 12, 6) and tab[1].p2 - tab[1].p0 == 96 + 24
