"""Aligned face chips on the device (cf_align_faces, cf_op_align_faces, ops.align_faces, Engine.align_faces[_device],
CenterFace.detect_aligned): the similarity warp of the network-sized frame onto a chip template from the detector's five landmarks.

The contract: kernel == the numpy restatement below, BIT FOR BIT, in chips and in the float64 matrices.  The arithmetic is this
project's own statement (float64 estimate in a fixed operation order, fixed-point warp with 1/32-pixel positions and weights out of
1024); it has the same optimum as SimilarityTransform.estimate + cv2.warpAffine but is not claimed bit-identical to cv2.warpAffine
(whose weight table has 15 bits).  The restatement itself is pinned by known answers and by a float64 bilinear warp."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCFACE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]], np.float64)
# a template whose points are exact in float32 and stay exact under integer shifts (known answers without rounding)
QUARTER = np.array([[38.25, 51.75], [73.5, 51.5], [56.0, 71.75], [41.5, 92.25], [70.75, 92.25]], np.float32)


# ------------------------------------------------------------------------------------------ numpy restatement
def template_points(S, template=None):
    if template is None:
        return ARCFACE * (S / 112.0)
    return np.asarray(template, np.float32).astype(np.float64).reshape(5, 2)


def estimate(lm, q, S):
    """The chip -> source matrix M (6 float64) of one face: lm = 10 float32 landmark values, q = template points [5,2] float64."""
    f = np.float64
    with np.errstate(all="ignore"):
        p = np.asarray(lm, np.float32).astype(np.float64).reshape(5, 2)
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


def warp(img, M, S, want_inside=False):
    """The S x S chip of img [H,W,3] uint8 under M (all-zero M: the chip of an all-zero source)."""
    H, W = img.shape[:2]
    if not np.any(M):
        chip = np.zeros((S, S, 3), np.uint8)
        return (chip, np.zeros((S, S), bool)) if want_inside else chip
    t = np.arange(S, dtype=np.float64)
    ad = np.rint(M[0] * t * 1024.0).astype(np.int64)
    bd = np.rint(M[3] * t * 1024.0).astype(np.int64)
    X0 = np.rint((M[1] * t + M[2]) * 1024.0).astype(np.int64) + 16
    Y0 = np.rint((M[4] * t + M[5]) * 1024.0).astype(np.int64) + 16
    X = (X0[:, None] + ad[None, :]) >> 5
    Y = (Y0[:, None] + bd[None, :]) >> 5
    assert max(np.abs(X0).max() + np.abs(ad).max(), np.abs(Y0).max() + np.abs(bd).max()) < 2 ** 31      # the kernel's int32
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    acc = np.zeros((S, S, 3), np.int64)
    inside_all = np.ones((S, S), bool)
    for dy, dx, w in ((0, 0, (32 - fx) * (32 - fy)), (0, 1, fx * (32 - fy)), (1, 0, (32 - fx) * fy), (1, 1, fx * fy)):
        yy, xx = sy + dy, sx + dx
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        inside_all &= inside
        pix = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
        acc += (w * inside)[..., None] * pix
    chip = ((acc + 512) >> 10).astype(np.uint8)
    return (chip, inside_all) if want_inside else chip


def finish(chip, out="u8", rgb=False, mean=0.0, scale=1.0):
    if out == "u8":
        return chip
    v = (chip.astype(np.float32) - np.float32(mean)) * np.float32(scale)
    v = v[..., ::-1] if rgb else v
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def align_ref(imgs, lms, counts, size=112, template=None, out="u8", rgb=False, mean=0.0, scale=1.0):
    """ops.align_faces restated: (chips, matrices)."""
    q = template_points(size, template)
    chips, mats, n = [], [], 0
    for b, c in enumerate(counts):
        for i in range(int(c)):
            M = estimate(lms[n], q, size)
            chips.append(finish(warp(imgs[b], M, size), out, rgb, mean, scale))
            mats.append(M)
            n += 1
    shape = (0, 3, size, size) if out == "f32" else (0, size, size, 3)
    return (np.stack(chips) if chips else np.zeros(shape, np.float32 if out == "f32" else np.uint8),
            np.stack(mats) if mats else np.zeros((0, 6)))


def bits_equal(a, b):
    """Bit for bit (float64 matrices: -0.0 is not 0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------ inputs
def noise_images(rng, B, h, w):
    return rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)


def smooth_images(rng, B, h, w):
    """Neighbouring pixels differ by at most 8 levels (asserted)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((B, h, w, 3), np.uint8)
    for b in range(B):
        for c in range(3):
            px, py, ph = rng.uniform(25, 60), rng.uniform(25, 60), rng.uniform(0, 6.28, 2)
            out[b, :, :, c] = np.rint(127.5 + 60 * np.sin(x / px + ph[0]) + 60 * np.cos(y / py + ph[1]))
    i = out.astype(np.int32)
    assert np.abs(np.diff(i, axis=1)).max() <= 8 and np.abs(np.diff(i, axis=2)).max() <= 8
    return out


def pose_landmarks(rng, n, h, w, S, template=None, scale=(0.15, 4.0), margin=0.0, noise=0.5):
    """n landmark rows: the template (chip size S) scaled by a face scale from ``scale``, rotated by any angle, centred inside the
    image (``margin`` < 0: up to that fraction outside), plus a little jitter."""
    q = template_points(S, template)
    qc = q - q.mean(0)
    out = np.empty((n, 10), np.float32)
    for k in range(n):
        s, th = rng.uniform(*scale) * 112.0 / S, rng.uniform(0, 2 * np.pi)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        c = np.array([rng.uniform(margin * w, (1 - margin) * w), rng.uniform(margin * h, (1 - margin) * h)])
        out[k] = (s * qc @ R.T + c + rng.normal(0, noise, (5, 2))).reshape(10)
    return out


def hard_landmarks(rng, h, w, S):
    """The degenerate rows and the chips partly / wholly outside the image."""
    base = pose_landmarks(rng, 12, h, w, S, scale=(0.3, 1.5))
    base[0, :] = base[0, :2].repeat(5).reshape(2, 5).T.reshape(10)         # five coincident points: den = 0
    base[1, 3] = np.nan
    base[2, 6] = np.inf
    base[3, 0] = -np.inf
    base[4] = base[4, :2].repeat(5).reshape(2, 5).T.reshape(10) + rng.normal(0, 1e-5, 10).astype(np.float32)     # a face of a few float32 ulps
    base[5] = base[5] * np.float32(3e7)                                      # a face of millions of pixels, far away
    base[6] = base[6] - np.float32(20000.0)                                  # wholly outside
    base[7] = base[7] + np.float32(5000.0)
    base[8, 0::2] -= base[8, 0::2].mean() - 2.0                              # centred on the left edge
    base[9, 1::2] += (h - 3.0) - base[9, 1::2].mean()                        # ... the bottom edge
    base[10, 0::2] += (w - 1.0) - base[10, 0::2].mean()                      # ... the right edge
    base[10, 1::2] -= base[10, 1::2].mean()                                  # and the top one
    base[11] = np.float32(1e30)                                              # finite, coincident, sums overflow nothing but den = 0
    return base


# ------------------------------------------------------------------------------------------ CPU: the restatement
def test_restatement_translation_is_a_crop():
    rng = np.random.default_rng(0)
    img = noise_images(rng, 1, 400, 500)[0]
    dx, dy, S = 200, 150, 112
    # the exact-in-float32 template: M to the last bits
    lm = (QUARTER + np.float32([dx, dy])).reshape(10)
    M = estimate(lm, template_points(S, QUARTER), S)
    assert np.allclose(M, [1, 0, dx, 0, 1, dy], rtol=0, atol=1e-11), M
    assert np.array_equal(warp(img, M, S), img[dy:dy + S, dx:dx + S])
    # the default (ArcFace) template, landmarks rounded to float32: M to that rounding, the chip still exact
    lm = (ARCFACE + [dx, dy]).astype(np.float32).reshape(10)
    M = estimate(lm, template_points(S), S)
    assert np.allclose(M, [1, 0, dx, 0, 1, dy], rtol=0, atol=1e-4), M
    assert np.array_equal(warp(img, M, S), img[dy:dy + S, dx:dx + S])
    # another chip size scales the default template with it: landmarks = template * 2 + shift at S = 224
    lm = (ARCFACE * 2 + [dx, dy]).astype(np.float32).reshape(10)
    assert np.array_equal(warp(img, estimate(lm, template_points(224), 224), 224), img[dy:dy + 224, dx:dx + 224])


def test_restatement_rotated_template_gives_the_rotated_crop():
    rng = np.random.default_rng(1)
    img = noise_images(rng, 1, 400, 500)[0]
    dx, dy, S = 200, 150, 112
    lm = (QUARTER + np.float32([dx, dy])).reshape(10)
    # the template turned by 90 degrees inside the chip: chip pixel (x', y') = (S-1-y, x) of the upright chip
    turned = np.stack([S - 1 - QUARTER[:, 1], QUARTER[:, 0]], 1).astype(np.float32)
    M = estimate(lm, template_points(S, turned), S)
    assert np.allclose(M, [0, 1, dx, -1, 0, dy + S - 1], rtol=0, atol=1e-10), M
    assert np.array_equal(warp(img, M, S), np.rot90(img[dy:dy + S, dx:dx + S], -1))


def test_restatement_degenerate_landmarks_give_zero():
    rng = np.random.default_rng(2)
    img = noise_images(rng, 1, 64, 64)[0]
    q = template_points(112)
    good = (ARCFACE * 0.3 + 10).astype(np.float32).reshape(10)
    assert np.any(estimate(good, q, 112)) and np.any(warp(img, estimate(good, q, 112), 112))
    bad = [np.tile(np.float32([20, 30]), 5)]
    for v in (np.nan, np.inf, -np.inf):
        for k in (0, 7):
            r = good.copy()
            r[k] = v
            bad.append(r)
    bad.append(good * np.float32(1e30))                                     # |M| * S beyond the fixed-point range
    bad.append(good * np.float32(2e5))
    for r in bad:
        M = estimate(r, q, 112)
        assert bits_equal(M, np.zeros(6)), (r, M)
        assert not np.any(warp(img, M, 112))


def test_restatement_border_is_per_neighbour():
    rng = np.random.default_rng(3)
    img = noise_images(rng, 1, 200, 200)[0]
    S = 112
    lm = (QUARTER + np.float32([-3.0, -2.5])).reshape(10)                   # chip pixel (x, y) samples the image at (x - 3, y - 2.5)
    M = estimate(lm, template_points(S, QUARTER), S)
    assert np.allclose(M, [1, 0, -3, 0, 1, -2.5], rtol=0, atol=1e-11)
    chip = warp(img, M, S).astype(np.int64)
    i = img.astype(np.int64)
    assert not chip[:2].any() and not chip[:, :3].any()                     # wholly outside: zero
    assert np.array_equal(chip[2, 3:], (i[0, :S - 3] * 512 + 512) >> 10)    # the row above the image contributes 0: half weight
    assert np.array_equal(chip[3, 3:], (i[0, :S - 3] * 512 + i[1, :S - 3] * 512 + 512) >> 10)
    # over the right / bottom edge
    lm = (QUARTER + np.float32([200 - S + 2.5, 200 - S + 3.0])).reshape(10)
    chip = warp(img, estimate(lm, template_points(S, QUARTER), S), S).astype(np.int64)
    assert not chip[S - 3:].any() and not chip[:, S - 2:].any()
    assert np.array_equal(chip[:S - 3, S - 3], (i[200 - S + 3:200, 199] * 512 + 512) >> 10)


def bilinear_f64(img, M, S):
    """Bilinear interpolation in float64 at the unquantised positions, rounded to the nearest level."""
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    u, v = M[0] * x + M[1] * y + M[2], M[3] * x + M[4] * y + M[5]
    H, W = img.shape[:2]
    x0, y0 = np.floor(u), np.floor(v)
    fx, fy = (u - x0)[..., None], (v - y0)[..., None]
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    g = lambda yy, xx: img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.float64)      # noqa: E731
    val = (g(yi, xi) * (1 - fx) + g(yi, xi + 1) * fx) * (1 - fy) + (g(yi + 1, xi) * (1 - fx) + g(yi + 1, xi + 1) * fx) * fy
    return np.floor(val + 0.5)


def test_restatement_within_one_level_of_float64_bilinear():
    """Smooth image (neighbours differ by <= 8 levels), 300 random poses with face scale 0.15-4, any rotation, centres inside the
    image: every chip pixel whose four neighbours lie inside the image is within 1 level of the rounded float64 value.  Position
    error <= 1/64 + 2/1024 px per axis x 2 axes x 8 levels < 0.3; the two roundings add 0.5 each: the sum is under 1.5."""
    rng = np.random.default_rng(4)
    S, h, w = 112, 480, 640
    img = smooth_images(rng, 1, h, w)[0]
    lms = pose_landmarks(rng, 300, h, w, S)
    q = template_points(S)
    compared, worst = 0, 0
    for lm in lms:
        M = estimate(lm, q, S)
        assert np.any(M)
        chip, inside = warp(img, M, S, want_inside=True)
        d = np.abs(chip.astype(np.int64) - bilinear_f64(img, M, S).astype(np.int64))[inside]
        compared += d.size
        worst = max(worst, int(d.max(initial=0)))
    print("compared %d values, worst difference %d" % (compared, worst))
    assert compared > 3_000_000
    assert worst <= 1


def test_restatement_agrees_with_least_squares():
    """The estimate is the least-squares similarity source -> chip: against numpy.linalg.lstsq on [x -y 1 0; y x 0 1]."""
    rng = np.random.default_rng(5)
    q = template_points(112)
    for lm in pose_landmarks(rng, 50, 480, 640, 112, noise=2.0):
        p = lm.astype(np.float64).reshape(5, 2)
        A = np.zeros((10, 4))
        A[0::2] = np.stack([p[:, 0], -p[:, 1], np.ones(5), np.zeros(5)], 1)
        A[1::2] = np.stack([p[:, 1], p[:, 0], np.zeros(5), np.ones(5)], 1)
        a, b, tx, ty = np.linalg.lstsq(A, q.reshape(10), rcond=None)[0]
        fwd = np.array([[a, -b, tx], [b, a, ty], [0, 0, 1]])
        want = np.linalg.inv(fwd)[:2].reshape(6)
        got = estimate(lm, q, 112)
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * max(1.0, np.abs(want).max())), (got, want)


# ------------------------------------------------------------------------------------------ CPU: the ABI
def _opts(**kw):
    return cfa._lib.align_opts(**kw)[0]


def test_align_abi_declared_exported_and_validated_without_a_gpu():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(CF_CHIP_[A-Z0-9_]+)\s+(\d+)", text)}
    assert consts == {"CF_CHIP_U8_HWC_BGR": 0, "CF_CHIP_F32_NCHW": 1}
    for k, v in consts.items():
        assert getattr(cfa._lib, k) == v
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fields = re.search(r"typedef struct cf_align_opts\s*\{(.*?)\}\s*cf_align_opts;", code, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[;,]", fields)
    assert names == ["size", "format", "rgb", "mean", "scale", "tmpl", "max_per_image"]
    assert [f for f, _ in cfa._lib.AlignOpts._fields_] == names
    L = cfa._lib.lib()
    for sym in ("cf_align_faces", "cf_op_align_faces"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), sym
        assert sym in cfa._lib.EXPORTS and hasattr(L, sym)
    img = np.zeros((1, 32, 32, 3), np.uint8)
    lms = np.zeros((1, 10), np.float32)
    cnt = np.ones((1,), np.int32)
    chips = np.zeros((1, 512, 512, 3), np.float32)
    P = cfa._lib.ptr

    def op(o, imgs=img, lm=lms, c=cnt, out=chips, B=1, h=32, w=32):
        return L.cf_op_align_faces(0, P(imgs), B, h, w, P(lm), P(c), C.byref(o) if o is not None else None, P(out), None)
    for size in (0, 12, 15, 18, 113, 516, 1024, -112):
        assert op(_opts(size=size)) == -1, size
        assert b"size" in L.cf_op_last_error()
    for fmt in (-1, 2, 7):
        assert op(_opts(out=fmt)) == -1, fmt
    assert op(_opts(max_per_image=-1)) == -1
    assert op(None) == -1
    assert op(_opts(), imgs=None) == -1 and op(_opts(), lm=None) == -1 and op(_opts(), c=None) == -1 and op(_opts(), out=None) == -1
    assert op(_opts(), B=0) == -1 and op(_opts(), h=0) == -1 and op(_opts(), w=1) == -1
    assert op(_opts(), c=np.array([-1], np.int32)) == -1
    # cf_align_faces: nothing works without a context, and nothing reaches the GPU
    offs = np.zeros((2,), np.int32)
    o = _opts()
    assert L.cf_align_faces(None, C.byref(o), P(chips), None, P(offs), 1, 0) == -1
    assert L.cf_align_faces(None, None, None, None, None, -1, 0) == -1
    with pytest.raises(ValueError):
        cfa._lib.align_opts(out="yuv")
    with pytest.raises(ValueError):
        cfa._lib.align_opts(template=np.zeros((4, 2)))
    with pytest.raises(ValueError):
        ops.align_faces(img, lms, np.array([2], np.int32))


def test_align_source_has_no_scalar_memory_writes_and_no_switch():
    src = open(os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc", "cf_align.hip")).read().lower()
    words = ["s_" + mid + kind for mid in ("", "buffer_", "scratch_") for kind in ("sto" + "re", "ato" + "mic")] + ["s_dca" + "che"]
    for wd in words:
        assert wd not in src, wd
    for wd in ("getenv", "cf_env_int", "cf_ab_int", "asm"):
        assert wd not in src, wd
    mk = open(os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc", "Makefile")).read()
    assert "cf_align.hip" in mk and re.search(r"EXTRA_cf_align\s*=\s*-ffp-contract=off", mk)


# ------------------------------------------------------------------------------------------ on the GPU
OP_CASES = [
    # B, h, w, S, template, chip options, image kind
    (1, 96, 128, 16, None, dict(out="u8"), "noise"),
    (3, 200, 320, 112, None, dict(out="u8"), "noise"),
    (3, 200, 320, 112, "custom", dict(out="f32", rgb=True, mean=127.5, scale=1 / 128.0), "smooth"),
    (3, 241, 323, 512, "custom", dict(out="u8"), "smooth"),
    (3, 120, 90, 128, None, dict(out="f32", rgb=False, mean=3.25, scale=0.0173), "noise"),
    (64, 96, 96, 128, "custom", dict(out="f32", rgb=True, mean=0.0, scale=1.0), "smooth"),
    (64, 64, 80, 112, None, dict(out="u8"), "noise"),
]


def _custom_template(S):
    """A five-point pattern of its own (not a scaled ArcFace): eyes higher and wider, in chip pixels of size S."""
    return (np.float32([[0.30, 0.35], [0.70, 0.36], [0.5, 0.55], [0.35, 0.74], [0.66, 0.75]]) * np.float32(S)).astype(np.float32)


@pytest.mark.gpu
def test_op_align_faces_bit_exact():
    """The kernel alone against the restatement, bit for bit in chips and float64 matrices: noise and smooth images, B = 1, 3, 64,
    S = 16, 112, 128, 512, default and custom templates, both formats and channel orders, non-trivial mean / scale, counts with
    zeros, the degenerate landmark rows and chips partly / wholly outside the image."""
    total = zero_mats = partial = outside = 0
    seen = set()
    for k, (B, h, w, S, tmpl, opt, kind) in enumerate(OP_CASES):
        rng = np.random.default_rng(100 + k)
        imgs = (noise_images if kind == "noise" else smooth_images)(rng, B, h, w)
        template = _custom_template(S) if tmpl == "custom" else None
        if B == 64:
            counts = rng.integers(0, 5, B).astype(np.int32)
            counts[[0, 7, 63]] = 0
            counts[1] = 12                                          # the hard rows all land in image 1
        else:
            counts = np.array([12, 0, 5][:B] if B == 3 else [12 + 4], np.int32)
        n = int(counts.sum())
        lms = pose_landmarks(rng, n, h, w, S, template, scale=(0.15, 4.0) if S < 512 else (0.15, 1.2), margin=-0.2)
        first = int(counts[:1].sum()) if B == 64 else 0
        lms[first:first + 12] = hard_landmarks(rng, h, w, S)
        got_c, got_m = ops.align_faces(imgs, lms, counts, size=S, template=template, **opt)
        want_c, want_m = align_ref(imgs, lms, counts, S, template, **opt)
        assert got_c.dtype == want_c.dtype and got_c.shape == want_c.shape
        assert bits_equal(got_m, want_m), (k, np.argwhere(got_m != want_m)[:5])
        assert bits_equal(got_c, want_c), (k, np.argwhere(got_c != want_c)[:5])
        total += n
        zero_mats += int((~want_m.any(1)).sum())
        u8 = want_c if opt["out"] == "u8" else None
        if u8 is not None:
            blank = [~c.any(2) for c in u8]                        # pixels the border rule zeroed (the images hold no black pixel to speak of)
            partial += sum(1 for z, m in zip(blank, want_m) if m.any() and z.sum() > 50 and (~z).sum() > 50)
            outside += sum(1 for z, m in zip(blank, want_m) if m.any() and z.all())
        seen.add((B, S, tmpl, opt["out"], bool(opt.get("rgb")), kind))
    assert total >= 200, total
    assert zero_mats >= 6 * len(OP_CASES)                           # the degenerate rows were there, in every case
    assert partial >= 3 and outside >= 3                            # and chips that hang over an edge or miss the image altogether
    assert {s[0] for s in seen} == {1, 3, 64} and {s[1] for s in seen} == {16, 112, 128, 512}
    # no faces at all
    c0, m0 = ops.align_faces(imgs[:2], np.zeros((0, 10), np.float32), np.zeros(2, np.int32), size=16)
    assert c0.shape == (0, 16, 16, 3) and m0.shape == (0, 6)


FEEDS = ("forward", "forward_device", "resized", "yuv", "images", "images_identity")


# what the frames of a feed are made of, tried in this order until the default weights keep a face (they answer to fine detail: noise
# that a resize has smoothed may leave no cell above the threshold): (kind, (h, w) of the source for the feeds that resize)
SOURCES = (("noise", (75, 101)), ("binary", (75, 101)), ("binary", (96, 127)), ("noise", (192, 256)), ("binary", (192, 256)),
           ("blocks", (150, 200)), ("binary", (97, 129)), ("blocks", (75, 101)))


def source_frames(rng, kind, shape):
    """uint8 frames of any shape: uniform noise, noise of the two extreme levels, or 4-pixel runs of one noise value along the last two
    axes that vary (coarse noise that survives a resize)."""
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "binary":
        return rng.choice(np.array([0, 255], np.uint8), shape)
    ax = (1, 2)
    small = tuple((n + 3) // 4 if a in ax else n for a, n in enumerate(shape))
    a = rng.integers(0, 256, small, dtype=np.uint8)
    for k in ax:
        a = np.repeat(a, 4, axis=k)
    return np.ascontiguousarray(a[tuple(slice(0, n) for n in shape)])


def _feed(eng, how, rng, keep, kind="noise", hw=(75, 101)):
    """Run one forward of the named kind on frames of ``kind``; returns the uint8 batch the network read."""
    H, W, B = eng.H, eng.W, 3
    if how == "forward":
        x = source_frames(rng, kind, (B, H, W, 3))
        eng.forward_enqueue(x)
        return x
    if how == "forward_device":
        x = source_frames(rng, kind, (B, H, W, 3))
        d = eng.device_alloc(x.nbytes)
        keep.append(d)
        eng.memcpy_h2d(d, x)
        eng.forward_enqueue(d, on_device=True, B=B, in_format=cfa._lib.CF_IN_U8_HWC_BGR)
        return x
    if how == "resized":
        eng.forward_resized_enqueue(source_frames(rng, kind, (B,) + hw + (3,)))
    elif how == "yuv":
        h, w = hw[0] // 2 * 2, hw[1] // 2 * 2
        eng.forward_yuv_enqueue(source_frames(rng, kind, (B, h * 3 // 2, w)), "nv12")
    elif how == "images":
        eng.forward_images_enqueue(list(source_frames(rng, kind, (B,) + hw + (3,))))
    elif how == "images_identity":
        ims = list(source_frames(rng, kind, (B, H, W, 3)))
        eng.forward_images_enqueue(ims)
        return np.stack(ims)
    return eng.resized_input()


def _feed_until_faces(eng, how, rng, keep, need=1):
    """The first of SOURCES whose forward + threshold decode (network coordinates) keeps at least ``need`` faces:
    (the batch the network read, the decode's result).  Fails when none does."""
    tried = []
    for kind, hw in SOURCES:
        src = _feed(eng, how, rng, keep, kind, hw)
        base = eng.decode_threshold(0.3, 0.3, 64)
        tried.append((kind, hw, [len(d) for d, _ in base]))
        if sum(len(d) for d, _ in base) >= need:
            print("feed %s: %s %s keeps %s faces" % ((how,) + tried[-1]))
            return src, base
    raise AssertionError("no source kept %d faces with the default weights: %s" % (need, tried))


@pytest.mark.gpu
@pytest.mark.parametrize("how", FEEDS)
def test_engine_align_faces_equals_restatement(how):
    """Engine.align_faces behind every kind of forward + decode_threshold, default weights: bit for bit the restatement applied to
    the batch the network read and the decode's UNRESCALED landmarks, with set_rescale off and on; the decode's own outputs are not
    changed by the call."""
    rng = np.random.default_rng(FEEDS.index(how))
    eng = cfa.Engine(96, 128, max_batch=3, dtype="bf16")
    keep = []
    src, base = _feed_until_faces(eng, how, rng, keep)
    counts = np.array([len(d) for d, _ in base], np.int32)
    net_lms = np.concatenate([l for _, l in base])
    for rescale, opt in ((False, dict(size=112)), (True, dict(size=128, out="f32", rgb=True, mean=127.5, scale=1 / 128.0, template=_custom_template(128)))):
        eng.set_rescale(1.37, 1.21) if rescale else eng.set_rescale(0.0, 0.0)
        dec = eng.decode_threshold(0.3, 0.3, 64)
        chips, offs, mats = eng.align_faces(**opt)
        again = eng.decode_threshold(0.3, 0.3, 64)
        for (d, l), (d2, l2), (d0, l0) in zip(dec, again, base):
            assert bits_equal(d, d2) and bits_equal(l, l2)
            if rescale:
                assert np.array_equal(l[:, 0::2], np.floor(l0[:, 0::2].astype(np.float64) / np.float64(np.float32(1.21))).astype(np.float32))
            else:
                assert bits_equal(l, l0) and bits_equal(d, d0)
        assert np.array_equal(offs, np.concatenate([[0], np.cumsum(counts)]))
        want_c, want_m = align_ref(src, net_lms, counts, **opt)
        assert len(chips) == len(want_c) == int(counts.sum())
        assert bits_equal(mats, want_m) and bits_equal(chips, want_c), (how, rescale)
        assert int(want_m.any(1).sum()) >= 1, "no alignable face in this case: nothing was compared"
    eng.set_rescale(0.0, 0.0)
    # a per-image limit keeps the first rows of every image
    chips2, offs2, mats2 = eng.align_faces(112, max_per_image=1)
    c1 = np.minimum(counts, 1)
    assert np.array_equal(offs2, np.concatenate([[0], np.cumsum(c1)]))
    full_c, _, full_m = eng.align_faces(112)
    first = np.concatenate([[0], np.cumsum(counts)])[:-1][counts > 0]
    assert bits_equal(chips2, full_c[first]) and bits_equal(mats2, full_m[first])
    for d in keep:
        eng.device_free(d)
    eng.close()


@pytest.mark.gpu
def test_engine_align_truncation_state_errors_and_device_form():
    rng = np.random.default_rng(21)
    eng = cfa.Engine(96, 128, max_batch=3, dtype="bf16")
    L, P = cfa._lib.lib(), cfa._lib.ptr
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):      # a batch of which the default weights keep two faces or more
        x = source_frames(rng, kind, (3, 96, 128, 3))
        eng.forward_enqueue(x)
        if sum(len(d) for d, _ in eng.decode_threshold(0.3, 0.3, 64)) >= 2:
            break
    eng.close()
    eng = cfa.Engine(96, 128, max_batch=3, dtype="bf16")                   # a fresh context: nothing forwarded yet
    # before any forward / before any threshold decode / after a float forward: CF_ESTATE
    for prepare in (lambda: None, lambda: eng.forward_enqueue(x), lambda: (eng.forward_enqueue(x), eng.decode_topk(10)),
                    lambda: (eng.forward_enqueue(np.zeros((2, 3, 96, 128), np.float32)), eng.decode_threshold())):
        prepare()
        with pytest.raises(cfa._lib.CenterFaceError) as e:
            eng.align_faces()
        assert e.value.code == cfa._lib.CF_ESTATE
    eng.forward_enqueue(x)
    dec = eng.decode_threshold(0.3, 0.3, 64)
    total = sum(len(d) for d, _ in dec)
    assert total >= 2
    chips, offs, mats = eng.align_faces(112)
    assert len(chips) == total == offs[-1]
    # a forward after the decode: the decode is gone
    eng.forward_enqueue(x)
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        eng.align_faces()
    assert e.value.code == cfa._lib.CF_ESTATE
    dec = eng.decode_threshold(0.3, 0.3, 64)
    # truncation: cap_faces below the total leaves the later rows untouched and reports the number wanted
    cap = total - 1
    o = cfa._lib.align_opts(112)[0]
    buf = np.full((total, 112, 112, 3), 0xAB, np.uint8)
    mb = np.full((total, 6), -7.0)
    of = np.zeros(4, np.int32)
    assert L.cf_align_faces(eng._h, C.byref(o), P(buf), P(mb), P(of), cap, 0) == 0
    assert of[-1] == total and np.array_equal(of, offs)
    assert bits_equal(buf[:cap], chips[:cap]) and bits_equal(mb[:cap], mats[:cap])
    assert (buf[cap:] == 0xAB).all() and (mb[cap:] == -7.0).all()
    c2, o2, m2 = eng.align_faces(112, max_faces=cap)
    assert len(c2) == cap and o2[-1] == total and bits_equal(c2, chips[:cap])
    c3, o3, _ = eng.align_faces(112, max_faces=0)
    assert len(c3) == 0 and o3[-1] == total
    # a decode that wrote fewer rows than it kept: only the written rows are faces
    # (the Python wrapper regrows max_out: the library is called directly for a short decode)
    d5, l10, cn = np.empty((3, 1, 5), np.float32), np.empty((3, 1, 10), np.float32), np.empty(3, np.int32)
    assert L.cf_decode_threshold(eng._h, 0.3, 0.3, 1, P(d5), P(l10), P(cn)) == 0
    c4, o4, m4 = eng.align_faces(112)
    assert np.array_equal(o4, np.concatenate([[0], np.cumsum(np.minimum(cn, 1))]))
    firsts = offs[:-1][np.diff(offs) > 0]
    assert bits_equal(c4, chips[firsts]) and bits_equal(m4, mats[firsts])
    # bad arguments on a live context
    for bad in (dict(size=100 + 2), dict(size=8), dict(size=520), dict(out=5)):
        with pytest.raises(ValueError):
            eng.align_faces(**{"size": 112, **bad})
    assert L.cf_align_faces(eng._h, C.byref(o), P(buf), None, P(of), -1, 0) == -1
    assert L.cf_align_faces(eng._h, C.byref(o), None, None, P(of), 1, 0) == -1
    assert L.cf_align_faces(eng._h, C.byref(o), P(buf), None, None, 1, 0) == -1
    # the device-output form: asynchronous, equal to the host form after synchronize
    eng.decode_threshold(0.3, 0.3, 64)
    opt = dict(size=64, out="f32", rgb=True, mean=10.0, scale=0.5)
    want_c, want_o, want_m = eng.align_faces(**opt)
    nb = total * 3 * 64 * 64 * 4
    dc, dm, do = eng.device_alloc(nb), eng.device_alloc(total * 48), eng.device_alloc(16)
    eng.align_faces_device(dc, do, total, dm, **opt)
    eng.synchronize()
    gc, gm, go = np.empty((total, 3, 64, 64), np.float32), np.empty((total, 6)), np.empty(4, np.int32)
    eng.memcpy_d2h(gc, dc)
    eng.memcpy_d2h(gm, dm)
    eng.memcpy_d2h(go, do)
    assert bits_equal(gc, want_c) and bits_equal(gm, want_m) and np.array_equal(go, want_o)
    with pytest.raises(ValueError):
        eng.align_faces_device(dc + 4, do, total, dm, **opt)                  # misaligned chips
    for p in (dc, dm, do):
        eng.device_free(p)
    eng.close()


@pytest.mark.gpu
def test_centerface_detect_aligned():
    """dets / lms identical to detect_batch (rescale included), chips = the Engine path's rows, an image without detections gives
    an empty [0,S,S,3] array; landmarks=False instances refuse."""
    rng = np.random.default_rng(31)
    sd = cfa.weights.synthetic_state_dict(0)
    for hw in ((100, 150), (96, 128)):                                        # resized on the device / identity
        face = cfa.CenterFace(*hw, dtype="bf16", max_batch=2)
        for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):     # frames of which the default weights keep a face
            imgs = list(source_frames(rng, kind, (3,) + hw + (3,)))
            want = face.detect_batch(imgs)
            if sum(len(d) for d, _ in want) >= 1:
                break
        got = face.detect_aligned(imgs, size=112)
        assert len(got) == 3
        n_faces = 0
        for (d, l, c), (wd, wl) in zip(got, want):
            assert bits_equal(d, wd) and bits_equal(l, wl)
            assert c.shape == (len(d), 112, 112, 3) and c.dtype == np.uint8
            n_faces += len(d)
        assert n_faces >= 1
        # the same rows as the Engine path, chunk by chunk (max_batch = 2)
        eng = face.engine
        rows = []
        for i in (0, 2):
            chunk = np.stack(imgs[i:i + 2])
            eng.forward_enqueue(chunk) if hw == (96, 128) else eng.forward_resized_enqueue(chunk)
            eng.decode_threshold(0.3, face.nms_thresh, face.max_dets)
            rows.append(eng.align_faces(112)[0])
        assert bits_equal(np.concatenate([c for _, _, c in got]), np.concatenate(rows))
        f32 = face.detect_aligned(imgs, size=64, out="f32", rgb=True, mean=127.5, scale=1 / 128.0)
        assert all(c.shape == (len(d), 3, 64, 64) and c.dtype == np.float32 for d, _, c in f32)
        face.close()
    # no detections: a heat-map bias far below the threshold
    quiet = dict(sd)
    quiet["hm.1.bias"] = sd["hm.1.bias"] - np.float32(100.0)
    face = cfa.CenterFace(96, 128, dtype="bf16", max_batch=2, weights=quiet)
    for d, l, c in face.detect_aligned(imgs, size=112):
        assert d.shape == (0, 5) and l.shape == (0, 10) and c.shape == (0, 112, 112, 3) and c.dtype == np.uint8
    face.close()
    plain = cfa.CenterFace(96, 128, landmarks=False, dtype="bf16")
    with pytest.raises(ValueError):
        plain.detect_aligned(imgs)
    plain.close()
