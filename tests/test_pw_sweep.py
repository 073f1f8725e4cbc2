"""Every pointwise-conv kernel variant ``dispatch_nbw`` (csrc/cf_pw.hip) picks, crossed with the tails each one clamps.

``cf_pw.hip`` is the GEMM under every 1x1 convolution of the network: three kernels (``pw_kernel``, ``pw_wlds_kernel``,
``pw_ksplit_kernel``) and ~150 template instances chosen from the shape -- storage type, n-blocks per wave (NBW 1..5), LDS ring
depth (NST 2/3/4), epilogue.  The production shapes the rest of the suite uses have M a multiple of 32 and the network's own K and
N; here every case FIRST asserts which instance it reached (``ops.last_kernel()``), so a retuned heuristic cannot silently drop
coverage, and then checks parity at shapes whose tails are all live:

  * M % 32 in {1, 2, 3, 5, 6, 7, 13, 15, 23, 27, 29, 30, 31}, and M % 128 < 32 (whole idle waves)
  * N % 32 in {8, 16, 24}; NB not a multiple of NBW (the ``nbv < NBW`` paths: b3, c2, c4, e1, e3)
  * odd NC in bf16 (K % 16 = 8: one lane half owns a chunk less -- none at all for K = 8, a1), odd NCh in split mode (the last
    chunk of a lane half is unpaired), NCh % 4 != 0 (a K tail tile), NT = 1 < NST - 1 (c1, c7), a short K quarter of a k-split
    wave (e1: NCh = 33, per = 9)

References and bounds (the project's own):
  * fp32 / fp32_split: a float64 numpy restatement of the op on the float32 inputs, at F32 (2e-5) / SPLIT (1e-4) of
    tests/test_gpu_parity.py.  With these inputs a reversed-order float32 sum sits at 0.10 of the fp32 bound and a three-product
    bf16 split at 0.53 of the split bound (CPU check): a correct kernel has margin, a dropped chunk or split term has none.
  * bf16: ``E.pw_op`` under ``E.tolerance`` / ``E.accept``, applied three times -- whole tensor, the last M % 128 pixels, the
    channels of the last n-block -- so that the outlier fraction ``accept`` tolerates cannot hide a wrong tail.
  * every dtype: no NaN / Inf anywhere.  The per-op path fills y and the pad behind every buffer with 0xFF bytes, so a skipped
    store or a read past a buffer IS a NaN.

Measured ratios: profiles/pw_sweep_parity.md.  The checks of the two hooks that need no GPU (declared, exported, layout bits
validated before any GPU work) are in tests/test_abi.py, where this module's ``pytestmark`` does not reach.
"""
import functools

import numpy as np
import pytest
import torch

import centerface_amd as cfa
from centerface_amd import ops
from oracle import bf16_emulation as E
from test_gpu_parity import F32, SPLIT

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "fp32_split", "bf16")
_T = {"bf16": "unsigned short", "fp32": "float", "fp32_split": "sp32_t"}
_ACT = ("none", "swish", "relu")


def _full_tag(short, dtype):
    """'pw<1,0,0,false>' / 'wl<3,0,1,4>' / 'ks<3,0,1>' -> the symbol set_kernel_tag prints."""
    kind, args = short[:2], short[3:-1].replace(",", ", ")
    if kind == "pw":
        return "void cf::pw_kernel<%s, %s>(cf::PwParams)" % (_T[dtype], args)
    if kind == "wl":
        return "void cf::pw_wlds_kernel<%s, %s>(cf::PwParams)" % (_T[dtype], args)
    assert kind == "ks" and dtype == "bf16"
    return "void cf::pw_ksplit_kernel<%s>(cf::PwParams)" % args


# id: (B, H, W, K, N, act, bias, res, bf16 tag, fp32 and fp32_split tag)
CASES = {
    "a1": (1, 5, 7, 8, 8, 0, 0, 0, "pw<1,0,0,false>", None),
    "a2": (2, 9, 11, 24, 40, 0, 0, 1, "pw<1,0,1,false>", None),
    "a3": (1, 13, 17, 40, 24, 1, 0, 0, "pw<1,1,0,false>", None),
    "a4": (3, 7, 9, 72, 56, 1, 1, 0, "pw<1,1,0,true>", None),
    "a5": (1, 11, 13, 24, 88, 2, 1, 0, "pw<1,2,0,true>", None),
    "a6": (1, 6, 37, 56, 16, 0, 1, 0, "pw<1,0,0,true>", None),
    "b1": (1, 157, 419, 16, 120, 1, 0, 0, "pw<2,1,0,false>", None),
    "b2": (1, 157, 419, 24, 168, 0, 1, 0, "pw<3,0,0,true>", None),
    "b3": (1, 157, 419, 16, 216, 0, 0, 0, "pw<4,0,0,false>", None),
    "b4": (1, 157, 419, 8, 248, 1, 1, 0, "pw<4,1,0,true>", None),
    "b5": (3, 47, 929, 24, 152, 0, 0, 1, "pw<5,0,1,false>", None),
    "b6": (1, 157, 419, 40, 184, 2, 1, 0, "pw<3,2,0,true>", None),
    "c1": (1, 9, 15, 64, 72, 0, 0, 0, "wl<3,0,0,4>", None),
    "c2": (2, 7, 23, 72, 152, 0, 0, 1, "wl<3,0,1,4>", None),
    "c3": (1, 19, 21, 200, 120, 1, 0, 0, "wl<4,1,0,4>", None),
    "c4": (3, 5, 11, 88, 216, 0, 0, 1, "wl<4,0,1,4>", None),
    "c5": (1, 23, 29, 136, 312, 1, 0, 0, "wl<5,1,0,3>", None),
    "c6": (1, 3, 43, 328, 320, 0, 0, 1, "wl<5,0,1,3>", None),
    "c7": (1, 17, 19, 64, 384, 1, 0, 0, "wl<4,1,0,4>", "wl<3,1,0,4>"),       # wide fp32 expand: three n-blocks per wave
    "d1": (1, 131, 127, 72, 88, 1, 0, 0, "wl<3,1,0,2>", None),
    "d2": (1, 131, 127, 104, 104, 0, 0, 1, "wl<4,0,1,2>", None),
    "d3": (1, 91, 93, 64, 312, 0, 0, 0, "wl<5,0,0,2>", None),
    "d4": (1, 131, 127, 64, 384, 1, 0, 0, "wl<4,1,0,2>", "wl<3,1,0,2>"),
    "e1": (1, 31, 34, 520, 136, 0, 0, 1, "ks<3,0,1>", "wl<3,0,1,4>"),
    "e2": (1, 32, 33, 512, 288, 1, 0, 0, "ks<3,1,0>", "wl<4,1,0,4>"),
    "e3": (2, 33, 32, 584, 200, 0, 0, 0, "ks<2,0,0>", "wl<4,0,0,4>"),
    "e4": (1, 37, 41, 960, 128, 0, 0, 1, "ks<2,0,1>", "wl<4,0,1,4>"),
    "e5": (1, 63, 65, 520, 136, 0, 0, 0, "ks<3,0,0>", "wl<3,0,0,4>"),
    # just outside each k-split threshold (HW < 1024, HW = 4096, N < 128, K < 512): pw_wlds_kernel in every dtype
    "e6": (1, 31, 33, 520, 136, 0, 0, 0, "wl<3,0,0,4>", None),
    "e7": (1, 64, 64, 520, 136, 0, 0, 0, "wl<3,0,0,4>", None),
    "e8": (1, 32, 33, 520, 120, 0, 0, 0, "wl<4,0,0,4>", None),
    "e9": (1, 32, 33, 504, 136, 0, 0, 0, "wl<3,0,0,4>", None),
}


def expected_tag(cid, dtype):
    c = CASES[cid]
    return _full_tag(c[8] if dtype == "bf16" or c[9] is None else c[9], dtype)


def _seed(cid):
    return int.from_bytes(cid.encode(), "little")


def _make(rng, shape, quantised, scale=1.0):
    v = (scale * rng.standard_normal(shape)).astype(np.float32)
    return E.q_bf16(torch.from_numpy(v)).numpy() if quantised else v


@functools.lru_cache(maxsize=None)
def _inputs(cid, quantised, shape=None):
    """(x, w, bias, res) of a case, seeded from its id; ``shape`` = another (B, H, W) for the same layer."""
    B, H, W, K, N, act, bias, res = CASES[cid][:8]
    if shape is not None:
        B, H, W = shape
    rng = np.random.default_rng(_seed(cid))
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = (0.5 * rng.standard_normal(N)).astype(np.float32) if bias else None
    x = _make(rng, (B, K, H, W), quantised)
    r = _make(rng, (B, N, H, W), quantised) if res else None
    return x, w, b, r                      # shared between the tests: never written to


def _launch(cid, dtype, x, w, b, r, layout=0):
    y = ops.conv_pw(x, w, act=_ACT[CASES[cid][5]], bias=b, residual=r, dtype=dtype, layout=layout)
    return y, ops.last_kernel()


def _run(cid, dtype, layout=0):
    return _launch(cid, dtype, *_inputs(cid, dtype == "bf16"), layout=layout)


def _ref64(cid, x, w, b, r):
    """float64 restatement: multiply the float32 inputs in float64, + bias, act (swish = v / (1 + exp(-v))), + residual."""
    act = CASES[cid][5]
    v = np.einsum("bkhw,nk->bnhw", x.astype(np.float64), w.astype(np.float64), optimize=True)
    if b is not None:
        v = v + b.astype(np.float64).reshape(1, -1, 1, 1)
    if act == 1:
        v = v / (1.0 + np.exp(-v))
    elif act == 2:
        v = np.maximum(v, 0.0)
    if r is not None:
        v = v + r.astype(np.float64)
    return v


def _emu_stat(ratio):
    return (float(ratio.max()), float((ratio > 1).mean()), float((ratio > 0.5).mean()), float((ratio > 0).mean()))


def _check_parity(cid, dtype, y, x, w, b, r):
    """Worst |d| / bound of the case (asserted <= 1 for fp32 / split; under E.accept on three slices for bf16)."""
    assert np.isfinite(y).all(), "%s %s: %d non-finite outputs, first at %s" % (
        cid, dtype, int((~np.isfinite(y)).sum()), np.argwhere(~np.isfinite(y))[0])
    B, N, H, W = y.shape
    if dtype != "bf16":
        tol = F32 if dtype == "fp32" else SPLIT
        ref = _ref64(cid, x, w, b, r)
        ratio = np.abs(y.astype(np.float64) - ref) / (tol["atol"] + tol["rtol"] * np.abs(ref))
        worst = float(ratio.max())
        print("PWSWEEP %s %s %.4f" % (cid, dtype, worst))
        assert worst <= 1.0, "%s %s: |d| / (atol + rtol |ref|) = %.3f at %s" % (cid, dtype, worst, np.unravel_index(ratio.argmax(), ratio.shape))
        return worst
    ref = E.pw_op(x, w, bias=b, act=_ACT[CASES[cid][5]], residual=r).numpy().astype(np.float64)
    ratio = np.abs(y.astype(np.float64) - ref) / E.tolerance(ref)
    M = B * H * W
    tail = M % 128 or 128
    by_pixel = ratio.transpose(0, 2, 3, 1).reshape(M, N)                 # pixel-major, the kernel's m
    slices = (("whole", ratio), ("last %d pixels" % tail, by_pixel[M - tail:]), ("last n-block", ratio[:, (N - 1) // 32 * 32:]))
    print("PWSWEEP %s %s %.4f differing %.2e" % (cid, dtype, float(ratio.max()), float((ratio > 0).mean())))
    for what, part in slices:
        stat = _emu_stat(part)
        assert E.accept(stat, True, part.size), "%s bf16, %s: max |d|/tol %.2f, frac > tol %.1e, > tol/2 %.1e, differing %.1e (n = %d)" % (
            (cid, what) + stat + (part.size,))
    return float(ratio.max())


# ------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", list(CASES))
def test_variant_reached_and_parity(cid, dtype):
    y, tag = _run(cid, dtype)
    assert tag == expected_tag(cid, dtype), (cid, dtype, tag)
    _check_parity(cid, dtype, y, *_inputs(cid, dtype == "bf16"))


# ------------------------------------------------------------------------------- pixel-block addressing
LAYOUTS = [(c, 0b111) for c in ("a2", "b5", "c2", "c6", "d2", "e1", "e4")] + [(c, 0b011) for c in ("b1", "c3", "e2")]
LAYOUTS += [("a1", 0b011), ("b4", 0b011)]         # K = 8 in pixel-block order: a chunk past a bf16 pixel's row is the NEXT BLOCK's


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid,layout", LAYOUTS, ids=["%s-%d" % cl for cl in LAYOUTS])
def test_pixel_block_layouts_change_only_the_addressing(cid, layout, dtype):
    """x / y / residual in pixel-block order (PwParams::xblock / yblock / resblock, what the engine's late layers use): the same
    instance, the same bits."""
    y0, tag0 = _run(cid, dtype)
    y1, tag1 = _run(cid, dtype, layout)
    assert tag1 == tag0 == expected_tag(cid, dtype)
    assert np.array_equal(y0, y1), (cid, dtype, int((y0 != y1).sum()), np.argwhere(y0 != y1)[:3])


# ------------------------------------------------------------------------------- batch invariance
@pytest.mark.parametrize("dtype", DTYPES)
def test_ring_depth_does_not_change_an_image(dtype):
    """d1's layer at B = 1 and B = 42 on a 19x21 map: M = 399 runs the 4-stage ring, M = 16758 (132 workgroup columns) the
    2-stage one; image 0 must not notice."""
    q = dtype == "bf16"
    x, w, b, r = _inputs("d1", q, (42, 19, 21))
    y42, tag42 = _launch("d1", dtype, x, w, b, r)
    y1, tag1 = _launch("d1", dtype, np.ascontiguousarray(x[:1]), w, b, r)
    assert tag1 == _full_tag("wl<3,1,0,4>", dtype) and tag42 == _full_tag("wl<3,1,0,2>", dtype) and tag1 != tag42
    assert np.array_equal(y1[0], y42[0])
    _check_parity("d1", dtype, y1, np.ascontiguousarray(x[:1]), w, b, r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_n_blocks_per_wave_do_not_change_a_pixel(dtype):
    """b3's layer on a 13x17 map (one n-block per wave) and on 157x419 (four): the same values fed to pixels of both must give
    the same outputs (the K order of an output does not depend on NBW)."""
    q = dtype == "bf16"
    x, w, b, r = _inputs("b3", q)
    ybig, tagbig = _run("b3", dtype)
    xs = np.ascontiguousarray(x[:, :, :13, :17])
    ys, tags = _launch("b3", dtype, xs, w, b, r)
    assert tags == _full_tag("pw<1,0,0,false>", dtype) and tagbig == expected_tag("b3", dtype) and tags != tagbig
    assert np.array_equal(ys, ybig[:, :, :13, :17])
    _check_parity("b3", dtype, ys, xs, w, b, r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_k_split_layer_is_batch_invariant(dtype):
    """e1 (pw_ksplit_kernel in bf16: chosen by the layer's map, never by the batch) at B = 1 and B = 3."""
    q = dtype == "bf16"
    x, w, b, r = _inputs("e1", q, (3, 31, 34))
    y3, tag3 = _launch("e1", dtype, x, w, b, r)
    y1, tag1 = _launch("e1", dtype, np.ascontiguousarray(x[1:2]), w, b, np.ascontiguousarray(r[1:2]))
    assert tag1 == tag3 == expected_tag("e1", dtype)
    assert np.array_equal(y1[0], y3[1])
    _check_parity("e1", dtype, y3, x, w, b, r)


# ------------------------------------------------------------------------------- refusals
def test_unsupported_epilogues_and_widths_are_refused_loudly():
    """No instance exists for swish + residual, relu without bias, bias + residual; Cin / Cout must be multiples of 8.  Each is
    an error with a message, never a silently different computation, and leaves the next call intact."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 16, 5, 7)).astype(np.float32)
    w = rng.standard_normal((24, 16)).astype(np.float32)
    bias = rng.standard_normal(24).astype(np.float32)
    res = rng.standard_normal((1, 24, 5, 7)).astype(np.float32)
    refused = {
        "swish + residual": dict(x=x, w=w, act="swish", residual=res),
        "swish + residual (LDS-weights shape)": dict(x=rng.standard_normal((1, 64, 5, 7)).astype(np.float32),
                                                     w=rng.standard_normal((96, 64)).astype(np.float32), act="swish",
                                                     residual=rng.standard_normal((1, 96, 5, 7)).astype(np.float32)),
        "relu without bias": dict(x=x, w=w, act="relu"),
        "bias + residual": dict(x=x, w=w, bias=bias, residual=res),
        "Cin % 8": dict(x=x[:, :12], w=w[:, :12]),
        "Cout % 8": dict(x=x, w=w[:20]),
    }
    for dtype in DTYPES:
        for what, kw in refused.items():
            with pytest.raises(cfa._lib.CenterFaceError) as e:
                ops.conv_pw(dtype=dtype, **kw)
            assert str(e.value).strip() and e.value.code != 0, (what, dtype)
            # a valid call straight afterwards is unharmed
            y, tag = _launch("a1", dtype, *_inputs("a1", dtype == "bf16"))
            assert tag == expected_tag("a1", dtype), (what, dtype, tag)
            _check_parity("a1", dtype, y, *_inputs("a1", dtype == "bf16"))
