"""Bit-identity of the three front-half kernels whose expand phase deals halo rows to waves by row pair (profiles/r10_halo_deal.md).

Only WHO computes which cell of the expanded halo changed: an expand value does not depend on the MFMA row it is computed in, and the
Swish, the fp16 rounding, the cell contents, the depthwise, the project and every rounding point are where they were.  Halo columns 18
and 19 of the 3x3 kernels, which meet only zero entries of the Toeplitz operand, changed from finite values to zeros: a sum that
starts at +0 does not move by that.  So the check is a digest, as in tests/test_front_overhead.py:
``tests/golden/halo_deal_digests.json`` holds, per case, the kernel tag and the sha256 of the raw output bytes as the build BEFORE the
change produced them on an MI355X (``record()`` below writes the file; pytest does not run it).  Every case first asserts which
instance it reached, then the digest.  All cases are bf16, B = 2.  The tag does not carry the MODE parameter; every tensor here is far
below the sizes at which the launchers fall back to the general kernels, so the release library runs the new deal in all of them.
The other forms are held to the same digests through the experiments build, whose launchers read ``CF_FRONT_MODE`` (2: the kernels
as they were before this deal, 0: the general kernels):
``make -C <csrc> EXP=1 && CF_LIB=<...>/libcenterface_hip_exp.so CF_FRONT_MODE=2 pytest tests/test_halo_deal.py``
(profiles/r10_halo_deal.md records those runs and the kernel names their traces show).

Cases:
  * ``ops.mbconv`` with the block shapes of layer1.1 (24 -> 144 -> 24, k3, residual) and layer2.1 (32 -> 192 -> 32, k5, residual) on
    maps of 1 x 1, 15 x 15 (one tile minus one), 16 x 16 (one whole tile), 17 x 17 (a second tile row and column of one pixel), 16 x 33
    (three tiles in x, the last one pixel wide) and 35 x 35 (3 x 3 tiles whose middle tile has its whole halo inside the map);
  * the fused stem (``stem0_mx_kernel``) through plan entry 0 of a bf16 engine (``Engine.trace(x, 0)``) at 32 x 32, 64 x 64 and
    96 x 96, uint8 and float input;
  * LDS leftovers, one case per kernel.  A cell half that the expand phase leaves unwritten keeps what the workgroup before it left
    in LDS, the depthwise multiplies it by a zero weight, and 0 * NaN is NaN.  So the same op first runs on an input that is NaN
    everywhere (its output is NaN, nothing else happens: the tiles it leaves in LDS are NaN patterns), then on the finite input, in
    the same process: that output must be finite and must have the recorded digest.  The stem is poisoned through its float instance
    (a uint8 image has no NaN) and then checked in both formats.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
import mbconv_cases as MC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "halo_deal_digests.json")

# block -> (Cin, hid, Cout, k, the benchmarked instance)
BLOCKS = {
    "l11": (24, 144, 24, 3, "mbconv_mx_kernel<3,2,2,true,16,16,4,true,false,true,false>"),
    "l21": (32, 192, 32, 5, "mbconv_mx_kernel<5,2,2,true,16,16,4,false,false,true,false>"),
}
MAPS = ((1, 1), (15, 15), (16, 16), (17, 17), (16, 33), (35, 35))
LEFT_MAP = (35, 35)
STEM_TAG = "void cf::stem0_mx_kernel<%d>(cf::Stem0Params)"
STEM_SIZES = (32, 64, 96)
LEFT_SIZE = 96


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _mb_inputs(blk, H, W):
    Cin, hid, Cout, k = BLOCKS[blk][:4]
    rng = np.random.default_rng(int.from_bytes(("halo-%s-%d-%d" % (blk, H, W)).encode(), "little") % (1 << 63))
    we, wd, wp = MC.weights(rng, Cin, hid, Cout, k)
    x = rng.standard_normal((2, Cin, H, W)).astype(np.float32)
    return x, we, wd, wp


def _run_mb(blk, H, W, poison=False):
    k = BLOCKS[blk][3]
    x, we, wd, wp = _mb_inputs(blk, H, W)
    if poison:
        yn = ops.mbconv(np.full_like(x, np.nan), we, wd, wp, k, 1, dtype="bf16")
        assert np.isnan(yn).all()
    y = ops.mbconv(x, we, wd, wp, k, 1, dtype="bf16")
    assert y.shape == (2, BLOCKS[blk][2], H, W)
    return ops.last_kernel(), {"all": _digest(y), "finite": bool(np.isfinite(y).all())}


_SD = []


def _stem(fmt, size, x=None):
    if not _SD:
        _SD.append(cfa.weights.synthetic_state_dict(0))
    if x is None:
        rng = np.random.default_rng(2000 * size + (7 if fmt == "u8" else 11))
        if fmt == "u8":
            x = rng.integers(0, 256, (2, size, size, 3), dtype=np.uint8)
        else:
            x = rng.standard_normal((2, 3, size, size)).astype(np.float32)
    eng = cfa.Engine(size, size, max_batch=2, dtype="bf16", device=0, weights=_SD[0])
    try:
        assert eng.plan()[0]["name"] == "first_conv+layer0.0"
        y = eng.trace(x, 0)
        tag = ops.last_kernel()
    finally:
        eng.close()
    assert y.shape == (2, 16, size // 2, size // 2)
    return tag, y


def _run_stem(fmt, size):
    tag, y = _stem(fmt, size)
    return tag, {"all": _digest(y), "finite": bool(np.isfinite(y).all())}


def _run_stem_left(size):
    _, yn = _stem("f32", size, np.full((2, 3, size, size), np.nan, np.float32))
    assert np.isnan(yn).all()
    tag8, y8 = _stem("u8", size)
    tagf, yf = _stem("f32", size)
    assert tagf == STEM_TAG % cfa._lib.CF_IN_F32_NCHW, tagf
    return tag8, {"all": _digest(y8), "f32": _digest(yf), "finite": bool(np.isfinite(y8).all() and np.isfinite(yf).all())}


def _cases():
    out = {}
    for blk in BLOCKS:
        for H, W in MAPS:
            out["%s-%dx%d" % (blk, H, W)] = (_run_mb, (blk, H, W))
        out["%s-left" % blk] = (_run_mb, (blk,) + LEFT_MAP + (True,))
    for fmt in ("u8", "f32"):
        for size in STEM_SIZES:
            out["stem-%s-%d" % (fmt, size)] = (_run_stem, (fmt, size))
    out["stem-u8-left"] = (_run_stem_left, (LEFT_SIZE,))
    return out


CASES = _cases()


def record(path=GOLDEN):
    """Write the digest file from the library that is loaded (run once, with the build before a kernel change)."""
    rec = {}
    for cid, (fn, args) in CASES.items():
        try:
            tag, dig = fn(*args)
        except Exception as e:                               # keep going: the file then lacks the case and the test says so
            print(cid, "FAILED", repr(e))
            continue
        rec[cid] = {"kernel": tag, "sha256": dig}
        print(cid, tag, dig)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    return rec


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _want_tag(cid):
    if cid.startswith("stem"):
        return STEM_TAG % (cfa._lib.CF_IN_U8_HWC_BGR if cid.startswith("stem-u8") else cfa._lib.CF_IN_F32_NCHW)
    return MC.full_tag(BLOCKS[cid[:3]][4], "bf16")


def test_every_case_is_recorded():
    assert sorted(_golden()) == sorted(CASES)


def test_leftover_cases_share_the_plain_digests():
    """The poisoned cases run the inputs of a plain case: the file must say the same bytes for both."""
    g = _golden()
    for blk in BLOCKS:
        assert g["%s-left" % blk]["sha256"]["all"] == g["%s-%dx%d" % ((blk,) + LEFT_MAP)]["sha256"]["all"]
    assert g["stem-u8-left"]["sha256"]["all"] == g["stem-u8-%d" % LEFT_SIZE]["sha256"]["all"]
    assert g["stem-u8-left"]["sha256"]["f32"] == g["stem-f32-%d" % LEFT_SIZE]["sha256"]["all"]


@pytest.mark.parametrize("cid", list(CASES))
def test_bits_unchanged(cid):
    want = _golden()[cid]
    fn, args = CASES[cid]
    tag, dig = fn(*args)
    assert tag == _want_tag(cid), (cid, tag)
    assert tag == want["kernel"], (cid, tag, want["kernel"])
    assert dig["finite"], "%s: a NaN reached the output (a cell the depthwise reads under a zero weight was left unwritten?)" % cid
    assert dig == want["sha256"], (cid, dig, want["sha256"])
