"""Bit-identity of the front-half kernels whose address, padding and epilogue bookkeeping was trimmed (profiles/r09_front_overhead.md).

Only instructions around the round loops changed (coordinates from tables, 32-bit offsets, zero padding by address): every MFMA, every
Swish and every rounding point is where it was.  So the check is a digest, as in tests/test_loop_overhead.py:
``tests/golden/front_overhead_digests.json`` holds, per case, the kernel tag and the sha256 of the raw output bytes as the build BEFORE
the change produced them on an MI355X (``record()`` below writes the file; pytest does not run it).  Every case first asserts which
instance it reached, then the digest.  All cases are bf16, B = 2.

The tag does not carry the MODE parameter (as for ``expdw_mx_kernel``), and every tensor here is below 2 GiB: in the release library
these cases run the MODE 3 / MODE 1 instances, never the general ones.  The general kernels are held to the same digests through the
experiments build, whose launchers read ``CF_FRONT_MODE``:
``make -C <csrc> EXP=1 && CF_LIB=<...>/libcenterface_hip_exp.so CF_FRONT_MODE=0 pytest tests/test_front_overhead.py``
(profiles/r09_front_overhead.md records that run and the kernel names a trace of it shows).

Cases:
  * ``ops.mbconv`` with the block shapes of layer1.0 (16 -> 96 -> 24, k3 s2), layer1.1 (24 -> 144 -> 24, k3 s1, residual) and layer2.0
    (24 -> 144 -> 32, k5 s2: the network's layer2.0 and the widest output the benchmarked instance, one n-block, serves; Cout = 40 is
    refused for this block shape), each on an output map of 1 x 1, one tile minus one, one tile plus a row and a column, and 3 x 3 tiles whose
    middle tile's whole halo (the quad-padded columns included) lies inside the input, so that the padded and the unpadded load path
    both run;
  * for the two Cin = 24 blocks the NaN-poison case of tests/test_loop_overhead.py: a lane of the upper half reads chunks 2 and 3 of
    its pixel, and chunk 3 (channels 24-31) lies past the pixel's row -- it is the NEXT pixel's channels 0-7.  The second run writes NaN
    into channels 0-7 of every pixel of input column 0 (what the last pixel of each row over-reads).  Outputs out of the depthwise
    window's reach from column 0 may not move by a bit and may not turn NaN.  The reach is the first output QUAD, x < 4, for both
    blocks: the matrix-core depthwise multiplies all inputs of an output quad's window by a banded matrix whose entries outside a
    pixel's k taps are zero, and 0 * NaN is NaN.  Stride 1, k = 3 (pad 1 in front): quad q reads inputs 4q - 1 .. 4q + 6; stride 2,
    k = 5 (pad 1 in front): quad q reads the three input quads 2q .. 2q + 2 of the halo = inputs 8q - 1 .. 8q + 10.  Column 0 is in
    quad 0's window only;
  * the fused stem (first_conv + layer0.0, ``stem0_mx_kernel``) in both input formats it is instantiated for.  ``ops.stem`` launches
    the unfused first_conv kernel, so the stem is reached the way the engine reaches it: plan entry 0 of a bf16 engine
    (``Engine.trace(x, 0)``).  Inputs 32 x 32 (one tile, every edge), 64 x 64 (four corner tiles) and 96 x 96 (one interior tile:
    ``interior`` and ``halo_inside`` both true).
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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "front_overhead_digests.json")

# block -> (Cin, hid, Cout, k, stride, tile h, tile w, the benchmarked instance)
BLOCKS = {
    "l10": (16, 96, 24, 3, 2, 8, 16, "mbconv_px_kernel<3,2,1,false,4,1,32,8,16>"),
    "l11": (24, 144, 24, 3, 1, 16, 16, "mbconv_mx_kernel<3,2,2,true,16,16,4,true,false,true,false>"),
    "l20": (24, 144, 32, 5, 2, 8, 16, "mbconv_mx2_kernel<5,2,2,8,16,true,false,false>"),
}
STEM_TAG = "void cf::stem0_mx_kernel<%d>(cf::Stem0Params)"
STEM_SIZES = (32, 64, 96)
FAR = 4                        # first output column out of input column 0's reach (module docstring)


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _in_size(blk, mp):
    """Input (H, W) of a map case: stride-2 blocks alternate even and odd input sizes."""
    _, _, _, k, s, th, tw, _ = BLOCKS[blk]
    if s == 1:
        return {"one": (1, 1), "minus": (th - 1, tw - 1), "plus": (th + 1, tw + 1), "tiles": (2 * th + 3, 2 * tw + 3)}[mp]
    return {"one": (2, 3), "minus": (2 * (th - 1), 2 * (tw - 1)), "plus": (2 * (th + 1) + 1, 2 * (tw + 1) + 1),
            "tiles": (2 * (2 * th + 1) + 1, 2 * (2 * tw + 1) + 1)}[mp]


def _mb_inputs(blk, H, W):
    Cin, hid, Cout, k = BLOCKS[blk][:4]
    rng = np.random.default_rng(int.from_bytes(("%s-%d-%d" % (blk, H, W)).encode(), "little") % (1 << 63))
    we, wd, wp = MC.weights(rng, Cin, hid, Cout, k)
    x = rng.standard_normal((2, Cin, H, W)).astype(np.float32)
    return x, we, wd, wp


def _run_mb(blk, mp):
    k, s = BLOCKS[blk][3:5]
    H, W = _in_size(blk, mp)
    x, we, wd, wp = _mb_inputs(blk, H, W)
    y = ops.mbconv(x, we, wd, wp, k, s, dtype="bf16")
    assert y.shape[2:] == tuple(MC.out_size(n, k, s) for n in (H, W))
    return ops.last_kernel(), {"all": _digest(y)}


def _run_nan(blk):
    k, s = BLOCKS[blk][3:5]
    H, W = _in_size(blk, "plus")
    x, we, wd, wp = _mb_inputs(blk, H, W)
    y = ops.mbconv(x, we, wd, wp, k, s, dtype="bf16")
    tag = ops.last_kernel()
    xn = x.copy()
    xn[:, :8, :, 0] = np.nan
    yn = ops.mbconv(xn, we, wd, wp, k, s, dtype="bf16")
    assert ops.last_kernel() == tag
    return tag, {"all": _digest(y), "far": _digest(y[..., FAR:]), "far_nan": _digest(yn[..., FAR:]),
                 "finite": bool(np.isfinite(y).all() and np.isfinite(yn[..., FAR:]).all())}


_SD = []


def _run_stem(fmt, size):
    if not _SD:
        _SD.append(cfa.weights.synthetic_state_dict(0))
    rng = np.random.default_rng(1000 * size + (7 if fmt == "u8" else 11))
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
    return tag, {"all": _digest(y)}


def _cases():
    out = {}
    for blk in BLOCKS:
        for mp in ("one", "minus", "plus", "tiles"):
            out["%s-%s" % (blk, mp)] = (_run_mb, (blk, mp))
        if BLOCKS[blk][0] == 24:
            out["%s-nan" % blk] = (_run_nan, (blk,))
    for fmt in ("u8", "f32"):
        for size in STEM_SIZES:
            out["stem-%s-%d" % (fmt, size)] = (_run_stem, (fmt, size))
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
    return MC.full_tag(BLOCKS[cid[:3]][7], "bf16")


def test_every_case_is_recorded():
    assert sorted(_golden()) == sorted(CASES)


@pytest.mark.parametrize("cid", list(CASES))
def test_bits_unchanged(cid):
    want = _golden()[cid]
    fn, args = CASES[cid]
    tag, dig = fn(*args)
    assert tag == _want_tag(cid), (cid, tag)
    assert tag == want["kernel"], (cid, tag, want["kernel"])
    if "far" in dig:
        assert dig["finite"], "%s: NaN past a pixel's row reached an output it has no tap on" % cid
        assert dig["far_nan"] == dig["far"], "%s: the chunk past a pixel's row moved outputs it has no tap on" % cid
    assert dig == want["sha256"], (cid, dig, want["sha256"])
