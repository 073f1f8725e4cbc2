"""Bit-identity of the back-half kernels whose loop bookkeeping was trimmed (profiles/r07_loop_overhead.md).

The trimmed kernels compute exactly what they computed before: only addresses, padding selects and register copies changed.  So
the check is not a tolerance but a digest: ``tests/golden/loop_overhead_digests.json`` holds, per case, the kernel tag and the
sha256 of the raw output bytes as the build BEFORE the change produced them on an MI355X (``record()`` below writes the file).
Every case first asserts which instance it reached (``ops.last_kernel()``), then the digest.

Cases:
  * each of the four ``expdw_mx_kernel`` instances on a 1 x 1 map, on one tile plus a row and a column, and on one tile minus one
    (B = 2, four rounds of hidden channels);
  * one Cin per JX class with an odd chunk count (56, 88, 152): the upper lane half's last chunk lies past the pixel's row.  The
    bytes there are the NEXT pixel's first eight channels (a row has no spare bytes to poison), so the second run writes NaN into
    channels 0-7 of every pixel of input column 0 -- the chunk the last pixel of each row over-reads.  Outputs out of the kernel's
    reach from column 0 may not move by a bit and may not turn NaN: the digest of those columns is the same in both runs, and is
    the recorded one.  The reach is the first output QUAD, x < 4: the matrix-core depthwise multiplies the eight inputs 4q - pad ..
    4q - pad + 7 of an output quad q by a banded matrix whose entries outside a pixel's k taps are zero, and 0 * NaN is NaN;
  * ``pw_wlds_kernel`` at M = 129 (a second workgroup with one live pixel block; B = 1, 3 x 43 -- 129 is odd) over the project
    shapes (K, N) of the late layers, with and without residual, row-major and pixel-block order, bf16 + one fp32 + one split case.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from centerface_amd import ops
import mbconv_cases as MC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_overhead_digests.json")

# instance -> (Cin of the JX class, odd-chunk Cin, k, tile h, tile w, short tag)
XMX = {
    "x40": (64, 56, 5, 10, 40, "expdw_mx_kernel<5,4,10,40,8,true>"),
    "x41": (96, 88, 5, 10, 40, "expdw_mx_kernel<5,6,10,40,8,true>"),
    "x51": (160, 152, 5, 20, 20, "expdw_mx_kernel<5,10,20,20,4,false>"),
    "x60": (160, 152, 3, 10, 20, "expdw_mx_kernel<3,10,10,20,4,true>"),
}
HID = 128                      # four rounds of 32 hidden channels; no Cin of the table (hid == Cin is refused)
PW_KN = ((384, 96), (576, 96), (576, 160), (960, 160), (960, 320))


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _xmx_inputs(name, Cin, k, H, W):
    rng = np.random.default_rng(int.from_bytes(("%s-%d-%d-%d" % (name, Cin, H, W)).encode(), "little") % (1 << 63))
    we, wd, _ = MC.weights(rng, Cin, HID, 0, k)
    x = rng.standard_normal((2, Cin, H, W)).astype(np.float32)
    return x, we, wd


def _xmx_maps(name):
    th, tw = XMX[name][3:5]
    return {"one": (1, 1), "plus": (th + 1, tw + 1), "minus": (th - 1, tw - 1)}


def _run_xmx(name, mp):
    Cin, _, k = XMX[name][:3]
    H, W = _xmx_maps(name)[mp]
    x, we, wd = _xmx_inputs(name, Cin, k, H, W)
    y = ops.expand_dw(x, we, wd, k, 1, dtype="bf16")
    return ops.last_kernel(), {"all": _digest(y)}


def _run_odd(name):
    _, Cin, k = XMX[name][:3]
    H, W = _xmx_maps(name)["plus"]
    x, we, wd = _xmx_inputs(name, Cin, k, H, W)
    y = ops.expand_dw(x, we, wd, k, 1, dtype="bf16")
    tag = ops.last_kernel()
    xn = x.copy()
    xn[:, :8, :, 0] = np.nan
    yn = ops.expand_dw(xn, we, wd, k, 1, dtype="bf16")
    assert ops.last_kernel() == tag
    far = 4                                                  # first output column whose quad's input window misses column 0
    return tag, {"all": _digest(y), "far": _digest(y[..., far:]), "far_nan": _digest(yn[..., far:]),
                 "finite": bool(np.isfinite(y).all() and np.isfinite(yn[..., far:]).all())}


def _run_pw(K, N, res, dtype, layout):
    rng = np.random.default_rng(K * 1000 + N)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    x = rng.standard_normal((1, K, 3, 43)).astype(np.float32)
    r = rng.standard_normal((1, N, 3, 43)).astype(np.float32) if res else None
    y = ops.conv_pw(x, w, residual=r, dtype=dtype, layout=layout)
    return ops.last_kernel(), {"all": _digest(y)}


def _cases():
    out = {}
    for name in XMX:
        for mp in ("one", "plus", "minus"):
            out["%s-%s" % (name, mp)] = (_run_xmx, (name, mp))
        out["%s-odd" % name] = (_run_odd, (name,))
    for K, N in PW_KN:
        for res in (0, 1):
            for layout in (0, 0b111 if res else 0b011):
                out["pw-%d-%d-r%d-bf16-l%d" % (K, N, res, layout)] = (_run_pw, (K, N, res, "bf16", layout))
    out["pw-576-96-r1-fp32-l0"] = (_run_pw, (576, 96, 1, "fp32", 0))
    out["pw-960-160-r0-fp32_split-l0"] = (_run_pw, (960, 160, 0, "fp32_split", 0))
    out["pw-960-160-r1-fp32_split-l7"] = (_run_pw, (960, 160, 1, "fp32_split", 0b111))
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


def test_every_case_is_recorded():
    assert sorted(_golden()) == sorted(CASES)


@pytest.mark.parametrize("cid", list(CASES))
def test_bits_unchanged(cid):
    want = _golden()[cid]
    fn, args = CASES[cid]
    tag, dig = fn(*args)
    if cid.startswith("x"):
        assert tag == MC.full_tag(XMX[cid[:3]][5], "bf16"), (cid, tag)
    else:
        assert tag.startswith("void cf::pw_wlds_kernel<"), (cid, tag)
    assert tag == want["kernel"], (cid, tag, want["kernel"])
    if "far" in dig:
        assert dig["finite"], "%s: NaN past a pixel's row reached an output it has no tap on" % cid
        assert dig["far_nan"] == dig["far"], "%s: the chunk past a pixel's row moved outputs it has no tap on" % cid
    assert dig == want["sha256"], (cid, dig, want["sha256"])
