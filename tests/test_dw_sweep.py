"""Every standalone depthwise kernel instance the release picker hands out, over the class of shapes its table row accepts.

``launch_dw`` (csrc/cf_dw.hip) serves layers 4.0 - 6.0 of the exact fp32 plan, every block of the ``fuse=False`` plans, the
ShuffleV2 block and ``cf_op_dwconv`` from eleven ``(k, s, TH, TW)`` instances -- six of dw_strip_kernel (stride 1), five of
dw_lds_kernel (stride 2, times act x bias) -- each in float and bf16 storage, picked by output width (and height, for the late
stride-2 maps).  Behind an instance, host-computed geometry decides how a tile is staged: the channel chunk (the largest divisor of
C in whole 16-byte groups that the LDS budget holds), the 16-byte groups per pixel, the workgroup size of the strip kernel (64 -
256 threads) and its staging step, the XCD-contiguous work list.  The table (tests/dw_cases.py, kept honest against
``ops.dw_pick`` by tests/test_dw_cases.py, no GPU needed) visits each of those per instance and storage type on the smallest
maps at which the edge logic is live, and stands on both sides of every class boundary.

Every case FIRST asserts the instance it reached (``ops.last_kernel()``), then that the output is finite (``cf_op_dwconv`` fills
y with 0xFF bytes before the launch: a skipped store IS a NaN), then parity with the project's own references and bounds:
  * fp32: ``dw_cases.ref64`` (float64; tied to the oracle on the production shapes by tests/test_dw_cases.py) at rtol = atol =
    2e-5 (tests/test_gpu_parity.py's F32), every element;
  * fp32_split (one case per instance): the same float kernel -- bit-equal to the fp32 result;
  * bf16: ``E.dw_op`` (fp32 taps, fp32 accumulate, one bf16 rounding at the store) under ``E.tolerance`` / ``E.accept``, as
    tests/test_gpu_parity.py::_emu_close;
each on the whole tensor, the first and last output row, the first and last output column and the channels of the last chunk, so
that a failure names the edge.

The experiments build is not swept (``CF_DW_TILE`` / ``CF_DW_CAP`` / ``CF_DW_WGS``, the band and marching kernels): the release
library does not contain those paths.  Measured ratios: profiles/dw_sweep_parity.md.
"""
import functools

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from oracle import bf16_emulation as E

import dw_cases as D

pytestmark = pytest.mark.gpu

F32 = dict(rtol=2e-5, atol=2e-5)          # tests/test_gpu_parity.py


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    """(x, w, bias) of a case (shared between the tests: never written to)."""
    return D.inputs(cid)


def _launch(cid, dtype=None):
    _, cdtype, C, H, W, k, s, pad, act, bias, B = D.case(cid)[:11]
    x, w, b = _inputs(cid)
    y = ops.conv_dw(x, w, k, s, pad=D.pads(k, s, pad), act=act, bias=b, dtype=dtype or cdtype)
    return y, ops.last_kernel()


def _reference(cid):
    _, dtype, C, H, W, k, s, pad, act, bias, B = D.case(cid)[:11]
    x, w, b = _inputs(cid)
    if dtype != "bf16":
        return D.ref64(x, w, k, s, D.pads(k, s, pad), act, b)
    return E.dw_op(x, w, k, s, D.pads(k, s, pad), act, b).numpy().astype(np.float64)


def _check_parity(cid, y, ref):
    """Worst |d| / bound of the case, after asserting it on the whole tensor and on each edge."""
    dtype, Cc = D.case(cid)[1], D.case(cid)[12]
    bad = ~np.isfinite(y)
    assert not bad.any(), "%s %s: %d of %d outputs are not finite, first at (b, c, y, x) = %s" % (cid, dtype, int(bad.sum()), y.size, np.argwhere(bad)[0])
    assert y.shape == ref.shape, (cid, y.shape, ref.shape)
    d = np.abs(y.astype(np.float64) - ref)
    ratio = d / (F32["atol"] + F32["rtol"] * np.abs(ref)) if dtype != "bf16" else d / E.tolerance(ref)
    print("DWSWEEP %s %.4f %s differing %.2e" % (cid, float(ratio.max()), ops.last_kernel().split("(")[0].replace("void cf::", ""), float((d > 0).mean())))
    for what, part in D.edges(ratio, Cc):
        at = np.unravel_index(part.argmax(), part.shape)
        if dtype != "bf16":
            assert part.max() <= 1.0, "%s %s, %s: |d| / (atol + rtol |ref|) = %.3f at %s of the slice" % (cid, dtype, what, part.max(), at)
        else:
            stat = (float(part.max()), float((part > 1).mean()), float((part > 0.5).mean()), float((part > 0).mean()))
            assert E.accept(stat, True, part.size), "%s bf16, %s: max |d|/tol %.2f at %s, frac > tol %.1e, > tol/2 %.1e, differing %.1e (n = %d)" % (
                (cid, what, stat[0], at) + stat[1:] + (part.size,))
    return float(ratio.max())


# ------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("cid", D.IDS)
def test_instance_reached_and_parity(cid):
    c = D.case(cid)
    y, tag = _launch(cid)
    assert tag == D.full_tag(c[11], c[1], c[8], c[9]), (cid, tag)
    _check_parity(cid, y, _reference(cid))


@pytest.mark.parametrize("cid", D.SPLIT_CASES)
def test_fp32_split_takes_the_fp32_kernel_bit_for_bit(cid):
    c = D.case(cid)
    y, tag = _launch(cid)
    ys, tags = _launch(cid, "fp32_split")
    assert tag == tags == D.full_tag(c[11], "fp32", c[8], c[9]), (cid, tag, tags)
    assert np.isfinite(y).all() and np.isfinite(ys).all()
    assert np.array_equal(y, ys), (cid, int((y != ys).sum()), np.argwhere(y != ys)[:3])


# ------------------------------------------------------------------------------- refusals
def test_refused_shapes_are_refused_with_a_gpu_present_too():
    """The GPU-less form (every refusal, output untouched) is tests/test_dw_cases.py; here: the same refusals with a GPU present,
    and a valid call straight afterwards is unharmed."""
    for what, (dtype, C, H, W, k, s, pad) in D.REFUSED.items():
        assert not ops.dw_pick(C, H, W, k, s, pad=pad, dtype=dtype)["ok"], what
        with pytest.raises(cfa._lib.CenterFaceValueError):
            ops.conv_dw(np.ones((1, C, H, W), np.float32), np.ones((C, 1, k, k), np.float32), k, s, pad=pad, dtype=dtype)
    y, tag = _launch("Cb-row")
    assert tag == D.full_tag("strip<3,1,10,20>", "bf16", "swish", False)
    _check_parity("Cb-row", y, _reference("Cb-row"))
