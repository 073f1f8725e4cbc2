"""Every fused-MBConv / expand+depthwise kernel instance, over the class of block shapes its table row accepts.

``mb_geometry`` / ``expdw_geometry`` pick a table row by (k, stride, JX, n-blocks, residual[, tail]) and then only require
``hid % HC == 0``, so each of the nine families (csrc/cf_mbconv.hip ... cf_mbconv6.hip) serves far more than the eight production
block shapes the rest of the suite runs: two Cin per JX class in bf16 (the lower one leaves the upper lane half a chunk short),
every Cout of an n-block count, any number of hidden chunks (one; none but the 16-channel tail; one more than a workgroup of
expdw_f32_kernel takes), and -- where a family's HC does not divide hid -- the family behind it.  The table (tests/mbconv_cases.py,
kept honest against the geometry functions by tests/test_abi.py, no GPU needed) visits each of those per row, on the smallest maps
at which the tile-edge and clamp logic is live: 1x1, one column taller than a tile, a tile - 1, a tile + 1 (four tiles), odd
stride-2 inputs; B = 2.

Every case FIRST asserts the instance it reached (``ops.last_kernel()``), so a retuned table cannot silently move it, then that
the output is finite (the per-op path fills y and the pad behind every buffer with 0xFF bytes: a skipped store or a read past a
buffer IS a NaN), then parity with the project's own references and bounds:
  * fp32 / fp32_split: ``mbconv_cases.ref64`` (float64, tied to the oracle on the production shapes by tests/test_abi.py) at
    rtol = atol = 1e-4, what the fused-MBConv tests of tests/test_gpu_parity.py hold both modes to;
  * bf16: ``E.mbconv_fused`` / ``E.expand_dw(out_scaled=False)`` under ``E.tolerance`` / ``E.accept``, as
    tests/test_bf16_parity.py::_assert_close;
each on the whole tensor, the last output row, the last output column and the last 8 output channels, so that an edge is named.
Sixteen bf16 cases (rows b2t / b3t / b4t / b4u) assert a refusal instead: their hid is divided only by the HC of cf_mbconv.hip's
own bf16 instances, which this sweep measured 1.1 - 4.7 bounds off the emulation (other rounding points) and which ``mb_geometry``
no longer hands out; a few more are refused under a product switch (the table's last column).
Measured ratios: profiles/mbconv_sweep_parity.md.
"""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import centerface_amd as cfa
from centerface_amd import ops
from oracle import bf16_emulation as E

import mbconv_cases as M

pytestmark = pytest.mark.gpu

EXACT_TOL = dict(rtol=1e-4, atol=1e-4)      # fp32 and fp32_split fused blocks (tests/test_gpu_parity.py)


def _seed(cid):
    return int.from_bytes(cid.encode(), "little")


@functools.lru_cache(maxsize=None)
def _inputs(cid, B=2):
    """(x, we, wd, wp) of a case, seeded from its id (shared between the tests: never written to)."""
    _, dtype, Cin, hid, Cout, k, s, H, W = M.case(cid)[:9]
    rng = np.random.default_rng(_seed(cid))
    we, wd, wp = M.weights(rng, Cin, hid, Cout, k)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    if dtype == "bf16":
        x = E.q_bf16(torch.from_numpy(x)).numpy()
    return x, we, wd, wp


def _launch(cid, x, we, wd, wp):
    _, dtype, Cin, hid, Cout, k, s = M.case(cid)[:7]
    y = ops.expand_dw(x, we, wd, k, s, dtype=dtype) if Cout == 0 else ops.mbconv(x, we, wd, wp, k, s, dtype=dtype)
    return y, ops.last_kernel()


def _reference(cid, x, we, wd, wp):
    _, dtype, Cin, hid, Cout, k, s = M.case(cid)[:7]
    if dtype != "bf16":
        return M.ref64(x, we, wd, wp, k, s)
    xt = torch.from_numpy(x)
    ref = E.expand_dw(xt, we, wd, k, s, out_scaled=False) if Cout == 0 else E.mbconv_fused(xt, we, wd, wp, k, s, Cin == Cout and s == 1)
    return ref.numpy().astype(np.float64)


def _check_parity(cid, y, ref):
    """Worst |d| / bound of the case, after asserting it on the whole tensor and on each edge."""
    dtype = M.case(cid)[1]
    bad = ~np.isfinite(y)
    assert not bad.any(), "%s %s: %d of %d outputs are not finite, first at (b, c, y, x) = %s" % (cid, dtype, int(bad.sum()), y.size, np.argwhere(bad)[0])
    assert y.shape == ref.shape, (cid, y.shape, ref.shape)
    d = np.abs(y.astype(np.float64) - ref)
    ratio = d / (EXACT_TOL["atol"] + EXACT_TOL["rtol"] * np.abs(ref)) if dtype != "bf16" else d / E.tolerance(ref)
    parts = (("whole tensor", ratio), ("last output row", ratio[:, :, -1:, :]), ("last output column", ratio[:, :, :, -1:]),
             ("last 8 output channels", ratio[:, -8:]))
    print("MBSWEEP %s %s %s %.4f differing %.2e" % (cid, dtype, ops.last_kernel().split("(")[0].replace("void cf::", ""), float(ratio.max()), float((d > 0).mean())))
    for what, part in parts:
        at = np.unravel_index(part.argmax(), part.shape)
        if dtype != "bf16":
            assert part.max() <= 1.0, "%s %s, %s: |d| / (atol + rtol |ref|) = %.3f at %s of the slice" % (cid, dtype, what, part.max(), at)
        else:
            stat = (float(part.max()), float((part > 1).mean()), float((part > 0.5).mean()), float((part > 0).mean()))
            assert E.accept(stat, True, part.size), "%s bf16, %s: max |d|/tol %.2f at %s, frac > tol %.1e, > tol/2 %.1e, differing %.1e (n = %d)" % (
                (cid, what, stat[0], at) + stat[1:] + (part.size,))
    return float(ratio.max())


# ------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("cid", M.IDS, ids=["%s-%s" % (c[1], c[0]) for c in M.CASES])
def test_variant_reached_and_parity(cid):
    c = M.case(cid)
    short = M.short_tag(c, os.environ)
    x, we, wd, wp = _inputs(cid)
    if short == "REFUSED":          # under the dtype's product switch no family serves this shape: loud, before any launch
        assert c[4] != 0 and not ops.mbconv_pick(c[2], c[3], c[4], c[5], c[6], c[1])["ok"]
        with pytest.raises(cfa._lib.CenterFaceValueError):
            _launch(cid, x, we, wd, wp)
        return
    y, tag = _launch(cid, x, we, wd, wp)
    assert tag == M.full_tag(short, c[1]), (cid, tag)
    _check_parity(cid, y, _reference(cid, x, we, wd, wp))


# ------------------------------------------------------------------------------- batch invariance
# one case per family, on its tile + 1 map (four workgroups per image)
FAMILY_CASES = {"MB_TILE": "f40d", "MB_PX": "b30d", "XD_PX": "y50d", "XD_MX": "y41d", "MB_MX": "b21d", "MB_MX2": "b20d", "MB_F32": "s11d",
                "XD_F32": "x50d", "MB_SP": "s2sd"}


@pytest.mark.parametrize("fam", list(FAMILY_CASES))
def test_batch_index_does_not_change_an_image(fam):
    """The same image at batch index 0 and at index 1 of a B = 2 call, and alone: three bit-identical outputs."""
    cid = FAMILY_CASES[fam]
    c = M.case(cid)
    x, we, wd, wp = _inputs(cid)
    x1 = np.ascontiguousarray(x[1:2])
    x2 = np.ascontiguousarray(np.concatenate([x1, x1]))
    y2, tag2 = _launch(cid, x2, we, wd, wp)
    y1, tag1 = _launch(cid, x1, we, wd, wp)
    assert tag1 == tag2 == M.full_tag(M.short_tag(c, os.environ), c[1]) and M.family(M.short_tag(c, os.environ)) == fam
    assert np.isfinite(y2).all() and np.isfinite(y1).all()
    assert np.array_equal(y2[0], y2[1]), (cid, int((y2[0] != y2[1]).sum()), np.argwhere(y2[0] != y2[1])[:3])
    assert np.array_equal(y1[0], y2[0]), (cid, int((y1[0] != y2[0]).sum()), np.argwhere(y1[0] != y2[0])[:3])


# ------------------------------------------------------------------------------- the product switches
# Seconds one child took on an MI355X, rounded up (4.5 and 4.4: profiles/mbconv_sweep_parity.md); the timeout is three times that.
CHILD_SECONDS = {"CF_DW_MATRIX": 5, "CF_F4_VARIANT": 5}


@pytest.mark.parametrize("name,value,select", [("CF_DW_MATRIX", "0", "bf16"), ("CF_F4_VARIANT", "1", "fp32")],
                         ids=["CF_DW_MATRIX=0", "CF_F4_VARIANT=1"])
def test_product_switches_keep_the_sweep(name, value, select):
    """``CF_DW_MATRIX=0`` puts every bf16 block on the v_dot2c family (mbconv_px_kernel / expdw_px_kernel), ``CF_F4_VARIANT=1``
    every fp32 block on mbconv_f32_kernel.  Both are read once per process: the sweep's cases of the storage types the switch
    governs run again in one child process with it set, each against the instance the table's last column names for it."""
    want = sum(1 for c in M.CASES if c[1].startswith(select))
    moved = sum(1 for c in M.CASES if c[1].startswith(select) and c[10] is not None)
    assert moved >= 20                                      # the switch is what the child is about
    env = dict(os.environ)
    env[name] = value
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_variant_reached_and_parity and %s" % select],
                       env=env, capture_output=True, text=True, timeout=3 * CHILD_SECONDS[name])
    print("MBSWEEP child %s=%s: %.1f s" % (name, value, time.time() - t0))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "%d passed" % want in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]


# ------------------------------------------------------------------------------- refusals
def test_shapes_no_family_serves_are_refused_loudly():
    """The GPU-less form (every refusal, output untouched) is tests/test_abi.py::test_mbconv_refusals_need_no_gpu; here: the
    same refusals with a GPU present, and a valid call straight afterwards is unharmed."""
    rng = np.random.default_rng(0)
    for what, (dtype, Cin, hid, Cout, k, s) in M.REFUSED.items():
        x = rng.standard_normal((1, Cin, 5, 6)).astype(np.float32)
        we, wd, wp = M.weights(rng, Cin, hid, Cout, k)
        with pytest.raises(cfa._lib.CenterFaceValueError):
            ops.expand_dw(x, we, wd, k, s, dtype=dtype) if Cout == 0 else ops.mbconv(x, we, wd, wp, k, s, dtype=dtype)
    y, tag = _launch("b10a", *_inputs("b10a"))
    assert tag == M.full_tag(M.short_tag(M.case("b10a"), os.environ), "bf16")
    _check_parity("b10a", y, _reference("b10a", *_inputs("b10a")))
