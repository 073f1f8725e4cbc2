"""Bit-identity of the matrix-core MBConv kernels across the move to one device vocabulary (csrc/cf_mx.h, profiles/mx_vocab_refactor.md).

The refactor rewrote ``expdw_mx_kernel``, ``mbconv_mx_kernel`` and ``mbconv_mx2_kernel`` (csrc/cf_mbconv3.hip) over shared device
blocks; no rounding point, no summation order and no cell moved, so the check is a digest, built like tests/test_halo_deal.py:
``tests/golden/mx_vocab_digests.json`` holds, per case, the kernel tag and the sha256 of the raw output bytes as the library of the commit
BEFORE the refactor produced them on an MI355X (``record()`` below writes the file from whatever library ``CF_LIB`` names; pytest does
not run it).  Every case first asserts which instance it reached, then the digest.

Cases: every row of tests/mbconv_cases.py whose release-library tag belongs to XD_MX, MB_MX or MB_MX2, with that sweep's own inputs
(seeded from the case id, B = 2, x rounded to bf16): 1 x 1 maps, a tile - 1, a tile + 1, odd stride-2 inputs; both Cin of a JX class,
hid = 16 (the 16-channel tail round alone) and hid = 144 (four rounds and the tail).  The tags do not carry the MODE parameter: all of
these tensors are far below the sizes at which the launchers fall back to the general kernels, so the release library runs the fast
instances; the experiments build holds the general ones to the same digests under ``CF_FRONT_MODE=0`` (and the pre-deal ones under
``CF_FRONT_MODE=2``), a by-hand run recorded in the profile note.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from centerface_amd import ops
from oracle import bf16_emulation as E
import mbconv_cases as MC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mx_vocab_digests.json")
FAMILIES = ("XD_MX", "MB_MX", "MB_MX2")
CASES = tuple(c for c in MC.CASES if MC.family(c[9]) in FAMILIES)


def _run(c):
    cid, dtype, Cin, hid, Cout, k, s, H, W = c[:9]
    rng = np.random.default_rng(int.from_bytes(cid.encode(), "little"))            # tests/test_mbconv_sweep.py::_inputs
    we, wd, wp = MC.weights(rng, Cin, hid, Cout, k)
    x = E.q_bf16(torch.from_numpy(rng.standard_normal((2, Cin, H, W)).astype(np.float32))).numpy()
    y = ops.expand_dw(x, we, wd, k, s, dtype=dtype) if Cout == 0 else ops.mbconv(x, we, wd, wp, k, s, dtype=dtype)
    assert y.shape == (2, Cout or hid, MC.out_size(H, k, s), MC.out_size(W, k, s)), (cid, y.shape)
    return ops.last_kernel(), {"all": hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest(), "finite": bool(np.isfinite(y).all())}


def record(path=GOLDEN):
    """Write the digest file from the library that is loaded (run once, with the build before a kernel change)."""
    rec = {}
    for c in CASES:
        try:
            tag, dig = _run(c)
        except Exception as e:                               # keep going: the file then lacks the case and the test says so
            print(c[0], "FAILED", repr(e))
            continue
        rec[c[0]] = {"kernel": tag, "sha256": dig}
        print(c[0], tag, dig)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    return rec


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_recorded():
    assert {MC.family(c[9]) for c in CASES} == set(FAMILIES) and all(c[1] == "bf16" for c in CASES)
    assert sorted(_golden()) == sorted(c[0] for c in CASES)


@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_bits_unchanged(cid):
    c = MC.case(cid)
    want = _golden()[cid]
    tag, dig = _run(c)
    assert tag == MC.full_tag(c[9], "bf16"), (cid, tag)
    assert tag == want["kernel"], (cid, tag, want["kernel"])
    assert dig["finite"], "%s: a NaN reached the output" % cid
    assert dig == want["sha256"], (cid, dig, want["sha256"])
