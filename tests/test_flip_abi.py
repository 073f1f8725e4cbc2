"""Flip test (cf_set_flip_test, cf_op_mirror, cf_op_flip_heads): what can be checked without a GPU -- the declarations, the refusals that
come before any device work, the numpy restatement of tests/flip_cases.py against the header's worked example, and its swap property.

What needs a context (the batch limit, the state rules, the merged heads of a forward) is in tests/test_flip.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from flip_cases import PAIR, WORKED_OUT, WORKED_PLANE, WORKED_RECORDS, flip_heads_ref, maps_to_records, mirror_ref, records_to_maps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = cfa._lib
SYMBOLS = ("cf_set_flip_test", "cf_op_mirror", "cf_op_flip_heads")
CF_EINVAL, CF_EHIP = -1, -3
POISON = 0xA5


def _devices():
    n = C.c_int(0)
    return n.value if L.lib().cf_device_count(C.byref(n)) == 0 else 0


# ------------------------------------------------------------------------------------------ the declarations
def test_flip_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), sym
        assert sym in L.EXPORTS and hasattr(lib, sym)
        assert getattr(lib, sym).argtypes is not None, sym
    assert lib.cf_version() == 100
    assert re.search(r"#define\s+CF_VERSION\s+100\b", text)
    # the statement and the worked example are in the header; the kernels are in the build, without FMA contraction
    for word in ("cf_set_flip_test", "MEAN LOGIT", "Worked example", "dataset/dataset.py:125-128", ":166-174", "centerface_ext.py:162-163", "model/losses.py:94-116"):
        assert word in text, word
    mk = open(os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "cf_flip.hip" in srcs and re.search(r"EXTRA_cf_flip\s*=\s*-ffp-contract=off", mk)
    # the Python surface
    import inspect
    for cls in (cfa.Engine, cfa.CenterFace, cfa.CenterFaceBuckets):
        assert inspect.signature(cls.__init__).parameters["flip_test"].default is False, cls
    assert isinstance(cfa.Engine.flip_test, property) and cfa.Engine.flip_test.fset is None
    assert callable(ops.mirror_batch) and callable(ops.flip_heads)


# ------------------------------------------------------------------------------------------ refusals before any device work
def test_set_flip_test_refuses_a_null_context():
    assert L.lib().cf_set_flip_test(None, 1) == CF_EINVAL
    assert L.lib().cf_set_flip_test(None, 0) == CF_EINVAL


def _mirror(fmt=0, B=1, H=32, W=32, x=True, out=True):
    n = max(B, 1) * max(H, 1) * max(W, 1) * 3
    src = np.zeros(n, np.uint8 if fmt != 1 else np.float32)
    dst = np.full(n * (4 if fmt == 1 else 1), POISON, np.uint8)
    code = L.lib().cf_op_mirror(0, fmt, L.ptr(src) if x else None, B, H, W, L.ptr(dst) if out else None)
    return code, bool((dst == POISON).all())


def _merge(B=1, h=2, w=3, rec=True, out=True, plane=True):
    n = max(B, 1) * max(h, 1) * max(w, 1)
    r = np.zeros(2 * n * 16, np.float32)
    o, p = np.full(n * 16, 7.5, np.float32), np.full(n, 7.5, np.float32)
    code = L.lib().cf_op_flip_heads(0, L.ptr(r) if rec else None, B, h, w, L.ptr(o) if out else None, L.ptr(p) if plane else None)
    return code, bool((o == 7.5).all() and (p == 7.5).all())


def test_flip_ops_refuse_bad_arguments_before_any_device_work():
    lib = L.lib()
    for kw in (dict(x=False), dict(out=False), dict(B=0), dict(B=-2), dict(W=31), dict(W=48), dict(W=0), dict(W=-32), dict(H=0), dict(fmt=2), dict(fmt=-1),
               dict(fmt=1, W=40), dict(fmt=1, B=0), dict(fmt=1, x=False)):
        code, untouched = _mirror(**kw)
        assert code == CF_EINVAL and untouched, kw
        assert b"cf_op_mirror" in lib.cf_op_last_error(), kw
    assert _mirror(W=48)[0] == CF_EINVAL and b"W=48" in lib.cf_op_last_error()                    # the value is named
    assert _mirror(fmt=7)[0] == CF_EINVAL and b"format 7" in lib.cf_op_last_error()
    for kw in (dict(rec=False), dict(out=False), dict(plane=False), dict(B=0), dict(B=-1), dict(h=0), dict(w=0)):
        code, untouched = _merge(**kw)
        assert code == CF_EINVAL and untouched, kw
        assert b"cf_op_flip_heads" in lib.cf_op_last_error(), kw
    # fine arguments get as far as the device: CF_EHIP where there is none, no crash either way
    want = 0 if _devices() > 0 else CF_EHIP
    for kw in (dict(), dict(fmt=1), dict(B=2, H=64, W=96), dict(H=1)):
        assert _mirror(**kw)[0] == want, kw
    for kw in (dict(), dict(B=2, h=1, w=1), dict(w=40)):
        assert _merge(**kw)[0] == want, kw
    if want == CF_EHIP:
        assert b"cf_op_flip_heads" in lib.cf_op_last_error()
    with pytest.raises(ValueError):
        ops.mirror_batch(np.zeros((1, 32, 32, 4), np.uint8))
    with pytest.raises(ValueError):
        ops.mirror_batch(np.zeros((1, 4, 32, 32), np.float32))
    with pytest.raises(ValueError):
        ops.flip_heads(np.zeros((3, 2, 2, 16), np.float32), 2)
    with pytest.raises(ValueError):
        ops.flip_heads(np.zeros((2, 2, 2, 15), np.float32), 1)


# ------------------------------------------------------------------------------------------ the restatement
def test_restatement_reproduces_the_worked_example():
    out, plane = flip_heads_ref(WORKED_RECORDS, 1)
    assert out.dtype == np.float32 and out.shape == (1, 1, 2, 16) and plane.shape == (1, 2)
    assert np.array_equal(out, WORKED_OUT) and np.array_equal(plane, WORKED_PLANE)
    # by hand, without the restatement: cell (0, 0) pairs with the mirrored pass's cell (0, 1)
    a, m = WORKED_RECORDS[0, 0, 0], WORKED_RECORDS[1, 0, 1]
    assert WORKED_OUT[0, 0, 0, 3] == (a[3] - m[5]) / 2 == -0.5 and WORKED_OUT[0, 0, 0, 11] == (a[11] - m[9]) / 2 == -0.625
    assert WORKED_OUT[0, 0, 0, 12] == (a[12] + m[10]) / 2 == 1.5 and tuple(WORKED_OUT[0, 0, 0, 13:15]) == (a[13], a[14])
    # the maps of cf_get_heads and the records are two views of the same numbers
    maps = records_to_maps(out)
    assert maps["lm"].shape == (1, 10, 1, 2) and np.array_equal(maps_to_records(maps), out)
    assert np.array_equal(maps["hm"][0, 0], out[0, :, :, 15]) and np.array_equal(maps["hm_sigmoid"][0, 0], out[0, :, :, 0])


def test_mirror_restatement_reverses_pixels_not_bytes():
    x = np.arange(2 * 2 * 4 * 3, dtype=np.uint8).reshape(2, 2, 4, 3)
    y = mirror_ref(x, 0)
    assert y.flags["C_CONTIGUOUS"] and np.array_equal(y[1, 1, 0], x[1, 1, 3]) and np.array_equal(y[0, 0, 1], x[0, 0, 2])
    assert np.array_equal(mirror_ref(y), x)
    f = np.arange(1 * 3 * 2 * 4, dtype=np.float32).reshape(1, 3, 2, 4)
    g = mirror_ref(f, 1)
    assert np.array_equal(g[0, 2, 1], f[0, 2, 1, ::-1]) and np.array_equal(mirror_ref(g), f)


def swap_property(first, second, w):
    """merge(M, A) against merge(A, M), both [B, h, w, 16]: at column w - 1 - x the same heat, wh and logit, the landmarks negated in x
    with the pairs swapped.  Exact: a + m == m + a, and (m - a) * 0.5 == -((a - m) * 0.5) in IEEE arithmetic."""
    back = second[:, :, ::-1, :]
    ok = all(np.array_equal(back[..., k], first[..., k]) for k in (0, 1, 2, 15))
    for j, p in enumerate(PAIR):
        ok = ok and np.array_equal(back[..., 3 + 2 * j], -first[..., 3 + 2 * p]) and np.array_equal(back[..., 4 + 2 * j], first[..., 4 + 2 * p])
    return ok


def test_restatement_swap_property_is_exact_on_random_records():
    rng = np.random.default_rng(11)
    for B, h, w in ((1, 1, 2), (2, 3, 5), (3, 8, 8)):
        rec = (rng.standard_normal((2 * B, h, w, 16)) * 7).astype(np.float32)
        assert (rec < 0).any()
        ab, _ = flip_heads_ref(rec, B)
        ba, plane = flip_heads_ref(np.concatenate([rec[B:], rec[:B]]), B)
        assert swap_property(ab, ba, w)
        assert np.array_equal(plane, ba[..., 0].reshape(B, -1))
        assert np.array_equal(ab[..., 13:15], rec[:B, :, :, 13:15]) and np.array_equal(ba[..., 13:15], rec[B:, :, :, 13:15])
