"""The fp32 and fp32_split ENGINES, launch by launch, against float64.

These two modes carry the parity claim (fp32: exact mode; fp32_split: the 1e-3 tolerance mode, benchmarked at B = 64), and until this
file they were held to it only end to end at rtol = atol = 1e-3 -- 50 times the project's per-op bound, and silent on where an error
arose -- plus op-level sweeps through ``ops.*`` that reach neither the engine's launch plan nor its buffers (the pixel-block layouts
between the split mode's late blocks, the fused stem's uint8 and float staging, cf_neck.hip / cf_uphead.hip / cf_head.hip on real maps).

Here every entry of the engine's own plan is traced (``Engine.trace``) and compared with ``exact_cases.check_layers64``: the float64
restatement of that entry applied to the engine's OWN float32 input(s) for it (teacher forcing), at the project's per-op bounds --
F32 2e-5 / SPLIT 1e-4 for a single conv, EXACT_TOL 1e-4 for a fused launch, every element, no outlier allowance.  Float32 arithmetic
itself sits at <= 0.08 of those bounds on this data (tests/test_abi.py ties the check to the pinned oracle and shows that one wrong
tap, a dropped k-chunk or a wrong pad column is > 100 bounds out).  Measured ratios: profiles/exact_layers_parity.md.
"""
import re

import numpy as np
import pytest

import centerface_amd as cfa

import exact_cases as X
from test_gpu_parity import F32, SPLIT
from test_mbconv_sweep import EXACT_TOL

pytestmark = pytest.mark.gpu

SD = cfa.weights.synthetic_state_dict(0)
HEADS = ("hm", "wh", "lm", "reg", "hm_sigmoid")
# the smallest sizes that give every kernel a one-cell map (32x32), a map narrower than a tile (32x640), partial tiles in both
# directions, M = B h w not a multiple of 32 in the pixel-block buffers (32x32, 32x640, 96x128 with B = 3) and interior tiles (352x640)
SIZES = [((32, 32), 1), ((32, 640), 2), ((64, 96), 2), ((96, 128), 3), ((160, 224), 2), ((352, 640), 1)]


def test_bounds_are_the_projects_own():
    assert X.F32 == F32 and X.SPLIT == SPLIT and X.EXACT_TOL == EXACT_TOL and not X.RAISED


def _images(size, B):
    H, W = size
    return np.random.default_rng(H + 3 * W).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def _trace_some(eng, x, names):
    """{plan entry name: traced output} for the named entries of the engine's plan."""
    idx = {op["name"]: op["index"] for op in eng.plan() if not op["fused_away"]}
    return {n: eng.trace(x, idx[n]) for n in names}


def _report_and_assert(ratios, dtype, size, expect, what=""):
    for entry, r in ratios.items():
        print("EXACTLAYERS %s %dx%d %s%s %.4f" % (dtype, size[0], size[1], what, entry, r))
    assert sorted(ratios) == sorted(expect), (sorted(ratios), sorted(expect))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, "%s %s: |d| / (atol + rtol |ref|) > 1 for %s" % (dtype, size, bad)


def _assert_forward_reproduces(eng, x, g):
    """forward_enqueue (eager, then graph capture, then graph replay) gives the traced head record bit for bit."""
    for _ in range(3):
        eng.forward_enqueue(x)
        hd = eng.heads(sigmoid_hm=True)
        for k in HEADS:
            assert np.array_equal(hd[k], g[k]), k


@pytest.mark.parametrize("size,B", SIZES, ids=["%dx%d" % s for s, _ in SIZES])
@pytest.mark.parametrize("dtype", X.DTYPES)
def test_exact_engine_layer_by_layer_teacher_forced(dtype, size, B):
    """Every launch of the default plan -- fp32: 23 (fused stem, 8 fused blocks, 3 x expand / depthwise / project, conv_last, up1-3,
    heads), fp32_split: 19 (fused stem, 6 fused blocks, 5 x expand+dw / project, fused neck, up3+heads) -- on random uint8 images.  In
    the split mode conv_last and up1 (LDS only inside the neck launch) come from a ``neck=False`` engine and up3 from an
    ``uphead=False`` one, after the tensors the plans share are found bit-equal, so the fused launches are also checked stage by stage."""
    H, W = size
    x = _images(size, B)
    eng = cfa.Engine(H, W, max_batch=B, dtype=dtype, weights=SD)
    g, names = X.engine_record(eng, x)
    assert names == X.plan_entries(dtype), names
    expect = names + ["hm_sigmoid"]
    if dtype == "fp32_split":
        e3 = cfa.Engine(H, W, max_batch=B, dtype=dtype, weights=SD, neck=False)
        t3 = _trace_some(e3, x, ["layer6.0.project", "conv_last", "up1", "up2", "up3+heads"])
        assert np.array_equal(t3["layer6.0.project"], g["layer6.0"]) and np.array_equal(t3["up2"], g["up2"])
        assert np.array_equal(t3["up3+heads"][:, 1:], X._record_heads(g)) and np.array_equal(t3["up3+heads"][:, 0:1], g["hm_sigmoid"])
        g["conv_last"], g["up1"] = t3["conv_last"], t3["up1"]
        e3.close()
        e2 = cfa.Engine(H, W, max_batch=B, dtype=dtype, weights=SD, uphead=False)
        t2 = _trace_some(e2, x, ["conv_last+up1+up2", "up3", "heads"])
        assert np.array_equal(t2["conv_last+up1+up2"], g["up2"])
        assert np.array_equal(t2["heads"][:, 1:], X._record_heads(g)) and np.array_equal(t2["heads"][:, 0:1], g["hm_sigmoid"])
        g["up3"] = t2["up3"]
        e2.close()
        expect += ["conv_last", "up1", "up2", "up3", "heads"]
    assert len(expect) == (24 if dtype == "fp32" else 25)
    _report_and_assert(X.check_layers64(SD, g, dtype), dtype, size, expect)
    _assert_forward_reproduces(eng, x, g)
    eng.close()


# Derived from the code, not from a run: tests/test_abi.py pins the family of every block (exact_cases.PLAN -> FAMILY_KERNEL); the three
# split blocks of the exact mode run pw_wlds_kernel (K >= 64, >= 3 n-blocks, no bias: cf_pw.hip dispatch_nbw) around dw_lds_kernel
# (layer5.0, stride 2) / dw_strip_kernel (stride 1: cf_dw.hip dw_by_stride); conv_last and the IDAUp stages carry a bias -> pw_kernel;
# the split mode's project GEMMs are pw_wlds_kernel too, its neck and up3+heads one launch each.
KERNELS = {
    "fp32": ["dw_lds_kernel", "dw_strip_kernel", "head_kernel", "mbconv_f32_kernel", "mbconv_kernel", "pw_kernel", "pw_wlds_kernel", "stem0_kernel"],
    "fp32_split": ["expdw_f32_kernel", "mbconv6_kernel", "mbconv_f32_kernel", "mbconv_kernel", "neck_kernel", "pw_wlds_kernel", "stem0_kernel",
                   "uphead_kernel"],
}


@pytest.mark.parametrize("dtype", X.DTYPES)
def test_exact_plans_reach_their_kernels(dtype):
    """The default plans at 96x128 launch exactly the kernels the layer-by-layer test is meant to cover, each entry the one of its family."""
    fams = {X.FAMILY_KERNEL[f] for _, f in X.PLAN[dtype] if f}
    rest = {"stem0_kernel", "pw_wlds_kernel"} | ({"neck_kernel", "uphead_kernel"} if dtype == "fp32_split" else
                                                 {"pw_kernel", "dw_lds_kernel", "dw_strip_kernel", "head_kernel"})
    assert sorted(fams | rest) == KERNELS[dtype]
    eng = cfa.Engine(96, 128, max_batch=3, dtype=dtype, weights=SD)
    prof = eng.profile_forward(_images((96, 128), 3))
    eng.close()
    assert [p["name"] for p in prof] == X.plan_entries(dtype)
    base = {p["name"]: re.search(r"cf::(\w+)", p["kernel"]).group(1) for p in prof}
    assert sorted(set(base.values())) == KERNELS[dtype], base
    assert re.match(r"void cf::stem0_kernel<%s, \d+>" % ("float" if dtype == "fp32" else "sp32_t"), prof[0]["kernel"]), prof[0]["kernel"]
    for prefix, fam in X.PLAN[dtype]:
        if fam in ("MB_TILE", "MB_F32", "MB_SP"):
            assert base[prefix + ".mbconv"] == X.FAMILY_KERNEL[fam], (prefix, base)
        elif fam == "XD_F32":
            assert (base[prefix + ".expand+dw"], base[prefix + ".project"]) == ("expdw_f32_kernel", "pw_wlds_kernel"), (prefix, base)
        else:
            assert (base[prefix + ".expand"], base[prefix + ".project"]) == ("pw_wlds_kernel", "pw_wlds_kernel"), (prefix, base)
            assert base[prefix + ".dw"] == ("dw_lds_kernel" if prefix == "layer5.0" else "dw_strip_kernel"), (prefix, base)


@pytest.mark.parametrize("size,B", [((32, 640), 2), ((96, 128), 3)], ids=["32x640", "96x128"])
@pytest.mark.parametrize("dtype", X.DTYPES)
def test_exact_float_input_stem(dtype, size, B):
    """``CF_IN_F32_NCHW`` staging of the fused stem (an already normalised tensor, as the reference hands it to the network), standard
    normal float32: entry 0 against float64.  No normalisation step on this path, so a difference from the uint8 case is the staging."""
    H, W = size
    x = np.random.default_rng(H + 3 * W + 1).standard_normal((B, 3, H, W)).astype(np.float32)
    eng = cfa.Engine(H, W, max_batch=B, dtype=dtype, weights=SD)
    assert eng.plan()[0]["name"] == "first_conv+layer0.0"
    g = {"x": x, "layer0.0": eng.trace(x, 0)}
    eng.close()
    _report_and_assert(X.check_layers64(SD, g, dtype), dtype, size, ["first_conv+layer0.0"], "float-input ")


_ALT = [("fp32", dict(fuse=False)), ("fp32", dict(collapse_heads=False)), ("fp32_split", dict(fuse=False)), ("fp32_split", dict(collapse_heads=False)),
        ("fp32_split", dict(neck=False, uphead=False))]


@pytest.mark.parametrize("size,B", [((64, 96), 2), ((96, 128), 3)], ids=["64x96", "96x128"])
@pytest.mark.parametrize("dtype,flags", _ALT, ids=["%s-%s" % (d, "+".join(sorted(f))) for d, f in _ALT])
def test_exact_alternative_plans(dtype, flags, size, B):
    """The same check on the plans behind the engine's switches: ``fuse=False`` (cf_stem.hip's first_conv, every block as expand GEMM /
    depthwise / project GEMM), ``collapse_heads=False`` (the two-stage head kernel, which keeps the reference's operation order; in the
    split mode also up3 as a launch of its own) and, in the split mode, the separate conv_last / up1 / up2 / up3 launches."""
    H, W = size
    x = _images(size, B)
    eng = cfa.Engine(H, W, max_batch=B, dtype=dtype, weights=SD, **flags)
    g, names = X.engine_record(eng, x)
    collapse = flags.get("collapse_heads", True)
    assert names == X.plan_entries(dtype, fuse=flags.get("fuse", True), neck=flags.get("neck", True), uphead=flags.get("uphead", True) and collapse), names
    assert len(names) == {"fuse": 41, "collapse_heads": 23 if dtype == "fp32" else 20, "neck": 22}[sorted(flags)[0]]
    _report_and_assert(X.check_layers64(SD, g, dtype), dtype, size, names + ["hm_sigmoid"], "+".join("%s=%s" % kv for kv in sorted(flags.items())) + " ")
    _assert_forward_reproduces(eng, x, g)
    eng.close()
