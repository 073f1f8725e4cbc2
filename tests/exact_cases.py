"""Float64 restatement of every launch-plan entry of the fp32 and fp32_split engines, and the bounds they are held to.

No GPU use: tests/test_abi.py ties ``check_layers64`` to the pinned float32 oracle and shows that it sees a wrong tap, a dropped
k-chunk and a wrong pad; tests/test_exact_layers.py applies it to the engine's traced tensors.

The reference is ``oracle/centerface_oracle.py`` itself: its functions are dtype-generic, so they are called with torch.float64
tensors and a float64 copy of the state dict.  TEACHER FORCING: every entry's float64 output is computed from the engine's own
float32 input(s) for that entry, so an error is charged to the launch that made it and nothing accumulates.

The record ``g`` is keyed as ``test_bf16_parity._engine_record`` keys it ("img_u8" or "x", "layer0.0", "layerN.M" = block output,
"layerN.M.dw" = depthwise tensor, "conv_last", "up1", "up2", "up3", "hm" / "wh" / "lm" / "reg"), plus "hm_sigmoid" (record
channel 0), "first_conv" and "layerN.M.expand" (the unfused plan) and two markers, "neck_fused" / "uphead_fused", set where the
plan runs conv_last+up1+up2 / up3+heads as one launch.  ``engine_record`` builds it from an engine.

Bounds, |d| <= atol + rtol |ref| on every element (no outlier allowance), all of them the project's own:
    F32        2e-5   tests/test_gpu_parity.py   fp32 entries that are a single conv
    SPLIT      1e-4   tests/test_gpu_parity.py   the same entries in fp32_split (split-bf16 products, ~2^-16 relative each)
    EXACT_TOL  1e-4   tests/test_mbconv_sweep.py every fused entry, both modes
    hm_sigmoid        F32's atol against float64 clip(sigmoid(.), 1e-4, 1 - 1e-4) of the engine's OWN raw heat map, and every value
                      inside the float32 interval [1e-4, 1 - 1e-4]
Float32 arithmetic itself (the oracle, teacher-forced the same way on CPU) sits at <= 0.08 of these bounds on random uint8 images;
``RAISED`` holds per-entry bounds re-derived from a measurement (profiles/exact_layers_parity.md): none.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import centerface_oracle as O

F32 = dict(rtol=2e-5, atol=2e-5)
SPLIT = dict(rtol=1e-4, atol=1e-4)
EXACT_TOL = dict(rtol=1e-4, atol=1e-4)
RAISED = {}                                  # (dtype, entry) -> dict(rtol, atol); see the module docstring
DTYPES = ("fp32", "fp32_split")
SIG_LO, SIG_HI = np.float32(1e-4), np.float32(1 - 1e-4)

BLOCKS = tuple(O.blocks_table())             # (prefix, cin, cout, t, k, s)
_PREV = dict(zip([b[0] for b in BLOCKS], ["first_conv"] + [b[0] for b in BLOCKS[:-1]]))
_SKIP = {"up1": "layer4.1", "up2": "layer2.1", "up3": "layer1.1"}
_LOW = {"up1": "conv_last", "up2": "up1", "up3": "up2"}

# Which kernel family serves each backbone block behind the fused stem, per mode: ops.mbconv_pick's family, or -- where the engine
# splits the block (no fused family has the shape, or Cout > 64 and cf_mbconv5.hip has it: build_plan) -- XD_F32 (expand+dw launch
# + project GEMM) or None (expand GEMM, depthwise, project GEMM: three launches).  tests/test_abi.py holds the pickers to it.
PLAN = {
    "fp32": (("layer1.0", "MB_TILE"), ("layer1.1", "MB_TILE"), ("layer2.0", "MB_TILE"), ("layer2.1", "MB_F32"), ("layer3.0", "MB_TILE"), ("layer3.1", "MB_TILE"),
             ("layer4.0", "MB_TILE"), ("layer4.1", "MB_TILE"), ("layer5.0", None), ("layer5.1", None), ("layer6.0", None)),
    "fp32_split": (("layer1.0", "MB_F32"), ("layer1.1", "MB_F32"), ("layer2.0", "MB_F32"), ("layer2.1", "MB_SP"), ("layer3.0", "MB_TILE"), ("layer3.1", "MB_TILE"),
                   ("layer4.0", "XD_F32"), ("layer4.1", "XD_F32"), ("layer5.0", "XD_F32"), ("layer5.1", "XD_F32"), ("layer6.0", "XD_F32")),
}
FAMILY_KERNEL = {"MB_TILE": "mbconv_kernel", "MB_F32": "mbconv_f32_kernel", "MB_SP": "mbconv6_kernel", "XD_F32": "expdw_f32_kernel"}


def plan_entries(dtype, fuse=True, neck=True, uphead=True):
    """The names of the launches ``Engine(dtype=dtype, ...).plan()`` must hold (fused-away entries left out), from PLAN."""
    if not fuse:
        out = ["first_conv", "layer0.0.dw", "layer0.0.project"]
        for prefix, _ in PLAN[dtype]:
            out += [prefix + ".expand", prefix + ".dw", prefix + ".project"]
        return out + ["conv_last", "up1", "up2", "up3", "heads"]
    out = ["first_conv+layer0.0"]
    for prefix, fam in PLAN[dtype]:
        out += [prefix + ".mbconv"] if fam in ("MB_TILE", "MB_F32", "MB_SP") else \
               [prefix + ".expand+dw", prefix + ".project"] if fam == "XD_F32" else [prefix + ".expand", prefix + ".dw", prefix + ".project"]
    split = dtype == "fp32_split"
    out += ["conv_last+up1+up2"] if (split and neck) else ["conv_last", "up1", "up2"]
    return out + (["up3+heads"] if (split and uphead) else ["up3", "heads"])


def engine_record(eng, x):
    """Trace every launch of the engine's plan on input ``x`` -> (g, names): the record described in the module docstring and the
    plan entry names it came from."""
    g = {("img_u8" if x.dtype == np.uint8 else "x"): x}
    names = []
    for op in eng.plan():
        if op["fused_away"]:
            continue
        name, v = op["name"], eng.trace(x, op["index"])
        names.append(name)
        if name == "first_conv+layer0.0":
            g["layer0.0"] = v
        elif name.endswith(".mbconv") or name.endswith(".project"):
            g[name.rsplit(".", 1)[0]] = v
        elif name.endswith(".expand+dw"):
            g[name.rsplit(".", 1)[0] + ".dw"] = v
        elif name == "conv_last+up1+up2":
            g["up2"], g["neck_fused"] = v, True
        elif name in ("up3+heads", "heads"):
            g["hm_sigmoid"], g["wh"], g["lm"], g["reg"], g["hm"] = v[:, 0:1], v[:, 1:3], v[:, 3:13], v[:, 13:15], v[:, 15:16]
            if name == "up3+heads":
                g["uphead_fused"] = True
        else:                                              # first_conv, layerN.M.expand, layerN.M.dw, conv_last, up1, up2, up3
            g[name] = v
    return g, names


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(torch.float64)


def input64(g):
    """The network input in float64: the float tensor as it is, or the uint8 image normalised in float64 with the reference's
    (float32) constants -- /255, (x - mean) / std in BGR order, HWC -> CHW (centerface.py:32-37)."""
    if "x" in g:
        return _t64(g["x"])
    img = _t64(g["img_u8"]) / 255.0
    img = (img - _t64(O.MEAN).reshape(1, 1, 1, 3)) / _t64(O.STD).reshape(1, 1, 1, 3)
    return img.permute(0, 3, 1, 2).contiguous()


def heads64(x, sd):
    """Record channels 1..15 (wh, lm, reg, hm_raw) of the head pairs on a float64 up3 map."""
    return torch.cat([O.head(x, sd, n) for n in ("wh", "lm", "reg", "hm")], 1)


def _record_heads(g):
    return np.concatenate([g["wh"], g["lm"], g["reg"], g["hm"]], 1)


def tolerance(dtype, entry):
    if (dtype, entry) in RAISED:
        return RAISED[(dtype, entry)]
    single = entry in ("first_conv", "conv_last", "up1", "up2", "up3") or entry.rsplit(".", 1)[-1] in ("expand", "dw", "project")
    return EXACT_TOL if not single else F32 if dtype == "fp32" else SPLIT


def ratio_map(got, ref, tol):
    ref = ref.numpy() if hasattr(ref, "numpy") else np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    with np.errstate(invalid="ignore"):
        r = np.abs(got - ref) / (tol["atol"] + tol["rtol"] * np.abs(ref))
    return np.where(np.isfinite(got), r, np.inf)


@torch.no_grad()
def check_layers64(sd, g, dtype, maps=None):
    """{plan entry: worst |d| / (atol + rtol |ref|)} for every entry the record ``g`` holds, each float64 output computed from the
    record's own float32 input(s) of that entry.  ``maps`` (a dict): filled with the whole ratio map per entry, for a look at
    where an error sits."""
    assert dtype in DTYPES, dtype
    sd = {k: (_t64(v) if np.asarray(v).dtype.kind == "f" else torch.from_numpy(np.asarray(v))) for k, v in sd.items()}
    out = {}

    def put(entry, got, ref):
        r = ratio_map(got, ref, tolerance(dtype, entry))
        if maps is not None:
            maps[entry] = r
        out[entry] = float(r.max())

    if "first_conv" in g:                                                                       # the unfused plan
        put("first_conv", g["first_conv"], O.conv_swish(input64(g), sd["first_conv.0.1.weight"], 3, 2))
    elif "layer0.0" in g:
        stem = O.conv_swish(input64(g), sd["first_conv.0.1.weight"], 3, 2)
        put("first_conv+layer0.0", g["layer0.0"], O.mbconv(stem, sd, *BLOCKS[0]))
    for prefix, cin, cout, t, k, s in BLOCKS:
        hid, src, j = cin * t, _PREV[prefix], int(t != 1)
        if prefix == "layer0.0" and "first_conv" not in g:
            continue
        if prefix + ".dw" not in g:                                                             # one launch
            if prefix in g:
                put(prefix + ".mbconv", g[prefix], O.mbconv(_t64(g[src]), sd, prefix, cin, cout, t, k, s))
            continue
        wd = sd["%s.conv.%d.1.weight" % (prefix, j)]
        if prefix + ".expand" in g:
            put(prefix + ".expand", g[prefix + ".expand"], O.conv_swish(_t64(g[src]), sd[prefix + ".conv.0.1.weight"], 1, 1))
            put(prefix + ".dw", g[prefix + ".dw"], O.conv_swish(_t64(g[prefix + ".expand"]), wd, k, s, groups=hid))
        elif t == 1:
            put(prefix + ".dw", g[prefix + ".dw"], O.conv_swish(_t64(g[src]), wd, k, s, groups=hid))
        else:
            e = O.conv_swish(_t64(g[src]), sd[prefix + ".conv.0.1.weight"], 1, 1)
            put(prefix + ".expand+dw", g[prefix + ".dw"], O.conv_swish(e, wd, k, s, groups=hid))
        y = F.conv2d(_t64(g[prefix + ".dw"]), sd["%s.conv.%d.weight" % (prefix, j + 1)])
        put(prefix + ".project", g[prefix], y + _t64(g[src]) if (cin == cout and s == 1) else y)
    if "conv_last" in g:
        put("conv_last", g["conv_last"], O.conv_1x1_bn(_t64(g["layer6.0"]), sd))
    for up in ("up1", "up2", "up3"):
        if up in g and _LOW[up] in g:
            put(up, g[up], O.idaup(_t64(g[_LOW[up]]), _t64(g[_SKIP[up]]), sd, up))
    if g.get("neck_fused"):
        y = O.idaup(O.conv_1x1_bn(_t64(g["layer6.0"]), sd), _t64(g["layer4.1"]), sd, "up1")
        put("conv_last+up1+up2", g["up2"], O.idaup(y, _t64(g["layer2.1"]), sd, "up2"))
    if "hm" in g:
        if "up3" in g:
            put("heads", _record_heads(g), heads64(_t64(g["up3"]), sd))
        if g.get("uphead_fused"):
            put("up3+heads", _record_heads(g), heads64(O.idaup(_t64(g["up2"]), _t64(g["layer1.1"]), sd, "up3"), sd))
    if "hm_sigmoid" in g:
        sg = np.asarray(g["hm_sigmoid"])
        r = ratio_map(sg, torch.clamp(torch.sigmoid(_t64(g["hm"])), min=1e-4, max=1 - 1e-4), dict(atol=F32["atol"], rtol=0.0))
        r = np.where((sg >= SIG_LO) & (sg <= SIG_HI), r, np.inf)
        if maps is not None:
            maps["hm_sigmoid"] = r
        out["hm_sigmoid"] = float(r.max())
    return out
