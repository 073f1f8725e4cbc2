"""CPU-side checks of the drop-in boundary: the C-ABI library loads without a GPU, exports every
symbol include/centerface_hip.h declares, reports errors instead of falling back, and the host
logic (schema, sharding, transform) is right.  No compute calls here."""
import ctypes
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa

import mbconv_cases as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cf_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    L = cfa._lib.lib()
    declared = _declared_symbols()
    assert len(declared) >= 28
    missing = [s for s in declared if not hasattr(L, s)]
    assert not missing, missing
    assert sorted(cfa._lib.EXPORTS) == declared
    assert L.cf_version() == 100
    assert L.cf_strerror(-5).decode().startswith("state_dict")


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        cfa.Engine(64, 64)
    assert e.value.code == -3          # CF_EHIP: fails loudly, no silent CPU path
    with pytest.raises((cfa._lib.CenterFaceError, ValueError)):
        cfa.ops.conv_pw(np.zeros((1, 8, 4, 4), np.float32), np.zeros((8, 8), np.float32))


def test_argument_validation_happens_before_any_gpu_work():
    L = cfa._lib.lib()
    h = ctypes.c_void_p()
    assert L.cf_create(0, 1, 100, 64, 0, 0, ctypes.byref(h)) == -1        # H not a multiple of 32
    assert b"multiples of 32" in L.cf_last_error(None)
    assert L.cf_create(0, 0, 64, 64, 0, 0, ctypes.byref(h)) == -1
    assert L.cf_create(0, 1, 64, 64, 7, 0, ctypes.byref(h)) == -1         # unknown dtype


def test_pwconv_test_hooks_are_declared_exported_and_validate_first():
    """The hooks tests/test_pw_sweep.py stands on: ``cf_op_last_kernel`` (which instance ran) and ``cf_op_pwconv_ex`` (pixel-block
    addressing per operand); unknown layout bits, or a pixel-block residual without a residual, are CF_EINVAL before any GPU work."""
    L = cfa._lib.lib()
    declared = _declared_symbols()
    for name in ("cf_op_last_kernel", "cf_op_pwconv_ex"):
        assert name in declared and name in cfa._lib.EXPORTS and hasattr(L, name), name
    assert isinstance(cfa.ops.last_kernel(), str)
    x, w, y = np.zeros((1, 8, 4, 4), np.float32), np.zeros((8, 8), np.float32), np.zeros((1, 8, 4, 4), np.float32)
    p = cfa._lib.ptr
    for layout in (8, -1, 4, 5, 1 << 20):                  # 4 / 5: residual bit, no residual
        assert L.cf_op_pwconv_ex(0, 0, p(x), p(w), None, None, p(y), 1, 8, 8, 4, 4, 0, layout) == -1, layout
        assert L.cf_op_last_error()
    assert L.cf_op_pwconv_ex(0, 0, p(x), p(w), None, None, p(y), 1, 12, 8, 4, 4, 0, 0) == -1      # Cin % 8
    with pytest.raises(ValueError) as e:
        cfa.ops.conv_pw(x, w, layout=8)
    assert isinstance(e.value, cfa._lib.CenterFaceError) and e.value.code == -1 and "layout" in str(e.value)


# ------------------------------------------------------------------------------- the MBConv sweep's GPU-less half
_HIDS = (16, 32, 48, 64, 96, 144, 192, 384, 576, 960)
_DTYPES = ("fp32", "fp32_split", "bf16")


def _pick(c):
    _, dtype, Cin, hid, Cout, k, s = c[:7]
    return cfa.ops.expand_dw_pick(Cin, hid, k, s, dtype) if Cout == 0 else cfa.ops.mbconv_pick(Cin, hid, Cout, k, s, dtype)


def _assert_lands_where_claimed(c, short, g):
    """The geometry's answer for case c against what the tag ``short`` says about its table row."""
    _, dtype, Cin, hid, Cout, k, s = c[:7]
    if short == "REFUSED":
        assert not g["ok"], (c[0], g)
        return
    assert g["ok"], (c[0], "refused")
    claim = M.claimed(short)
    have = dict(kind=g["kind"], k=k, s=s, JX=g["JX"], HC=g["HC"], nbo=(Cout + 31) // 32, res=int(Cin == Cout and s == 1), tail=int(hid % 32 == 16))
    wrong = {n: (v, have[n]) for n, v in claim.items() if have[n] != v}
    assert not wrong, (c[0], short, wrong)
    assert g["nq"] == hid // g["HC"] and (hid % g["HC"] == 0 or (claim.get("tail") and hid % 32 == 16)), (c[0], g)


def test_mbconv_pick_hooks_are_declared_exported_and_need_no_gpu():
    """``cf_op_mbconv_pick`` / ``cf_op_expand_dw_pick``: the geometry functions alone.  Production shapes land where DESIGN.md says."""
    L = cfa._lib.lib()
    declared = _declared_symbols()
    for name in ("cf_op_mbconv_pick", "cf_op_expand_dw_pick"):
        assert name in declared and name in cfa._lib.EXPORTS and hasattr(L, name), name
    out = (ctypes.c_int * 8)()
    assert L.cf_op_mbconv_pick(7, 16, 96, 24, 3, 2, out) == -1 and L.cf_op_mbconv_pick(0, 16, 96, 24, 3, 2, None) == -1
    assert L.cf_op_expand_dw_pick(-1, 96, 576, 5, 2, out) == -1
    g = cfa.ops.mbconv_pick(16, 96, 24, 3, 2, "bf16")
    assert g == dict(ok=True, kind="MB_PX", HC=32, nq=3, JX=1, NBO=1, HALF=g["HALF"], KG=g["KG"])
    assert cfa.ops.mbconv_pick(32, 192, 32, 5, 1, "fp32_split")["kind"] == "MB_SP"
    assert cfa.ops.expand_dw_pick(160, 960, 3, 1, "bf16")["kind"] == "XD_MX" and cfa.ops.expand_dw_pick(96, 576, 5, 2, "fp32_split")["HALF"] == 18
    assert cfa.ops.mbconv_pick(32, 32, 32, 5, 1, "fp32") == dict(ok=False, kind=None, HC=0, nq=0, JX=0, NBO=0, HALF=0, KG=0)


def test_mbconv_sweep_table_is_well_formed():
    assert len(set(M.IDS)) == len(M.IDS) >= 150
    for c in M.CASES:
        cid, dtype, Cin, hid, Cout, k, s, H, W, tag, alt = c
        assert dtype in _DTYPES and 1 <= M.out_size(H, k, s) <= 45 and 1 <= M.out_size(W, k, s) <= 45, cid
        for t in (tag, alt):
            if t not in (None, "REFUSED"):
                assert M.family(t) in cfa.ops.MB_KINDS.values() and (Cout == 0) == M.family(t).startswith("XD_"), cid
                assert M.full_tag(t, dtype).startswith("void cf::") and " T," not in M.full_tag(t, dtype), cid


def test_mbconv_sweep_covers_every_group_of_accepted_shapes():
    """Every block shape the two geometry functions accept, grouped by the table row that serves it -- (dtype, family, k, s, JX,
    n-blocks, residual, tail, HC): each group has a case in the sweep's table, and each case is accepted and lands on the row its
    tag names.  A new table row, or a retuned HC, without cases of its own fails here, without a GPU."""
    groups = {}
    for dtype in _DTYPES:
        for k in (3, 5):
            for s in (1, 2):
                for Cin in range(8, 161, 8):
                    for hid in _HIDS:
                        g = cfa.ops.expand_dw_pick(Cin, hid, k, s, dtype)
                        if g["ok"]:
                            groups.setdefault(M.group_key(dtype, g, Cin, hid, 0, k, s), (Cin, hid, 0))
                        for Cout in range(8, 97, 8):
                            g = cfa.ops.mbconv_pick(Cin, hid, Cout, k, s, dtype)
                            if g["ok"]:
                                groups.setdefault(M.group_key(dtype, g, Cin, hid, Cout, k, s), (Cin, hid, Cout))
    assert len(groups) >= 40
    covered = set()
    for c in M.CASES:
        g = _pick(c)
        _assert_lands_where_claimed(c, c[9], g)
        if g["ok"]:
            covered.add(M.group_key(c[1], g, c[2], c[3], c[4], c[5], c[6]))
    missing = {key: first for key, first in groups.items() if key not in covered}
    assert not missing, "groups of accepted shapes without a sweep case (key: first member (Cin, hid, Cout)): %s" % missing
    assert {key[1] for key in covered} == set(cfa.ops.MB_KINDS.values())          # all nine families


@pytest.mark.parametrize("name,value", [("CF_DW_MATRIX", "0"), ("CF_F4_VARIANT", "1")])
def test_mbconv_sweep_switch_column_matches_the_geometry(name, value):
    """The switches are read once per process: a child asks the geometry functions with the switch set, and every case must land
    where the table's last column says (None: where it lands without the switch)."""
    import json
    import subprocess
    import sys
    code = ("import json, sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_abi as T, mbconv_cases as M; "
            "print(json.dumps([T._pick(c) for c in M.CASES]))" % (REPO, os.path.join(REPO, "tests")))
    env = dict(os.environ)
    env[name] = value
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    picks = json.loads(r.stdout.strip().splitlines()[-1])
    moved = 0
    for c, g in zip(M.CASES, picks):
        if M.SWITCH[c[1]] != (name, value):
            continue
        _assert_lands_where_claimed(c, M.short_tag(c, {name: value}), g)
        moved += c[10] is not None
    assert moved >= 20
    families = {M.family(c[10]) for c in M.CASES if M.SWITCH[c[1]] == (name, value) and c[10] not in (None, "REFUSED")}
    assert families >= ({"MB_PX", "XD_PX"} if name == "CF_DW_MATRIX" else {"MB_F32"})


def test_mbconv_refusals_need_no_gpu():
    """Shapes no family serves are CF_EINVAL before a device is opened (this machine may have none), with a message, and the
    output buffer is not touched."""
    L, p = cfa._lib.lib(), cfa._lib.ptr
    rng = np.random.default_rng(0)
    for what, (dtype, Cin, hid, Cout, k, s) in M.REFUSED.items():
        x = rng.standard_normal((1, Cin, 5, 6)).astype(np.float32)
        we, wd, wp = M.weights(rng, Cin, hid, Cout, k)
        y = np.full((1, Cout or hid, 5, 6), 7.0, np.float32)
        dt = cfa.ops._DT[dtype]
        if Cout == 0:
            assert not cfa.ops.expand_dw_pick(Cin, hid, k, s, dtype)["ok"], what
            code = L.cf_op_expand_dw(0, dt, p(x), p(we), p(wd), p(y), 1, Cin, hid, 5, 6, k, s)
        else:
            assert not cfa.ops.mbconv_pick(Cin, hid, Cout, k, s, dtype)["ok"], what
            code = L.cf_op_mbconv(0, dt, p(x), p(we), p(wd), p(wp), p(y), 1, Cin, hid, Cout, 5, 6, k, s)
        assert code == -1 and L.cf_op_last_error() and (y == 7.0).all(), what
        with pytest.raises(cfa._lib.CenterFaceValueError):
            cfa.ops.expand_dw(x, we, wd, k, s, dtype=dtype) if Cout == 0 else cfa.ops.mbconv(x, we, wd, wp, k, s, dtype=dtype)


def test_float64_mbconv_restatement_matches_the_oracle_on_the_production_shapes():
    """``mbconv_cases.ref64`` (the sweep's fp32 / fp32_split reference) against ``O.mbconv``, the pinned float32 oracle, on the
    eight fused block shapes (hid = 6 Cin, production Cout): float32 round-off of the oracle's own sums and nothing else."""
    import torch
    from oracle import centerface_oracle as O
    done = 0
    for prefix, cin, cout, t, k, s in O.blocks_table():
        if t == 1 or cout > 96:
            continue
        rng = np.random.default_rng(cin * 100 + cout)
        we, wd, wp = M.weights(rng, cin, cin * t, cout, k)
        x = rng.standard_normal((2, cin, 9, 12)).astype(np.float32)
        sd = {prefix + ".conv.0.1.weight": torch.from_numpy(we.reshape(cin * t, cin, 1, 1)), prefix + ".conv.1.1.weight": torch.from_numpy(wd),
              prefix + ".conv.2.weight": torch.from_numpy(wp.reshape(cout, cin * t, 1, 1))}
        ref = O.mbconv(torch.from_numpy(x), sd, prefix, cin, cout, t, k, s).numpy()
        got = M.ref64(x, we, wd, wp, k, s)
        assert got.shape == ref.shape == (2, cout, M.out_size(9, k, s), M.out_size(12, k, s))
        # the oracle's float32 sums: <= 576 terms of O(1/sqrt(n)) each, eps 6e-8 -> a few 1e-6 on O(1) outputs
        np.testing.assert_allclose(ref, got, rtol=2e-5, atol=2e-5, err_msg=prefix)
        d = M.ref64(x, we, wd, None, k, s)
        assert d.shape == (2, cin * t, ref.shape[2], ref.shape[3])
        dref = O.conv_swish(O.conv_swish(torch.from_numpy(x), sd[prefix + ".conv.0.1.weight"], 1, 1), sd[prefix + ".conv.1.1.weight"], k, s, groups=cin * t).numpy()
        np.testing.assert_allclose(dref, d, rtol=2e-5, atol=2e-5, err_msg=prefix + " expand+dw")
        done += 1
    assert done == 8


def test_schema_matches_reference_checkpoint_layout():
    sch = cfa.schema.state_dict_schema()
    assert len(sch) == 94
    assert sum(int(np.prod(s)) for s in sch.values()) == 1308126
    assert sch["layer0.0.conv.0.1.weight"] == (32, 1, 3, 3) and sch["layer0.0.conv.1.weight"] == (16, 32, 1, 1)
    assert sch["layer2.0.conv.1.1.weight"] == (144, 1, 5, 5)
    assert sch["up1.conv.0.weight"] == (24, 96, 1, 1) and sch["lm.1.weight"] == (10, 24, 1, 1)
    sd = cfa.weights.synthetic_state_dict(3)
    assert list(sd) == list(sch)
    bad = dict(sd); bad["extra"] = np.zeros(1, np.float32)
    with pytest.raises(ValueError):
        cfa.weights.validate_state_dict(bad)
    bad = dict(sd); bad["hm.0.bias"] = np.zeros(25, np.float32)
    with pytest.raises(ValueError):
        cfa.weights.validate_state_dict(bad)


def test_shard_range_partitions_in_order():
    for n in (0, 1, 7, 64, 512, 513):
        for world in (1, 2, 3, 8):
            spans = [cfa.distributed.shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        cfa.distributed.shard_range(4, 2, 2)


def test_transform_table(golden):
    g = golden("decode_d1")
    face = object.__new__(cfa.CenterFace)
    for (h, w), ref in zip(g["tf_in"], g["tf_out"]):
        assert np.array_equal(np.asarray(cfa.CenterFace.transform(face, int(h), int(w)), np.float64), ref)


def test_wider_result_format(tmp_path):
    """demo.py:81-87: path line, count line, then 'x y w h score' with w = x2 - x1 + 1."""
    dets = np.array([[10.0, 20.0, 29.0, 59.0, 0.98765], [0.0, 0.0, 5.5, 7.25, 0.05]], np.float32)
    txt = cfa.demo.format_wider_result("0--Parade/0_Parade_marchingband_1_465.jpg", dets)
    assert txt == "0--Parade/0_Parade_marchingband_1_465.jpg\n2\n10.0 20.0 20.0 40.0 0.988\n0.0 0.0 6.5 8.2 0.050\n"
    p = cfa.demo.write_wider_result(str(tmp_path), "0--Parade", "img_1", np.empty((0, 5), np.float32))
    assert open(p).read() == "0--Parade/img_1.jpg\n0\n" and p.endswith("0--Parade/img_1.txt")


def test_fast_floor_division_equals_numpy_floor_divide():
    """CenterFace._floordiv must be `a // scale` (centerface.py:56,58) bit for bit: random coordinates, values at and one
    ulp around exact integer multiples of the scale, negatives (landmarks left of the image), signed zeros, scale 1."""
    import centerface_amd as cfa
    rng = np.random.default_rng(0)
    for trial in range(40):
        h = int(rng.integers(33, 1300))
        s = (int(np.ceil(h / 32) * 32) / h) if trial else 1.0
        s32 = np.float32(s)
        n = rng.integers(0, 1300, 20000).astype(np.float32)
        near = (n * s32).astype(np.float32)
        a = np.concatenate([rng.uniform(-50, 1300, 50000).astype(np.float32), near, np.nextafter(near, np.float32(np.inf)),
                            np.nextafter(near, np.float32(-np.inf)), -near[:500], np.array([0.0, -0.0], np.float32)])
        ref, got = a // s, cfa.CenterFace._floordiv(a, s)
        assert got.dtype == np.float32 and np.array_equal(ref, got) and np.array_equal(np.signbit(ref), np.signbit(got)), s


# ------------------------------------------------------------------------------- the exact-mode layer check's GPU-less half
import exact_cases as X


def _oracle_record(sd, img, defect=None):
    """The float32 oracle run launch by launch, as an engine whose every entry is its own launch would record it (the unfused plan
    + the head record), in the keys of ``exact_cases.engine_record``.  ``defect``: one deliberately wrong step --
    "dw_tap" (layer3.1: the centre tap of the last output column reads the column to its left), "k_chunk" (layer5.1's project GEMM
    without its last 8 input channels) or "stem_pad" (the stem's right / bottom zero pad replaced by edge replication)."""
    import torch
    import torch.nn.functional as F
    from oracle import centerface_oracle as O
    g = {"img_u8": img}
    x = torch.from_numpy(np.concatenate([O.preprocess(im) for im in img]))
    w = sd["first_conv.0.1.weight"]
    cur = O.swish(F.conv2d(F.pad(x, [0, 1, 0, 1], mode="replicate"), w, None, 2)) if defect == "stem_pad" else O.conv_swish(x, w, 3, 2)
    g["first_conv"] = cur
    for prefix, cin, cout, t, k, s in X.BLOCKS:
        src, j = cur, int(t != 1)
        if t != 1:
            src = g[prefix + ".expand"] = O.conv_swish(cur, sd[prefix + ".conv.0.1.weight"], 1, 1)
        wd = sd["%s.conv.%d.1.weight" % (prefix, j)]
        if defect == "dw_tap" and prefix == "layer3.1":
            pre = F.conv2d(O.same_pad(src, k, s), wd, None, s, 0, 1, cin * t)
            pre[..., -1] += wd[:, 0, k // 2, k // 2].reshape(1, -1, 1) * (src[..., -2] - src[..., -1])
            d = O.swish(pre)
        else:
            d = O.conv_swish(src, wd, k, s, groups=cin * t)
        g[prefix + ".dw"] = d
        wp = sd["%s.conv.%d.weight" % (prefix, j + 1)]
        y = F.conv2d(d[:, :-8], wp[:, :-8]) if (defect == "k_chunk" and prefix == "layer5.1") else F.conv2d(d, wp)
        cur = g[prefix] = cur + y if (cin == cout and s == 1) else y
    g["conv_last"] = O.conv_1x1_bn(cur, sd)
    g["up1"] = O.idaup(g["conv_last"], g["layer4.1"], sd, "up1")
    g["up2"] = O.idaup(g["up1"], g["layer2.1"], sd, "up2")
    g["up3"] = O.idaup(g["up2"], g["layer1.1"], sd, "up3")
    for name in ("hm", "wh", "lm", "reg"):
        g[name] = O.head(g["up3"], sd, name)
    g["hm_sigmoid"] = O.sigmoid_clamp(g["hm"])
    return {k2: (v.numpy() if hasattr(v, "numpy") else v) for k2, v in g.items()}


def _as_fused(g, dtype):
    """The same tensors as the DEFAULT plan of ``dtype`` would record them: what a fused launch keeps on chip is left out."""
    names = X.plan_entries(dtype)
    keep = {"img_u8", "hm", "wh", "lm", "reg", "hm_sigmoid", "layer0.0"}
    for n in names:
        if n.endswith(".mbconv") or n.endswith(".project"):
            keep.add(n.rsplit(".", 1)[0])
        elif n.endswith(".expand+dw"):
            keep.add(n.rsplit(".", 1)[0] + ".dw")
        elif n in g:
            keep.add(n)
    out = {k2: v for k2, v in g.items() if k2 in keep}
    if "conv_last+up1+up2" in names:
        out["up2"], out["neck_fused"] = g["up2"], True
    if "up3+heads" in names:
        out["uphead_fused"] = True
    return out, names


@pytest.fixture(scope="module")
def exact_oracle_records():
    import torch
    from oracle import centerface_oracle as O
    torch.manual_seed(0)
    sd = O.to_torch_sd(cfa.weights.synthetic_state_dict(0))
    rng = np.random.default_rng(96 + 3 * 128)
    img = rng.integers(0, 256, (2, 96, 128, 3), dtype=np.uint8)
    return sd, img, _oracle_record(sd, img)


def test_exact_layer_check_is_tied_to_the_pinned_oracle(exact_oracle_records):
    """``exact_cases.check_layers64`` on the pinned float32 oracle's own features (two random uint8 images, 96x128), fed in as if they
    were an engine's: float32 round-off is all that separates them from the float64 restatement, <= 0.25 of every bound (measured
    <= 0.08).  The launch-by-launch float32 run that supplies the tensors ``O.forward`` does not expose (up1, up2, the expanded and
    depthwise tensors) reproduces every feature ``O.forward`` does expose bit for bit, so each entry ends in a pinned tensor; the
    fused entries of both default plans are checked on the same tensors."""
    import torch
    from oracle import centerface_oracle as O
    sd, img, g = exact_oracle_records
    out, feats = O.forward(sd, torch.from_numpy(np.concatenate([O.preprocess(im) for im in img])), return_features=True)
    for k2, v in list(feats.items()) + list(out.items()):
        assert np.array_equal(v.numpy(), g["first_conv" if k2 == "stem" else k2]), k2
    ratios = X.check_layers64(sd, g, "fp32")
    assert sorted(ratios) == sorted(X.plan_entries("fp32", fuse=False) + ["hm_sigmoid"]) and len(ratios) == 3 + 33 + 5 + 1
    for dtype in X.DTYPES:
        gf, names = _as_fused(g, dtype)
        r = X.check_layers64(sd, gf, dtype)
        assert sorted(r) == sorted(names + ["hm_sigmoid"]), sorted(r)
        ratios.update({"%s/%s" % (dtype, k2): v for k2, v in r.items() if k2 not in ratios})
    for k2, v in ratios.items():
        print("EXACTLAYERS oracle 96x128 %s %.4f" % (k2, v))
    assert max(ratios.values()) <= 0.25, {k2: v for k2, v in ratios.items() if v > 0.25}


@pytest.mark.parametrize("defect,entry", [("dw_tap", "layer3.1.mbconv"), ("k_chunk", "layer5.1.project"), ("stem_pad", "first_conv+layer0.0")])
def test_exact_layer_check_sees_one_injected_defect(exact_oracle_records, defect, entry):
    """One wrong step in an otherwise correct float32 network -- a depthwise tap taken from the neighbouring column on the last
    output column only, the last 8 input channels of a project GEMM dropped, the stem's zero pad replaced by edge replication --
    puts the entry that holds it (a fused block, a single GEMM, the fused stem) more than 100 bounds out.  Teacher forcing keeps it
    there: every entry upstream keeps its ratio to the bit, every entry downstream (whose inputs are now the defective network's
    tensors) stays within the 0.25 of a correct one."""
    sd, img, good = exact_oracle_records
    dtype = "fp32_split" if entry.endswith(".project") else "fp32"           # (the default plan that runs the entry as a launch of its own)
    gf, _ = _as_fused(_oracle_record(sd, img[:1], defect), dtype)
    ref, _ = _as_fused(_oracle_record(sd, img[:1]), dtype)
    r, r0 = X.check_layers64(sd, gf, dtype), X.check_layers64(sd, ref, dtype)
    assert r[entry] > 100.0 and r0[entry] <= 0.25, (entry, r[entry], r0[entry])
    names = list(r)
    assert names == list(r0)
    for n in names[:names.index(entry)]:
        assert r[n] == r0[n], (n, r[n], r0[n])
    others = {n: v for n, v in r.items() if n != entry}
    assert max(others.values()) <= 0.25, {n: v for n, v in others.items() if v > 0.25}
    print("EXACTLAYERS defect %s %s %.1f" % (defect, entry, r[entry]))


def test_exact_plans_pick_the_expected_family_per_block():
    """Which kernel family serves each of the 11 backbone blocks behind the fused stem, in both modes (``exact_cases.PLAN``, from which
    tests/test_exact_layers.py takes the plan entries and kernel names it expects): the fused pick, and the engine's rule for
    splitting a block -- no fused family, or Cout > 64 where the expand+depthwise family has the shape."""
    for dtype in X.DTYPES:
        assert [p for p, _ in X.PLAN[dtype]] == [b[0] for b in X.BLOCKS[1:]]
        for (prefix, cin, cout, t, k, s), (_, fam) in zip(X.BLOCKS[1:], X.PLAN[dtype]):
            mb = cfa.ops.mbconv_pick(cin, cin * t, cout, k, s, dtype)
            xd = cfa.ops.expand_dw_pick(cin, cin * t, k, s, dtype)
            assert xd["ok"] == (dtype == "fp32_split" and cout > 64) and (not xd["ok"] or xd["kind"] == "XD_F32"), (dtype, prefix, xd)
            have = "XD_F32" if (xd["ok"] and (cout > 64 or not mb["ok"])) else mb["kind"]
            assert have == fam and mb["ok"] == (cout <= 96), (dtype, prefix, mb, xd)
    assert len(X.plan_entries("fp32")) == 1 + 8 + 9 + 5 and len(X.plan_entries("fp32_split")) == 1 + 6 + 10 + 2
    assert len(X.plan_entries("fp32_split", neck=False, uphead=False)) == 1 + 6 + 10 + 5
