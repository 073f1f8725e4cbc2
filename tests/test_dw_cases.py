"""The GPU-less half of the standalone-depthwise sweep (tests/test_dw_sweep.py): ``cf_op_dw_pick`` -- the host half of
``launch_dw`` -- against the case table of tests/dw_cases.py, the refusals, the sensitivity of the sweep's bounds to the faults
this kernel family is prone to, and the float64 restatement against the oracle.  No compute calls here."""
import ctypes
import math

import numpy as np
import pytest
import torch

import centerface_amd as cfa
from centerface_amd import ops
from oracle import bf16_emulation as E
from oracle import centerface_oracle as O

import dw_cases as D
from test_abi import _declared_symbols

F32 = dict(rtol=2e-5, atol=2e-5)          # the fp32 bound of the depthwise tests (tests/test_gpu_parity.py)


def _pick(c, **over):
    _, dtype, C, H, W, k, s, pad, act, bias, B = c[:11]
    a = dict(C_=C, H=H, W=W, k=k, stride=s, pad=D.pads(k, s, pad), dtype=dtype, B=B, act=act, bias=bias)
    a.update(over)
    return ops.dw_pick(**a)


def _primes(n):
    return n > 1 and all(n % q for q in range(2, int(math.isqrt(n)) + 1))


# ------------------------------------------------------------------------------- the hook
def test_dw_pick_is_declared_exported_and_needs_no_gpu():
    L = cfa._lib.lib()
    assert "cf_op_dw_pick" in _declared_symbols() and "cf_op_dw_pick" in cfa._lib.EXPORTS and hasattr(L, "cf_op_dw_pick")
    out = (ctypes.c_int * 16)()
    assert L.cf_op_dw_pick(7, 1, 16, 9, 9, 3, 1, 1, 1, 1, 0, out, None, 0) == -1          # unknown dtype
    assert L.cf_op_dw_pick(0, 1, 16, 9, 9, 3, 1, 1, 1, 1, 0, None, None, 0) == -1         # no out
    assert L.cf_op_dw_pick(0, 0, 16, 9, 9, 3, 1, 1, 1, 1, 0, out, None, 0) == -1          # no image
    assert L.cf_op_dw_pick(0, 1, 16, 9, 9, 3, 1, 1, 1, 1, 0, out, None, 0) == 0 and out[0] == 1 and out[6] == 16      # (the tag is optional)
    # layer1.0's depthwise at 640 x 640, B = 64, bf16: what DESIGN.md and profiles/r06_dw_xcd.md describe
    g = ops.dw_pick(96, 320, 320, 3, 2, dtype="bf16", B=64)
    assert g == dict(ok=True, strip=0, k=3, s=2, TH=4, TW=32, Cc=32, nchunk=3, cpp=4, threads=256, lds_bytes=39040, ntx=5, nty=40,
                     workgroups=64 * 3 * 5 * 40, Ho=160, Wo=160, tag=D.full_tag("lds<3,2,4,32>", "bf16", "swish", False))
    # the budget edge the 16 x 32 tile was tuned to: 48 bf16 channels fill 61440 of 61440 bytes
    g = ops.dw_pick(48, 3, 256, 3, 1, dtype="bf16")
    assert (g["Cc"], g["lds_bytes"], g["tag"]) == (48, 61440, D.full_tag("strip<3,1,16,32>", "bf16", "swish", False))
    # one image of 4 GiB or more in the storage type is refused (32-bit byte offsets inside an image): 2^32 bytes in fp32, half in bf16
    assert not ops.dw_pick(8, 16384, 8192, 3, 1, dtype="fp32")["ok"] and ops.dw_pick(8, 16384, 8192, 3, 1, dtype="bf16")["ok"]
    assert ops.dw_pick(8, 16384, 8191, 3, 1, dtype="fp32")["ok"] and not ops.dw_pick(16, 16384, 8192, 3, 1, dtype="bf16")["ok"]
    # fp32_split is fp32 storage here: the same choice
    a, b = ops.dw_pick(96, 40, 40, 5, 2, dtype="fp32"), ops.dw_pick(96, 40, 40, 5, 2, dtype="fp32_split")
    assert a == b and a["ok"]


# ------------------------------------------------------------------------------- the table
def test_dw_table_is_well_formed():
    assert len(set(D.IDS)) == len(D.IDS) >= 250
    for c in D.CASES:
        cid, dtype, C, H, W, k, s, pad, act, bias, B, short, Cc, nchunk, threads = c
        assert dtype in D.DTYPES and k in (3, 5) and s in (1, 2) and pad in ("same", "sym") and act in ("none", "swish"), cid
        assert B * C * H * W < 2_000_000, cid                                   # the size limit of a case
        assert max(H, W) < 640 and min(H, W) <= 60 and (H, W) not in ((320, 320), (160, 160)), cid      # no production map
        assert B in (1, 2, 3) and C % 8 == 0 and C == Cc * nchunk, cid
        assert short in [row[0] for row in D.INSTANCES.values()], cid
        if cid[0] != "X":
            assert D.INSTANCES[cid[0]][0] == short and cid[1] == dtype[0], cid
    assert all(D.case(cid)[1] == "fp32" for cid in D.SPLIT_CASES)
    assert sorted(D.letter_of(D.case(cid)[11]) for cid in D.SPLIT_CASES) == sorted(D.INSTANCES)


def test_every_dw_case_lands_where_its_row_says():
    """(tag, Cc, nchunk, threads) of every row against ``ops.dw_pick``, and the output map against the class the picker's table
    gives the instance: a retuned table cannot silently move a case."""
    for c in D.CASES:
        cid, dtype, C, H, W, k, s, pad, act, bias, B, short, Cc, nchunk, threads = c
        g = _pick(c)
        assert g["ok"], cid
        assert g["tag"] == D.full_tag(short, dtype, act, bias), (cid, g["tag"])
        assert (g["Cc"], g["nchunk"], g["threads"]) == (Cc, nchunk, threads), (cid, g)
        name, ik, is_, th, tw = D.parse_instance(short)
        assert (g["strip"], g["k"], g["s"], g["TH"], g["TW"]) == (int(name == "strip"), ik, is_, th, tw) and (ik, is_) == (k, s), cid
        p = D.pads(k, s, pad)
        assert (g["Ho"], g["Wo"]) == (D.out_size(H, k, s, p), D.out_size(W, k, s, p)), cid
        assert D.INSTANCES[D.letter_of(short)][2](g["Ho"], g["Wo"]), cid
        assert (g["ntx"], g["nty"]) == (-(-g["Wo"] // tw), -(-g["Ho"] // th)) and g["workgroups"] == B * nchunk * g["ntx"] * g["nty"], cid
        assert g["cpp"] * (8 if dtype == "bf16" else 4) == Cc and g["lds_bytes"] <= D.INSTANCES[D.letter_of(short)][1] * 1024 + k * k * Cc * 4, cid


def _achievable(letter, dtype, Ho, Wo):
    """(cpp values, thread counts, largest Cc) the instance can be made to run with on an Ho x Wo output, over C = 8 ... 1024."""
    short = D.INSTANCES[letter][0]
    _, k, s, th, tw = D.parse_instance(short)
    H, W = (Ho, Wo) if s == 1 else (2 * Ho, 2 * Wo)
    cpps, thr, cmax = set(), set(), 0
    for C in range(8, 1025, 8):
        g = ops.dw_pick(C, H, W, k, s, pad=D.pads(k, s, "sym"), dtype=dtype)
        assert g["ok"] and g["tag"] == D.full_tag(short, dtype, "swish", False), (letter, C)
        cpps.add(g["cpp"]); thr.add(g["threads"]); cmax = max(cmax, g["Cc"])
    return cpps, thr, cmax


@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("letter", list(D.INSTANCES))
def test_dw_table_visits_every_item_for_each_instance(letter, dtype):
    """Map sizes, channel geometry, work lists, padding and epilogues: the list of the module docstring of tests/dw_cases.py, per
    instance and storage type."""
    short, cap_kb, cls = D.INSTANCES[letter]
    name, k, s, TH, TW = D.parse_instance(short)
    rows = [(c, _pick(c)) for c in D.CASES if c[11] == short and c[1] == dtype]
    assert len(rows) >= 10
    widths = [w for w in range(1, 600) if cls(TH + 1 if letter != "G" else 11, w)]
    w_lo = widths[0]

    def some(what, pred):
        hits = [c[0] for c, g in rows if pred(c, g)]
        assert hits, "%s %s: no case with %s" % (short, dtype, what)
        return hits

    # ---- map sizes (the smallest at which the edge logic is live, Wo inside the class)
    h_lo = 9 if letter == "G" else 1
    some("one output row", lambda c, g: g["Ho"] == h_lo and g["nty"] == 1)
    # (a class that starts above one tile: one column more than its first width -- a partial last tile; G's class ends at its tile)
    w_t1 = w_lo + 1 if w_lo > 1 else TW + 1 if TW + 1 in widths else widths[-1]
    some("one row and one column more than a tile", lambda c, g: (g["Ho"], g["Wo"]) == (TH + 1, w_t1))
    if w_lo == 1 and letter != "G":
        some("four tiles", lambda c, g: (g["ntx"], g["nty"]) == (2, 2))
    w_tm = TW - 1 if cls(TH - 1, TW - 1) else w_lo
    some("a tile - 1", lambda c, g: (g["Ho"], g["Wo"]) == (TH - 1, w_tm))
    if name == "strip":
        for r in (1, 2, 3):
            some("Wo %% 4 = %d" % r, lambda c, g: g["Wo"] % 4 == r)
    if cls(1, 1):
        some("a 1 x 1 input", lambda c, g: (c[3], c[4]) == (1, 1) and (g["Ho"], g["Wo"]) == (1, 1))
    # ---- channel geometry
    cpps, thr, cmax = _achievable(letter, dtype, TH + 1, w_t1)
    assert (1 in cpps) == (dtype == "bf16") and 2 in cpps
    for cpp in sorted(cpps & {1, 2, 3}):
        some("cpp = %d" % cpp, lambda c, g: g["cpp"] == cpp)
    if name == "strip":
        for t in sorted(thr):
            some("%d-thread workgroups" % t, lambda c, g: g["threads"] == t)
        if (TH, TW) == (10, 20):
            assert thr == {64, 128, 192, 256} if dtype == "bf16" else thr >= {128, 256}
            for cpp, t in ((1, 64), (2, 128), (3, 192)):
                assert all(g["threads"] == t for c, g in rows if g["cpp"] == cpp)
    else:
        assert thr == {256}
    some("a C that fits whole", lambda c, g: g["nchunk"] == 1)
    P = 8 if dtype == "bf16" else 4
    for cid in some("C at the LDS-budget edge", lambda c, g: g["Cc"] == cmax and g["nchunk"] >= 2):
        c, g = next(r for r in rows if r[0][0] == cid)
        assert g["lds_bytes"] <= cap_kb * 1024 + (0 if name == "strip" else k * k * cmax * 4)
        # one more 16-byte group: C = 2 (cmax + P) has no divisor between itself and cmax + P, so a chunk of cmax + P would be taken if
        # the budget held it
        over = _pick(c, C_=2 * (cmax + P))
        assert over["ok"] and over["Cc"] < cmax + P and over["nchunk"] > 2, (cid, over)
    some("C = 8 x prime in one-group chunks, an odd work list",
         lambda c, g: _primes(c[2] // 8) and g["Cc"] == 8 and g["nchunk"] == c[2] // 8 >= 37 and g["workgroups"] % 2 == 1 and g["workgroups"] % 8 != 0)
    # ---- work list
    if letter != "A":                                 # (A's class starts at 256 columns: eight tiles per row)
        some("fewer than 8 workgroups", lambda c, g: g["workgroups"] < 8)
    some("8 n + r workgroups, r != 0", lambda c, g: g["workgroups"] > 8 and g["workgroups"] % 8 != 0)
    some("B = 3", lambda c, g: c[10] == 3)
    assert all(c[10] in (2, 3) or (c[10] == 1 and g["workgroups"] < 8 and 2 * g["workgroups"] >= 8) for c, g in rows)
    # ---- padding
    some("the reference's pad", lambda c, g: c[7] == "same")
    some("the ShuffleV2 pad", lambda c, g: c[7] == "sym")
    if s == 2:
        assert D.pads(k, 2, "same")[0] != D.pads(k, 2, "same")[1]          # (asymmetric)
        for pad in ("same", "sym"):
            some("odd inputs, %s" % pad, lambda c, g: c[7] == pad and c[3] % 2 == 1)
            some("even inputs, %s" % pad, lambda c, g: c[7] == pad and c[3] % 2 == 0 and c[4] % 2 == 0)
            some("odd width, %s" % pad, lambda c, g: c[7] == pad and c[4] % 2 == 1)
    # ---- epilogue
    for act, bias in ((("none", True), ("swish", False)) if s == 1 else (("none", False), ("none", True), ("swish", False), ("swish", True))):
        some("act %s, bias %s" % (act, bias), lambda c, g: (c[8], c[9]) == (act, bias))
    some("the ShuffleV2 flavour: no activation, bias, k // 2 on both sides", lambda c, g: (c[7], c[8], c[9]) == ("sym", "none", True))


@pytest.mark.parametrize("dtype", D.DTYPES)
def test_dw_table_stands_on_both_sides_of_every_class_boundary(dtype):
    seen = {}
    for c in D.CASES:
        if c[1] == dtype:
            g = _pick(c)
            seen.setdefault((c[5], c[6]), set()).add((g["Ho"], g["Wo"], c[11]))

    def at(k, s, wo=None, ho=None):
        inst = {i for (h, w, i) in seen[(k, s)] if (wo is None or w == wo) and (ho is None or h == ho)}
        assert len(inst) == 1, (k, s, ho, wo, inst)
        return inst.pop()
    assert [at(3, 1, w) for w in (95, 96, 255, 256)] == ["strip<3,1,10,20>", "strip<3,1,8,40>", "strip<3,1,8,40>", "strip<3,1,16,32>"]
    assert [at(5, 1, w) for w in (31, 32, 63, 64)] == ["strip<5,1,10,20>", "strip<5,1,20,20>", "strip<5,1,20,20>", "strip<5,1,16,16>"]
    assert [at(3, 2, w) for w in (63, 64)] == ["lds<3,2,4,16>", "lds<3,2,4,32>"]
    assert [at(5, 2, w) for w in (63, 64)] == ["lds<5,2,4,32>", "lds<5,2,8,16>"]
    assert [at(3, 2, w, h) for h, w in ((8, 20), (9, 20), (20, 20), (21, 20), (20, 21))] == [
        "lds<3,2,4,16>", "lds<3,2,10,20>", "lds<3,2,10,20>", "lds<3,2,4,16>", "lds<3,2,4,16>"]


# ------------------------------------------------------------------------------- refusals
def test_dw_refusals_need_no_gpu_and_fill_no_output():
    L, p = cfa._lib.lib(), cfa._lib.ptr
    for what, (dtype, C, H, W, k, s, pad) in D.REFUSED.items():
        assert ops.dw_pick(C, H, W, k, s, pad=pad, dtype=dtype) == dict(
            ok=False, tag=None, strip=0, k=0, s=0, TH=0, TW=0, Cc=0, nchunk=0, cpp=0, threads=0, lds_bytes=0, ntx=0, nty=0, workgroups=0, Ho=0, Wo=0), what
        x, w = np.ones((1, C, H, W), np.float32), np.ones((C, 1, k, k), np.float32)
        y = np.full(4 * C * (H + 4) * (W + 4), 7.0, np.float32)                # larger than any output size either side could mean
        assert L.cf_op_dwconv(0, ops._DT[dtype], p(x), p(w), None, p(y), 1, C, H, W, k, s, pad[0], pad[1], 1) == -1, what
        assert (y == 7.0).all(), what
        with pytest.raises(cfa._lib.CenterFaceValueError):
            ops.conv_dw(x, w, k, s, pad=pad, dtype=dtype)
    # an activation code the kernels have no instance for
    x, w, y = np.ones((1, 8, 4, 4), np.float32), np.ones((8, 1, 3, 3), np.float32), np.full(8 * 16, 7.0, np.float32)
    assert L.cf_op_dwconv(0, 0, p(x), p(w), None, p(y), 1, 8, 4, 4, 3, 1, 1, 1, 2) == -1 and (y == 7.0).all()


# ------------------------------------------------------------------------------- what the bounds can see
SENSITIVITY_CASE = "Cb-edge"      # 3x3 stride 1 on the 10 x 20 tile, two channel chunks of 80, 5 x 21 outputs in two tile columns


def _faults(cid):
    """The float64 reference of a case, and the same with each of the faults this family is prone to."""
    _, dtype, C, H, W, k, s, pad, act, bias, B, short, Cc, nchunk, threads = D.case(cid)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    w = (rng.standard_normal((C, 1, k, k)) * 0.3).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    p = D.pads(k, s, pad)
    ref = D.ref64(x, w, k, s, p, act, b)
    out = {}
    # one wrong tap on one output column: the column's last tap of the first kernel row takes the weight of the tap before it
    w1 = w.copy()
    w1[:, 0, 0, k - 1] = w[:, 0, 0, k - 2]
    out["one wrong tap on one output column"] = ref.copy()
    out["one wrong tap on one output column"][:, :, :, 7] = D.ref64(x, w1, k, s, p, act, b)[:, :, :, 7]
    # the pad shifted by one (the same output size)
    out["a pad shifted by one"] = D.ref64(x, w, k, s, (p[0] + 1, p[1] - 1), act, b)
    # the last channel chunk read from pixel 0 (round 6's magic_div(1): every 16-byte chunk of the tile fetched from its first pixel)
    x0 = x.copy()
    x0[:, -Cc:] = x[:, -Cc:, :1, :1]
    out["a channel chunk read from pixel 0"] = D.ref64(x0, w, k, s, p, act, b)
    # every chunk with the bias of the chunk after it
    out["the bias of the neighbouring chunk"] = D.ref64(x, w, k, s, p, act, np.roll(b, -Cc))
    return ref, out, Cc


def test_dw_sweep_bounds_see_the_faults_of_this_family():
    """Each injected fault, as a multiple of the fp32 bound and of the bf16 tolerance of the sweep: all above 10 bounds (measured here:
    the factors are printed), and the bf16 acceptance rule rejects each of them."""
    ref, faults, Cc = _faults(SENSITIVITY_CASE)
    assert D.parse_instance(D.case(SENSITIVITY_CASE)[11])[3:] == (10, 20) and D.case(SENSITIVITY_CASE)[13] >= 2
    assert len(faults) == 4
    for what, bad in faults.items():
        d = np.abs(bad - ref)
        f32 = d / (F32["atol"] + F32["rtol"] * np.abs(ref))
        b16 = d / E.tolerance(ref)
        print("DWSENS %s: %.0f fp32 bounds, %.1f bf16 tolerances, %.1f %% of the elements beyond one" % (what, f32.max(), b16.max(), 100.0 * (b16 > 1).mean()))
        assert f32.max() >= 10.0 and b16.max() >= 10.0, what
        stat = (float(b16.max()), float((b16 > 1).mean()), float((b16 > 0.5).mean()), float((b16 > 0).mean()), int(b16.size))
        assert not E.accept(stat, True), what
        # ... and the edge slices name it: at least one slice of the sweep sees it on its own
        assert any((part_d / (F32["atol"] + F32["rtol"] * np.abs(part_r))).max() >= 10.0
                   for (_, part_d), (_, part_r) in zip(D.edges(d, Cc), D.edges(ref, Cc))), what


# ------------------------------------------------------------------------------- the restatement against the oracle
@pytest.mark.parametrize("C,k,s,H", [(96, 3, 2, 320), (32, 3, 1, 320), (144, 3, 1, 160), (192, 5, 1, 80), (144, 5, 2, 160), (960, 3, 1, 20)])
def test_dw_ref64_is_the_oracles_depthwise_on_the_production_shapes(C, k, s, H):
    """``dw_cases.ref64`` against the oracle's ZeroPad2d -> depthwise Conv2d -> Swish (oracle/centerface_oracle.py: same_pad,
    conv_swish) in float64 on the six standalone production shapes, one image each: within 1e-6."""
    rng = np.random.default_rng(C + 7 * k + s)
    x = rng.standard_normal((1, C, H, H)).astype(np.float32)
    w = (rng.standard_normal((C, 1, k, k)) * 0.3).astype(np.float32)
    want = O.conv_swish(torch.from_numpy(x).double(), torch.from_numpy(w).double(), k, s, groups=C).numpy()
    got = D.ref64(x, w, k, s, D.pads(k, s, "same"))
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-6
