"""The threshold decode and its greedy NMS on the device (thresh_collect / thresh_rank / thresh_mask / thresh_sweep, csrc/cf_decode.hip)
against the project's plain statements, at the candidate counts, ties and suppression chains of tests/nms_cases.py: every count on a
block (64), rank-chunk (4096), workspace (4096) and propagation-path (nw 17 / 18, 65 / 66) boundary, both overlap measures, the
truncated outputs, heat maps with an exact number of cells above the threshold, batches of unequal counts, and the engine's own decode
(dense heat plane, persistent workspace, rescale in the kernel).  tests/test_nms_cases.py shows on the CPU that these cases change their
result under each of ten subtle kernel defects.

Everything here is selection and float32 arithmetic without contraction: EVERY comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import eval_widerface as ew
from centerface_amd import ops
from oracle import centerface_oracle as O

import nms_cases as N

pytestmark = pytest.mark.gpu
f32 = np.float32


def say(cid, n, kept):
    print("NMSSWEEP %s n=%d kept=%d" % (cid, n, kept))


# ------------------------------------------------------------------------------------------ the NMS stages alone (cf_op_nms, IoU)
@pytest.mark.parametrize("n", N.NS)
@pytest.mark.parametrize("family", sorted(N.FAMILIES))
def test_nms_stages_keep_what_nms_greedy_keeps(family, n):
    b, s = N.family_case(family, n)
    for thr in N.THRESHOLDS:
        want = N.family_reference(family, n, thr)
        got = ew.nms(b, s, thr)
        say("%s-%d@%.1f" % (family, n, thr), n, len(got))
        assert got == want, (family, n, thr, len(got), len(want))


def test_nms_through_the_detector_class_is_the_same_op():
    b, s = N.family_case("random", 1089)
    got = cfa.CenterFace.nms(type("dev", (), {"device": 0})(), b, s, 0.3)
    say("random-1089@0.3 (CenterFace.nms)", 1089, len(got))
    assert [int(k) for k in got] == N.family_reference("random", 1089, 0.3)


@pytest.mark.parametrize("pos", N.EXACT_POS)
def test_overlap_equal_to_the_threshold_suppresses_and_the_next_float_does_not(pos):
    """`ovr >= thresh` at equality: IoU 100 / 200 = 0.5 exactly, with the pair inside a block, on its last bit, across the 64 boundary."""
    b, s = N.exact_case("iou", pos)
    for thr in (0.5, N.HALF_UP):
        got = ew.nms(b, s, thr)
        say("exact-iou-%d@%.9g" % (pos, thr), len(s), len(got))
        assert got == N.reference_keep(b, s, thr, key=("exact", "iou", pos)) == N.exact_want(pos, thr)


# ------------------------------------------------------------------------------------------ IoS: the merge with the identity mapping
FRAME = (256, 256)                                       # one rectangle = the frame = the network input, edge 0: the merge is the NMS stages


def merge_identity(b, s, l, thr, max_out, fill=None):
    n = len(s)
    kw = {}
    if fill is not None:
        kw = dict(dets=np.full((1, max_out, 5), fill, np.float32), lms=np.full((1, max_out, 10), fill, np.float32))
    od, ol, oc, fl = ops.merge_tiles([(0, 0, FRAME[1], FRAME[0])], FRAME, FRAME, b.reshape(1, 1, n, 4), s.reshape(1, 1, n), l.reshape(1, 1, n, 10),
                                     [[n]], max_out, metric="ios", thresh=thr, edge=0.0, **kw)
    assert fl.tolist() == [0]
    return od[0], ol[0], int(oc[0])


def ios_rows(b, s, l, keep):
    return np.concatenate([b[keep], s[keep][:, None]], 1).astype(np.float32), l[keep]


@pytest.mark.parametrize("n", N.NS)
@pytest.mark.parametrize("family", N.IOS_FAMILIES)
def test_merge_with_identity_mapping_keeps_what_the_ios_restatement_keeps(family, n):
    b, s = N.family_case(family, n)
    l = N.landmarks_for(n)
    for thr in N.THRESHOLDS:
        keep = N.family_reference(family, n, thr, "ios")
        wd, wl = ios_rows(b, s, l, keep)
        d, lm, cnt = merge_identity(b, s, l, thr, n)
        say("%s-ios-%d@%.1f" % (family, n, thr), n, cnt)
        assert cnt == len(keep), (family, n, thr, cnt, len(keep))
        assert d[:cnt].tobytes() == wd.tobytes() and lm[:cnt].tobytes() == wl.tobytes(), (family, n, thr)
        assert not d[cnt:].any() and not lm[cnt:].any()                      # the wrapper's zero fill, untouched


@pytest.mark.parametrize("pos", N.EXACT_POS)
def test_ios_equal_to_the_threshold_suppresses_and_the_next_float_does_not(pos):
    """IoS 50 / 100 = 0.5 exactly (IoU 0.2; over the larger area it would be 0.25)."""
    b, s = N.exact_case("ios", pos)
    l = N.landmarks_for(len(s), 1)
    for thr in (0.5, N.HALF_UP):
        keep = N.reference_keep(b, s, thr, "ios", key=("exact", "ios", pos))
        assert keep == N.exact_want(pos, thr)
        wd, wl = ios_rows(b, s, l, keep)
        d, lm, cnt = merge_identity(b, s, l, thr, len(s))
        say("exact-ios-%d@%.9g" % (pos, thr), len(s), cnt)
        assert cnt == len(keep) and d[:cnt].tobytes() == wd.tobytes() and lm[:cnt].tobytes() == wl.tobytes()


# ------------------------------------------------------------------------------------------ truncation
@pytest.mark.parametrize("max_out", (1, 63, 64, 65))
def test_merge_truncated_below_the_kept_count(max_out):
    """Counts report every kept row; the rows below max_out are the reference's first rows; with room to spare the rows at and behind the
    count come back as the caller's fill bytes."""
    for family, n in (("pool67", 4161), ("random", 1089)):
        b, s = N.family_case(family, n)
        l = N.landmarks_for(n)
        keep = N.family_reference(family, n, 0.5, "ios")
        assert len(keep) > 65
        wd, wl = ios_rows(b, s, l, keep)
        d, lm, cnt = merge_identity(b, s, l, 0.5, max_out, fill=-7.25)
        say("%s-ios-%d max_out=%d" % (family, n, max_out), n, cnt)
        assert cnt == len(keep)
        assert d.tobytes() == wd[:max_out].tobytes() and lm.tobytes() == wl[:max_out].tobytes()
        room = len(keep) + max_out
        d, lm, cnt = merge_identity(b, s, l, 0.5, room, fill=-7.25)
        assert cnt == len(keep) and d[:cnt].tobytes() == wd.tobytes() and lm[:cnt].tobytes() == wl.tobytes()
        assert d[cnt:].tobytes() == np.full((max_out, 5), -7.25, np.float32).tobytes()
        assert lm[cnt:].tobytes() == np.full((max_out, 10), -7.25, np.float32).tobytes()


# ------------------------------------------------------------------------------------------ collect + NMS on maps (cf_op_decode_threshold_ex)
def decode_op(mode, maps, max_out, nms_thresh=0.3, thr=N.MAP_THRESH):
    """cf_op_decode_threshold_ex on a list of map cases of one shape: (dets [B,max_out,5], lms [B,max_out,10], counts [B]); the output
    arrays are handed over full of 0xAB bytes."""
    hm, wh, reg, lm = (np.ascontiguousarray(np.concatenate([m[k] for m in maps])) for k in ("hm", "wh", "reg", "lm"))
    B, _, h, w = hm.shape
    dets, lms = (np.full(B * max_out * k * 4, 0xAB, np.uint8).view(np.float32).reshape(B, max_out, k) for k in (5, 10))
    cnt = np.full(B, -1, np.int32)
    ih, iw = maps[0]["size"]
    rc = cfa._lib.lib().cf_op_decode_threshold_ex(0, mode, cfa._lib.ptr(hm), cfa._lib.ptr(wh), cfa._lib.ptr(reg), cfa._lib.ptr(lm), B, h, w, ih, iw,
                                                  C.c_float(thr), C.c_float(nms_thresh), max_out, cfa._lib.ptr(dets), cfa._lib.ptr(lms), cfa._lib.ptr(cnt))
    assert rc == 0, cfa._lib.lib().cf_op_last_error()
    return dets, lms, cnt


def check_maps(cid, shape, counts, mode):
    h, w = shape
    maps = [N.map_case(h, w, c) for c in counts]
    want = [N.map_reference(h, w, c, mode) for c in counts]
    max_out = max(len(d) for d, _ in want) + 2            # two rows of room: the op's zero fill must show behind every image's rows
    dets, lms, cnt = decode_op(mode, maps, max_out)
    for b, (wd, wl) in enumerate(want):
        say("%s[%d]-d%d" % (cid, b, mode + 1), counts[b], int(cnt[b]))
        assert int(cnt[b]) == len(wd), (cid, b, mode, int(cnt[b]), len(wd))
        assert dets[b, :len(wd)].tobytes() == wd.tobytes(), (cid, b, mode)
        assert lms[b, :len(wd)].tobytes() == wl.tobytes(), (cid, b, mode)
        assert not dets[b, len(wd):].view(np.uint32).any() and not lms[b, len(wd):].view(np.uint32).any(), (cid, b, mode)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("h,w,ncand", N.MAP_SHAPES)
def test_decode_on_maps_with_an_exact_candidate_count(h, w, ncand, mode):
    check_maps("map-%dx%d-%d" % (h, w, ncand), (h, w), (ncand,), mode)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("shape,counts", N.MAP_BATCHES)
def test_decode_on_batches_of_unequal_candidate_counts(shape, counts, mode):
    """(0, 4097, 65): one image forces the grow-and-rerun and all three must come out right; (4096, 63): the count equals the capacity."""
    check_maps("batch-%dx%d-%s" % (shape + ("+".join(map(str, counts)),)), shape, counts, mode)


@pytest.mark.parametrize("max_out", (1, 63, 64, 65))
def test_decode_truncated_below_the_kept_count(max_out):
    """Counts report every kept row, the rows below max_out are the reference's first rows (and there are no others)."""
    h, w, ncand = 25, 41, 1025
    for mode in (0, 1):
        wd, wl = N.map_reference(h, w, ncand, mode)
        assert len(wd) > 65
        dets, lms, cnt = decode_op(mode, [N.map_case(h, w, ncand)], max_out)
        say("map-%dx%d-%d-d%d max_out=%d" % (h, w, ncand, mode + 1, max_out), ncand, int(cnt[0]))
        assert int(cnt[0]) == len(wd)
        assert dets[0].tobytes() == wd[:max_out].tobytes() and lms[0].tobytes() == wl[:max_out].tobytes()


# ------------------------------------------------------------------------------------------ the engine's own decode
def engine_case(H, W, dtype, B=3, seed=11):
    """An engine with the synthetic weights after one forward of B random frames, its own head maps, and a score threshold read off
    them so that every image has more than 64 cells above it and at least one has more than 128.  The size head's bias is raised (boxes
    of some 9 x 13 pixels on the 4-pixel grid instead of a pixel or two), so that neighbouring candidates overlap and the NMS has work."""
    rng = np.random.default_rng(seed + H)
    x = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    sd = dict(cfa.weights.synthetic_state_dict(0))
    sd["wh.1.bias"] = (np.asarray(sd["wh.1.bias"], np.float32) + np.float32([2.0, 3.0])).astype(np.float32)
    eng = cfa.Engine(H, W, max_batch=B, dtype=dtype, weights=sd)
    eng.forward_enqueue(x)
    g = eng.heads(sigmoid_hm=True)
    hm = np.sort(g["hm_sigmoid"].reshape(B, -1), 1)[:, ::-1]
    thr = min(float(hm[:, 65].min()), float(hm[:, 129].max()))      # the value of a cell: that cell is ON the threshold and stays out (`>`)
    above = (g["hm_sigmoid"].reshape(B, -1) > f32(thr)).sum(1)
    assert (hm == f32(thr)).any()
    print("engine %dx%d %s: threshold %.9g, cells above it per image: %s" % (H, W, dtype, thr, above.tolist()))
    assert above.min() > 64 and above.max() > 128, above
    return eng, x, g, thr, sd


def oracle_rows(g, b, size, thr, mode):
    if mode == "d1":
        d, l = O.decode_d1(g["hm_sigmoid"][b:b + 1], g["wh"][b:b + 1], g["reg"][b:b + 1], g["lm"][b:b + 1], size, fixed_threshold=f32(thr))
        return np.asarray(d, np.float32).reshape(-1, 5), np.asarray(l, np.float32).reshape(-1, 10)
    d = O.decode_d2(g["hm_sigmoid"][b], g["wh"][b], g["reg"][b], size, threshold=f32(thr))
    return np.asarray(d, np.float32).reshape(-1, 5), None


@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
@pytest.mark.parametrize("H,W", ((96, 128), (160, 224)))
def test_engine_decode_equals_the_oracle_on_its_own_head_maps(H, W, dtype):
    eng, _, g, thr, _ = engine_case(H, W, dtype)
    sh, sw = 96 / 90, 128 / 121                          # not representable, as transform() produces them
    cells = kept = 0
    for mode in ("d1", "d2"):
        plain = eng.decode_threshold(thr, 0.3, mode=mode)
        eng.set_rescale(sh, sw)
        scaled = eng.decode_threshold(thr, 0.3, mode=mode)
        eng.set_rescale(0.0, 0.0)
        for b, ((d, l), (ds, ls)) in enumerate(zip(plain, scaled)):
            wd, wl = oracle_rows(g, b, (H, W), thr, mode)
            say("engine-%dx%d-%s-%s[%d]" % (H, W, dtype, mode, b), int((g["hm_sigmoid"][b] > f32(thr)).sum()), len(d))
            assert d.tobytes() == wd.tobytes(), (mode, b, d.shape, wd.shape)
            if wl is not None:
                assert l.tobytes() == wl.tobytes(), (mode, b)
            want_d, want_l = d.copy(), l.copy()
            want_d[:, 0:4:2], want_d[:, 1:4:2] = d[:, 0:4:2] // sw, d[:, 1:4:2] // sh            # the reference's own statement
            want_l[:, 0:10:2], want_l[:, 1:10:2] = l[:, 0:10:2] // sw, l[:, 1:10:2] // sh
            assert ds.tobytes() == want_d.tobytes() and ls.tobytes() == want_l.tobytes(), (mode, b)
            cells, kept = cells + int((g["hm_sigmoid"][b] > f32(thr)).sum()), kept + len(d)
    eng.close()
    assert kept < cells, (kept, cells)                   # the inputs made the NMS suppress something


def test_engine_workspace_that_has_grown_leaves_no_stale_suppression_bits():
    """A decode at a threshold below every cell of a 72 x 64 map (4608 candidates per image: the 4096 workspace grows, capacity and word
    stride stay grown), then a decode at the ordinary threshold on the same engine: it must equal a fresh engine's result and the
    oracle's.  (The 96 x 128 and 160 x 224 engines have fewer than 4096 cells: their workspace is born at its final size, so this takes
    the smallest engine whose map is the map generator's 72 x 64.)"""
    H, W = 288, 256
    eng, x, g, thr, sd = engine_case(H, W, "fp32", B=2)
    low = float(np.nextafter(g["hm_sigmoid"].min(), f32(0)))
    every = eng.decode_threshold(low, 0.3)
    wd, wl = oracle_rows(g, 0, (H, W), low, "d1")
    say("engine-288x256-fp32-every-cell[0]", 4608, len(every[0][0]))
    assert every[0][0].tobytes() == wd.tobytes() and every[0][1].tobytes() == wl.tobytes()
    after = eng.decode_threshold(thr, 0.3)
    eng.close()
    fresh = cfa.Engine(H, W, max_batch=2, dtype="fp32", weights=sd)
    fresh.forward_enqueue(x)
    first = fresh.decode_threshold(thr, 0.3)
    fresh.close()
    for b in range(2):
        wd, wl = oracle_rows(g, b, (H, W), thr, "d1")
        say("engine-288x256-fp32-after-growth[%d]" % b, int((g["hm_sigmoid"][b] > f32(thr)).sum()), len(after[b][0]))
        assert after[b][0].tobytes() == first[b][0].tobytes() == wd.tobytes()
        assert after[b][1].tobytes() == first[b][1].tobytes() == wl.tobytes()
