"""Flip test on the GPU: the mirror and merge kernels alone (cf_op_mirror, cf_op_flip_heads), a context switched to flip test
(cf_set_flip_test) against a plain context that is handed the batch and its mirror, the decodes and the product paths behind it.  Every
comparison is bit for bit against the numpy restatement of tests/flip_cases.py: each merged value is one rounding of exact inputs."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from flip_cases import flip_heads_ref, maps_to_records, mirror_ref, records_to_maps
from test_flip_abi import swap_property

pytestmark = pytest.mark.gpu

NET = (64, 96)                  # (H, W) of every context here: a 16 x 24 map
FIELDS = ("hm", "hm_sigmoid", "wh", "lm", "reg")
L = cfa._lib


def images(seed, B, hw=NET):
    return np.random.default_rng(seed).integers(0, 256, (B,) + tuple(hw) + (3,), dtype=np.uint8)


def plain_records(eng, staged):
    """The head records of a plain engine on the staged batch with its mirror appended: [2B, h, w, 16]."""
    eng.forward_enqueue(np.concatenate([staged, mirror_ref(staged)]))
    return maps_to_records(eng.heads(sigmoid_hm=True))


def assert_heads(got, want_records, what):
    want = records_to_maps(want_records)
    for k in FIELDS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert len(bad) == 0, (what, k, len(bad), bad[:4].tolist())


# ------------------------------------------------------------------------------------------ the mirror kernel
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("hw", ((32, 32), (64, 96), (32, 160)))
@pytest.mark.parametrize("kind", ("u8", "f32"))
def test_op_mirror_bit_exact(kind, hw, B):
    """One group per row (W = 32: two 48-byte groups), several, and more lanes than one workgroup (64 x 96 x 3 images); every byte."""
    rng = np.random.default_rng(hw[1] + B)
    if kind == "u8":
        x = rng.integers(0, 256, (B, hw[0], hw[1], 3), dtype=np.uint8)
    else:
        x = rng.standard_normal((B, 3, hw[0], hw[1])).astype(np.float32)
    got = ops.mirror_batch(x)
    want = mirror_ref(x)
    assert got.dtype == x.dtype and got.shape == x.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (kind, hw, B, len(bad), bad[:4].tolist())


# ------------------------------------------------------------------------------------------ the merge kernel
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("hw", ((8, 8), (16, 24), (8, 40)))
def test_op_flip_heads_bit_exact(hw, B):
    """Random records, negatives included: records and hm_plane equal the restatement, hm_plane is channel 0, and merging (M, A) instead
    of (A, M) gives the mirrored result with the landmarks negated in x and the pairs swapped."""
    rng = np.random.default_rng(7 * hw[1] + B)
    rec = (rng.standard_normal((2 * B, hw[0], hw[1], 16)) * 5).astype(np.float32)
    assert (rec < 0).any()
    got, plane = ops.flip_heads(rec, B)
    want, wplane = flip_heads_ref(rec, B)
    assert got.shape == want.shape and plane.shape == wplane.shape == (B, hw[0] * hw[1])
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (hw, B, len(bad), bad[:4].tolist())
    assert plane.tobytes() == wplane.tobytes() and np.array_equal(plane.reshape(B, hw[0], hw[1]), got[..., 0])
    back, _ = ops.flip_heads(np.concatenate([rec[B:], rec[:B]]), B)
    assert swap_property(got, back, hw[1])


# ------------------------------------------------------------------------------------------ a context in flip test
@pytest.mark.parametrize("dtype", ("fp32", "bf16", "fp32_split"))
def test_engine_flip_heads_equal_the_merge_of_a_plain_double_batch(dtype):
    """B = 3 through a flip engine = the restated merge of a plain engine's records of concat(X, mirror(X)); three forwards in a row
    (eager, graph capture, graph replay), a context whose capacity leaves the mirrored half at slot B, and one without graphs."""
    sd = cfa.weights.synthetic_state_dict(0)
    X = images(3, 3)
    plain = cfa.Engine(NET[0], NET[1], max_batch=6, dtype=dtype, weights=sd)
    rec = plain_records(plain, X)
    assert plain.flip_test is False
    with pytest.raises(ValueError):
        plain.set_flip_test(True)
    plain.close()
    assert rec.shape == (6, 16, 24, 16)
    want, wplane = flip_heads_ref(rec, 3)
    assert not np.array_equal(want, rec[:3])                               # the merge changes the heads
    for kw in (dict(max_batch=3), dict(max_batch=4), dict(max_batch=3, graph=False)):
        eng = cfa.Engine(NET[0], NET[1], dtype=dtype, weights=sd, flip_test=True, **kw)
        assert eng.flip_test is True and eng.max_batch == kw["max_batch"]
        for run in range(3):
            eng.forward_enqueue(X)
            assert eng.last_B == 3
            assert_heads(eng.heads(sigmoid_hm=True), want, (dtype, kw, run))
        eng.close()


def test_engine_flip_input_paths():
    """Every way a batch reaches the network, B = 2: the flip engine's heads are the merge of a plain engine's heads on the same staged
    input with its mirror appended."""
    sd = cfa.weights.synthetic_state_dict(0)
    eng = cfa.Engine(NET[0], NET[1], max_batch=2, dtype="bf16", weights=sd, flip_test=True)
    plain = cfa.Engine(NET[0], NET[1], max_batch=4, dtype="bf16", weights=sd)
    rng = np.random.default_rng(17)

    def check(what, staged):
        assert eng.last_B == len(staged) == 2, what
        assert_heads(eng.heads(sigmoid_hm=True), flip_heads_ref(plain_records(plain, staged), 2)[0], what)

    X = images(5, 2)
    eng.forward_enqueue(X)
    check("host uint8", X)
    Xf = rng.standard_normal((2, 3) + NET).astype(np.float32)
    eng.forward_enqueue(Xf)
    check("host float32", Xf)
    # a device tensor that is only 4-byte aligned: 4 bytes behind a 16-byte boundary
    dev = eng.device_alloc(X.nbytes + 16)
    assert dev % 16 == 0
    eng.memcpy_h2d(dev + 4, X)
    for run in range(3):                                                  # (eager, capture, replay of the fl_in graph)
        eng.forward_enqueue(dev + 4, on_device=True, B=2, in_format=L.CF_IN_U8_HWC_BGR)
        check("device uint8 + 4, run %d" % run, X)
    back = np.empty_like(X)
    eng.memcpy_d2h(back, dev + 4)
    assert np.array_equal(back, X)                                        # read in place: the caller's tensor is untouched
    eng.device_free(dev)
    small = images(6, 2, (40, 120))
    eng.forward_resized_enqueue(small)
    check("resized", eng.resized_input())
    eng.forward_images_enqueue(list(small))
    check("images", eng.resized_input())
    eng.forward_images_enqueue(list(X))                                   # network-sized: through a host-input slot
    check("images, network-sized", X)
    yuv = rng.integers(0, 256, (2, 48 * 3 // 2, 64), dtype=np.uint8)
    eng.forward_yuv_enqueue(yuv, "nv12")
    check("nv12", eng.resized_input())
    eng.forward_fit_enqueue(small, "bgr", fill=(1, 2, 3))
    check("fit", eng.resized_input())
    frame = images(8, 1, (80, 120))
    eng.forward_tiles_enqueue(frame, [(0, 0, 64, 48), (40, 20, 80, 60)], "bgr")
    tiles = eng.resized_input()
    assert np.array_equal(tiles, ops.cut_tiles(frame, [(0, 0, 64, 48), (40, 20, 80, 60)], NET, "bgr").reshape(tiles.shape))
    check("tiles", tiles)
    with pytest.raises(ValueError) as e:                                  # three tiles do not fit the flip batch of 2
        eng.forward_tiles_enqueue(frame, [(0, 0, 64, 48), (40, 20, 80, 60), (0, 0, 120, 80)], "bgr")
    assert "flip test" in str(e.value)
    eng.close()
    plain.close()


def test_decodes_read_the_merged_heads():
    """Top-K (K = 10) and the threshold decode of a flip engine = the explicit-map ops on the merged maps, at a threshold that keeps
    rows in every image."""
    sd = cfa.weights.synthetic_state_dict(0)
    X = images(9, 3)
    plain = cfa.Engine(NET[0], NET[1], max_batch=6, dtype="fp32", weights=sd)
    merged, _ = flip_heads_ref(plain_records(plain, X), 3)
    plain.close()
    maps = records_to_maps(merged)
    eng = cfa.Engine(NET[0], NET[1], max_batch=3, dtype="fp32", weights=sd, flip_test=True)
    eng.forward_enqueue(X)
    dets, lms, inds = eng.decode_topk(K=10)
    wd, wl, wi = ops.ctdet_decode(maps["hm_sigmoid"], maps["wh"], maps["reg"], 10, maps["lm"])
    assert dets.tobytes() == wd.tobytes() and lms.tobytes() == wl.tobytes() and np.array_equal(inds, wi)
    thr = float(maps["hm_sigmoid"].reshape(3, -1).max(axis=1).min()) * 0.75          # below every image's highest heat
    for mode, m in (("d1", 0), ("d2", 1)):
        rows = eng.decode_threshold(thr, 0.3, 512, mode=mode)
        od, ol = np.zeros((3, 512, 5), np.float32), np.zeros((3, 512, 10), np.float32)
        oc = np.zeros(3, np.int32)
        hm, wh, reg, lm = (np.ascontiguousarray(maps[k]) for k in ("hm_sigmoid", "wh", "reg", "lm"))
        rc = L.lib().cf_op_decode_threshold_ex(0, m, L.ptr(hm), L.ptr(wh), L.ptr(reg), L.ptr(lm), 3, 16, 24, NET[0], NET[1], thr, 0.3, 512,
                                               L.ptr(od), L.ptr(ol), L.ptr(oc))
        assert rc == 0, L.lib().cf_op_last_error()
        assert [len(d) for d, _ in rows] == oc.tolist() and min(oc.tolist()) >= 1, (mode, thr, oc)
        for b, (d, l) in enumerate(rows):
            assert d.tobytes() == od[b, :oc[b]].tobytes(), (mode, b)
            assert mode == "d2" or l.tobytes() == ol[b, :oc[b]].tobytes(), (mode, b)          # (D2 has no landmarks)
        if mode == "d1":
            # cf_align_faces samples the UNMIRRORED half of the doubled input, with the merged landmarks
            chips, offs, mats = eng.align_faces(32)
            wc, wm = ops.align_faces(X, np.concatenate([l for _, l in rows]), oc, 32)
            assert offs.tolist() == [0] + np.cumsum(oc).tolist()
            assert chips.tobytes() == wc.tobytes() and mats.tobytes() == wm.tobytes()
    # cf_detect_topk: the forward inside it is a flip forward too
    d2, l2, i2 = np.empty_like(dets), np.empty_like(lms), np.empty_like(inds)
    eng._chk(L.lib().cf_detect_topk(eng._h, L.ptr(X), L.CF_IN_U8_HWC_BGR, 0, 3, 10, L.ptr(d2), L.ptr(l2), L.ptr(i2), 0))
    assert d2.tobytes() == wd.tobytes() and l2.tobytes() == wl.tobytes() and np.array_equal(i2, wi)
    eng.close()


def test_flip_state_rules():
    """Off gives the heads of an engine that never flipped, on again the flip heads; a batch above max_batch is refused with CF_EINVAL
    and leaves the last results decodable; the trace and the profile are CF_ESTATE while it is on."""
    sd = cfa.weights.synthetic_state_dict(0)
    X = images(12, 2)
    plain = cfa.Engine(NET[0], NET[1], max_batch=4, dtype="bf16", weights=sd)
    rec = plain_records(plain, X)
    plain.close()
    flipped, _ = flip_heads_ref(rec, 2)
    eng = cfa.Engine(NET[0], NET[1], max_batch=2, dtype="bf16", weights=sd, flip_test=True)
    eng.forward_enqueue(X)
    assert_heads(eng.heads(sigmoid_hm=True), flipped, "on")
    eng.set_flip_test(False)
    assert eng.flip_test is False
    assert_heads(eng.heads(sigmoid_hm=True), flipped, "off, before the next forward")          # the last results stay
    eng.forward_enqueue(X)
    assert_heads(eng.heads(sigmoid_hm=True), rec[:2], "off")
    eng.forward_enqueue(np.concatenate([X, X]))                                                # the whole capacity is usable again
    assert eng.last_B == 4
    eng.set_flip_test(True)
    assert eng.flip_test is True
    eng.forward_enqueue(X)
    assert_heads(eng.heads(sigmoid_hm=True), flipped, "on again")
    before = eng.decode_topk(K=10)
    with pytest.raises(ValueError) as e:
        eng.forward_enqueue(images(13, 3))
    assert e.value.code == -1 and "B=3" in str(e.value) and "flip test" in str(e.value)
    assert eng.last_B == 2
    after = eng.decode_topk(K=10)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    for call in (lambda: eng.trace(X, 0), lambda: eng.profile_forward(X)):
        with pytest.raises(cfa._lib.CenterFaceError) as e:
            call()
        assert e.value.code == L.CF_ESTATE and "flip test" in str(e.value)
    assert eng._L.cf_set_flip_test(eng._h, 2) == -1 and b"on=2" in eng._L.cf_last_error(eng._h)
    eng.close()
    one = cfa.Engine(NET[0], NET[1], max_batch=1, dtype="bf16", weights=sd)
    assert one._L.cf_set_flip_test(one._h, 1) == -1 and b"max_batch=1" in one._L.cf_last_error(one._h)
    one.close()


# ------------------------------------------------------------------------------------------ the product paths
def test_centerface_with_flip_test():
    """CenterFace(flip_test=True) over 5 frames (chunks of 2, 2 and 1) returns the rows of the engine-level calls, and anonymize covers
    exactly the bytes ops.redact_faces covers for those rows.  The heat bias is raised until every frame has a cell whose heat is above
    0.5 in both passes, so every frame has rows at the product's threshold of 0.3."""
    sd = dict(cfa.weights.synthetic_state_dict(0))
    frames = images(21, 5)
    plain = cfa.Engine(NET[0], NET[1], max_batch=10, dtype="fp32", weights=sd)
    plain.forward_enqueue(np.concatenate([frames, mirror_ref(frames)]))
    logit = plain.heads()["hm"][:, 0]
    plain.close()
    both = np.minimum(logit[:5], logit[5:, :, ::-1])                       # per cell, the lower logit of the two passes
    sd["hm.1.bias"] = (sd["hm.1.bias"] + np.float32(0.5) - both.reshape(5, -1).max(axis=1).min()).astype(np.float32)
    eng = cfa.Engine(NET[0], NET[1], max_batch=2, dtype="fp32", weights=sd, flip_test=True, decode_stream=False)
    want, boxes, counts = [], [], []
    for i in range(0, 5, 2):
        eng.forward_enqueue(frames[i:i + 2])
        base = eng.decode_threshold(0.3, 0.3, 1024)                        # network coordinates: what the redaction takes
        boxes += [d[:, :4] for d, _ in base]
        counts += [len(d) for d, _ in base]
        eng.set_rescale(1.0, 1.0)
        want += eng.decode_threshold(0.3, 0.3, 1024)
        eng.set_rescale(0.0, 0.0)
    eng.close()
    assert min(counts) >= 1, counts
    face = cfa.CenterFace(NET[0], NET[1], dtype="fp32", max_batch=2, weights=sd, flip_test=True)
    assert face.engine.flip_test is True and face.engine.max_batch == 2
    got = face.detect_batch(list(frames))
    assert len(got) == 5
    for b, ((d, l), (wd, wl)) in enumerate(zip(got, want)):
        assert d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes(), b
    opts = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    out, dets = face.anonymize(list(frames), **opts)
    for (d, l), (wd, wl) in zip(dets, want):
        assert d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes()
    ref = ops.redact_faces(frames.copy(), np.concatenate(boxes), np.array(counts, np.int32), NET, "bgr", **opts)
    assert np.array_equal(out, ref) and not np.array_equal(out, frames)
    face.close()
    # a plain CenterFace on the same frames sees other heads
    face = cfa.CenterFace(NET[0], NET[1], dtype="fp32", max_batch=2, weights=sd)
    assert face.engine.flip_test is False
    other = face.detect_batch(list(frames))
    assert any(d.tobytes() != wd.tobytes() for (d, _), (wd, _) in zip(other, want))
    face.close()
