"""Scene cuts on the GPU: cf_op_scene against the numpy restatement (tests/scene_cases.py) on every int32, then the check behind an engine
-- host and device forms, shared objects, the reset of a tracker's streams on the device -- and the product paths that take ``scenes=``."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from scene_cases import CUT, FIRST, FORMATS, SAME, RefScene, brighter, dense, luma_of, moved_views, pack, run_scene, scene
from test_redact import source_frames
from test_track import _blank_batch, _feed_until_faces, _same_update
from track_cases import RefTracker

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    for name, g, w in zip(("out", "sigs"), got, want):
        assert g.dtype == w.dtype == np.int32 and g.shape == w.shape, (what, name)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError("%s: %s differs at %s: got %s, want %s" % (what, name, bad[:6].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def _story(rng, fmt, h, w):
    """Five frames of one stream: a scene, the same frame again, a view of it moved by (4, 2), the frame 40 levels brighter, another scene."""
    a, moved = moved_views(rng, fmt, h, w, ((0, 0), (4, 2)))
    a = (a >> 1).astype(np.uint8)                                          # [0, 128): the other scene lies in [128, 256)
    return [a, a, (moved >> 1).astype(np.uint8), brighter(a, 40), scene(rng, fmt, h, w, 128, 256)]


# (24, 48): rows and frames that are multiples of 16 bytes (the 16-byte loads) with cells narrower than a run
@pytest.mark.parametrize("hw", ((8, 8), (10, 14), (18, 22), (76, 102), (24, 48)), ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("fmt", FORMATS)
def test_sequence_equals_the_restatement(fmt, hw):
    rng = np.random.default_rng(11)
    h, w = hw
    s0 = _story(rng, fmt, h, w)
    s1 = [s0[k] for k in (4, 3, 0, 0, 2)]                                  # stream 1 sees the frames in another order: no shared state
    imgs = [im for pair in zip(s0, s1) for im in pair]                     # frame f of stream s at f * 2 + s
    for pad0, pad1 in ((0, 0), (5, 3)):
        frames, lumas = pack(rng, fmt, imgs, pad0, pad1)
        want = run_scene(lumas, 2)
        _same(ops.scene_sequence(frames, fmt, 2, sigs=True), want, (fmt, hw, pad0))
        assert want[0][:, 0, 0].tolist() == [FIRST, SAME, want[0][2, 0, 0], want[0][3, 0, 0], CUT]
    assert np.array_equal(ops.scene_signature(frames[3], fmt), want[1][1, 1])
    assert np.array_equal(ops.scene_sequence(frames, fmt, 2), want[0])


@pytest.mark.parametrize("hw", ((270, 482), (1080, 1920)), ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("fmt", ("nv12", "bgr"))
def test_large_frames(fmt, hw):
    """Many workgroups per frame, dword loads (482) and 16-byte loads (1920), one real frame size."""
    rng = np.random.default_rng(12)
    h, w = hw
    a = scene(rng, fmt, h, w, 0, 200, block=8)
    arr, lumas = dense(fmt, [a, np.roll(a, (2, 4), axis=(0, 1)), scene(rng, fmt, h, w, 100, 256, block=8)], rng)
    want = run_scene(lumas, 1)
    _same(ops.scene_sequence(arr, fmt, 1, sigs=True), want, (fmt, hw))
    assert want[0][:, 0, 0].tolist() == [FIRST, SAME, CUT]


@pytest.mark.parametrize("fmt", ("i420", "bgr"))
def test_threshold_boundary(fmt):
    rng = np.random.default_rng(13)
    h, w = 18, 22
    frames, lumas = pack(rng, fmt, [scene(rng, fmt, h, w, 0, 256), scene(rng, fmt, h, w, 0, 256)], 3, 1)
    _, hist, grid, _ = run_scene(lumas, 1, 0, 0)[0][1, 0]
    assert 0 < hist < 1000 and 0 < grid < 16320
    for hi, gr, code in ((hist, grid, CUT), (hist + 1, grid, SAME), (hist, grid + 1, SAME), (0, 0, CUT), (1000, 16320, SAME)):
        got = ops.scene_sequence(frames, fmt, 1, hist=hi, grid=gr)
        assert np.array_equal(got, run_scene(lumas, 1, hi, gr)[0]) and got[1, 0].tolist() == [code, hist, grid, 0 if code == CUT else 1]


# ---------------------------------------------------------------------------------------------- behind an engine
def _to_device(eng, frames):
    """Dense BGR frames [B,h,w,3] with 3w a multiple of 4 on the device: (address, plane tuples)."""
    B, h, w, _ = frames.shape
    assert (3 * w) % 4 == 0
    p = eng.device_alloc(frames.nbytes)
    eng.memcpy_h2d(p, frames)
    return p, [(p + b * h * w * 3,) for b in range(B)]


def test_engine_check_host_and_device_forms_shared_objects_and_forget():
    rng = np.random.default_rng(14)
    eng, eng2 = (cfa.Engine(64, 96, max_batch=3, dtype="bf16") for _ in range(2))      # no forward is ever run
    scn, ref = cfa.SceneCuts(0, 5), RefScene(5)                            # created by the first check
    h, w = 76, 104
    a = np.stack([scene(rng, "bgr", h, w, 0, 128) for _ in range(3)])
    b = np.stack([a[0], scene(rng, "bgr", h, w, 128, 256), brighter(a[2], 9)])
    lum = lambda x: [luma_of((f.reshape(h, -1),), "bgr") for f in x]       # noqa: E731
    want = lambda x, s0: np.array([ref.check(s0 + k, l) for k, l in enumerate(lum(x))], np.int32)      # noqa: E731
    # host form: B = 3 at stream0 = 1
    got = eng.scene_check(a, "bgr", scn, None, 1)
    assert got.dtype == np.int32 and np.array_equal(got, want(a, 1)) and (got[:, 0] == FIRST).all()
    got = eng.scene_check(b, "bgr", scn, stream0=1)
    assert np.array_equal(got, want(b, 1)) and got[:, 0].tolist() == [SAME, CUT, SAME]
    assert eng.scene_check(b, "bgr", scn, stream0=1, codes=False) is None
    want(b, 1)
    # device form, two engines sharing the object in alternation, nothing read in between
    out = [e.device_alloc(3 * 4 * 4) for e in (eng, eng2)]
    seq = [a, b, b, a]
    held = [_to_device((eng, eng2)[k % 2], x) for k, x in enumerate(seq)]
    got = []
    for k, (x, (_, planes)) in enumerate(zip(seq, held)):
        e = (eng, eng2)[k % 2]
        if k >= 2:                                                         # the buffer's earlier result, before it is written again
            e.synchronize()
            got.append(np.zeros((3, 4), np.int32))
            e.memcpy_d2h(got[-1], out[k % 2])
        e.scene_check_device(planes, "bgr", 3, h, w, 3 * w, 0, scn, None, 1, out[k % 2])
    for k in (0, 1):
        (eng, eng2)[k].synchronize()
        got.append(np.zeros((3, 4), np.int32))
        (eng, eng2)[k].memcpy_d2h(got[-1], out[k])
    for g, x in zip(got, seq):
        assert np.array_equal(g, want(x, 1)), (g, x.shape)
    assert got[0][:, 0].tolist() == [SAME, CUT, SAME] and got[2][:, 0].tolist() == [SAME, SAME, SAME]
    eng.scene_check_device(held[0][1], "bgr", 3, h, w, 3 * w, 0, scn, stream0=1)      # no output buffer at all
    want(a, 1)
    # forget(1): stream 1 is FIRST again and no other; streams 0 and 4 were never checked
    scn.forget(1)
    ref.forget(1)
    got = eng2.scene_check(a, "bgr", scn, stream0=1)
    assert np.array_equal(got, want(a, 1)) and got[:, 0].tolist() == [FIRST, SAME, SAME]
    got = eng.scene_check(a[:2], "bgr", scn, stream0=0)
    assert np.array_equal(got, want(a[:2], 0)) and got[0].tolist() == [FIRST, 0, 0, 0] and got[1, 0] != FIRST
    got = eng.scene_check(a[:1], "bgr", scn, stream0=4)
    assert np.array_equal(got, want(a[:1], 4)) and got[0].tolist() == [FIRST, 0, 0, 0]
    # frames of another size are FIRST
    got = eng.scene_check(np.ascontiguousarray(a[:, :40, :60]), "bgr", scn, stream0=1)
    assert (got[:, 0] == FIRST).all()
    # argument errors: before any GPU work
    trk = cfa.Tracker(eng, 3)
    for call in (lambda: eng.scene_check(a, "bgr", scn, None, 3), lambda: eng.scene_check(a, "bgr", scn, None, -1),
                 lambda: eng.scene_check(a, "bgr", scn, trk, 1),                                     # streams 1..3 of a tracker with 3
                 lambda: eng.scene_check(np.concatenate([a, a[:1]]), "bgr", scn, None, 0),           # B = 4 > max_batch
                 lambda: eng.scene_check(np.zeros((1, 6, 8, 3), np.uint8), "bgr", scn), lambda: eng.scene_check(np.zeros((1, 9, 8, 3), np.uint8), "bgr", scn)):
        with pytest.raises(ValueError):
            call()
    for e, (p, _) in zip((eng, eng2, eng, eng2), held):
        e.device_free(p)
    for e, p in zip((eng, eng2), out):
        e.device_free(p)
    trk.close(), scn.close(), eng.close(), eng2.close()


def test_a_cut_resets_the_streams_tracks_on_the_device():
    eng = cfa.Engine(64, 96, max_batch=2, dtype="bf16")
    for seed in range(8):                                                  # a source with a face in both frames
        rng = np.random.default_rng(20 + seed)
        src, base = _feed_until_faces(eng, rng, need=2, B=2)
        if all(len(d) for d, _ in base):
            break
    else:
        raise AssertionError("no source holds a face in both frames with the default weights")
    opts = dict(iou=0.3, max_age=15, min_hits=2, max_tracks=64, hold_grow=0.05)
    trk, ref = cfa.Tracker(eng, 2, **opts), RefTracker(2, **opts)
    scn, sref = cfa.SceneCuts(eng, 2), RefScene(2)
    h, w = src.shape[1] & ~1, src.shape[2] & ~1
    seen = np.ascontiguousarray(src[:, :h, :w])                            # the even-sized part of the source, as the stream's frames
    cut = np.stack([scene(rng, "bgr", h, w, 0, 40), seen[1]])              # frame 0: another scene (dark); frame 1: the frame seen before
    lum = lambda x: [luma_of((f.reshape(h, -1),), "bgr") for f in x]       # noqa: E731
    want = lambda x: np.array([sref.check(k, l) for k, l in enumerate(lum(x))], np.int32)      # noqa: E731

    def update(rows):
        got, flags = eng.track_update(trk)
        top[0:] = [max(top + got[0][2].tolist())]
        _same_update(got, [ref.update(b, d[:, :4], d[:, 4], l, len(d)) for b, (d, l) in enumerate(rows)])
        return got

    got = eng.scene_check(seen, "bgr", scn, trk)
    assert np.array_equal(got, want(seen)) and (got[:, 0] == FIRST).all()
    top = [0]
    first = update(base)                                                   # the decode of _feed_until_faces
    eng.forward_resized_enqueue(src)
    update(eng.decode_threshold(0.3, 0.3, 64))                             # twice: the tracks are confirmed
    # the check without a tracker resets nothing: the blank batch holds every track of both streams
    got = eng.scene_check(cut, "bgr", scn, None)
    assert np.array_equal(got, want(cut)) and got[:, 0].tolist() == [CUT, SAME]
    held = update(_blank_batch(eng, B=2))
    assert all(len(g[0]) and (g[4] == 1).all() for g in held)
    # with the tracker: stream 0 (back from the dark scene: a cut again) is reset on the device, stream 1 is not
    got = eng.scene_check(seen, "bgr", scn, trk)
    assert np.array_equal(got, want(seen)) and got[:, 0].tolist() == [CUT, SAME]
    ref.reset(0)
    held = update(_blank_batch(eng, B=2))
    assert len(held[0][0]) == 0 and len(held[1][0]) and (held[1][4] == 2).all()
    before = top[0]
    eng.forward_resized_enqueue(src)
    again = update(eng.decode_threshold(0.3, 0.3, 64))
    assert len(again[0][2]) and int(again[0][2].min()) > before            # ids are not reused
    trk.close(), scn.close(), eng.close()


# ---------------------------------------------------------------------------------------------- product paths
def _count_forwards(eng):
    calls = []
    for name in ("forward_enqueue", "forward_resized_enqueue", "forward_images_enqueue", "forward_yuv_enqueue", "forward_tiles_enqueue"):
        real = getattr(eng, name)
        setattr(eng, name, lambda *a, _real=real, **k: (calls.append(1), _real(*a, **k))[1])
    return calls


def _by_hand(face, trk, scn, frame, opt, detect, fo):
    """One call of anonymize([frame], tracker=, scenes=, detect=, follow=fo) at max_batch = 1, restated from public Engine calls: (frame
    out, result, whether a forward ran)."""
    eng, out = face.engine, np.stack([frame])
    codes = eng.scene_check(out, "bgr", scn, trk, 0)
    key = detect or codes[0, 0] != SAME
    if key:
        eng.set_rescale(face.scale_h, face.scale_w)
        eng.forward_resized_enqueue(np.stack([frame]))
        res = eng.decode_threshold(0.3, face.nms_thresh, face.max_dets)
        eng.track_update_device(trk, 0)
        eng.set_rescale(0.0, 0.0)
    if fo is not None:
        d, l, _, n, _ = eng.track_follow(out, "bgr", trk, 0, **fo)
        if not detect:
            fx, fy = out.shape[2] / float(face.img_w_new), out.shape[1] / float(face.img_h_new)
            dd, ll = d[0, :n[0]].astype(np.float64), l[0, :n[0]].astype(np.float64)
            dd[:, 0:4:2] *= fx; dd[:, 1:4:2] *= fy; ll[:, 0::2] *= fx; ll[:, 1::2] *= fy      # noqa: E702
            res = [(dd, ll)]
    eng.cover_faces(out, "bgr", **opt)
    return out, res, bool(key)


def test_anonymize_detects_only_where_a_scene_starts():
    rng = np.random.default_rng(41)
    hw = (76, 102)
    face, face2 = (cfa.CenterFace(*hw, dtype="bf16", max_batch=1) for _ in range(2))
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        A = source_frames(rng, kind, (1,) + hw + (3,))[0]
        if len(face.detect_batch([A])[0][0]) >= 1:
            break
    else:
        raise AssertionError("no source holds a face with the default weights")
    B = (source_frames(rng, kind, (1,) + hw + (3,))[0] >> 2).astype(np.uint8)      # another scene, in the dark quarter of the range
    video = [A, A, B, B]
    opt = dict(mode="solid", shape="rect", fill=(1, 2, 3))
    fo = dict(search=4, max_sad=65280)
    with pytest.raises(ValueError):
        face.anonymize([A], scenes=cfa.SceneCuts(0, 1), **opt)              # scenes needs a tracker
    for detect, follow in ((False, fo), (True, None)):
        trk, trk2 = (cfa.Tracker(f.engine, 1, min_hits=1, max_age=3) for f in (face, face2))
        scn, scn2 = (cfa.SceneCuts(f.engine, 1) for f in (face, face2))
        calls = _count_forwards(face.engine)
        ran, want_ran, covered = [], [], []
        for frame in video:
            n = len(calls)
            out, dets = face.anonymize([frame], tracker=trk, scenes=scn, detect=detect, follow=follow, **opt)
            ran.append(len(calls) - n)
            want, want_dets, key = _by_hand(face2, trk2, scn2, frame, opt, detect, follow)
            want_ran.append(int(key))
            assert np.array_equal(out, want), (detect, len(ran))
            for (d, l), (wd, wl) in zip(dets, want_dets):
                assert d.dtype == wd.dtype and d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes()
            covered.append(bool((out != frame[None]).any()))
        assert ran == want_ran == ([1, 0, 1, 0] if not detect else [1, 1, 1, 1]), (detect, ran, want_ran)
        assert covered[0] and covered[1]                                    # the face of A, detected in frame 0 and followed in frame 1
        for name in ("forward_enqueue", "forward_resized_enqueue", "forward_images_enqueue", "forward_yuv_enqueue", "forward_tiles_enqueue"):
            delattr(face.engine, name)                                      # the wrappers of _count_forwards
        trk.close(), trk2.close(), scn.close(), scn2.close()
    face.close(), face2.close()
