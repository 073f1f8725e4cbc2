"""Annotation of the source frame on the device (cf_draw_faces / cf_op_draw, csrc/cf_draw.hip) against the numpy restatement of
tests/draw_cases.py, bit for bit on every byte of every buffer, pitch padding and guard bands included: through ops.draw_faces for the
cases of draw_cases.CASES (tests/test_draw_abi.py shows on the CPU that each of them draws something), and through a context behind a
real threshold decode, a tile merge and the tracker."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
from draw_cases import CASES, Frames, draw_ref, opt, permuted, pitches_for, yuv_opt
from test_redact import _feed_until_faces, redact_ref

pytestmark = pytest.mark.gpu

LOOK = dict(box_color=(2, 255, 0), held_color=(0, 255, 255), lm_color=(0, 0, 255), text_color=(0, 0, 0))       # CenterFace.annotate's colours


def _run(case, fr):
    assert ops.draw_faces(fr.arg, case.boxes, case.scores, case.counts, case.net, **case.kwargs()) is fr.arg
    return fr


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_op_draw_bit_exact(case):
    fr = case.frames()
    want, maps = case.expect(fr)
    assert not want.same(fr)                                                # the restatement changed at least one byte
    if case.layers:
        assert all(any((m == k).any() for m in maps) for k in (1, 2, 3, 4))
    got = _run(case, fr.clone())
    assert got.same(want), (case.name, got.diff(want))


@pytest.mark.parametrize("name", ("bgr-pitched", "nv12-pitched", "i420-wide", "bgr-300-rows"))
def test_row_order_does_not_matter(name):
    case = next(c for c in CASES if c.name == name)
    fr = case.frames()
    a = _run(case, fr.clone())
    other = permuted(case)
    b = _run(other, fr.clone())
    assert a.same(b), (name, a.diff(b))
    want, _ = other.expect(fr)                                              # and once against the restatement of the permuted rows
    assert b.same(want) and not b.same(fr)


# ------------------------------------------------------------------------------------------ behind a context
def _rows(results):
    """Per-image (dets [n,5], lms [n,10], ...) -> packed boxes, scores, lms, counts."""
    return (np.concatenate([r[0][:, :4] for r in results]), np.concatenate([r[0][:, 4] for r in results]), np.concatenate([r[1] for r in results]),
            np.array([len(r[0]) for r in results], np.int32))


def _engine_case(eng, fmt, h, w, rows, net, dense=False, info=None, differs_from=None, **o):
    """Engine.draw_faces == the restatement on ``rows``, which draws something -- or, with ``differs_from`` (other rows), something else
    than those would."""
    boxes, scores, lms, counts = rows
    p0, p1 = pitches_for(fmt, w)
    fr = Frames(np.random.default_rng(13), fmt, len(counts), h, w, p0, p1, dense)
    want = fr.clone()
    draw_ref(want.views, fmt, boxes, scores, counts, net, h, w, lms=lms, info=info, **o)
    other = fr
    if differs_from is not None:
        other = fr.clone()
        draw_ref(other.views, fmt, differs_from[0], differs_from[1], differs_from[3], net, h, w, lms=differs_from[2], info=info, **o)
    assert not want.same(other), (fmt, o)
    assert eng.draw_faces(fr.arg, fmt, **o) is fr.arg
    assert fr.same(want), (fmt, o, fr.diff(want))
    return fr


def _state(call):
    with pytest.raises(cfa._lib.CenterFaceError) as e:
        call()
    assert e.value.code == cfa._lib.CF_ESTATE


@pytest.mark.parametrize("how", ("resized", "yuv"))
def test_engine_draw_equals_restatement(how):
    """Engine.draw_faces behind forward_resized_enqueue / forward_yuv_enqueue + decode_threshold on the default weights, context 64 x 96:
    the restatement on the rows the decode returned (network coordinates), host and device form; the context's state is untouched."""
    rng = np.random.default_rng(("resized", "yuv").index(how))
    eng = cfa.Engine(64, 96, max_batch=3, dtype="bf16")
    frames0 = rng.integers(0, 256, (3, 76, 102, 3), dtype=np.uint8)
    _state(lambda: eng.draw_faces(frames0.copy(), "bgr"))                  # before any forward
    src, base = _feed_until_faces(eng, how, rng, need=4)                    # four faces in three images: one image has two
    rows = _rows(base)
    net = (64, 96)
    bgr_o, yuv_o = opt(label_scale=2), yuv_opt(opt(label_scale=2, thickness=2))
    _engine_case(eng, "bgr", 76, 102, rows, net, **bgr_o)
    _engine_case(eng, "nv12", 76, 102, rows, net, **yuv_o)
    _engine_case(eng, "bgr", 75, 101, rows, net, dense=True, **opt(scale=1.3, label="none"))
    _engine_case(eng, "yv12", 128, 256, rows, net, dense=True, **yuv_opt(opt(label_scale=3)))
    # the track id is only known behind an update; nothing is written
    keep = frames0.copy()
    _state(lambda: eng.draw_faces(keep, "bgr", **opt(label="id")))
    assert np.array_equal(keep, frames0)
    with pytest.raises(ValueError):
        eng.draw_faces(frames0[:2].copy(), "bgr", **bgr_o)                  # B is not the forward's
    with pytest.raises(ValueError):
        eng.draw_faces(frames0.copy(), "bgr", **opt(thickness=0))
    # the call changed no state: a redaction behind the draws gives the bytes it gives on a fresh copy, and the decode's rows are unchanged
    a = frames0.copy()
    eng.draw_faces(a, "bgr", **bgr_o)
    b = frames0.copy()
    eng.redact_faces(b, "bgr", mode="mosaic", shape="ellipse", cell=6)
    ref = frames0.copy()
    redact_ref([(f.reshape(76, -1),) for f in ref], "bgr", rows[0], rows[3], net, 76, 102, mode="mosaic", shape="ellipse", cell=6)
    assert np.array_equal(b, ref) and not np.array_equal(b, frames0)
    c = frames0.copy()
    eng.draw_faces(c, "bgr", **bgr_o)                                       # a second draw: the same picture
    assert np.array_equal(a, c)
    again = eng.decode_threshold(0.3, 0.3, 64)
    assert all(d.tobytes() == d0.tobytes() and l.tobytes() == l0.tobytes() for (d, l), (d0, l0) in zip(again, base))
    # the device form, on device_alloc planes and on torch tensors, equals the host form: padding and guards included
    import torch
    for fmt, o in (("bgr", bgr_o), ("nv12", yuv_o), ("yv12", yuv_o)):
        p0, p1 = pitches_for(fmt, 102, aligned=True)
        fr = Frames(np.random.default_rng(13), fmt, 3, 76, 102, p0, p1, False)
        want = fr.clone()
        draw_ref(want.views, fmt, *rows[:2], rows[3], net, 76, 102, lms=rows[2], info=None, **o)
        n = len(fr.geo)
        if fmt == "nv12":
            tens = [torch.from_numpy(b.copy()).cuda() for b in fr.bufs]
            dev = [t.data_ptr() for t in tens]
        else:
            dev = [eng.device_alloc(b.nbytes) for b in fr.bufs]
            for d, b in zip(dev, fr.bufs):
                eng.memcpy_h2d(d, b)
        eng.draw_faces_device([tuple(dev[b * n:(b + 1) * n]) for b in range(3)], fmt, 3, 76, 102, p0, p1, **o)
        eng.synchronize()
        if fmt == "nv12":
            for t, b in zip(tens, fr.bufs):
                b[:] = t.cpu().numpy()
        else:
            for d, b in zip(dev, fr.bufs):
                eng.memcpy_d2h(b, d)
        assert fr.same(want), (fmt, fr.diff(want))
        with pytest.raises(ValueError):                                    # a misaligned device plane, a pitch that is no multiple of 4
            eng.draw_faces_device([(dev[b * n] + 2,) + tuple(dev[b * n + 1:(b + 1) * n]) for b in range(3)], fmt, 3, 76, 102, p0, p1, **o)
        with pytest.raises(ValueError):
            eng.draw_faces_device([tuple(dev[b * n:(b + 1) * n]) for b in range(3)], fmt, 3, 76, 102, p0 + 2, p1, **o)
        if fmt != "nv12":
            for d in dev:
                eng.device_free(d)
    # a decode that wrote one row per image while its counts say more: only the rows written are drawn (min(count, rows_cap))
    L, P = cfa._lib.lib(), cfa._lib.ptr
    d5, l10, cn = np.empty((3, 1, 5), np.float32), np.empty((3, 1, 10), np.float32), np.empty(3, np.int32)
    assert L.cf_decode_threshold(eng._h, 0.3, 0.3, 1, P(d5), P(l10), P(cn)) == 0
    assert np.array_equal(cn, rows[3]) and cn.max() >= 2
    firsts = _rows([(d[:1], l[:1]) for d, l in base])
    _engine_case(eng, "bgr", 76, 102, firsts, net, differs_from=rows, **bgr_o)      # (the first rows alone may all be skipped ones)
    eng.close()


@pytest.mark.parametrize("fmt", ("bgr", "nv12"))
def test_draw_after_a_merge_uses_the_merged_rows(fmt):
    from test_tiles import tiled_engine, pitched_frames, FRAME_HW
    eng, dense, rects, thr = tiled_engine(fmt, seed=1)
    h, w = FRAME_HW
    eng.decode_threshold(thr, 0.5, 256)
    o = opt(label_scale=2) if fmt == "bgr" else yuv_opt(opt(label_scale=2))
    views, bufs, _, _ = pitched_frames(dense, fmt, 0xA5)
    _state(lambda: eng.draw_faces(views, fmt, **o))                         # a tiled forward and a decode, but no merge
    merged, _ = eng.merge_tiles(max_out=256)
    boxes, scores, lms, counts = _rows(merged)
    assert int(counts.sum()) >= 2
    views, bufs, _, _ = pitched_frames(dense, fmt, 0xA5)
    wviews, wbufs, _, _ = pitched_frames(dense, fmt, 0xA5)
    draw_ref(wviews, fmt, boxes, scores, counts, (h, w), h, w, lms=lms, info=None, **o)      # frame pixels: (H, W) = (h, w), fx = fy = 1
    assert eng.draw_faces(views, fmt, **o) is views
    assert all(np.array_equal(a, b) for a, b in zip(bufs, wbufs))
    assert not all(np.array_equal(a, b) for a, b in zip(bufs, pitched_frames(dense, fmt, 0xA5)[1]))
    eng.close()


def test_draw_behind_the_tracker_shows_held_tracks():
    """Three frames with a dropout in the middle: the rows of track_update, ids as labels; the held rows of the blank frame are drawn
    dashed in held_color with their id and without dots."""
    from test_track import _blank_batch
    rng = np.random.default_rng(3)
    eng = cfa.Engine(64, 96, max_batch=3, dtype="bf16")
    trk = cfa.Tracker(eng, 3, iou=0.3, max_age=3, min_hits=1, max_tracks=70, hold_grow=0.1)
    net = (64, 96)
    o = opt(label="id", label_scale=1)

    def check(got, fmt, oo):
        rows = _rows(got)
        info = np.concatenate([np.stack([g[2], g[3], g[4]], 1) for g in got]).astype(np.int32)
        return _engine_case(eng, fmt, 76, 102, rows, net, info=info, **oo), info
    src, base = _feed_until_faces(eng, "resized", rng)
    got, _ = eng.track_update(trk)
    assert sum(len(g[0]) for g in got) >= 2
    _, info = check(got, "bgr", o)
    assert (info[:, 2] == 0).all() and (info[:, 0] > 0).all()
    # the dropout
    assert sum(len(d) for d, _ in _blank_batch(eng)) == 0
    plain = rng.integers(0, 256, (3, 76, 102, 3), dtype=np.uint8)
    keep = plain.copy()
    eng.draw_faces(keep, "bgr", **opt())                                    # without an update: the decode's rows, none
    assert np.array_equal(keep, plain)
    held, _ = eng.track_update(trk)
    assert sum(len(g[0]) for g in held) >= 2 and all((g[4] == 1).all() for g in held)
    fr, info = check(held, "bgr", o)
    check(held, "nv12", yuv_opt(o))
    # only layers 1 (held_color) and 3 (text_color) are in the picture: no box_color, no lm_color byte triple was written
    boxes, scores, lms, counts = _rows(held)
    maps = draw_ref(fr.clone().views, "bgr", boxes, scores, counts, net, 76, 102, lms=lms, info=info, **o)
    seen = set(np.unique(np.concatenate([m.reshape(-1) for m in maps])).tolist())
    assert seen == {0, 1, 3}, seen
    # the faces come back
    eng.forward_resized_enqueue(src)
    eng.decode_threshold(0.3, 0.3, 64)
    back, _ = eng.track_update(trk)
    _, info = check(back, "bgr", o)
    assert (info[:, 2] == 0).any() and (info[:, 1] >= 2).any()             # matched again: the ids of the first frame
    assert set(np.concatenate([g[2] for g in back]).tolist()) >= set(np.concatenate([g[2] for g in got]).tolist())
    trk.close(), eng.close()


def test_centerface_annotate():
    """annotate / annotate_yuv: the inputs stay, the detections are detect_batch's / detect_yuv's, and the outputs are the bytes of
    Engine.draw_faces behind the same forward -- the restatement on its network rows with the reference's look."""
    rng = np.random.default_rng(31)
    hw = (76, 102)
    face = cfa.CenterFace(*hw, dtype="bf16", max_batch=3)
    from test_redact import source_frames
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        imgs = list(source_frames(rng, kind, (3,) + hw + (3,)))
        want = face.detect_batch(imgs)
        if sum(len(d) for d, _ in want) >= 1:
            break
    keep = [im.copy() for im in imgs]
    out, dets = face.annotate(imgs)
    assert all(np.array_equal(a, b) for a, b in zip(imgs, keep)) and out.shape == (3,) + hw + (3,) and out.dtype == np.uint8
    assert all(d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes() for (d, l), (wd, wl) in zip(dets, want))
    o = dict(what=3, thickness=1, radius=2, label="score", label_scale=2, dash_held=1, scale=1.0, **LOOK)
    same = np.stack(keep)
    face.engine.draw_faces(same, "bgr", **o)                                # the engine still holds the forward
    rows = _rows(face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets))
    ref = np.stack(keep)
    draw_ref([(f.reshape(hw[0], -1),) for f in ref], "bgr", rows[0], rows[1], rows[3], (face.img_h_new, face.img_w_new), hw[0], hw[1], lms=rows[2], **o)
    assert np.array_equal(out, same) and np.array_equal(out, ref) and not np.array_equal(out, np.stack(keep))
    out2, _ = face.annotate(imgs, label="none", box_color=(9, 8, 7), thickness=2)
    ref = np.stack(keep)
    draw_ref([(f.reshape(hw[0], -1),) for f in ref], "bgr", rows[0], rows[1], rows[3], (face.img_h_new, face.img_w_new), hw[0], hw[1], lms=rows[2],
             **dict(o, label="none", box_color=(9, 8, 7), thickness=2))
    assert np.array_equal(out2, ref)
    # 4:2:0: the BGR colours are converted
    for kind in ("noise", "binary", "blocks", "noise", "binary", "blocks"):
        yuv = source_frames(rng, kind, (3, hw[0] * 3 // 2, hw[1]))
        wanty = face.detect_yuv(yuv, "nv12")
        if sum(len(d) for d, _ in wanty) >= 1:
            break
    keepy = yuv.copy()
    outy, detsy = face.annotate_yuv(yuv, "nv12")
    assert np.array_equal(yuv, keepy) and outy.shape == yuv.shape
    assert all(d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes() for (d, l), (wd, wl) in zip(detsy, wanty))
    samey = keepy.copy()
    face.engine.draw_faces(samey, "nv12", **yuv_opt(o))
    rows = _rows(face.engine.decode_threshold(0.3, face.nms_thresh, face.max_dets))
    refy = keepy.copy()
    draw_ref([(f[:hw[0]], f[hw[0]:]) for f in refy], "nv12", rows[0], rows[1], rows[3], (face.img_h_new, face.img_w_new), hw[0], hw[1], lms=rows[2], **yuv_opt(o))
    assert np.array_equal(outy, samey) and np.array_equal(outy, refy) and not np.array_equal(outy, keepy)
    # with a tracker the label is the id
    trk = cfa.Tracker(face.engine, 3, min_hits=1, max_age=2)
    outt, _ = face.annotate(imgs, tracker=trk)
    samet = np.stack(keep)
    face.engine.draw_faces(samet, "bgr", **dict(o, label="id"))
    assert np.array_equal(outt, samet) and not np.array_equal(outt, out)
    trk.close(), face.close()


def test_centerface_annotate_tiled():
    """annotate(tiled=True): a copy drawn with the merged rows, which are the returned detections (frame pixels: fx = fy = 1)."""
    from test_redact import source_frames
    from test_tiles import ENG_HW, FRAME_HW
    rng = np.random.default_rng(2)
    h, w = FRAME_HW
    face = cfa.CenterFace(ENG_HW[0], ENG_HW[1], dtype="bf16", max_batch=24)
    for kind in ("blocks", "binary", "noise", "blocks", "binary", "noise"):
        imgs = source_frames(rng, kind, (3, h, w, 3))
        if sum(len(d) for d, _ in face.detect_tiled(imgs)) >= 2:
            break
    keep = imgs.copy()
    out, dets = face.annotate(list(imgs), tiled=True, thickness=2)
    assert np.array_equal(imgs, keep) and sum(len(d) for d, _ in dets) >= 2
    rows = _rows(dets)
    ref = keep.copy()
    draw_ref([(f.reshape(h, -1),) for f in ref], "bgr", rows[0], rows[1], rows[3], (h, w), h, w, lms=rows[2],
             **dict(what=3, thickness=2, radius=2, label="score", label_scale=2, dash_held=1, scale=1.0, **LOOK))
    assert np.array_equal(out, ref) and not np.array_equal(out, keep)
    face.close()
