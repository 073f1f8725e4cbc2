"""Host-input staging of the runtime (cf_runtime.hip): every host-input form of the engine back to back on ONE context, across the 8 MiB
rule -- below it the copies go on the context's main stream, from it on they go on the device's copy stream -- with no synchronisation
between the calls.  What is pinned is the protocol between the forms (which stream a copy goes on, which event it and the forward
wait for, when a staging buffer may be overwritten or re-allocated), not the arithmetic of any one form: the wanted results come from
a second engine of the same shape that runs every step alone."""

import numpy as np
import pytest

import centerface_amd as cfa

H, W, MAXB, K = 352, 640, 13, 50
RULE = 8 << 20                       # the runtime's threshold between the two regimes, in bytes of one call's copies


def pitched(plane, pad):
    """A view of ``plane``'s rows inside a wider buffer (row stride = row bytes + pad; the padding holds 0xFF)."""
    rows = plane.reshape(plane.shape[0], -1)
    buf = np.full((rows.shape[0], rows.shape[1] + pad), 0xFF, np.uint8)
    buf[:, :rows.shape[1]] = rows
    return buf[:, :rows.shape[1]]


def planes_of(frame, fmt):
    """(y, c0[, c1]) 2-D views of one dense [h*3//2, w] frame."""
    rows, w = frame.shape
    h = rows * 2 // 3
    if fmt in ("nv12", "nv21"):
        return frame[:h], frame[h:]
    q = (h // 2) * (w // 2)
    rest = frame[h:].reshape(-1)
    return frame[:h], rest[:q].reshape(h // 2, w // 2), rest[q:].reshape(h // 2, w // 2)


def forward_yuv_pitched(eng, frames, fmt, pad_y, pad_c):
    """cf_forward_yuv on host planes whose rows are padded (Engine.forward_yuv_enqueue takes dense host frames only)."""
    L, f = cfa._lib.lib(), cfa._lib.yuv_format(fmt)
    h, w = frames.shape[1] * 2 // 3, frames.shape[2]
    keep = [[pitched(p, pad_y if k == 0 else pad_c) for k, p in enumerate(planes_of(fr, fmt))] for fr in frames]
    descs = (cfa._lib.YuvPlanes * len(frames))()
    for d, pl in zip(descs, keep):
        d.y, d.c0, d.c1 = pl[0].ctypes.data, pl[1].ctypes.data, pl[2].ctypes.data if len(pl) > 2 else None
    eng._chk(L.cf_forward_yuv(eng._h, f, descs, 0, len(frames), h, w, pl[0].strides[0], pl[1].strides[0]))
    eng.last_B = len(frames)
    return keep


@pytest.mark.gpu
@pytest.mark.isolated
def test_host_input_forms_back_to_back():
    """One bf16 engine of 352 x 640, max_batch 13 (13 network-sized images = 8.79 MB, just over the rule).  Fifteen steps, every host-input
    form once under and once over the rule (over: 2 BGR frames of 1200 x 1280 = 9.2 MB, 2 4:2:0 frames of 1536 x 1920 = 8.8 MB, 13
    network-sized images), the yuv and tiled forms also with padded rows and the yuv form with 50 x 70 I420 frames (chroma rows of 35
    bytes).  The order gives, for the users of the two network-sized slots (S) and separately for the users of the source-frame staging
    buffer (F), every ordered pair of regimes (m = main stream, c = copy stream), and the staging buffer grows twice after it has been
    used (step 3 on the main stream, step 5 on the copy stream):

         1 resized 1 x 90 x 110          F m        9 yuv i420 3 x 50 x 70          F m  (c -> m)
         2 images 2 x network size       S m       10 upload + forward 1 x network  S m  (c -> m)
         3 yuv nv12 2 x 96 x 128         F m (m -> m, grows)   11 tiles bgr 2 x 1200 x 1280, T = 4   F c  (m -> c)
         4 plain 1                       S m (m -> m)          12 yuv i420 2 x 1536 x 1920           F c  (c -> c)
         5 resized 2 x 1200 x 1280       F c (m -> c, grows)   13 tiles nv12 2 x 72 x 96, T = 3      F m  (c -> m)
         6 plain 13                      S c (m -> c)          14 yuv nv12 2 x 64 x 96, padded rows  F m  (m -> m)
         7 upload + forward 2 x 1200 x 1280  F c (c -> c)      15 tiles bgr 2 x 72 x 96, padded rows F m
         8 images 13 x network size      S c (c -> c)

    The sequence runs twice without a synchronisation between the steps (eager, then the replayed graphs), each step followed by a
    device-output top-K decode into buffers of its own; after the one synchronize() at the end of a pass every step's dets, lms and
    inds equal those of the same step run alone, and read out at once, on the second engine."""
    rng = np.random.default_rng(2024)
    u8 = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)      # noqa: E731
    net1, net13 = u8(1, H, W, 3), u8(13, H, W, 3)
    imgs2, imgs13, up1 = [u8(H, W, 3) for _ in range(2)], [u8(H, W, 3) for _ in range(13)], [u8(H, W, 3)]       # pageable, one allocation each
    small, big = u8(1, 90, 110, 3), u8(2, 1200, 1280, 3)
    big_list = [u8(1200, 1280, 3) for _ in range(2)]
    nv12_s, i420_odd, i420_big, nv12_p = u8(2, 144, 128), u8(3, 75, 70), u8(2, 2304, 1920), u8(2, 96, 96)
    tile_nv12, tile_bgr = u8(2, 108, 96), u8(2, 72, 96, 3)
    tile_bgr_p = [(pitched(f.reshape(72, 288), 10),) for f in tile_bgr]
    rects_big = [(0, 0, 1280, 1200), (0, 0, 640, 352), (640, 600, 640, 600), (320, 424, 642, 354)]
    rects_small = [(0, 0, 96, 72), (10, 20, 64, 32), (32, 0, 64, 72)]
    for over in (net13, big, i420_big):
        assert over.nbytes > RULE
    assert sum(a.nbytes for a in imgs13) > RULE and sum(a.nbytes for a in big_list) > RULE
    for under in (net1, small, nv12_s, i420_odd, nv12_p, tile_nv12, tile_bgr):
        assert under.nbytes < RULE
    assert small.nbytes < nv12_s.nbytes < big.nbytes                 # the staging buffer grows at steps 3 and 5

    def upload_then_forward(e, images):
        e.upload_images(images)
        e.forward_uploaded()
    steps = [                                                          # (B, the call)
        (1, lambda e: e.forward_resized_enqueue(small)),
        (2, lambda e: e.forward_images_enqueue(imgs2)),
        (2, lambda e: e.forward_yuv_enqueue(nv12_s, "nv12")),
        (1, lambda e: e.forward_enqueue(net1)),
        (2, lambda e: e.forward_resized_enqueue(big)),
        (13, lambda e: e.forward_enqueue(net13)),
        (2, lambda e: upload_then_forward(e, big_list)),
        (13, lambda e: e.forward_images_enqueue(imgs13)),
        (3, lambda e: e.forward_yuv_enqueue(i420_odd, "i420")),
        (1, lambda e: upload_then_forward(e, up1)),
        (8, lambda e: e.forward_tiles_enqueue(big, rects_big, "bgr")),
        (2, lambda e: e.forward_yuv_enqueue(i420_big, "i420")),
        (6, lambda e: e.forward_tiles_enqueue(tile_nv12, rects_small, "nv12")),
        (2, lambda e: forward_yuv_pitched(e, nv12_p, "nv12", 10, 6)),
        (6, lambda e: e.forward_tiles_enqueue(tile_bgr_p, rects_small, "bgr")),
    ]
    ref = cfa.Engine(H, W, max_batch=MAXB, dtype="bf16")
    want = []
    for B, step in steps:
        held = step(ref)                                               # (alive until the decode has waited for the forward)
        assert ref.last_B == B
        want.append(ref.decode_topk(K))
        del held
    ref.close()

    eng = cfa.Engine(H, W, max_batch=MAXB, dtype="bf16")
    outs = [(eng.device_alloc(B * K * 24), eng.device_alloc(B * K * 40), eng.device_alloc(B * K * 8)) for B, _ in steps]
    for rnd in ("eager", "graphs"):
        held = []                                                      # whatever a step allocated for its call
        for (B, step), o in zip(steps, outs):
            held.append(step(eng))
            eng.decode_topk_device(K, *o)
        eng.synchronize()
        for i, ((B, _), o, (wd, wl, wi)) in enumerate(zip(steps, outs, want)):
            dets, lms, inds = np.empty((B, K, 6), np.float32), np.empty((B, K, 10), np.float32), np.empty((B, K), np.int64)
            eng.memcpy_d2h(dets, o[0])
            eng.memcpy_d2h(lms, o[1])
            eng.memcpy_d2h(inds, o[2])
            assert np.array_equal(dets, wd), (rnd, i + 1, "dets")
            assert np.array_equal(lms, wl), (rnd, i + 1, "lms")
            assert np.array_equal(inds, wi), (rnd, i + 1, "inds")
    for o in outs:
        for p in o:
            eng.device_free(p)
    eng.close()
