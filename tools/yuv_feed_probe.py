#!/usr/bin/env python3
"""Host-fed steps from page-locked memory, BGR against NV12 (cf_forward_yuv): 64 x 640x640 bf16 + a top-100 decode into device buffers,
one context and the ring of two.  A BGR batch is 78.6 MB over the link, the same frames as NV12 39.3 MB (converted on the device).
BGR and NV12 windows alternate in one process; medians of 7 windows of 20 steps.  One JSON line: images/s and link GB/s of payload.
--short: a few steps of each input and one 1080x1920 -> 1088x1920 convert + resize, for a rocprofv3 --kernel-trace --stats run of
its own (kernel times: yuv_bgr_identity8_kernel at B = 64, yuv_bgr_resize_kernel at 1080p)."""
import os, sys, time, json
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa
from centerface_amd import ops

short = "--short" in sys.argv
B, S, K = 64, 640, 100
per_img = {"bgr": S * S * 3, "nv12": S * S * 3 // 2}
rng = np.random.default_rng(0)
out = {"images_per_s": {}, "GBps": {}}
for depth in ((2,) if short else (1, 2)):
    ring = cfa.EngineRing(S, S, depth=depth, max_batch=B, dtype="bf16")
    e0 = ring.engines[0]
    bgr = [e0.pinned_array((B, S, S, 3)) for _ in range(2 * depth)]
    nv12 = [e0.pinned_array((B, S * 3 // 2, S)) for _ in range(2 * depth)]
    for a in bgr + nv12:
        a[...] = rng.integers(0, 256, a.shape, dtype=np.uint8)
    outs = [(e.device_alloc(B * K * 24), e.device_alloc(B * K * 40), e.device_alloc(B * K * 8)) for e in ring.engines]

    def step(i, kind):
        e, o = ring.engines[i % depth], outs[i % depth]
        if kind == "bgr":
            e.forward_enqueue(bgr[i % len(bgr)])
        else:
            e.forward_yuv_enqueue(nv12[i % len(nv12)], "nv12")
        e.decode_topk_device(K, o[0], o[1], o[2])
    for kind in ("bgr", "nv12"):
        for i in range(3 if short else 8):
            step(i, kind)
        ring.synchronize()
    if short:
        ring.close()
        break
    rates = {"bgr": [], "nv12": []}
    for _ in range(7):
        for kind in ("bgr", "nv12"):
            t0 = time.perf_counter()
            for i in range(20):
                step(i, kind)
            ring.synchronize()
            rates[kind].append(B * 20 / (time.perf_counter() - t0))
    for kind, r in rates.items():
        v = float(np.median(r))
        out["images_per_s"]["%s_depth_%d" % (kind, depth)] = round(v, 1)
        out["GBps"]["%s_depth_%d" % (kind, depth)] = round(v * per_img[kind] / 1e9, 1)
    ring.close()
if short:
    frame = rng.integers(0, 256, (1, 1620, 1920), dtype=np.uint8)
    for _ in range(5):
        ops.yuv_to_bgr(frame, "nv12", size=(1088, 1920))
    out = {"short": True}
print(json.dumps(out))
