#!/usr/bin/env python3
"""Blur redaction in device-resident 1080p frames: B = 16 NV12 frames of 1080 x 1920 behind a 544 x 960 bf16 engine that reads the
surfaces in place (cf_forward_yuv, in_on_device = 1) and a threshold decode with max_out = 8 -- the set-up of tools/redact_probe.py, so
at most 8 faces per frame, at a score threshold lowered until every frame has its 8 (the synthetic weights decide where they are; the
boxes are read back once, for the face sizes and mask areas reported, never inside a timed window).

What is timed, after warming up every launch involved, with the engine's events on its main stream around 10 back-to-back calls on the
same planes, divided by 10; median and spread of 7 such windows:
  blur_r0_us / blur_r8_us / blur_r24_us   cf_blur_faces alone (on_device = 1, ellipse, scale 1.3) at radius 0 (per face), 8 and 24
  mosaic_us                               cf_redact_faces (mosaic, ellipse, cell 20, scale 1.3) on the same frames and boxes, in the same
                                          process: the yardstick, since nothing comparable to the blur has been measured
One JSON line.  --short: a few calls only, for a rocprofv3 --kernel-trace --stats run of its own (kernels: blur_compute_kernel,
blur_write_kernel)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa

short = "--short" in sys.argv
B, h, w, H, W, MAXF, REP, WIN = 16, 1080, 1920, 544, 960, 8, 10, 7
SCALE, CELL = 1.3, 20
rng = np.random.default_rng(0)
eng = cfa.Engine(H, W, max_batch=B, dtype="bf16", decode_stream=False)
L, P = cfa._lib.lib(), cfa._lib.ptr

# coarse noise (8-pixel blocks): detail that survives the 2x downsize to the network
small = rng.integers(0, 256, (B, h * 3 // 2 // 8 + 1, w // 8), dtype=np.uint8)
nv12 = np.ascontiguousarray(np.repeat(np.repeat(small, 8, 1), 8, 2)[:, :h * 3 // 2, :w])
# the forward reads a copy of its own, so the faces stay what they are while the other copy is blurred over and over
d_src, d_nv12 = eng.device_alloc(nv12.nbytes), eng.device_alloc(nv12.nbytes)
eng.memcpy_h2d(d_src, nv12)
eng.memcpy_h2d(d_nv12, nv12)
one = h * w * 3 // 2
planes = [(d_nv12 + b * one, d_nv12 + b * one + h * w) for b in range(B)]
source = [(d_src + b * one, d_src + b * one + h * w) for b in range(B)]

eng.forward_yuv_enqueue(source, "nv12", on_device=True, h=h, w=w)
for thr in (0.3, 0.1, 0.03, 0.01, 0.001):
    dets, lms, counts = np.zeros((B, MAXF, 5), np.float32), np.zeros((B, MAXF, 10), np.float32), np.zeros(B, np.int32)
    eng._chk(L.cf_decode_threshold(eng._h, thr, 0.3, MAXF, P(dets), P(lms), P(counts)))
    rows = np.minimum(counts, MAXF)
    if int(rows.min()) == MAXF:
        break
# the faces that write something (a row with x2 <= x1 or y2 <= y1 is skipped), the smaller side of their scaled boxes in frame pixels,
# the per-face r that radius = 0 makes of it, and the luma samples their ellipses cover (union per frame): csrc/cf_redact.hip's statement
sides, mask_px = [], 0
U, V = 2 * np.arange(w, dtype=np.int64) + 1, 2 * np.arange(h, dtype=np.int64) + 1
for b in range(B):
    cov = np.zeros((h, w), bool)
    for x1, y1, x2, y2 in dets[b, :rows[b], :4].astype(np.float64):
        cx, cy, hw, hh = (x1 + x2) * 0.5, (y1 + y2) * 0.5, (x2 - x1) * 0.5 * np.float64(np.float32(SCALE)), (y2 - y1) * 0.5 * np.float64(np.float32(SCALE))
        if not (np.isfinite([x1, y1, x2, y2]).all() and hw > 0 and hh > 0):
            continue
        X1, X2 = int(np.floor((cx - hw) * (w / W))), int(np.ceil((cx + hw) * (w / W)))
        Y1, Y2 = int(np.floor((cy - hh) * (h / H))), int(np.ceil((cy + hh) * (h / H)))
        X1, Y1, X2, Y2 = X1 - X1 % 2, Y1 - Y1 % 2, X2 + X2 % 2, Y2 + Y2 % 2
        A, Bv = X2 - X1, Y2 - Y1
        sides.append(min(A, Bv))
        cov |= (((U - (X1 + X2)) * Bv) ** 2)[None, :] + (((V - (Y1 + Y2)) * A) ** 2)[:, None] <= (A * Bv) ** 2
    mask_px += int(cov.sum())
sides = np.array(sides if sides else [0])
auto_r = np.clip(sides // 8, 1, 24)

CALLS = {"blur_r0": lambda: eng.blur_faces_device(planes, "nv12", B, h, w, w, w, shape="ellipse", radius=0, scale=SCALE),
         "blur_r8": lambda: eng.blur_faces_device(planes, "nv12", B, h, w, w, w, shape="ellipse", radius=8, scale=SCALE),
         "blur_r24": lambda: eng.blur_faces_device(planes, "nv12", B, h, w, w, w, shape="ellipse", radius=24, scale=SCALE),
         "mosaic": lambda: eng.redact_faces_device(planes, "nv12", B, h, w, w, w, mode="mosaic", shape="ellipse", cell=CELL, scale=SCALE)}
for _ in range(2):                                                              # warm-up: code objects, the scratches
    for call in CALLS.values():
        call()
eng.synchronize()
out = {"shape": "%d x %dx%d NV12 frames, engine %dx%d bf16, ellipse, scale %.1f" % (B, h, w, H, W, SCALE),
       "score_thresh": thr, "rows": int(rows.sum()), "faces_written": len(sides), "mask_px": mask_px,
       "mask_px_share": round(mask_px / (B * h * w), 5), "box_min_side_px_median": int(np.median(sides)), "box_min_side_px_max": int(sides.max()),
       "auto_r_median": int(np.median(auto_r)), "auto_r_max": int(auto_r.max())}
if not short:
    for name, call in CALLS.items():
        us = []
        for _ in range(WIN):
            eng.event_record(0)
            for _ in range(REP):
                call()
            eng.event_record(1)
            eng.synchronize()
            us.append(eng.event_elapsed_ms(0, 1) * 1e3 / REP)
        out["%s_us" % name] = round(float(np.median(us)), 2)
        out["%s_us_min_max" % name] = [round(min(us), 2), round(max(us), 2)]
eng.synchronize()
for p in (d_src, d_nv12):
    eng.device_free(p)
eng.close()
print(json.dumps(out))
