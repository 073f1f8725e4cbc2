#!/usr/bin/env python3
"""Face redaction in device-resident 1080p frames: B = 16 frames of 1080 x 1920, NV12 and BGR, behind a 544 x 960 bf16 engine that reads
the NV12 surfaces in place (cf_forward_yuv, in_on_device = 1) and a threshold decode with max_out = 8 -- so at most 8 faces per frame,
at a score threshold lowered until every frame has its 8 (the synthetic weights decide where they are; the boxes are read back once, for
the mask areas reported, never inside a timed window).

What is timed, after warming up every launch involved:
  <fmt>_<mode>_us   the redaction ALONE (cf_redact_faces, on_device = 1, ellipse, scale 1.3, cell 20): HIP events on the engine's main
                    stream around 20 back-to-back calls on the same planes, divided by 20; median and spread of 7 such windows
  forward_ms_per_step   host clock around 20 steps of forward + threshold decode enqueue ending in a synchronise, median of 7 windows
and, from the boxes, per format: the samples the masks cover (union per frame), the algorithmic bytes (SOLID: the mask written once;
MOSAIC: read once and written once) and the GB/s that the median time makes of them.  One JSON line.
--short: a few calls only, for a rocprofv3 --kernel-trace --stats run of its own (kernels: redact_means_kernel, redact_write_kernel)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa

short = "--short" in sys.argv
B, h, w, H, W, MAXF, REP, WIN = 16, 1080, 1920, 544, 960, 8, 20, 7
SCALE, CELL = 1.3, 20
rng = np.random.default_rng(0)
eng = cfa.Engine(H, W, max_batch=B, dtype="bf16", decode_stream=False)
L, P = cfa._lib.lib(), cfa._lib.ptr

# coarse noise (8-pixel blocks): detail that survives the 2x downsize to the network
small = rng.integers(0, 256, (B, h * 3 // 2 // 8 + 1, w // 8), dtype=np.uint8)
nv12 = np.ascontiguousarray(np.repeat(np.repeat(small, 8, 1), 8, 2)[:, :h * 3 // 2, :w])
bgr = np.ascontiguousarray(np.repeat(np.repeat(rng.integers(0, 256, (B, h // 8, w // 8, 3), dtype=np.uint8), 8, 1), 8, 2))
# the forward reads a copy of its own, so the faces (and the mask areas reported) stay what they are while the other copies are redacted
d_src, d_nv12, d_bgr = eng.device_alloc(nv12.nbytes), eng.device_alloc(nv12.nbytes), eng.device_alloc(bgr.nbytes)
eng.memcpy_h2d(d_src, nv12)
eng.memcpy_h2d(d_nv12, nv12)
eng.memcpy_h2d(d_bgr, bgr)
one = h * w * 3 // 2
planes = {"nv12": [(d_nv12 + b * one, d_nv12 + b * one + h * w) for b in range(B)], "bgr": [(d_bgr + b * h * w * 3,) for b in range(B)]}
pitch = {"nv12": (w, w), "bgr": (3 * w, 0)}
source = [(d_src + b * one, d_src + b * one + h * w) for b in range(B)]


def forward():
    eng.forward_yuv_enqueue(source, "nv12", on_device=True, h=h, w=w)


def decode_rows(thr):
    dets, lms, counts = np.zeros((B, MAXF, 5), np.float32), np.zeros((B, MAXF, 10), np.float32), np.zeros(B, np.int32)
    eng._chk(L.cf_decode_threshold(eng._h, thr, 0.3, MAXF, P(dets), P(lms), P(counts)))
    return dets, np.minimum(counts, MAXF)


forward()
for thr in (0.3, 0.1, 0.03, 0.01, 0.001):
    dets, rows = decode_rows(thr)
    if int(rows.min()) == MAXF:
        break


def masks(chroma):
    """samples covered per frame (union of the faces' ellipses), luma / BGR pixels or chroma samples: the statement of csrc/cf_redact.hip"""
    total = 0
    rr, cc = (h // 2, w // 2) if chroma else (h, w)
    U = (4 * np.arange(cc, dtype=np.int64) + 2) if chroma else (2 * np.arange(cc, dtype=np.int64) + 1)
    V = (4 * np.arange(rr, dtype=np.int64) + 2) if chroma else (2 * np.arange(rr, dtype=np.int64) + 1)
    for b in range(B):
        cov = np.zeros((rr, cc), bool)
        for x1, y1, x2, y2 in dets[b, :rows[b], :4].astype(np.float64):
            cx, cy, hw, hh = (x1 + x2) * 0.5, (y1 + y2) * 0.5, (x2 - x1) * 0.5 * np.float64(np.float32(SCALE)), (y2 - y1) * 0.5 * np.float64(np.float32(SCALE))
            if not (np.isfinite([x1, y1, x2, y2]).all() and hw > 0 and hh > 0):
                continue
            X1, X2 = int(np.floor((cx - hw) * (w / W))), int(np.ceil((cx + hw) * (w / W)))
            Y1, Y2 = int(np.floor((cy - hh) * (h / H))), int(np.ceil((cy + hh) * (h / H)))
            X1, Y1, X2, Y2 = X1 - X1 % 2, Y1 - Y1 % 2, X2 + X2 % 2, Y2 + Y2 % 2
            A, Bv = X2 - X1, Y2 - Y1
            cov |= (((U - (X1 + X2)) * Bv) ** 2)[None, :] + (((V - (Y1 + Y2)) * A) ** 2)[:, None] <= (A * Bv) ** 2
        total += int(cov.sum())
    return total


def redact(fmt, mode):
    eng.redact_faces_device(planes[fmt], fmt, B, h, w, pitch[fmt][0], pitch[fmt][1], mode=mode, shape="ellipse", cell=CELL, scale=SCALE,
                            fill=(16, 128, 128) if fmt == "nv12" else (0, 0, 0))


def step():
    forward()
    eng.decode_threshold_enqueue(thr, 0.3, MAXF)


for _ in range(3):                                                              # warm-up: graph capture, code objects, the cell scratch
    step()
    for fmt in planes:
        for mode in ("solid", "mosaic"):
            redact(fmt, mode)
eng.synchronize()
luma, chroma = masks(False), masks(True)
out = {"shape": "%d x %dx%d frames, engine %dx%d bf16, ellipse, scale %.1f, cell %d" % (B, h, w, H, W, SCALE, CELL),
       "score_thresh": thr, "faces": int(rows.sum()), "mask_px": luma, "mask_px_share": round(luma / (B * h * w), 4)}
if not short:
    for fmt in planes:
        mask_bytes = luma * 3 if fmt == "bgr" else luma + 2 * chroma
        for mode in ("solid", "mosaic"):
            us = []
            for _ in range(WIN):
                step()
                eng.event_record(0)
                for _ in range(REP):
                    redact(fmt, mode)
                eng.event_record(1)
                eng.synchronize()
                us.append(eng.event_elapsed_ms(0, 1) * 1e3 / REP)
            med = float(np.median(us))
            algo = mask_bytes * (2 if mode == "mosaic" else 1)
            out["%s_%s_us" % (fmt, mode)] = round(med, 2)
            out["%s_%s_us_min_max" % (fmt, mode)] = [round(min(us), 2), round(max(us), 2)]
            out["%s_%s_algo_MB" % (fmt, mode)] = round(algo / 1e6, 3)
            out["%s_%s_algo_GBps" % (fmt, mode)] = round(algo / (med * 1e-6) / 1e9, 1)
    ms = []
    for _ in range(WIN):
        t0 = time.perf_counter()
        for _ in range(REP):
            step()
        eng.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / REP)
    out["forward_ms_per_step"] = round(float(np.median(ms)), 4)
    out["forward_ms_per_step_min_max"] = [round(min(ms), 4), round(max(ms), 4)]
eng.synchronize()
for p in (d_src, d_nv12, d_bgr):
    eng.device_free(p)
eng.close()
print(json.dumps(out))
