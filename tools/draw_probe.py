#!/usr/bin/env python3
"""Annotation of device-resident 1080p frames beside the mosaic redaction of the same rows: B = 16 NV12 frames of 1080 x 1920 behind a
544 x 960 bf16 engine that reads the surfaces in place (cf_forward_yuv, in_on_device = 1) and a threshold decode with max_out = 8 -- at
most 8 faces per frame, at a score threshold lowered until every frame has its 8 (the synthetic weights decide where they are).

What is timed, after warming up every launch involved -- HIP events on the engine's main stream around 20 back-to-back calls on the same
planes, divided by 20; median and spread of 7 windows, the three candidates alternating window by window in one run:
  draw_us         cf_draw_faces, on_device = 1: outlines (t = 1), dots (r = 2), score labels (k = 2) -- draw_prep_kernel + draw_paint_kernel
  mosaic_us       cf_redact_faces, on_device = 1, mosaic, ellipse, scale 1.3, cell 20, the same rows
  draw_empty_us   cf_draw_faces behind a decode that keeps nothing (all counts 0): the per-tile early-out that every frame pays
and forward_ms_per_step, the host clock around 20 steps of forward + decode enqueue ending in a synchronise.  One JSON line, then the
table of profiles/draw.md.
--short: a few calls only, for a rocprofv3 --kernel-trace --stats run of its own."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa
from centerface_amd import ops

short = "--short" in sys.argv
B, h, w, H, W, MAXF, REP, WIN = 16, 1080, 1920, 544, 960, 8, 20, 7
rng = np.random.default_rng(0)
eng = cfa.Engine(H, W, max_batch=B, dtype="bf16", decode_stream=False)
L, P = cfa._lib.lib(), cfa._lib.ptr

# coarse noise (8-pixel blocks): detail that survives the 2x downsize to the network
small = rng.integers(0, 256, (B, h * 3 // 2 // 8 + 1, w // 8), dtype=np.uint8)
nv12 = np.ascontiguousarray(np.repeat(np.repeat(small, 8, 1), 8, 2)[:, :h * 3 // 2, :w])
# the forward reads a copy of its own, so the faces stay what they are while the other copy is drawn on and redacted
d_src, d_nv12 = eng.device_alloc(nv12.nbytes), eng.device_alloc(nv12.nbytes)
eng.memcpy_h2d(d_src, nv12)
eng.memcpy_h2d(d_nv12, nv12)
one = h * w * 3 // 2
planes = [(d_nv12 + b * one, d_nv12 + b * one + h * w) for b in range(B)]
source = [(d_src + b * one, d_src + b * one + h * w) for b in range(B)]
COLORS = {k: ops.bgr_to_yuv_color(v) for k, v in (("box_color", (2, 255, 0)), ("held_color", (0, 255, 255)), ("lm_color", (0, 0, 255)), ("text_color", (0, 0, 0)))}


def forward():
    eng.forward_yuv_enqueue(source, "nv12", on_device=True, h=h, w=w)


def rows_at(thr):
    dets, lms, counts = np.zeros((B, MAXF, 5), np.float32), np.zeros((B, MAXF, 10), np.float32), np.zeros(B, np.int32)
    eng._chk(L.cf_decode_threshold(eng._h, thr, 0.3, MAXF, P(dets), P(lms), P(counts)))
    return np.minimum(counts, MAXF)


forward()
for thr in (0.3, 0.1, 0.03, 0.01, 0.001):
    rows = rows_at(thr)
    if int(rows.min()) == MAXF:
        break
EMPTY = 2.0                                                                      # no sigmoid reaches it: every count is 0
assert int(rows_at(EMPTY).sum()) == 0


def draw():
    eng.draw_faces_device(planes, "nv12", B, h, w, w, w, thickness=1, radius=2, label="score", label_scale=2, **COLORS)


def mosaic():
    eng.redact_faces_device(planes, "nv12", B, h, w, w, w, mode="mosaic", shape="ellipse", cell=20, scale=1.3)


def step(t):
    forward()
    eng.decode_threshold_enqueue(t, 0.3, MAXF)


CAND = (("draw_us", thr, draw), ("mosaic_us", thr, mosaic), ("draw_empty_us", EMPTY, draw))
for _ in range(3):                                                              # warm-up: graph capture, code objects, the scratches
    for _, t, call in CAND:
        step(t)
        call()
eng.synchronize()
out = {"shape": "%d x %dx%d NV12 frames, engine %dx%d bf16" % (B, h, w, H, W), "score_thresh": thr, "faces": int(rows.sum())}
if not short:
    us = {name: [] for name, _, _ in CAND}
    for _ in range(WIN):
        for name, t, call in CAND:                                              # alternating: every window of one candidate has the others beside it
            step(t)
            eng.event_record(0)
            for _ in range(REP):
                call()
            eng.event_record(1)
            eng.synchronize()
            us[name].append(eng.event_elapsed_ms(0, 1) * 1e3 / REP)
    for name, v in us.items():
        out[name] = round(float(np.median(v)), 2)
        out[name + "_min_max"] = [round(min(v), 2), round(max(v), 2)]
    ms = []
    for _ in range(WIN):
        t0 = time.perf_counter()
        for _ in range(REP):
            step(thr)
        eng.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / REP)
    out["forward_ms_per_step"] = round(float(np.median(ms)), 4)
    out["forward_ms_per_step_min_max"] = [round(min(ms), 4), round(max(ms), 4)]
eng.synchronize()
for p in (d_src, d_nv12):
    eng.device_free(p)
eng.close()
print(json.dumps(out))
if not short:
    print("| call (16 NV12 1080p frames, %d faces) | median us | min .. max us | us per frame |" % out["faces"])
    print("|---|---|---|---|")
    for name, label in (("draw_us", "cf_draw_faces, boxes + dots + score labels"), ("mosaic_us", "cf_redact_faces, mosaic ellipse cell 20"),
                        ("draw_empty_us", "cf_draw_faces, all counts 0")):
        print("| %s | %.2f | %.2f .. %.2f | %.2f |" % ((label, out[name]) + tuple(out[name + "_min_max"]) + (out[name] / B,)))
