#!/usr/bin/env python3
"""Tiled detection of device-resident 1080p NV12 frames: Bf = 7 frames of 1080 x 1920, nine 640 x 640 tiles each (the 4 x 2 grid with
128 pixels of overlap plus the whole frame: 63 images), behind a 640 x 640 bf16 engine that reads the surfaces in place
(cf_forward_tiles, in_on_device = 1), a per-tile threshold decode with max_out = 64 at a score threshold lowered until every tile keeps
rows, and the merge (cf_merge_tiles, device form, IoS 0.5, edge 2).

What is timed, after warming up every launch involved (host clock around REP steps ending in a synchronise, median and spread of WIN
windows; `step` = forward + threshold decode enqueue [+ merge]):
  step_tiled_ms     cf_forward_tiles + decode + merge: the tiled step
  step_ready_ms     cf_forward_yuv of 63 ready-made 640 x 640 NV12 frames + decode: the same network batch with nothing to cut or merge;
                    the difference of the two is what cutting and merging cost
  step_resize_ms    cf_forward_yuv of 63 NV12 frames of 720 x 720 + decode: the whole-frame convert + resize kernel writing the same
                    number of output bytes as the cutter
and with HIP events on the engine's main stream around REP back-to-back calls:
  merge_us          cf_merge_tiles alone (collect + rank + mask + sweep over Bf frames x 9 x 64 candidate slots)
  decode_us         the threshold decode alone (collect + rank + mask + sweep over 63 images), the yardstick for the merge
The cutter and the convert + resize kernel have no entry point of their own: their kernel times come from a
`rocprofv3 --kernel-trace --stats` run of `tile_probe.py --short` (kernels: cut_tiles_kernel, yuv_bgr_resize_kernel,
collect_rows_kernel).  One JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa
from centerface_amd import ops

short = "--short" in sys.argv
Bf, h, w, S, MAXF, REP, WIN = 7, 1080, 1920, 640, 64, 20, 7
RS = 720                                                                        # the frames of step_resize
rng = np.random.default_rng(0)
rects = ops.tile_grid(h, w, S, 128)
T = len(rects)
assert T == 9
B = Bf * T
eng = cfa.Engine(S, S, max_batch=B, dtype="bf16", decode_stream=False)
L, P = cfa._lib.lib(), cfa._lib.ptr


def coarse(n, hh, ww):
    """NV12 frames of coarse noise (8-pixel blocks): detail that survives a resize"""
    small = rng.integers(0, 256, (n, hh * 3 // 2 // 8 + 1, ww // 8), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(small, 8, 1), 8, 2)[:, :hh * 3 // 2, :ww])


def on_device(frames, hh, ww):
    d = eng.device_alloc(frames.nbytes)
    eng.memcpy_h2d(d, frames)
    one = hh * ww * 3 // 2
    return d, [(d + b * one, d + b * one + hh * ww) for b in range(frames.shape[0])]


d_full, full = on_device(coarse(Bf, h, w), h, w)
d_ready, ready = on_device(coarse(B, S, S), S, S)
d_rs, resize = on_device(coarse(B, RS, RS), RS, RS)
d_out = [eng.device_alloc(Bf * MAXF * 5 * 4), eng.device_alloc(Bf * MAXF * 10 * 4), eng.device_alloc(Bf * 4), eng.device_alloc(Bf * 4)]


def decode_counts(thr):
    dets, lms, counts = np.zeros((B, MAXF, 5), np.float32), np.zeros((B, MAXF, 10), np.float32), np.zeros(B, np.int32)
    eng._chk(L.cf_decode_threshold(eng._h, thr, 0.3, MAXF, P(dets), P(lms), P(counts)))
    return counts


eng.forward_tiles_enqueue(full, rects, "nv12", on_device=True, h=h, w=w)
for thr in (0.3, 0.1, 0.03, 0.01, 0.001):
    counts = decode_counts(thr)
    if int(counts.min()) >= 8:
        break


def merge():
    eng.merge_tiles_device(MAXF, *d_out, metric="ios", thresh=0.5, edge=2.0)


def decode():
    eng.decode_threshold_enqueue(thr, 0.3, MAXF)


def step_tiled():
    eng.forward_tiles_enqueue(full, rects, "nv12", on_device=True, h=h, w=w)
    decode()
    merge()


def step_ready():
    eng.forward_yuv_enqueue(ready, "nv12", on_device=True, h=S, w=S)
    decode()


def step_resize():
    eng.forward_yuv_enqueue(resize, "nv12", on_device=True, h=RS, w=RS)
    decode()


steps = {"step_tiled_ms": step_tiled, "step_ready_ms": step_ready, "step_resize_ms": step_resize}
for _ in range(3):                                                              # warm-up: graph capture, code objects, workspaces
    for fn in steps.values():
        fn()
eng.synchronize()
step_tiled()
merged = np.zeros(Bf, np.int32)
eng.synchronize()
eng.memcpy_d2h(merged, d_out[2])
out = {"shape": "%d x %dx%d NV12 frames, %d tiles each, engine %dx%d bf16, decode max_out %d" % (Bf, h, w, T, S, S, MAXF),
       "score_thresh": thr, "rows_per_tile_min_max": [int(np.minimum(counts, MAXF).min()), int(np.minimum(counts, MAXF).max())],
       "candidates_per_frame": np.minimum(counts, MAXF).reshape(Bf, T).sum(1).tolist(), "merged_per_frame": merged.tolist(),
       "cut_out_MB": round(B * S * S * 3 / 1e6, 2)}
if not short:
    ms = {k: [] for k in steps}                                                  # the three steps alternate, window by window
    for _ in range(WIN):
        for k, fn in steps.items():
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(REP):
                fn()
            eng.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / REP)
    for k, v in ms.items():
        out[k] = round(float(np.median(v)), 4)
        out[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    out["cut_and_merge_share_of_step"] = round((out["step_tiled_ms"] - out["step_ready_ms"]) / out["step_tiled_ms"], 4)
    step_tiled()
    for name, fn in (("merge_us", merge), ("decode_us", decode)):
        us = []
        for _ in range(WIN):
            eng.event_record(0)
            for _ in range(REP):
                fn()
            eng.event_record(1)
            eng.synchronize()
            us.append(eng.event_elapsed_ms(0, 1) * 1e3 / REP)
        out[name] = round(float(np.median(us)), 2)
        out[name + "_min_max"] = [round(min(us), 2), round(max(us), 2)]
eng.synchronize()
for p in [d_full, d_ready, d_rs] + d_out:
    eng.device_free(p)
eng.close()
print(json.dumps(out))
