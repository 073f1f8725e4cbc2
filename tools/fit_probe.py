#!/usr/bin/env python3
"""The letterbox input stage against the stretch it replaces: 16 NV12 and 16 BGR frames of 1080 x 1920, resident on the device, behind a
640 x 640 bf16 engine that reads them in place.

What is timed, after warming up every launch involved, with HIP events on the engine's main stream around REP back-to-back calls
(median and spread of WIN windows; the steps alternate window by window):
  step_fit_<fmt>_ms       cf_forward_fit: the fit kernel (rw 640, rh 360, dy 140) + the network
  step_stretch_<fmt>_ms   the input stage those frames take today + the network: cf_forward_yuv (NV12: convert + resize kernel) or
                          cf_forward_resized (BGR: resize kernel), both stretching to 640 x 640
  step_ready_ms           cf_forward of a ready-made 640 x 640 uint8 batch on the device: the network alone
  fit_<fmt>_us            step_fit - step_ready per window: the fit launch up to the start of the network
  stretch_<fmt>_us        step_stretch - step_ready per window: the stage it replaces, the yardstick
  unfit_us                cf_unfit_rows (device form) alone, behind a threshold decode with max_out = 64
  decode_us               that threshold decode alone, for scale
The bytes are computed from the shapes: the canvas written (B x 640 x 640 x 3) and the distinct source bytes the taps touch (the fit reads
about 4 of every 9 source pixels at this 3 x shrink; the stretch at 1.69 x 3 reads nearly all).  The fraction of peak is bytes / time
over 8 TB/s.  A kernel-level cross-check is a `rocprofv3 --kernel-trace --stats` run of `fit_probe.py --short` (kernels:
fit_frames_kernel, yuv_bgr_resize_kernel, resize_u8_kernel, unfit_rows_kernel).  One JSON line."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa
from centerface_amd import ops

short = "--short" in sys.argv
B, h, w, S, MAXF, REP, WIN = 16, 1080, 1920, 640, 64, 20, 7
PEAK = 8e12
rng = np.random.default_rng(0)
eng = cfa.Engine(S, S, max_batch=B, dtype="bf16", decode_stream=False)
L, P = cfa._lib.lib(), cfa._lib.ptr
rw, rh, dx, dy = ops.fit_geometry(h, w, S, S)


def coarse(shape):
    """frames of coarse noise (8-pixel blocks): detail that survives a resize"""
    small = rng.integers(0, 256, (shape[0], shape[1] // 8 + 1, shape[2] // 8 + 1) + shape[3:], dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(small, 8, 1), 8, 2)[:, :shape[1], :shape[2]])


def on_device(a):
    d = eng.device_alloc(a.nbytes)
    eng.memcpy_h2d(d, a)
    return d


def taps(src, dst):
    """the distinct source indices the bilinear taps of a src -> dst resize touch (cf_cvresize.h: floor((d + 0.5) * src / dst - 0.5) and its
    neighbour, clamped)"""
    s = np.floor((np.arange(dst) + 0.5) * (src / dst) - 0.5).astype(np.int64)
    return np.unique(np.clip(np.concatenate([s, s + 1]), 0, src - 1))


def source_bytes(fmt, dh, dw):
    ys, xs = taps(h, dh), taps(w, dw)
    if fmt == "bgr":
        return len(ys) * len(xs) * 3
    return len(ys) * len(xs) + len(np.unique(ys >> 1)) * len(np.unique(xs >> 1)) * 2


nv12 = coarse((B, h * 3 // 2, w))
bgr = coarse((B, h, w, 3))
d_nv12, d_bgr = on_device(nv12), on_device(bgr)
one = h * w * 3 // 2
planes = {"nv12": [(d_nv12 + b * one, d_nv12 + b * one + h * w) for b in range(B)], "bgr": [(d_bgr + b * h * w * 3,) for b in range(B)]}
eng.forward_fit_enqueue(planes["bgr"], "bgr", on_device=True, h=h, w=w)
ready = eng.resized_input()
d_ready = on_device(ready)
d_out = [eng.device_alloc(B * MAXF * 5 * 4), eng.device_alloc(B * MAXF * 10 * 4), eng.device_alloc(B * 4), eng.device_alloc(B * 4)]


def step_fit(fmt):
    eng.forward_fit_enqueue(planes[fmt], fmt, on_device=True, h=h, w=w)


def step_stretch(fmt):
    if fmt == "nv12":
        eng.forward_yuv_enqueue(planes["nv12"], "nv12", on_device=True, h=h, w=w)
    else:
        eng._chk(L.cf_forward_resized(eng._h, d_bgr, 1, B, h, w))
        eng.last_B = B


def step_ready():
    eng.forward_enqueue(d_ready, on_device=True, B=B, in_format=cfa._lib.CF_IN_U8_HWC_BGR)


def decode_counts(thr):
    dets, lms, counts = np.zeros((B, MAXF, 5), np.float32), np.zeros((B, MAXF, 10), np.float32), np.zeros(B, np.int32)
    eng._chk(L.cf_decode_threshold(eng._h, thr, 0.3, MAXF, P(dets), P(lms), P(counts)))
    return counts


steps = {"step_fit_nv12_ms": lambda: step_fit("nv12"), "step_stretch_nv12_ms": lambda: step_stretch("nv12"),
         "step_fit_bgr_ms": lambda: step_fit("bgr"), "step_stretch_bgr_ms": lambda: step_stretch("bgr"), "step_ready_ms": step_ready}
for _ in range(3):                                                              # warm-up: graph capture, code objects, workspaces
    for fn in steps.values():
        fn()
eng.synchronize()
step_fit("nv12")
for thr in (0.3, 0.1, 0.03, 0.01, 0.001):
    counts = decode_counts(thr)
    if int(counts.min()) >= 8:
        break
eng.unfit_rows_device(MAXF, *d_out)
mapped = np.zeros(B, np.int32)
eng.synchronize()
eng.memcpy_d2h(mapped, d_out[2])
canvas_bytes = B * S * S * 3
out = {"shape": "%d x %dx%d frames (NV12 and BGR) on the device, engine %dx%d bf16, content %dx%d at (%d, %d), decode max_out %d" % (B, h, w, S, S, rw, rh, dx, dy, MAXF),
       "score_thresh": thr, "rows_per_image_min_max": [int(np.minimum(counts, MAXF).min()), int(np.minimum(counts, MAXF).max())],
       "mapped_per_image_min_max": [int(mapped.min()), int(mapped.max())], "canvas_MB": round(canvas_bytes / 1e6, 2),
       "read_MB": {"fit_nv12": round(B * source_bytes("nv12", rh, rw) / 1e6, 2), "fit_bgr": round(B * source_bytes("bgr", rh, rw) / 1e6, 2),
                   "stretch_nv12": round(B * source_bytes("nv12", S, S) / 1e6, 2), "stretch_bgr": round(B * source_bytes("bgr", S, S) / 1e6, 2)}}


def timed(fn):
    eng.event_record(0)
    for _ in range(REP):
        fn()
    eng.event_record(1)
    eng.synchronize()
    return eng.event_elapsed_ms(0, 1) / REP


if not short:
    ms = {k: [] for k in steps}
    for _ in range(WIN):
        for k, fn in steps.items():
            eng.synchronize()
            ms[k].append(timed(fn))
    for k, v in ms.items():
        out[k] = round(float(np.median(v)), 4)
        out[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    for fmt in ("nv12", "bgr"):
        for kind in ("fit", "stretch"):
            us = [(a - b) * 1e3 for a, b in zip(ms["step_%s_%s_ms" % (kind, fmt)], ms["step_ready_ms"])]
            name = "%s_%s_us" % (kind, fmt)
            out[name] = round(float(np.median(us)), 2)
            out[name + "_min_max"] = [round(min(us), 2), round(max(us), 2)]
            moved = canvas_bytes + out["read_MB"]["%s_%s" % (kind, fmt)] * 1e6
            out["%s_%s_fraction_of_8TBps" % (kind, fmt)] = round(moved / (out[name] * 1e-6) / PEAK, 4) if out[name] > 0 else None
    step_fit("nv12")
    decode_counts(thr)
    for name, fn in (("unfit_us", lambda: eng.unfit_rows_device(MAXF, *d_out)), ("decode_us", lambda: eng.decode_threshold_enqueue(thr, 0.3, MAXF))):
        us = [timed(fn) * 1e3 for _ in range(WIN)]
        out[name] = round(float(np.median(us)), 2)
        out[name + "_min_max"] = [round(min(us), 2), round(max(us), 2)]
eng.synchronize()
for p in [d_nv12, d_bgr, d_ready] + d_out:
    eng.device_free(p)
eng.close()
print(json.dumps(out))
