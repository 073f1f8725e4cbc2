#!/usr/bin/env python3
"""The input stage of rotated sources against the unrotated fit: 16 NV12 and 16 BGR frames of 1080 x 1920, resident on the device,
behind a 640 x 640 bf16 engine that reads them in place.

What is timed, after warming up every launch involved, with HIP events on the engine's main stream around REP back-to-back calls
(median and spread of WIN windows; the steps alternate window by window):
  step_rot<R>_<fmt>_ms        cf_forward_rot with rot = R (0, 90, 180, 270) and the default fit + the network.  rot 0 launches the fit
                              kernel of the parent commit (fit_frames_kernel): the yardstick, re-measured in the same run
  step_rot90_stretch_<fmt>_ms cf_forward_rot with rot = 90, the upright view stretched to 640 x 640 + the network
  step_ready_ms               cf_forward of a ready-made 640 x 640 uint8 batch on the device: the network alone
  rot<R>_<fmt>_us ...         step - step_ready per window: the input launch up to the start of the network
  ratio_90_to_0_<fmt>         rot90_<fmt>_us / rot0_<fmt>_us (medians)
  unfit_rot<R>_us             cf_unfit_rows (device form) alone behind a rot = R forward and a threshold decode with max_out = 64
A kernel-level cross-check is a `rocprofv3 --kernel-trace --stats` run of `rot_probe.py --short` (kernels: fit_frames_kernel,
fit_frames_kernel, rot_quarter_kernel, unfit_rows_kernel).  One JSON line."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa
from centerface_amd import ops

short = "--short" in sys.argv
B, h, w, S, MAXF, REP, WIN = 16, 1080, 1920, 640, 64, 20, 7
ROTS = (0, 90, 180, 270)
rng = np.random.default_rng(0)
eng = cfa.Engine(S, S, max_batch=B, dtype="bf16", decode_stream=False)
L, P = cfa._lib.lib(), cfa._lib.ptr


def coarse(shape):
    """frames of coarse noise (8-pixel blocks): detail that survives a resize"""
    small = rng.integers(0, 256, (shape[0], shape[1] // 8 + 1, shape[2] // 8 + 1) + shape[3:], dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(small, 8, 1), 8, 2)[:, :shape[1], :shape[2]])


def on_device(a):
    d = eng.device_alloc(a.nbytes)
    eng.memcpy_h2d(d, a)
    return d


nv12 = coarse((B, h * 3 // 2, w))
bgr = coarse((B, h, w, 3))
d_nv12, d_bgr = on_device(nv12), on_device(bgr)
one = h * w * 3 // 2
planes = {"nv12": [(d_nv12 + b * one, d_nv12 + b * one + h * w) for b in range(B)], "bgr": [(d_bgr + b * h * w * 3,) for b in range(B)]}


def step_rot(fmt, rot, fit=True):
    eng.forward_rot_enqueue(planes[fmt], fmt, rot, fit=fit, on_device=True, h=h, w=w)


step_rot("bgr", 0)
d_ready = on_device(eng.resized_input())
d_out = [eng.device_alloc(B * MAXF * 5 * 4), eng.device_alloc(B * MAXF * 10 * 4), eng.device_alloc(B * 4), eng.device_alloc(B * 4)]


def step_ready():
    eng.forward_enqueue(d_ready, on_device=True, B=B, in_format=cfa._lib.CF_IN_U8_HWC_BGR)


def decode_counts(thr):
    dets, lms, counts = np.zeros((B, MAXF, 5), np.float32), np.zeros((B, MAXF, 10), np.float32), np.zeros(B, np.int32)
    eng._chk(L.cf_decode_threshold(eng._h, thr, 0.3, MAXF, P(dets), P(lms), P(counts)))
    return counts


steps = {"step_ready_ms": step_ready}
for fmt in ("nv12", "bgr"):
    for rot in ROTS:
        steps["step_rot%d_%s_ms" % (rot, fmt)] = lambda fmt=fmt, rot=rot: step_rot(fmt, rot)
    steps["step_rot90_stretch_%s_ms" % fmt] = lambda fmt=fmt: step_rot(fmt, 90, None)
for _ in range(3):                                                              # warm-up: graph capture, code objects, workspaces
    for fn in steps.values():
        fn()
eng.synchronize()
out = {"shape": "%d x %dx%d stored frames (NV12 and BGR) on the device, engine %dx%d bf16, decode max_out %d" % (B, h, w, S, S, MAXF),
       "geometry": {str(r): list(ops.rot_geometry(h, w, S, S, r, True)) for r in ROTS}}


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
    for k in steps:
        if k != "step_ready_ms":
            us = [(a - b) * 1e3 for a, b in zip(ms[k], ms["step_ready_ms"])]
            name = k[len("step_"):-len("_ms")] + "_us"
            out[name] = round(float(np.median(us)), 2)
            out[name + "_min_max"] = [round(min(us), 2), round(max(us), 2)]
    for fmt in ("nv12", "bgr"):
        out["ratio_90_to_0_" + fmt] = round(out["rot90_%s_us" % fmt] / out["rot0_%s_us" % fmt], 3) if out["rot0_%s_us" % fmt] > 0 else None
for rot in ROTS:
    step_rot("nv12", rot)
    for thr in (0.3, 0.1, 0.03, 0.01, 0.001):
        counts = decode_counts(thr)
        if int(counts.min()) >= 8:
            break
    eng.unfit_rows_device(MAXF, *d_out)
    mapped = np.zeros(B, np.int32)
    eng.synchronize()
    eng.memcpy_d2h(mapped, d_out[2])
    out["unfit_rot%d_rows" % rot] = {"score_thresh": thr, "decoded_min_max": [int(np.minimum(counts, MAXF).min()), int(np.minimum(counts, MAXF).max())],
                                     "mapped_min_max": [int(mapped.min()), int(mapped.max())]}
    if not short:
        us = [timed(lambda: eng.unfit_rows_device(MAXF, *d_out)) * 1e3 for _ in range(WIN)]
        out["unfit_rot%d_us" % rot] = round(float(np.median(us)), 2)
        out["unfit_rot%d_us_min_max" % rot] = [round(min(us), 2), round(max(us), 2)]
eng.synchronize()
for p in [d_nv12, d_bgr, d_ready] + d_out:
    eng.device_free(p)
eng.close()
print(json.dumps(out))
