#!/usr/bin/env python3
"""The views cutter and cf_merge_views beside the two existing stages their numbers are to be read against: 16 NV12 and 16 BGR frames of
1080 x 1920, resident on the device, behind a 640 x 640 bf16 engine that reads them in place.  The layout is the header's worked example:
tile 640, overlap 128, levels 1.0 and 0.5 -- 8 tiles, 640 x 360 at y = 140, 320 x 180 at (160, 230), V = 10, 160 canvases a call.

What is timed, after warming up every launch involved, with HIP events on the engine's main stream around REP back-to-back calls (median
and spread of WIN windows; the steps alternate window by window).  An input stage is the step with it minus the network alone at the same
batch, per window:
  views_<fmt>_us      cf_forward_views (the V = 10 layout) - cf_forward of 160 ready canvases: the views cutter
  tiles_<fmt>_us      cf_forward_tiles on the eight tile rectangles alone - cf_forward of 128 ready canvases: the tile cutter
  fit_<fmt>_us        cf_forward_fit - cf_forward of 16 ready canvases: the fit stage
  merge_views_us      cf_merge_views (device form) alone, behind a threshold decode with max_out = 64
  merge_tiles_us      cf_merge_tiles (device form) alone, behind the same decode of the eight-tile forward
  decode_us           that threshold decode of the 160 canvases alone, for scale
The network at batch 160 takes milliseconds and the cutters tens of microseconds, so the spread of the differences is printed beside
every median: read the two together.  No threshold is set here.  A kernel-level cross-check is a kernel-trace run of
`view_probe.py --short` (kernels: cut_views_kernel, cut_tiles_kernel, fit_frames_kernel, collect_rows_kernel).
One JSON line; `--md` prints the table of profiles/views.md instead."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa
from centerface_amd import ops

short, as_md = "--short" in sys.argv, "--md" in sys.argv
B, h, w, S, MAXF, REP, WIN = 16, 1080, 1920, 640, 64, 4, 7
views = ops.view_layout(h, w, S, S, tile=S, overlap=128, scales=(1.0, 0.5))
rects = ops.tile_grid(h, w, S, 128, with_full=False)
V, T = len(views), len(rects)
assert (V, T) == (10, 8) and views[:8, :4].tolist() == rects.tolist()
rng = np.random.default_rng(0)
eng = cfa.Engine(S, S, max_batch=B * V, dtype="bf16", decode_stream=False)


def coarse(shape):
    """frames of coarse noise (8-pixel blocks): detail that survives a resize"""
    small = rng.integers(0, 256, (shape[0], shape[1] // 8 + 1, shape[2] // 8 + 1) + shape[3:], dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(small, 8, 1), 8, 2)[:, :shape[1], :shape[2]])


def on_device(a):
    d = eng.device_alloc(a.nbytes)
    eng.memcpy_h2d(d, a)
    return d


nv12, bgr = coarse((B, h * 3 // 2, w)), coarse((B, h, w, 3))
d_nv12, d_bgr = on_device(nv12), on_device(bgr)
one = h * w * 3 // 2
planes = {"nv12": [(d_nv12 + b * one, d_nv12 + b * one + h * w) for b in range(B)], "bgr": [(d_bgr + b * h * w * 3,) for b in range(B)]}
eng.forward_views_enqueue(planes["bgr"], views, "bgr", on_device=True, h=h, w=w)
d_ready = on_device(eng.resized_input())                 # 160 ready canvases; the first 128 and the first 16 serve the smaller batches
d_out = [eng.device_alloc(B * MAXF * 5 * 4), eng.device_alloc(B * MAXF * 10 * 4), eng.device_alloc(B * 4), eng.device_alloc(B * 4)]

steps = {}
for fmt in ("nv12", "bgr"):
    steps["step_views_%s" % fmt] = lambda fmt=fmt: eng.forward_views_enqueue(planes[fmt], views, fmt, on_device=True, h=h, w=w)
    steps["step_tiles_%s" % fmt] = lambda fmt=fmt: eng.forward_tiles_enqueue(planes[fmt], rects, fmt, on_device=True, h=h, w=w)
    steps["step_fit_%s" % fmt] = lambda fmt=fmt: eng.forward_fit_enqueue(planes[fmt], fmt, on_device=True, h=h, w=w)
for name, n in (("views", B * V), ("tiles", B * T), ("fit", B)):
    steps["step_ready_%s" % name] = lambda n=n: eng.forward_enqueue(d_ready, on_device=True, B=n, in_format=cfa._lib.CF_IN_U8_HWC_BGR)
for _ in range(3):                                       # warm-up: graph capture, code objects, workspaces
    for fn in steps.values():
        fn()
eng.synchronize()


def decoded(forward):
    """the forward, then a threshold decode at the first score at which every canvas keeps a few rows"""
    for thr in (0.3, 0.1, 0.03, 0.01, 0.001):
        forward()
        per = eng.decode_threshold(thr, 0.3, MAXF)
        if min(len(d) for d, _ in per) >= 4:
            break
    return thr, [len(d) for d, _ in per]


def timed(fn):
    eng.event_record(0)
    for _ in range(REP):
        fn()
    eng.event_record(1)
    eng.synchronize()
    return eng.event_elapsed_ms(0, 1) / REP


thr, kept = decoded(steps["step_views_nv12"])
eng.merge_views_device(MAXF, *d_out)
merged = np.zeros(B, np.int32)
eng.synchronize()
eng.memcpy_d2h(merged, d_out[2])
out = {"shape": "%d x %dx%d frames (NV12 and BGR) on the device, engine %dx%d bf16, V = %d views (T = %d tiles + levels 1.0, 0.5), decode max_out %d"
                % (B, h, w, S, S, V, T, MAXF),
       "score_thresh": thr, "rows_per_canvas_min_max": [min(kept), max(kept)], "merged_per_frame_min_max": [int(merged.min()), int(merged.max())],
       "canvas_MB": {"views": round(B * V * S * S * 3 / 1e6, 1), "tiles": round(B * T * S * S * 3 / 1e6, 1), "fit": round(B * S * S * 3 / 1e6, 1)}}
if not short:
    ms = {k: [] for k in steps}
    for _ in range(WIN):
        for k, fn in steps.items():
            eng.synchronize()
            ms[k].append(timed(fn))
    for k, v in ms.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
    for fmt in ("nv12", "bgr"):
        for kind in ("views", "tiles", "fit"):
            us = [(a - b) * 1e3 for a, b in zip(ms["step_%s_%s" % (kind, fmt)], ms["step_ready_%s" % kind])]
            out["%s_%s_us" % (kind, fmt)] = round(float(np.median(us)), 1)
            out["%s_%s_us_min_max" % (kind, fmt)] = [round(min(us), 1), round(max(us), 1)]
    rows = {}
    decoded(steps["step_views_nv12"])
    rows["merge_views_us"] = lambda: eng.merge_views_device(MAXF, *d_out)
    rows["decode_us"] = lambda: eng.decode_threshold_enqueue(thr, 0.3, MAXF)
    for name, fn in rows.items():
        us = [timed(fn) * 1e3 for _ in range(WIN)]
        out[name], out[name + "_min_max"] = round(float(np.median(us)), 1), [round(min(us), 1), round(max(us), 1)]
    steps["step_tiles_nv12"]()
    eng.decode_threshold(thr, 0.3, MAXF)
    us = [timed(lambda: eng.merge_tiles_device(MAXF, *d_out)) * 1e3 for _ in range(WIN)]
    out["merge_tiles_us"], out["merge_tiles_us_min_max"] = round(float(np.median(us)), 1), [round(min(us), 1), round(max(us), 1)]
eng.synchronize()
for p in [d_nv12, d_bgr, d_ready] + d_out:
    eng.device_free(p)
eng.close()
if as_md and not short:
    print("| stage | NV12 us (min .. max) | BGR us (min .. max) |\n|---|---|---|")
    for kind, what in (("views", "views cutter, V = 10 (160 canvases)"), ("tiles", "tile cutter, the 8 tile rectangles alone (128 canvases)"),
                       ("fit", "fit stage alone (16 canvases)")):
        print("| %s | %s | %s |" % (what, *("%.1f (%.1f .. %.1f)" % ((out["%s_%s_us" % (kind, f)],) + tuple(out["%s_%s_us_min_max" % (kind, f)])) for f in ("nv12", "bgr"))))
    print("\n| call | us (min .. max) |\n|---|---|")
    for k in ("merge_views_us", "merge_tiles_us", "decode_us"):
        print("| %s | %.1f (%.1f .. %.1f) |" % ((k[:-3], out[k]) + tuple(out[k + "_min_max"])))
print(json.dumps(out))
