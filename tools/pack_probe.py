#!/usr/bin/env python3
"""Packed views beside the unpacked path they are to be read against: 16 NV12 and 16 BGR frames of 1080 x 1920, resident on the device,
behind a 640 x 640 bf16 engine that reads them in place, at levels (1.0, 0.5, 0.25).  Unpacked is cf_forward_views: V = 3 views, 48
canvases a call.  Packed is cf_pack_views (gutter 0) + cf_forward_packed: 16 canvases a call, each with the 640 x 360 full level and,
in the strip below it, half and quarter levels.

What is timed, after warming up every launch involved, with HIP events on the engine's main stream around REP back-to-back calls (median
and spread of WIN windows; the steps alternate window by window):
  cut_views_<fmt>_us     cf_forward_views - cf_forward of 48 ready canvases, per window: the views cutter writing 48 canvases
  cut_packed_<fmt>_us    cf_forward_packed - cf_forward of 16 ready canvases, per window: the packed cutter writing 16 canvases
  e2e_views_<fmt>_ms     cf_forward_views + threshold decode (enqueue form, max_out 64) + cf_merge_views (device form)
  e2e_packed_<fmt>_ms    cf_forward_packed + the same decode + cf_merge_packed (device form)
  ready_16_ms, ready_48_ms   the network alone at the two batches, for scale
The network takes milliseconds and the cutters tens of microseconds, so the spread of the differences is printed beside every median:
read the two together.  Expectations to compare against, not asserted: the packed end-to-end time near that of a 16-canvas forward; the
packed cutter no more than the unpacked cutter (it writes a third of the bytes).  No threshold is set here.  One JSON line; `--md`
prints the table of profiles/pack.md instead."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa
from centerface_amd import ops

as_md = "--md" in sys.argv
B, h, w, S, MAXF, REP, WIN = 16, 1080, 1920, 640, 64, 4, 7
views = ops.view_layout(h, w, S, S, scales=(1.0, 0.5, 0.25))
places, N = ops.pack_views(views, B, (S, S), 0)
V = len(views)
assert (V, N) == (3, 16)
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
d_ready = on_device(eng.resized_input())                 # 48 ready canvases; the first 16 serve the smaller batch
d_out = [eng.device_alloc(B * MAXF * 5 * 4), eng.device_alloc(B * MAXF * 10 * 4), eng.device_alloc(B * 4), eng.device_alloc(B * 4)]
THR = 0.3


def fwd_views(fmt):
    eng.forward_views_enqueue(planes[fmt], views, fmt, on_device=True, h=h, w=w)


def fwd_packed(fmt):
    eng.forward_packed_enqueue(planes[fmt], places, N, fmt, on_device=True, h=h, w=w)


def e2e_views(fmt):
    fwd_views(fmt)
    eng.decode_threshold_enqueue(THR, 0.3, MAXF)
    eng.merge_views_device(MAXF, *d_out)


def e2e_packed(fmt):
    fwd_packed(fmt)
    eng.decode_threshold_enqueue(THR, 0.3, MAXF)
    eng.merge_packed_device(MAXF, *d_out)


steps = {}
for fmt in ("nv12", "bgr"):
    steps["fwd_views_%s" % fmt] = lambda fmt=fmt: fwd_views(fmt)
    steps["fwd_packed_%s" % fmt] = lambda fmt=fmt: fwd_packed(fmt)
    steps["e2e_views_%s" % fmt] = lambda fmt=fmt: e2e_views(fmt)
    steps["e2e_packed_%s" % fmt] = lambda fmt=fmt: e2e_packed(fmt)
for n in (N, B * V):
    steps["ready_%d" % n] = lambda n=n: eng.forward_enqueue(d_ready, on_device=True, B=n, in_format=cfa._lib.CF_IN_U8_HWC_BGR)
for _ in range(3):                                       # warm-up: graph capture, code objects, workspaces
    for fn in steps.values():
        fn()
eng.synchronize()


def timed(fn):
    eng.event_record(0)
    for _ in range(REP):
        fn()
    eng.event_record(1)
    eng.synchronize()
    return eng.event_elapsed_ms(0, 1) / REP


merged = {}
for name, fn in (("views", e2e_views), ("packed", e2e_packed)):
    fn("nv12")
    got = np.zeros(B, np.int32)
    eng.synchronize()
    eng.memcpy_d2h(got, d_out[2])
    merged[name] = [int(got.min()), int(got.max())]
out = {"shape": "%d x %dx%d frames (NV12 and BGR) on the device, engine %dx%d bf16, levels 1.0 / 0.5 / 0.25: %d canvases unpacked, %d packed, decode max_out %d"
                % (B, h, w, S, S, B * V, N, MAXF),
       "score_thresh": THR, "merged_per_frame_min_max": merged,
       "canvas_MB": {"views": round(B * V * S * S * 3 / 1e6, 1), "packed": round(N * S * S * 3 / 1e6, 1)}}
ms = {k: [] for k in steps}
for _ in range(WIN):
    for k, fn in steps.items():
        eng.synchronize()
        ms[k].append(timed(fn))
for k, v in ms.items():
    out[k + "_ms"] = round(float(np.median(v)), 4)
    out[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
for fmt in ("nv12", "bgr"):
    for kind, n in (("views", B * V), ("packed", N)):
        us = [(a - b) * 1e3 for a, b in zip(ms["fwd_%s_%s" % (kind, fmt)], ms["ready_%d" % n])]
        out["cut_%s_%s_us" % (kind, fmt)] = round(float(np.median(us)), 1)
        out["cut_%s_%s_us_min_max" % (kind, fmt)] = [round(min(us), 1), round(max(us), 1)]
eng.synchronize()
for p in [d_nv12, d_bgr, d_ready] + d_out:
    eng.device_free(p)
eng.close()
if as_md:
    print("| stage | NV12 (min .. max) | BGR (min .. max) |\n|---|---|---|")
    for key, what, unit in (("cut_views_%s_us", "views cutter, 48 canvases, us", "%.1f"), ("cut_packed_%s_us", "packed cutter, 16 canvases, us", "%.1f"),
                            ("e2e_views_%s_ms", "unpacked forward + decode + merge, 48 canvases, ms", "%.3f"),
                            ("e2e_packed_%s_ms", "packed forward + decode + merge, 16 canvases, ms", "%.3f")):
        cells = []
        for f in ("nv12", "bgr"):
            k = key % f
            cells.append((unit + " (" + unit + " .. " + unit + ")") % ((out[k],) + tuple(out[k + "_min_max"])))
        print("| %s | %s | %s |" % (what, cells[0], cells[1]))
    print("\n| network alone | ms (min .. max) |\n|---|---|")
    for n in (N, B * V):
        print("| %d ready canvases | %.3f (%.3f .. %.3f) |" % ((n, out["ready_%d_ms" % n]) + tuple(out["ready_%d_ms_min_max" % n])))
print(json.dumps(out))
