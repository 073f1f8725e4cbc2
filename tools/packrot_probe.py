#!/usr/bin/env python3
"""The rotated packed cutter beside the unrotated one of the same run: 16 NV12 and 16 BGR frames STORED as 1080 x 1920, resident on the
device, behind a 640 x 640 bf16 engine that reads them in place, levels (1.0, 0.5, 0.25) packed with gutter 0.  At rot 0 and 180 the
upright view is 1080 x 1920 (the 640 x 360 full level and, in the strip below it, half and quarter levels); at rot 90 and 270 it is
1920 x 1080 (the 360 x 640 full level and, beside it, half and quarter levels).  Either way 16 canvases a call.

What is timed, after warming up every launch involved, with HIP events on the engine's main stream around REP back-to-back calls (median
and spread of WIN windows; the steps alternate window by window):
  cut_rot<R>_<fmt>_us    cf_forward_packed_rot(R) - cf_forward of 16 ready canvases, per window: the packed cutter writing 16 canvases
                         (R = 0 is cf_forward_packed's own launch: the yardstick, which this code does not touch)
  e2e_rot<R>_<fmt>_ms    the forward + threshold decode (enqueue form, max_out 64) + cf_merge_packed (device form), R = 0 and 90
  ready_16_ms            the network alone, for scale
The network takes milliseconds and the cutters tens of microseconds, so the spread of the differences is printed beside every median:
read the two together.  The single-view quarter turn came out at 1.00 to 1.10 x its unrotated fit (profiles/rot.md); no number is fixed
here for the packed one, and no threshold is set.  One JSON line; `--md` prints the table of profiles/pack_rot.md instead."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa
from centerface_amd import ops

as_md = "--md" in sys.argv
B, h, w, S, MAXF, REP, WIN = 16, 1080, 1920, 640, 64, 4, 7
ROTS = (0, 90, 180, 270)
layout = {}
for rot in ROTS:
    hu, wu = (w, h) if rot in (90, 270) else (h, w)
    layout[rot] = ops.pack_views(ops.view_layout(hu, wu, S, S, scales=(1.0, 0.5, 0.25)), B, (S, S), 0)
    assert layout[rot][1] == B, (rot, layout[rot][1])
N = B
rng = np.random.default_rng(0)
eng = cfa.Engine(S, S, max_batch=N, dtype="bf16", decode_stream=False)


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
eng.forward_packed_enqueue(planes["bgr"], *layout[0], "bgr", on_device=True, h=h, w=w)
d_ready = on_device(eng.resized_input())                 # 16 ready canvases
d_out = [eng.device_alloc(B * MAXF * 5 * 4), eng.device_alloc(B * MAXF * 10 * 4), eng.device_alloc(B * 4), eng.device_alloc(B * 4)]
THR = 0.3


def fwd(fmt, rot):
    eng.forward_packed_enqueue(planes[fmt], *layout[rot], fmt, on_device=True, h=h, w=w, rot=rot)


def e2e(fmt, rot):
    fwd(fmt, rot)
    eng.decode_threshold_enqueue(THR, 0.3, MAXF)
    eng.merge_packed_device(MAXF, *d_out)


steps = {}
for fmt in ("nv12", "bgr"):
    for rot in ROTS:
        steps["fwd_rot%d_%s" % (rot, fmt)] = lambda fmt=fmt, rot=rot: fwd(fmt, rot)
    for rot in (0, 90):
        steps["e2e_rot%d_%s" % (rot, fmt)] = lambda fmt=fmt, rot=rot: e2e(fmt, rot)
steps["ready_%d" % N] = lambda: eng.forward_enqueue(d_ready, on_device=True, B=N, in_format=cfa._lib.CF_IN_U8_HWC_BGR)
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
for rot in (0, 90):
    e2e("nv12", rot)
    got = np.zeros(B, np.int32)
    eng.synchronize()
    eng.memcpy_d2h(got, d_out[2])
    merged["rot%d" % rot] = [int(got.min()), int(got.max())]
out = {"shape": "%d x %dx%d stored frames (NV12 and BGR) on the device, engine %dx%d bf16, levels 1.0 / 0.5 / 0.25 packed into %d canvases, decode max_out %d"
                % (B, h, w, S, S, N, MAXF),
       "score_thresh": THR, "merged_per_frame_min_max": merged}
ms = {k: [] for k in steps}
for _ in range(WIN):
    for k, fn in steps.items():
        eng.synchronize()
        ms[k].append(timed(fn))
for k, v in ms.items():
    out[k + "_ms"] = round(float(np.median(v)), 4)
    out[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
for fmt in ("nv12", "bgr"):
    for rot in ROTS:
        us = [(a - b) * 1e3 for a, b in zip(ms["fwd_rot%d_%s" % (rot, fmt)], ms["ready_%d" % N])]
        out["cut_rot%d_%s_us" % (rot, fmt)] = round(float(np.median(us)), 1)
        out["cut_rot%d_%s_us_min_max" % (rot, fmt)] = [round(min(us), 1), round(max(us), 1)]
eng.synchronize()
for p in [d_nv12, d_bgr, d_ready] + d_out:
    eng.device_free(p)
eng.close()
if as_md:
    print("| stage | NV12 (min .. max) | BGR (min .. max) |\n|---|---|---|")
    rows = [("cut_rot%d_%%s_us" % rot, "packed cutter, rot %d, 16 canvases, us" % rot, "%.1f") for rot in ROTS]
    rows += [("e2e_rot%d_%%s_ms" % rot, "forward + decode + merge, rot %d, 16 canvases, ms" % rot, "%.3f") for rot in (0, 90)]
    for key, what, unit in rows:
        cells = []
        for f in ("nv12", "bgr"):
            k = key % f
            cells.append((unit + " (" + unit + " .. " + unit + ")") % ((out[k],) + tuple(out[k + "_min_max"])))
        print("| %s | %s | %s |" % (what, cells[0], cells[1]))
    print("\n| network alone | ms (min .. max) |\n|---|---|")
    print("| %d ready canvases | %.3f (%.3f .. %.3f) |" % ((N, out["ready_%d_ms" % N]) + tuple(out["ready_%d_ms_min_max" % N])))
print(json.dumps(out))
