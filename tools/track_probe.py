#!/usr/bin/env python3
"""The tracker's update beside the threshold decode it follows: B = 16 images (16 streams) behind a 544 x 960 bf16 engine, a threshold
decode with max_out = 20 at a score threshold lowered until every image has its 20 rows (the synthetic weights decide where they are),
one tracker of 16 streams x 256 slots in the device form (cf_track_update, out_on_device = 1: nothing is read on the host).

An update may follow a decode only once, so the update is never timed alone.  Two kinds of window alternate on the engine's main stream,
each fenced by the engine's events and a synchronize, after warming up every launch involved:
  decode_us          10 x cf_decode_threshold_enqueue, divided by 10
  decode_update_us   10 x (cf_decode_threshold_enqueue + cf_track_update), divided by 10
median and spread of 7 windows of each kind, taken alternately; update_us = the difference of the medians, update_share = update_us /
decode_us: the update as a share of the decode it follows, from this one run.  The steady state is what is timed: the same 20 faces per
stream match their tracks at IoU 1 in every update.  One JSON line.  --short: a few calls only, for a rocprofv3 --kernel-trace --stats
run of its own (kernel: track_update_kernel)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa

short = "--short" in sys.argv
B, H, W, MAXF, REP, WIN = 16, 544, 960, 20, 10, 7
rng = np.random.default_rng(0)
eng = cfa.Engine(H, W, max_batch=B, dtype="bf16", decode_stream=False)
L, P = cfa._lib.lib(), cfa._lib.ptr
small = rng.integers(0, 256, (B, H // 8, W // 8, 3), dtype=np.uint8)             # coarse noise: 8-pixel blocks
eng.forward_enqueue(np.ascontiguousarray(np.repeat(np.repeat(small, 8, 1), 8, 2)))
for thr in (0.3, 0.1, 0.03, 0.01, 0.001):
    dets, lms, counts = np.zeros((B, MAXF, 5), np.float32), np.zeros((B, MAXF, 10), np.float32), np.zeros(B, np.int32)
    eng._chk(L.cf_decode_threshold(eng._h, thr, 0.3, MAXF, P(dets), P(lms), P(counts)))
    if int(np.minimum(counts, MAXF).min()) == MAXF:
        break
trk = cfa.Tracker(eng, B, max_tracks=256)
d_counts = eng.device_alloc(4 * B)


def decode():
    eng.decode_threshold_enqueue(thr, 0.3, MAXF)


def decode_update():
    eng.decode_threshold_enqueue(thr, 0.3, MAXF)
    eng.track_update_device(trk, 0, counts_ptr=d_counts)


for _ in range(3):                                                              # warm-up: code objects, the context's tracked rows
    decode()
    decode_update()
eng.synchronize()
tracked = np.zeros(B, np.int32)
eng.memcpy_d2h(tracked, d_counts)
out = {"shape": "%d images %dx%d bf16, decode max_out %d, tracker %d streams x 256 slots" % (B, H, W, MAXF, B), "score_thresh": thr,
       "rows_per_image": [int(c) for c in np.minimum(counts, MAXF)], "tracked_per_stream": tracked.tolist()}
if not short:
    us = {"decode": [], "decode_update": []}
    for _ in range(WIN):
        for name, call in (("decode", decode), ("decode_update", decode_update)):
            eng.event_record(0)
            for _ in range(REP):
                call()
            eng.event_record(1)
            eng.synchronize()
            us[name].append(eng.event_elapsed_ms(0, 1) * 1e3 / REP)
    for name, v in us.items():
        out["%s_us" % name] = round(float(np.median(v)), 2)
        out["%s_us_min_max" % name] = [round(min(v), 2), round(max(v), 2)]
    out["update_us"] = round(out["decode_update_us"] - out["decode_us"], 2)
    out["update_share"] = round(out["update_us"] / out["decode_us"], 3)
eng.synchronize()
eng.device_free(d_counts)
trk.close()
eng.close()
print(json.dumps(out))
