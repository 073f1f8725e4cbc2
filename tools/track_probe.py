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
run of its own (kernel: track_update_kernel).

--weak: the tracker with two thresholds (cf_track_create_weak) beside the plain one, in the same run and the same alternation.  Two
more kinds of window on the SAME rows -- a weak tracker whose birth_score is the decode's threshold, so every row is strong and the
second pass finds nothing to do:
  decode_update_weak_us         10 x (the same decode + cf_track_update of the weak tracker)
and three on a LARGER row count, a decode at a threshold lowered further until every image has 60 rows (max_out = 60):
  decode60_us, decode60_update_us (a plain tracker: every row associates and is born), decode60_update_weak_us (birth_score = the
  median over the images of the 21st row's score, so about 20 rows per image are strong and 40 weak: the weak rows only look for a
  confirmed track, find none -- a weak row is never born -- and are discarded in every update)
update_*_us are the differences to the decode of the same rows.

--motion: the tracker with constant-velocity prediction (cf_track_create_ex) beside the plain one, in the same run and the same
alternation, on the SAME 20 rows:
  decode_update_motion_us       10 x (the same decode + cf_track_update of a motion tracker, gain 0.5, damp 1.0)
update_motion_us is the difference to decode_us, to be read beside update_us of this run.  The faces stand still, so every velocity is 0
and every row matches its predicted box at IoU 1: what is timed is the motion instance's extra loads and stores (vel, the stored box of a
winner), not a different association.  No threshold is attached to the figure."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa

short, weak, motion = "--short" in sys.argv, "--weak" in sys.argv, "--motion" in sys.argv
B, H, W, MAXF, MAXW, REP, WIN = 16, 544, 960, 20, 60, 10, 7
rng = np.random.default_rng(0)
eng = cfa.Engine(H, W, max_batch=B, dtype="bf16", decode_stream=False)
L, P = cfa._lib.lib(), cfa._lib.ptr
small = rng.integers(0, 256, (B, H // 8, W // 8, 3), dtype=np.uint8)             # coarse noise: 8-pixel blocks
eng.forward_enqueue(np.ascontiguousarray(np.repeat(np.repeat(small, 8, 1), 8, 2)))


def lowered(ladder, max_out):
    """The first threshold of ``ladder`` at which every image has ``max_out`` rows (else the last): (threshold, scores [B, max_out], counts)."""
    for t in ladder:
        dets, lms, counts = np.zeros((B, max_out, 5), np.float32), np.zeros((B, max_out, 10), np.float32), np.zeros(B, np.int32)
        eng._chk(L.cf_decode_threshold(eng._h, t, 0.3, max_out, P(dets), P(lms), P(counts)))
        if int(np.minimum(counts, max_out).min()) == max_out:
            break
    return t, dets[:, :, 4], counts


thr, _, counts = lowered((0.3, 0.1, 0.03, 0.01, 0.001), MAXF)
trk = cfa.Tracker(eng, B, max_tracks=256)
d_counts = eng.device_alloc(4 * B)


def decode():
    eng.decode_threshold_enqueue(thr, 0.3, MAXF)


def decode_update():
    eng.decode_threshold_enqueue(thr, 0.3, MAXF)
    eng.track_update_device(trk, 0, counts_ptr=d_counts)


calls = [("decode", decode), ("decode_update", decode_update)]
out = {"shape": "%d images %dx%d bf16, decode max_out %d, tracker %d streams x 256 slots" % (B, H, W, MAXF, B), "score_thresh": thr}
trackers = [trk]
if weak:
    thr_w, scores_w, counts_w = lowered([thr * f for f in (0.5, 0.25, 0.1, 0.03, 0.01, 0.001)], MAXW)
    n_w = np.minimum(counts_w, MAXW)
    # max_out keeps the best rows, so all 60 may well lie above the first threshold: birth_score for them is the median over the images
    # of the 21st row's score -- about 20 strong and 40 weak rows per image
    birth60 = max(float(np.median(scores_w[:, MAXF])), float(np.nextafter(np.float32(thr_w), np.float32(1))))
    strong = [int((scores_w[b, :n_w[b]] > np.float32(birth60)).sum()) for b in range(B)]
    same, plain60, weak60 = (cfa.Tracker(eng, B, max_tracks=256, weak_score=thr_w, birth_score=thr), cfa.Tracker(eng, B, max_tracks=256),
                             cfa.Tracker(eng, B, max_tracks=256, weak_score=thr_w, birth_score=birth60))
    trackers += [same, plain60, weak60]

    def update_of(t, score, max_out):
        def call():
            eng.decode_threshold_enqueue(score, 0.3, max_out)
            eng.track_update_device(t, 0, counts_ptr=d_counts)
        return call

    calls += [("decode_update_weak", update_of(same, thr, MAXF)), ("decode60", lambda: eng.decode_threshold_enqueue(thr_w, 0.3, MAXW)),
              ("decode60_update", update_of(plain60, thr_w, MAXW)), ("decode60_update_weak", update_of(weak60, thr_w, MAXW))]
    out.update(weak_score_thresh=thr_w, birth_score60=birth60, rows60_per_image=[int(c) for c in n_w], strong_rows60_per_image=strong)

if motion:
    moving = cfa.Tracker(eng, B, max_tracks=256, motion=True)
    trackers.append(moving)

    def decode_update_motion():
        eng.decode_threshold_enqueue(thr, 0.3, MAXF)
        eng.track_update_device(moving, 0, counts_ptr=d_counts)

    calls.append(("decode_update_motion", decode_update_motion))
    out.update(motion=moving.motion)

for _ in range(3):                                                              # warm-up: code objects, the context's tracked rows
    for _, call in calls:
        call()
eng.synchronize()
decode_update()
eng.synchronize()
tracked = np.zeros(B, np.int32)
eng.memcpy_d2h(tracked, d_counts)
out.update(rows_per_image=[int(c) for c in np.minimum(counts, MAXF)], tracked_per_stream=tracked.tolist())
if not short:
    us = {name: [] for name, _ in calls}
    for _ in range(WIN):
        for name, call in calls:
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
    if weak:
        out["update_weak_us"] = round(out["decode_update_weak_us"] - out["decode_us"], 2)
        out["update60_us"] = round(out["decode60_update_us"] - out["decode60_us"], 2)
        out["update60_weak_us"] = round(out["decode60_update_weak_us"] - out["decode60_us"], 2)
    if motion:
        out["update_motion_us"] = round(out["decode_update_motion_us"] - out["decode_us"], 2)
eng.synchronize()
eng.device_free(d_counts)
for t in trackers:
    t.close()
eng.close()
print(json.dumps(out))
