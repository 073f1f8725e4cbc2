#!/usr/bin/env python3
"""The follow beside the forward + threshold decode it replaces on the frames between two detections: B = 16 NV12 frames of 1080 x 1920
on the device (16 streams), a 544 x 960 bf16 engine, a threshold decode with max_out = 8 at a score threshold lowered until every image
has its 8 rows, one tracker of 16 streams x 64 slots.  The faces are the rows the synthetic weights give -- their sides in frame pixels
are reported (face_side_px), the cost of the follow grows with them (c * c pixels per cell) -- so the 8 x 16 faces are whatever size the
decode says, not a chosen one.

The tracker is updated once with those rows and followed once (every slot learns); after that a follow of the same frames finds every
face where it is and changes nothing, so the timed steady state can repeat.  Three kinds of window alternate on the engine's main stream,
each fenced by the engine's events and a synchronize, after warming up every launch involved:
  detect_us   5 x (cf_forward_yuv on the device planes + cf_decode_threshold_enqueue), divided by 5
  forward_us  5 x cf_forward_yuv alone, divided by 5 (how much of detect_us is the network: the decode of noise frames sees many cells)
  follow_us   5 x cf_track_follow in the device form (nothing read on the host), divided by 5
median and spread of 7 windows of each kind, taken alternately; follow_share = follow_us / detect_us, from this one run.  One JSON
line.  --short: a few calls only, for a rocprofv3 --kernel-trace --stats run of its own (kernels: follow_kernel, follow_emit_kernel)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa

short = "--short" in sys.argv
B, H, W, FH, FW, MAXF, REP, WIN = 16, 544, 960, 1080, 1920, 8, 5, 7
rng = np.random.default_rng(0)
eng = cfa.Engine(H, W, max_batch=B, dtype="bf16", decode_stream=False)
L, P = cfa._lib.lib(), cfa._lib.ptr
small = rng.integers(0, 256, (B, FH * 3 // 2 // 8 + 1, FW // 8), dtype=np.uint8)  # coarse noise: 8-pixel blocks
frames = np.ascontiguousarray(np.repeat(np.repeat(small, 8, 1), 8, 2)[:, :FH * 3 // 2])
one = FH * 3 // 2 * FW
d_frames = eng.device_alloc(B * one)
eng.memcpy_h2d(d_frames, frames)
planes = [(d_frames + b * one, d_frames + b * one + FH * FW, None) for b in range(B)]


def detect(thr):
    eng.forward_yuv_enqueue(planes, "nv12", on_device=True, h=FH, w=FW)
    eng.decode_threshold_enqueue(thr, 0.3, MAXF)


for thr in (0.3, 0.1, 0.03, 0.01, 0.001):
    eng.forward_yuv_enqueue(planes, "nv12", on_device=True, h=FH, w=FW)
    dets, lms, counts = np.zeros((B, MAXF, 5), np.float32), np.zeros((B, MAXF, 10), np.float32), np.zeros(B, np.int32)
    eng._chk(L.cf_decode_threshold(eng._h, thr, 0.3, MAXF, P(dets), P(lms), P(counts)))
    if int(np.minimum(counts, MAXF).min()) == MAXF:
        break
trk = cfa.Tracker(eng, B, min_hits=1, max_tracks=64)
eng.track_update_device(trk, 0)
fdets, _, _, fcounts, fmoves = eng.track_follow(frames, "nv12", trk)               # host form once: every slot learns; the rows tell the sizes
side = np.concatenate([np.maximum((fdets[b, :fcounts[b], 2] - fdets[b, :fcounts[b], 0]) * (FW / W), (fdets[b, :fcounts[b], 3] - fdets[b, :fcounts[b], 1]) * (FH / H))
                       for b in range(B)])
d_moves = eng.device_alloc(B * 64 * 4 * 4)


def follow():
    eng.track_follow_device(planes, "nv12", B, FH, FW, FW, FW, trk, 0, moves_ptr=d_moves)


for _ in range(3):                                                              # warm-up: code objects, graphs, the context's rows
    detect(thr)
    follow()
eng.synchronize()
moves = np.zeros((B, 64, 4), np.int32)
eng.memcpy_d2h(moves, d_moves)
codes = np.concatenate([moves[b, :fcounts[b], 3] for b in range(B)])
out = {"shape": "%d NV12 frames %dx%d on the device, engine %dx%d bf16, decode max_out %d, tracker %d streams x 64 slots, search 4" % (B, FH, FW, H, W, MAXF, B),
       "score_thresh": thr, "faces_per_frame": [int(c) for c in fcounts], "face_side_px": {"min": round(float(side.min()), 1), "median": round(float(np.median(side)), 1),
                                                                                          "max": round(float(side.max()), 1)} if len(side) else None,
       "codes": {str(k): int((codes == k).sum()) for k in range(4)}}
if not short:
    us = {"detect": [], "forward": [], "follow": []}
    for _ in range(WIN):
        for name, call in (("detect", lambda: detect(thr)), ("forward", lambda: eng.forward_yuv_enqueue(planes, "nv12", on_device=True, h=FH, w=FW)), ("follow", follow)):
            eng.event_record(0)
            for _ in range(REP):
                call()
            eng.event_record(1)
            eng.synchronize()
            us[name].append(eng.event_elapsed_ms(0, 1) * 1e3 / REP)
    for name, v in us.items():
        out["%s_us" % name] = round(float(np.median(v)), 2)
        out["%s_us_min_max" % name] = [round(min(v), 2), round(max(v), 2)]
    out["follow_share"] = round(out["follow_us"] / out["detect_us"], 4)
    out["follow_share_of_forward"] = round(out["follow_us"] / out["forward_us"], 4)
eng.synchronize()
eng.device_free(d_moves)
eng.device_free(d_frames)
trk.close()
eng.close()
print(json.dumps(out))
