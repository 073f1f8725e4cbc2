#!/usr/bin/env python3
"""The scene check beside the follow and the forward + decode it precedes: B = 16 frames of 1080 x 1920 on the device (16 streams), once
as NV12 and once as BGR, a 544 x 960 bf16 engine, a threshold decode with max_out = 8 at a score threshold lowered until every image has
its 8 rows, one tracker of 16 streams x 64 slots, one scene object of 16 streams at the default thresholds.

The tracker is updated once with the decode's rows and followed once (every slot learns); the scene object has seen the frames once.
After that a check of the same frames is SAME on every stream and resets nothing, and a follow finds every face where it is, so the
timed steady state can repeat.  Windows of four kinds alternate on the engine's main stream, each fenced by the engine's events and a
synchronize, after warming up every launch involved:
  check_us    5 x cf_scene_check in the device form with the tracker (nothing read on the host), divided by 5 -- per format
  follow_us   5 x cf_track_follow in the device form on the same frames, divided by 5 -- per format
  forward_us  5 x cf_forward_yuv alone on the NV12 planes, divided by 5
  detect_us   5 x (cf_forward_yuv + cf_decode_threshold_enqueue), divided by 5
median and spread of 7 windows of each kind, taken alternately.  check_gbps = bytes of luma source read (h * w per NV12 frame, 3 * h * w
per BGR frame) over check_us.  One JSON line.  --short: a few calls only, for a rocprofv3 --kernel-trace --stats run of its own (kernels:
scene_sums_kernel, scene_decide_kernel)."""
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
nv12 = np.ascontiguousarray(np.repeat(np.repeat(small, 8, 1), 8, 2)[:, :FH * 3 // 2])
bgr = np.ascontiguousarray(np.repeat(nv12[:, :FH, :, None], 3, axis=3))          # the same luma (29 + 150 + 77 = 256), three bytes per pixel
one = {"nv12": FH * 3 // 2 * FW, "bgr": FH * FW * 3}
dev = {"nv12": eng.device_alloc(B * one["nv12"]), "bgr": eng.device_alloc(B * one["bgr"])}
eng.memcpy_h2d(dev["nv12"], nv12)
eng.memcpy_h2d(dev["bgr"], bgr)
planes = {"nv12": [(dev["nv12"] + b * one["nv12"], dev["nv12"] + b * one["nv12"] + FH * FW, None) for b in range(B)],
          "bgr": [(dev["bgr"] + b * one["bgr"],) for b in range(B)]}
pitch = {"nv12": (FW, FW), "bgr": (3 * FW, 0)}
luma_bytes = {"nv12": B * FH * FW, "bgr": B * FH * FW * 3}


def forward():
    eng.forward_yuv_enqueue(planes["nv12"], "nv12", on_device=True, h=FH, w=FW)


def detect(thr):
    forward()
    eng.decode_threshold_enqueue(thr, 0.3, MAXF)


for thr in (0.3, 0.1, 0.03, 0.01, 0.001):
    forward()
    dets, lms, counts = np.zeros((B, MAXF, 5), np.float32), np.zeros((B, MAXF, 10), np.float32), np.zeros(B, np.int32)
    eng._chk(L.cf_decode_threshold(eng._h, thr, 0.3, MAXF, P(dets), P(lms), P(counts)))
    if int(np.minimum(counts, MAXF).min()) == MAXF:
        break
trk = cfa.Tracker(eng, B, min_hits=1, max_tracks=64)
scn = {f: cfa.SceneCuts(eng, B) for f in ("nv12", "bgr")}
eng.track_update_device(trk, 0)
_, _, _, fcounts, _ = eng.track_follow(nv12, "nv12", trk)                        # host form once: every slot learns
d_out = eng.device_alloc(B * 4 * 4)


def check(f):
    eng.scene_check_device(planes[f], f, B, FH, FW, pitch[f][0], pitch[f][1], scn[f], trk, 0, d_out)


def follow(f):
    eng.track_follow_device(planes[f], f, B, FH, FW, pitch[f][0], pitch[f][1], trk, 0)


codes = {}
for f in ("nv12", "bgr"):
    for _ in range(3):                                                          # warm-up: code objects, the object's first signature
        check(f)
        follow(f)
    eng.synchronize()
    got = np.zeros((B, 4), np.int32)
    eng.memcpy_d2h(got, d_out)
    codes[f] = {str(k): int((got[:, 0] == k).sum()) for k in range(3)}
for _ in range(3):
    detect(thr)
eng.synchronize()
out = {"shape": "%d frames %dx%d on the device as NV12 and as BGR, engine %dx%d bf16, decode max_out %d, tracker %d streams x 64 slots, scene thresholds 350 / 640"
                % (B, FH, FW, H, W, MAXF, B),
       "score_thresh": thr, "faces_per_frame": [int(c) for c in fcounts], "codes": codes}
if not short:
    kinds = [("check_%s" % f, lambda f=f: check(f)) for f in ("nv12", "bgr")] + [("follow_%s" % f, lambda f=f: follow(f)) for f in ("nv12", "bgr")] + \
            [("forward", forward), ("detect", lambda: detect(thr))]
    us = {name: [] for name, _ in kinds}
    for _ in range(WIN):
        for name, call in kinds:
            eng.event_record(0)
            for _ in range(REP):
                call()
            eng.event_record(1)
            eng.synchronize()
            us[name].append(eng.event_elapsed_ms(0, 1) * 1e3 / REP)
    for name, v in us.items():
        out["%s_us" % name] = round(float(np.median(v)), 2)
        out["%s_us_min_max" % name] = [round(min(v), 2), round(max(v), 2)]
    for f in ("nv12", "bgr"):
        out["check_%s_gbps" % f] = round(luma_bytes[f] / out["check_%s_us" % f] / 1e3, 1)
        out["check_%s_over_follow" % f] = round(out["check_%s_us" % f] / out["follow_%s_us" % f], 4)
        out["check_%s_over_forward" % f] = round(out["check_%s_us" % f] / out["forward_us"], 4)
        out["check_%s_over_detect" % f] = round(out["check_%s_us" % f] / out["detect_us"], 4)
eng.synchronize()
for p in (d_out, dev["nv12"], dev["bgr"]):
    eng.device_free(p)
trk.close()
for s in scn.values():
    s.close()
eng.close()
print(json.dumps(out))
