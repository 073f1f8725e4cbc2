#!/usr/bin/env python3
"""One best-shot offer beside the cf_align_faces_frame it follows: B = 16 NV12 frames of 1080 x 1920 on the device (16 streams), a
544 x 960 bf16 engine, a threshold decode with max_out = 8 at a score threshold lowered until every image has its 8 rows, the tracker's
default table (256 slots per stream) and the table's defaults (112 x 112 chips, 320 entries per stream, all three weights).  The faces
are the rows the synthetic weights give on coarse noise, not chosen ones.

The tracker is updated once with those rows (min_hits = 1, so every row is eligible at once); the chips are cut and offered once, which
fills the entries.  After that an offer of the same chips finds every entry alive and -- the earlier frame wins a tie -- copies no
chip, so the steady state the windows time is the score and the decide launches plus a copy launch whose workgroups all leave; the
first offer, which copies every chip, is timed once on its own (first_offer_us, one call).  Two kinds of window alternate on the engine's
main stream, each fenced by the engine's events and a synchronize, after warming up every launch involved:
  align_us   5 x cf_align_faces_frame in the device form (128 chips of 112 x 112), divided by 5
  offer_us   5 x cf_bestshot_offer in the device form (three launches, nothing read on the host), divided by 5
median and spread of 7 windows of each kind, taken alternately, from this one run.  One JSON line.  --short: a few calls only, for a
rocprofv3 --kernel-trace --stats run of its own (kernels: best_score_kernel, best_decide_kernel, best_copy_kernel)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa

short = "--short" in sys.argv
B, H, W, FH, FW, MAXF, REP, WIN, SIZE = 16, 544, 960, 1080, 1920, 8, 5, 7, 112
rng = np.random.default_rng(0)
eng = cfa.Engine(H, W, max_batch=B, dtype="bf16", decode_stream=False)
L, P = cfa._lib.lib(), cfa._lib.ptr
small = rng.integers(0, 256, (B, FH * 3 // 2 // 8 + 1, FW // 8), dtype=np.uint8)  # coarse noise: 8-pixel blocks
frames = np.ascontiguousarray(np.repeat(np.repeat(small, 8, 1), 8, 2)[:, :FH * 3 // 2])
one = FH * 3 // 2 * FW
d_frames = eng.device_alloc(B * one)
eng.memcpy_h2d(d_frames, frames)
planes = [(d_frames + b * one, d_frames + b * one + FH * FW, None) for b in range(B)]
for thr in (0.3, 0.1, 0.03, 0.01, 0.001):
    eng.forward_yuv_enqueue(planes, "nv12", on_device=True, h=FH, w=FW)
    dets, lms, counts = np.zeros((B, MAXF, 5), np.float32), np.zeros((B, MAXF, 10), np.float32), np.zeros(B, np.int32)
    eng._chk(L.cf_decode_threshold(eng._h, thr, 0.3, MAXF, P(dets), P(lms), P(counts)))
    if int(np.minimum(counts, MAXF).min()) == MAXF:
        break
trk = cfa.Tracker(eng, B, min_hits=1)
shots = cfa.BestShots(eng, B, size=SIZE, min_hits=1)
eng.track_update_device(trk, 0)
CAP = B * MAXF
d_chips, d_offs, d_q, d_fl = (eng.device_alloc(n) for n in (CAP * SIZE * SIZE * 3, (B + 1) * 4, CAP * 8, B * 4))


def align():
    eng.align_faces_frame_device(planes, "nv12", B, FH, FW, FW, FW, d_chips, d_offs, CAP, size=SIZE)


def offer():
    eng.bestshot_offer_device(shots, d_chips, d_offs, CAP, B, (FH, FW), 0, d_q, d_fl)


align()
eng.synchronize()
eng.event_record(0)
offer()                                                                          # the first offer: every eligible chip enters and is copied
eng.event_record(1)
eng.synchronize()
first_us = eng.event_elapsed_ms(0, 1) * 1e3
q, fl, offs = np.zeros((CAP,), np.int64), np.zeros((B,), np.int32), np.zeros((B + 1,), np.int32)
eng.memcpy_d2h(q, d_q), eng.memcpy_d2h(fl, d_fl), eng.memcpy_d2h(offs, d_offs)
for _ in range(3):                                                              # warm-up
    align()
    offer()
eng.synchronize()
out = {"shape": "%d NV12 frames %dx%d on the device, engine %dx%d bf16, decode max_out %d, tracker %d streams x 256 slots, table %d entries of %dx%d chips"
                % (B, FH, FW, H, W, MAXF, B, shots.entries, SIZE, SIZE),
       "score_thresh": thr, "chips": int(offs[-1]), "eligible": int((q >= 0).sum()), "overflow_flags": int(fl.sum()),
       "quality": {"min": int(q[q >= 0].min()), "median": int(np.median(q[q >= 0])), "max": int(q[q >= 0].max())} if (q >= 0).any() else None,
       "first_offer_us": round(first_us, 2)}
if not short:
    us = {"align": [], "offer": []}
    for _ in range(WIN):
        for name, call in (("align", align), ("offer", offer)):
            eng.event_record(0)
            for _ in range(REP):
                call()
            eng.event_record(1)
            eng.synchronize()
            us[name].append(eng.event_elapsed_ms(0, 1) * 1e3 / REP)
    for name, v in us.items():
        out["%s_us" % name] = round(float(np.median(v)), 2)
        out["%s_us_min_max" % name] = [round(min(v), 2), round(max(v), 2)]
    out["offer_share_of_align"] = round(out["offer_us"] / out["align_us"], 4)
_, _, records, _, _, counts, _, _ = eng.bestshot_collect(shots, flush=True)
out["collected_at_flush"] = int(counts.sum())
rec = np.concatenate([records[b, :counts[b]] for b in range(B)])
if len(rec):                                                                     # why the qualities are what they are: the parts of the entries
    parts = np.stack([rec[:, 5], rec[:, 6] & 1023, (rec[:, 6] >> 10) & 1023, rec[:, 6] >> 20], axis=1)
    out["parts_median"] = dict(zip(("sharp", "size_w", "pose_w", "score_w"), (int(v) for v in np.median(parts, axis=0))))
    out["parts_zero"] = dict(zip(("sharp", "size_w", "pose_w", "score_w"), (int(v) for v in (parts == 0).sum(axis=0))))
eng.synchronize()
for p in (d_chips, d_offs, d_q, d_fl, d_frames):
    eng.device_free(p)
shots.close()
trk.close()
eng.close()
print(json.dumps(out))
