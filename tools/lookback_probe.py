#!/usr/bin/env python3
"""One lookback step beside the cf_track_update it follows: 16 streams, 256 rows per stream (a tracker of 16 streams x 256 slots, a
lookback object of 16 streams x 256 rows, depth 8, the default grow and confirm), a 128 x 160 bf16 engine at B = 16 on noise, a threshold
decode with max_out = 64 at a score threshold lowered until every image keeps rows.

An update needs a decode of its own and a push needs an update of its own, so no call can be timed alone in a loop.  Windows of three
kinds alternate on the engine's main stream (decode_stream=False: everything is on it), each fenced by the engine's events and a
synchronize, after warming up every launch involved and filling the delay line:
  decode_us   5 x cf_decode_threshold_enqueue of the same forward, divided by 5
  update_us   5 x (decode + cf_track_update in the device form), divided by 5
  step_us     5 x (decode + update + cf_lookback_step in the device form, a push that emits), divided by 5
median and spread of 7 windows of each kind, taken alternately; update_alone_us = update_us - decode_us and step_alone_us = step_us -
update_us are differences of medians.  The same frame is decoded every time; on noise the decode keeps overlapping boxes, the greedy
match leaves some of them unmatched in every update, and tracks keep being born until the tracker's 256 slots are full (min_hits = 1
holds every one of them).  The timed step is then the largest there is at this size: a push of 256 rows, the copy of the 256 own rows
of the due entry, and the walk over eight entries whose born rows find no place (rows_per_stream, backfilled_per_stream and dropped
are those of the last timed step).  One JSON line.  --short: a few calls only, for a rocprofv3 --kernel-trace --stats run of its own
(kernel: lookback_step_kernel)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa

short = "--short" in sys.argv
B, H, W, MAXF, M, DEPTH, REP, WIN = 16, 128, 160, 64, 256, 8, 5, 7
rng = np.random.default_rng(0)
eng = cfa.Engine(H, W, max_batch=B, dtype="bf16", decode_stream=False)
L, P = cfa._lib.lib(), cfa._lib.ptr
x = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
eng.forward_enqueue(x)
for thr in (0.3, 0.1, 0.03, 0.01, 0.001):
    dets, lms, counts = np.zeros((B, MAXF, 5), np.float32), np.zeros((B, MAXF, 10), np.float32), np.zeros(B, np.int32)
    eng._chk(L.cf_decode_threshold(eng._h, thr, 0.3, MAXF, P(dets), P(lms), P(counts)))
    if int(counts.min()) >= 8:
        break
trk = cfa.Tracker(eng, B, min_hits=1, max_tracks=M)
lb = cfa.Lookback(eng, B, depth=DEPTH, rows=M)
d_state = eng.device_alloc(B * 4 * 4)


def decode():
    eng.decode_threshold_enqueue(thr, 0.3, MAXF)


def update():
    decode()
    eng.track_update_device(trk, 0)


def step():
    update()
    eng.lookback_step_device(lb, 0, B, True, state_ptr=d_state)


for _ in range(DEPTH + 3):                                                   # warm-up: code objects; the line fills, every later push emits
    step()
eng.synchronize()
out = {"shape": "%d streams, engine %dx%d bf16, decode max_out %d, tracker %d slots, lookback depth %d x %d rows" % (B, H, W, MAXF, M, DEPTH, M),
       "score_thresh": thr}
if not short:
    kinds = (("decode", decode), ("update", update), ("step", step))
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
    out["update_alone_us"] = round(out["update_us"] - out["decode_us"], 2)
    out["step_alone_us"] = round(out["step_us"] - out["update_us"], 2)
eng.synchronize()
state = np.zeros((B, 4), np.int32)
eng.memcpy_d2h(state, d_state)
out.update(rows_per_stream=[int(v) for v in state[:, 1]], backfilled_per_stream=[int(v) for v in state[:, 2]], dropped=int((state[:, 3] & 1).sum()),
           emitted_seq=int(state[0, 0]))
eng.device_free(d_state)
lb.close()
trk.close()
eng.close()
print(json.dumps(out))
