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
(kernel: lookback_step_kernel).

--traced: the step of an object with cf_lookback_trace_enable (cf_lookback_step_frames) beside the untraced one, 16 streams of 1920 x 1080
frames on the device (NV12, then BGR; the same noise frame at every step, so every chain runs its full eight distances and finds
displacement 0), depth 8, rows in the network space of the same 128 x 160 engine (fx = 12, fy = 8.4375).  The births are made with the
tracker: a tracker of k slots that is reset before every update gives k newborn tracks per stream and step (k = 1, 16); for k = 0 the
decode's score threshold is 2.0, so there is no row and no birth: the step is retain, a trace launch whose workgroups leave, and an empty push.  Windows as above -- 5 x (decode [+ reset] + update) and 5 x (the same +
step), 7 of each, alternately; the step alone is the difference of the medians -- for the untraced step, the traced step on NV12 and
on BGR, each on an object of its own.  Beside them scene_us: 5 x cf_scene_check (device form, both of its kernels) over the same frames,
whose first kernel is the existing pass over the same luma.  births_side_px: the sides, in frame pixels, of the boxes that were born.
--short here: a few traced steps with 16 births on NV12 and on BGR and a few scene checks, for a rocprofv3 --kernel-trace --stats run
(kernels: lookback_retain_kernel, lookback_trace_kernel, lookback_step_kernel, the scene check's two).

--kernels FMT K: the births of the engine's decode have whatever size the noise gives them, and the trace costs what its largest face
costs.  This mode runs chosen rows instead, through cf_op_lookback_trace, for a rocprofv3 --kernel-trace --stats run that times the
kernels themselves: 16 streams of 1920 x 1080 frames in FMT (one noise frame throughout), rows in frame pixels, depth 8, 16 pushes; the
first eight bear nothing, each of the last eight bears K tracks of 64 x 64 pixels per stream (c = 4), whose chains run all eight
distances.  Then cf_op_scene over the same frames.  (The retain launch is the same in all sixteen steps; of the trace launches the
first eight find no born row -- their time is the minimum in the statistics, the full chains' the maximum.)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa

short = "--short" in sys.argv
if "--kernels" in sys.argv:
    fmt, K = sys.argv[sys.argv.index("--kernels") + 1], int(sys.argv[sys.argv.index("--kernels") + 2])
    S, F, FH, FW = 16, 16, 1080, 1920
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 256, (FH, FW, 3) if fmt == "bgr" else (FH * 3 // 2, FW), dtype=np.uint8)
    frames = [(frame.reshape(FH, -1),) if fmt == "bgr" else (frame[:FH], frame[FH:]) for _ in range(F * S)]
    rows = 8 * max(K, 1)
    d, l, i = np.zeros((F, S, rows, 5), np.float32), np.zeros((F, S, rows, 10), np.float32), np.zeros((F, S, rows, 3), np.int32)
    c = np.zeros((F, S), np.int32)
    for f in range(8, F):
        n = (f - 7) * K
        c[f] = n
        for k in range(n):                                                       # track k + 1, born at step 8 + k // K, stands still
            x, y = 40.0 + (k % 16) * 110.0, 30.0 + (k // 16) * 120.0
            d[f, :, k] = (x, y, x + 64.0, y + 64.0, 0.9)
            i[f, :, k] = (k + 1, f - 7 - k // K, 0)
    out = cfa.ops.lookback_trace_sequence(d, l, i, c, frames, fmt, (FH, FW), tiled=True, depth=8, rows=max(rows, 8))
    codes = sorted(set(out[5][8:, :, :, 3].ravel().tolist()))
    sc = cfa.ops.scene_sequence(frames, fmt, S)
    print(json.dumps({"fmt": fmt, "births_per_stream_and_step": K, "backfilled_per_stream": sorted(set(out[4][8:, :, 2].ravel().tolist())),
                      "codes": codes, "moves": sorted(set(np.abs(out[5][8:, :, :, :2]).ravel().tolist())), "scene_codes": sorted(set(sc[:, :, 0].ravel().tolist()))}))
    sys.exit(0)
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


def traced_mode():
    """See the module's docstring.  Prints one JSON line."""
    FH, FW = 1080, 1920
    frames = {}
    for fmt, nbytes in (("nv12", FH * FW * 3 // 2), ("bgr", FH * FW * 3)):
        host = rng.integers(0, 256, nbytes, dtype=np.uint8)
        base = [eng.device_alloc(nbytes) for _ in range(B)]
        for p in base:
            eng.memcpy_h2d(p, host)
        planes = [(p, p + FH * FW) if fmt == "nv12" else (p,) for p in base]
        frames[fmt] = (base, planes, FW if fmt == "nv12" else 3 * FW, FW if fmt == "nv12" else 0)
    scn = cfa.SceneCuts(eng, B)
    d_state = eng.device_alloc(B * 4 * 4)
    out = {"shape": "%d streams of %dx%d frames, rows of a %dx%d bf16 engine, lookback depth %d x %d rows, search 4" % (B, FW, FH, H, W, DEPTH, M),
           "score_thresh": thr}

    def window(call):
        eng.event_record(0)
        for _ in range(REP):
            call()
        eng.event_record(1)
        eng.synchronize()
        return eng.event_elapsed_ms(0, 1) * 1e3 / REP

    def scene(fmt):
        _, planes, p0, p1 = frames[fmt]
        eng.scene_check_device(planes, fmt, B, FH, FW, p0, p1, scn)

    for k in ((16,) if short else (0, 1, 16)):
        trk = cfa.Tracker(eng, B, min_hits=1, max_tracks=max(k, 1) if k else 16)

        def update():
            eng.decode_threshold_enqueue(thr if k else 2.0, 0.3, MAXF)          # (k = 0: no score passes, no row, no birth)
            if k:
                trk.reset()
            eng.track_update_device(trk, 0)

        objs = {"untraced": cfa.Lookback(eng, B, depth=DEPTH, rows=M), "nv12": cfa.Lookback(eng, B, depth=DEPTH, rows=M).trace(),
                "bgr": cfa.Lookback(eng, B, depth=DEPTH, rows=M).trace()}

        def step(name):
            update()
            if name == "untraced":
                eng.lookback_step_device(objs[name], 0, B, True, state_ptr=d_state)
            else:
                _, planes, p0, p1 = frames[name]
                eng.lookback_step_frames_device(objs[name], planes, name, B, FH, FW, p0, p1, 0, True, state_ptr=d_state)

        for _ in range(20):                                                      # the slots fill; then no update bears a track unless it was reset
            update()
        eng.synchronize()
        res = {}
        for name in (("nv12", "bgr") if short else ("untraced", "nv12", "bgr")):
            for _ in range(DEPTH + 3):                                           # warm-up: code objects; the line fills, every later push emits
                step(name)
            eng.synchronize()
            if not short:
                us = {"update": [], "step": []}
                for _ in range(WIN):
                    us["update"].append(window(update))
                    us["step"].append(window(lambda: step(name)))
                res["%s_step_alone_us" % name] = round(float(np.median(us["step"]) - np.median(us["update"])), 2)
                res["%s_step_us_min_max" % name] = [round(min(us["step"]), 2), round(max(us["step"]), 2)]
                res["%s_update_us" % name] = round(float(np.median(us["update"])), 2)
            eng.synchronize()
            state = np.zeros((B, 4), np.int32)
            eng.memcpy_d2h(state, d_state)
            res["%s_backfilled_per_stream" % name] = sorted(set(int(v) for v in state[:, 2]))
        update()
        got = eng.lookback_step_frames(objs["nv12"], None, "nv12", push=False)      # one emitted frame read back: the sides of what was born
        sides = [float(max((d[2] - d[0]) * FW / W, (d[3] - d[1]) * FH / H)) for b in range(B) for d, i in zip(got[0][b, :got[3][b]], got[2][b, :got[3][b]])
                 if i[1] == 0 and i[2] > 0]
        res["births_side_px"] = [round(min(sides), 1), round(float(np.median(sides)), 1), round(max(sides), 1)] if sides else []
        out["births_%d" % k] = res
        for o in objs.values():
            o.close()
        trk.close()
    for fmt in ("nv12", "bgr"):
        for _ in range(3):
            scene(fmt)
        eng.synchronize()
        if not short:
            v = [window(lambda: scene(fmt)) for _ in range(WIN)]
            out["scene_%s_us" % fmt] = round(float(np.median(v)), 2)
            out["scene_%s_us_min_max" % fmt] = [round(min(v), 2), round(max(v), 2)]
    eng.synchronize()
    scn.close()
    eng.device_free(d_state)
    for base, _, _, _ in frames.values():
        for p in base:
            eng.device_free(p)
    eng.close()
    print(json.dumps(out))


if "--traced" in sys.argv:
    if thr > 0.01 or int(counts.min()) < 16:                                    # sixteen births per stream need sixteen rows per image
        for thr in (0.01, 0.003, 0.001, 0.0001):
            eng._chk(L.cf_decode_threshold(eng._h, thr, 0.3, MAXF, P(dets), P(lms), P(counts)))
            if int(counts.min()) >= 16:
                break
    traced_mode()
    sys.exit(0)
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
