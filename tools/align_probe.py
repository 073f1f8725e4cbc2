#!/usr/bin/env python3
"""Aligned face chips at the flagship shape: 64 x 640x640 bf16, threshold decode (0.3 / 0.3), chips of S = 112 (uint8 BGR) for every kept
face, everything device-resident (the uint8 batch is uploaded once; chips, offsets and matrices stay in device buffers).

What is timed, after warming up every launch involved:
  align_us        the align launch ALONE: HIP events on the engine's main stream around 20 back-to-back cf_align_faces launches of the
                  same batch, divided by 20; median and spread of 7 such windows (chips_per_s = faces / that time)
  step_*_ms       host clock around 20 steps ending in a synchronise, step = forward + threshold decode enqueue [+ align], the two
                  kinds of window alternating in one process; medians of 7 windows
One JSON line.  --short: a few steps only, for a rocprofv3 --kernel-trace --stats run of its own (kernel name: align_chips_kernel)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa

short = "--short" in sys.argv
B, H, S, REP, WIN = 64, 640, 112, 20, 7
rng = np.random.default_rng(0)
eng = cfa.Engine(H, H, max_batch=B, dtype="bf16", decode_stream=False)
x = rng.integers(0, 256, (B, H, H, 3), dtype=np.uint8)
d_in = eng.device_alloc(x.nbytes)
eng.memcpy_h2d(d_in, x)
U8 = cfa._lib.CF_IN_U8_HWC_BGR


def forward_decode():
    eng.forward_enqueue(d_in, on_device=True, B=B, in_format=U8)
    eng.decode_threshold_enqueue(0.3, 0.3, 1024)


eng.forward_enqueue(d_in, on_device=True, B=B, in_format=U8)
faces = sum(len(d) for d, _ in eng.decode_threshold(0.3, 0.3, 1024))          # also sizes the decode's workspace
cap = max(faces, 1)
d_chips, d_off, d_mat = eng.device_alloc(cap * S * S * 3), eng.device_alloc((B + 1) * 4), eng.device_alloc(cap * 48)


def align():
    eng.align_faces_device(d_chips, d_off, cap, d_mat, size=S)


for _ in range(3):                                                              # warm-up: graph capture, code objects
    forward_decode()
    align()
eng.synchronize()
out = {"shape": "%d x %dx%d bf16, S=%d u8" % (B, H, H, S), "faces": faces}
if not short:
    us = []
    for _ in range(WIN):
        forward_decode()
        eng.event_record(0)
        for _ in range(REP):
            align()
        eng.event_record(1)
        us.append(eng.event_elapsed_ms(0, 1) * 1e3 / REP)
    ms = {"detect_decode": [], "detect_decode_align": []}
    for _ in range(WIN):
        for kind in ms:
            t0 = time.perf_counter()
            for _ in range(REP):
                forward_decode()
                if kind == "detect_decode_align":
                    align()
            eng.synchronize()
            ms[kind].append((time.perf_counter() - t0) * 1e3 / REP)
    med = float(np.median(us))
    out.update({"align_us": round(med, 2), "align_us_min_max": [round(min(us), 2), round(max(us), 2)],
                "chips_per_s": round(faces / (med * 1e-6)) if faces else 0,
                "chip_MB_written": round(faces * S * S * 3 / 1e6, 2)})
    for kind, v in ms.items():
        out["step_%s_ms" % kind] = round(float(np.median(v)), 4)
        out["step_%s_ms_min_max" % kind] = [round(min(v), 4), round(max(v), 4)]
    out["images_per_s"] = {k: round(B / (out["step_%s_ms" % k] * 1e-3)) for k in ms}
offs = np.empty(B + 1, np.int32)
eng.synchronize()
eng.memcpy_d2h(offs, d_off)
assert int(offs[-1]) == faces, (int(offs[-1]), faces)
for p in (d_chips, d_off, d_mat, d_in):
    eng.device_free(p)
eng.close()
print(json.dumps(out))
