#!/usr/bin/env python3
"""Aligned face chips at the flagship shape: 64 x 640x640 bf16, threshold decode (0.3 / 0.3), chips of S = 112 (uint8 BGR) for every kept
face, everything device-resident (the uint8 batch is uploaded once; chips, offsets and matrices stay in device buffers).

What is timed, after warming up every launch involved:
  align_us        the align launch ALONE: HIP events on the engine's main stream around 20 back-to-back cf_align_faces launches of the
                  same batch, divided by 20; median and spread of 7 such windows (chips_per_s = faces / that time)
  step_*_ms       host clock around 20 steps ending in a synchronise, step = forward + threshold decode enqueue [+ align], the two
                  kinds of window alternating in one process; medians of 7 windows
One JSON line.  --short: a few steps only, for a rocprofv3 --kernel-trace --stats run of its own (kernel name: align_chips_kernel).

--frame: the chips cut from the SOURCE frames instead (cf_align_faces_frame): 16 NV12 1080p frames resident on the device, a 640 x 640
bf16 context fed by cf_forward_yuv, a threshold decode with a low score threshold so that every frame keeps at least 8 faces, chips of
the first 8 faces per frame (max_per_image = 8), S = 112 and S = 224 uint8, device outputs.  Per S:
  frame_us        HIP events around 20 back-to-back cf_align_faces_frame launches, divided by 20; median and spread of 7 windows
  batch_us        the same for cf_align_faces on the 640 x 640 batch, the same faces and options
  copy_us         the time of the bytes the frame launch must move -- the chips written plus the source footprint of every chip (its
                  area in frame pixels from the matrix, 1.5 bytes per NV12 pixel) -- at the device-to-device copy rate measured here
                  (a 256 MB torch copy, read + written bytes over the event time)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa

short = "--short" in sys.argv


def frame_mode():
    import torch
    Bf, h, w, H, PER, REP, WIN = 16, 1080, 1920, 640, 8, 20, 7
    rng = np.random.default_rng(0)
    eng = cfa.Engine(H, H, max_batch=Bf, dtype="bf16", decode_stream=False)
    # 4-pixel runs of noise: detail that survives the stretch to 640 x 640 (the default weights answer to it)
    small = rng.integers(0, 256, (Bf, h * 3 // 2 // 4 + 1, w // 4), dtype=np.uint8)
    frames = np.ascontiguousarray(np.repeat(np.repeat(small, 4, 1), 4, 2)[:, :h * 3 // 2, :w])
    d_fr = eng.device_alloc(frames.nbytes)
    eng.memcpy_h2d(d_fr, frames)
    one = h * 3 // 2 * w
    planes = [(d_fr + b * one, d_fr + b * one + h * w) for b in range(Bf)]

    def forward_decode(thr):
        eng.forward_yuv_enqueue(planes, "nv12", on_device=True, h=h, w=w)
        return eng.decode_threshold(thr, 0.3, 1024)
    for thr in (0.3, 0.2, 0.1, 0.05, 0.02, 0.01):
        kept = [len(d) for d, _ in forward_decode(thr)]
        if min(kept) >= PER:
            break
    out = {"shape": "%d NV12 %dx%d frames, 640x640 bf16 context, %d faces per frame" % (Bf, w, h, PER), "score_thresh": thr,
           "kept_per_frame_min_max": [min(kept), max(kept)]}
    if min(kept) < PER:
        out["error"] = "the default weights keep fewer than %d faces in some frame" % PER
        print(json.dumps(out))
        return
    faces = Bf * PER
    a, b = torch.empty(256 << 20, dtype=torch.uint8, device="cuda"), torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rates = []
    for _ in range(5):
        ev[0].record()
        b.copy_(a)
        ev[1].record()
        torch.cuda.synchronize()
        rates.append(2 * a.numel() / (ev[0].elapsed_time(ev[1]) * 1e-3))
    rate = float(np.median(rates[1:]))
    out["copy_GB_per_s"] = round(rate / 1e9, 1)
    del a, b
    for S in (112, 224):
        d_chips, d_off, d_mat = eng.device_alloc(faces * S * S * 3), eng.device_alloc((Bf + 1) * 4), eng.device_alloc(faces * 48)
        calls = {"frame": lambda: eng.align_faces_frame_device(planes, "nv12", Bf, h, w, w, w, d_chips, d_off, faces, d_mat, size=S, max_per_image=PER),
                 "batch": lambda: eng.align_faces_device(d_chips, d_off, faces, d_mat, size=S, max_per_image=PER)}
        res = {}
        for name, call in calls.items():
            for _ in range(3):
                call()
            eng.synchronize()
            us = []
            for _ in range(2 if short else WIN):
                eng.event_record(0)
                for _ in range(REP):
                    call()
                eng.event_record(1)
                eng.synchronize()
                us.append(eng.event_elapsed_ms(0, 1) * 1e3 / REP)
            res[name + "_us"] = round(float(np.median(us)), 2)
            res[name + "_us_min_max"] = [round(min(us), 2), round(max(us), 2)]
            if name == "frame":                               # the matrices of the frame launch: the source footprint of every chip
                mats, offs = np.empty((faces, 6)), np.empty(Bf + 1, np.int32)
                eng.memcpy_d2h(mats, d_mat)
                eng.memcpy_d2h(offs, d_off)
                assert int(offs[-1]) == faces, (int(offs[-1]), faces)
                area = np.minimum((mats[:, 0] ** 2 + mats[:, 1] ** 2) * S * S, float(h * w))
                moved = faces * S * S * 3 + float(area.sum()) * 1.5
                res.update({"alignable": int(mats.any(1).sum()), "chip_MB_written": round(faces * S * S * 3 / 1e6, 2),
                            "source_MB_footprint": round(float(area.sum()) * 1.5 / 1e6, 2), "copy_us": round(moved / rate * 1e6, 2),
                            "median_source_px_per_chip_px": round(float(np.median(np.hypot(mats[:, 0], mats[:, 1]))), 3)})
        out["S%d" % S] = res
        for p in (d_chips, d_off, d_mat):
            eng.device_free(p)
    eng.device_free(d_fr)
    eng.close()
    print(json.dumps(out))


if "--frame" in sys.argv:
    frame_mode()
    sys.exit(0)
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
