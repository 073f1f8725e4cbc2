#!/usr/bin/env python3
"""What the flip test costs: one bf16 engine of 640 x 640 (built with flip_test=True, max_batch 32: its context holds 64 images) on a
uint8 batch that is resident on the device and read in place.

What is timed, after warming up every launch involved (three forwards per step: eager, graph capture, replay), with HIP events on the
engine's main stream around REP back-to-back calls between two synchronises (median and spread of WIN windows; the steps alternate
window by window, so a drift of the machine hits all three alike):
  flip_b32_ms     a flip forward of B = 32: mirror kernel (which also copies the caller's 32 images into the context's 2B input) ->
                  the plan over 64 images -> merge kernel
  plain_b64_ms    a plain forward of B = 64 on the same 32 images with their mirrors behind them, ready-made: the plan alone
  plain_b32_ms    a plain forward of B = 32: what a caller pays without the flip test
  mirror_merge_us flip_b32 - plain_b64 per window: what the two kernels of csrc/cf_flip.hip cost
  flip_over_plain flip_b32 / plain_b32 per window: the price of the flip test
The bytes the two kernels move are computed from the shapes: the mirror reads 32 images and writes 64 (B * H * W * 3 bytes each way per
image), the merge reads 64 x 160 x 160 records of 64 bytes, writes 32 x 160 x 160 of them and the heat plane.  Their share of 8 TB/s is
bytes over mirror_merge_us; it is an upper bound on the time, since the difference also holds the two launches.  A kernel-level
cross-check is a `rocprofv3 --kernel-trace --stats` run of `flip_probe.py --short` (kernels: mirror_u8_kernel, flip_heads_kernel).  One
JSON line.  No accuracy claim is made anywhere: there are no trained weights and no labelled set here."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import centerface_amd as cfa

short = "--short" in sys.argv
B, S, REP, WIN = 32, 640, 50, 7
PEAK = 8e12
U8 = cfa._lib.CF_IN_U8_HWC_BGR
rng = np.random.default_rng(0)
eng = cfa.Engine(S, S, max_batch=B, dtype="bf16", decode_stream=False, flip_test=True)
x = rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
both = np.concatenate([x, x[:, :, ::-1, :]])
d_both = eng.device_alloc(both.nbytes)
eng.memcpy_h2d(d_both, both)
del both


def flip_b32():
    eng.forward_enqueue(d_both, on_device=True, B=B, in_format=U8)


def plain_b64():
    eng.forward_enqueue(d_both, on_device=True, B=2 * B, in_format=U8)


def plain_b32():
    eng.forward_enqueue(d_both, on_device=True, B=B, in_format=U8)


steps = {"flip_b32_ms": (True, flip_b32), "plain_b64_ms": (False, plain_b64), "plain_b32_ms": (False, plain_b32)}


def timed(on, fn, rep):
    eng.set_flip_test(on)
    eng.synchronize()
    eng.event_record(0)
    for _ in range(rep):
        fn()
    eng.event_record(1)
    eng.synchronize()
    return eng.event_elapsed_ms(0, 1) / rep


for on, fn in steps.values():                                                   # warm-up: code objects, graph capture, the 2B input buffer
    timed(on, fn, 3)
# the flip forward and the plain forward of the doubled batch see the same 64 images: their heads must agree as tests/test_flip.py says
eng.set_flip_test(True)
flip_b32()
h_flip = eng.heads(sigmoid_hm=True)
mirror_bytes = 3 * B * S * S * 3
merge_bytes = (2 * B + B) * (S // 4) * (S // 4) * 64 + B * (S // 4) * (S // 4) * 4
out = {"shape": "%d x %dx%d uint8 images on the device, engine %dx%d bf16, flip_test context of %d" % (B, S, S, S, S, 2 * B),
       "rep": REP, "windows": WIN, "mirror_MB": round(mirror_bytes / 1e6, 2), "merge_MB": round(merge_bytes / 1e6, 2),
       "flip_heat_min_max": [float(h_flip["hm_sigmoid"].min()), float(h_flip["hm_sigmoid"].max())]}
if not short:
    ms = {k: [] for k in steps}
    for _ in range(WIN):
        for k, (on, fn) in steps.items():
            ms[k].append(timed(on, fn, REP))
    for k, v in ms.items():
        out[k] = round(float(np.median(v)), 4)
        out[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    us = [(a - b) * 1e3 for a, b in zip(ms["flip_b32_ms"], ms["plain_b64_ms"])]
    out["mirror_merge_us"] = round(float(np.median(us)), 2)
    out["mirror_merge_us_min_max"] = [round(min(us), 2), round(max(us), 2)]
    ratio = [a / b for a, b in zip(ms["flip_b32_ms"], ms["plain_b32_ms"])]
    out["flip_over_plain"] = round(float(np.median(ratio)), 4)
    out["flip_over_plain_min_max"] = [round(min(ratio), 4), round(max(ratio), 4)]
    out["mirror_merge_fraction_of_8TBps"] = round((mirror_bytes + merge_bytes) / (out["mirror_merge_us"] * 1e-6) / PEAK, 4) if out["mirror_merge_us"] > 0 else None
eng.synchronize()
eng.device_free(d_both)
eng.close()
print(json.dumps(out))
