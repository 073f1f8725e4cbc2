"""Restatements of the rotated sources (cf_rot_geometry, cf_forward_rot / cf_op_rot, cf_unfit_rows behind it / cf_op_unrot) in numpy,
shared by tests/test_rot_abi.py (no GPU) and tests/test_rot.py: the upright view is numpy's own rot90, the canvas what
tests/fit_cases.py (fit) or the oracle's resize (stretch) makes of it, and the rows come back through the statement's table in
float64 -> float32."""
import numpy as np

from fit_cases import fit_geometry_ref, fit_ref
from oracle.centerface_oracle import resize_bilinear_u8

ROTS = (0, 90, 180, 270)
K = {0: 0, 90: -1, 180: 2, 270: 1}          # rot (clockwise degrees that make the stored frame upright) -> np.rot90's k


def upright(bgr, rot):
    """The upright view U of one stored BGR frame [h,w,3]."""
    return np.ascontiguousarray(np.rot90(bgr, K[rot]))


def rot_geometry_ref(h, w, H, W, rot, stretch, anchor="center", upscale=True):
    """(rw, rh, dx, dy) of the upright view of a stored h x w frame in the canvas."""
    if stretch:
        return W, H, 0, 0
    hu, wu = (w, h) if rot in (90, 270) else (h, w)
    return fit_geometry_ref(hu, wu, H, W, anchor, upscale)


def rot_ref(bgr, rot, H, W, stretch, **fit):
    """The canvas of one stored BGR frame [h,w,3]."""
    if stretch:
        return resize_bilinear_u8(upright(bgr, rot), H, W)
    return fit_ref(upright(bgr, rot), H, W, **fit)


def unrot_ref(geom, frame_hw, rot, dets_net, scores, lms_net, counts):
    """fit_cases.unfit_ref's loop with the statement's table: dets_net [B,rows,4], scores [B,rows], lms_net [B,rows,10], counts [B] ->
    ([(dets [n,5], lms [n,10]) per image], flags [B]), in the pixels of the STORED frame of ``frame_hw`` = (h, w).  Kept or dropped in
    canvas coordinates; ux = (float64(x) - dx) * (float64(wu) / rw), uy likewise; the differences (h-1) - . and (w-1) - . are taken in
    float64 and rounded to float32 once; the box is an assignment of mapped corners."""
    rw, rh, dx, dy = (int(v) for v in geom)
    h, w = frame_hw
    hu, wu = (w, h) if rot in (90, 270) else (h, w)
    d, s, l = (np.asarray(a, np.float32) for a in (dets_net, scores, lms_net))
    B, rows = d.shape[:2]
    half = np.float32(0.5)
    sx, sy = np.float64(wu) / np.float64(rw), np.float64(hu) / np.float64(rh)
    h1, w1 = np.float64(h - 1), np.float64(w - 1)

    def point(x, y):
        with np.errstate(over="ignore", invalid="ignore"):
            ux, uy = (np.float64(x) - np.float64(dx)) * sx, (np.float64(y) - np.float64(dy)) * sy
            X, Y = {0: (ux, uy), 90: (uy, h1 - ux), 180: (w1 - ux, h1 - uy), 270: (w1 - uy, ux)}[rot]
            return np.float32(X), np.float32(Y)

    out, flags = [], np.zeros(B, np.int32)
    for b in range(B):
        n = int(counts[b])
        flags[b] = 1 if n > rows else 0
        od, ol = [], []
        for i in range(min(max(n, 0), rows)):
            x1, y1, x2, y2 = d[b, i]
            if not np.isfinite(d[b, i]).all():
                continue
            with np.errstate(over="ignore"):
                cx, cy = (x1 + x2) * half, (y1 + y2) * half
            if not (np.float32(dx) <= cx < np.float32(dx + rw) and np.float32(dy) <= cy < np.float32(dy + rh)):
                continue
            # (X1, Y1), (X2, Y2) as the statement assigns them: which canvas corner feeds which value
            a, c = {0: ((x1, y1), (x2, y2)), 90: ((x2, y1), (x1, y2)), 180: ((x2, y2), (x1, y1)), 270: ((x1, y2), (x2, y1))}[rot]
            box = np.array(point(*a) + point(*c), np.float32)
            lm = np.array([v for k in range(5) for v in point(l[b, i, 2 * k], l[b, i, 2 * k + 1])], np.float32)
            od.append(np.concatenate([box, s[b, i:i + 1]]))
            ol.append(lm)
        out.append((np.array(od, np.float32).reshape(-1, 5), np.array(ol, np.float32).reshape(-1, 10)))
    return out, flags
