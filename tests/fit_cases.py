"""Restatements of the aspect-preserving input (cf_fit_geometry, cf_forward_fit / cf_op_fit, cf_unfit_rows / cf_op_unfit) in Python
integers and numpy, shared by tests/test_fit_abi.py (no GPU) and tests/test_fit.py: the geometry, the canvas (the oracle's resize of the
restated conversion, pasted into a filled canvas) and the mapping of decoded rows back into frame pixels."""
import numpy as np

from oracle.centerface_oracle import resize_bilinear_u8

CENTER, TOPLEFT = 0, 1
ANCHORS = {"center": CENTER, "topleft": TOPLEFT}

# the worked values of the statement: (h, w), (H, W), upscale -> (rw, rh, dx, dy) with centre anchoring
WORKED = (
    ((1080, 1920), (640, 640), 1, (640, 360, 0, 140)),
    ((40, 120), (64, 96), 1, (96, 32, 0, 16)),
    ((120, 40), (64, 96), 1, (21, 64, 37, 0)),
    ((128, 192), (64, 96), 1, (96, 64, 0, 0)),
    ((30, 50), (64, 96), 0, (50, 30, 23, 17)),
)


def fit_geometry_ref(h, w, H, W, anchor="center", upscale=True):
    """(rw, rh, dx, dy) in Python integers (exact at any size)."""
    anchor = ANCHORS[anchor] if isinstance(anchor, str) else int(anchor)
    if not upscale and h <= H and w <= W:
        rw, rh = w, h
    elif w * H <= h * W:
        rh, rw = H, max(1, (2 * w * H + h) // (2 * h))
    else:
        rw, rh = W, max(1, (2 * h * W + w) // (2 * w))
    if anchor == CENTER:
        return rw, rh, (W - rw) // 2, (H - rh) // 2
    return rw, rh, 0, 0


def fit_ref(bgr, H, W, anchor="center", upscale=True, fill=(0, 0, 0)):
    """The canvas of one BGR frame [h,w,3]: resize to (rh, rw), then pad with ``fill``."""
    h, w = bgr.shape[:2]
    rw, rh, dx, dy = fit_geometry_ref(h, w, H, W, anchor, upscale)
    canvas = np.empty((H, W, 3), np.uint8)
    canvas[:] = np.asarray(fill, np.uint8)
    canvas[dy:dy + rh, dx:dx + rw] = resize_bilinear_u8(bgr, rh, rw)
    return canvas


def unfit_ref(geom, frame_hw, dets_net, scores, lms_net, counts):
    """The rows of a decode over fitted images mapped back: dets_net [B,rows,4], scores [B,rows], lms_net [B,rows,10], counts [B] ->
    ([(dets [n,5], lms [n,10]) per image], flags [B]).  Rows i < min(count, rows) in order; dropped when a corner is not finite or the
    float32 centre lies outside the content; X = float32((float64(x) - dx) * (float64(w) / float64(rw))), y likewise."""
    rw, rh, dx, dy = (int(v) for v in geom)
    h, w = frame_hw
    d, s, l = (np.asarray(a, np.float32) for a in (dets_net, scores, lms_net))
    B, rows = d.shape[:2]
    half = np.float32(0.5)
    sx, sy = np.float64(w) / np.float64(rw), np.float64(h) / np.float64(rh)
    off = np.array([dx, dy], np.float64)
    scale = np.array([sx, sy], np.float64)
    out, flags = [], np.zeros(B, np.int32)
    for b in range(B):
        n = int(counts[b])
        flags[b] = 1 if n > rows else 0
        od, ol = [], []
        for i in range(min(max(n, 0), rows)):
            c = d[b, i]
            if not np.isfinite(c).all():
                continue
            with np.errstate(over="ignore"):
                cx, cy = (c[0] + c[2]) * half, (c[1] + c[3]) * half
            if not (np.float32(dx) <= cx < np.float32(dx + rw) and np.float32(dy) <= cy < np.float32(dy + rh)):
                continue
            with np.errstate(over="ignore", invalid="ignore"):
                box = ((c.astype(np.float64) - np.tile(off, 2)) * np.tile(scale, 2)).astype(np.float32)
                lm = ((l[b, i].astype(np.float64) - np.tile(off, 5)) * np.tile(scale, 5)).astype(np.float32)
            od.append(np.concatenate([box, s[b, i:i + 1]]))
            ol.append(lm)
        out.append((np.array(od, np.float32).reshape(-1, 5), np.array(ol, np.float32).reshape(-1, 10)))
    return out, flags
