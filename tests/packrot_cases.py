"""Restatements of rotated sources through packed views (cf_forward_packed_rot / cf_op_packed_rot, cf_merge_packed behind it /
cf_op_merge_packed_rot) in numpy, shared by tests/test_packrot_abi.py (no GPU) and tests/test_packrot.py.  The canvases: the stored
frame's BGR (the restated conversion for 4:2:0, taken before the turn), turned with numpy's own rot90, then the canvas restatement of
tests/pack_cases.py.  The rows: the statement's formulas in float64 -- the three drop rules in canvas coordinates with the interior test
against the UPRIGHT view, ux / uy, the table of the turn with the difference rounded to float32 once, the corner assignment per rot --
followed by the restated NMS of the packed merge.  A placement is a row (frame, canvas, sx0, sy0, sw, sh, dx, dy, dw, dh) whose source
rectangle is in pixels of the upright view."""
import numpy as np

from pack_cases import merge_packed_ref, packed_canvases_ref
from rot_cases import upright
from test_tiles_abi import nms_ref

ROTS = (90, 180, 270)


def upright_hw(frame_hw, rot):
    h, w = frame_hw
    return (w, h) if rot in (90, 270) else (h, w)


def packed_rot_canvases_ref(bgr_frames, rot, places, n_canvases, size, fill=(0, 0, 0)):
    """[N,H,W,3] of STORED BGR frames [Bf,h,w,3]: every frame turned upright, then tests/pack_cases.py's canvases."""
    return packed_canvases_ref(np.stack([upright(f, rot) for f in bgr_frames]), places, n_canvases, size, fill)


def merge_packed_rot_ref(places, n_frames, frame_hw, rot, dets_net, scores, lms_net, counts, metric="ios", thresh=0.5, edge=2.0):
    """cf_merge_packed behind cf_forward_packed_rot restated: per frame (dets [n,5], lms [n,10]) in the pixels of the STORED frame of
    ``frame_hw`` = (h, w) -- ALL kept rows, in keep order -- and the flags.  rot 0 is tests/pack_cases.py's merge."""
    if rot == 0:
        return merge_packed_ref(places, n_frames, frame_hw, dets_net, scores, lms_net, counts, metric, thresh, edge)
    h, w = frame_hw
    hu, wu = upright_hw(frame_hw, rot)
    dets_net, scores, lms_net = (np.asarray(a, np.float32) for a in (dets_net, scores, lms_net))
    rows = scores.shape[1]
    e, half = np.float32(edge), np.float32(0.5)
    h1, w1 = np.float64(h - 1), np.float64(w - 1)
    out, flags = [], np.zeros(n_frames, np.int32)
    places = np.asarray(places).reshape(-1, 10).tolist()
    for f in range(n_frames):
        cand_b, cand_s, cand_l = [], [], []
        for pf, img, sx0, sy0, sw, sh, dx, dy, dw, dh in places:
            if pf != f:
                continue
            n = int(counts[img])
            if n > rows:
                flags[f] |= 1
            xlo, xhi, ylo, yhi = np.float32(dx), np.float32(dx + dw), np.float32(dy), np.float32(dy + dh)
            sx, sy = np.float64(sw) / np.float64(dw), np.float64(sh) / np.float64(dh)

            def point(x, y):
                with np.errstate(over="ignore", invalid="ignore"):
                    ux = (np.float64(x) - np.float64(dx)) * sx + np.float64(sx0)
                    uy = (np.float64(y) - np.float64(dy)) * sy + np.float64(sy0)
                    X, Y = (uy, h1 - ux) if rot == 90 else (w1 - ux, h1 - uy) if rot == 180 else (w1 - uy, ux)
                    return np.float32(X), np.float32(Y)

            for i in range(min(n, rows)):
                c = dets_net[img, i]
                if not np.isfinite(c).all():
                    continue
                x1, y1, x2, y2 = c
                with np.errstate(over="ignore"):
                    cx, cy = (x1 + x2) * half, (y1 + y2) * half
                if not (xlo <= cx < xhi and ylo <= cy < yhi):
                    continue
                if (sx0 > 0 and x1 < xlo + e) or (sx0 + sw < wu and x2 > xhi - e) or (sy0 > 0 and y1 < ylo + e) or (sy0 + sh < hu and y2 > yhi - e):
                    continue
                # (X1, Y1), (X2, Y2) as the statement assigns them: which canvas corner feeds which value
                a, b = {90: ((x2, y1), (x1, y2)), 180: ((x2, y2), (x1, y1)), 270: ((x1, y2), (x2, y1))}[rot]
                cand_b.append(np.array(point(*a) + point(*b), np.float32))
                lm = lms_net[img, i]
                cand_l.append(np.array([v for k in range(5) for v in point(lm[2 * k], lm[2 * k + 1])], np.float32))
                cand_s.append(scores[img, i])
        if not cand_b:
            out.append((np.zeros((0, 5), np.float32), np.zeros((0, 10), np.float32)))
            continue
        b, s, l = np.stack(cand_b), np.array(cand_s, np.float32), np.stack(cand_l)
        keep = nms_ref(b, s, thresh, metric)
        out.append((np.concatenate([b[keep], s[keep][:, None]], 1), l[keep]))
    return out, flags
