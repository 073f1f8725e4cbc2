"""Restatements of packed views (cf_pack_views, cf_forward_packed / cf_op_packed, cf_merge_packed / cf_op_merge_packed) in Python integers
and numpy, shared by tests/test_pack_abi.py (no GPU) and tests/test_pack.py: the first-fit shelf packer, the canvases (a filled canvas,
then per placement the restated cut of its source rectangle pasted at its content) and the merge (``merge_views_ref`` generalised to
placements: the three drop rules against the placement's content, the float64 map, the restated greedy NMS).  A placement is a row
(frame, canvas, sx0, sy0, sw, sh, dx, dy, dw, dh)."""
import numpy as np

from test_tiles_abi import cut_ref, nms_ref

# the worked example of the statement: 1080 x 1920 frames in 640 x 640, levels 1000, 500 and 250, Bf = 2; (canvas, dx, dy) per item
WORKED_VIEWS = [(0, 0, 1920, 1080, 0, 140, 640, 360), (0, 0, 1920, 1080, 160, 230, 320, 180), (0, 0, 1920, 1080, 240, 275, 160, 90)]
WORKED_GUTTER_0 = [(0, 0, 0), (0, 0, 360), (0, 320, 360), (1, 0, 0), (1, 0, 360), (0, 480, 360)]
WORKED_GUTTER_16 = [(0, 0, 0), (0, 0, 376), (0, 336, 376), (1, 0, 0), (1, 0, 376), (1, 336, 376)]


def pack_views_ref(views, Bf, H, W, gutter=0):
    """cf_pack_views in Python integers: (placements, number of canvases), or None where the library answers CF_EINVAL."""
    views = [tuple(int(k) for k in v) for v in np.asarray(views).reshape(-1, 8).tolist()]
    if len(views) < 1 or Bf < 1 or gutter < 0 or H < 1 or W < 1:
        return None
    if any(v[6] < 1 or v[7] < 1 or v[6] > W or v[7] > H for v in views):
        return None
    canvases, places = [], []                            # a canvas: [shelves [[y, height, x_next], ...], y_next]
    for f in range(Bf):
        for v in views:
            dw, dh = v[6], v[7]
            spot = None
            for n, cv in enumerate(canvases):
                for shelf in cv[0]:
                    if dh <= shelf[1] and shelf[2] + dw <= W:
                        spot = (n, shelf[2], shelf[0])
                        shelf[2] += dw + gutter
                        break
                if spot is None and cv[1] + dh <= H:
                    spot = (n, 0, cv[1])
                    cv[0].append([cv[1], dh, dw + gutter])
                    cv[1] += dh + gutter
                if spot is not None:
                    break
            if spot is None:
                canvases.append([[[0, dh, dw + gutter]], dh + gutter])
                spot = (len(canvases) - 1, 0, 0)
            places.append((f, spot[0]) + v[:4] + (spot[1], spot[2], dw, dh))
    return places, len(canvases)


def unpacked_places(views, Bf):
    """The placement list {f, f * V + v, views[v]}: the one that reproduces cf_forward_views and cf_merge_views."""
    views = [tuple(int(k) for k in v) for v in np.asarray(views).reshape(-1, 8).tolist()]
    return [(f, f * len(views) + v) + views[v] for f in range(Bf) for v in range(len(views))]


def packed_canvases_ref(bgr_frames, places, n_canvases, size, fill=(0, 0, 0)):
    """[N,H,W,3] of BGR frames [Bf,h,w,3]: every canvas ``fill``, then per placement the restated cut of its source rectangle at (dh, dw)
    pasted at (dy, dx)."""
    out = np.empty((n_canvases, size[0], size[1], 3), np.uint8)
    out[:] = np.asarray(fill, np.uint8)
    for f, n, sx0, sy0, sw, sh, dx, dy, dw, dh in np.asarray(places).reshape(-1, 10).tolist():
        out[n, dy:dy + dh, dx:dx + dw] = cut_ref(bgr_frames[f], (sx0, sy0, sw, sh), (dh, dw))
    return out


def merge_packed_ref(places, n_frames, frame_hw, dets_net, scores, lms_net, counts, metric="ios", thresh=0.5, edge=2.0):
    """cf_merge_packed restated: per frame (dets [n,5], lms [n,10]) in frame pixels -- ALL kept rows, in keep order -- and the flags.
    dets_net [N,rows,4], scores [N,rows], lms_net [N,rows,10], counts [N]; a frame's candidates are walked in (placement index, row)
    order."""
    h, w = frame_hw
    dets_net, scores, lms_net = (np.asarray(a, np.float32) for a in (dets_net, scores, lms_net))
    rows = scores.shape[1]
    e, half = np.float32(edge), np.float32(0.5)
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
            scale = np.array([np.float64(sw) / np.float64(dw), np.float64(sh) / np.float64(dh)] * 5, np.float64)
            sub = np.array([dx, dy] * 5, np.float64)
            add = np.array([sx0, sy0] * 5, np.float64)
            for i in range(min(n, rows)):
                c = dets_net[img, i]
                if not np.isfinite(c).all():
                    continue
                x1, y1, x2, y2 = c
                with np.errstate(over="ignore"):
                    cx, cy = (x1 + x2) * half, (y1 + y2) * half
                if not (xlo <= cx < xhi and ylo <= cy < yhi):
                    continue
                if (sx0 > 0 and x1 < xlo + e) or (sx0 + sw < w and x2 > xhi - e) or (sy0 > 0 and y1 < ylo + e) or (sy0 + sh < h and y2 > yhi - e):
                    continue
                with np.errstate(over="ignore", invalid="ignore"):
                    cand_b.append(((c.astype(np.float64) - sub[:4]) * scale[:4] + add[:4]).astype(np.float32))
                    cand_l.append(((lms_net[img, i].astype(np.float64) - sub) * scale + add).astype(np.float32))
                cand_s.append(scores[img, i])
        if not cand_b:
            out.append((np.zeros((0, 5), np.float32), np.zeros((0, 10), np.float32)))
            continue
        b, s, l = np.stack(cand_b), np.array(cand_s, np.float32), np.stack(cand_l)
        keep = nms_ref(b, s, thresh, metric)
        out.append((np.concatenate([b[keep], s[keep][:, None]], 1), l[keep]))
    return out, flags
