"""Restatements of multi-scale detection (cf_view_layout, cf_forward_views / cf_op_views, cf_merge_views / cf_op_merge_views) in Python
integers and numpy, shared by tests/test_views_abi.py (no GPU) and tests/test_views.py: the layout on top of the restated tile grid and
fit geometry, the canvases (the restated tile cut of each view's source rectangle, pasted into a filled canvas) and the merge (the three
drop rules, the float64 map, the restated greedy NMS)."""
import numpy as np

from fit_cases import fit_geometry_ref
from test_tiles_abi import cut_ref, nms_ref, tile_grid_ref

CENTER, TOPLEFT = 0, 1
ANCHORS = {"center": CENTER, "topleft": TOPLEFT}

# the worked example of the statement: 1080 x 1920 in 640 x 640, tile 640, overlap 128, levels 1000 and 500
WORKED = [(0, 0, 640, 640, 0, 0, 640, 640), (426, 0, 640, 640, 0, 0, 640, 640), (852, 0, 640, 640, 0, 0, 640, 640), (1280, 0, 640, 640, 0, 0, 640, 640),
          (0, 440, 640, 640, 0, 0, 640, 640), (426, 440, 640, 640, 0, 0, 640, 640), (852, 440, 640, 640, 0, 0, 640, 640),
          (1280, 440, 640, 640, 0, 0, 640, 640), (0, 0, 1920, 1080, 0, 140, 640, 360), (0, 0, 1920, 1080, 160, 230, 320, 180)]


def view_layout_ref(h, w, H, W, tile_h=0, tile_w=0, overlap=0, anchor="center", scales_pm=(1000,)):
    """cf_view_layout in Python integers: [(sx0, sy0, sw, sh, dx, dy, dw, dh), ...], or None where the library answers CF_EINVAL."""
    anchor = ANCHORS[anchor] if isinstance(anchor, str) else int(anchor)
    if anchor not in (CENTER, TOPLEFT) or not 0 <= len(scales_pm) <= 8 or any(not 1 <= pm <= 1000 for pm in scales_pm):
        return None
    if not (2 <= h <= 8192 and 2 <= w <= 8192 and H >= 1 and W >= 1):
        return None
    out = []
    if tile_h != 0 or tile_w != 0:
        bad = h < 2 or w < 2 or tile_h < 2 or tile_w < 2 or overlap < 0 or ((h | w | tile_h | tile_w | overlap) & 1) or overlap >= min(tile_h, tile_w)
        if bad:
            return None
        tiles = tile_grid_ref(h, w, tile_h, tile_w, overlap, with_full=False)
        if len(tiles) > 1:
            out += [(x0, y0, rw, rh, 0, 0, W, H) for x0, y0, rw, rh in tiles]
    if scales_pm:
        rw, rh, _, _ = fit_geometry_ref(h, w, H, W, "center", True)
        for pm in scales_pm:
            dw, dh = max(1, (rw * pm + 500) // 1000), max(1, (rh * pm + 500) // 1000)
            out.append((0, 0, w, h) + (((W - dw) // 2, (H - dh) // 2) if anchor == CENTER else (0, 0)) + (dw, dh))
    return out or None


def views_ref(bgr, views, H, W, fill=(0, 0, 0)):
    """The canvases [V,H,W,3] of one BGR frame [h,w,3]: per view the restated cut of its source rectangle at (dh, dw), pasted into a
    canvas of ``fill``."""
    out = np.empty((len(views), H, W, 3), np.uint8)
    out[:] = np.asarray(fill, np.uint8)
    for v, (sx0, sy0, sw, sh, dx, dy, dw, dh) in enumerate(np.asarray(views).reshape(-1, 8).tolist()):
        out[v, dy:dy + dh, dx:dx + dw] = cut_ref(bgr, (sx0, sy0, sw, sh), (dh, dw))
    return out


def canvases_ref(bgr_frames, views, size, fill=(0, 0, 0)):
    """[Bf,V,H,W,3] of BGR frames [Bf,h,w,3]."""
    return np.stack([views_ref(f, views, size[0], size[1], fill) for f in bgr_frames])


def merge_views_ref(views, frame_hw, dets_net, scores, lms_net, counts, metric="ios", thresh=0.5, edge=2.0):
    """cf_merge_views restated: per frame (dets [n,5], lms [n,10]) in frame pixels -- ALL kept rows, in keep order -- and the flags.
    dets_net [Bf,V,rows,4], scores [Bf,V,rows], lms_net [Bf,V,rows,10], counts [Bf,V]."""
    h, w = frame_hw
    dets_net, scores, lms_net = (np.asarray(a, np.float32) for a in (dets_net, scores, lms_net))
    Bf, V, rows = scores.shape
    e, half = np.float32(edge), np.float32(0.5)
    out, flags = [], np.zeros(Bf, np.int32)
    for f in range(Bf):
        cand_b, cand_s, cand_l = [], [], []
        for v, (sx0, sy0, sw, sh, dx, dy, dw, dh) in enumerate(np.asarray(views).reshape(-1, 8).tolist()):
            n = int(counts[f][v])
            if n > rows:
                flags[f] |= 1
            xlo, xhi, ylo, yhi = np.float32(dx), np.float32(dx + dw), np.float32(dy), np.float32(dy + dh)
            scale = np.array([np.float64(sw) / np.float64(dw), np.float64(sh) / np.float64(dh)] * 5, np.float64)
            sub = np.array([dx, dy] * 5, np.float64)
            add = np.array([sx0, sy0] * 5, np.float64)
            for i in range(min(n, rows)):
                c = dets_net[f, v, i]
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
                    cand_l.append(((lms_net[f, v, i].astype(np.float64) - sub) * scale + add).astype(np.float32))
                cand_s.append(scores[f, v, i])
        if not cand_b:
            out.append((np.zeros((0, 5), np.float32), np.zeros((0, 10), np.float32)))
            continue
        b, s, l = np.stack(cand_b), np.array(cand_s, np.float32), np.stack(cand_l)
        keep = nms_ref(b, s, thresh, metric)
        out.append((np.concatenate([b[keep], s[keep][:, None]], 1), l[keep]))
    return out, flags
