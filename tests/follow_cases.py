"""The follower (include/centerface_hip.h "follow tracked faces between detections", csrc/cf_follow.hip) restated in numpy on top of the
tracker's restatement, line by line, and the scenes the tests run through it.

Integers are Python / int64 integers; the box geometry and the move are float64 (Python floats) in the order the header writes them;
a float32 value is a numpy float32 scalar.  Nothing here knows how the device computes."""
import math

import numpy as np

from track_cases import DEFAULTS, F32, RefTracker, grown

NONE, LEARNED, MOVED, LOST = 0, 1, 2, 3
P = 16
FORMATS = ("nv12", "nv21", "i420", "yv12", "bgr")


def luma_of(planes, fmt):
    """The luma of one frame given as its tuple of 2-D row views (plane 0: the Y plane [h, w], or the BGR rows [h, 3w]): int64 [h, w]."""
    p0 = np.asarray(planes[0]).astype(np.int64)
    if fmt != "bgr":
        return p0
    b, g, r = p0[:, 0::3], p0[:, 1::3], p0[:, 2::3]
    return (29 * b + 150 * g + 77 * r + 128) >> 8


def cells(luma, CX, CY, c, lo, n):
    """The n x n cells i, j in [lo, lo + n) about (CX, CY): [j][i] = (sum of luma + c*c/2) / (c*c), coordinates clamped into the frame."""
    h, w = luma.shape
    xs = np.clip(CX + np.arange(lo * c, (lo + n) * c), 0, w - 1)
    ys = np.clip(CY + np.arange(lo * c, (lo + n) * c), 0, h - 1)
    sums = luma[np.ix_(ys, xs)].reshape(n, c, n, c).sum(axis=(1, 3))
    return (sums + c * c // 2) // (c * c)


class Record(object):
    __slots__ = ("tpl", "c", "id", "box")

    def __init__(self):
        self.tpl, self.c, self.id, self.box = np.zeros((P, P), np.int64), 0, 0, np.zeros(4, F32).tobytes()


class RefFollower(RefTracker):
    """RefTracker plus the follower records.  ``space_hw``: the (H, W) the rows are in; ``tiled``: they are in frame pixels."""

    def __init__(self, n_streams, space_hw, tiled=False, search=4, max_sad=4096, **track_opts):
        RefTracker.__init__(self, n_streams, **track_opts)
        self.space, self.tiled, self.R, self.max_sad = (int(space_hw[0]), int(space_hw[1])), bool(tiled), int(search), int(max_sad)
        self.fol = [[Record() for _ in range(self.M)] for _ in range(n_streams)]

    def follow(self, s, luma):
        """One follow of stream s in the frame whose luma is ``luma`` [h, w].  Returns (dets [k,5], lms [k,10], info [k,3], moves [k,4])."""
        h, w = luma.shape
        if self.tiled:
            assert (h, w) == self.space
            fx = fy = 1.0
        else:
            fx, fy = float(w) / float(self.space[1]), float(h) / float(self.space[0])
        R = self.R
        moves = []
        for sl, rec in zip(self.slots[s], self.fol[s]):
            if not sl.alive:
                continue
            x1, y1, x2, y2 = (float(v) for v in sl.box)
            if not all(math.isfinite(v) for v in (x1, y1, x2, y2)):
                moves.append((0, 0, 0, NONE))
                continue
            side = max((x2 - x1) * fx, (y2 - y1) * fy)
            if not side > 0:
                moves.append((0, 0, 0, NONE))
                continue
            CX = int(math.floor(min(max((x1 + x2) * 0.5 * fx, -8192.0), 16384.0)))
            CY = int(math.floor(min(max((y1 + y2) * 0.5 * fy, -8192.0), 16384.0)))
            S = int(math.ceil(min(max(side, 1.0), 8192.0)))
            bits = np.asarray(sl.box, F32).tobytes()
            if rec.id != sl.id or rec.box != bits:                        # LEARN
                rec.c = (S + 15) // 16
                rec.tpl = cells(luma, CX, CY, rec.c, -8, P)
                rec.id, rec.box = sl.id, bits
                moves.append((0, 0, 0, LEARNED))
                continue
            c = rec.c                                                     # FOLLOW
            win = cells(luma, CX, CY, c, -8 - R, P + 2 * R)
            best = None
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    sad = int(np.abs(win[R + dy:R + dy + P, R + dx:R + dx + P] - rec.tpl).sum())
                    key = (sad, dx * dx + dy * dy, dy, dx)
                    if best is None or key < best:
                        best = key
            sad, _, dy, dx = best
            px, py = dx * c, dy * c
            if sad > self.max_sad:
                moves.append((px, py, sad, LOST))
                continue
            mx, my = float(px) / fx, float(py) / fy
            sl.box = np.array([F32(float(v) + (my if q & 1 else mx)) for q, v in enumerate(sl.box)], F32)
            sl.lms = np.array([F32(float(v) + (my if q & 1 else mx)) for q, v in enumerate(sl.lms)], F32)
            rec.box = sl.box.tobytes()
            moves.append((px, py, sad, MOVED))
        alive = [sl for sl in self.slots[s] if sl.alive]                  # step 5 of the update, from the moved state
        dets, olms, info = np.zeros((len(alive), 5), F32), np.zeros((len(alive), 10), F32), np.zeros((len(alive), 3), np.int32)
        for k, sl in enumerate(alive):
            dets[k, :4] = grown(sl.box, self.hold_grow, sl.misses)
            dets[k, 4] = sl.score
            olms[k] = sl.lms
            info[k] = (sl.id, sl.hits, sl.misses)
        return dets, olms, info, np.array(moves, np.int32).reshape(-1, 4)


def run_follow(boxes, scores, lms, counts, lumas, space_hw, detect=None, tiled=False, search=4, max_sad=4096, dets0=None, lms0=None,
               info0=None, moves0=None, **opts):
    """The tables ``ops.follow_sequence`` returns, from the restatement.  lumas[f * S + s] = the luma of frame f of stream s; rows at
    and past a count keep the bytes of dets0 / lms0 / info0 / moves0 (zeros by default)."""
    o = dict(DEFAULTS, **opts)
    boxes = np.asarray(boxes, F32)
    F, S, rows, _ = boxes.shape
    M = o["max_tracks"]
    detect = np.ones(F, bool) if detect is None else np.asarray(detect).astype(bool)
    dets = np.zeros((F, S, M, 5), F32) if dets0 is None else np.array(dets0, F32).reshape(F, S, M, 5)
    olms = np.zeros((F, S, M, 10), F32) if lms0 is None else np.array(lms0, F32).reshape(F, S, M, 10)
    info = np.zeros((F, S, M, 3), np.int32) if info0 is None else np.array(info0, np.int32).reshape(F, S, M, 3)
    moves = np.zeros((F, S, M, 4), np.int32) if moves0 is None else np.array(moves0, np.int32).reshape(F, S, M, 4)
    cnt, flags = np.zeros((F, S), np.int32), np.zeros((F, S), np.int32)
    trk = RefFollower(S, space_hw, tiled, search, max_sad, **o)
    for f in range(F):
        for s in range(S):
            if detect[f]:
                d, l, i, fl = trk.update(s, boxes[f, s], np.asarray(scores, F32)[f, s], np.asarray(lms, F32)[f, s], np.asarray(counts)[f, s])
                k = len(d)
                dets[f, s, :k], olms[f, s, :k], info[f, s, :k], flags[f, s] = d, l, i, fl      # (the device's update writes them too)
            d, l, i, m = trk.follow(s, lumas[f * S + s])
            k = len(d)
            dets[f, s, :k], olms[f, s, :k], info[f, s, :k], moves[f, s, :k], cnt[f, s] = d, l, i, m, k
    return dets, olms, info, cnt, flags, moves


# ---------------------------------------------------------------------------------------------- scenes
def planes_of(rng, fmt, luma_or_bgr, pad0=0, pad1=0):
    """One frame as the tuple of pitched 2-D row views ``frame_planes`` takes: plane 0 holds ``luma_or_bgr`` (uint8 [h, w] for 4:2:0,
    [h, w, 3] for BGR) in rows of pad0 more bytes than needed, the chroma planes are noise in rows padded by pad1."""
    a = np.asarray(luma_or_bgr, np.uint8)
    h, w = a.shape[:2]
    row0 = 3 * w if fmt == "bgr" else w
    buf = rng.integers(0, 256, (h, row0 + pad0), dtype=np.uint8)
    buf[:, :row0] = a.reshape(h, row0)
    out = [buf[:, :row0]]
    if fmt != "bgr":
        cw = w if fmt in ("nv12", "nv21") else w // 2
        for _ in range(1 if fmt in ("nv12", "nv21") else 2):
            out.append(rng.integers(0, 256, (h // 2, cw + pad1), dtype=np.uint8)[:, :cw])
    return tuple(out)


def canvas(rng, fmt, h, w, margin, smooth=4):
    """A random texture of (h + 2 margin) x (w + 2 margin) pixels, constant over smooth x smooth blocks so that a displaced match differs
    from the true one by a graded amount: uint8 [., .] for 4:2:0, [., ., 3] for BGR."""
    H, W = h + 2 * margin, w + 2 * margin
    shape = ((H + smooth - 1) // smooth, (W + smooth - 1) // smooth) + ((3,) if fmt == "bgr" else ())
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    return np.repeat(np.repeat(a, smooth, axis=0), smooth, axis=1)[:H, :W]


def view(cv, h, w, margin, tx, ty):
    """The h x w frame that sees the canvas moved by (tx, ty) pixels: everything in it moves by (tx, ty)."""
    return cv[margin - ty:margin - ty + h, margin - tx:margin - tx + w]
