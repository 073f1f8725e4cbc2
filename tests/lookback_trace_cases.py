"""The traced lookback ("lookback with a trace" in include/centerface_hip.h) restated in numpy: RefLookback (tests/lookback_cases.py) extended by
the retained luma planes and the backward walk, built from the follower's restated pieces (follow_cases.cells / luma_of), and the scenes
the tests run through it and through the device.

Integers are Python / int64 integers; the box geometry and the move are float64 (Python floats) in the order the header writes them; a
float32 value is a numpy float32 scalar.  Nothing here knows how the device computes."""
import math

import numpy as np

from follow_cases import LOST, MOVED, NONE, P, canvas, cells, luma_of, planes_of, view
from lookback_cases import CONFIRM, CUT, DEPTH, GROW, ROWS, SAME, RefLookback, _Entry, grown

F32 = np.float32


def moved_row(box, lms, px, py, fx, fy):
    """The follower's formula: every x of the box and the landmarks plus px / fx, every y plus py / fy, float64, one rounding."""
    mx, my = float(px) / fx, float(py) / fy
    b = np.array([F32(float(v) + (my if q & 1 else mx)) for q, v in enumerate(box)], F32)
    l = np.array([F32(float(v) + (my if q & 1 else mx)) for q, v in enumerate(lms)], F32)
    return b, l


class RefLookbackTrace(RefLookback):
    """RefLookback whose entries also hold the luma of their frame and the trace table of their born rows.  ``space_hw``: the (H, W) the
    rows are in; ``tiled``: they are in frame pixels."""

    def __init__(self, streams, space_hw, tiled=False, search=4, max_sad=4096, **opts):
        RefLookback.__init__(self, streams, **opts)
        self.space, self.tiled, self.R, self.max_sad = (int(space_hw[0]), int(space_hw[1])), bool(tiled), int(search), int(max_sad)

    def scale(self, luma):
        h, w = luma.shape
        if self.tiled:
            assert (h, w) == self.space
            return 1.0, 1.0
        return float(w) / float(self.space[1]), float(h) / float(self.space[0])

    def trace(self, q):
        """The trace table of the newest entry E = q[-1]: {row: {distance: (PX, PY, SAD, code)}}."""
        E, m, R = q[-1], len(q) - 1, self.R
        fx, fy = self.scale(E.luma)
        T = {}
        for i in range(E.n):
            x1, y1, x2, y2 = (float(v) for v in E.dets[i, :4])
            if not E.born[i] or not all(math.isfinite(v) for v in (x1, y1, x2, y2)):
                continue
            side = max((x2 - x1) * fx, (y2 - y1) * fy)
            if not side > 0:
                T[i] = {d: (0, 0, 0, NONE) for d in range(1, m + 1)}
                continue
            CX = int(math.floor(min(max((x1 + x2) * 0.5 * fx, -8192.0), 16384.0)))
            CY = int(math.floor(min(max((y1 + y2) * 0.5 * fy, -8192.0), 16384.0)))
            S = int(math.ceil(min(max(side, 1.0), 8192.0)))
            c = (S + 15) // 16
            tpl = cells(E.luma, CX, CY, c, -8, P)
            PX = PY = 0
            T[i] = {}
            for d in range(1, m + 1):
                if q[m - d + 1].cut:
                    break
                win = cells(q[m - d].luma, CX + PX, CY + PY, c, -8 - R, P + 2 * R)
                best = None
                for dy in range(-R, R + 1):
                    for dx in range(-R, R + 1):
                        sad = int(np.abs(win[R + dy:R + dy + P, R + dx:R + dx + P] - tpl).sum())
                        key = (sad, dx * dx + dy * dy, dy, dx)
                        if best is None or key < best:
                            best = key
                sad, _, dy, dx = best
                if sad > self.max_sad:
                    for e in range(d, m + 1):
                        T[i][e] = (PX, PY, sad, LOST)
                    break
                PX, PY = PX + dx * c, PY + dy * c
                T[i][d] = (PX, PY, sad, MOVED)
        return T

    def step(self, s, push=True, dets=None, lms=None, info=None, count=0, code=None, luma=None):
        """As RefLookback.step, with ``luma`` [h, w] the luma of the pushed frame.  Returns (dets, lms, info, state, moves [k, 4])."""
        q = self.queue[s]
        if push:
            n = min(max(int(count), 0), len(dets), self.rows)
            ids = np.asarray(info[:n, 0], np.int32)
            cut = bool(self.pending[s]) or (code is not None and int(code) != SAME)
            self.pending[s] = 0
            e = _Entry(self.seq_next[s], cut, np.array(dets[:n], F32), np.array(lms[:n], F32), np.array(info[:n], np.int32), ids > self.max_id[s])
            e.luma = np.asarray(luma, np.int64)
            q.append(e)
            e.T = self.trace(q)
            self.seq_next[s] += 1
            if n:
                self.max_id[s] = max(self.max_id[s], int(ids.max()))
        if not (len(q) == self.depth + 1 if push else len(q) > 0):
            return (np.zeros((0, 5), F32), np.zeros((0, 10), F32), np.zeros((0, 3), np.int32), np.array([-1, 0, 0, 0], np.int32),
                    np.zeros((0, 4), np.int32))
        t = q.pop(0)
        od, ol, oi, om = [t.dets], [t.lms], [t.info], [np.zeros((t.n, 4), np.int32)]
        written, flags = t.n, 0
        stop = next((j for j, e in enumerate(q) if e.cut), len(q))
        for j0 in range(stop):
            e, j = q[j0], j0 + 1
            fx, fy = self.scale(e.luma)
            for i in range(e.n):
                if not e.born[i] or not np.isfinite(e.dets[i, :4]).all():
                    continue
                seen = sum(1 for later in q[j0:stop] if (later.info[:, 0] == e.info[i, 0]).any())
                if seen < self.confirm:
                    continue
                if written >= self.rows:
                    flags |= 1
                    continue
                px, py, sad, tc = e.T[i][j]
                row, lm = e.dets[i].copy(), e.lms[i].copy()
                if px != 0 or py != 0:
                    row[:4], lm = moved_row(row[:4], lm, px, py, fx, fy)
                row[:4] = grown(row[:4], self.grow, j)
                od.append(row[None]), ol.append(lm[None]), oi.append(np.array([[e.info[i, 0], 0, j]], np.int32))
                om.append(np.array([[px, py, sad, tc]], np.int32))
                written += 1
        return (np.concatenate(od), np.concatenate(ol), np.concatenate(oi), np.array([t.seq, t.n, written - t.n, flags], np.int32),
                np.concatenate(om))


def run_lookback_trace(dets_in, lms_in, info_in, counts_in, lumas, space_hw, push=None, cuts=None, tiled=False, search=4, max_sad=4096,
                       dets=None, lms_out=None, info=None, moves=None, **opts):
    """RefLookbackTrace over the tables ``ops.lookback_trace_sequence`` takes (lumas[f * S + s] = the luma of frame f of stream s); the same
    return, rows at and past a count keeping the prefill."""
    o = dict(depth=DEPTH, rows=ROWS, grow=GROW, confirm=CONFIRM)
    o.update(opts)
    F, S = np.asarray(counts_in).shape
    R = o["rows"]
    od = np.zeros((F, S, R, 5), F32) if dets is None else np.array(dets, F32)
    ol = np.zeros((F, S, R, 10), F32) if lms_out is None else np.array(lms_out, F32)
    oi = np.zeros((F, S, R, 3), np.int32) if info is None else np.array(info, np.int32)
    om = np.zeros((F, S, R, 4), np.int32) if moves is None else np.array(moves, np.int32)
    oc, st = np.zeros((F, S), np.int32), np.zeros((F, S, 4), np.int32)
    ref = RefLookbackTrace(S, space_hw, tiled, search, max_sad, **o)
    for f in range(F):
        for s in range(S):
            c = 0 if cuts is None else int(cuts[f][s])
            if c & 2:
                ref.forget(s)
            pushed = push is None or bool(push[f])
            d, l, i, state, m = ref.step(s, pushed, dets_in[f][s], lms_in[f][s], info_in[f][s], counts_in[f][s],
                                         None if cuts is None else (CUT if c & 1 else SAME), lumas[f * S + s])
            k = len(d)
            od[f, s, :k], ol[f, s, :k], oi[f, s, :k], om[f, s, :k], oc[f, s], st[f, s] = d, l, i, m, k, state
    return od, ol, oi, oc, st, om


# ---------------------------------------------------------------------------------------------- scenes
def shifted(box, tx, ty):
    return (box[0] + tx, box[1] + ty, box[2] + tx, box[3] + ty)


def moving_frames(seed, fmt, h, w, shifts, S=1, pads=(0, 0), smooth=4):
    """frames[f * S + s]: stream s sees its own texture moved by shifts[f] (every stream by the same amount), as plane tuples."""
    rng = np.random.default_rng(seed)
    margin = 8 + max(max(abs(tx), abs(ty)) for tx, ty in shifts)
    cvs = [canvas(rng, fmt, h, w, margin, smooth) for _ in range(S)]
    return [planes_of(rng, fmt, view(cvs[s], h, w, margin, tx, ty), *pads) for tx, ty in shifts for s in range(S)]


def lumas_of(frames, fmt):
    return [luma_of(pl, fmt) for pl in frames]


def planted(seed, fmt, hw, F, move, births, depth, pads=(0, 0), smooth=4):
    """A canvas that moves by ``move`` = (tx, ty) pixels per frame under an h x w window, and tracks that move with it: births = a list of
    (frame of birth, box in that frame); id k + 1 is the k-th birth (births sorted by frame), present from its birth on.  Then ``depth``
    drains.  Returns (tabs = dets_in, lms_in, info_in, counts_in, push; frames; per-frame rows)."""
    from lookback_cases import tracked_tables
    h, w = hw
    shifts = [(move[0] * f, move[1] * f) for f in range(F)] + [(0, 0)] * depth
    frames = moving_frames(seed, fmt, h, w, shifts, pads=pads, smooth=smooth)
    rows = [[[(k + 1, shifted(box, move[0] * (f - fb), move[1] * (f - fb))) for k, (fb, box) in enumerate(births) if fb <= f]] for f in range(F)]
    d, l, i, c = tracked_tables(rows + [[[]]] * depth, max(len(births), 1))
    push = np.array([1] * F + [0] * depth, np.uint8)
    return (d, l, i, c, push), frames, rows


# The hand-checked case and the planted-move scenes: 64 x 96 frames, rows in a 64 x 96 network space (fx = fy = 1).  The face is 32
# pixels wide (c = 2); the canvas moves by (+4, -2) per frame, two cells right and one up.
HW = (64, 96)
HAND_BOX = (30.5, 16.25, 62.5, 48.25)
HAND_MOVE = (4, -2)
# (seed, format, move, box): moves are multiples of c with |move| <= R * c = 8 per axis; the template and every true match lie inside the frame
PLANTED = ((11, "nv12", (4, -2), HAND_BOX), (12, "bgr", (-6, 4), (40.0, 14.0, 72.0, 44.0)), (13, "i420", (2, 8), (20.25, 30.5, 50.25, 62.25)),
           (14, "yv12", (-8, -2), (40.0, 24.0, 71.5, 56.0)))
