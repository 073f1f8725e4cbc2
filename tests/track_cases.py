"""The tracker's update (include/centerface_hip.h, csrc/cf_track.hip) restated in numpy, and the scenarios the tests run through it.

The arithmetic is the statement's: the "+1" IoU with every operation rounded to float32 (numpy float32 scalars, one Python loop over the
slots, nothing vectorised), the growth of a held box in float64 (Python floats) in the stated order, `>=` against the float32
threshold.  A NaN measure never wins because `v > best` is false for it."""
import numpy as np

F32 = np.float32
ONE, ZERO = F32(1.0), F32(0.0)
DEFAULTS = dict(iou=0.3, max_age=15, min_hits=2, max_tracks=256, hold_grow=0.0)


def iou32(t, d):
    """float32 "+1" IoU of two boxes (x1, y1, x2, y2), the decode's arithmetic."""
    t = [F32(v) for v in t]
    d = [F32(v) for v in d]
    with np.errstate(all="ignore"):
        at = (t[2] - t[0] + ONE) * (t[3] - t[1] + ONE)
        ad = (d[2] - d[0] + ONE) * (d[3] - d[1] + ONE)
        w = max(ZERO, min(t[2], d[2]) - max(t[0], d[0]) + ONE)
        h = max(ZERO, min(t[3], d[3]) - max(t[1], d[1]) + ONE)
        inter = F32(w * h)
        return F32(inter / F32(F32(at + ad) - inter))


def grown(box, hold_grow, misses):
    """The output box of a slot: bit for bit with misses == 0, else grown about its centre in float64."""
    if misses <= 0:
        return [F32(v) for v in box]
    x1, y1, x2, y2 = (float(F32(v)) for v in box)
    g = 1.0 + float(F32(hold_grow)) * float(misses)
    cx, hw = (x1 + x2) * 0.5, (x2 - x1) * 0.5 * g
    cy, hh = (y1 + y2) * 0.5, (y2 - y1) * 0.5 * g
    with np.errstate(all="ignore"):
        return [F32(cx - hw), F32(cy - hh), F32(cx + hw), F32(cy + hh)]


class Slot(object):
    __slots__ = ("alive", "id", "hits", "misses", "box", "score", "lms")

    def __init__(self):
        self.alive, self.id, self.hits, self.misses = False, 0, 0, 0
        self.box, self.score, self.lms = None, None, None


class RefTracker(object):
    """n_streams independent streams of max_tracks slots; next_id starts at 1 and is never reused."""

    def __init__(self, n_streams, iou=0.3, max_age=15, min_hits=2, max_tracks=256, hold_grow=0.0):
        self.S, self.iou, self.max_age, self.min_hits, self.M, self.hold_grow = n_streams, F32(iou), int(max_age), int(min_hits), int(max_tracks), F32(hold_grow)
        self.slots = [[Slot() for _ in range(self.M)] for _ in range(n_streams)]
        self.next_id = [1] * n_streams

    def reset(self, stream=-1):
        for s in (range(self.S) if stream < 0 else (stream,)):
            for sl in self.slots[s]:
                sl.alive = False

    def update(self, s, boxes, scores, lms, count):
        """One frame of stream s: rows i < min(count, len(boxes)).  Returns (dets [k,5], lms [k,10], info [k,3] int32, flag)."""
        slots = self.slots[s]
        boxes = np.asarray(boxes, F32).reshape(-1, 4)
        scores = np.asarray(scores, F32).reshape(-1)
        lms = np.asarray(lms, F32).reshape(-1, 10)
        n = min(max(int(count), 0), len(boxes))
        start = [sl.alive for sl in slots]
        start_box = [list(sl.box) if sl.alive else None for sl in slots]
        matched = [False] * self.M
        new = []
        for i in range(n):
            d = boxes[i]
            if not np.all(np.isfinite(d)):
                continue                                             # 1. skipped
            best, best_v = -1, F32(-np.inf)
            for k in range(self.M):                                  # 2. ascending slots, strictly greater: ties go to the lowest
                if not start[k] or matched[k]:
                    continue
                v = iou32(start_box[k], d)
                if v > best_v:
                    best, best_v = k, v
            if best >= 0 and best_v >= self.iou:
                sl = slots[best]
                matched[best] = True
                sl.box, sl.score, sl.lms = d.copy(), scores[i], lms[i].copy()
                sl.hits, sl.misses = min(sl.hits + 1, 1 << 30), 0
            else:
                new.append(i)
        for k, sl in enumerate(slots):                               # 3. age
            if start[k] and not matched[k]:
                if sl.hits < self.min_hits:
                    sl.alive = False
                else:
                    sl.misses += 1
                    if sl.misses > self.max_age:
                        sl.alive = False
        flag = 0
        free = [k for k, sl in enumerate(slots) if not sl.alive]
        for r, i in enumerate(new):                                  # 4. birth
            if r >= len(free):
                flag = 1
                break
            sl = slots[free[r]]
            sl.alive, sl.id, sl.hits, sl.misses = True, self.next_id[s], 1, 0
            self.next_id[s] += 1
            sl.box, sl.score, sl.lms = boxes[i].copy(), scores[i], lms[i].copy()
        alive = [sl for sl in slots if sl.alive]                      # 5. output
        dets = np.zeros((len(alive), 5), F32)
        olms = np.zeros((len(alive), 10), F32)
        info = np.zeros((len(alive), 3), np.int32)
        for k, sl in enumerate(alive):
            dets[k, :4] = grown(sl.box, self.hold_grow, sl.misses)
            dets[k, 4] = sl.score
            olms[k] = sl.lms
            info[k] = (sl.id, sl.hits, sl.misses)
        return dets, olms, info, flag


def run_sequence(boxes, scores, lms, counts, dets0=None, lms0=None, info0=None, resets=(), **opts):
    """The tables ``ops.track_sequence`` returns, from the restatement: boxes [F, S, rows, 4], scores [F, S, rows], lms [F, S, rows, 10],
    counts [F, S]; rows at and past a count keep the bytes of dets0 / lms0 / info0 (zeros by default).  ``resets``: (frame, stream)
    pairs -- a reset of that stream (-1: all) before that frame."""
    o = dict(DEFAULTS, **opts)
    boxes = np.asarray(boxes, F32)
    F, S, rows, _ = boxes.shape
    M = o["max_tracks"]
    dets = np.zeros((F, S, M, 5), F32) if dets0 is None else np.array(dets0, F32).reshape(F, S, M, 5)
    olms = np.zeros((F, S, M, 10), F32) if lms0 is None else np.array(lms0, F32).reshape(F, S, M, 10)
    info = np.zeros((F, S, M, 3), np.int32) if info0 is None else np.array(info0, np.int32).reshape(F, S, M, 3)
    cnt, flags = np.zeros((F, S), np.int32), np.zeros((F, S), np.int32)
    trk = RefTracker(S, **o)
    for f in range(F):
        for rf, rs in resets:
            if rf == f:
                trk.reset(rs)
        for s in range(S):
            d, l, i, fl = trk.update(s, boxes[f, s], np.asarray(scores, F32)[f, s], np.asarray(lms, F32)[f, s], np.asarray(counts)[f, s])
            k = len(d)
            dets[f, s, :k], olms[f, s, :k], info[f, s, :k], cnt[f, s], flags[f, s] = d, l, i, k, fl
    return dets, olms, info, cnt, flags


# ---------------------------------------------------------------------------------------------- scenario builders
def tables(frames, rows, S=1):
    """frames[f][s] = list of (x1, y1, x2, y2[, score]) -> (boxes, scores, lms, counts) tables of `rows` rows; a row's landmarks are
    derived from its box and the frame (so that "last seen" shows), rows past the count hold a sentinel that must never be read."""
    F = len(frames)
    boxes = np.full((F, S, rows, 4), 7777.0, F32)
    scores = np.full((F, S, rows), -5.0, F32)
    lms = np.full((F, S, rows, 10), -3333.0, F32)
    counts = np.zeros((F, S), np.int32)
    for f, per in enumerate(frames):
        for s, faces in enumerate(per):
            counts[f, s] = len(faces)
            for i, face in enumerate(faces[:rows]):
                boxes[f, s, i] = face[:4]
                scores[f, s, i] = face[4] if len(face) > 4 else 0.5 + 0.001 * i + 0.01 * f
                with np.errstate(all="ignore"):
                    lms[f, s, i] = np.nan_to_num(np.resize(np.asarray(face[:4], F32), 10), nan=0.0, posinf=0.0, neginf=0.0) + F32(0.25 * f) + np.arange(10, dtype=F32)
    return boxes, scores, lms, counts


def grid_faces(n, size=20.0, gap=12.0, per_row=16, dx=0.0, dy=0.0):
    """n well-separated boxes of `size` on a grid, shifted by (dx, dy)."""
    out = []
    for i in range(n):
        x, y = (i % per_row) * (size + gap) + dx, (i // per_row) * (size + gap) + dy
        out.append((x, y, x + size, y + size))
    return out


def random_sequence(seed, S=3, F=12, max_faces=40, rows=48):
    """Jittered faces on a coarse integer lattice (so that equal IoUs -- ties -- and exact duplicates occur), some dropped per frame, some
    frames empty, a count above `rows` now and then."""
    rng = np.random.default_rng(seed)
    frames = []
    base = [[(int(x) * 8, int(y) * 8, int(x) * 8 + int(w), int(y) * 8 + int(w)) for x, y, w in
             zip(rng.integers(0, 24, max_faces), rng.integers(0, 16, max_faces), rng.choice([15, 23, 31], max_faces))] for _ in range(S)]
    for f in range(F):
        per = []
        for s in range(S):
            faces = []
            for (x1, y1, x2, y2) in base[s]:
                if rng.random() < 0.25:
                    continue                                            # a dropout
                j = rng.integers(-1, 2, 4) * rng.choice([0, 4])         # lattice jitter: many exact repeats
                faces.append((x1 + j[0], y1 + j[1], x2 + j[2], y2 + j[3]))
                if rng.random() < 0.1:
                    faces.append(faces[-1])                             # an exact duplicate row
            if rng.random() < 0.1:
                faces = []
            order = rng.permutation(len(faces))
            per.append([faces[k] for k in order])
        frames.append(per)
    boxes, scores, lms, counts = tables(frames, rows, S)
    return boxes, scores, lms, counts
