"""The tracker's update with two thresholds (include/centerface_hip.h "two thresholds", csrc/cf_track.hip) restated in numpy on top of
tests/track_cases.py, and the scenarios the tests run through it.

A row is STRONG when ``score > birth_score`` (numpy float32 scalars, strict: a NaN score and a score equal to the threshold are weak).
The strong pass is track_cases' step 2 over the strong rows; the weak pass runs behind it over the weak rows, among the slots that
were alive and had ``hits >= min_hits`` when the update began and that neither pass has matched yet; a winner with ``iou >= weak_iou``
takes the row as a strong match does, any other weak row is discarded.  Steps 3 to 5 are track_cases'.  Flag bit 1: a weak row matched.
The arithmetic keeps that file's float32 discipline (``iou32``, one Python loop over the slots, `v > best` never true for a NaN)."""
import numpy as np

from track_cases import DEFAULTS, F32, RefTracker, grid_faces, grown, iou32, tables

WEAK_DEFAULTS = dict(birth_score=0.3, weak_iou=0.5)


class WeakRefTracker(RefTracker):
    def __init__(self, n_streams, birth_score=0.3, weak_iou=0.5, **opts):
        RefTracker.__init__(self, n_streams, **opts)
        self.birth, self.weak_iou = F32(birth_score), F32(weak_iou)

    def _best(self, start_box, eligible, d):
        """(slot, measure) of the arg-max over the eligible slots in ascending order: strictly greater, so ties go to the lowest."""
        best, best_v = -1, F32(-np.inf)
        for k in range(self.M):
            if not eligible[k]:
                continue
            v = iou32(start_box[k], d)
            if v > best_v:
                best, best_v = k, v
        return best, best_v

    def update(self, s, boxes, scores, lms, count):
        """One frame of stream s.  Returns (dets [k,5], lms [k,10], info [k,3] int32, flags): bit 0 a new row was dropped, bit 1 a weak
        row matched."""
        slots = self.slots[s]
        boxes = np.asarray(boxes, F32).reshape(-1, 4)
        scores = np.asarray(scores, F32).reshape(-1)
        lms = np.asarray(lms, F32).reshape(-1, 10)
        n = min(max(int(count), 0), len(boxes))
        start = [sl.alive for sl in slots]
        confirmed = [sl.alive and sl.hits >= self.min_hits for sl in slots]          # when the update began
        start_box = [list(sl.box) if sl.alive else None for sl in slots]
        matched = [False] * self.M
        finite = [bool(np.all(np.isfinite(boxes[i]))) for i in range(n)]             # 1. skipped, strong or weak
        strong = [bool(scores[i] > self.birth) for i in range(n)]                    # float32, strict; False for a NaN

        def take(k, i):
            sl = slots[k]
            matched[k] = True
            sl.box, sl.score, sl.lms = boxes[i].copy(), scores[i], lms[i].copy()
            sl.hits, sl.misses = min(sl.hits + 1, 1 << 30), 0

        new, weak_hit = [], False
        for i in range(n):                                                           # 2a. the strong pass
            if not finite[i] or not strong[i]:
                continue
            best, v = self._best(start_box, [start[k] and not matched[k] for k in range(self.M)], boxes[i])
            if best >= 0 and v >= self.iou:
                take(best, i)
            else:
                new.append(i)
        for i in range(n):                                                           # 2b. the weak pass, behind every strong row
            if not finite[i] or strong[i]:
                continue
            best, v = self._best(start_box, [confirmed[k] and not matched[k] for k in range(self.M)], boxes[i])
            if best >= 0 and v >= self.weak_iou:
                take(best, i)
                weak_hit = True                                                      # (otherwise discarded: never new)
        for k, sl in enumerate(slots):                                               # 3. age
            if start[k] and not matched[k]:
                if sl.hits < self.min_hits:
                    sl.alive = False
                else:
                    sl.misses += 1
                    if sl.misses > self.max_age:
                        sl.alive = False
        flag = 2 if weak_hit else 0
        free = [k for k, sl in enumerate(slots) if not sl.alive]
        for r, i in enumerate(new):                                                  # 4. birth
            if r >= len(free):
                flag |= 1
                break
            sl = slots[free[r]]
            sl.alive, sl.id, sl.hits, sl.misses = True, self.next_id[s], 1, 0
            self.next_id[s] += 1
            sl.box, sl.score, sl.lms = boxes[i].copy(), scores[i], lms[i].copy()
        alive = [sl for sl in slots if sl.alive]                                     # 5. output
        dets = np.zeros((len(alive), 5), F32)
        olms = np.zeros((len(alive), 10), F32)
        info = np.zeros((len(alive), 3), np.int32)
        for k, sl in enumerate(alive):
            dets[k, :4] = grown(sl.box, self.hold_grow, sl.misses)
            dets[k, 4] = sl.score
            olms[k] = sl.lms
            info[k] = (sl.id, sl.hits, sl.misses)
        return dets, olms, info, flag


def run_weak_sequence(boxes, scores, lms, counts, dets0=None, lms0=None, info0=None, birth_score=0.3, weak_iou=0.5, **opts):
    """The tables ``ops.track_sequence(..., birth_score=, weak_iou=)`` returns, from the restatement (as track_cases.run_sequence)."""
    o = dict(DEFAULTS, **opts)
    boxes = np.asarray(boxes, F32)
    F, S, rows, _ = boxes.shape
    M = o["max_tracks"]
    dets = np.zeros((F, S, M, 5), F32) if dets0 is None else np.array(dets0, F32).reshape(F, S, M, 5)
    olms = np.zeros((F, S, M, 10), F32) if lms0 is None else np.array(lms0, F32).reshape(F, S, M, 10)
    info = np.zeros((F, S, M, 3), np.int32) if info0 is None else np.array(info0, np.int32).reshape(F, S, M, 3)
    cnt, flags = np.zeros((F, S), np.int32), np.zeros((F, S), np.int32)
    trk = WeakRefTracker(S, birth_score, weak_iou, **o)
    for f in range(F):
        for s in range(S):
            d, l, i, fl = trk.update(s, boxes[f, s], np.asarray(scores, F32)[f, s], np.asarray(lms, F32)[f, s], np.asarray(counts)[f, s])
            k = len(d)
            dets[f, s, :k], olms[f, s, :k], info[f, s, :k], cnt[f, s], flags[f, s] = d, l, i, k, fl
    return dets, olms, info, cnt, flags


# ---------------------------------------------------------------------------------------------- scenario builders
STRONG, WEAK = 0.8, 0.2                                                   # on either side of birth_score = 0.3
# A, A2, A3: 41 x 51 boxes ("+1" area 2091), each shifted by (6, 4) from the one before: IoU(A, A2) = IoU(A2, A3) = 1645 / 2537 = 0.648,
# IoU(A, A3) = 1247 / 2935 = 0.425 -- a weak match at 0.5 between neighbours, a strong match at 0.3 even two steps apart
A, A2, A3 = (1000, 1000, 1040, 1050), (1006, 1004, 1046, 1054), (1012, 1008, 1052, 1058)
FAR = (3000, 3000, 3040, 3050)


def at(box, score):
    return tuple(box) + (score,)


def crowd(n, dx=0.0, dy=0.0, score=0.9):
    """n strong faces on track_cases' grid (far from A and FAR): they fill the slots 0 .. n - 1 so that the face of a scenario lives in
    slot n -- beyond a 64-lane boundary when n says so."""
    return [at(f, score) for f in grid_faces(n, dx=dx, dy=dy)]


def pad_for(M):
    """The crowd in front of a one-face scenario in a tracker of M slots: the face takes the last slot, 70 rows at the most."""
    return min(M - 1, 69)


def mixed_random_sequence(seed, S=2, F=8, max_faces=60, rows=70):
    """track_cases.random_sequence's lattice faces with scores drawn from both sides of the threshold, the threshold itself, the next
    float32 above it and NaN.  Returns (boxes, scores, lms, counts)."""
    from track_cases import random_sequence
    b, s, l, c = random_sequence(seed, S=S, F=F, max_faces=max_faces, rows=rows)
    rng = np.random.default_rng(1000 + seed)
    pool = np.array([0.05, 0.2, 0.29, 0.3, np.nextafter(F32(0.3), F32(1)), 0.31, 0.6, 0.9, np.nan], F32)
    s = pool[rng.choice(len(pool), s.shape, p=[0.1, 0.15, 0.1, 0.08, 0.07, 0.1, 0.2, 0.15, 0.05])]
    return b, s, l, c


__all__ = ["WeakRefTracker", "run_weak_sequence", "tables", "crowd", "pad_for", "at", "mixed_random_sequence", "A", "A2", "A3", "FAR", "STRONG", "WEAK",
           "WEAK_DEFAULTS"]
