"""The tracker's update with constant-velocity prediction (include/centerface_hip.h "constant velocity", csrc/cf_track.hip) restated in
numpy on top of tests/track_cases.py, tests/weak_cases.py and tests/follow_cases.py, and the scenarios the tests run through it.

Per slot vel = (vx, vy), numpy float32 scalars.  The rows are matched against P = the stored box + vel (one rounded float32 addition per
corner); a winner's velocity is updated from the stored box, misses and hits BEFORE the take; a held slot coasts (box and landmarks by
vel, vel by damp) or is freed when a coasted corner passes 2^24; a birth zeroes vel.  Rows with a corner beyond 2^24 are skipped like
the non-finite ones.  The float32 discipline is track_cases.iou32's: numpy float32 scalars, one operation per line, nothing vectorised."""
import numpy as np

from follow_cases import RefFollower
from track_cases import DEFAULTS, F32, ONE, ZERO, grid_faces, grown, iou32, tables
from weak_cases import WeakRefTracker

HALF = F32(0.5)
FAR = F32(16777216.0)                                                     # 2^24
MOTION_DEFAULTS = dict(gain=0.5, damp=1.0)


def far(box):
    """A corner of magnitude above 2^24."""
    return any(abs(F32(v)) > FAR for v in box)


def learn(v, d1, d2, o1, o2, g, hb, gain):
    """One component of the velocity behind a match: row corners d1, d2, stored corners o1, o2, g = misses and hb = hits before the take."""
    sd = F32(F32(d1) + F32(d2))
    cd = F32(sd * HALF)
    so = F32(F32(o1) + F32(o2))
    co = F32(so * HALF)
    disp = F32(cd - co)
    r = F32(disp - v)
    a = ONE if hb == 1 else gain
    n = F32(g + 1)
    q = F32(r / n)
    step = F32(a * q)
    return F32(v + step)


def motion_update(self, s, boxes, scores, lms, count):
    """One frame of stream s of a tracker with velocities: plain when ``self.birth`` is None, else with two thresholds.  Returns (dets
    [k,5], lms [k,10], info [k,3] int32, flags) and leaves the velocities of the output rows in ``self.out_vel`` [k,2]."""
    slots, vel = self.slots[s], self.vel[s]
    fol = self.fol[s] if getattr(self, "fol", None) is not None else None
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    scores = np.asarray(scores, F32).reshape(-1)
    lms = np.asarray(lms, F32).reshape(-1, 10)
    n = min(max(int(count), 0), len(boxes))
    weak = self.birth is not None
    start = [sl.alive for sl in slots]
    confirmed = [sl.alive and sl.hits >= self.min_hits for sl in slots]                # when the update began
    pred = [None] * self.M                                                           # P
    for k, sl in enumerate(slots):
        if sl.alive:
            vx, vy = vel[k]
            pred[k] = [F32(F32(sl.box[0]) + vx), F32(F32(sl.box[1]) + vy), F32(F32(sl.box[2]) + vx), F32(F32(sl.box[3]) + vy)]
    matched = [False] * self.M
    ok = [bool(np.all(np.isfinite(boxes[i]))) and not far(boxes[i]) for i in range(n)]   # 1'. skipped
    strong = [bool(scores[i] > self.birth) if weak else True for i in range(n)]

    def best_of(eligible, d):
        best, best_v = -1, F32(-np.inf)
        for k in range(self.M):                                                      # ascending, strictly greater: ties go to the lowest
            if not eligible[k]:
                continue
            v = iou32(pred[k], d)
            if v > best_v:
                best, best_v = k, v
        return best, best_v

    def take(k, i):
        sl, d = slots[k], boxes[i]
        o, g, hb = sl.box, sl.misses, sl.hits                                        # before the take
        vx, vy = vel[k]
        vel[k] = [learn(vx, d[0], d[2], o[0], o[2], g, hb, self.gain), learn(vy, d[1], d[3], o[1], o[3], g, hb, self.gain)]
        matched[k] = True
        sl.box, sl.score, sl.lms = d.copy(), scores[i], lms[i].copy()
        sl.hits, sl.misses = min(sl.hits + 1, 1 << 30), 0

    new, weak_hit = [], False
    for i in range(n):                                                               # 2' / 2a'
        if not ok[i] or not strong[i]:
            continue
        best, v = best_of([start[k] and not matched[k] for k in range(self.M)], boxes[i])
        if best >= 0 and v >= self.iou:
            take(best, i)
        else:
            new.append(i)
    if weak:
        for i in range(n):                                                           # 2b'
            if not ok[i] or strong[i]:
                continue
            best, v = best_of([confirmed[k] and not matched[k] for k in range(self.M)], boxes[i])
            if best >= 0 and v >= self.weak_iou:
                take(best, i)
                weak_hit = True
    for k, sl in enumerate(slots):                                                   # 3'. age, and coast what is held
        if not start[k] or matched[k]:
            continue
        if sl.hits < self.min_hits:
            sl.alive = False
            continue
        sl.misses += 1
        if sl.misses > self.max_age:
            sl.alive = False
            continue
        vx, vy = vel[k]
        before = np.asarray(sl.box, F32)
        coasted = np.array([F32(before[0] + vx), F32(before[1] + vy), F32(before[2] + vx), F32(before[3] + vy)], F32)
        if far(coasted):
            sl.alive = False
            continue
        sl.box = coasted
        sl.lms = np.array([F32(F32(v) + (vy if q & 1 else vx)) for q, v in enumerate(sl.lms)], F32)
        vel[k] = [F32(vx * self.damp), F32(vy * self.damp)]
        if fol is not None and fol[k].id == sl.id and fol[k].box == before.tobytes():
            fol[k].box = coasted.tobytes()                                           # the next follow FOLLOWS from the coasted place
    flag = 2 if weak_hit else 0
    free = [k for k, sl in enumerate(slots) if not sl.alive]
    for r, i in enumerate(new):                                                      # 4'. birth
        if r >= len(free):
            flag |= 1
            break
        k = free[r]
        sl = slots[k]
        sl.alive, sl.id, sl.hits, sl.misses = True, self.next_id[s], 1, 0
        self.next_id[s] += 1
        sl.box, sl.score, sl.lms = boxes[i].copy(), scores[i], lms[i].copy()
        vel[k] = [ZERO, ZERO]
    alive = [k for k, sl in enumerate(slots) if sl.alive]                            # 5. output
    dets = np.zeros((len(alive), 5), F32)
    olms = np.zeros((len(alive), 10), F32)
    info = np.zeros((len(alive), 3), np.int32)
    self.out_vel = np.zeros((len(alive), 2), F32)
    for r, k in enumerate(alive):
        sl = slots[k]
        dets[r, :4] = grown(sl.box, self.hold_grow, sl.misses)
        dets[r, 4] = sl.score
        olms[r] = sl.lms
        info[r] = (sl.id, sl.hits, sl.misses)
        self.out_vel[r] = vel[k]
    return dets, olms, info, flag


def _init_motion(self, gain, damp):
    self.gain, self.damp = F32(gain), F32(damp)
    self.vel = [[[ZERO, ZERO] for _ in range(self.M)] for _ in range(self.S)]
    self.out_vel = np.zeros((0, 2), F32)


class MotionRefTracker(WeakRefTracker):
    """WeakRefTracker (``birth_score=None``: track_cases.RefTracker's single pass) with velocities."""

    def __init__(self, n_streams, gain=0.5, damp=1.0, birth_score=None, weak_iou=0.5, **opts):
        WeakRefTracker.__init__(self, n_streams, 0.3 if birth_score is None else birth_score, weak_iou, **opts)
        if birth_score is None:
            self.birth = None
        _init_motion(self, gain, damp)

    update = motion_update


class MotionRefFollower(RefFollower):
    """follow_cases.RefFollower whose updates are the motion tracker's: a coast takes the follower record's tpl_box along."""

    birth = None

    def __init__(self, n_streams, space_hw, gain=0.5, damp=1.0, **opts):
        RefFollower.__init__(self, n_streams, space_hw, **opts)
        _init_motion(self, gain, damp)

    update = motion_update


def motion_of(motion):
    """The ``motion=`` argument of the ops -> the two numbers."""
    return dict(MOTION_DEFAULTS, **(motion if isinstance(motion, dict) else {}))


def run_motion_sequence(boxes, scores, lms, counts, motion=True, birth_score=None, weak_iou=0.5, dets0=None, lms0=None, info0=None, vel0=None, **opts):
    """The tables ``ops.track_sequence(..., motion=, vel=True)`` returns, from the restatement (as track_cases.run_sequence), the
    velocities [F, S, max_tracks, 2] last."""
    o = dict(DEFAULTS, **opts)
    boxes = np.asarray(boxes, F32)
    F, S, rows, _ = boxes.shape
    M = o["max_tracks"]
    dets = np.zeros((F, S, M, 5), F32) if dets0 is None else np.array(dets0, F32).reshape(F, S, M, 5)
    olms = np.zeros((F, S, M, 10), F32) if lms0 is None else np.array(lms0, F32).reshape(F, S, M, 10)
    info = np.zeros((F, S, M, 3), np.int32) if info0 is None else np.array(info0, np.int32).reshape(F, S, M, 3)
    vel = np.zeros((F, S, M, 2), F32) if vel0 is None else np.array(vel0, F32).reshape(F, S, M, 2)
    cnt, flags = np.zeros((F, S), np.int32), np.zeros((F, S), np.int32)
    trk = MotionRefTracker(S, birth_score=birth_score, weak_iou=weak_iou, **dict(o, **motion_of(motion)))
    for f in range(F):
        for s in range(S):
            d, l, i, fl = trk.update(s, boxes[f, s], np.asarray(scores, F32)[f, s], np.asarray(lms, F32)[f, s], np.asarray(counts)[f, s])
            k = len(d)
            dets[f, s, :k], olms[f, s, :k], info[f, s, :k], vel[f, s, :k], cnt[f, s], flags[f, s] = d, l, i, trk.out_vel, k, fl
    return dets, olms, info, cnt, flags, vel


def run_motion_follow(boxes, scores, lms, counts, lumas, space_hw, motion=True, detect=None, tiled=False, search=4, max_sad=4096, **opts):
    """The tables ``ops.follow_sequence(..., motion=)`` returns, from the restatement (as follow_cases.run_follow, zeros behind the counts)."""
    o = dict(DEFAULTS, **opts)
    boxes = np.asarray(boxes, F32)
    F, S, rows, _ = boxes.shape
    M = o["max_tracks"]
    detect = np.ones(F, bool) if detect is None else np.asarray(detect).astype(bool)
    dets, olms, info = np.zeros((F, S, M, 5), F32), np.zeros((F, S, M, 10), F32), np.zeros((F, S, M, 3), np.int32)
    moves = np.zeros((F, S, M, 4), np.int32)
    cnt, flags = np.zeros((F, S), np.int32), np.zeros((F, S), np.int32)
    trk = MotionRefFollower(S, space_hw, tiled=tiled, search=search, max_sad=max_sad, **dict(o, **motion_of(motion)))
    for f in range(F):
        for s in range(S):
            if detect[f]:
                d, l, i, fl = trk.update(s, boxes[f, s], np.asarray(scores, F32)[f, s], np.asarray(lms, F32)[f, s], np.asarray(counts)[f, s])
                k = len(d)
                dets[f, s, :k], olms[f, s, :k], info[f, s, :k], flags[f, s] = d, l, i, fl
            d, l, i, m = trk.follow(s, lumas[f * S + s])
            k = len(d)
            dets[f, s, :k], olms[f, s, :k], info[f, s, :k], moves[f, s, :k], cnt[f, s] = d, l, i, m, k
    return dets, olms, info, cnt, flags, moves


# ---------------------------------------------------------------------------------------------- scenario builders
A = (1000, 1000, 1040, 1050)                                              # 41 x 51, "+1" area 2091


def shifted(box, dx, dy=0.0):
    return (box[0] + dx, box[1] + dy, box[2] + dx, box[3] + dy)


def crowded(frames, pad, score=0.9):
    """Every frame of a one-stream scenario (a list of face lists) behind a static crowd of ``pad`` faces on track_cases' grid, far from
    A: the crowd is born first and fills the slots 0 .. pad - 1, so the faces of the scenario live in the slots from ``pad`` on."""
    front = [tuple(f) + (score,) for f in grid_faces(pad)]
    return [[front + list(faces)] for faces in frames]


def drifting_sequence(seed, S=3, F=12, max_faces=40, rows=48):
    """track_cases.random_sequence's kind of tables with faces that MOVE: every face has its own drift per frame (some zero, some
    fractional, some fast), a little jitter, dropouts, empty frames, and scores on both sides of 0.3.  Returns (boxes, scores, lms, counts)."""
    rng = np.random.default_rng(seed)
    frames = []
    base = []
    for s in range(S):
        per = []
        for _ in range(max_faces):
            x, y, w = float(rng.integers(0, 40)) * 24.0, float(rng.integers(0, 24)) * 24.0, float(rng.choice([15, 23, 31]))
            dx, dy = rng.choice([0.0, 0.0, 1.5, -2.25, 4.0, -6.0, 9.0]), rng.choice([0.0, 0.0, 0.75, -1.5, 3.0, 5.0])
            per.append((x, y, w, float(dx), float(dy)))
        base.append(per)
    for f in range(F):
        per = []
        for s in range(S):
            faces = []
            for (x, y, w, dx, dy) in base[s]:
                if rng.random() < 0.25:
                    continue                                            # a dropout
                jx, jy = float(rng.integers(-1, 2)) * float(rng.choice([0.0, 0.5, 1.0])), float(rng.integers(-1, 2)) * float(rng.choice([0.0, 0.5]))
                x1, y1 = x + dx * f + jx, y + dy * f + jy
                faces.append((x1, y1, x1 + w, y1 + w, float(rng.choice([0.1, 0.29, 0.3, 0.31, 0.6, 0.9]))))
            if rng.random() < 0.1:
                faces = []
            order = rng.permutation(len(faces))
            per.append([faces[k] for k in order])
        frames.append(per)
    return tables(frames, rows, S)


__all__ = ["MotionRefTracker", "MotionRefFollower", "run_motion_sequence", "run_motion_follow", "motion_update", "learn", "far", "A", "shifted",
           "crowded", "drifting_sequence", "MOTION_DEFAULTS", "FAR"]
