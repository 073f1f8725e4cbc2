"""The lookback statement of include/centerface_hip.h restated in numpy (RefLookback), and the builders of the sequences the tests feed
to it and to the device.  Bit copies and integers, except the growth of a back-filled box: float64 in the order of the tracker's held
rows, one rounding to float32 at the end."""
import numpy as np

SAME, CUT = 1, 2                                                           # CF_SCENE_SAME, CF_SCENE_CUT
DEPTH, ROWS, GROW, CONFIRM = 8, 256, 0.05, 1                               # the defaults of the Python layer


def grown(box, grow, j):
    """The four corners of ``box`` (float32) grown about the centre by 1 + grow * j: float64, in the order of cf_trackemit.h."""
    x1, y1, x2, y2 = (np.float64(v) for v in np.asarray(box, np.float32))
    g = np.float64(1.0) + np.float64(np.float32(grow)) * np.float64(j)
    with np.errstate(all="ignore"):
        cx, hw = (x1 + x2) * 0.5, (x2 - x1) * 0.5 * g
        cy, hh = (y1 + y2) * 0.5, (y2 - y1) * 0.5 * g
        return np.array([cx - hw, cy - hh, cx + hw, cy + hh], np.float64).astype(np.float32)


class _Entry(object):
    def __init__(self, seq, cut, dets, lms, info, born):
        self.seq, self.cut, self.dets, self.lms, self.info, self.born = seq, cut, dets, lms, info, born

    @property
    def n(self):
        return len(self.dets)


class RefLookback(object):
    """n_streams independent streams; ``step`` is one step of one stream."""

    def __init__(self, streams, depth=DEPTH, rows=ROWS, grow=GROW, confirm=CONFIRM):
        self.depth, self.rows, self.grow, self.confirm = int(depth), int(rows), np.float32(grow), int(confirm)
        self.queue = [[] for _ in range(streams)]
        self.max_id, self.seq_next, self.pending = [0] * streams, [0] * streams, [0] * streams

    def forget(self, stream=-1):
        for s in (range(len(self.queue)) if stream < 0 else (stream,)):
            self.pending[s] = 1

    def step(self, s, push=True, dets=None, lms=None, info=None, count=0, code=None):
        """dets [stride, 5], lms [stride, 10], info [stride, 3] of the pushed image, ``count`` as the tracker left it, ``code`` the scene
        code of the frame or None.  Returns (dets [k, 5], lms [k, 10], info [k, 3], state [4])."""
        q = self.queue[s]
        if push:
            n = min(max(int(count), 0), len(dets), self.rows)
            ids = np.asarray(info[:n, 0], np.int32)
            cut = bool(self.pending[s]) or (code is not None and int(code) != SAME)
            self.pending[s] = 0
            q.append(_Entry(self.seq_next[s], cut, np.array(dets[:n], np.float32), np.array(lms[:n], np.float32), np.array(info[:n], np.int32),
                            ids > self.max_id[s]))
            self.seq_next[s] += 1
            if n:
                self.max_id[s] = max(self.max_id[s], int(ids.max()))
        if not (len(q) == self.depth + 1 if push else len(q) > 0):
            return np.zeros((0, 5), np.float32), np.zeros((0, 10), np.float32), np.zeros((0, 3), np.int32), np.array([-1, 0, 0, 0], np.int32)
        t = q.pop(0)
        od, ol, oi = [t.dets], [t.lms], [t.info]
        written, flags = t.n, 0
        stop = next((j for j, e in enumerate(q) if e.cut), len(q))         # e_1 .. e_stop of the statement are q[0 .. stop - 1]
        for j0 in range(stop):
            e, j = q[j0], j0 + 1
            for i in range(e.n):
                if not e.born[i] or not np.isfinite(e.dets[i, :4]).all():
                    continue
                seen = sum(1 for later in q[j0:stop] if (later.info[:, 0] == e.info[i, 0]).any())
                if seen < self.confirm:
                    continue
                if written >= self.rows:
                    flags |= 1
                    continue
                row = e.dets[i].copy()
                row[:4] = grown(e.dets[i, :4], self.grow, j)
                od.append(row[None]), ol.append(e.lms[i][None]), oi.append(np.array([[e.info[i, 0], 0, j]], np.int32))
                written += 1
        return np.concatenate(od), np.concatenate(ol), np.concatenate(oi), np.array([t.seq, t.n, written - t.n, flags], np.int32)


def run_lookback(dets_in, lms_in, info_in, counts_in, push=None, cuts=None, dets=None, lms_out=None, info=None, **opts):
    """RefLookback over the tables ``ops.lookback_sequence`` takes; the same return, rows at and past a count keeping the prefill."""
    o = dict(depth=DEPTH, rows=ROWS, grow=GROW, confirm=CONFIRM)
    o.update(opts)
    F, S = np.asarray(counts_in).shape
    R = o["rows"]
    od = np.zeros((F, S, R, 5), np.float32) if dets is None else np.array(dets, np.float32)
    ol = np.zeros((F, S, R, 10), np.float32) if lms_out is None else np.array(lms_out, np.float32)
    oi = np.zeros((F, S, R, 3), np.int32) if info is None else np.array(info, np.int32)
    oc, st = np.zeros((F, S), np.int32), np.zeros((F, S, 4), np.int32)
    ref = RefLookback(S, **o)
    for f in range(F):
        for s in range(S):
            c = 0 if cuts is None else int(cuts[f][s])
            if c & 2:
                ref.forget(s)
            pushed = push is None or bool(push[f])
            d, l, i, state = ref.step(s, pushed, dets_in[f][s], lms_in[f][s], info_in[f][s], counts_in[f][s],
                                      None if cuts is None else (CUT if c & 1 else SAME))
            k = len(d)
            od[f, s, :k], ol[f, s, :k], oi[f, s, :k], oc[f, s], st[f, s] = d, l, i, k, state
    return od, ol, oi, oc, st


def face_box(k, size=20.0):
    """Box k of a lattice of disjoint faces (float32 values that are not round numbers)."""
    x, y = 7.25 + (k % 32) * (size + 5.5), 3.5 + (k // 32) * (size + 4.75)
    return (x, y, x + size, y + size * 1.25)


def tracked_tables(frames, rows_in, S=1):
    """frames[f][s] = a list of (id, box[, hits, misses]) -> dets_in [F,S,rows_in,5], lms_in, info_in, counts_in as a tracker would have
    left them: scores and landmarks derived from the id and the frame, rows past the list filled with a pattern nothing may copy."""
    F = len(frames)
    d = np.full((F, S, rows_in, 5), -7.5, np.float32)
    l = np.full((F, S, rows_in, 10), -3.25, np.float32)
    i = np.full((F, S, rows_in, 3), -5, np.int32)
    c = np.zeros((F, S), np.int32)
    for f, per in enumerate(frames):
        for s, rows in enumerate(per):
            c[f, s] = len(rows)
            for k, row in enumerate(rows[:rows_in]):
                tid, box = row[0], row[1]
                d[f, s, k, :4] = box
                d[f, s, k, 4] = 0.5 + 0.001 * (tid % 400) + 0.0001 * f
                l[f, s, k] = np.arange(10, dtype=np.float32) * 1.5 + tid + 0.125 * f
                i[f, s, k] = (tid, row[2] if len(row) > 2 else 1, row[3] if len(row) > 3 else 0)
    return d, l, i, c


def random_tracked(seed, F=14, S=3, rows_in=16, p_cut=0.2):
    """A seeded sequence of tracked rows: ids rise, tracks live a few frames, some vanish and recur, some rows are held (misses > 0), a
    few corners are not finite; plus cut codes [F, S] with forgets."""
    rng = np.random.default_rng(seed)
    frames, cuts = [], np.zeros((F, S), np.int32)
    nxt, live = [1] * S, [dict() for _ in range(S)]
    for f in range(F):
        per = []
        for s in range(S):
            cuts[f, s] = (1 if rng.random() < p_cut else 0) | (2 if rng.random() < p_cut / 2 else 0)
            for tid in list(live[s]):
                if rng.random() < 0.25:
                    del live[s][tid]
            for _ in range(int(rng.integers(0, 6))):
                if len(live[s]) < rows_in + 3:
                    live[s][nxt[s]] = face_box(int(rng.integers(0, 300)), float(rng.integers(8, 40)))
                    nxt[s] += 1
            rows = []
            for tid in sorted(live[s], key=lambda t: (t * 7) % 11):
                if rng.random() < 0.2:
                    continue                                                # the id is missing in this frame and may recur
                box = live[s][tid]
                if rng.random() < 0.04:
                    box = (box[0], float("nan") if rng.random() < 0.5 else float("inf"), box[2], box[3])
                rows.append((tid, box, int(rng.integers(1, 5)), int(rng.integers(0, 2))))
            per.append(rows)
        frames.append(per)
    return tracked_tables(frames, rows_in, S) + (cuts,)
