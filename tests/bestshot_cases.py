"""Best-shot selection (include/centerface_hip.h "best-shot selection", csrc/cf_bestshot.hip) restated in numpy, line by line, and the
chips, rows and scripted sequences the tests run through it.

Integers are Python integers; the three weights are float64 (Python floats) in the order the header writes them; a float32 value is a
numpy float32 scalar.  Nothing here knows how the device computes."""
import math

import numpy as np

SIZE, POSE, SCORE = 1, 2, 4
FREE, LIVE, DONE = 0, 1, 2
F32 = np.float32
SIZES = (16, 20, 112, 512)


def luma(chip):
    c = np.asarray(chip).astype(np.int64)
    return (29 * c[..., 0] + 150 * c[..., 1] + 77 * c[..., 2] + 128) >> 8


def sharpness(chip):
    """Step 2: the variance of the 4-neighbour Laplacian over the central half, as an integer quotient."""
    S = chip.shape[0]
    L = luma(chip)
    a, b = S // 4, 3 * S // 4
    lap = 4 * L[a:b, a:b] - L[a - 1:b - 1, a:b] - L[a + 1:b + 1, a:b] - L[a:b, a - 1:b - 1] - L[a:b, a + 1:b + 1]
    N = (S // 2) * (S // 2)
    S1, S2 = int(lap.sum()), int((lap * lap).sum())
    V = N * S2 - S1 * S1
    assert V >= 0
    return V // (N * N)


def size_weight(box, fx, fy, S):
    x1, y1, x2, y2 = (float(v) for v in box)
    wx, wy = (x2 - x1) * fx, (y2 - y1) * fy
    if not (wx > 0) or not (wy > 0):
        return 0
    side = wx if wx < wy else wy
    side_i = S if side >= float(S) else int(math.floor(side))
    return side_i * 256 // S


def pose_weight(lms, fx, fy):
    if not all(math.isfinite(float(v)) for v in lms):
        return 0
    P = [(float(lms[2 * j]) * fx, float(lms[2 * j + 1]) * fy) for j in range(5)]
    ex, ey = (P[0][0] + P[1][0]) * 0.5, (P[0][1] + P[1][1]) * 0.5
    mx, my = (P[3][0] + P[4][0]) * 0.5, (P[3][1] + P[4][1]) * 0.5
    ax, ay = mx - ex, my - ey
    dx, dy = P[2][0] - ex, P[2][1] - ey
    cr, len2 = ax * dy - ay * dx, ax * ax + ay * ay
    if not (len2 > 0):
        return 0
    t = abs(cr) / len2 * 512.0
    return 0 if not (t < 256.0) else 256 - int(math.floor(t))


def score_weight(score):
    t = float(score) * 256.0
    return 0 if not (t > 0) else (256 if t >= 256.0 else int(math.floor(t)))


def quality_ref(chip, box, score, lms, fx=1.0, fy=1.0, terms=7):
    """(Q, parts) of one chip and its row."""
    S = chip.shape[0]
    fx, fy = float(fx), float(fy)
    parts = (sharpness(chip), size_weight(box, fx, fy, S) if terms & SIZE else 256, pose_weight(lms, fx, fy) if terms & POSE else 256,
             score_weight(score) if terms & SCORE else 256)
    return parts[0] * parts[1] * parts[2] * parts[3], parts


class Entry(object):
    def __init__(self):
        self.state, self.id, self.Q, self.parts = FREE, 0, 0, (0, 0, 0, 0)
        self.best_t = self.first_t = self.last_t = self.n_offered = self.done_seq = 0
        self.det, self.lms, self.chip = None, None, None

    def record(self):
        p = self.parts
        return [self.id, self.best_t, self.first_t, self.last_t, self.n_offered, p[0], p[1] | p[2] << 10 | p[3] << 20, self.done_seq]


class RefBestShots(object):
    def __init__(self, n_streams, entries=320, min_hits=2, terms=7, fx=1.0, fy=1.0):
        self.E, self.min_hits, self.terms, self.fx, self.fy = int(entries), int(min_hits), int(terms), float(fx), float(fy)
        self.tab = [[Entry() for _ in range(self.E)] for _ in range(n_streams)]
        self.t, self.seq, self.sticky = [0] * n_streams, [0] * n_streams, [0] * n_streams

    def offer(self, s, boxes, scores, lms, info, count, chips, chip_count=None):
        """One offer of stream s: the rows i < min(count, rows) of the tables; the leading ``chip_count`` rows have the chip chips[i]
        (default: as many as ``chips`` holds).  Returns (quality [rows] int64, -1 where no chip of an eligible row; the offer's flags)."""
        rows = len(boxes)
        n = min(max(int(count), 0), rows)
        have = len(chips) if chip_count is None else min(int(chip_count), rows)
        tab, t = self.tab[s], self.t[s]
        counted, seen = [], set()
        for i in range(n):
            tid = int(info[i][0])
            counted.append(tid >= 1 and tid not in seen)
            seen.add(tid)
        present = set(int(info[i][0]) for i in range(n) if counted[i])
        for e in tab:
            if e.state == LIVE:
                if e.id in present:
                    e.last_t = t
                else:
                    e.state, e.done_seq = DONE, self.seq[s]
                    self.seq[s] += 1
        quality, flag = np.full((rows,), -1, np.int64), 0
        for i in range(n):
            tid, hits, misses = (int(v) for v in info[i])
            if not counted[i] or not (misses == 0 and hits >= self.min_hits and i < have):
                continue
            Q, parts = quality_ref(chips[i], boxes[i], scores[i], lms[i], self.fx, self.fy, self.terms)
            quality[i] = Q
            e = next((e for e in tab if e.state == LIVE and e.id == tid), None)
            if e is not None:
                e.n_offered = min(e.n_offered + 1, 1 << 30)
                if not Q > e.Q:
                    continue
            else:
                e = next((e for e in tab if e.state == FREE), None)
                if e is None:
                    flag |= 1
                    self.sticky[s] |= 1
                    continue
                e.state, e.id, e.first_t, e.last_t, e.n_offered = LIVE, tid, t, t, 1
            e.Q, e.parts, e.best_t = Q, parts, t
            e.det = np.concatenate([np.asarray(boxes[i], F32), np.asarray([scores[i]], F32)])
            e.lms, e.chip = np.asarray(lms[i], F32).copy(), np.asarray(chips[i], np.uint8).copy()
        self.t[s] += 1
        return quality, flag

    def collect(self, s, cap, flush=False):
        """(the collected entries in finishing order -- copies --, pending, the sticky flags)."""
        tab = self.tab[s]
        if flush:
            for e in tab:
                if e.state == LIVE:
                    e.state, e.done_seq = DONE, self.seq[s]
                    self.seq[s] += 1
        done = sorted((e for e in tab if e.state == DONE), key=lambda e: e.done_seq)
        out = []
        for e in done[:max(int(cap), 0)]:
            c = Entry()
            c.__dict__.update(e.__dict__)
            out.append(c)
            e.state = FREE
        flags, self.sticky[s] = self.sticky[s], 0
        return out, len(done) - len(out), flags


def empty_out(F, S, cap, Sz, fill=0):
    """The five row-wise outputs of a sequence, every byte ``fill``."""
    shapes = {"chips": ((F, S, cap, Sz, Sz, 3), np.uint8), "quality": ((F, S, cap), np.int64), "records": ((F, S, cap, 8), np.int32),
              "dets": ((F, S, cap, 5), np.float32), "lms": ((F, S, cap, 10), np.float32)}
    out = {}
    for k, (sh, dt) in shapes.items():
        a = np.empty(sh, dt)
        a.view(np.uint8).fill(fill)
        out[k] = a
    return out


def run_ref(boxes, scores, lms, info, counts, chips, collect, cap=None, fx=1.0, fy=1.0, chip_counts=None, entries=320, min_hits=2, terms=7, out=None):
    """``ops.bestshot_sequence`` through RefBestShots: the same arguments, the same dict of arrays."""
    F, S, rows = np.asarray(boxes).shape[:3]
    Sz = np.asarray(chips).shape[3]
    cap = entries if cap is None else cap
    r = empty_out(F, S, cap, Sz) if out is None else {k: np.array(v, copy=True) for k, v in out.items()}
    for k in ("counts", "pending", "flags", "offer_flags"):
        r[k] = np.zeros((F, S), np.int32)
    r["offer_quality"] = np.zeros((F, S, rows), np.int64)
    ref = RefBestShots(S, entries, min_hits, terms, fx, fy)
    for f in range(F):
        for s in range(S):
            q, fl = ref.offer(s, boxes[f][s], scores[f][s], lms[f][s], info[f][s], counts[f][s], chips[f][s], rows if chip_counts is None else chip_counts[f][s])
            r["offer_quality"][f, s], r["offer_flags"][f, s] = q, fl
        if collect[f]:
            for s in range(S):
                got, pending, flags = ref.collect(s, cap, collect[f] == 2)
                r["counts"][f, s], r["pending"][f, s], r["flags"][f, s] = len(got), pending, flags
                for k, e in enumerate(got):
                    r["chips"][f, s, k], r["quality"][f, s, k], r["records"][f, s, k] = e.chip, e.Q, e.record()
                    r["dets"][f, s, k], r["lms"][f, s, k] = e.det, e.lms
    return r


def same(got, want):
    """Every array of two sequence results, byte for byte."""
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:4].tolist())


# ---------------------------------------------------------------------------------------------- chips
def flat_chip(S, v=93):
    return np.full((S, S, 3), v, np.uint8)


def stripes_chip(S, d=10, tag=0):
    """Grey columns alternating 100 / 100 + d: lap = -+2d, sharp = 4*d*d.  ``tag`` marks a corner pixel, outside the window."""
    c = np.full((S, S, 3), 100, np.uint8)
    c[:, 1::2] = 100 + d
    c[0, 0] = tag
    return c


def checker_chip(S):
    y, x = np.mgrid[0:S, 0:S]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def box_blur(chip, times):
    """3 x 3 box mean with replicated border, rounded, ``times`` times."""
    c = np.asarray(chip).astype(np.int64)
    for _ in range(times):
        p = np.pad(c, ((1, 1), (1, 1), (0, 0)), mode="edge")
        c = (sum(p[dy:dy + c.shape[0], dx:dx + c.shape[1]] for dy in range(3) for dx in range(3)) + 4) // 9
    return c.astype(np.uint8)


def seven_chips(rng, S):
    """random colour, flat, stripes, the 0 / 255 checkerboard, a blurred one, two random ones."""
    rnd = lambda: rng.integers(0, 256, (S, S, 3), dtype=np.uint8)      # noqa: E731
    grey = np.repeat(rng.integers(0, 256, (S, S, 1), dtype=np.uint8), 3, axis=2)
    return np.stack([rnd(), flat_chip(S), stripes_chip(S), checker_chip(S), box_blur(grey, 2), rnd(), rnd()])


FRONTAL = (30.0, 30.0, 50.0, 30.0, 40.0, 40.0, 32.0, 50.0, 48.0, 50.0)      # eyes, nose on the axis, mouth corners


def frontal(nose_dx=0.0):
    """Landmarks whose eye-mouth axis is (0, 20) long: the nose ``nose_dx`` sideways of it gives t = |nose_dx| / 20 * 512."""
    l = np.array(FRONTAL, F32)
    l[4] += F32(nose_dx)
    return l


def edge_rows():
    """(boxes [n,4], scores [n], lms [n,10]) that put each weight at its edges."""
    nan, inf = float("nan"), float("inf")
    rows = [((10, 10, 10, 30), 0.9, frontal()),                 # side 0
            ((10, 10, 9, 30), 0.9, frontal()),                  # negative side
            ((10, 10, 4000, 4000), 0.9, frontal()),             # side >= S
            ((10, 10, 18.5, 40), 0.9, frontal()),               # a fractional side
            ((nan, 10, 30, 30), 0.9, frontal()),                # a NaN corner
            ((10, 10, inf, 30), 0.9, frontal()),
            ((10, 10, 30, 30), 0.9, np.array([30, 30, 50, 30, 40, 40, 30, 30, 50, 30], F32)),      # eyes and mouth coincide
            ((10, 10, 30, 30), 0.9, frontal(0.0)),              # the nose on the axis: 256
            ((10, 10, 30, 30), 0.9, frontal(10.0)),             # offset 0.5: 0
            ((10, 10, 30, 30), 0.9, frontal(-9.99)),
            ((10, 10, 30, 30), 0.9, frontal(3.0)),
            ((10, 10, 30, 30), 0.9, np.array([30, 30, 50, 30, nan, 40, 32, 50, 48, 50], F32)),
            ((10, 10, 30, 30), 0.9, np.array([30, 30, 50, 30, 40, inf, 32, 50, 48, 50], F32)),
            ((10, 10, 30, 30), 0.0, frontal()), ((10, 10, 30, 30), -0.5, frontal()), ((10, 10, 30, 30), 0.5, frontal()),
            ((10, 10, 30, 30), 1.0, frontal()), ((10, 10, 30, 30), 7.5, frontal()), ((10, 10, 30, 30), nan, frontal()),
            ((10, 10, 30, 30), 0.999, frontal()), ((10, 10, 30, 30), 1e-9, frontal())]
    return (np.array([r[0] for r in rows], F32), np.array([r[1] for r in rows], F32), np.stack([np.asarray(r[2], F32) for r in rows]))


# ---------------------------------------------------------------------------------------------- scripted sequences
def script_tables(frames, n_streams, rows, Sz, rng=None):
    """frames[f][s] = a list of rows (id, hits, misses, d[, tag]) -> the tables of ``ops.bestshot_sequence``: the chip of a row is
    ``stripes_chip(Sz, d, tag)`` (sharp = 4*d*d; tag defaults to the frame number), the boxes, scores and landmarks are random where
    ``rng`` is given and a frontal 20-pixel face otherwise.  Rows past a count hold junk that must not matter."""
    F = len(frames)
    boxes, scores = np.full((F, n_streams, rows, 4), 777.0, F32), np.full((F, n_streams, rows), 0.5, F32)
    lms, info = np.full((F, n_streams, rows, 10), 5.0, F32), np.full((F, n_streams, rows, 3), 3, np.int32)
    counts, chips = np.zeros((F, n_streams), np.int32), np.full((F, n_streams, rows, Sz, Sz, 3), 200, np.uint8)
    chips[:, :, :, ::2] = 3                                     # (junk with a high sharpness)
    for f, per_stream in enumerate(frames):
        for s, rws in enumerate(per_stream):
            counts[f, s] = len(rws)
            for i, r in enumerate(rws):
                info[f, s, i] = r[:3]
                chips[f, s, i] = stripes_chip(Sz, r[3], r[4] if len(r) > 4 else f)
                if rng is None:
                    boxes[f, s, i], scores[f, s, i], lms[f, s, i] = (10 + i, 10, 30 + i, 30), 0.75, frontal()
                else:
                    x, y = rng.uniform(0, 40, 2)
                    boxes[f, s, i], scores[f, s, i] = (x, y, x + rng.uniform(4, 30), y + rng.uniform(4, 30)), rng.uniform(0.3, 1.0)
                    lms[f, s, i] = frontal(rng.uniform(-6, 6)) + F32(rng.uniform(-2, 2))
    return dict(boxes=boxes, scores=scores, lms=lms, info=info, counts=counts, chips=chips)


def R(tid, d, hits=5, misses=0, tag=None):
    return (tid, hits, misses, d) if tag is None else (tid, hits, misses, d, tag)


# name -> (frames, collect, options): one stream unless said otherwise
SCRIPTS = {
    # the second frame's chip is as sharp: the first stays; the third is sharper and wins; then the id is gone
    "tie": ([[[R(1, 5)]], [[R(1, 5)]], [[R(1, 3)]], [[R(1, 7)]], [[R(1, 7)]], [[]]], [0, 0, 0, 0, 0, 1], dict(terms=0)),
    # held (misses 1) with a sharper chip: not offered, but alive; a tentative row (hits 1 < min_hits) neither
    "held": ([[[R(1, 5)]], [[R(1, 9, misses=1)]], [[R(1, 9, hits=1)]], [[R(1, 4)]], [[]], [[]]], [0, 0, 0, 0, 0, 1], dict(terms=0)),
    # three ids vanish one after the other and together: DONE in the next offer, seq in entry order
    "vanish": ([[[R(1, 5), R(2, 6), R(3, 7), R(4, 2)]], [[R(2, 6), R(3, 7), R(4, 2)]], [[R(4, 3)]], [[]]], [0, 0, 1, 1], dict(terms=0)),
    # two entries for three ids: the third is flagged until a collect frees an entry, then enters
    "full": ([[[R(1, 5), R(2, 6), R(3, 7)]], [[R(2, 6), R(3, 7)]], [[R(2, 6), R(3, 8)]], [[R(2, 6), R(3, 4)]], [[]]], [0, 0, 1, 0, 2], dict(terms=0, entries=2)),
    # five finished, cap 2: pending 3, 1, 0 in seq order
    "cap": ([[[R(k, k) for k in range(1, 6)]], [[R(5, 1), R(3, 1), R(1, 1)]], [[]], [[]], [[]]], [0, 0, 1, 1, 1], dict(terms=0, cap=2)),
    # flush finishes the live ones behind the finished one
    "flush": ([[[R(1, 5), R(2, 6), R(3, 7)]], [[R(1, 5), R(3, 7)]], [[R(1, 6), R(3, 7)]]], [0, 0, 2], dict(terms=0)),
    # an entry freed by a collect is reused under a new id in the next frame
    "reuse": ([[[R(1, 5)]], [[R(2, 6)]], [[R(3, 7)]], [[R(4, 8)]]], [1, 1, 1, 2], dict(terms=0, entries=2)),
    # duplicate ids (the first row counts), ids 0 and -3 never enter
    "dups": ([[[R(1, 5), R(1, 9), R(0, 9), R(-3, 9), R(2, 4)]], [[R(2, 4), R(2, 8), R(1, 2, misses=2), R(1, 9)]], [[]]], [0, 0, 1], dict(terms=0)),
}


def script_args(name, Sz=16, rng=None):
    frames, collect, opts = SCRIPTS[name]
    rows = max(max(len(r) for per in frames for r in per), 1) + 1
    t = script_tables(frames, len(frames[0]), rows, Sz, rng)
    o = dict(opts)
    entries = o.setdefault("entries", 8)
    t.update(collect=np.array(collect, np.uint8), cap=o.pop("cap", entries))
    return t, o
