"""Cases for the threshold decode and its greedy NMS (thresh_collect / thresh_rank / thresh_mask / thresh_sweep in csrc/cf_decode.hip):
candidate counts on every block, chunk and cap boundary of those kernels, box families whose kept set is known by construction,
heat maps with an exact number of cells above the threshold -- and the references, which are the plain statements the project
already has (oracle.nms_greedy, tests/test_tiles_abi.nms_ref for IoS, oracle.decode_d1 / decode_d2), never a kernel's output.

No GPU is needed to import this module.  tests/test_nms_cases.py shows on the CPU that the cases tell a subtly wrong kernel from a
right one; tests/test_nms_sweep.py runs them on the device.  Everything is selection and float32 arithmetic: every comparison that
uses these cases is bit for bit."""
import functools

import numpy as np

from oracle import centerface_oracle as O
from test_tiles_abi import nms_ref

# n relative to the sweep's 64-candidate blocks, the rank kernel's 4096-score chunks, the 4096-candidate workspace, and the number of
# suppression words nw = ceil(n / 64): 1088 / 1089 = nw 17 / 18 (the lane = word propagation runs for the first time, and hands over to
# the lane = row one at block 1), 4160 / 4161 = nw 65 / 66 (one exactly full 64-word trip from block 0 / a second trip with one live lane)
NS = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1087, 1088, 1089, 1152, 1153, 4095, 4096, 4097, 4160, 4161, 4225)
THRESHOLDS = (0.3, 0.5)
HALF_UP = float(np.nextafter(np.float32(0.5), np.float32(1)))          # the float32 after 0.5

f32 = np.float32


def descending_scores(n):
    """1 - i / 8192: strictly descending and exact in float32 for every i < 8192."""
    assert n <= 8192
    return (f32(1) - np.arange(n, dtype=np.float32) / f32(8192)).astype(np.float32)


def boxes_at(x1, y1=0, size=20):
    """size x size boxes (x2 - x1 = size - 1, so the "+1" area is size^2) with integer corners."""
    x1 = np.asarray(x1, np.float32)
    y1 = np.broadcast_to(np.asarray(y1, np.float32), x1.shape)
    return np.stack([x1, y1, x1 + f32(size - 1), y1 + f32(size - 1)], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------ box families
def chain(n):
    """A row of 20 x 20 boxes, each shifted from the one before by 6 (IoU 280 / 520: suppresses at 0.3 and at 0.5), 12 (160 / 640) or 25
    (neither does), scores strictly descending along the row: the kept set is a serial parity chain with pseudo-random phase breaks, so
    one wrong bit at a block boundary flips everything behind it."""
    rng = np.random.default_rng(1000 + n)
    x1 = np.cumsum(rng.choice([6, 6, 6, 12, 25], n))
    return boxes_at(x1), descending_scores(n)


def chain_serial_keep(boxes):
    """The kept set of `chain` restated serially: a box goes exactly when the last kept box starts 6 before it (boxes that are not
    neighbours lie at least 12 apart, which does not suppress)."""
    keep, last = [], None
    for i, x in enumerate(boxes[:, 0].tolist()):
        if last is None or x - last != 6:
            keep.append(i)
            last = x
    return keep


def chain_perm(n):
    """`chain` under a seeded permutation with the same score vector: rank != index, neighbours in space are far apart in rank."""
    b, s = chain(n)
    return b[np.random.default_rng(2000 + n).permutation(n)], s


def chain_tie(n):
    """`chain` with all scores equal: the order is index descending through every 4096-chunk of the rank kernel."""
    b, _ = chain(n)
    return b, np.full(n, 0.5, np.float32)


def pool(n):
    """Candidate i is a copy of box id_i = rng.integers(0, 1 + i // 8), boxes 40 apart: kept are exactly the first occurrences, every
    block has some, and most suppression comes from a keeper many blocks earlier."""
    return boxes_at(40 * np.array(pool_ids(n), np.int64)), descending_scores(n)


def pool_ids(n):
    rng = np.random.default_rng(3000 + n)
    return [int(rng.integers(0, 1 + i // 8)) for i in range(n)]


def pool67(n):
    """Candidate i is a copy of box i % 67: exactly the first min(n, 67) are kept, every block behind the second ends up empty."""
    return boxes_at(40 * (np.arange(n) % 67)), descending_scores(n)


def random_boxes(n):
    """Clustered boxes with fractional float32 corners (the rounding of every product, sum and quotient matters) and scores drawn from 40
    quantised values (many ties)."""
    rng = np.random.default_rng(4000 + n)
    centres = rng.uniform(0, 60.0 * np.sqrt(n) + 40, (max(1, n // 6), 2))
    c = centres[rng.integers(0, len(centres), n)] + rng.normal(0, 9, (n, 2))
    wh = rng.uniform(8, 60, (n, 2))
    b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    return b, rng.choice(np.linspace(0.31, 0.99, 40).astype(np.float32), n)


FAMILIES = {"chain": chain, "chain_perm": chain_perm, "chain_tie": chain_tie, "pool": pool, "pool67": pool67, "random": random_boxes}
IOS_FAMILIES = ("random", "pool", "pool67")


@functools.lru_cache(maxsize=None)
def family_case(family, n):
    b, s = FAMILIES[family](n)
    b.setflags(write=False)
    s.setflags(write=False)
    return b, s


# The pair whose overlap EQUALS the threshold.  IoU: [0,0,9,9] (area 100) inside [0,0,9,19] (area 200): 100 / 200 = 0.5 exactly.  IoS:
# [0,0,9,9] against [5,0,14,19]: intersection 5 x 10 = 50, smaller area 100: 0.5 exactly (IoU 50 / 250, the larger area would give 0.25).
EXACT_PAIR = {"iou": ((0, 0, 9, 9), (0, 0, 9, 19)), "ios": ((0, 0, 9, 9), (5, 0, 14, 19))}
EXACT_POS = (0, 62, 63, 64, 127)             # rank of the pair's first box: inside a block, on its last bit, across the boundary, behind it
EXACT_N = 130


@functools.lru_cache(maxsize=None)
def exact_case(metric, pos):
    """EXACT_N candidates, scores strictly descending; ranks pos and pos + 1 hold the pair, every other box stands alone 100 apart."""
    b = boxes_at(1000 + 100 * np.arange(EXACT_N))
    b[pos], b[pos + 1] = EXACT_PAIR[metric]
    s = descending_scores(EXACT_N)
    b.setflags(write=False)
    s.setflags(write=False)
    return b, s


def exact_want(pos, thresh):
    """At the threshold 0.5 the pair's second box goes (`>=`), at the next float32 it stays."""
    return [i for i in range(EXACT_N) if not (i == pos + 1 and f32(thresh) <= f32(0.5))]


def landmarks_for(n, seed=0):
    """Landmark rows that ride along with n candidates (the merge carries them through untouched)."""
    return np.random.default_rng(5000 + seed + n).normal(50, 20, (n, 10)).astype(np.float32)


# ------------------------------------------------------------------------------------------ references
_REF = {}


def reference_keep(boxes, scores, thresh, metric="iou", key=None):
    """Kept indices in keep order by the project's plain statements.  `key` (hashable) caches the result for the session."""
    if key is not None and (key, float(thresh), metric) in _REF:
        return _REF[(key, float(thresh), metric)]
    keep = O.nms_greedy(boxes, scores, thresh) if metric == "iou" else nms_ref(boxes, scores, thresh, "ios")
    if key is not None:
        _REF[(key, float(thresh), metric)] = keep
    return keep


def family_reference(family, n, thresh, metric="iou"):
    b, s = family_case(family, n)
    return reference_keep(b, s, thresh, metric, key=(family, n))


def reach(n):
    """Which parts of the sweep a count reaches: (blocks, 'row' / 'word' / 'word2' propagation paths, rank chunks)."""
    nw = (n + 63) // 64
    paths = set()
    for blk in range(nw):
        rest = nw - blk - 1
        if 0 < rest <= 16:
            paths.add("row")
        elif rest > 16:
            paths.add("word2" if rest > 64 else "word")
    return nw, sorted(paths), (n + 4095) // 4096


# ------------------------------------------------------------------------------------------ heat maps
#               h   w  cells above the threshold
MAP_SHAPES = ((7, 9, 63), (5, 13, 65), (33, 31, 1023), (25, 41, 1025), (72, 64, 0), (72, 64, 4096), (72, 64, 4097), (72, 64, 4608),
              (66, 64, 4161))
MAP_BATCHES = (((72, 64), (0, 4097, 65)), ((72, 64), (4096, 63)))       # one image forces the grow-and-rerun / the count equals the cap
MAP_THRESH = 0.3


@functools.lru_cache(maxsize=None)
def map_case(h, w, ncand, thr=MAP_THRESH):
    """Head maps of one image with EXACTLY ncand cells above thr: hm [1,1,h,w], wh [1,2,h,w], reg [1,2,h,w], lm [1,10,h,w] and the clamp
    size (4h - 6, 4w - 10), which is inside the map so that the min(.., img_w) / min(.., img_h) clamps engage.  The background is uniform
    in (0.01, thr]; one candidate sits on the float32 right above thr, three background cells on thr itself (`>` excludes them)."""
    rng = np.random.default_rng(6000 + 131 * h + 17 * w + ncand)
    t = f32(thr)
    hw = h * w
    hm = np.minimum(rng.uniform(0.01, thr, hw).astype(np.float32), t)
    cells = rng.permutation(hw)
    above, below = cells[:ncand], cells[ncand:]
    hm[above] = rng.choice(np.linspace(0.31, 0.99, 50).astype(np.float32), ncand)
    if ncand:
        hm[above[0]] = np.nextafter(t, f32(1))
    hm[below[:3]] = t
    assert int((hm > t).sum()) == ncand
    out = dict(hm=hm.reshape(1, 1, h, w), wh=rng.uniform(0.5, 6, (1, 2, h, w)).astype(np.float32),
               reg=rng.uniform(0, 1, (1, 2, h, w)).astype(np.float32), lm=rng.normal(0, 1, (1, 10, h, w)).astype(np.float32))
    for a in out.values():
        a.setflags(write=False)
    out["size"] = (4 * h - 6, 4 * w - 10)
    return out


def _subsequence(rows, of):
    """Positions in `of` of the rows of `rows`, which is a subsequence of it (both in the NMS order)."""
    pos, k = [], 0
    for r in rows:
        while of[k].tobytes() != r.tobytes():
            k += 1
        pos.append(k)
        k += 1
    return pos


@functools.lru_cache(maxsize=None)
def map_reference(h, w, ncand, mode, nms_thresh=0.3, thr=MAP_THRESH):
    """(dets [k,5], lms [k,10]) of one map by oracle.decode_d1 (mode 0) / decode_d2 (mode 1).  decode_d2 returns no landmarks: they are
    decode_d1's rows (the landmark arithmetic does not depend on the mode) of the candidates decode_d2 kept -- both functions list the
    candidates in the same order when nothing is suppressed (nms_thresh 2), and the kept rows are a subsequence of that list."""
    m = map_case(h, w, ncand, thr)
    t = f32(thr)
    if ncand == 0:
        return np.zeros((0, 5), np.float32), np.zeros((0, 10), np.float32)
    if mode == 0:
        d, l = O.decode_d1(m["hm"], m["wh"], m["reg"], m["lm"], m["size"], nms_thresh=nms_thresh, fixed_threshold=t)
        return np.asarray(d, np.float32).reshape(-1, 5), np.asarray(l, np.float32).reshape(-1, 10)
    d = np.asarray(O.decode_d2(m["hm"][0], m["wh"][0], m["reg"][0], m["size"], threshold=t, nms_thresh=nms_thresh), np.float32).reshape(-1, 5)
    every = np.asarray(O.decode_d2(m["hm"][0], m["wh"][0], m["reg"][0], m["size"], threshold=t, nms_thresh=2.0), np.float32).reshape(-1, 5)
    _, every_l = O.decode_d1(m["hm"], m["wh"], m["reg"], m["lm"], m["size"], nms_thresh=2.0, fixed_threshold=t)
    assert len(every) == ncand == len(every_l)
    return d, np.asarray(every_l, np.float32)[_subsequence(d, every)]
