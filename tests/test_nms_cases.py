"""Do the cases of tests/nms_cases.py discriminate?  (No GPU.)

A numpy model of the threshold decode AS THE KERNELS STRUCTURE IT (csrc/cf_decode.hip): the 16-segment collect with its capacity guard
and rerun, the rank with the 4096-chunked comparison, the upper-triangle suppression words, the sweep over 64-candidate blocks with a
`removed` bitmap and the two propagation paths picked by the number of words still ahead.  The model must equal the references on every
case; then each of a list of subtle defects is switched on, one at a time, and at least one named case must change its result.  That is
the evidence that tests/test_nms_sweep.py, which runs the same cases on the device against the same references, would fail on a kernel
with such a defect.  `python tests/test_nms_cases.py` prints the case table and the defect / case matrix of profiles/nms_sweep.md."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import nms_cases as N

f32 = np.float32
CH = 4096                                                # scores staged per trip of the rank kernel

RANK_DEFECTS = {"tie_reversed": "the tie rule reversed ((j0 + j) < i)",
                "tie_chunk_local": "rank compared within a 4096 chunk only (the tie index is j, not j0 + j)"}
MASK_DEFECTS = {"nms_gt": "> for >= at the NMS threshold",
                "area_no_plus1": "areas without the +1",
                "ios_larger": "IoS over the larger area"}
SWEEP_DEFECTS = {"drop_far_words": "propagation dropped for words more than 16 ahead",
                 "drop_second_trip": "propagation dropped for words in the second 64-word trip",
                 "lose_bit63": "bit 63 of a full block lost",
                 "count_past_n": "rows past n counted in the last block"}
MAP_DEFECTS = {"score_ge": ">= for > at the score threshold"}
DEFECTS = {**RANK_DEFECTS, **MASK_DEFECTS, **SWEEP_DEFECTS, **MAP_DEFECTS}


# ------------------------------------------------------------------------------------------ the blocked model
def model_order(scores, defect=None):
    """thresh_rank_kernel: rank = number of candidates that precede in (score desc, index desc), counted chunk by chunk; order[rank] = i.
    None when the ranks are not a permutation (a defect can do that: the kernel would leave holes in `order`)."""
    n = len(scores)
    i = np.arange(n)
    rank = np.zeros(n, np.int64)
    for j0 in range(0, n, CH):
        sj = scores[j0:j0 + CH]
        j = np.arange(len(sj))
        jj = j if defect == "tie_chunk_local" else j0 + j
        tie = (jj[None, :] < i[:, None]) if defect == "tie_reversed" else (jj[None, :] > i[:, None])
        rank += ((sj[None, :] > scores[:, None]) | ((sj[None, :] == scores[:, None]) & tie)).sum(1)
    if len(set(rank.tolist())) != n:
        return None
    order = np.empty(n, np.int64)
    order[rank] = i
    return order


def model_words(b, threshes, metric="iou", defect=None):
    """thresh_mask_kernel on candidates in sorted order: for every threshold the [n, nw] uint64 words, bit (r, c) set when row r suppresses
    column c > r; words with cw * 64 + 63 <= r are zero.  One pass over the overlaps serves all thresholds."""
    n = len(b)
    nw = (n + 63) // 64
    one = f32(0) if defect == "area_no_plus1" else f32(1)
    x1, y1, x2, y2 = (np.ascontiguousarray(b[:, k], np.float32) for k in range(4))
    area = (x2 - x1 + one) * (y2 - y1 + one)
    out = [np.zeros((n, nw), np.uint64) for _ in threshes]
    cols = np.arange(nw * 64)
    with np.errstate(all="ignore"):
        for blk in range(nw):
            r0, r1 = blk * 64, min(n, blk * 64 + 64)
            c = slice(r0, n)
            w = np.maximum(f32(0), np.minimum(x2[r0:r1, None], x2[None, c]) - np.maximum(x1[r0:r1, None], x1[None, c]) + f32(1))
            h = np.maximum(f32(0), np.minimum(y2[r0:r1, None], y2[None, c]) - np.maximum(y1[r0:r1, None], y1[None, c]) + f32(1))
            inter = w * h
            if metric == "ios":
                den = (np.maximum if defect == "ios_larger" else np.minimum)(area[r0:r1, None], area[None, c])
            else:
                den = area[r0:r1, None] + area[None, c] - inter
            ovr = inter / den
            upper = cols[None, r0:n] > np.arange(r0, r1)[:, None]
            for k, t in enumerate(threshes):
                sup = np.zeros((r1 - r0, (nw - blk) * 64), bool)
                sup[:, :n - r0] = ((ovr > f32(t)) if defect == "nms_gt" else (ovr >= f32(t))) & upper
                out[k][r0:r1, blk:] = np.packbits(sup, axis=1, bitorder="little").view("<u8")
    return out


def model_sweep(words, n, defect=None):
    """thresh_sweep_kernel: kept ranks in keep order.  A rank >= n in the result is a row past the count (a defect can emit one)."""
    nw = (n + 63) // 64
    removed = np.zeros(nw, np.uint64)
    kept = []
    for blk in range(nw):
        nvalid = min(64, n - blk * 64)
        rem, kb = int(removed[blk]), 0
        diag = [int(v) for v in words[blk * 64:blk * 64 + nvalid, blk]] + [0] * (64 - nvalid)      # rows past n are all-zero
        for i in range(64):                              # the serial scalar loop
            if not (rem >> i) & 1:
                kb |= 1 << i
                rem |= diag[i]
        if nvalid < 64 and defect != "count_past_n":
            kb &= (1 << nvalid) - 1
        if nvalid == 64 and defect == "lose_bit63":
            kb &= (1 << 63) - 1
        rows = [blk * 64 + i for i in range(64) if (kb >> i) & 1]
        kept += rows
        live = [r for r in rows if r < n]
        rest = nw - (blk + 1)
        if not live or rest == 0:
            continue
        if rest <= 16:                                   # lane = row: the remaining words of every kept row, one wave-wide OR per word
            removed[blk + 1:nw] |= np.bitwise_or.reduce(words[live, blk + 1:nw], axis=0)
        else:                                            # lane = word: trips of 64 words
            for trip, w0 in enumerate(range(blk + 1, nw, 64)):
                w1 = min(w0 + 64, nw)
                if defect == "drop_second_trip" and trip >= 1:
                    continue
                if defect == "drop_far_words":
                    w1 = min(w1, blk + 17)
                if w1 > w0:
                    removed[w0:w1] |= np.bitwise_or.reduce(words[live, w0:w1], axis=0)
    return kept


class Model:
    """The stages of one case with their intermediate results kept, so that a defect recomputes only what lies behind it."""

    def __init__(self, boxes, scores, threshes, metric="iou"):
        self.b, self.s, self.t, self.metric = np.asarray(boxes, np.float32), np.asarray(scores, np.float32), tuple(threshes), metric
        self.n = len(self.s)
        self._order, self._words = {}, {}

    def order(self, defect=None):
        d = defect if defect in RANK_DEFECTS else None
        if d not in self._order:
            self._order[d] = model_order(self.s, d)
        return self._order[d]

    def words(self, defect=None):
        rd, md = (defect if defect in RANK_DEFECTS else None), (defect if defect in MASK_DEFECTS else None)
        if rd is not None and self.order(rd) is not None and np.array_equal(self.order(rd), self.order()):
            rd = None                                    # the defect left the order alone: the same words
        if (rd, md) not in self._words:
            self._words[(rd, md)] = model_words(self.b[self.order(rd)], self.t, self.metric, md)
        return self._words[(rd, md)]

    def keep(self, defect=None):
        """Per threshold: kept ORIGINAL indices in keep order (-1 = a row past n), or None when the order is no permutation."""
        order = self.order(defect)
        if order is None:
            return [None] * len(self.t)
        sd = defect if defect in SWEEP_DEFECTS else None
        return [[int(order[r]) if r < self.n else -1 for r in model_sweep(w, self.n, sd)] for w in self.words(defect)]


# candidate arithmetic of thresh_emit, vectorised (float64 intermediates from float32 maps, cast at the end)
def model_candidates(m, cells, mode):
    h, w = m["hm"].shape[2:]
    cy, cx = np.divmod(cells, w)
    at = lambda a, k: a[0, k].reshape(-1)[cells]
    s0, s1 = at(m["wh"], 0) * f32(4), at(m["wh"], 1) * f32(4)
    ox = at(m["reg"], 1).astype(np.float64) if mode == 1 else 0.0
    oy = at(m["reg"], 0).astype(np.float64) if mode == 1 else 0.0
    ih, iw = (float(v) for v in m["size"])
    x1 = np.minimum(np.maximum(0.0, (cx + ox + 0.5) * 4 - (s0 / f32(2)).astype(np.float64)), iw)
    y1 = np.minimum(np.maximum(0.0, (cy + oy + 0.5) * 4 - (s1 / f32(2)).astype(np.float64)), ih)
    x2, y2 = np.minimum(x1 + s0.astype(np.float64), iw), np.minimum(y1 + s1.astype(np.float64), ih)
    dets = np.stack([x1, y1, x2, y2, at(m["hm"], 0).astype(np.float64)], 1).astype(np.float32)
    lms = np.empty((len(cells), 10), np.float64)
    for j in range(5):
        lms[:, 2 * j] = (at(m["lm"], 2 * j).astype(np.float64) + cx + 0.5) * 4
        lms[:, 2 * j + 1] = (at(m["lm"], 2 * j + 1).astype(np.float64) + cy + 0.5) * 4
    return dets, lms.astype(np.float32)


def model_collect(hm, thr, cap, defect=None):
    """thresh_collect_kernel: 16 waves, each a contiguous segment of ceil(HW / 16) cells rounded up to 64; the hits of every segment
    behind the prefix of the wave counts, stored only while pos < cap.  Returns (cells stored, total)."""
    flat = hm.reshape(-1)
    HW = flat.size
    seg = ((HW + 15) // 16 + 63) // 64 * 64
    hit = (flat >= f32(thr)) if defect == "score_ge" else (flat > f32(thr))
    per_wave = [np.nonzero(hit[wv * seg:min(wv * seg + seg, HW)])[0] + wv * seg for wv in range(16) if wv * seg < HW]
    idx = np.concatenate(per_wave) if per_wave else np.zeros(0, np.int64)
    return idx[:cap], len(idx)


def model_decode(m, mode, nms_thresh=0.3, thr=N.MAP_THRESH, defect=None):
    """The whole decode of one map: (dets, lms, cap the workspace ended at, reruns)."""
    HW = m["hm"].size
    cap = (HW + 63) // 64 * 64 if HW < 4096 else 4096
    reruns = 0
    while True:
        cells, total = model_collect(m["hm"], thr, cap, defect)
        if total <= cap:
            break
        cap, reruns = (min(total, HW) + 63) // 64 * 64, reruns + 1
        assert reruns < 2
    dets, lms = model_candidates(m, cells, mode)
    if not len(cells):
        return dets, lms, cap, reruns
    keep = Model(dets[:, :4], dets[:, 4], (nms_thresh,)).keep(defect if defect not in MAP_DEFECTS else None)[0]
    return dets[keep], lms[keep], cap, reruns


# ------------------------------------------------------------------------------------------ the cases, named
def box_cases():
    """(id, boxes, scores, thresholds, metric, reference keep per threshold) for every box case of nms_cases."""
    for fam in N.FAMILIES:
        for n in N.NS:
            b, s = N.family_case(fam, n)
            yield "%s-%d" % (fam, n), b, s, N.THRESHOLDS, "iou", [N.family_reference(fam, n, t) for t in N.THRESHOLDS]
    for fam in N.IOS_FAMILIES:
        for n in N.NS:
            b, s = N.family_case(fam, n)
            yield "%s-ios-%d" % (fam, n), b, s, N.THRESHOLDS, "ios", [N.family_reference(fam, n, t, "ios") for t in N.THRESHOLDS]
    for metric in ("iou", "ios"):
        for pos in N.EXACT_POS:
            b, s = N.exact_case(metric, pos)
            t = (0.5, N.HALF_UP)
            yield "exact-%s-%d" % (metric, pos), b, s, t, metric, [N.reference_keep(b, s, v, metric, key=("exact", metric, pos)) for v in t]


_MODELS = {}


def model_of(cid, b, s, t, metric):
    if cid not in _MODELS:
        _MODELS[cid] = Model(b, s, t, metric)
    return _MODELS[cid]


CASE_GROUPS = sorted(N.FAMILIES) + ["%s-ios" % f for f in N.IOS_FAMILIES] + ["exact"]


def _group(cid):
    return cid.rsplit("-", 1)[0] if not cid.startswith("exact") else "exact"


# ------------------------------------------------------------------------------------------ the generators do what they say
def test_generators_have_the_properties_the_cases_rest_on():
    assert N.NS == (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1087, 1088, 1089, 1152, 1153, 4095, 4096, 4097, 4160, 4161, 4225)
    assert [N.reach(n)[0] for n in (1088, 1089, 4160, 4161)] == [17, 18, 65, 66]
    assert N.reach(1088)[1] == ["row"] and N.reach(1089)[1] == ["row", "word"] and N.reach(4160)[1] == ["row", "word"]
    assert N.reach(4161)[1] == ["row", "word", "word2"] and N.reach(4096)[2] == 1 and N.reach(4097)[2] == 2
    kept = []
    for n in N.NS:
        b, s = N.family_case("chain", n)
        assert b.dtype == s.dtype == np.float32 and np.array_equal(b, np.round(b)) and np.all(np.diff(s) < 0)
        assert np.array_equal(s.astype(np.float64), 1 - np.arange(n) / 8192)                 # exact in float32
        want = N.chain_serial_keep(b)
        assert N.family_reference("chain", n, 0.3) == want == N.family_reference("chain", n, 0.5)
        kept.append(len(want))
        bp, sp = N.family_case("chain_perm", n)
        assert np.array_equal(np.sort(bp[:, 0]), b[:, 0]) and np.array_equal(sp, s)
        assert N.family_reference("chain_tie", n, 0.3)[0] == n - 1                           # ties: the higher index first
        ids = N.pool_ids(n)
        first = [i for i, v in enumerate(ids) if v not in ids[:i]]
        assert N.family_reference("pool", n, 0.3) == first == N.family_reference("pool", n, 0.5, "ios")
        assert n < 128 or all(any(64 * k <= i < 64 * k + 64 for i in first) for k in range(n // 64))      # keepers in every block
        assert N.family_reference("pool67", n, 0.3) == list(range(min(n, 67))) == N.family_reference("pool67", n, 0.5, "ios")
        rb, rs = N.family_case("random", n)
        assert len(set(rs.tolist())) <= 40 and (n < 63 or len(set(rs.tolist())) < n) and np.all(rb[:, 2:] > rb[:, :2])
    assert kept[0] == 1 and kept[-1] > 2000
    for metric in ("iou", "ios"):
        for pos in N.EXACT_POS:
            b, s = N.exact_case(metric, pos)
            assert N.reference_keep(b, s, 0.5, metric) == N.exact_want(pos, 0.5) == [i for i in range(N.EXACT_N) if i != pos + 1]
            assert N.reference_keep(b, s, N.HALF_UP, metric) == N.exact_want(pos, N.HALF_UP) == list(range(N.EXACT_N))
    assert f32(N.HALF_UP) > f32(0.5) and float(f32(N.HALF_UP)) == N.HALF_UP


def test_map_generator_puts_exactly_ncand_cells_above_the_threshold():
    t = f32(N.MAP_THRESH)
    for h, w, ncand in N.MAP_SHAPES + tuple((hw[0], hw[1], c) for hw, cs in N.MAP_BATCHES for c in cs):
        m = N.map_case(h, w, ncand)
        hm = m["hm"].reshape(-1)
        assert int((hm > t).sum()) == ncand and hm.min() > 0.01 - 1e-6
        assert int((hm == t).sum()) >= min(3, h * w - ncand)                                 # on the threshold: excluded
        assert ncand == 0 or int((hm == np.nextafter(t, f32(1))).sum()) >= 1                 # right above it: included
        assert m["size"] == (4 * h - 6, 4 * w - 10)
        for mode in (0, 1):
            d, l = N.map_reference(h, w, ncand, mode)
            assert d.shape == (len(l), 5) and l.shape[1] == 10 and (len(d) > 0) == (ncand > 0)
            if ncand > 60:
                assert (d[:, 2] == m["size"][1]).any() and (d[:, 3] == m["size"][0]).any()   # both clamps engage


# ------------------------------------------------------------------------------------------ the model equals the references
@pytest.mark.parametrize("group", CASE_GROUPS)
def test_blocked_model_equals_the_references(group):
    seen = 0
    for cid, b, s, t, metric, want in box_cases():
        if _group(cid) != group:
            continue
        got = model_of(cid, b, s, t, metric).keep()
        for k, thr in enumerate(t):
            assert got[k] == want[k], (cid, thr)
        seen += 1
    assert seen == (len(N.EXACT_POS) * 2 if group == "exact" else len(N.NS))


def test_blocked_model_equals_the_map_decodes():
    for h, w, ncand in N.MAP_SHAPES:
        m = N.map_case(h, w, ncand)
        for mode in (0, 1):
            d, l, cap, reruns = model_decode(m, mode)
            wd, wl = N.map_reference(h, w, ncand, mode)
            assert d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes(), (h, w, ncand, mode)
            assert reruns == (1 if ncand > 4096 else 0) and cap >= ncand, (h, w, ncand, cap, reruns)


# ------------------------------------------------------------------------------------------ injected defects
def heavy(cid):
    """The mask has to be rebuilt for a defect in the overlap arithmetic or in the order; that arithmetic does not depend on the count, so
    these defects run on the counts up to 1153 (and on 4097 / 4225 for the tie rules, which need the second rank chunk)."""
    return int(cid.rsplit("-", 1)[1]) > 1153 and not cid.startswith("exact")


def defect_matrix():
    """{defect: [ids of the cases whose result changes]} over every case the defect is run on."""
    caught = {d: [] for d in DEFECTS}
    for cid, b, s, t, metric, want in box_cases():
        mdl = model_of(cid, b, s, t, metric)
        base = mdl.keep()
        assert base == want, cid
        for d in list(RANK_DEFECTS) + list(MASK_DEFECTS) + list(SWEEP_DEFECTS):
            if d == "ios_larger" and metric != "ios":
                continue
            if d in MASK_DEFECTS and heavy(cid):
                continue
            if d in RANK_DEFECTS and heavy(cid) and not (_group(cid) in ("chain_tie", "random") and int(cid.rsplit("-", 1)[1]) in (4097, 4225)):
                continue
            if mdl.keep(d) != base:
                caught[d].append(cid)
    for h, w, ncand in N.MAP_SHAPES:
        m = N.map_case(h, w, ncand)
        for mode in (0, 1):
            wd, _ = N.map_reference(h, w, ncand, mode)
            d, _, _, _ = model_decode(m, mode, defect="score_ge")
            if d.tobytes() != wd.tobytes():
                caught["score_ge"].append("map-%dx%d-%d-d%d" % (h, w, ncand, mode + 1))
    return caught


_MATRIX = {}


def matrix():
    if not _MATRIX:
        _MATRIX.update(defect_matrix())
    return _MATRIX


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_every_injected_defect_changes_a_named_case(defect):
    caught = matrix()[defect]
    print("NMSDEFECT %s (%s): %d cases, e.g. %s" % (defect, DEFECTS[defect], len(caught), caught[:6]))
    assert caught, "no case notices: %s" % DEFECTS[defect]


def test_defects_are_caught_where_the_structure_says():
    """The boundaries the counts were chosen for: each of these defects is noticed at the first count that reaches its path and at none
    that does not."""
    mx = matrix()
    ns = lambda d, fam: sorted(int(c.rsplit("-", 1)[1]) for c in mx[d] if _group(c) == fam)
    assert ns("drop_far_words", "pool67") == [n for n in N.NS if n >= 1089]              # nw >= 18: a word 17 ahead exists
    assert ns("drop_second_trip", "pool67") == [n for n in N.NS if n >= 4161]            # nw >= 66
    assert ns("count_past_n", "pool67") == [n for n in N.NS if n % 64]
    assert ns("count_past_n", "chain") == [n for n in N.NS if n % 64]
    assert set(ns("lose_bit63", "chain")) | set(ns("lose_bit63", "chain_tie")) | set(ns("lose_bit63", "pool67")) >= {n for n in N.NS if n >= 64}
    assert ns("tie_chunk_local", "chain_tie") == [4097, 4225] and ns("tie_reversed", "chain_tie") == [n for n in N.NS if 2 <= n <= 1153 or n in (4097, 4225)]         # the first kept index is n - 1, not 0
    assert sorted(c for c in mx["nms_gt"] if c.startswith("exact")) == sorted("exact-%s-%d" % (m, p) for m in ("iou", "ios") for p in N.EXACT_POS)
    assert sorted(c for c in mx["ios_larger"] if c.startswith("exact")) == sorted("exact-ios-%d" % p for p in N.EXACT_POS)
    assert len(mx["score_ge"]) == 2 * sum(1 for h, w, c in N.MAP_SHAPES if c < h * w)     # every map with a cell ON the threshold


if __name__ == "__main__":
    print("| case | n | blocks | propagation | rank chunks | kept at 0.3 | kept at 0.5 |\n|---|---|---|---|---|---|---|")
    for cid, b, s, t, metric, want in box_cases():
        nw, paths, chunks = N.reach(len(s))
        print("| %s | %d | %d | %s | %d | %d | %d |" % (cid, len(s), nw, "+".join(paths) or "-", chunks, len(want[0]), len(want[1])))
    print()
    mx = defect_matrix()
    print("| defect | cases that notice | of them |\n|---|---|---|")
    for d, ids in mx.items():
        groups = {}
        for c in ids:
            g = _group(c) if not c.startswith("map") else "map"
            groups.setdefault(g, []).append(c.rsplit("-", 1)[1] if g not in ("map",) else c[4:])
        print("| %s | %d | %s |" % (DEFECTS[d], len(ids), "; ".join("%s: %s" % (g, ",".join(v)) for g, v in groups.items())))
