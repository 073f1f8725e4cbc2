"""Best-shot selection on the GPU: the scoring kernel and whole scripted sequences against the numpy restatement
(tests/bestshot_cases.py) bit for bit, then the table behind an engine's tracked rows and aligned chips, and CenterFace.best_shots."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
import bestshot_cases as bc
from bestshot_cases import R, RefBestShots, quality_ref
from test_redact import SOURCES, source_frames
from test_track import _blank_batch, _feed_until_faces, _state_error

pytestmark = pytest.mark.gpu


def check_quality(chips, boxes, scores, lms, fx, fy, terms=7):
    q, parts = ops.chip_quality(chips, boxes, scores, lms, fx, fy, terms=terms)
    want = [quality_ref(c, b, s, l, fx, fy, terms) for c, b, s, l in zip(chips, boxes, scores, lms)]
    assert q.dtype == np.int64 and parts.dtype == np.int32
    assert q.tolist() == [w[0] for w in want] and parts.tolist() == [list(w[1]) for w in want]
    return q, parts


def random_rows(rng, n):
    x, y = rng.uniform(0, 40, (2, n))
    boxes = np.stack([x, y, x + rng.uniform(2, 60, n), y + rng.uniform(2, 60, n)], axis=1).astype(np.float32)
    lms = np.stack([bc.frontal(d) for d in rng.uniform(-8, 8, n)]) + rng.uniform(-1, 1, (n, 10)).astype(np.float32)
    return boxes, rng.uniform(0.2, 1.0, n).astype(np.float32), lms.astype(np.float32)


@pytest.mark.parametrize("S", bc.SIZES)
def test_chip_quality_of_seven_chips(S):
    rng = np.random.default_rng(S)
    chips = bc.seven_chips(rng, S)
    rows = random_rows(rng, 7)
    for fx, fy in ((1.0, 1.0), (3.0, 1.6875)):
        q, parts = check_quality(chips, *rows, fx, fy)
        assert parts[1:4, 0].tolist() == [0, 400, 1040400] and parts[0, 0] > parts[4, 0] > 0 and (q >= 0).all()
    q, parts = check_quality(chips, *rows, 1.0, 1.0, terms=0)
    assert q[3] == 1040400 << 24                                           # the int64 extreme of the sums at S = 512


@pytest.mark.parametrize("fxy", ((1.0, 1.0), (3.0, 1.6875)))
def test_chip_quality_at_the_edges_of_every_weight(fxy):
    boxes, scores, lms = bc.edge_rows()
    chips = np.stack([bc.stripes_chip(16, 10, tag=k) for k in range(len(boxes))])
    q, parts = check_quality(chips, boxes, scores, lms, *fxy)
    assert (parts[:, 0] == 400).all() and (q == 0).sum() >= 8 and (q > 0).sum() >= 4
    if fxy == (1.0, 1.0):
        assert parts[:4, 1].tolist() == [0, 0, 256, 128] and parts[6:10, 2].tolist() == [0, 256, 0, 1]


@pytest.mark.parametrize("terms", range(8))
def test_chip_quality_with_every_terms_mask(terms):
    rng = np.random.default_rng(terms)
    chips = bc.seven_chips(rng, 16)
    _, parts = check_quality(chips, *random_rows(rng, 7), 1.5, 0.75, terms=terms)
    for bit, col in ((1, 1), (2, 2), (4, 3)):
        assert terms & bit or (parts[:, col] == 256).all()


# ---------------------------------------------------------------------------------------------- whole sequences
def check_sequence(t, o, fill=0xAB):
    """ops.bestshot_sequence == the restatement on every output; rows at and past a count keep the sentinel bytes."""
    F, S = t["counts"].shape
    Sz, cap = t["chips"].shape[3], t["cap"]
    out = bc.empty_out(F, S, cap, Sz, fill)
    want = bc.run_ref(out=out, **t, **o)
    got = ops.bestshot_sequence(out={k: v.copy() for k, v in out.items()}, **t, **o)
    bc.same(got, want)
    for f in range(F):
        for s in range(S):
            for k in out:
                assert (got[k][f, s, got["counts"][f, s]:].view(np.uint8) == fill).all(), (k, f, s)
    return got


@pytest.mark.parametrize("name", sorted(bc.SCRIPTS))
def test_scripted_sequences(name):
    got = check_sequence(*bc.script_args(name))
    assert got["counts"].sum() >= 1
    rng = np.random.default_rng(len(name))
    t, o = bc.script_args(name, rng=rng)
    check_sequence(t, dict(o, terms=7), fill=0x11)


def _histories(rng, F, S, rows, lifetime=4):
    """Per stream a changing population of ids: births, deaths, held and tentative rows, shuffled row order."""
    frames, nxt, alive = [], [1] * S, [[] for _ in range(S)]
    for f in range(F):
        per = []
        for s in range(S):
            alive[s] = [(tid, born) for tid, born in alive[s] if rng.random() > 1.0 / lifetime]
            while len(alive[s]) < rows - 1 and rng.random() < 0.6 + 0.1 * s:
                alive[s].append((nxt[s], f))
                nxt[s] += 1
            rws = [R(tid, int(rng.integers(1, 12)), hits=f - born + 1, misses=int(rng.random() < 0.2)) for tid, born in alive[s]]
            per.append([rws[k] for k in rng.permutation(len(rws))])
        frames.append(per)
    return frames


def test_three_streams_with_different_histories_collected_every_frame_or_at_the_end():
    rng = np.random.default_rng(2)
    F, S, rows = 10, 3, 7
    frames = _histories(rng, F, S, rows)
    t = bc.script_tables(frames, S, rows, 16, rng)
    assert t["counts"].max() >= 5 and len(set(t["counts"][-1].tolist())) > 1
    o = dict(entries=5, min_hits=2, terms=7, fx=1.5, fy=0.75)
    every = check_sequence(dict(t, collect=np.ones((F,), np.uint8), cap=2), o)
    assert every["pending"].any() and every["offer_flags"].any() and every["flags"].any()
    last = np.zeros((F,), np.uint8)
    last[-1] = 2
    end = check_sequence(dict(t, collect=last, cap=5), o)
    assert end["counts"][-1].min() >= 3 and not end["pending"][-1].any()
    # chip_counts below the counts: the rows past them have no chip
    cc = np.maximum(t["counts"] - rng.integers(0, 3, t["counts"].shape), 0).astype(np.int32)
    cut = check_sequence(dict(t, collect=last, cap=5, chip_counts=cc), o)
    assert (cut["offer_quality"] != end["offer_quality"]).any()


def test_rows_and_entries_that_cross_a_wave():
    """70 rows and 130 entries: ids come and go 35 at a time, so that row ranks, entry ranks, the free list and the seqs all pass 64, and
    the table overflows once."""
    rows, E = 70, 130
    frames = [[[R(tid, (tid * 7 + f) % 12 + 1, hits=2 + f) for tid in range(1 + 35 * f, 71 + 35 * f)][::-1 if f % 2 else 1]] for f in range(4)]
    t = bc.script_tables(frames, 1, rows, 16)
    got = check_sequence(dict(t, collect=np.array([0, 0, 1, 2], np.uint8), cap=E), dict(entries=E, terms=0))
    assert got["offer_flags"][:, 0].tolist() == [0, 0, 1, 0] and got["counts"][:, 0].tolist() == [0, 0, 70, 105]
    assert got["records"][2, 0, :70, 7].tolist() == list(range(70))


# ---------------------------------------------------------------------------------------------- behind an engine
def _info(g):
    return np.stack([g[2], g[3], g[4]], axis=1).astype(np.int32)


def _ref_offer(ref, got, chips, offs):
    q = []
    for b, g in enumerate(got):
        m = int(offs[b + 1] - offs[b])
        qb, _ = ref.offer(b, g[0][:, :4], g[0][:, 4], g[1], _info(g), len(g[0]), chips[offs[b]:offs[b + 1]])
        q.append(qb[:m])
    return np.concatenate(q) if q else np.zeros((0,), np.int64)


def _same_collect(got, ref, B, cap, flush=False):
    chips, quality, records, dets, lms, counts, pending, flags = got
    total = 0
    for b in range(B):
        want, wp, wf = ref.collect(b, cap, flush)
        assert (counts[b], pending[b], flags[b]) == (len(want), wp, wf), b
        for k, e in enumerate(want):
            assert quality[b, k] == e.Q and records[b, k].tolist() == e.record()
            assert chips[b, k].tobytes() == e.chip.tobytes() and dets[b, k].tobytes() == e.det.tobytes() and lms[b, k].tobytes() == e.lms.tobytes()
        total += len(want)
    return total


def test_engine_offers_tracked_chips_and_collects_the_finished_ones():
    rng, E = np.random.default_rng(3), 16
    eng, eng2 = (cfa.Engine(64, 96, max_batch=3, dtype="bf16") for _ in range(2))
    topts = dict(iou=0.3, max_age=0, min_hits=1, max_tracks=70)
    trk, trk2 = cfa.Tracker(eng, 3, **topts), cfa.Tracker(eng2, 3, **topts)
    sopts = dict(size=16, entries=E, min_hits=1)
    shots, twin, third = (cfa.BestShots(eng, 3, **sopts) for _ in range(3))
    src, base = _feed_until_faces(eng, rng)
    h, w = src.shape[1:3]
    ref = RefBestShots(3, entries=E, min_hits=1, terms=7, fx=float(w) / 96.0, fy=float(h) / 64.0)
    chips, offs, _ = eng.align_faces_frame(src, "bgr", size=16)
    _state_error(lambda: eng.bestshot_offer(shots, chips, offs, (h, w)))    # no update behind the decode: the rows have no ids
    got, _ = eng.track_update(trk)
    chips, offs, _ = eng.align_faces_frame(src, "bgr", size=16)
    assert len(chips) == sum(len(g[0]) for g in got) >= 2
    before = src.copy()
    eng.redact_faces(before, "bgr", mode="mosaic", shape="ellipse", cell=6)
    q, fl = eng.bestshot_offer(shots, chips, offs, (h, w))
    assert q.tolist() == _ref_offer(ref, got, chips, offs).tolist() and not fl.any() and (q >= 0).all()
    after = src.copy()
    eng.redact_faces(after, "bgr", mode="mosaic", shape="ellipse", cell=6)  # the offer changed no state of the context
    assert np.array_equal(after, before) and not np.array_equal(after, src)
    # the device form, into a twin table
    n = len(chips)
    dev = [eng.device_alloc(max(x, 16)) for x in (chips.nbytes, offs.nbytes, n * 8, 3 * 4)]
    eng.memcpy_h2d(dev[0], chips), eng.memcpy_h2d(dev[1], offs)
    eng.bestshot_offer_device(twin, dev[0], dev[1], n, 3, (h, w), 0, dev[2], dev[3])
    eng.bestshot_offer_device(third, dev[0], dev[1], n, 3, (h, w))          # (and a third, without outputs)
    q2, fl2 = np.empty((n,), np.int64), np.empty((3,), np.int32)
    eng.synchronize()
    eng.memcpy_d2h(q2, dev[2]), eng.memcpy_d2h(fl2, dev[3])
    assert q2.tolist() == q.tolist() and fl2.tolist() == fl.tolist()
    with pytest.raises(ValueError):
        eng.bestshot_offer(shots, chips, offs, (h, w), stream0=1)           # streams 1 .. 3 of a table with 3
    with pytest.raises(ValueError):
        eng.bestshot_offer(shots, chips, offs[:3], (h, w))                  # B = 2, the rows are of 3 images
    with pytest.raises(ValueError):
        eng.bestshot_offer_device(shots, dev[0] + 4, dev[1], n, 3, (h, w))  # chips not 16-byte aligned
    # a second context offers to the same table: its tracker hands out the same ids, so its offer lands in the entries of the first
    eng2.forward_resized_enqueue(src)
    eng2.decode_threshold(0.3, 0.3, 64)
    got2, _ = eng2.track_update(trk2)
    chips2, offs2, _ = eng2.align_faces_frame(src, "bgr", size=16)
    q3, _ = eng2.bestshot_offer(shots, chips2, offs2, (h, w))
    assert q3.tolist() == _ref_offer(ref, got2, chips2, offs2).tolist()
    assert sum(e.n_offered == 2 for tab in ref.tab for e in tab) >= 2
    # a blank batch: max_age = 0 frees every track, the ids are gone, the entries finish
    assert sum(len(d) for d, _ in _blank_batch(eng)) == 0
    got, _ = eng.track_update(trk)
    assert sum(len(g[0]) for g in got) == 0
    chips0, offs0, _ = eng.align_faces_frame(src, "bgr", size=16)
    assert chips0.shape == (0, 16, 16, 3) and offs0.tolist() == [0, 0, 0, 0]
    q0, _ = eng.bestshot_offer(shots, chips0, offs0, (h, w))
    assert len(q0) == 0 and len(_ref_offer(ref, got, chips0, offs0)) == 0
    assert _same_collect(eng.bestshot_collect(shots, cap=1), ref, 3, 1) >= 1
    assert _same_collect(eng.bestshot_collect(shots), ref, 3, E) >= 1
    # the twin and the third still hold their entries alive: the device form of a flushing collect equals the host form
    host = eng.bestshot_collect(third, flush=True)
    sizes = (3 * E * 768, 3 * E * 8, 3 * E * 32, 3 * E * 20, 3 * E * 40, 12, 12, 12)
    out = [eng.device_alloc(x) for x in sizes]
    eng.bestshot_collect_device(twin, 0, 3, E, True, *out)
    eng.synchronize()
    back = [np.zeros_like(a) for a in host]
    for a, p in zip(back, out):
        eng.memcpy_d2h(a, p)
    assert host[5].sum() >= 2 and back[5].tolist() == host[5].tolist() and back[6].tolist() == host[6].tolist()
    for b in range(3):
        for a, x in zip(back[:5], host[:5]):
            assert a[b, :host[5][b]].tobytes() == x[b, :host[5][b]].tobytes()
    for p in dev + out:
        eng.device_free(p)
    for x in (shots, twin, third, trk, trk2, eng, eng2):
        x.close()


def test_best_shots_over_two_chunks_equals_the_calls_by_hand():
    rng = np.random.default_rng(17)
    faces, tried = {}, []
    for kind, hw in SOURCES:
        if hw not in faces:                                                  # best_shots takes frames of the size the instance was built for
            for old in list(faces):
                for f in faces.pop(old):
                    f.close()
            faces[hw] = [cfa.CenterFace(*hw, dtype="bf16", max_batch=2) for _ in range(2)]
        face, face2 = faces[hw]
        frames = source_frames(rng, kind, (3,) + hw + (3,))
        n = [len(d) for d, _ in face.detect_batch(list(frames))]
        tried.append((kind, hw, n))
        if sum(n) >= 2 and n[2] >= 1:
            break
    else:
        raise AssertionError("no source holds two faces, one of them behind the first chunk, with the default weights: %s" % tried)
    topts, sopts = dict(min_hits=1, max_age=0), dict(size=16, entries=16, min_hits=1)
    trk, trk2 = cfa.Tracker(face.engine, 3, **topts), cfa.Tracker(face2.engine, 3, **topts)
    shots, shots2 = cfa.BestShots(face.engine, 3, **sopts), cfa.BestShots(face2.engine, 3, **sopts)
    eng = face2.engine

    def by_hand(batch, flush):
        eng.set_rescale(face2.scale_h, face2.scale_w)
        for i in range(0, 3, 2):
            eng.forward_resized_enqueue(batch[i:i + 2])
            eng.decode_threshold(0.3, face2.nms_thresh, face2.max_dets)
            eng.track_update_device(trk2, i)
            cut, offs, _ = eng.align_faces_frame(batch[i:i + 2], "bgr", 16)
            eng.bestshot_offer(shots2, cut, offs, batch.shape[1:3], i)
        eng.set_rescale(0.0, 0.0)
        return eng.bestshot_collect(shots2, 0, 3, flush=flush)

    blank = np.full_like(frames, 128)
    total = 0
    for batch, flush in ((frames, False), (frames, False), (blank, False), (frames, True)):
        got = face.best_shots(batch, tracker=trk, shots=shots, flush=flush)
        chips, quality, records, dets, lms, counts = by_hand(batch, flush)[:6]
        assert [len(g) for g in got] == counts.tolist()
        for s, lst in enumerate(got):
            for k, d in enumerate(lst):
                assert (d["id"], d["quality"]) == (records[s, k, 0], quality[s, k]) and d["record"].tolist() == records[s, k].tolist()
                assert d["chip"].tobytes() == chips[s, k].tobytes() and d["det"].tobytes() == dets[s, k].tobytes() and d["lms"].tobytes() == lms[s, k].tobytes()
        total += int(counts.sum())
    assert total >= 2                                                       # the flush of the last call, if nothing else, finished them
    for x in (shots, shots2, trk, trk2, face, face2):
        x.close()
