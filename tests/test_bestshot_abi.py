"""The best-shot table's C ABI and Python binding, the hand-checked cases of its numpy restatement, and the calls CenterFace.best_shots
asks of its engine (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
import bestshot_cases as bc
from bestshot_cases import RefBestShots, quality_ref
import test_product_paths as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "centerface_hip.h")).read()
SYMBOLS = ("cf_bestshot_create", "cf_bestshot_destroy", "cf_bestshot_offer", "cf_bestshot_collect", "cf_op_chip_quality", "cf_op_bestshot")


def test_symbols_exported_declared_and_bound():
    L = cfa._lib.lib()
    for s in SYMBOLS:
        assert s in cfa._lib.EXPORTS
        assert re.search(r"\bint %s\(" % s, HEADER), s
        assert hasattr(L, s) and getattr(L, s).argtypes, s
    assert L.cf_version() == 100
    assert callable(cfa.ops.chip_quality) and callable(cfa.ops.bestshot_sequence)
    for name in ("bestshot_offer", "bestshot_offer_device", "bestshot_collect", "bestshot_collect_device"):
        assert callable(getattr(cfa.Engine, name))
    assert callable(cfa.CenterFace.best_shots) and callable(cfa.BestShots.close)


def test_opts_and_terms_agree_with_the_header():
    body = re.search(r"typedef struct cf_bestshot_opts \{(.*?)\} cf_bestshot_opts;", HEADER, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t)\s+(\w+);", body, re.M)
    assert [(n, C.c_int32) for _, n in fields] == list(cfa._lib.BestShotOpts._fields_)
    assert [n for _, n in fields] == ["size", "entries", "min_hits", "terms"]
    assert C.sizeof(cfa._lib.BestShotOpts) == 16
    assert C.sizeof(cfa._lib.TrackOpts) == 20 and C.sizeof(cfa._lib.RedactOpts) == 20 and C.sizeof(cfa._lib.FollowOpts) == 8      # the others kept their size
    for name, value in (("SIZE", 1), ("POSE", 2), ("SCORE", 4)):
        assert re.search(r"^#define CF_BEST_%s\s+%d\s*$" % (name, value), HEADER, re.M), name
        assert getattr(cfa._lib, "CF_BEST_" + name) == value and getattr(bc, name) == value
    o = cfa._lib.bestshot_opts()
    assert (o.size, o.entries, o.min_hits, o.terms) == (112, 320, 2, 7)
    assert cfa._lib.bestshot_opts(terms=("pose",)).terms == 2 and cfa._lib.bestshot_opts(terms=()).terms == 0 and cfa._lib.bestshot_opts(terms=5).terms == 5
    with pytest.raises(ValueError):
        cfa._lib.bestshot_opts(terms=("sharp",))
    # the statement is in the header
    for phrase in ("Quality of one chip", "One offer of stream s", "Collect of stream s", "no accuracy claim"):
        assert phrase in HEADER, phrase


def test_makefile_builds_the_kernel_without_fma_contraction():
    mk = open(os.path.join(ROOT, "lightweight-face-detection-centernet_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "cf_bestshot.hip" in srcs
    assert re.search(r"^EXTRA_cf_bestshot\s*=\s*-ffp-contract=off\s*$", mk, re.M)


# ---------------------------------------------------------------------------------------------- refusals
def _why():
    return (cfa._lib.lib().cf_op_last_error() or b"").decode()


def _quality(opts=(16, 1, 2, 7), n=2, fx=1.0, fy=1.0, null=None, null_opts=False):
    a = dict(chips=np.zeros((max(n, 1), opts[0], opts[0], 3), np.uint8), boxes=np.zeros((max(n, 1), 4), np.float32), scores=np.zeros((max(n, 1),), np.float32),
             lms=np.zeros((max(n, 1), 10), np.float32), quality=np.full((max(n, 1),), 9, np.int64), parts=np.full((max(n, 1), 4), 9, np.int32))
    if null:
        a[null] = None
    P = cfa._lib.ptr
    o = cfa._lib.BestShotOpts(*opts)
    r = cfa._lib.lib().cf_op_chip_quality(0, None if null_opts else C.byref(o), P(a["chips"]), P(a["boxes"]), P(a["scores"]), P(a["lms"]), n, fx, fy,
                                          P(a["quality"]), P(a["parts"]))
    for k in ("quality", "parts"):
        assert a[k] is None or (a[k] == 9).all(), k
    return r, _why()


def test_chip_quality_refuses_bad_arguments_before_any_device():
    for kw, word in ((dict(opts=(15, 1, 2, 7)), "size"), (dict(opts=(18, 1, 2, 7)), "size"), (dict(opts=(516, 1, 2, 7)), "size"), (dict(opts=(12, 1, 2, 7)), "size"),
                     (dict(opts=(16, 0, 2, 7)), "entries"), (dict(opts=(16, 2049, 2, 7)), "entries"), (dict(opts=(16, 1, 0, 7)), "min_hits"),
                     (dict(opts=(16, 1, 1001, 7)), "min_hits"), (dict(opts=(16, 1, 2, 8)), "terms"), (dict(opts=(16, 1, 2, -1)), "terms"),
                     (dict(n=0), "n must be"), (dict(n=65537), "n must be"), (dict(fx=0.0), "fx and fy"), (dict(fy=float("nan")), "fx and fy"),
                     (dict(fx=float("inf")), "fx and fy"), (dict(fy=-1.0), "fx and fy"), (dict(null_opts=True), "null options")):
        r, why = _quality(**kw)
        assert r == -1 and "cf_op_chip_quality" in why and word in why, (kw, why)
    for k in ("chips", "boxes", "scores", "lms", "quality", "parts"):
        r, why = _quality(null=k)
        assert r == -1 and "null argument" in why, (k, why)


ORDER_IN = ("boxes", "scores", "lms", "info", "counts", "chip_counts", "chips", "collect")
ORDER_OUT = ("out_chips", "out_quality", "out_records", "out_dets", "out_lms", "out_counts", "out_pending", "out_flags", "offer_flags", "offer_quality")


def _sequence(opts=(16, 4, 2, 7), S=2, F=2, rows=3, cap=4, fx=1.0, fy=1.0, null=None, null_opts=False, edit=None):
    Sz, k = opts[0], max(cap, 1)
    a = dict(boxes=np.zeros((F, S, rows, 4), np.float32), scores=np.zeros((F, S, rows), np.float32), lms=np.zeros((F, S, rows, 10), np.float32),
             info=np.ones((F, S, rows, 3), np.int32), counts=np.ones((F, S), np.int32), chip_counts=np.ones((F, S), np.int32),
             chips=np.zeros((F, S, rows, Sz, Sz, 3), np.uint8), collect=np.ones((F,), np.uint8),
             out_chips=np.full((F, S, k, Sz, Sz, 3), 9, np.uint8), out_quality=np.full((F, S, k), 9, np.int64), out_records=np.full((F, S, k, 8), 9, np.int32),
             out_dets=np.full((F, S, k, 5), 9, np.float32), out_lms=np.full((F, S, k, 10), 9, np.float32), out_counts=np.full((F, S), 9, np.int32),
             out_pending=np.full((F, S), 9, np.int32), out_flags=np.full((F, S), 9, np.int32), offer_flags=np.full((F, S), 9, np.int32),
             offer_quality=np.full((F, S, rows), 9, np.int64))
    if edit:
        edit(a)
    if null:
        a[null] = None
    P = cfa._lib.ptr
    o = cfa._lib.BestShotOpts(*opts)
    r = cfa._lib.lib().cf_op_bestshot(0, None if null_opts else C.byref(o), S, F, rows, *[P(a[k]) for k in ORDER_IN], cap, fx, fy, *[P(a[k]) for k in ORDER_OUT])
    for k in ORDER_OUT:                                                   # refused: nothing was written
        assert a[k] is None or (a[k] == 9).all(), k
    return r, _why()


def test_sequence_refuses_bad_arguments_before_any_device():
    def neg(key):
        def edit(a):
            a[key][1, 0] = -1
        return edit

    def collect3(a):
        a["collect"][1] = 3
    for kw, word in ((dict(opts=(18, 4, 2, 7)), "size"), (dict(opts=(16, 0, 2, 7)), "entries"), (dict(opts=(16, 4, 0, 7)), "min_hits"), (dict(opts=(16, 4, 2, 9)), "terms"),
                     (dict(S=0), "n_streams"), (dict(S=4097), "n_streams"), (dict(F=0), "n_frames"), (dict(rows=0), "rows"), (dict(rows=1025), "rows"),
                     (dict(cap=-1), "cap"), (dict(cap=5), "cap"), (dict(fx=0.0), "fx and fy"), (dict(fy=float("nan")), "fx and fy"),
                     (dict(null_opts=True), "null options"), (dict(edit=neg("counts")), "negative count"), (dict(edit=neg("chip_counts")), "negative count"),
                     (dict(edit=collect3), "collect must be")):
        r, why = _sequence(**kw)
        assert r == -1 and "cf_op_bestshot" in why and word in why, (kw, why)
    for k in ORDER_IN + ORDER_OUT:
        r, why = _sequence(null=k)
        assert r == -1 and "null argument" in why, (k, why)
    with pytest.raises(ValueError):
        cfa.ops.bestshot_sequence(np.zeros((2, 2, 3, 5), np.float32), 0, 0, 0, 0, np.zeros((2, 2, 3, 16, 16, 3), np.uint8), [0, 1])
    with pytest.raises(ValueError):
        cfa.ops.bestshot_sequence(np.zeros((2, 2, 3, 4), np.float32), 0, 0, 0, 0, np.zeros((2, 2, 3, 16, 12, 3), np.uint8), [0, 1])
    with pytest.raises(ValueError):
        cfa.ops.chip_quality(np.zeros((2, 16, 12, 3), np.uint8), 0, 0, 0)


def test_create_and_offer_check_their_arguments_before_the_context():
    L = cfa._lib.lib()
    out = C.c_void_p()
    for opts, streams, word in (((18, 4, 2, 7), 1, "size"), ((16, 2049, 2, 7), 1, "entries"), ((16, 4, 1001, 7), 1, "min_hits"), ((16, 4, 2, 8), 1, "terms"),
                                ((16, 4, 2, 7), 0, "n_streams"), ((16, 4, 2, 7), 4097, "n_streams")):
        o = cfa._lib.BestShotOpts(*opts)
        assert L.cf_bestshot_create(None, streams, C.byref(o), C.byref(out)) == -1
        assert "cf_bestshot_create" in _why() and word in _why() and "null context" not in _why(), _why()
        with pytest.raises(ValueError):
            cfa.BestShots(0, streams, *opts)
    o = cfa._lib.bestshot_opts()
    assert L.cf_bestshot_create(None, 1, None, C.byref(out)) == -1 and "null options" in _why()
    assert L.cf_bestshot_create(None, 1, C.byref(o), None) == -1 and "null out" in _why()
    assert L.cf_bestshot_create(None, 1, C.byref(o), C.byref(out)) == -1 and "null context" in _why()
    assert out.value is None
    shots = cfa.BestShots(0, 3, size=16, entries=4, terms=("pose",))      # a device index: nothing is created yet
    assert (shots.streams, shots.size, shots.entries, shots._o.terms, shots._h) == (3, 16, 4, 2, None)
    shots.close()
    assert L.cf_bestshot_destroy(None) == 0
    chips, offs = np.zeros((1, 16, 16, 3), np.uint8), np.zeros((2,), np.int32)
    P = cfa._lib.ptr
    table = C.c_void_p(4096)
    for args, word in (((None, 0, 1, P(chips), P(offs), 1, 0, 64, 64), "null table"), ((table, 0, 1, None, P(offs), 1, 0, 64, 64), "null chips"),
                       ((table, 0, 1, P(chips), None, 1, 0, 64, 64), "null chips or offsets"), ((table, 0, 1, P(chips), P(offs), -1, 0, 64, 64), "cap_faces"),
                       ((table, 0, 0, P(chips), P(offs), 1, 0, 64, 64), "B must be"), ((table, 0, 1, P(chips), P(offs), 1, 0, 1, 64), "h and w"),
                       ((table, 0, 1, P(chips), P(offs), 1, 0, 64, 8193), "h and w"), ((table, 0, 1, C.c_void_p(4104), P(offs), 1, 1, 64, 64), "16-byte aligned"),
                       ((table, 0, 1, P(chips), P(offs), 1, 0, 64, 64), "null context")):
        q, fl = np.full((1,), 9, np.int64), np.full((1,), 9, np.int32)
        assert L.cf_bestshot_offer(None, *args, P(q), P(fl), 0) == -1
        assert "cf_bestshot_offer" in _why() and word in _why(), (word, _why())
        assert q[0] == 9 and fl[0] == 9
    assert L.cf_bestshot_collect(None, table, 0, 1, 1, 0, None, None, None, None, None, None, None, None, 0) == -1


# ---------------------------------------------------------------------------------------------- the restatement, checked by hand
ROW = (np.array([10, 10, 30, 30], np.float32), np.float32(0.75), bc.frontal())


@pytest.mark.parametrize("S", bc.SIZES)
def test_restatement_sharpness_of_flat_stripes_and_checkerboard(S):
    assert bc.sharpness(bc.flat_chip(S)) == 0
    assert bc.sharpness(bc.stripes_chip(S, 10)) == 400 and bc.sharpness(bc.stripes_chip(S, 3, tag=7)) == 36
    assert bc.sharpness(bc.checker_chip(S)) == 1040400
    # colour: the luma weights, and the window only -- whatever lies outside rows and columns a - 1 .. b is not looked at
    c = bc.stripes_chip(S, 10)
    c[: S // 4 - 1], c[:, 3 * S // 4 + 1:] = 255, 0
    assert bc.sharpness(c) == 400
    c = bc.flat_chip(S)
    c[:, 1::2] = (0, 0, 255)                                               # L = 93 | (77 * 255 + 128) >> 8 = 77: lap = -+32
    assert bc.sharpness(c) == 32 * 32


def test_restatement_blur_lowers_the_sharpness():
    rng = np.random.default_rng(0)
    grey = np.repeat(rng.integers(0, 256, (112, 112, 1), dtype=np.uint8), 3, axis=2)
    got = [bc.sharpness(bc.box_blur(grey, k)) for k in (0, 1, 2, 4, 8)]
    assert all(a > 2 * b for a, b in zip(got, got[1:])) and got == sorted(got, reverse=True) and got[0] > 100000 and got[-1] < 100, got


def test_restatement_weights_at_their_edges():
    size = lambda box, fx=1.0, fy=1.0, S=16: bc.size_weight(np.array(box, np.float32), fx, fy, S)      # noqa: E731
    assert size((10, 10, 10, 30)) == 0 and size((10, 10, 9, 30)) == 0 and size((10, 10, 30, 10)) == 0          # side 0 or less
    assert size((10, 10, 26, 30)) == 256 and size((10, 10, 4000, 4000)) == 256 and size((10, 10, float("inf"), 40)) == 256      # side >= S
    assert size((10, 10, 18.5, 40)) == 8 * 256 // 16 and size((10, 10, 25.99, 40)) == 15 * 256 // 16
    assert size((float("nan"), 10, 30, 30)) == 0 and size((10, 10, 30, float("nan"))) == 0
    assert size((10, 10, 14, 40), 3.0, 1.6875) == 12 * 256 // 16 and size((10, 10, 40, 14), 3.0, 1.6875) == 6 * 256 // 16      # 4 * 3 | 4 * 1.6875 = 6.75
    assert size((0, 0, 50, 50), S=112) == 50 * 256 // 112
    assert bc.pose_weight(bc.frontal(0.0), 1.0, 1.0) == 256                 # the nose on the axis
    assert bc.pose_weight(bc.frontal(10.0), 1.0, 1.0) == 0 and bc.pose_weight(bc.frontal(-10.0), 1.0, 1.0) == 0      # offset 0.5 of a 20-pixel axis
    assert bc.pose_weight(bc.frontal(5.0), 1.0, 1.0) == 128 and bc.pose_weight(bc.frontal(-2.5), 1.0, 1.0) == 192
    assert bc.pose_weight(bc.frontal(5.0), 2.0, 1.0) == 0                   # anisotropic frames: x doubles, the axis does not
    assert bc.pose_weight(np.array([30, 30, 50, 30, 40, 40, 30, 30, 50, 30], np.float32), 1.0, 1.0) == 0      # eyes and mouth coincide
    for bad in (float("nan"), float("inf")):
        l = bc.frontal()
        l[7] = bad
        assert bc.pose_weight(l, 1.0, 1.0) == 0
    assert [bc.score_weight(np.float32(v)) for v in (0.0, -0.5, 0.5, 1.0, 7.5, float("nan"), 0.999)] == [0, 0, 128, 256, 256, 0, 255]
    chip = bc.stripes_chip(16, 10)
    assert quality_ref(chip, *ROW) == (400 * 256 * 256 * 192, (400, 256, 256, 192))
    assert quality_ref(chip, *ROW, terms=0) == (400 << 24, (400, 256, 256, 256))
    assert quality_ref(chip, np.array([10, 10, 18, 30], np.float32), ROW[1], bc.frontal(5.0), terms=3) == (400 * 128 * 128 * 256, (400, 128, 128, 256))
    assert quality_ref(chip, ROW[0], np.float32(0), ROW[2])[0] == 0


def _run(name):
    t, o = bc.script_args(name)
    return bc.run_ref(**t, **o), t


def _rec(r, f, s=0):
    return r["records"][f, s, :r["counts"][f, s]].tolist()


def test_restatement_a_tie_keeps_the_earlier_frame():
    r, t = _run("tie")
    assert r["counts"][:, 0].tolist() == [0, 0, 0, 0, 0, 1] and not r["pending"].any() and not r["flags"].any() and not r["offer_flags"].any()
    # id 1: best at t = 3 (the first of the two d = 7 frames), seen 0 .. 4, offered 5 times, sharp 4 * 49, all weights 256, seq 0
    assert _rec(r, 5) == [[1, 3, 0, 4, 5, 196, 256 | 256 << 10 | 256 << 20, 0]]
    assert r["quality"][5, 0, 0] == 196 << 24 and r["chips"][5, 0, 0, 0, 0, 0] == 3 and r["chips"][5, 0, 0].tobytes() == t["chips"][3, 0, 0].tobytes()
    assert r["dets"][5, 0, 0].tolist() == [10, 10, 30, 30, 0.75] and r["lms"][5, 0, 0].tobytes() == bc.frontal().tobytes()
    assert r["offer_quality"][:, 0, 0].tolist() == [100 << 24, 100 << 24, 36 << 24, 196 << 24, 196 << 24, -1]
    assert (r["offer_quality"][:, 0, 1] == -1).all()


def test_restatement_a_held_row_keeps_its_entry_alive_but_is_not_offered():
    r, _ = _run("held")
    assert r["offer_quality"][:, 0, 0].tolist() == [100 << 24, -1, -1, 64 << 24, -1, -1]
    assert _rec(r, 5) == [[1, 0, 0, 3, 2, 100, 256 | 256 << 10 | 256 << 20, 0]]


def test_restatement_a_vanished_id_is_done_in_the_next_offer():
    r, _ = _run("vanish")
    assert r["counts"][:, 0].tolist() == [0, 0, 3, 1] and r["pending"][:, 0].tolist() == [0, 0, 0, 0]
    assert [x[0] for x in _rec(r, 2)] == [1, 2, 3] and [x[7] for x in _rec(r, 2)] == [0, 1, 2]      # 1 in frame 1; 2 and 3 in frame 2, in entry order
    assert [x[3] for x in _rec(r, 2)] == [0, 1, 1]
    assert _rec(r, 3) == [[4, 2, 0, 2, 3, 36, 256 | 256 << 10 | 256 << 20, 3]]


def test_restatement_a_full_table_flags_the_row_and_it_enters_later():
    r, _ = _run("full")
    assert r["offer_flags"][:, 0].tolist() == [1, 1, 1, 0, 0]              # a DONE entry is not free: id 3 waits for the collect
    assert r["offer_quality"][2, 0, :2].tolist() == [144 << 24, 256 << 24]      # it was scored all the same
    assert r["flags"][:, 0].tolist() == [0, 0, 1, 0, 0] and r["counts"][:, 0].tolist() == [0, 0, 1, 0, 2]
    assert _rec(r, 2) == [[1, 0, 0, 0, 1, 100, 256 | 256 << 10 | 256 << 20, 0]]
    assert _rec(r, 4) == [[3, 3, 3, 3, 1, 64, 256 | 256 << 10 | 256 << 20, 1], [2, 0, 0, 3, 4, 144, 256 | 256 << 10 | 256 << 20, 2]]      # id 3 sits in entry 0


def test_restatement_collect_below_the_done_count_leaves_pending_in_seq_order():
    r, _ = _run("cap")
    assert r["counts"][:, 0].tolist() == [0, 0, 2, 2, 1] and r["pending"][:, 0].tolist() == [0, 0, 3, 1, 0]
    assert [x[0] for f in (2, 3, 4) for x in _rec(r, f)] == [2, 4, 1, 3, 5] and [x[7] for f in (2, 3, 4) for x in _rec(r, f)] == [0, 1, 2, 3, 4]


def test_restatement_flush_finishes_the_live_entries():
    r, _ = _run("flush")
    assert [x[0] for x in _rec(r, 2)] == [2, 1, 3] and [x[7] for x in _rec(r, 2)] == [0, 1, 2] and [x[1] for x in _rec(r, 2)] == [0, 2, 0]
    ref = RefBestShots(1, entries=2, terms=0)
    assert ref.collect(0, 2, True) == ([], 0, 0) and ref.t == [0] and ref.seq == [0]


def test_restatement_reuse_and_duplicates():
    r, _ = _run("reuse")
    assert [_rec(r, f) for f in range(4)][1][0][:4] == [1, 0, 0, 0] and [x[0] for x in _rec(r, 3)] == [3, 4] and r["counts"][:, 0].tolist() == [0, 1, 1, 2]
    r, _ = _run("dups")
    assert r["offer_quality"][0, 0, :5].tolist() == [100 << 24, -1, -1, -1, 64 << 24] and r["offer_quality"][1, 0, :4].tolist() == [64 << 24, -1, -1, -1]
    assert sorted(x[0] for x in _rec(r, 2)) == [1, 2] and [x[4] for x in sorted(_rec(r, 2))] == [1, 2]


# ---------------------------------------------------------------------------------------------- CenterFace.best_shots
SHOTS = type("Shots", (), {"size": 16, "streams": 8, "entries": 4})()


class BestEngine(pp.StubEngine):
    def bestshot_offer(self, shots, chips, offsets, hw, stream0=0):
        self._log("bestshot_offer", shots is SHOTS, chips.shape, chips[:, 0, 0, 0].tolist(), np.asarray(offsets).tolist(), tuple(hw), stream0)
        return np.zeros((len(chips),), np.int64), np.zeros((len(offsets) - 1,), np.int32)

    def bestshot_collect(self, shots, stream0=0, B=None, cap=None, flush=False):
        self._log("bestshot_collect", shots is SHOTS, stream0, B, cap, flush)
        k = 2
        chips = (np.arange(B * k, dtype=np.uint8).reshape(B, k, 1, 1, 1) + np.zeros((1, 1, 16, 16, 3), np.uint8)).astype(np.uint8)
        quality, records = 100 + np.arange(B * k, dtype=np.int64).reshape(B, k), np.arange(B * k * 8, dtype=np.int32).reshape(B, k, 8)
        dets, lms = np.arange(B * k * 5, dtype=np.float32).reshape(B, k, 5), np.arange(B * k * 10, dtype=np.float32).reshape(B, k, 10)
        return chips, quality, records, dets, lms, np.array([1, 0, 2][:B], np.int32), np.zeros((B,), np.int32), np.zeros((B,), np.int32)


@pytest.mark.parametrize("flush", (False, True))
def test_best_shots_issues_exactly_these_calls_over_two_chunks(flush):
    script = pp.Script()
    face = pp.make_face((pp.H, pp.W), BestEngine(script))
    frames = np.zeros((3,) + pp.BGR, np.uint8)
    got = face.best_shots(frames, tracker=pp.TRK, shots=SHOTS, flush=flush, template=None)
    per = pp.BGR
    want = [("set_rescale",) + pp.S_BGR,
            ("forward_resized_enqueue", pp.chunk(0, 2, per, "frames")), ("decode_threshold", 0.3, pp.NMS, pp.MAXD), ("track_update_device", True, 0),
            ("align_faces_frame", pp.chunk(0, 2, per, "frames"), "bgr", 16, dict(template=None)),
            ("bestshot_offer", True, (2, 16, 16, 3), [0, 1], [0, 2, 2], (pp.H, pp.W), 0),
            ("forward_resized_enqueue", pp.chunk(2, 1, per, "frames")), ("decode_threshold", 0.3, pp.NMS, pp.MAXD), ("track_update_device", True, 2),
            ("align_faces_frame", pp.chunk(2, 1, per, "frames"), "bgr", 16, dict(template=None)),
            ("bestshot_offer", True, (1, 16, 16, 3), [2], [0, 1], (pp.H, pp.W), 2),
            ("bestshot_collect", True, 0, 3, None, flush), ("set_rescale", 0.0, 0.0)]
    assert [e[1:] for e in pp.resolve(script.log, dict(frames=frames))] == want
    assert [len(s) for s in got] == [1, 0, 2]
    assert got[0][0]["id"] == 0 and got[0][0]["quality"] == 100 and got[0][0]["chip"].shape == (16, 16, 3) and got[0][0]["record"].tolist() == list(range(8))
    assert [d["id"] for d in got[2]] == [32, 40] and [d["quality"] for d in got[2]] == [104, 105] and got[2][1]["det"].tolist() == [25, 26, 27, 28, 29]
    assert got[2][1]["lms"].tolist() == list(range(50, 60)) and (got[2][1]["chip"] == 5).all()
    assert sorted(got[2][0]) == ["chip", "det", "id", "lms", "quality", "record"]
    with pytest.raises(ValueError):
        face.best_shots(frames, tracker=None, shots=SHOTS)
    with pytest.raises(ValueError):
        face.best_shots(frames[:, :10], tracker=pp.TRK, shots=SHOTS)


@pytest.mark.parametrize("how", ("tiled", "fit"))
def test_best_shots_tiled_and_fitted_collect_once_after_the_last_chunk(how):
    """The chips are cut from the frames behind the merge (the unfit) and the update of every chunk; ONE collect over streams 0 .. n stands
    after the last chunk, and nothing rescales."""
    script = pp.Script()
    face = pp.make_face((pp.YH, pp.YW), BestEngine(script))
    n, per = 3, pp.BGR_EVEN
    frames = np.zeros((n,) + per, np.uint8)
    got = face.best_shots(frames, tracker=pp.TRK, shots=SHOTS, **({"tiled": True} if how == "tiled" else {"fit": dict(anchor="topleft")}))
    rects = tuple(map(tuple, pp.ops.tile_grid(pp.YH, pp.YW, (pp.NH, pp.NW), 24, True).tolist()))
    step = pp.NB // len(rects) if how == "tiled" else pp.NB
    want = []
    for i in range(0, n, step):
        b = min(step, n - i)
        part, faces = pp.chunk(i, b, per, "frames"), list(pp.COUNTS[i:i + b])
        if how == "tiled":
            want += [("forward_tiles_enqueue", part, rects, "bgr"), ("decode_threshold", 0.3, pp.NMS, pp.MAXD), ("merge_tiles", "ios", 0.5, 2.0, pp.MAXD)]
        else:
            want += [("forward_fit_enqueue", part, "bgr", dict(pp.FIT, anchor="topleft")), ("decode_threshold", 0.3, pp.NMS, pp.MAXD), ("unfit_rows", pp.MAXD)]
        ids = list(range(sum(pp.COUNTS[:i]), sum(pp.COUNTS[:i + b])))
        want += [("track_update_device", True, i), ("align_faces_frame", part, "bgr", 16, dict(template=None)),
                 ("bestshot_offer", True, (len(ids), 16, 16, 3), ids, np.concatenate([[0], np.cumsum(faces)]).tolist(), (pp.YH, pp.YW), i)]
    want += [("bestshot_collect", True, 0, n, None, False)]
    log = [e[1:] for e in pp.resolve(script.log, dict(frames=frames))]
    assert log == want
    assert [e[0] for e in log].count("bestshot_collect") == 1 and log[-1][0] == "bestshot_collect" and not frames.any()
    assert [len(s) for s in got] == [1, 0, 2]


def test_drive_without_best_issues_no_bestshot_call():
    script = pp.Script()
    face = pp.make_face((pp.H, pp.W), BestEngine(script))
    face.anonymize(list(np.zeros((3,) + pp.BGR, np.uint8)), tracker=pp.TRK, **pp.MOSAIC)
    assert not [e for e in script.log if "bestshot" in e[1] or e[1].startswith("align")]
