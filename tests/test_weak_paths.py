"""What CenterFace's product methods ask of their engine when the plan's tracker has two thresholds, pinned without a GPU in the manner
of tests/test_product_paths.py: the recording stand-in for ``Engine`` returns rows on both sides of ``birth_score``; with a weak tracker
every path decodes at the tracker's ``weak_score`` -- rescaled, unfit and merged rows alike -- and returns the rows above its
``birth_score``; with a plain tracker or none the log and the results are what they are without this feature."""
import types

import numpy as np
import pytest

import test_product_paths as pp

WEAK_SCORE, BIRTH = 0.125, 0.3
WTRK = types.SimpleNamespace(weak_score=WEAK_SCORE, birth_score=BIRTH)     # all that the paths read of a ``Tracker``
SHOTS = type("Shots", (), {"size": 16, "streams": 8, "entries": 4})()
SCORES = (0.9, 0.2, 0.3, float(np.nextafter(np.float32(0.3), np.float32(1))), 0.05, 0.31)      # 0.3 itself is weak


def rows_of(i):
    """The decode's (the unfit's, the merge's) rows of image i: pp.canned's and two more, the scores on both sides of the threshold."""
    n = pp.COUNTS[i] + 2
    d = (1000.0 * i + np.arange(n * 5, dtype=np.float32)).reshape(n, 5)
    d[:, 4] = np.array(SCORES[:n], np.float32)
    return d, (500.0 + 1000.0 * i + np.arange(n * 10, dtype=np.float32)).reshape(n, 10)


class WeakEngine(pp.StubEngine):
    def _mine(self):
        return [rows_of(i) for i in range(self.first, self.first + self.B)]

    def track_update_device(self, tracker, stream0=0):
        self._log("track_update_device", tracker is pp.TRK or tracker is WTRK, stream0)

    def bestshot_offer(self, shots, chips, offsets, hw, stream0=0):
        self._log("bestshot_offer", shots is SHOTS, chips.shape, np.asarray(offsets).tolist(), tuple(hw), stream0)
        return np.zeros((len(chips),), np.int64), np.zeros((len(offsets) - 1,), np.int32)

    def bestshot_collect(self, shots, stream0=0, B=None, cap=None, flush=False):
        self._log("bestshot_collect", shots is SHOTS, stream0, B, cap, flush)
        z = np.zeros
        return (z((B, 1, 16, 16, 3), np.uint8), z((B, 1), np.int64), z((B, 1, 8), np.int32), z((B, 1, 5), np.float32), z((B, 1, 10), np.float32),
                z((B,), np.int32), z((B,), np.int32), z((B,), np.int32))


#        id                      method          frame shape    hw              keywords                                   results at
CASES = [("anonymize-plain", "anonymize", pp.BGR, (pp.H, pp.W), dict(pp.MOSAIC), 1),
         ("anonymize-fit", "anonymize", pp.BGR, (pp.H, pp.W), dict(pp.MOSAIC, fit=True), 1),
         ("anonymize-tiled", "anonymize", pp.BGR_EVEN, (pp.YH, pp.YW), dict(pp.BLUR, tiled=True), 1),
         ("anonymize_yuv-plain", "anonymize_yuv", pp.YUV, (pp.YH, pp.YW), dict(pp.BLUR), 1),
         ("annotate-plain", "annotate", pp.BGR, (pp.H, pp.W), {}, 1),
         ("annotate-fit", "annotate", pp.BGR, (pp.H, pp.W), dict(fit=dict(anchor="topleft")), 1),
         ("annotate-tiled", "annotate", pp.BGR_EVEN, (pp.YH, pp.YW), dict(tiled=True), 1),
         ("detect_tiled-redact", "detect_tiled", pp.BGR_EVEN, (pp.YH, pp.YW), dict(redact=pp.MOSAIC), None),
         ("detect_fit-redact", "detect_fit", pp.BGR, (pp.H, pp.W), dict(redact=pp.BLUR), None),
         ("best_shots-plain", "best_shots", pp.BGR, (pp.H, pp.W), dict(shots=SHOTS, template=None), "shots"),
         ("best_shots-fit", "best_shots", pp.BGR_EVEN, (pp.YH, pp.YW), dict(shots=SHOTS, fit=True), "shots"),
         ("best_shots-tiled", "best_shots", pp.BGR_EVEN, (pp.YH, pp.YW), dict(shots=SHOTS, tiled=True), "shots")]
IDS = [c[0] for c in CASES]


def run(case, tracker, fail=None):
    """(the log with addresses resolved, what the method returned or the exception it raised, the source frames and their copy)."""
    _, method, per, hw, kw, _ = case
    script = pp.Script(fail)
    face = pp.make_face(hw, WeakEngine(script))
    src = np.random.default_rng(1).integers(0, 256, (pp.N,) + per, dtype=np.uint8)
    before = src.copy()
    try:
        ret = getattr(face, method)(src, **dict(kw, **({} if tracker is None and method != "best_shots" else dict(tracker=tracker))))
    except pp.Boom as e:
        ret = e
    regions = {"in": src}
    if isinstance(ret, tuple) and isinstance(ret[0], np.ndarray):
        regions["out"] = ret[0]
    return [e[1:] for e in pp.resolve(script.log, regions)], ret, src, before


def results_of(case, ret):
    at = case[5]
    return None if at == "shots" else ret if at is None else ret[at]


def check_rows(results, strong_only):
    assert isinstance(results, list) and len(results) == pp.N
    for i, (d, l) in enumerate(results):
        wd, wl = rows_of(i)
        if strong_only:
            keep = wd[:, 4] > np.float32(BIRTH)
            assert not keep.all() and (keep.any() or len(wd) <= 2)
            wd, wl = wd[keep], wl[keep]
        assert d.dtype == np.float32 and l.dtype == np.float32 and d.tobytes() == wd.tobytes() and l.tobytes() == wl.tobytes(), i
        assert not strong_only or (d[:, 4] > np.float32(BIRTH)).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_weak_tracker_lowers_the_decode_threshold_and_nothing_else(case):
    """The log of the call with a weak tracker is the log with a plain tracker with ``weak_score`` in place of 0.3 in every decode -- on
    the rescaled, the unfit and the merged rows -- and the results are the rows above ``birth_score``."""
    plain, ret0, _, _ = run(case, pp.TRK)
    weak, ret1, src, before = run(case, WTRK)
    decodes = [e for e in plain if e[0] == "decode_threshold"]
    assert len(decodes) >= 3 and all(e == ("decode_threshold", 0.3, pp.NMS, pp.MAXD) for e in decodes)
    assert weak == [("decode_threshold", WEAK_SCORE, pp.NMS, pp.MAXD) if e[0] == "decode_threshold" else e for e in plain]
    assert sum(e[0] == "track_update_device" for e in weak) == len(decodes)
    kind = "merge_tiles" if case[4].get("tiled") or case[1] == "detect_tiled" else "unfit_rows" if case[4].get("fit") or case[1] == "detect_fit" else None
    assert kind is None or sum(e[0] == kind for e in weak) == len(decodes)
    assert (kind is None) == any(e[0] == "set_rescale" for e in weak)
    if case[5] != "shots":
        check_rows(results_of(case, ret0), strong_only=False)
        check_rows(results_of(case, ret1), strong_only=True)
    if case[1] != "detect_tiled" and case[1] != "detect_fit":
        assert np.array_equal(src, before)


@pytest.mark.parametrize("case", [c for c in CASES if c[5] != "shots"], ids=[c[0] for c in CASES if c[5] != "shots"])
def test_without_a_tracker_the_log_and_the_results_are_todays(case):
    none, ret, _, _ = run(case, None)
    plain, _, _, _ = run(case, pp.TRK)
    # (without a tracker the annotation labels a face with its score, with one with the track's id)
    assert none == [e[:3] + (dict(e[3], label="score"),) if e[0] == "draw_faces" else e for e in plain if e[0] != "track_update_device"]
    assert all(e[1] == 0.3 for e in none if e[0] == "decode_threshold")
    check_rows(results_of(case, ret), strong_only=False)


def test_birth_score_is_the_trackers_own():
    """The filter reads the tracker's ``birth_score``, float32 and strict: at 0.2 the row that scores float32(0.2) itself stays out."""
    case = CASES[0]
    script = pp.Script()
    face = pp.make_face(case[3], WeakEngine(script))
    src = np.zeros((pp.N,) + case[2], np.uint8)
    _, results = face.anonymize(src, tracker=types.SimpleNamespace(weak_score=0.01, birth_score=0.2), **case[4])
    assert [e[2] for e in script.log if e[1] == "decode_threshold"] == [0.01] * 3
    for i, (d, _) in enumerate(results):
        want = rows_of(i)[0]
        assert d.tobytes() == want[want[:, 4] > np.float32(0.2)].tobytes() and np.float32(0.2) not in d[:, 4]
    assert sum(len(d) for d, _ in results) == sum(int((rows_of(i)[0][:, 4] > np.float32(0.25)).sum()) for i in range(pp.N))


def test_without_landmarks_the_strong_boxes_come_alone():
    script = pp.Script()
    face = pp.make_face((pp.H, pp.W), WeakEngine(script), landmarks=False)
    _, results = face.anonymize(np.zeros((pp.N,) + pp.BGR, np.uint8), tracker=WTRK, **pp.MOSAIC)
    for i, d in enumerate(results):
        want = rows_of(i)[0]
        assert isinstance(d, np.ndarray) and d.tobytes() == want[want[:, 4] > np.float32(BIRTH)].tobytes()


@pytest.mark.parametrize("kind", ("forward", "decode_threshold"))
@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("anonymize-plain", "anonymize_yuv-plain", "annotate-plain", "best_shots-plain")],
                         ids=lambda c: c[0])
def test_a_failing_second_chunk_switches_the_rescale_off(case, kind):
    """The enqueue or the decode of the second chunk raises: the log is the full log up to the failed call, then set_rescale(0, 0)."""
    full, _, _, _ = run(case, WTRK)
    log, ret, src, before = run(case, WTRK, fail=(kind, 1))
    assert isinstance(ret, pp.Boom)
    at = [k for k, e in enumerate(full) if (e[0].startswith("forward") if kind == "forward" else e[0] == kind)][1]
    assert pp.strip_out(log) == pp.strip_out(full[:at + 1] + [("set_rescale", 0.0, 0.0)])
    assert log[-1] == ("set_rescale", 0.0, 0.0) and full[0][0] == "set_rescale" and np.array_equal(src, before)
    assert sum(e[0] == "track_update_device" for e in log) == 1


def test_a_tracker_object_of_the_library_carries_the_two_scores():
    import centerface_amd as cfa
    t = cfa.Tracker(0, pp.N, weak_score=WEAK_SCORE)                          # a device index: nothing is created
    script = pp.Script()
    face = pp.make_face((pp.H, pp.W), WeakEngine(script))
    _, results = face.anonymize(np.zeros((pp.N,) + pp.BGR, np.uint8), tracker=t, **pp.MOSAIC)
    assert [e[2] for e in script.log if e[1] == "decode_threshold"] == [WEAK_SCORE] * 3
    check_rows(results, strong_only=True)
    t.close()
