"""What the four stream-state objects -- cf_tracker, cf_scene, cf_lookback, cf_bestshot -- share: the create / destroy / clear protocol
and the Python wrappers' constructor, range check and close (no GPU needed), then, on the GPU, the refusals every per-frame call makes
before it launches anything -- a null handle, a stream range outside the object, a batch above max_batch -- each of which must leave
the object usable: the valid call behind them gives what the numpy restatement of that kind gives for the step."""
import ctypes as C
import types

import numpy as np
import pytest

import centerface_amd as cfa
from bestshot_cases import RefBestShots
from follow_cases import RefFollower, canvas, luma_of
from lookback_cases import RefLookback
from scene_cases import FIRST, RefScene, scene
from test_bestshot import _ref_offer, _same_collect
from test_follow import _same_follow
from test_track import _feed_until_faces, _same_update

_lib = cfa._lib
EINVAL = -1

# kind: the Python class, the C entry points, the noun of the messages, the options, and options the library refuses
KINDS = {
    "tracker": dict(cls=cfa.Tracker, create="cf_track_create", destroy="cf_track_destroy", clear="cf_track_reset", clear_py="reset", noun="tracker",
                    opts=_lib.track_opts, bad=dict(max_tracks=0)),
    "scene": dict(cls=cfa.SceneCuts, create="cf_scene_create", destroy="cf_scene_destroy", clear="cf_scene_forget", clear_py="forget", noun="scene object",
                  opts=_lib.scene_opts, bad=dict(hist=-1)),
    "lookback": dict(cls=cfa.Lookback, create="cf_lookback_create", destroy="cf_lookback_destroy", clear="cf_lookback_forget", clear_py="forget",
                     noun="lookback object", opts=_lib.lookback_opts, bad=dict(depth=0)),
    # a table has no clear call: its entries leave through cf_bestshot_collect
    "bestshot": dict(cls=cfa.BestShots, create="cf_bestshot_create", destroy="cf_bestshot_destroy", clear=None, clear_py=None, noun="table",
                     opts=_lib.bestshot_opts, bad=dict(entries=0)),
}
kinds = pytest.mark.parametrize("kind", sorted(KINDS))
clearable = pytest.mark.parametrize("kind", sorted(k for k in KINDS if KINDS[k]["clear"]))


def _op_error():
    return (_lib.lib().cf_op_last_error() or b"").decode()


# ---------------------------------------------------------------------------------------------- without a GPU
@kinds
def test_create_without_a_context_tells_what_is_wrong_in_a_fixed_order(kind):
    """The options and the stream count come first, then the null out, then the null context; every text names the function."""
    k, L = KINDS[kind], _lib.lib()
    create, o, h = getattr(L, k["create"]), k["opts"](), C.c_void_p()

    def why(S, opts, out):
        assert create(None, S, opts, out) == EINVAL and h.value is None
        text = _op_error()
        assert text.startswith(k["create"] + ": "), text
        return text

    assert "null options" in why(0, None, None)                              # whatever else is wrong
    assert "null options" in why(2, None, C.byref(h))
    for S in (0, -1, 4097):
        assert "n_streams" in why(S, C.byref(o), None) and "n_streams" in why(S, C.byref(o), C.byref(h))
    assert "null out" in why(2, C.byref(o), None)
    assert why(2, C.byref(o), C.byref(h)) == k["create"] + ": null context"
    assert why(1, C.byref(o), C.byref(h)).endswith("null context") and why(4096, C.byref(o), C.byref(h)).endswith("null context")
    bad = k["opts"](**k["bad"])
    text = why(2, C.byref(bad), C.byref(h))
    assert "null context" not in text and "null o" not in text and "n_streams" not in text


@kinds
def test_destroy_of_a_null_handle_is_ok(kind):
    assert getattr(_lib.lib(), KINDS[kind]["destroy"])(None) == 0


@clearable
def test_clear_refuses_a_null_handle_and_names_itself(kind):
    k, L = KINDS[kind], _lib.lib()
    for stream in (-1, 0, 5):
        assert getattr(L, k["clear"])(None, stream) == EINVAL
        assert _op_error().startswith(k["clear"] + ": null ")


@kinds
def test_wrapper_for_a_device_index_checks_the_options_at_once_and_creates_nothing(kind):
    k = KINDS[kind]
    for kw in (k["bad"], dict(streams=0), dict(streams=4097)):
        kw = dict(dict(streams=2), **kw)
        with pytest.raises(_lib.CenterFaceValueError) as e:
            k["cls"](0, **kw)
        assert k["create"] in str(e.value) and "null context" not in str(e.value) and e.value.code == EINVAL
    x = k["cls"](1, 3)
    assert (x.device, x.streams, x._h) == (1, 3, None)
    with pytest.raises(ValueError, match="the %s was made for device 1, the engine runs on device 0" % k["noun"]):
        x._handle(types.SimpleNamespace(device=0, _h=None))                  # an engine of another GPU: refused before any create
    assert x._h is None
    x.close()
    x.close()                                                                # twice is harmless
    assert x._h is None
    del x


@clearable
def test_wrapper_checks_the_stream_of_a_clear_and_names_noun_and_count(kind):
    k = KINDS[kind]
    x = k["cls"](0, 3)
    clear = getattr(x, k["clear_py"])
    for stream in (-1, 0, 2):                                                # no engine yet: nothing is created, the range is checked
        assert clear(stream) is None
    assert clear() is None and x._h is None
    for stream in (-2, 3, 4096):
        with pytest.raises(ValueError, match="stream %d of a %s with 3" % (stream, k["noun"])):
            clear(stream)
    x.close()
    for stream in (3, -2):                                                   # a closed object still checks the range
        with pytest.raises(ValueError, match="of a %s with 3" % k["noun"]):
            clear(stream)
    assert clear(1) is None


# ---------------------------------------------------------------------------------------------- on the GPU
TRACK = dict(iou=0.3, max_age=3, min_hits=1, max_tracks=70, hold_grow=0.1)
FOLLOW = dict(search=3, max_sad=30000)


@pytest.fixture(scope="module")
def rig():
    """The smallest engine the tests of these objects build, and a source on which its decode keeps faces."""
    eng = cfa.Engine(64, 96, max_batch=2, dtype="bf16")
    src, _ = _feed_until_faces(eng, np.random.default_rng(3), need=2, B=2)
    yield eng, src
    eng.close()


def _decoded(eng, src):
    eng.forward_resized_enqueue(src)
    return eng.decode_threshold(0.3, 0.3, 64)


def _refused(eng, code, *words):
    why = (_lib.lib().cf_last_error(eng._h) or b"").decode()
    assert code == EINVAL, (code, why)
    for word in words:
        assert word in why, (word, why)


def _ranges(eng, call, obj, fn, noun, bounded=True):
    """The refusals of one per-frame call ``call(handle, stream0, B)`` on an object with 2 streams through an engine with max_batch 2."""
    _refused(eng, call(None, 0, 2), fn, "null " + noun)
    _refused(eng, call(obj._h, -1, 2), fn, "streams -1 .. 0 of a %s with 2" % noun)
    _refused(eng, call(obj._h, 1, 2), fn, "streams 1 .. 2 of a %s with 2" % noun)
    if bounded:
        _refused(eng, call(obj._h, 0, 3), fn, "B=3 exceeds max_batch 2")


def _frame_args(frames):
    (f, tab, dev, B, h, w, p0, p1), keep = _lib.host_frame_args(frames, "bgr", writable=False)
    return (f, tab, dev, h, w, p0, p1), keep


def _gpu_tracker(eng, src):
    L, rng = _lib.lib(), np.random.default_rng(4)
    base = _decoded(eng, src)
    trk, ref = cfa.Tracker(eng, 2, **TRACK), RefFollower(2, (64, 96), **FOLLOW, **TRACK)
    # the update takes B from the rows (2 here): max_batch bounds it through the forward
    _ranges(eng, lambda t, s0, B: L.cf_track_update(eng._h, t, s0, None, None, None, None, None, 0), trk, "cf_track_update", "tracker", bounded=False)
    got, flags = eng.track_update(trk)
    _same_update(got, [ref.update(b, d[:, :4], d[:, 4], l, len(d)) for b, (d, l) in enumerate(base)])
    assert not flags.any() and sum(len(g[0]) for g in got) >= 2
    frames = np.stack([canvas(rng, "bgr", 76, 102, 0, 4) for _ in range(3)])
    o = _lib.follow_opts(**FOLLOW)

    def follow(t, s0, B):
        a, keep = _frame_args(frames[:B])
        return L.cf_track_follow(eng._h, t, s0, B, C.byref(o), a[0], a[1], a[2], a[3], a[4], a[5], a[6], None, None, None, None, None, 0)
    _ranges(eng, follow, trk, "cf_track_follow", "tracker")
    got = eng.track_follow(frames[:2], "bgr", trk, 0, **FOLLOW)
    _same_follow(got, [ref.follow(b, luma_of((f.reshape(76, -1),), "bgr")) for b, f in enumerate(frames[:2])])
    assert got[3].sum() >= 2
    trk.close()


def _gpu_scene(eng, src):
    L, rng = _lib.lib(), np.random.default_rng(5)
    scn, ref = cfa.SceneCuts(eng, 2), RefScene(2)
    frames = np.stack([scene(rng, "bgr", 76, 104, 0, 128) for _ in range(3)])

    def check(t, s0, B):
        a, keep = _frame_args(frames[:B])
        return L.cf_scene_check(eng._h, t, None, s0, B, a[0], a[1], a[2], a[3], a[4], a[5], a[6], None, 0)
    _ranges(eng, check, scn, "cf_scene_check", "scene object")
    for _ in range(2):                                                       # FIRST, then SAME: no refused call was a check
        got = eng.scene_check(frames[:2], "bgr", scn)
        assert np.array_equal(got, np.array([ref.check(b, luma_of((f.reshape(76, -1),), "bgr")) for b, f in enumerate(frames[:2])], np.int32))
    assert (got[:, 0] != FIRST).all()
    scn.close()


def _gpu_lookback(eng, src):
    L, R = _lib.lib(), 70
    _decoded(eng, src)
    trk = cfa.Tracker(eng, 2, **TRACK)
    lb, ref = cfa.Lookback(eng, 2, depth=1, rows=R, grow=0.25), RefLookback(2, depth=1, rows=R, grow=0.25)
    tracked, _ = eng.track_update(trk)
    _ranges(eng, lambda t, s0, B: L.cf_lookback_step(eng._h, t, s0, B, 1, None, 0, None, None, None, None, None, 0), lb, "cf_lookback_step", "lookback object")
    for push in (True, False):                                               # the push emits nothing yet, the drain emits the tracked rows
        got = eng.lookback_step(lb, 0, 2, push=push)
        for b, (d, l, ids, hits, misses) in enumerate(tracked):
            n = len(d)
            pad = lambda a, k: np.concatenate([a, np.zeros((R - n, k), a.dtype)])      # noqa: E731
            rows = (pad(d, 5), pad(l, 10), pad(np.stack([ids, hits, misses], 1).astype(np.int32), 3), n) if push else ()
            wd, wl, wi, ws = ref.step(b, push, *rows)
            k = len(wd)
            assert got[3][b] == k and got[4][b].tolist() == ws.tolist(), (push, b)
            assert got[0][b, :k].tobytes() == wd.tobytes() and got[1][b, :k].tobytes() == wl.tobytes() and got[2][b, :k].tobytes() == wi.tobytes()
    assert got[3].sum() == sum(len(t[0]) for t in tracked) >= 2
    lb.close(), trk.close()


def _gpu_bestshot(eng, src):
    L, E = _lib.lib(), 16
    _decoded(eng, src)
    h, w = src.shape[1:3]
    trk = cfa.Tracker(eng, 2, iou=0.3, max_age=0, min_hits=1, max_tracks=70)
    shots = cfa.BestShots(eng, 2, size=16, entries=E, min_hits=1)
    ref = RefBestShots(2, entries=E, min_hits=1, terms=7, fx=float(w) / 96.0, fy=float(h) / 64.0)
    tracked, _ = eng.track_update(trk)
    chips, offs, _ = eng.align_faces_frame(src, "bgr", size=16)
    assert len(chips) >= 2
    offs3 = np.concatenate([offs, offs[-1:]])                                # a third image without faces

    def offer(t, s0, B):
        return L.cf_bestshot_offer(eng._h, t, s0, B, _lib.ptr(chips), _lib.ptr(offs if B == 2 else offs3), len(chips), 0, h, w, None, None, 0)
    _ranges(eng, offer, shots, "cf_bestshot_offer", "table")
    q, fl = eng.bestshot_offer(shots, chips, offs, (h, w))
    assert q.tolist() == _ref_offer(ref, tracked, chips, offs).tolist() and not fl.any() and (q >= 0).any()
    # the collect involves no rows of the context: max_batch does not bound it
    _ranges(eng, lambda t, s0, B: L.cf_bestshot_collect(eng._h, t, s0, B, E, 1, None, None, None, None, None, None, None, None, 0), shots,
            "cf_bestshot_collect", "table", bounded=False)
    assert _same_collect(eng.bestshot_collect(shots, flush=True), ref, 2, E, flush=True) >= 2
    shots.close(), trk.close()


@pytest.mark.gpu
@kinds
def test_per_frame_calls_refuse_before_any_launch_and_leave_the_object_usable(rig, kind):
    {"tracker": _gpu_tracker, "scene": _gpu_scene, "lookback": _gpu_lookback, "bestshot": _gpu_bestshot}[kind](*rig)
