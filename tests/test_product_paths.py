"""What CenterFace's product methods ask of their engine, pinned without a GPU: every method runs against a recording stand-in for
``Engine`` and the exact sequence of public Engine calls -- chunking, input form, rescale on / off, tracker stream offsets, which slice of
which array is covered -- is compared with a restatement of the chunk loop, together with what the method returns.  Only ``ops.tile_grid``
(host-only library code) is real.  ``pinned_copy`` needs a GPU, so the page-locked input form is reached by stubbing ``is_pinned``."""
import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops

H, W = 75, 101                      # BGR source size: the network is 96 x 128 and the rescale is live
YH, YW = 76, 102                    # 4:2:0 frames have even sides
NH, NW = 96, 128
NMS, MAXD = 0.25, 77                # not the defaults, so that their way into the decode shows
COUNTS = (2, 0, 1, 3, 0)            # faces per image: both chunk positions see an empty and a non-empty image
N, NB = len(COUNTS), 2
BGR, NET, YUV, BGR_EVEN, BGR_WIDE = (H, W, 3), (NH, NW, 3), (YH * 3 // 2, YW), (YH, YW, 3), (YH, 200, 3)
TRK = object()
MOSAIC = dict(mode="mosaic", shape="rect", cell=6)
BLUR = dict(mode="blur", radius=3)
CHIP = dict(out="f32", rgb=True)


class Boom(Exception):
    pass


def canned(i):
    n = COUNTS[i]
    d = (1000.0 * i + np.arange(n * 5, dtype=np.float32)).reshape(n, 5)
    return d, (500.0 + 1000.0 * i + np.arange(n * 10, dtype=np.float32)).reshape(n, 10)


def _desc(a):
    """An array argument as (shape, dtype, address); a list of arrays as ('list', ...)."""
    if isinstance(a, np.ndarray):
        return ("arr", a.shape, str(a.dtype), a.ctypes.data)
    return ("list",) + tuple(_desc(x) for x in a)


class Script(object):
    """What the engines of one case share: the call log, the index of the next image, the call that is to fail."""

    def __init__(self, fail=None):
        self.log, self.next, self.fail, self.seen = [], 0, fail, {}


class StubEngine(object):
    def __init__(self, script, name="e", max_batch=NB):
        self.s, self.name, self.max_batch, self.H, self.W, self.device = script, name, max_batch, NH, NW, 0
        self.first, self.B = 0, 0

    def _log(self, call, *args):
        self.s.log.append((self.name, call) + args)
        kind = "forward" if call.startswith("forward") else call
        k = self.s.seen[kind] = self.s.seen.get(kind, -1) + 1
        if self.s.fail == (kind, k):
            raise Boom(call)

    def _forward(self, call, frames, *args):
        self._log(call, _desc(frames), *args)
        self.first, self.B = self.s.next, len(frames)
        self.s.next += len(frames)

    def _mine(self):
        return [canned(i) for i in range(self.first, self.first + self.B)]

    def set_rescale(self, scale_h=0.0, scale_w=0.0):
        self._log("set_rescale", float(scale_h), float(scale_w))

    def forward_enqueue(self, x):
        self._forward("forward_enqueue", x)

    def forward_resized_enqueue(self, x):
        self._forward("forward_resized_enqueue", x)

    def forward_images_enqueue(self, images):
        self._forward("forward_images_enqueue", images)

    def forward_yuv_enqueue(self, frames, fmt="nv12"):
        self._forward("forward_yuv_enqueue", frames, fmt)

    def forward_tiles_enqueue(self, frames, rects, fmt="bgr"):
        self._forward("forward_tiles_enqueue", frames, tuple(map(tuple, np.asarray(rects).tolist())), fmt)
        self.T = len(rects)

    def decode_threshold(self, score_thresh=0.3, nms_thresh=0.3, max_out=1024):
        self._log("decode_threshold", score_thresh, nms_thresh, max_out)
        return self._mine()

    def merge_tiles(self, metric="ios", thresh=0.5, edge=2.0, max_out=1024):
        self._log("merge_tiles", metric, thresh, edge, max_out)
        return self._mine(), np.zeros((self.B,), np.int32)

    def track_update_device(self, tracker, stream0=0):
        self._log("track_update_device", tracker is TRK, stream0)

    def cover_faces(self, frames, fmt="bgr", **options):
        self._log("cover_faces", _desc(frames), fmt, options)
        for b in range(self.B):                                            # leaves a mark in every frame that has faces
            if COUNTS[self.first + b]:
                frames[b].reshape(-1)[0] ^= 0xFF
        return frames

    def _chips(self, size):
        n = [COUNTS[i] for i in range(self.first, self.first + self.B)]
        chips = np.empty((sum(n), size, size, 3), np.uint8)
        chips[...] = (sum(COUNTS[:self.first]) + np.arange(sum(n))).reshape(-1, 1, 1, 1)        # chip k holds the face's global index
        return chips, np.concatenate([[0], np.cumsum(n)]).astype(np.int32), np.zeros((sum(n), 6))

    def align_faces(self, size=112, **chip_options):
        self._log("align_faces", size, chip_options)
        return self._chips(size)

    def align_faces_frame(self, frames, fmt="bgr", size=112, **chip_options):
        self._log("align_faces_frame", _desc(frames), fmt, size, chip_options)
        return self._chips(size)


def make_face(hw, engine, engine2=None, landmarks=True):
    face = object.__new__(cfa.CenterFace)
    face.landmarks, face.src_hw = landmarks, hw
    face.img_h_new, face.img_w_new, face.scale_h, face.scale_w = face.transform(*hw)
    assert (face.img_h_new, face.img_w_new) == (NH, NW)
    face.nms_thresh, face.max_dets, face.device, face._engine_kw = NMS, MAXD, 0, {}
    face.engine, face._engine2 = engine, engine2
    return face


def resolve(log, regions):
    """The log with every address replaced by (name of the array it lies in, byte offset) or ('tmp', None)."""
    def fix(v):
        if isinstance(v, tuple) and v[:1] == ("arr",):
            for name, a in regions.items():
                if a.ctypes.data <= v[3] < a.ctypes.data + a.nbytes:
                    return v[1:3] + (name, v[3] - a.ctypes.data)
            return v[1:3] + ("tmp", None)
        if isinstance(v, tuple) and v[:1] == ("list",):
            return ("list",) + tuple(fix(x) for x in v[1:])
        return v
    return [tuple(fix(v) for v in entry) for entry in log]


# ------------------------------------------------------------------------------------------------ the restatement
def chunk(i, b, per, where):
    return ((b,) + per, "uint8", where, None if where == "tmp" else i * int(np.prod(per)))


def chunk_list(i, b, per, where):
    return ("list",) + tuple((per, "uint8", where, (i + k) * int(np.prod(per))) for k in range(b))


def fwd(call, per, where, *more, as_list=False):
    return lambda i, b: (call, (chunk_list if as_list else chunk)(i, b, per, where)) + more


def cover(per, where, fmt, options):
    return lambda i, b: ("cover_faces", chunk(i, b, per, where), fmt, options)


def frame_chips(per, where, fmt):
    return lambda i, b: ("align_faces_frame", chunk(i, b, per, where), fmt, 16, CHIP)


def net_chips(i, b):
    return ("align_faces", 16, CHIP)


def plain(forward, scale, track=False, cover=None, chips=None):
    """The untiled chunk loop: rescale on; per chunk forward, decode, track, cover, chips; rescale off."""
    log = [("set_rescale",) + scale]
    for i in range(0, N, NB):
        b = min(NB, N - i)
        log += [forward(i, b), ("decode_threshold", 0.3, NMS, MAXD)]
        log += [("track_update_device", True, i)] if track else []
        log += [step(i, b) for step in (cover, chips) if step]
    return log + [("set_rescale", 0.0, 0.0)]


def tiled(per_frame, where, fmt, tile_args=((NH, NW), 24, True), merge=("ios", 0.5, 2.0), track=False, cover=None, chips=None):
    """The tiled chunk loop: no rescale; per chunk of max_batch // T frames forward, decode, merge, track, cover, chips."""
    h, w = (per_frame[0], per_frame[1]) if len(per_frame) == 3 else (per_frame[0] * 2 // 3, per_frame[1])
    rects = tuple(map(tuple, ops.tile_grid(h, w, *tile_args).tolist()))
    per, log = NB // len(rects), []
    assert per >= 1
    for i in range(0, N, per):
        b = min(per, N - i)
        log += [("forward_tiles_enqueue", chunk(i, b, per_frame, where), rects, fmt), ("decode_threshold", 0.3, NMS, MAXD),
                ("merge_tiles",) + merge + (MAXD,)]
        log += [("track_update_device", True, i)] if track else []
        log += [step(i, b) for step in (cover, chips) if step]
    return log


S_BGR, S_YUV, S_ONE = (NH / H, NW / W), (NH / YH, NW / YW), (1.0, 1.0)


def case(id, method, per, expect, args=(), kw=None, hw=None, as_list=False, pinned=False, returns="dets", in_place=False):
    hw = hw or ((per[0], per[1]) if len(per) == 3 else (per[0] * 2 // 3, per[1]))
    if per == BGR_WIDE:
        hw = (YH, YW)                                                      # tiled: frames of any even size
    return pytest.param(dict(method=method, per=per, expect=expect, args=args, kw=kw or {}, hw=hw, as_list=as_list, pinned=pinned,
                             returns=returns, in_place=in_place), id=id)


def _forms(method, args=(), kw=None, chips=None, returns="dets"):
    """The three BGR input forms (network-sized, to be resized, page-locked) behind ``method``."""
    k = dict(args=args, kw=kw, returns=returns)
    return [case(method + "-network-sized", method, NET, lambda: plain(fwd("forward_enqueue", NET, "tmp"), S_ONE, chips=chips), **k),
            case(method + "-resized", method, BGR, lambda: plain(fwd("forward_resized_enqueue", BGR, "tmp"), S_BGR, chips=chips), as_list=True, **k),
            case(method + "-pinned", method, BGR, lambda: plain(fwd("forward_images_enqueue", BGR, "in", as_list=True), S_BGR, chips=chips),
                 as_list=True, pinned=True, **k)]


def _anonymize(options, track):
    kw = dict(options, **(dict(tracker=TRK) if track else {}))
    tag = "%s%s" % (options["mode"], "-tracker" if track else "")
    return [case("anonymize-" + tag, "anonymize", BGR, lambda: plain(fwd("forward_resized_enqueue", BGR, "tmp"), S_BGR, track, cover(BGR, "out", "bgr", options)),
                 kw=kw, as_list=True, returns="out"),
            case("anonymize_yuv-" + tag, "anonymize_yuv", YUV, lambda: plain(fwd("forward_yuv_enqueue", YUV, "in", "nv12"), S_YUV, track, cover(YUV, "out", "nv12", options)),
                 kw=kw, returns="out")]


CASES = (
    _forms("detect_batch") + _forms("detect_aligned", (16,), CHIP, net_chips, "chips") + [
        case("detect_yuv-array", "detect_yuv", YUV, lambda: plain(fwd("forward_yuv_enqueue", YUV, "in", "nv12"), S_YUV)),
        case("detect_yuv-list", "detect_yuv", YUV, lambda: plain(fwd("forward_yuv_enqueue", YUV, "in", "i420", as_list=True), S_YUV), ("i420",), as_list=True),
        case("detect_aligned_frames-bgr", "detect_aligned_frames", BGR,
             lambda: plain(fwd("forward_resized_enqueue", BGR, "in"), S_BGR, chips=frame_chips(BGR, "in", "bgr")), ("bgr", 16), CHIP, returns="chips"),
        case("detect_aligned_frames-nv12", "detect_aligned_frames", YUV,
             lambda: plain(fwd("forward_yuv_enqueue", YUV, "in", "nv12"), S_YUV, chips=frame_chips(YUV, "in", "nv12")), ("nv12", 16), CHIP, returns="chips"),
        case("detect_aligned_frames-tiled", "detect_aligned_frames", BGR_EVEN, lambda: tiled(BGR_EVEN, "in", "bgr", chips=frame_chips(BGR_EVEN, "in", "bgr")),
             ("bgr", 16), dict(CHIP, tiled=True), returns="chips"),
        case("detect_tiled-plain", "detect_tiled", BGR_EVEN, lambda: tiled(BGR_EVEN, "in", "bgr")),
        case("detect_tiled-redact", "detect_tiled", BGR_EVEN, lambda: tiled(BGR_EVEN, "in", "bgr", cover=cover(BGR_EVEN, "in", "bgr", MOSAIC)),
             kw=dict(redact=MOSAIC), in_place=True),
        case("detect_tiled-redact-tracker", "detect_tiled", YUV, lambda: tiled(YUV, "in", "nv12", track=True, cover=cover(YUV, "in", "nv12", BLUR)),
             (None, None, "nv12"), dict(redact=BLUR, tracker=TRK), in_place=True),
        case("detect_tiled-tracker", "detect_tiled", BGR_EVEN, lambda: tiled(BGR_EVEN, "in", "bgr", track=True), kw=dict(tracker=TRK)),
        case("detect_tiled-two-tiles", "detect_tiled", BGR_WIDE,                   # one frame per chunk; the merge's arguments pass through
             lambda: tiled(BGR_WIDE, "in", "bgr", ((NH, NW), 30, False), ("iou", 0.4, 1.0), True, cover(BGR_WIDE, "in", "bgr", MOSAIC)),
             (None, 30), dict(with_full=False, metric="iou", thresh=0.4, edge=1.0, redact=MOSAIC, tracker=TRK), in_place=True),
    ] + _anonymize(MOSAIC, False) + _anonymize(BLUR, False) + _anonymize(MOSAIC, True) + _anonymize(BLUR, True) + [
        case("anonymize-pinned", "anonymize", BGR, lambda: plain(fwd("forward_images_enqueue", BGR, "in", as_list=True), S_BGR, True, cover(BGR, "out", "bgr", MOSAIC)),
             kw=dict(MOSAIC, tracker=TRK), as_list=True, pinned=True, returns="out"),
        case("anonymize_yuv-list", "anonymize_yuv", YUV, lambda: plain(fwd("forward_yuv_enqueue", YUV, "in", "yv12", as_list=True), S_YUV, False, cover(YUV, "out", "yv12", BLUR)),
             ("yv12",), BLUR, as_list=True, returns="out"),
        case("anonymize-tiled", "anonymize", BGR_EVEN, lambda: tiled(BGR_EVEN, "out", "bgr", track=True, cover=cover(BGR_EVEN, "out", "bgr", MOSAIC)),
             kw=dict(MOSAIC, tiled=True, tracker=TRK), as_list=True, returns="out"),
        case("anonymize-tiled-blur", "anonymize", BGR_EVEN, lambda: tiled(BGR_EVEN, "out", "bgr", cover=cover(BGR_EVEN, "out", "bgr", BLUR)),
             kw=dict(BLUR, tiled=True), returns="out"),
        case("anonymize_yuv-tiled", "anonymize_yuv", YUV, lambda: tiled(YUV, "out", "nv21", track=True, cover=cover(YUV, "out", "nv21", BLUR)),
             ("nv21",), dict(BLUR, tiled=True, tracker=TRK), returns="out"),
        case("anonymize_yuv-tiled-mosaic", "anonymize_yuv", YUV, lambda: tiled(YUV, "out", "nv12", cover=cover(YUV, "out", "nv12", MOSAIC)),
             kw=dict(MOSAIC, tiled=True), as_list=True, returns="out"),
    ])


# ------------------------------------------------------------------------------------------------ running a case
def run(c, monkeypatch, fail=None, landmarks=True):
    """(resolved log, source array, its copy from before the call, what the method returned or the exception it raised)."""
    script = Script(fail)
    face = make_face(c["hw"], StubEngine(script), landmarks=landmarks)
    src = np.random.default_rng(1).integers(0, 256, (N,) + c["per"], dtype=np.uint8)
    before = src.copy()
    if c["pinned"]:
        monkeypatch.setattr(cfa.centerface, "is_pinned", lambda a: True)
    try:
        ret = getattr(face, c["method"])(list(src) if c["as_list"] else src, *c["args"], **c["kw"])
    except Boom as e:
        ret = e
    regions = {"in": src}
    if c["returns"] == "out" and not isinstance(ret, Boom):
        regions["out"] = ret[0]
    return [e[1:] for e in resolve(script.log, regions)], src, before, ret


def marked(before):
    want = before.copy()
    for i, n in enumerate(COUNTS):
        if n:
            want[i].reshape(-1)[0] ^= 0xFF
    return want


def check_results(results, landmarks=True, chips=False):
    assert isinstance(results, list) and len(results) == N
    face0 = 0
    for i, r in enumerate(results):
        d, l = canned(i)
        got = r if landmarks else (r,)
        assert len(got) == (3 if chips else 2 if landmarks else 1)
        for g, w in zip(got, (d, l)):
            assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g, w), (i, g, w)
        if chips:
            assert got[2].shape == (COUNTS[i], 16, 16, 3) and got[2].dtype == np.uint8
            assert (got[2] == np.arange(face0, face0 + COUNTS[i], dtype=np.uint8).reshape(-1, 1, 1, 1)).all(), i
        face0 += COUNTS[i]


@pytest.mark.parametrize("c", CASES)
def test_product_path(c, monkeypatch):
    log, src, before, ret = run(c, monkeypatch)
    assert log == c["expect"]()
    if c["returns"] == "out":
        out, results = ret
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == src.shape and not np.shares_memory(out, src)
        assert np.array_equal(out, marked(before)) and np.array_equal(src, before)
    else:
        results = ret
        assert np.array_equal(src, marked(before) if c["in_place"] else before)
    check_results(results, chips=c["returns"] == "chips")
    if c["kw"].get("tiled") or c["method"] == "detect_tiled":
        assert not any(e[0] == "set_rescale" for e in log)


FAILING = [p for p in CASES if p.id in ("detect_batch-resized", "detect_batch-pinned", "detect_yuv-list", "detect_aligned-resized", "detect_aligned_frames-nv12",
                                        "anonymize-mosaic-tracker", "anonymize_yuv-blur", "anonymize-pinned")]


@pytest.mark.parametrize("kind", ("forward", "decode_threshold"))
@pytest.mark.parametrize("c", FAILING)
def test_a_failing_second_chunk_switches_the_rescale_off(c, kind, monkeypatch):
    """The enqueue or the decode of the second chunk raises: the exception propagates, the log ends with set_rescale(0, 0) right behind
    the failed call, and nothing was tracked, covered or cut for that chunk."""
    log, src, before, ret = run(c, monkeypatch, fail=(kind, 1))
    assert isinstance(ret, Boom)
    full = c["expect"]()
    at = [k for k, e in enumerate(full) if (e[0].startswith("forward") if kind == "forward" else e[0] == kind)][1]
    # (the arrays of a call that raised are gone: the copy that anonymize would have returned resolves to 'tmp')
    strip = lambda entries: [tuple(v[:2] if isinstance(v, tuple) and len(v) == 4 and v[2] in ("out", "tmp") else v for v in e) for e in entries]      # noqa: E731
    assert strip(log) == strip(full[:at + 1] + [("set_rescale", 0.0, 0.0)])
    assert log[-1] == ("set_rescale", 0.0, 0.0)
    assert sum(e[0] in ("cover_faces", "align_faces", "align_faces_frame", "track_update_device") for e in log) == sum(
        e[0] in ("cover_faces", "align_faces", "align_faces_frame", "track_update_device") for e in full[:at])
    assert np.array_equal(src, before)


# ------------------------------------------------------------------------------------------------ detect_stream
def stream_log(forward, scale, fail=None):
    """Two engines alternate: the forward of chunk k + 1 is enqueued (rescale on) before the decode of chunk k (rescale off behind it)."""
    starts = list(range(0, N, NB))
    log = []
    for k in range(len(starts) + 1):
        if k < len(starts):
            e = "e%d" % (k & 1)
            log += [(e, "set_rescale") + scale, (e,) + forward(starts[k], min(NB, N - starts[k]))]
        if k:
            e = "e%d" % ((k - 1) & 1)
            log += [(e, "decode_threshold", 0.3, NMS, MAXD), (e, "set_rescale", 0.0, 0.0)]
    return log


STREAMS = [pytest.param(BGR, None, fwd("forward_resized_enqueue", BGR, "tmp"), S_BGR, False, id="bgr"),
           pytest.param(NET, None, fwd("forward_enqueue", NET, "tmp"), S_ONE, False, id="network-sized"),
           pytest.param(BGR, None, fwd("forward_images_enqueue", BGR, "in", as_list=True), S_BGR, True, id="pinned"),
           pytest.param(YUV, "nv12", fwd("forward_yuv_enqueue", YUV, "in", "nv12", as_list=True), S_YUV, False, id="nv12")]


def run_stream(per, fmt, pinned, monkeypatch, fail=None, landmarks=True):
    script = Script(fail)
    hw = (per[0], per[1]) if len(per) == 3 else (per[0] * 2 // 3, per[1])
    face = make_face(hw, StubEngine(script, "e0"), StubEngine(script, "e1"), landmarks=landmarks)
    src = np.random.default_rng(1).integers(0, 256, (N,) + per, dtype=np.uint8)
    before = src.copy()
    if pinned:
        monkeypatch.setattr(cfa.centerface, "is_pinned", lambda a: True)
    got, err = [], None
    try:
        for r in face.detect_stream(iter(src), **({} if fmt is None else dict(fmt=fmt))):
            got.append((r, len(script.log)))
    except Boom as e:
        err = e
    assert np.array_equal(src, before)
    return resolve(script.log, {"in": src}), got, err


@pytest.mark.parametrize("per, fmt, forward, scale, pinned", STREAMS)
def test_detect_stream(per, fmt, forward, scale, pinned, monkeypatch):
    log, got, err = run_stream(per, fmt, pinned, monkeypatch)
    want = stream_log(forward, scale)
    assert err is None and log == want
    # chunk k runs on engine k & 1, and the forward of chunk k + 1 is in the log before the decode of chunk k
    fwds = [k for k, e in enumerate(log) if e[1].startswith("forward")]
    decs = [k for k, e in enumerate(log) if e[1] == "decode_threshold"]
    assert [log[k][0] for k in fwds] == ["e0", "e1", "e0"] == [log[k][0] for k in decs]
    assert fwds[1] < decs[0] and fwds[2] < decs[1]
    check_results([r for r, _ in got])
    # the results of chunk k are yielded right behind its decode and rescale-off, before anything else is enqueued
    assert [at for _, at in got] == [decs[0] + 2] * 2 + [decs[1] + 2] * 2 + [decs[2] + 2]


def test_detect_stream_failures(monkeypatch):
    """A failed enqueue switches that context's rescale off again (it is per-context state); so does a failed decode."""
    forward = fwd("forward_resized_enqueue", BGR, "tmp")
    log, got, err = run_stream(BGR, None, False, monkeypatch, fail=("forward", 1))
    assert isinstance(err, Boom) and got == []
    assert log == stream_log(forward, S_BGR)[:4] + [("e1", "set_rescale", 0.0, 0.0)]
    log, got, err = run_stream(BGR, None, False, monkeypatch, fail=("decode_threshold", 1))
    assert isinstance(err, Boom) and len(got) == 2
    want = stream_log(forward, S_BGR)
    at = [k for k, e in enumerate(want) if e[1] == "decode_threshold"][1]
    assert log == want[:at + 1] + [("e1", "set_rescale", 0.0, 0.0)]


# ------------------------------------------------------------------------------------------------ landmarks=False, refusals
@pytest.mark.parametrize("c", [p for p in CASES if p.id in ("detect_batch-resized", "detect_yuv-array", "detect_tiled-redact", "anonymize-mosaic",
                                                            "anonymize_yuv-blur-tracker", "anonymize-tiled")])
def test_without_landmarks_the_boxes_come_alone(c, monkeypatch):
    log, src, before, ret = run(c, monkeypatch, landmarks=False)
    assert log == c["expect"]()
    check_results(ret[1] if c["returns"] == "out" else ret, landmarks=False)


def test_detect_stream_without_landmarks(monkeypatch):
    log, got, err = run_stream(BGR, None, False, monkeypatch, landmarks=False)
    assert err is None
    check_results([r for r, _ in got], landmarks=False)


def test_refusals_come_before_any_engine_call():
    script = Script()
    face = make_face((YH, YW), StubEngine(script), landmarks=False)
    imgs, yuv = np.zeros((N,) + BGR_EVEN, np.uint8), np.zeros((N,) + YUV, np.uint8)
    for call in (lambda: face.detect_aligned(imgs, 16), lambda: face.detect_aligned_frames(imgs, "bgr", 16),
                 lambda: face.detect_aligned_frames(yuv, "nv12", 16), lambda: face.detect_aligned_frames(imgs, "bgr", 16, tiled=True)):
        with pytest.raises(ValueError, match="needs the landmarks"):
            call()
    face.landmarks = True
    for bad in (dict(mode="blur", cell=6), dict(mode="blur", fill=(1, 2, 3)), dict(mode="mosaic", radius=3), dict(radius=3)):
        for call in (lambda: face.anonymize(imgs, **bad), lambda: face.anonymize(imgs, tiled=True, **bad), lambda: face.anonymize_yuv(yuv, "nv12", **bad),
                     lambda: face.anonymize_yuv(yuv, "nv12", tiled=True, **bad), lambda: face.detect_tiled(imgs, redact=bad),
                     lambda: face.anonymize(imgs, tracker=TRK, **bad)):
            with pytest.raises(ValueError, match="radius belongs|takes shape, radius and scale"):
                call()
    with pytest.raises(ValueError, match="need max_batch >= 3"):
        face.detect_tiled(np.zeros((1,) + BGR_WIDE, np.uint8))                    # two tiles and the whole frame, max_batch = 2
    with pytest.raises(ValueError, match="this instance was built for"):
        face.detect_aligned_frames(np.zeros((N,) + BGR, np.uint8), "bgr", 16)
    with pytest.raises(ValueError, match="frames must be uint8"):
        face.detect_yuv(np.zeros((N,) + BGR, np.uint8))
    assert script.log == []
