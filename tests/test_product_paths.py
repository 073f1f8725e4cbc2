"""What CenterFace's product methods ask of their engine, pinned without a GPU: every method runs against a recording stand-in for
``Engine`` and the exact sequence of public Engine calls -- chunking, input form, rescale on / off, tracker stream offsets, which slice of
which array is covered -- is compared with a restatement of the chunk loop, together with what the method returns.  Only ``ops.tile_grid``
(host-only library code) is real.  ``pinned_copy`` needs a GPU, so the page-locked input form is reached by stubbing ``is_pinned``."""
import re

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
FOLLOWED, M = (1, 0, 2, 1, 3), 4     # rows per image that a follow returns, of M slots
TRK, SCN = object(), object()
SAME, CUT = cfa._lib.CF_SCENE_SAME, cfa._lib.CF_SCENE_CUT
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


def followed(i):
    """The tracker's rows of image i as ``track_follow`` hands them out: FOLLOWED[i] valid rows of M, the rest zero."""
    d, l = np.zeros((M, 5), np.float32), np.zeros((M, 10), np.float32)
    n = FOLLOWED[i]
    d[:n] = (7000.0 + 100.0 * i + np.arange(n * 5, dtype=np.float32)).reshape(n, 5)
    l[:n] = (9000.0 + 100.0 * i + np.arange(n * 10, dtype=np.float32)).reshape(n, 10)
    return d, l


class Script(object):
    """What the engines of one case share: the call log, the index of the next image, the call that is to fail, the images whose scene
    check says CUT (every other says SAME)."""

    def __init__(self, fail=None, cuts=()):
        self.log, self.next, self.fail, self.seen, self.cuts = [], 0, fail, {}, cuts


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

    def forward_fit_enqueue(self, frames, fmt="bgr", *, anchor="center", upscale=True, fill=(0, 0, 0)):
        self._forward("forward_fit_enqueue", frames, fmt, dict(anchor=anchor, upscale=upscale, fill=fill))      # (what the engine is asked, spelled out or not)

    def unfit_rows(self, max_out=1024):
        self._log("unfit_rows", max_out)
        return self._mine(), np.zeros((self.B,), np.int32)

    def track_update_device(self, tracker, stream0=0):
        self._log("track_update_device", tracker is TRK, stream0)

    def scene_check(self, frames, fmt, scenes, tracker=None, stream0=0, *, codes=True, out_ptr=None):
        self._log("scene_check", _desc(frames), fmt, scenes is SCN, tracker is TRK, stream0, codes, out_ptr)
        self.s.next = stream0                                              # the chunk of image stream0, whether or not the chunks before it ran a forward
        if codes and not out_ptr:
            return np.array([[CUT if stream0 + b in self.s.cuts else SAME, 0, 0, 0] for b in range(len(frames))], np.int32)

    def track_follow(self, frames, fmt, tracker, stream0=0, **options):
        self._log("track_follow", _desc(frames), fmt, tracker is TRK, stream0, options)
        self.first, self.B = stream0, len(frames)                          # the engine now holds the followed rows of these images
        rows = [followed(i) for i in range(stream0, stream0 + len(frames))]
        return (np.stack([d for d, _ in rows]), np.stack([l for _, l in rows]), None, np.array(FOLLOWED[stream0:stream0 + len(frames)], np.int32),
                None)

    def _mark(self, frames, at):
        for b in range(self.B):                                            # leaves a mark in every frame that has faces
            if COUNTS[self.first + b]:
                frames[b].reshape(-1)[at] ^= 0xFF
        return frames

    def cover_faces(self, frames, fmt="bgr", **options):
        self._log("cover_faces", _desc(frames), fmt, options)
        return self._mark(frames, 0)

    def draw_faces(self, frames, fmt="bgr", **options):
        self._log("draw_faces", _desc(frames), fmt, options)
        return self._mark(frames, 1)

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


def case(id, method, per, expect, args=(), kw=None, hw=None, as_list=False, pinned=False, returns="dets", in_place=False, **more):
    hw = hw or ((per[0], per[1]) if len(per) == 3 else (per[0] * 2 // 3, per[1]))
    if per == BGR_WIDE:
        hw = (YH, YW)                                                      # tiled: frames of any even size
    # (the last line: what only the cases of the later steps set -- whose rows are returned, which byte is marked, the CUT images, which
    # forward or decode is made to fail, whether the decode rescales)
    return pytest.param(dict(dict(method=method, per=per, expect=expect, args=args, kw=kw or {}, hw=hw, as_list=as_list, pinned=pinned,
                                  returns=returns, in_place=in_place,
                                  rows="canned", mark=0, cuts=(), fail_at=1, rescales=True), **more), id=id)


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


# ------------------------------------------------------------------------------------------------ the later steps, restated
FIT = dict(anchor="center", upscale=True, fill=(0, 0, 0))
COLOURS = dict(box_color=(2, 255, 0), lm_color=(0, 0, 255), held_color=(0, 255, 255), text_color=(0, 0, 0))


def draw_options(label, yuv=False, landmarks=True, **given):
    """The complete options ``draw_faces`` gets: the reference's look, the label by tracker, 4:2:0 colours converted."""
    o = dict(COLOURS, thickness=1, radius=2, label=label, label_scale=2, dash_held=True, scale=1.0, landmarks=landmarks)
    o.update(given)
    return dict(o, **{k: ops.bgr_to_yuv_color(o[k]) for k in COLOURS}) if yuv else o


def steps(kind, per, where, fmt="bgr", *, reads="tmp", fit=FIT, scenes=False, track=False, follow=None, detect=True, cuts=(), cover=None, draw=None,
          chips=False):
    """The chunk loop with every step.  ``kind`` 'fit' / 'tiled': the forward reads the frames in ``where``, the rows reach frame space by
    ``unfit_rows`` / ``merge_tiles``, and there is no rescale; otherwise ``kind`` names the enqueue of the untiled path, which reads
    ``reads``, and the decode rescales.  Per chunk: the scene check; the detection -- forward, decode, rows to frame space, update --
    with ``detect``, else only in a chunk that holds one of the ``cuts``; the follow; cover, draw, chips, all on the slice of ``where``.
    The rescale is on for the whole call with ``detect``, else only around the detection of a key chunk."""
    hw = per[:2] if len(per) == 3 else (per[0] * 2 // 3, per[1])
    n, scale, to_frame = NB, None, []
    if kind == "fit":
        forward, to_frame = fwd("forward_fit_enqueue", per, where, fmt, fit), [("unfit_rows", MAXD)]
    elif kind == "tiled":
        rects = tuple(map(tuple, ops.tile_grid(hw[0], hw[1], (NH, NW), 24, True).tolist()))
        forward, n, to_frame = fwd("forward_tiles_enqueue", per, where, rects, fmt), NB // len(rects), [("merge_tiles", "ios", 0.5, 2.0, MAXD)]
    else:
        forward, scale = fwd(kind, per, reads, *((fmt,) if kind == "forward_yuv_enqueue" else ())), (NH / hw[0], NW / hw[1])
    on, off = ([("set_rescale",) + scale], [("set_rescale", 0.0, 0.0)]) if scale else ([], [])
    log = list(on) if detect else []
    for i in range(0, N, n):
        b = min(n, N - i)
        part = chunk(i, b, per, where)
        log += [("scene_check", part, fmt, True, True, i, not detect, None)] if scenes else []
        if detect or any(i <= k < i + b for k in cuts):
            log += ([] if detect else on) + [forward(i, b), ("decode_threshold", 0.3, NMS, MAXD)] + to_frame
            log += [("track_update_device", True, i)] if track else []
            log += [] if detect else off
        log += [("track_follow", part, fmt, True, i, follow)] if follow is not None else []
        log += [("cover_faces", part, fmt, cover)] if cover is not None else []
        log += [("draw_faces", part, fmt, draw)] if draw is not None else []
        log += [("align_faces_frame", part, fmt, 16, CHIP)] if chips else []
    return log + (off if detect else [])


def step_case(id, method, kind, per, where, fmt="bgr", args=(), kw=None, *, as_list=False, returns="dets", in_place=False, rows="canned", cuts=(),
              **said):
    return case(id, method, per, lambda: steps(kind, per, where, fmt, cuts=cuts, **said), args, kw, as_list=as_list, returns=returns, in_place=in_place,
                rows=rows, mark=0 if said.get("draw") is None else 1, cuts=cuts, fail_at=0 if cuts else 1, rescales=kind not in ("fit", "tiled"))


RESIZED, FROM_YUV = "forward_resized_enqueue", "forward_yuv_enqueue"


def _fit_cases():
    return [step_case("detect_fit-bgr", "detect_fit", "fit", BGR, "in"),
            step_case("detect_fit-nv12", "detect_fit", "fit", YUV, "in", "nv12", ("nv12",)),
            step_case("detect_fit-options", "detect_fit", "fit", BGR, "in", kw=dict(anchor="topleft", upscale=False, fill=(1, 2, 3)),
                      fit=dict(anchor="topleft", upscale=False, fill=(1, 2, 3))),
            step_case("detect_fit-redact-tracker", "detect_fit", "fit", BGR, "in", kw=dict(redact=MOSAIC, tracker=TRK), in_place=True, track=True, cover=MOSAIC),
            step_case("anonymize-fit", "anonymize", "fit", BGR, "out", kw=dict(MOSAIC, fit=True), as_list=True, returns="out", cover=MOSAIC),
            step_case("anonymize_yuv-fit-topleft", "anonymize_yuv", "fit", YUV, "out", "nv12", ("nv12",), dict(BLUR, fit=dict(anchor="topleft"), tracker=TRK),
                      returns="out", fit=dict(FIT, anchor="topleft"), track=True, cover=BLUR),
            step_case("detect_aligned_frames-fit", "detect_aligned_frames", "fit", BGR, "in", args=("bgr", 16), kw=dict(CHIP, fit=True), returns="chips",
                      chips=True)]


def _draw_cases():
    out = []
    for tag, kw, label in (("", {}, "score"), ("-tracker", dict(tracker=TRK), "id")):
        t = dict(returns="out", track=bool(kw))
        out += [step_case("annotate-plain" + tag, "annotate", RESIZED, BGR, "out", kw=kw, as_list=True, draw=draw_options(label), **t),
                step_case("annotate-tiled" + tag, "annotate", "tiled", BGR_EVEN, "out", kw=dict(kw, tiled=True), draw=draw_options(label), **t),
                step_case("annotate-fit" + tag, "annotate", "fit", BGR, "out", kw=dict(kw, fit=True), as_list=True, draw=draw_options(label), **t),
                step_case("annotate_yuv-plain" + tag, "annotate_yuv", FROM_YUV, YUV, "out", "nv12", kw=kw, reads="in", draw=draw_options(label, True), **t),
                step_case("annotate_yuv-tiled" + tag, "annotate_yuv", "tiled", YUV, "out", "nv21", ("nv21",), dict(kw, tiled=True), as_list=True,
                          draw=draw_options(label, True), **t),
                step_case("annotate_yuv-fit" + tag, "annotate_yuv", "fit", YUV, "out", "i420", ("i420",), dict(kw, fit=dict(fill=(9, 9, 9))),
                          fit=dict(FIT, fill=(9, 9, 9)), draw=draw_options(label, True), **t)]
    given = dict(thickness=3, box_color=(9, 8, 7), dash_held=False)
    return out + [step_case("annotate-options", "annotate", RESIZED, BGR, "out", kw=given, returns="out", draw=draw_options("score", **given)),
                  step_case("annotate_yuv-options", "annotate_yuv", FROM_YUV, YUV, "out", "nv12", kw=dict(given, tracker=TRK), reads="in", returns="out",
                            track=True, draw=draw_options("id", True, **given))]


def _follow_cases():
    out = []
    for tag, arg, o in (("", True, {}), ("-search", dict(search=2), dict(search=2))):
        t = dict(track=True, follow=o)
        out += [step_case("anonymize-follow" + tag, "anonymize", RESIZED, BGR, "out", kw=dict(MOSAIC, tracker=TRK, follow=arg), as_list=True, returns="out",
                          cover=MOSAIC, **t),
                step_case("detect_tiled-redact-follow" + tag, "detect_tiled", "tiled", BGR_EVEN, "in", kw=dict(redact=BLUR, tracker=TRK, follow=arg),
                          in_place=True, cover=BLUR, **t)]
    return out


def _detect_false_cases():
    kw, t = dict(tracker=TRK, detect=False), dict(rows="followed", detect=False, track=True, follow={})
    return [step_case("anonymize-nodetect", "anonymize", RESIZED, BGR, "out", kw=dict(MOSAIC, **kw), as_list=True, returns="out", cover=MOSAIC, **t),
            step_case("anonymize-nodetect-max_sad", "anonymize", RESIZED, BGR, "out", kw=dict(MOSAIC, follow=dict(max_sad=99), **kw), returns="out",
                      cover=MOSAIC, **dict(t, follow=dict(max_sad=99))),
            step_case("anonymize-fit-nodetect", "anonymize", "fit", BGR, "out", kw=dict(MOSAIC, fit=True, **kw), returns="out", cover=MOSAIC, **t),
            step_case("anonymize_yuv-tiled-nodetect", "anonymize_yuv", "tiled", YUV, "out", "nv12", kw=dict(BLUR, tiled=True, **kw), returns="out",
                      cover=BLUR, **t),
            step_case("annotate-tiled-nodetect", "annotate", "tiled", BGR_EVEN, "out", kw=dict(tiled=True, **kw), returns="out", draw=draw_options("id"), **t),
            step_case("annotate_yuv-nodetect", "annotate_yuv", FROM_YUV, YUV, "out", "nv12", kw=kw, reads="in", returns="out",
                      draw=draw_options("id", True), **t),
            step_case("detect_tiled-redact-nodetect", "detect_tiled", "tiled", BGR_EVEN, "in", kw=dict(redact=MOSAIC, **kw), in_place=True, cover=MOSAIC, **t),
            step_case("detect_fit-redact-nodetect", "detect_fit", "fit", YUV, "in", "nv12", ("nv12",), dict(redact=MOSAIC, **kw), in_place=True,
                      cover=MOSAIC, **t)]


def _scene_cases():
    kw, t = dict(tracker=TRK, scenes=SCN), dict(scenes=True, track=True)
    key = dict(t, rows="followed", detect=False, follow={})
    return [step_case("anonymize-scenes", "anonymize", RESIZED, BGR, "out", kw=dict(MOSAIC, **kw), as_list=True, returns="out", cover=MOSAIC, **t),
            step_case("annotate_yuv-scenes-follow", "annotate_yuv", FROM_YUV, YUV, "out", "nv12", kw=dict(kw, follow=True), reads="in", returns="out",
                      draw=draw_options("id", True), follow={}, **t),
            step_case("detect_tiled-redact-scenes", "detect_tiled", "tiled", BGR_EVEN, "in", kw=dict(redact=MOSAIC, **kw), in_place=True, cover=MOSAIC, **t),
            step_case("detect_fit-redact-scenes", "detect_fit", "fit", BGR, "in", kw=dict(redact=BLUR, **kw), in_place=True, cover=BLUR, **t),
            step_case("anonymize-scenes-key", "anonymize", RESIZED, BGR, "out", kw=dict(MOSAIC, detect=False, **kw), as_list=True, returns="out", cuts=(3,),
                      cover=MOSAIC, **key),
            step_case("annotate-scenes-first-chunk-key", "annotate", RESIZED, BGR, "out", kw=dict(detect=False, **kw), returns="out", cuts=(0,),
                      draw=draw_options("id"), **key),
            step_case("anonymize_yuv-tiled-scenes-key", "anonymize_yuv", "tiled", YUV, "out", "nv12", kw=dict(BLUR, tiled=True, detect=False, **kw),
                      returns="out", cuts=(3,), cover=BLUR, **key),
            step_case("detect_fit-redact-scenes-key", "detect_fit", "fit", BGR, "in", kw=dict(redact=MOSAIC, detect=False, **kw), in_place=True, cuts=(4,),
                      cover=MOSAIC, **key)]


STEP_CASES = _fit_cases() + _draw_cases() + _follow_cases() + _detect_false_cases() + _scene_cases()


# ------------------------------------------------------------------------------------------------ running a case
def run(c, monkeypatch, fail=None, landmarks=True):
    """(resolved log, source array, its copy from before the call, what the method returned or the exception it raised)."""
    script = Script(fail, c["cuts"])
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


def marked(before, at=0):
    want = before.copy()
    for i, n in enumerate(COUNTS):
        if n:
            want[i].reshape(-1)[at] ^= 0xFF
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


def check_followed(results, hw, landmarks=True):
    """``detect=False``: the followed rows in float64, mapped by w / W, h / H where the tracker works in network coordinates (``hw``),
    as they are where it works in frame pixels (``hw`` None)."""
    fx, fy = (1.0, 1.0) if hw is None else (hw[1] / NW, hw[0] / NH)
    assert isinstance(results, list) and len(results) == N
    for i, r in enumerate(results):
        d, l = (a[:FOLLOWED[i]].astype(np.float64) for a in followed(i))
        d[:, 0:4:2], d[:, 1:4:2], l[:, 0::2], l[:, 1::2] = d[:, 0:4:2] * fx, d[:, 1:4:2] * fy, l[:, 0::2] * fx, l[:, 1::2] * fy
        got = r if landmarks else (r,)
        assert len(got) == (2 if landmarks else 1)
        for g, w in zip(got, (d, l)):
            assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == w.shape and np.array_equal(g, w), (i, g, w)


@pytest.mark.parametrize("c", STEP_CASES)
def test_product_path_with_the_later_steps(c, monkeypatch):
    """Fit, draw, follow, ``detect=False`` and scenes: the same comparison as ``test_product_path``, against ``steps``."""
    log, src, before, ret = run(c, monkeypatch)
    assert log == c["expect"]()
    if c["returns"] == "out":
        out, results = ret
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == src.shape and not np.shares_memory(out, src)
        assert np.array_equal(out, marked(before, c["mark"])) and np.array_equal(src, before)
    else:
        results = ret
        assert np.array_equal(src, marked(before, c["mark"]) if c["in_place"] else before)
    if c["rows"] == "followed":
        check_followed(results, c["hw"] if c["rescales"] else None)
        assert not any(e[0].startswith("forward") or e[0] in ("decode_threshold", "track_update_device", "set_rescale") for e in log) or c["cuts"]
    else:
        check_results(results, chips=c["returns"] == "chips")
    if not c["rescales"]:
        assert not any(e[0] == "set_rescale" for e in log)
    if c["cuts"]:                                                          # exactly one chunk is a key chunk
        assert sum(e[0].startswith("forward") for e in log) == 1 == sum(e[0] == "track_update_device" for e in log)


@pytest.mark.parametrize("c", [p for p in STEP_CASES if p.id in ("annotate-plain", "annotate_yuv-tiled-tracker", "anonymize-nodetect", "detect_fit-bgr",
                                                                 "detect_tiled-redact-nodetect", "anonymize-scenes-key")])
def test_the_later_steps_without_landmarks(c, monkeypatch):
    """``landmarks`` of the draw options follows the instance, and the boxes come alone -- the followed ones too."""
    log, src, before, ret = run(c, monkeypatch, landmarks=False)
    want = [e[:3] + (dict(e[3], landmarks=False),) if e[0] == "draw_faces" else e for e in c["expect"]()]
    assert log == want
    results = ret[1] if c["returns"] == "out" else ret
    if c["rows"] == "followed":
        check_followed(results, c["hw"] if c["rescales"] else None, landmarks=False)
    else:
        check_results(results, landmarks=False)


def test_the_later_steps_cover_every_product_method_and_skip_nothing():
    new = STEP_CASES + REFUSALS
    assert {"detect_fit", "detect_tiled", "detect_aligned_frames", "anonymize", "anonymize_yuv", "annotate", "annotate_yuv"} <= {
        p.values[0]["method"] for p in STEP_CASES}
    assert "best_shots" in {p.values[0] for p in REFUSALS}                   # (its call sequences: test_bestshot_abi.py)
    assert len(STEP_CASES) >= 40 and len(REFUSALS) >= 60 and not any(p.marks for p in new)


FAILING = [p for p in CASES if p.id in ("detect_batch-resized", "detect_batch-pinned", "detect_yuv-list", "detect_aligned-resized", "detect_aligned_frames-nv12",
                                        "anonymize-mosaic-tracker", "anonymize_yuv-blur", "anonymize-pinned")]
FAILING += [p for p in STEP_CASES if p.id in ("anonymize-fit", "anonymize-scenes-key")]


def strip_out(entries):
    """(The arrays of a call that raised are gone: the copy that anonymize would have returned resolves to 'tmp'.)"""
    return [tuple(v[:2] if isinstance(v, tuple) and len(v) == 4 and v[2] in ("out", "tmp") else v for v in e) for e in entries]


@pytest.mark.parametrize("kind", ("forward", "decode_threshold"))
@pytest.mark.parametrize("c", FAILING)
def test_a_failing_second_chunk_switches_the_rescale_off(c, kind, monkeypatch):
    """The enqueue or the decode of the second chunk raises: the exception propagates, the log ends with set_rescale(0, 0) right behind
    the failed call, and nothing was tracked, covered or cut for that chunk.  A fitted path never switched the rescale on: its log ends
    with the failed call.  With ``detect=False`` the one forward and decode of the call are the key chunk's, and the rescale that was
    switched on for them goes off right behind the failed call."""
    log, src, before, ret = run(c, monkeypatch, fail=(kind, c["fail_at"]))
    assert isinstance(ret, Boom)
    full = c["expect"]()
    at = [k for k, e in enumerate(full) if (e[0].startswith("forward") if kind == "forward" else e[0] == kind)][c["fail_at"]]
    if not c["rescales"]:
        assert strip_out(log) == strip_out(full[:at + 1]) and not any(e[0] == "set_rescale" for e in log) and np.array_equal(src, before)
        return
    assert strip_out(log) == strip_out(full[:at + 1] + [("set_rescale", 0.0, 0.0)])
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


# ------------------------------------------------------------------------------------------------ the refusals every method shares
SHOTS = type("Shots", (), {"size": 16, "streams": 8, "entries": 4})()
NEEDS_TRACKER, SCENES_TRACKER, LOOK_TRACKER = "follow= and detect=False need tracker=", "scenes= needs tracker=", "lookback= needs tracker="
FLUSH, LOOK_REDACT, FIT_TILED = "flush= needs lookback=", "lookback= needs redact=", "fit= and tiled=True exclude each other"
FIT_KEYS, FOLLOW_KEYS = "fit takes anchor, upscale and fill, got ['radius']", "follow takes search and max_sad, got ['radius']"
TOO_MANY, UNEQUAL = "5 images for a lookback object with 3 streams", "different fill levels of the lookback object: [1, 0, 0, 0, 0]"
BUILT_FOR, NDIM = "(this instance was built for 76x102)", "frames must be uint8 [B,h,w,3] (bgr) or [B, h*3//2, w] (4:2:0), got"


class Uneven(cfa.Lookback):
    def fill(self, stream):
        return 1 if stream == 0 else 0


LOOKBACKS = {"eight": lambda: cfa.Lookback(0, 8), "three": lambda: cfa.Lookback(0, 3), "uneven": lambda: Uneven(0, 8)}
FRAMES = {"bgr": (N,) + BGR_EVEN, "yuv": (N,) + YUV, "odd": (N,) + BGR}


def _refusals():
    """(method, frames, arguments, keywords, landmarks, message): ``lookback`` names an entry of LOOKBACKS, made when the case runs."""
    rows = []
    add = lambda tag, m, f, a, kw, text, landmarks=True: rows.append(pytest.param(m, f, a, kw, landmarks, text, id="%s-%s" % (m, tag)))      # noqa: E731
    six = (("anonymize", "bgr", (), {}), ("anonymize_yuv", "yuv", ("nv12",), {}), ("annotate", "bgr", (), {}), ("annotate_yuv", "yuv", ("nv12",), {}),
           ("detect_tiled", "bgr", (), dict(redact=MOSAIC)), ("detect_fit", "bgr", (), dict(redact=MOSAIC)))
    shots = ("best_shots", "bgr", (), dict(tracker=TRK, shots=SHOTS))
    for m, f, a, kw in six:
        add("follow", m, f, a, dict(kw, follow=True), NEEDS_TRACKER)
        add("follow-options", m, f, a, dict(kw, follow=dict(search=2)), NEEDS_TRACKER)
        add("nodetect", m, f, a, dict(kw, detect=False), NEEDS_TRACKER)
        add("scenes", m, f, a, dict(kw, scenes=SCN), SCENES_TRACKER)
        add("lookback", m, f, a, dict(kw, lookback="eight"), LOOK_TRACKER)
        add("flush", m, f, a, dict(kw, flush=True), FLUSH)
        add("flush-tracker", m, f, a, dict(kw, flush=True, tracker=TRK), FLUSH)
        add("streams", m, f, a, dict(kw, tracker=TRK, lookback="three"), TOO_MANY)
        add("fill", m, f, a, dict(kw, tracker=TRK, lookback="uneven"), UNEQUAL)
        # which of two comes first: the lookback's rules stand before the follow's and the scenes'
        add("lookback-before-follow", m, f, a, dict(kw, lookback="eight", follow=True), LOOK_TRACKER)
        add("lookback-before-scenes", m, f, a, dict(kw, lookback="eight", scenes=SCN), LOOK_TRACKER)
        add("follow-before-scenes", m, f, a, dict(kw, follow=True, scenes=SCN), NEEDS_TRACKER)
    for m, f, a, kw in six + (shots,):
        add("follow-keys", m, f, a, dict(kw, tracker=TRK, follow=dict(radius=2)), FOLLOW_KEYS)
    for m, f, a, kw in (("detect_tiled", "bgr", (), {}), ("detect_fit", "yuv", ("nv12",), {})):
        add("lookback-redact", m, f, a, dict(kw, tracker=TRK, lookback="eight"), LOOK_REDACT)
        add("lookback-redact-first", m, f, a, dict(kw, lookback="eight"), LOOK_REDACT)      # ... and before the missing tracker
    for m, f, a, kw in six[:4] + (("detect_aligned_frames", "bgr", ("bgr", 16), {}), shots):
        add("fit-tiled", m, f, a, dict(kw, fit=True, tiled=True), FIT_TILED)
        add("fit-options-tiled", m, f, a, dict(kw, fit=dict(anchor="topleft"), tiled=True), FIT_TILED)
        add("fit-keys", m, f, a, dict(kw, fit=dict(radius=2)), FIT_KEYS)
        add("fit-tiled-first", m, f, a, dict(kw, fit=True, tiled=True, follow=True, scenes=SCN, flush=True) if m not in ("detect_aligned_frames", "best_shots")
            else dict(kw, fit=True, tiled=True), FIT_TILED, landmarks=False)
    add("fit-tiled-before-lookback", "anonymize", "bgr", (), dict(fit=True, tiled=True, lookback="eight"), FIT_TILED)
    add("fit-tiled-before-landmarks", "best_shots", "bgr", (), dict(fit=True, tiled=True, tracker=None, shots=None), FIT_TILED, False)
    add("landmarks", "best_shots", "bgr", (), shots[3], "best_shots needs the landmarks", False)
    add("landmarks-before-tracker", "best_shots", "bgr", (), dict(tracker=None, shots=SHOTS), "best_shots needs the landmarks", False)
    add("tracker", "best_shots", "bgr", (), dict(tracker=None, shots=SHOTS), "best_shots needs tracker= and shots=")
    add("shots", "best_shots", "bgr", (), dict(tracker=TRK, shots=None), "best_shots needs tracker= and shots=")
    add("tracker-before-follow", "best_shots", "bgr", (), dict(tracker=None, shots=SHOTS, follow=True), "best_shots needs tracker= and shots=")
    add("scenes-keys", "best_shots", "bgr", (), dict(shots[3], follow=dict(radius=2), scenes=SCN), FOLLOW_KEYS)
    for m, a, kw in (("detect_aligned_frames", ("bgr", 16), {}), ("best_shots", (), shots[3])):
        add("shape", m, "odd", a, kw, BUILT_FOR)
        add("shape-yuv", m, "bgr", ("nv12",) + a[1:], kw, NDIM)
        add("ndim", m, "yuv", a, kw, NDIM)
    add("shape-4:2:0", "detect_aligned_frames", "bgr", ("nv12", 16), {}, NDIM)
    return rows


REFUSALS = _refusals()


@pytest.mark.parametrize("method, frames, args, kw, landmarks, text", REFUSALS)
def test_a_refusal_names_its_rule_before_any_engine_call(method, frames, args, kw, landmarks, text):
    script = Script()
    face = make_face((YH, YW), StubEngine(script), landmarks=landmarks)
    lb = LOOKBACKS[kw["lookback"]]() if "lookback" in kw else None
    src = np.zeros(FRAMES[frames], np.uint8)
    with pytest.raises(ValueError, match=re.escape(text)):
        getattr(face, method)(src, *args, **(kw if lb is None else dict(kw, lookback=lb)))
    assert script.log == [] and not src.any()
    if lb is not None:
        lb.close()
