"""ctypes binding of libcenterface_hip.so (include/centerface_hip.h).  No CPU fallback: if the
library is missing or a call fails this module raises."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CF_LIB: load another build of the same library (A/B runs of kernel variants: tools/ab_build.sh); default = the in-tree build
LIB_PATH = os.environ.get("CF_LIB") or os.path.join(_HERE, "libcenterface_hip.so")
CSRC = os.path.join(_HERE, "csrc")

CF_OK = 0
CF_F32, CF_BF16, CF_F32_SPLIT = 0, 1, 2
CF_IN_U8_HWC_BGR, CF_IN_F32_NCHW = 0, 1
CF_FLAG_COLLAPSE_HEADS, CF_FLAG_NO_GRAPH, CF_FLAG_NO_FUSE, CF_FLAG_NO_UPHEAD, CF_FLAG_NO_NECK, CF_FLAG_NO_DECODE_STREAM, CF_FLAG_STREAM_HIGH = 1, 2, 4, 8, 16, 32, 64
CF_EOVERFLOW = -6
# 4:2:0 video frame formats of cf_forward_yuv / cf_op_yuv_to_bgr (cv2.COLOR_YUV2BGR_NV12 / _NV21 / _I420 / _YV12)
CF_YUV_NV12, CF_YUV_NV21, CF_YUV_I420, CF_YUV_YV12 = 0, 1, 2, 3
# chip formats of cf_align_faces / cf_op_align_faces
CF_CHIP_U8_HWC_BGR, CF_CHIP_F32_NCHW = 0, 1
CHIP_FORMATS = {"u8": CF_CHIP_U8_HWC_BGR, "uint8": CF_CHIP_U8_HWC_BGR, "f32": CF_CHIP_F32_NCHW, "float32": CF_CHIP_F32_NCHW}
CF_ESTATE = -4
# cf_redact_faces / cf_op_redact: CF_FRAME_BGR continues the CF_YUV_* numbering (one `format` integer for both families)
CF_FRAME_BGR = 4
CF_REDACT_SOLID, CF_REDACT_MOSAIC = 0, 1
CF_REDACT_RECT, CF_REDACT_ELLIPSE = 0, 1
REDACT_MODES = {"solid": CF_REDACT_SOLID, "mosaic": CF_REDACT_MOSAIC}
REDACT_SHAPES = {"rect": CF_REDACT_RECT, "ellipse": CF_REDACT_ELLIPSE}
# cf_draw_faces / cf_op_draw
CF_DRAW_BOX, CF_DRAW_LANDMARKS = 1, 2
CF_DRAW_LABEL_NONE, CF_DRAW_LABEL_SCORE, CF_DRAW_LABEL_ID = 0, 1, 2
DRAW_LABELS = {"none": CF_DRAW_LABEL_NONE, "score": CF_DRAW_LABEL_SCORE, "id": CF_DRAW_LABEL_ID}
# cf_merge_tiles / cf_op_merge_tiles
CF_ENOMEM = -2
CF_MERGE_IOU, CF_MERGE_IOS = 0, 1
MERGE_METRICS = {"iou": CF_MERGE_IOU, "ios": CF_MERGE_IOS}
# cf_forward_fit / cf_op_fit
CF_FIT_CENTER, CF_FIT_TOPLEFT = 0, 1
FIT_ANCHORS = {"center": CF_FIT_CENTER, "centre": CF_FIT_CENTER, "topleft": CF_FIT_TOPLEFT}
YUV_FORMATS = {"nv12": CF_YUV_NV12, "nv21": CF_YUV_NV21, "i420": CF_YUV_I420, "yuv420p": CF_YUV_I420, "yv12": CF_YUV_YV12}

# every symbol include/centerface_hip.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "cf_version", "cf_strerror", "cf_last_error", "cf_device_count", "cf_create", "cf_destroy",
    "cf_load_weights", "cf_forward", "cf_forward_resized", "cf_forward_yuv", "cf_forward_images", "cf_upload_images", "cf_forward_uploaded", "cf_get_resized_input", "cf_get_heads", "cf_decode_topk", "cf_decode_topk_post", "cf_affine_from_center_scale", "cf_decode_threshold", "cf_decode_threshold_ex", "cf_decode_threshold_sized", "cf_decode_threshold_enqueue", "cf_set_rescale",
    "cf_detect_topk", "cf_synchronize", "cf_event_record", "cf_event_elapsed_ms",
    "cf_profile_forward", "cf_plan_size", "cf_plan_op", "cf_forward_trace", "cf_graph_stats", "cf_get_streams", "cf_streams_share_queue", "cf_streams_share_queue_ex", "cf_spread_streams", "cf_reroll_streams", "cf_ctdet_loss", "cf_comm_unique_id", "cf_comm_create", "cf_comm_create_all", "cf_comm_create_loopback", "cf_comm_loopback_rank", "cf_comm_destroy", "cf_comm_abort", "cf_comm_query", "cf_comm_synchronize", "cf_comm_last_error", "cf_comm_debug", "cf_comm_set_shard", "cf_comm_stream", "cf_gather_topk", "cf_host_alloc", "cf_host_free", "cf_pinned_alloc", "cf_pinned_free", "cf_host_register", "cf_host_unregister", "cf_device_alloc", "cf_device_free", "cf_memcpy_h2d", "cf_memcpy_d2h",
    "cf_op_last_error", "cf_op_last_kernel", "cf_op_shufflev2", "cf_op_mbconv", "cf_op_expand_dw", "cf_op_mbconv_pick", "cf_op_expand_dw_pick", "cf_op_ctdet_loss", "cf_op_encode_targets", "cf_op_dwconv", "cf_op_dw_pick", "cf_op_pwconv", "cf_op_pwconv_ex", "cf_op_stem", "cf_op_idaup", "cf_op_heads",
    "cf_op_ctdet_decode", "cf_op_ctdet_post_process", "cf_op_decode_threshold", "cf_op_decode_threshold_ex", "cf_op_nms", "cf_op_box_match",
    "cf_op_yuv_to_bgr", "cf_align_faces", "cf_op_align_faces", "cf_align_faces_frame", "cf_op_align_frame", "cf_redact_faces", "cf_op_redact",
    "cf_blur_faces", "cf_op_blur",
    "cf_draw_faces", "cf_op_draw", "cf_draw_layout",
    "cf_tile_grid", "cf_forward_tiles", "cf_merge_tiles", "cf_op_cut_tiles", "cf_op_merge_tiles",
    "cf_fit_geometry", "cf_forward_fit", "cf_unfit_rows", "cf_op_fit", "cf_op_unfit",
    "cf_rot_geometry", "cf_forward_rot", "cf_op_rot", "cf_op_unrot",
    "cf_view_layout", "cf_forward_views", "cf_merge_views", "cf_op_views", "cf_op_merge_views",
    "cf_pack_views", "cf_forward_packed", "cf_merge_packed", "cf_op_packed", "cf_op_merge_packed",
    "cf_forward_packed_rot", "cf_op_packed_rot", "cf_op_merge_packed_rot",
    "cf_set_flip_test", "cf_op_mirror", "cf_op_flip_heads",
    "cf_track_create", "cf_track_destroy", "cf_track_reset", "cf_track_update", "cf_op_track",
    "cf_track_create_weak", "cf_op_track_weak",
    "cf_track_create_ex", "cf_op_track_ex", "cf_op_follow_ex",
    "cf_track_follow", "cf_op_follow",
    "cf_scene_create", "cf_scene_destroy", "cf_scene_forget", "cf_scene_check", "cf_op_scene",
    "cf_lookback_create", "cf_lookback_destroy", "cf_lookback_forget", "cf_lookback_step", "cf_op_lookback",
    "cf_lookback_trace_enable", "cf_lookback_step_frames", "cf_op_lookback_trace",
    "cf_bestshot_create", "cf_bestshot_destroy", "cf_bestshot_offer", "cf_bestshot_collect", "cf_op_chip_quality", "cf_op_bestshot",
)


class TensorDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("ndim", C.c_int32),
                ("dims", C.c_int64 * 4), ("dtype", C.c_int32)]


class OpTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("kind", C.c_char * 16), ("kernel", C.c_char * 160), ("ms", C.c_float),
                ("algo_bytes", C.c_double), ("flops", C.c_double)]


class OpInfo(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("kind", C.c_char * 16), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("fused_away", C.c_int32)]


class YuvPlanes(C.Structure):
    """cf_yuv_planes: the planes of one frame (c0 / c1 = the chroma planes in the format's order; c1 NULL for NV12 / NV21)."""
    _fields_ = [("y", C.c_void_p), ("c0", C.c_void_p), ("c1", C.c_void_p)]


class AlignOpts(C.Structure):
    """cf_align_opts: chip size / format / channel order / normalisation / template / per-image limit."""
    _fields_ = [("size", C.c_int32), ("format", C.c_int32), ("rgb", C.c_int32), ("mean", C.c_float), ("scale", C.c_float),
                ("tmpl", C.c_void_p), ("max_per_image", C.c_int32)]


def align_opts(size=112, out="u8", rgb=False, mean=0.0, scale=1.0, template=None, max_per_image=0):
    """(AlignOpts, the template array it points to or None -- keep it alive for the call, chip shape, chip dtype).  ``out``: 'u8'
    (uint8 [S,S,3] BGR) or 'f32' (float32 [3,S,S], ``(u8 - mean) * scale``, RGB planes with ``rgb``); integer codes pass through (the
    library validates them, like the size)."""
    if isinstance(out, str):
        if out.lower() not in CHIP_FORMATS:
            raise ValueError("unknown chip format %r (one of %s)" % (out, sorted(CHIP_FORMATS)))
        fmt = CHIP_FORMATS[out.lower()]
    else:
        fmt = int(out)
    tm = None
    if template is not None:
        tm = np.ascontiguousarray(template, dtype=np.float32)
        if tm.shape != (5, 2):
            raise ValueError("template must be [5][2] (x, y) points in chip pixels, got %s" % (tm.shape,))
    S = int(size)
    o = AlignOpts(S, fmt, 1 if rgb else 0, float(mean), float(scale), tm.ctypes.data if tm is not None else None, int(max_per_image))
    shape, dtype = ((3, S, S), np.float32) if fmt == CF_CHIP_F32_NCHW else ((S, S, 3), np.uint8)
    return o, tm, shape, dtype


class PlanesRW(C.Structure):
    """cf_planes_rw: the writable planes of one frame (BGR: p0 only; 4:2:0: Y, then the chroma planes in the format's order)."""
    _fields_ = [("p0", C.c_void_p), ("p1", C.c_void_p), ("p2", C.c_void_p)]


class RedactOpts(C.Structure):
    """cf_redact_opts: mode / shape / mosaic cell / box scale / fill bytes in the frame's channel order."""
    _fields_ = [("mode", C.c_int32), ("shape", C.c_int32), ("cell", C.c_int32), ("scale", C.c_float), ("fill", C.c_uint8 * 4)]


def redact_opts(mode="mosaic", shape="ellipse", cell=20, scale=1.3, fill=(0, 0, 0)):
    """RedactOpts from names ('solid' | 'mosaic', 'rect' | 'ellipse'); integer codes pass through (the library validates them, like
    the cell and the scale).  ``fill``: three bytes in the frame's own channel order (B,G,R or Y,U,V)."""
    def code(v, table, what):
        if isinstance(v, str):
            if v.lower() not in table:
                raise ValueError("unknown redaction %s %r (one of %s)" % (what, v, sorted(table)))
            return table[v.lower()]
        return int(v)
    fill = [int(v) for v in fill]
    if len(fill) != 3 or min(fill) < 0 or max(fill) > 255:
        raise ValueError("fill must be three bytes in the frame's channel order, got %r" % (fill,))
    return RedactOpts(code(mode, REDACT_MODES, "mode"), code(shape, REDACT_SHAPES, "shape"), int(cell), float(scale), (C.c_uint8 * 4)(*fill, 0))


class BlurOpts(C.Structure):
    """cf_blur_opts: shape / filter strength r (0 = per face, from the box size) / box scale."""
    _fields_ = [("shape", C.c_int32), ("radius", C.c_int32), ("scale", C.c_float)]


def blur_opts(shape="ellipse", radius=0, scale=1.3):
    """BlurOpts from a shape name ('rect' | 'ellipse'); integer codes pass through (the library validates them, like the radius and
    the scale)."""
    if isinstance(shape, str):
        if shape.lower() not in REDACT_SHAPES:
            raise ValueError("unknown redaction shape %r (one of %s)" % (shape, sorted(REDACT_SHAPES)))
        shape = REDACT_SHAPES[shape.lower()]
    return BlurOpts(int(shape), int(radius), float(scale))


class DrawOpts(C.Structure):
    """cf_draw_opts: what to draw / outline thickness / dot radius / label kind and scale / dashed held outlines / box scale / the four
    colours in the frame's channel order."""
    _fields_ = [("what", C.c_int32), ("thickness", C.c_int32), ("radius", C.c_int32), ("label", C.c_int32), ("label_scale", C.c_int32),
                ("dash_held", C.c_int32), ("scale", C.c_float), ("box_color", C.c_uint8 * 4), ("held_color", C.c_uint8 * 4),
                ("lm_color", C.c_uint8 * 4), ("text_color", C.c_uint8 * 4)]


def draw_opts(boxes=True, landmarks=True, thickness=1, radius=2, label="score", label_scale=2, dash_held=True, scale=1.0,
              box_color=(2, 255, 0), held_color=(0, 255, 255), lm_color=(0, 0, 255), text_color=(0, 0, 0), what=None):
    """DrawOpts: ``boxes`` / ``landmarks`` switch the outlines and the dots (``what``: the bits themselves, passed through), ``label``
    'none' | 'score' | 'id' (integer codes pass through; the library validates them, like the numbers).  The colours are three bytes
    in the frame's own channel order (B,G,R or Y,U,V; ``ops.bgr_to_yuv_color`` converts)."""
    if isinstance(label, str):
        if label.lower() not in DRAW_LABELS:
            raise ValueError("unknown label %r (one of %s)" % (label, sorted(DRAW_LABELS)))
        label = DRAW_LABELS[label.lower()]
    elif label is None:
        label = CF_DRAW_LABEL_NONE
    if what is None:
        what = (CF_DRAW_BOX if boxes else 0) | (CF_DRAW_LANDMARKS if landmarks else 0)

    def color(v, name):
        v = [int(x) for x in v]
        if len(v) != 3 or min(v) < 0 or max(v) > 255:
            raise ValueError("%s must be three bytes in the frame's channel order, got %r" % (name, v))
        return (C.c_uint8 * 4)(*v, 0)
    return DrawOpts(int(what), int(thickness), int(radius), int(label), int(label_scale), int(dash_held), float(scale),
                    color(box_color, "box_color"), color(held_color, "held_color"), color(lm_color, "lm_color"), color(text_color, "text_color"))


def split_redact_options(options):
    """Options of ``CenterFace.anonymize`` and its kin -> ('blur', blur_faces keywords) when ``mode`` is 'blur', else ('redact', the
    options as they are).  Blur takes shape, radius and scale; ``cell`` and ``fill`` belong to the other modes and are refused here,
    before RedactOpts is ever built."""
    mode = options.get("mode")
    if not (isinstance(mode, str) and mode.lower() == "blur"):
        if "radius" in options:
            raise ValueError("radius belongs to mode='blur'")
        return "redact", options
    extra = sorted(set(options) - {"mode", "shape", "radius", "scale"})
    if extra:
        raise ValueError("mode='blur' takes shape, radius and scale, not %s" % ", ".join(extra))
    return "blur", {k: v for k, v in options.items() if k != "mode"}


class TileRect(C.Structure):
    """cf_tile_rect: one rectangle of a frame, in frame pixels (all four values even)."""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class MergeOpts(C.Structure):
    """cf_merge_opts: suppression measure / threshold / edge margin in network pixels."""
    _fields_ = [("metric", C.c_int32), ("thresh", C.c_float), ("edge", C.c_float)]


def merge_opts(metric="ios", thresh=0.5, edge=2.0):
    """MergeOpts from a name ('iou' | 'ios'); integer codes pass through (the library validates them, like the numbers)."""
    if isinstance(metric, str):
        if metric.lower() not in MERGE_METRICS:
            raise ValueError("unknown merge metric %r (one of %s)" % (metric, sorted(MERGE_METRICS)))
        metric = MERGE_METRICS[metric.lower()]
    return MergeOpts(int(metric), float(thresh), float(edge))


class FitOpts(C.Structure):
    """cf_fit_opts: where the content sits in the canvas / whether a small frame is enlarged / the B, G, R bytes of the padding."""
    _fields_ = [("anchor", C.c_int32), ("upscale", C.c_int32), ("fill", C.c_uint8 * 4)]


class FitGeom(C.Structure):
    """cf_fit_geom: the content is rw x rh canvas pixels at (dx, dy)."""
    _fields_ = [("rw", C.c_int32), ("rh", C.c_int32), ("dx", C.c_int32), ("dy", C.c_int32)]


def fit_opts(anchor="center", upscale=True, fill=(0, 0, 0)):
    """FitOpts from an anchor name ('center' | 'topleft'); integer codes pass through (the library validates them, like ``upscale``).
    ``fill``: the three bytes B, G, R of the padding."""
    if isinstance(anchor, str):
        if anchor.lower() not in FIT_ANCHORS:
            raise ValueError("unknown fit anchor %r (one of %s)" % (anchor, sorted(FIT_ANCHORS)))
        anchor = FIT_ANCHORS[anchor.lower()]
    fill = [int(v) for v in fill]
    if len(fill) != 3 or min(fill) < 0 or max(fill) > 255:
        raise ValueError("fill must be three bytes B, G, R, got %r" % (fill,))
    return FitOpts(int(anchor), int(upscale), (C.c_uint8 * 4)(*fill, 0))


class View(C.Structure):
    """cf_view: a source rectangle of the frame (even values) and a content rectangle of the canvas."""
    _fields_ = [("sx0", C.c_int32), ("sy0", C.c_int32), ("sw", C.c_int32), ("sh", C.c_int32),
                ("dx", C.c_int32), ("dy", C.c_int32), ("dw", C.c_int32), ("dh", C.c_int32)]


class ViewOpts(C.Structure):
    """cf_view_opts: the tile grid (0, 0: none) / the anchor of the levels / the levels in per mille of the fitted size."""
    _fields_ = [("tile_h", C.c_int32), ("tile_w", C.c_int32), ("overlap", C.c_int32), ("anchor", C.c_int32), ("n_levels", C.c_int32),
                ("scale_pm", C.c_int32 * 8)]


def view_opts(tile=None, overlap=None, scales=(1.0,), anchor="center"):
    """ViewOpts from a tile size (None: no tiles; an int or (tile_h, tile_w)), the tiles' overlap (None: a fifth of the smaller tile
    side, rounded down to even), the levels as fractions of the fitted size (rounded to per mille; at most 8, each in 1..1000 per mille)
    and an anchor name ('center' | 'topleft')."""
    if isinstance(anchor, str):
        if anchor.lower() not in FIT_ANCHORS:
            raise ValueError("unknown anchor %r (one of %s)" % (anchor, sorted(FIT_ANCHORS)))
        anchor = FIT_ANCHORS[anchor.lower()]
    scales = [scales] if isinstance(scales, (int, float)) else list(scales)
    if len(scales) > 8:
        raise ValueError("at most 8 scales, got %d" % len(scales))
    pm = [int(round(float(v) * 1000.0)) for v in scales]
    for v, q in zip(scales, pm):
        if q < 1 or q > 1000:
            raise ValueError("scale %r is outside 0.001 .. 1.0" % (v,))
    if tile is None:
        th = tw = ov = 0
    else:
        th, tw = (int(tile), int(tile)) if isinstance(tile, int) else (int(tile[0]), int(tile[1]))
        ov = (min(th, tw) // 5) & ~1 if overlap is None else int(overlap)
    return ViewOpts(th, tw, ov, int(anchor), len(pm), (C.c_int32 * 8)(*pm))


def view_table(views):
    """(View table, V) of an int array-like [V][8] of (sx0, sy0, sw, sh, dx, dy, dw, dh) rows."""
    r = np.ascontiguousarray(views, dtype=np.int32).reshape(-1, 8)
    tab = (View * max(len(r), 1))()
    for v, row in enumerate(r.tolist()):
        (tab[v].sx0, tab[v].sy0, tab[v].sw, tab[v].sh, tab[v].dx, tab[v].dy, tab[v].dw, tab[v].dh) = row
    return tab, len(r)


class Place(C.Structure):
    """cf_place: one view of frame ``frame`` in canvas ``canvas`` (the view's content rectangle is its place in that canvas)."""
    _fields_ = [("frame", C.c_int32), ("canvas", C.c_int32), ("view", View)]


def place_table(places):
    """(Place table, P) of an int array-like [P][10] of (frame, canvas, sx0, sy0, sw, sh, dx, dy, dw, dh) rows."""
    r = np.ascontiguousarray(places, dtype=np.int32).reshape(-1, 10)
    tab = (Place * max(len(r), 1))()
    if len(r):
        C.memmove(tab, r.ctypes.data, r.nbytes)
    return tab, len(r)


def fill_bytes(fill):
    """The three bytes B, G, R of a padding colour as a ctypes array."""
    fill = [int(v) for v in fill]
    if len(fill) != 3 or min(fill) < 0 or max(fill) > 255:
        raise ValueError("fill must be three bytes B, G, R, got %r" % (fill,))
    return (C.c_uint8 * 4)(*fill, 0)


class RotOpts(C.Structure):
    """cf_rot_opts: the clockwise turn that makes the stored frame upright / stretch the upright view instead of fitting it / the fit."""
    _fields_ = [("rot", C.c_int32), ("stretch", C.c_int32), ("fit", FitOpts)]


def rot_opts(rot=0, fit=None):
    """RotOpts for a turn of ``rot`` clockwise degrees (the library validates the value).  ``fit`` = None: the upright view is stretched
    to the canvas; True: fitted with the default options; a dict: the keywords of ``fit_opts``."""
    if fit is None or fit is False:
        return RotOpts(int(rot), 1, fit_opts())
    return RotOpts(int(rot), 0, fit_opts(**({} if fit is True else dict(fit))))


class TrackOpts(C.Structure):
    """cf_track_opts: match threshold / frames a confirmed track is held / detections that confirm a track / slots per stream / growth of
    a held box per missed frame."""
    _fields_ = [("iou_thresh", C.c_float), ("max_age", C.c_int32), ("min_hits", C.c_int32), ("max_tracks", C.c_int32), ("hold_grow", C.c_float)]


def track_opts(iou=0.3, max_age=15, min_hits=2, max_tracks=256, hold_grow=0.0):
    """TrackOpts (the library validates the numbers).  The defaults are this project's choices; no accuracy claim is made for them."""
    return TrackOpts(float(iou), int(max_age), int(min_hits), int(max_tracks), float(hold_grow))


CF_FOLLOW_NONE, CF_FOLLOW_LEARNED, CF_FOLLOW_MOVED, CF_FOLLOW_LOST = 0, 1, 2, 3


class TrackWeakOpts(C.Structure):
    """cf_track_weak_opts: a row is strong when score > birth_score / the match threshold of the weak pass."""
    _fields_ = [("birth_score", C.c_float), ("weak_iou", C.c_float)]


def track_weak_opts(birth_score=0.3, weak_iou=0.5):
    """TrackWeakOpts (the library validates the numbers).  0.5 is ByteTrack's customary value and this project's choice: nobody has
    measured it here, and no accuracy claim is made."""
    return TrackWeakOpts(float(birth_score), float(weak_iou))


class TrackMotionOpts(C.Structure):
    """cf_track_motion_opts: the share of a measured residual the velocity takes / what is left of the velocity after a coasted frame."""
    _fields_ = [("gain", C.c_float), ("damp", C.c_float)]


def track_motion_opts(gain=0.5, damp=1.0):
    """TrackMotionOpts (the library validates the numbers).  0.5 and 1.0 (SORT's coast) are this project's choices: there is no labelled
    video here, nobody has measured them, and no accuracy claim is made."""
    return TrackMotionOpts(float(gain), float(damp))


def track_motion_of(motion):
    """The ``motion=`` argument of ``Tracker`` and the sequence ops: None (or False) -> None, True -> the defaults, a dict with ``gain``
    and / or ``damp`` -> those.  ValueError for anything else and for unknown keys; the library validates the numbers."""
    if motion is None or motion is False:
        return None
    if motion is True:
        return track_motion_opts()
    if not isinstance(motion, dict):
        raise ValueError("motion must be None, True or a dict with gain and / or damp, got %r" % (motion,))
    unknown = sorted(set(motion) - {"gain", "damp"})
    if unknown:
        raise ValueError("motion: unknown keys %s (gain, damp)" % (unknown,))
    return track_motion_opts(**motion)


class FollowOpts(C.Structure):
    """cf_follow_opts: search radius R in cells / the largest SAD of a match that still moves the track."""
    _fields_ = [("search", C.c_int32), ("max_sad", C.c_int32)]


def follow_opts(search=4, max_sad=4096):
    """FollowOpts (the library validates the numbers).  The defaults are this project's choices; no accuracy claim is made for them."""
    return FollowOpts(int(search), int(max_sad))


CF_SCENE_FIRST, CF_SCENE_SAME, CF_SCENE_CUT = 0, 1, 2


class SceneOpts(C.Structure):
    """cf_scene_opts: the per mille of pixels that must change histogram bin / the sum of cell-mean differences, both needed for a cut."""
    _fields_ = [("hist_thresh", C.c_int32), ("grid_thresh", C.c_int32)]


def scene_opts(hist=350, grid=640):
    """SceneOpts (the library validates the numbers).  The defaults are this project's choices: there is no labelled video here, nobody
    has measured them, and no accuracy claim is made for them."""
    return SceneOpts(int(hist), int(grid))


class LookbackOpts(C.Structure):
    """cf_lookback_opts: frames of delay / rows of an entry and of an output image / growth of a back-filled box per frame of distance /
    queued frames that must show a new id before it is back-filled."""
    _fields_ = [("depth", C.c_int32), ("rows", C.c_int32), ("grow", C.c_float), ("confirm", C.c_int32)]


def lookback_opts(depth=8, rows=256, grow=0.05, confirm=1):
    """LookbackOpts (the library validates the numbers).  The defaults are this project's choices: there is no labelled video here, nobody
    has measured them, and no accuracy claim is made for them."""
    return LookbackOpts(int(depth), int(rows), float(grow), int(confirm))


CF_BEST_SIZE, CF_BEST_POSE, CF_BEST_SCORE = 1, 2, 4
_BEST_TERMS = {"size": CF_BEST_SIZE, "pose": CF_BEST_POSE, "score": CF_BEST_SCORE}


class BestShotOpts(C.Structure):
    """cf_bestshot_opts: chip side / table entries per stream / hits a row needs to be offered / the CF_BEST_* weights that take part."""
    _fields_ = [("size", C.c_int32), ("entries", C.c_int32), ("min_hits", C.c_int32), ("terms", C.c_int32)]


def bestshot_opts(size=112, entries=320, min_hits=2, terms=("size", "pose", "score")):
    """BestShotOpts (the library validates the numbers).  ``terms``: an int mask of CF_BEST_*, or names out of size / pose / score.  The
    quality formula and the defaults are this project's choices; no accuracy claim is made for them."""
    if isinstance(terms, (int, np.integer)):
        mask = int(terms)
    else:
        unknown = [t for t in terms if t not in _BEST_TERMS]
        if unknown:
            raise ValueError("terms must be out of %s, got %s" % (sorted(_BEST_TERMS), unknown))
        mask = sum(set(_BEST_TERMS[t] for t in terms))
    return BestShotOpts(int(size), int(entries), int(min_hits), mask)


def tile_rects(rects):
    """(TileRect table, T) of an int array-like [T][4] of (x0, y0, w, h) rows."""
    r = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
    tab = (TileRect * max(len(r), 1))()
    for t, (x0, y0, w, h) in enumerate(r.tolist()):
        tab[t].x0, tab[t].y0, tab[t].w, tab[t].h = x0, y0, w, h
    return tab, len(r)


def frame_format(fmt):
    """The `format` integer of cf_redact_faces: 'bgr' -> CF_FRAME_BGR, otherwise as ``yuv_format``."""
    if isinstance(fmt, str) and fmt.lower() == "bgr":
        return CF_FRAME_BGR
    return yuv_format(fmt)


def frame_planes(frames, fmt, writable=True):
    """Host frames of ``Engine.redact_faces`` / ``ops.redact_faces`` as (PlanesRW table, B, h, w, pitch0, pitch1, arrays to keep alive):
    BGR uint8 [B,h,w,3]; 4:2:0 uint8 [B, h*3//2, w] (OpenCV's dense layout) or a list of such [h*3//2, w] frames; or a list of per-frame
    plane tuples of uint8 2-D arrays (rows of bytes; one common shape and row stride per plane; BGR: one [h, 3w] or [h,w,3] array).  The arrays are written in place,
    so nothing is copied here: a frame that is not writable or whose rows are not contiguous is refused (``writable=False``: the
    caller only reads them -- the tile cutter -- and read-only arrays pass)."""
    f = frame_format(fmt)
    bgr, il = f == CF_FRAME_BGR, f in (CF_YUV_NV12, CF_YUV_NV21)

    def rows_of(a, what):
        a = a if isinstance(a, np.ndarray) else np.asarray(a)
        if a.dtype != np.uint8 or a.ndim < 2 or (writable and not a.flags["WRITEABLE"]):
            raise ValueError("%s must be a writable uint8 array, got %s %s" % (what, a.dtype, a.shape))
        if a.ndim == 3:
            if a.strides[1:] != (a.shape[2], 1):
                raise ValueError("%s: the pixels of a row must be contiguous" % what)
            return a, a.shape[0], a.shape[1] * a.shape[2], a.strides[0]
        if a.ndim != 2 or a.strides[1] != 1:
            raise ValueError("%s: the bytes of a row must be contiguous" % what)
        return a, a.shape[0], a.shape[1], a.strides[0]
    if isinstance(frames, np.ndarray):
        x = frames
        if x.dtype != np.uint8 or not x.flags["C_CONTIGUOUS"] or (writable and not x.flags["WRITEABLE"]):
            raise ValueError("frames must be a writable C-contiguous uint8 array")
        if bgr:
            if x.ndim != 4 or x.shape[3] != 3:
                raise ValueError("BGR frames must be uint8 [B,h,w,3], got %s" % (x.shape,))
            B, h, w = x.shape[:3]
            tab = (PlanesRW * max(B, 1))()
            for b in range(B):
                tab[b].p0 = x.ctypes.data + b * h * w * 3
            return tab, B, h, w, 3 * w, 0, x
        if x.ndim != 3 or (x.shape[1] * 2 // 3) * 3 // 2 != x.shape[1]:
            raise ValueError("4:2:0 frames must be uint8 [B, h*3//2, w] with h even, got %s" % (x.shape,))
        tab, h, w, cp = dense_planes(f, x)
        return tab, x.shape[0], h, w, w, cp, x
    frames = list(frames)
    if not bgr and frames and all(isinstance(t, np.ndarray) and t.ndim == 2 for t in frames):
        # a list of dense [h*3//2, w] frames, as forward_yuv_enqueue takes them
        rows, w = frames[0].shape
        for x in frames:
            if x.dtype != np.uint8 or x.shape != (rows, w) or (rows * 2 // 3) * 3 // 2 != rows or not x.flags["C_CONTIGUOUS"] or (writable and not x.flags["WRITEABLE"]):
                raise ValueError("frames must be writable C-contiguous uint8 [h*3//2, w] arrays of one size, got %s %s" % (x.dtype, x.shape))
        tab, h, w, cp = dense_planes(f, frames)
        return tab, len(frames), h, w, w, cp, frames
    frames = [t if isinstance(t, (tuple, list)) else (t,) for t in frames]
    need = 1 if bgr else 2 if il else 3
    B = len(frames)
    if B == 0:
        raise ValueError("redact_faces needs at least one frame")
    tab = (PlanesRW * B)()
    keep, geo = [], None
    for b, t in enumerate(frames):
        t = [p for p in t if p is not None]
        if len(t) != need:
            raise ValueError("frame %d has %d planes, format %r takes %d" % (b, len(t), fmt, need))
        g = []
        for k, a in enumerate(t):
            a, rows, rowbytes, pitch = rows_of(a, "plane %d of frame %d" % (k, b))
            keep.append(a)
            g.append((rows, rowbytes, pitch))
            setattr(tab[b], "p%d" % k, a.ctypes.data)
        if geo is None:
            geo = g
        elif g != geo:
            raise ValueError("frame %d differs from frame 0 in a plane's shape or row stride" % b)
    h, row0, pitch0 = geo[0]
    if bgr and row0 % 3:
        raise ValueError("a BGR plane has 3w bytes per row, got %d" % row0)
    w = row0 // 3 if bgr else row0
    pitch1 = 0
    if not bgr:
        want = (h // 2, w if il else w // 2)
        for g in geo[1:]:
            if (g[0], g[1]) != want or g[2] != geo[1][2]:
                raise ValueError("chroma planes must be [%d, %d] with one row stride, got %s" % (want + (geo[1:],)))
        pitch1 = geo[1][2]
    return tab, B, h, w, pitch0, pitch1, keep


def dense_planes(f, frames):
    """(PlanesRW table, h, w, chroma pitch) of dense 4:2:0 host frames the caller has validated: a C-contiguous uint8 [B, h*3//2, w] array
    or a list of C-contiguous [h*3//2, w] arrays."""
    rows, w = frames.shape[1:] if isinstance(frames, np.ndarray) else frames[0].shape
    h = rows * 2 // 3
    offs, cp = yuv_dense_geometry(f, h, w)
    bases = [frames.ctypes.data + b * rows * w for b in range(len(frames))] if isinstance(frames, np.ndarray) else [a.ctypes.data for a in frames]
    tab = (PlanesRW * max(len(bases), 1))()
    for b, base in enumerate(bases):
        tab[b].p0, tab[b].p1, tab[b].p2 = base, base + offs[1], (base + offs[2]) if offs[2] is not None else None
    return tab, h, w, cp


def host_frame_args(frames, fmt, writable=True):
    """The frame arguments of cf_redact_faces / cf_blur_faces / cf_align_faces_frame / cf_forward_tiles for host ``frames`` as ``frame_planes``
    takes them: ((format, table, in_on_device = 0, B, h, w, pitch0, pitch1), the arrays to keep alive for the call)."""
    tab, B, h, w, pitch0, pitch1, keep = frame_planes(frames, fmt, writable)
    return (frame_format(fmt), tab, 0, B, h, w, pitch0, pitch1), keep


def device_frame_args(who, plane_ptrs, fmt, B, h, w, pitch0, pitch1):
    """The same arguments for B tuples of device addresses (in_on_device = 1); ``who`` names the caller in the refusal."""
    if int(B) != len(plane_ptrs):
        raise ValueError("%s: %d plane tuples for B=%d" % (who, len(plane_ptrs), B))
    return frame_format(fmt), device_planes(plane_ptrs), 1, int(B), int(h), int(w), int(pitch0), int(pitch1)


def device_planes(plane_ptrs):
    """PlanesRW table of B tuples (p0, p1, p2) of device addresses (missing planes None); cf_yuv_planes has the same layout."""
    tab = (PlanesRW * max(len(plane_ptrs), 1))()
    for b, t in enumerate(plane_ptrs):
        t = (tuple(t) if isinstance(t, (tuple, list)) else (t,)) + (None, None)
        tab[b].p0, tab[b].p1, tab[b].p2 = (int(v) if v else None for v in t[:3])
    return tab


def device_input_planes(who, plane_ptrs, f, h, w, pitch0=None, pitch1=None):
    """The ``on_device=True`` form of the forwards that read frames of format code ``f`` in place: (table, B, h, w, pitch0, pitch1) of B
    tuples of device addresses, the pitches dense rows by default; ``who`` names the caller in the refusal."""
    if h is None or w is None:
        raise ValueError("%s(on_device=True) needs h and w" % who)
    h, w, bgr = int(h), int(w), f == CF_FRAME_BGR
    return (device_planes(plane_ptrs), len(plane_ptrs), h, w, (3 * w if bgr else w) if pitch0 is None else int(pitch0),
            (0 if bgr else yuv_dense_geometry(f, h, w)[1]) if pitch1 is None else int(pitch1))


def box_rows(boxes, counts, B):
    """(boxes float32 [N,4], counts int32 [B]) of the packed box rows of B images, N = the sum of the counts."""
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
    if counts.shape[0] != B or (counts < 0).any() or int(counts.sum()) != boxes.shape[0]:
        raise ValueError("counts must be [B] non-negative and sum to the number of box rows")
    return boxes, counts


def frames_pitch4(tab, fmt, B, h, w, pitch0, pitch1):
    """The host frames of a ``frame_planes`` table with every pitch a multiple of 4: the table as it is when they are, else a new table
    over padded copies (zero padding).  Returns (table, pitch0, pitch1, arrays to keep alive)."""
    f = frame_format(fmt)
    bgr, il = f == CF_FRAME_BGR, f in (CF_YUV_NV12, CF_YUV_NV21)
    if pitch0 % 4 == 0 and (bgr or pitch1 % 4 == 0):
        return tab, pitch0, pitch1, None
    geo = [(h, 3 * w if bgr else w, pitch0)] + ([] if bgr else [(h // 2, w if il else w // 2, pitch1)] * (1 if il else 2))
    out, keep = (PlanesRW * max(B, 1))(), []
    for b in range(B):
        for k, (rows, rowbytes, pitch) in enumerate(geo):
            src = getattr(tab[b], "p%d" % k)
            n = (rows - 1) * pitch + rowbytes
            flat = np.frombuffer((C.c_uint8 * n).from_address(src), np.uint8)
            dst = np.zeros((rows, (rowbytes + 3) & ~3), np.uint8)
            dst[:, :rowbytes] = np.lib.stride_tricks.as_strided(flat, (rows, rowbytes), (pitch, 1))
            keep.append(dst)
            setattr(out[b], "p%d" % k, dst.ctypes.data)
    return out, (geo[0][1] + 3) & ~3, 0 if bgr else (geo[1][1] + 3) & ~3, keep


def yuv_format(fmt):
    """CF_YUV_* code of a format name ('nv12', 'nv21', 'i420' / 'yuv420p', 'yv12'); integer codes pass through unchanged (the
    library validates them)."""
    if isinstance(fmt, str):
        if fmt.lower() not in YUV_FORMATS:
            raise ValueError("unknown YUV format %r (one of %s)" % (fmt, sorted(YUV_FORMATS)))
        return YUV_FORMATS[fmt.lower()]
    return int(fmt)


def yuv_dense_geometry(fmt, h, w):
    """(plane offsets (y, c0, c1 or None), c_pitch) of one frame in OpenCV's single-buffer [h*3/2, w] layout."""
    if fmt in (CF_YUV_NV12, CF_YUV_NV21):
        return (0, h * w, None), w
    return (0, h * w, h * w + (h // 2) * (w // 2)), w // 2


def build(force=False, verbose=False):
    """Compile the HIP sources for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1))]
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, capture_output=not verbose)
    res = subprocess.run(args, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libcenterface_hip.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])
    if verbose:
        print(res.stdout[-2000:])
    return LIB_PATH


_lib = None


def lib():
    """The loaded library; raises (never falls back) if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback path)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.cf_strerror.restype = C.c_char_p
        L.cf_last_error.restype = C.c_char_p
        L.cf_last_error.argtypes = [C.c_void_p]
        L.cf_op_last_error.restype = C.c_char_p
        L.cf_op_last_kernel.restype = C.c_char_p
        L.cf_op_last_kernel.argtypes = []
        L.cf_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
        L.cf_destroy.argtypes = [C.c_void_p]
        L.cf_load_weights.argtypes = [C.c_void_p, C.POINTER(TensorDesc), C.c_int]
        L.cf_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        if hasattr(L, "cf_forward_lanes"):              # experiments build only (csrc/cf_experiments.h)
            L.cf_forward_lanes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
            L.cf_forward_lanes_flush.argtypes = [C.c_void_p]
        L.cf_forward_resized.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.cf_forward_yuv.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_int] * 5      # (a YuvPlanes or a PlanesRW table: one layout)
        L.cf_op_yuv_to_bgr.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5
        L.cf_align_faces.argtypes = [C.c_void_p, C.POINTER(AlignOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.cf_op_align_faces.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(AlignOpts), C.c_void_p, C.c_void_p]
        L.cf_align_faces_frame.argtypes = [C.c_void_p, C.POINTER(AlignOpts), C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3 + [C.c_int] * 2
        L.cf_op_align_frame.argtypes = [C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.POINTER(AlignOpts), C.c_void_p, C.c_void_p]
        L.cf_redact_faces.argtypes = [C.c_void_p, C.POINTER(RedactOpts), C.c_int, C.POINTER(PlanesRW)] + [C.c_int] * 6
        L.cf_op_redact.argtypes = [C.c_int, C.POINTER(RedactOpts), C.c_int, C.POINTER(PlanesRW)] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.cf_blur_faces.argtypes = [C.c_void_p, C.POINTER(BlurOpts), C.c_int, C.POINTER(PlanesRW)] + [C.c_int] * 6
        L.cf_op_blur.argtypes = [C.c_int, C.POINTER(BlurOpts), C.c_int, C.POINTER(PlanesRW)] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.cf_draw_faces.argtypes = [C.c_void_p, C.POINTER(DrawOpts), C.c_int, C.POINTER(PlanesRW)] + [C.c_int] * 6
        L.cf_op_draw.argtypes = [C.c_int, C.POINTER(DrawOpts), C.c_int, C.POINTER(PlanesRW)] + [C.c_int] * 5 + [C.c_void_p] * 5 + [C.c_int, C.c_int]
        L.cf_draw_layout.argtypes = [C.POINTER(DrawOpts), C.c_void_p, C.c_float, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
        L.cf_tile_grid.argtypes = [C.c_int] * 6 + [C.POINTER(TileRect), C.c_int, C.POINTER(C.c_int)]
        L.cf_forward_tiles.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.POINTER(TileRect), C.c_int]
        L.cf_merge_tiles.argtypes = [C.c_void_p, C.POINTER(MergeOpts), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.cf_op_cut_tiles.argtypes = [C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.POINTER(TileRect)] + [C.c_int] * 3 + [C.c_void_p]
        L.cf_op_merge_tiles.argtypes = [C.c_int, C.POINTER(MergeOpts), C.POINTER(TileRect)] + [C.c_int] * 6 + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p] * 4
        L.cf_fit_geometry.argtypes = [C.POINTER(FitOpts)] + [C.c_int] * 4 + [C.POINTER(FitGeom)]
        L.cf_forward_fit.argtypes = [C.c_void_p, C.POINTER(FitOpts), C.c_int, C.c_void_p] + [C.c_int] * 6
        L.cf_unfit_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.cf_op_fit.argtypes = [C.c_int, C.POINTER(FitOpts), C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]
        L.cf_op_unfit.argtypes = [C.c_int, C.POINTER(FitOpts)] + [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p] * 4
        L.cf_view_layout.argtypes = [C.POINTER(ViewOpts)] + [C.c_int] * 4 + [C.POINTER(View), C.c_int, C.POINTER(C.c_int)]
        L.cf_forward_views.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.POINTER(View), C.c_int, C.c_void_p]
        L.cf_merge_views.argtypes = [C.c_void_p, C.POINTER(MergeOpts), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.cf_op_views.argtypes = [C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.POINTER(View), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.cf_op_merge_views.argtypes = [C.c_int, C.POINTER(MergeOpts), C.POINTER(View)] + [C.c_int] * 6 + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p] * 4
        L.cf_pack_views.argtypes = [C.POINTER(View)] + [C.c_int] * 5 + [C.POINTER(Place), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.cf_forward_packed.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.POINTER(Place), C.c_int, C.c_int, C.c_void_p]
        L.cf_merge_packed.argtypes = [C.c_void_p, C.POINTER(MergeOpts), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.cf_op_packed.argtypes = [C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.POINTER(Place), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.cf_op_merge_packed.argtypes = [C.c_int, C.POINTER(MergeOpts), C.POINTER(Place)] + [C.c_int] * 7 + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p] * 4
        L.cf_forward_packed_rot.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.POINTER(Place), C.c_int, C.c_int, C.c_void_p]
        L.cf_op_packed_rot.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.POINTER(Place), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.cf_op_merge_packed_rot.argtypes = [C.c_int, C.c_int, C.POINTER(MergeOpts), C.POINTER(Place)] + [C.c_int] * 7 + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p] * 4
        L.cf_rot_geometry.argtypes = [C.POINTER(RotOpts)] + [C.c_int] * 4 + [C.POINTER(FitGeom)]
        L.cf_forward_rot.argtypes = [C.c_void_p, C.POINTER(RotOpts), C.c_int, C.c_void_p] + [C.c_int] * 6
        L.cf_op_rot.argtypes = [C.c_int, C.POINTER(RotOpts), C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]
        L.cf_op_unrot.argtypes = [C.c_int, C.POINTER(RotOpts)] + [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p] * 4
        L.cf_set_flip_test.argtypes = [C.c_void_p, C.c_int]
        L.cf_op_mirror.argtypes = [C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p]
        L.cf_op_flip_heads.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 2
        L.cf_track_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(TrackOpts), C.POINTER(C.c_void_p)]
        L.cf_track_destroy.argtypes = [C.c_void_p]
        L.cf_track_reset.argtypes = [C.c_void_p, C.c_int]
        L.cf_track_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
        L.cf_op_track.argtypes = [C.c_int, C.POINTER(TrackOpts)] + [C.c_int] * 3 + [C.c_void_p] * 9
        L.cf_track_create_weak.argtypes = [C.c_void_p, C.c_int, C.POINTER(TrackOpts), C.POINTER(TrackWeakOpts), C.POINTER(C.c_void_p)]
        L.cf_op_track_weak.argtypes = [C.c_int, C.POINTER(TrackOpts), C.POINTER(TrackWeakOpts)] + [C.c_int] * 3 + [C.c_void_p] * 9
        L.cf_track_create_ex.argtypes = [C.c_void_p, C.c_int, C.POINTER(TrackOpts), C.POINTER(TrackWeakOpts), C.POINTER(TrackMotionOpts), C.POINTER(C.c_void_p)]
        L.cf_op_track_ex.argtypes = [C.c_int, C.POINTER(TrackOpts), C.POINTER(TrackWeakOpts), C.POINTER(TrackMotionOpts)] + [C.c_int] * 3 + [C.c_void_p] * 10
        L.cf_op_follow_ex.argtypes = [C.c_int, C.POINTER(TrackOpts), C.POINTER(TrackWeakOpts), C.POINTER(TrackMotionOpts), C.POINTER(FollowOpts)] + \
            [C.c_int] * 3 + [C.c_void_p] * 5 + [C.c_int, C.POINTER(PlanesRW)] + [C.c_int] * 7 + [C.c_void_p] * 6
        L.cf_track_follow.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(FollowOpts), C.c_int, C.POINTER(PlanesRW)] + [C.c_int] * 5 + \
            [C.c_void_p] * 5 + [C.c_int]
        L.cf_op_follow.argtypes = [C.c_int, C.POINTER(TrackOpts), C.POINTER(FollowOpts)] + [C.c_int] * 3 + [C.c_void_p] * 5 + [C.c_int, C.POINTER(PlanesRW)] + \
            [C.c_int] * 7 + [C.c_void_p] * 6
        L.cf_scene_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(SceneOpts), C.POINTER(C.c_void_p)]
        L.cf_scene_destroy.argtypes = [C.c_void_p]
        L.cf_scene_forget.argtypes = [C.c_void_p, C.c_int]
        L.cf_scene_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(PlanesRW)] + [C.c_int] * 5 + [C.c_void_p, C.c_int]
        L.cf_op_scene.argtypes = [C.c_int, C.POINTER(SceneOpts), C.c_int, C.c_int, C.c_int, C.POINTER(PlanesRW)] + [C.c_int] * 4 + [C.c_void_p] * 2
        L.cf_lookback_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(LookbackOpts), C.POINTER(C.c_void_p)]
        L.cf_lookback_destroy.argtypes = [C.c_void_p]
        L.cf_lookback_forget.argtypes = [C.c_void_p, C.c_int]
        L.cf_lookback_step.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
        L.cf_op_lookback.argtypes = [C.c_int, C.POINTER(LookbackOpts)] + [C.c_int] * 3 + [C.c_void_p] * 11
        L.cf_lookback_trace_enable.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(FollowOpts), C.c_int, C.c_int]
        L.cf_lookback_step_frames.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p, C.c_int] + [C.c_int, C.POINTER(PlanesRW)] + [C.c_int] * 5 + \
            [C.c_void_p] * 6 + [C.c_int]
        L.cf_op_lookback_trace.argtypes = [C.c_int, C.POINTER(LookbackOpts), C.POINTER(FollowOpts)] + [C.c_int] * 3 + [C.c_void_p] * 6 + \
            [C.c_int, C.POINTER(PlanesRW)] + [C.c_int] * 7 + [C.c_void_p] * 6
        L.cf_bestshot_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(BestShotOpts), C.POINTER(C.c_void_p)]
        L.cf_bestshot_destroy.argtypes = [C.c_void_p]
        L.cf_bestshot_offer.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_int]
        L.cf_bestshot_collect.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 8 + [C.c_int]
        L.cf_op_chip_quality.argtypes = [C.c_int, C.POINTER(BestShotOpts)] + [C.c_void_p] * 4 + [C.c_int, C.c_double, C.c_double] + [C.c_void_p] * 2
        L.cf_op_bestshot.argtypes = [C.c_int, C.POINTER(BestShotOpts)] + [C.c_int] * 3 + [C.c_void_p] * 8 + [C.c_int, C.c_double, C.c_double] + [C.c_void_p] * 10
        L.cf_get_resized_input.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.cf_get_heads.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        L.cf_decode_topk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.cf_decode_topk_post.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.cf_affine_from_center_scale.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p]
        L.cf_op_ctdet_post_process.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.cf_decode_threshold_ex.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cf_decode_threshold_sized.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cf_decode_threshold_enqueue.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        L.cf_op_decode_threshold_ex.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cf_decode_threshold.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cf_detect_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.cf_synchronize.argtypes = [C.c_void_p]
        L.cf_event_record.argtypes = [C.c_void_p, C.c_int]
        L.cf_event_elapsed_ms.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.cf_profile_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(OpTime), C.c_int, C.POINTER(C.c_int)]
        L.cf_plan_size.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.cf_plan_op.argtypes = [C.c_void_p, C.c_int, C.POINTER(OpInfo)]
        L.cf_forward_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.cf_ctdet_loss.argtypes = [C.c_void_p] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p, C.c_void_p]
        L.cf_op_ctdet_loss.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 8 + [C.c_int, C.c_void_p, C.c_void_p]
        L.cf_op_encode_targets.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 8
        L.cf_comm_unique_id.argtypes = [C.c_void_p, C.c_int]
        L.cf_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.cf_comm_destroy.argtypes = [C.c_void_p]
        L.cf_comm_create_all.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
        L.cf_comm_create_loopback.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.cf_comm_loopback_rank.argtypes = [C.c_void_p, C.c_int]
        L.cf_comm_abort.argtypes = [C.c_void_p]
        L.cf_comm_query.argtypes = [C.c_void_p]
        L.cf_comm_synchronize.argtypes = [C.c_void_p]
        L.cf_comm_last_error.argtypes = [C.c_void_p]
        L.cf_comm_last_error.restype = C.c_char_p
        L.cf_comm_debug.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.cf_comm_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.cf_comm_stream.argtypes = [C.c_void_p]
        L.cf_comm_stream.restype = C.c_void_p
        L.cf_gather_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.cf_get_streams.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.cf_graph_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.cf_streams_share_queue.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.cf_streams_share_queue_ex.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.cf_spread_streams.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.cf_reroll_streams.argtypes = [C.c_void_p]
        L.cf_host_alloc.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        L.cf_host_free.argtypes = [C.c_void_p, C.c_void_p]
        L.cf_pinned_alloc.argtypes = [C.c_uint64, C.POINTER(C.c_void_p)]
        L.cf_pinned_free.argtypes = [C.c_void_p]
        L.cf_host_register.argtypes = [C.c_void_p, C.c_uint64]
        L.cf_host_unregister.argtypes = [C.c_void_p]
        L.cf_forward_images.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]
        L.cf_upload_images.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]
        L.cf_forward_uploaded.argtypes = [C.c_void_p]
        L.cf_set_rescale.argtypes = [C.c_void_p, C.c_float, C.c_float]
        L.cf_device_alloc.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        L.cf_device_free.argtypes = [C.c_void_p, C.c_void_p]
        L.cf_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.cf_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        fp, vp, i = C.c_void_p, C.c_void_p, C.c_int
        L.cf_op_dwconv.argtypes = [i, i, fp, fp, fp, fp] + [i] * 9
        L.cf_op_pwconv.argtypes = [i, i, fp, fp, fp, fp, fp] + [i] * 6
        L.cf_op_pwconv_ex.argtypes = [i, i, fp, fp, fp, fp, fp] + [i] * 7
        L.cf_op_stem.argtypes = [i, i, vp, i, fp, fp, i, i, i]
        L.cf_op_shufflev2.argtypes = [i, i, fp, fp] + [i] * 8 + [fp] * 10
        L.cf_op_mbconv.argtypes = [i, i, fp, fp, fp, fp, fp] + [i] * 8
        L.cf_op_expand_dw.argtypes = [i, i, fp, fp, fp, fp] + [i] * 7
        L.cf_op_dw_pick.argtypes = [i] * 11 + [C.POINTER(C.c_int), C.c_char_p, i]
        L.cf_op_mbconv_pick.argtypes = [i] * 6 + [C.POINTER(C.c_int)]
        L.cf_op_expand_dw_pick.argtypes = [i] * 5 + [C.POINTER(C.c_int)]
        L.cf_op_idaup.argtypes = [i, i, fp, fp, fp, fp, fp, fp, C.c_float, fp] + [i] * 5
        L.cf_op_heads.argtypes = [i, i, fp, fp, fp, fp, fp, fp, i, i, i, i]
        L.cf_op_ctdet_decode.argtypes = [i, fp, fp, fp, fp, i, i, i, i, fp, fp, vp]
        L.cf_op_decode_threshold.argtypes = [i, fp, fp, fp, i, i, i, i, i, C.c_float, C.c_float, i, fp, fp, vp]
        L.cf_op_nms.argtypes = [i, fp, fp, i, C.c_float, vp, vp]
        L.cf_op_box_match.argtypes = [i, i, fp, i, vp, fp, i, vp, C.c_float, vp, vp]
        _lib = L
    return _lib


def ptr(a):
    """Host pointer of a C-contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def vp(a):
    """An optional device address as the ABI takes it: c_void_p, or None for 0 / None."""
    return C.c_void_p(int(a)) if a else None


def f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


class CenterFaceError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("libcenterface_hip: %s (code %d)" % (text, code))
        self.code = code


class CenterFaceValueError(CenterFaceError, ValueError):
    """CF_EINVAL: an argument the library refuses (a ValueError, and a CenterFaceError like every other refusal)."""


def check(code, ctx=None, op=False):
    if code == CF_OK:
        return
    L = lib()
    detail = (L.cf_op_last_error() if op else L.cf_last_error(ctx)) or b""
    text = L.cf_strerror(code).decode()
    if detail:
        text += ": " + detail.decode(errors="replace")
    if code == -1:
        raise CenterFaceValueError(code, text)
    raise CenterFaceError(code, text)
