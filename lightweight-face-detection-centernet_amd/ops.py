"""numpy-in / numpy-out wrappers of the per-op C-ABI entry points (cf_op_*).  Signatures mirror the
torch ops of the reference they replace (NCHW float32 arrays); each call runs the production HIP
kernel on the GPU.  Used by the parity tests; no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import f32, ptr

_DT = {"fp32": 0, "bf16": 1, "fp32_split": 2, "bf16x3": 2}


def conv_dw(x, w, k, stride, pad=None, act="swish", bias=None, dtype="fp32", device=0):
    """ZeroPad2d -> depthwise Conv2d -> act (model/centernet.py:58-70; blocks.py:26-29).
    ``pad`` = (lo, hi) applied to both axes; default is the reference's TF-SAME rule."""
    x, w = f32(x), f32(w)
    B, Cc, H, W = x.shape
    if pad is None:
        p = max(k - stride, 0)
        pad = (p // 2, p - p // 2)
    Ho = (H + pad[0] + pad[1] - k) // stride + 1
    Wo = (W + pad[0] + pad[1] - k) // stride + 1
    y = np.empty((B, Cc, max(Ho, 0), max(Wo, 0)), np.float32)      # (no output: the library refuses the call)
    _lib.check(_lib.lib().cf_op_dwconv(device, _DT[dtype], ptr(x), ptr(w), ptr(f32(bias)), ptr(y), B, Cc, H, W,
                                       k, stride, pad[0], pad[1], {"none": 0, "swish": 1}[act]), op=True)
    return y


_DW_PICK = ("ok", "strip", "k", "s", "TH", "TW", "Cc", "nchunk", "cpp", "threads", "lds_bytes", "ntx", "nty", "workgroups", "Ho", "Wo")


def dw_pick(C_, H, W, k, stride, pad=None, dtype="fp32", B=1, act="swish", bias=False):
    """What ``conv_dw`` would launch for a shape, from the host half of the launcher alone (cf_op_dw_pick: no GPU needed):
    {ok, tag (the symbol ``last_kernel()`` reports after the launch), strip, k, s, TH, TW, Cc, nchunk, cpp, threads, lds_bytes,
    ntx, nty, workgroups, Ho, Wo}; ok = False (tag None, zeros) for a shape ``conv_dw`` refuses.  ``pad`` as in ``conv_dw``."""
    if pad is None:
        p = max(k - stride, 0)
        pad = (p // 2, p - p // 2)
    out, tag = (C.c_int * 16)(), C.create_string_buffer(160)
    _lib.check(_lib.lib().cf_op_dw_pick(_DT[dtype], int(B), int(C_), int(H), int(W), int(k), int(stride), int(pad[0]), int(pad[1]),
                                        {"none": 0, "swish": 1}[act], 1 if bias else 0, out, tag, 160), op=True)
    d = dict(zip(_DW_PICK, (int(v) for v in out)))
    d["ok"] = bool(d["ok"])
    d["tag"] = tag.value.decode() if d["ok"] else None
    return d


def last_kernel():
    """Demangled symbol of the kernel the last op call on this thread selected (cf_op_last_kernel)."""
    return (_lib.lib().cf_op_last_kernel() or b"").decode()


def conv_pw(x, w, act="none", bias=None, residual=None, dtype="fp32", device=0, layout=0):
    """1x1 Conv2d [+bias] [+act] [+residual] (model/centernet.py:109-110,117-118,134-137).  ``layout``: bit 0 / 1 / 2 = the
    kernel addresses x / y / the residual in pixel-block order (cf_op_pwconv_ex; arrays here stay NCHW either way)."""
    x = f32(x)
    w = f32(np.asarray(w).reshape(w.shape[0], -1))
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    y = np.empty((B, Cout, H, W), np.float32)
    _lib.check(_lib.lib().cf_op_pwconv_ex(device, _DT[dtype], ptr(x), ptr(w), ptr(f32(bias)), ptr(f32(residual)),
                                          ptr(y), B, Cin, Cout, H, W, {"none": 0, "swish": 1, "relu": 2}[act], int(layout)), op=True)
    return y


def mbconv(x, w_exp, w_dw, w_proj, k, stride, dtype="fp32", device=0):
    """MBConvBlock.forward (model/centernet.py:89-140, se=False) as the single fused kernel."""
    x = f32(x)
    B, Cin, H, W = x.shape
    w_exp = f32(np.asarray(w_exp).reshape(w_exp.shape[0], -1))
    hid = w_exp.shape[0]
    w_dw = f32(np.asarray(w_dw).reshape(hid, k * k))
    w_proj = f32(np.asarray(w_proj).reshape(w_proj.shape[0], -1))
    Cout = w_proj.shape[0]
    p = max(k - stride, 0)
    Ho, Wo = (H + p - k) // stride + 1, (W + p - k) // stride + 1
    y = np.empty((B, Cout, Ho, Wo), np.float32)
    _lib.check(_lib.lib().cf_op_mbconv(device, _DT[dtype], ptr(x), ptr(w_exp), ptr(w_dw), ptr(w_proj), ptr(y),
                                       B, Cin, hid, Cout, H, W, k, stride), op=True)
    return y


def expand_dw(x, w_exp, w_dw, k, stride, dtype="bf16", device=0):
    """Expand 1x1 + Swish -> depthwise k x k + Swish of an MBConv block (model/centernet.py:109-114) as the
    single kernel the engine uses for the wide late blocks (bf16 storage only)."""
    x = f32(x)
    B, Cin, H, W = x.shape
    w_exp = f32(np.asarray(w_exp).reshape(w_exp.shape[0], -1))
    hid = w_exp.shape[0]
    w_dw = f32(np.asarray(w_dw).reshape(hid, k * k))
    p = max(k - stride, 0)
    Ho, Wo = (H + p - k) // stride + 1, (W + p - k) // stride + 1
    y = np.empty((B, hid, Ho, Wo), np.float32)
    _lib.check(_lib.lib().cf_op_expand_dw(device, _DT[dtype], ptr(x), ptr(w_exp), ptr(w_dw), ptr(y),
                                          B, Cin, hid, H, W, k, stride), op=True)
    return y


_PICK = ("ok", "kind", "HC", "nq", "JX", "NBO", "HALF", "KG")
MB_KINDS = {0: "MB_TILE", 1: "MB_PX", 2: "XD_PX", 4: "XD_MX", 5: "MB_MX", 6: "MB_MX2", 7: "MB_F32", 8: "XD_F32", 9: "MB_SP"}


def _pick(code, out):
    _lib.check(code, op=True)
    d = dict(zip(_PICK, (int(v) for v in out)))
    d["ok"] = bool(d["ok"])
    d["kind"] = MB_KINDS.get(d["kind"], d["kind"]) if d["ok"] else None
    return d


def mbconv_pick(Cin, hid, Cout, k, stride, dtype="fp32"):
    """What ``mbconv`` would run for a block shape, from the geometry function alone (cf_op_mbconv_pick: no GPU needed):
    {ok, kind (family name), HC, nq, JX, NBO, HALF, KG}; ok = False for a shape ``mbconv`` refuses."""
    out = (C.c_int * 8)()
    return _pick(_lib.lib().cf_op_mbconv_pick(_DT[dtype], Cin, hid, Cout, k, stride, out), out)


def expand_dw_pick(Cin, hid, k, stride, dtype="bf16"):
    """The same for ``expand_dw`` (cf_op_expand_dw_pick)."""
    out = (C.c_int * 8)()
    return _pick(_lib.lib().cf_op_expand_dw_pick(_DT[dtype], Cin, hid, k, stride, out), out)


def stem(x, w, dtype="fp32", device=0):
    """first_conv (model/centernet.py:224): x uint8 [B,H,W,3] BGR (normalisation fused) or float32 [B,3,H,W]."""
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint8:
        B, H, W, _ = x.shape
        fmt = _lib.CF_IN_U8_HWC_BGR
    else:
        x = f32(x)
        B, _, H, W = x.shape
        fmt = _lib.CF_IN_F32_NCHW
    y = np.empty((B, 32, H // 2, W // 2), np.float32)
    _lib.check(_lib.lib().cf_op_stem(device, _DT[dtype], ptr(x), fmt, ptr(f32(w)), ptr(y), B, H, W), op=True)
    return y


def _bn4(sd, prefix):
    return f32(np.stack([sd[prefix + ".weight"], sd[prefix + ".bias"], sd[prefix + ".running_mean"],
                         sd[prefix + ".running_var"]]))


def idaup(lo, skip, sd, prefix, eps=1e-3, dtype="fp32", device=0):
    """IDAUp.forward (model/centernet.py:200-204) from a state_dict slice with raw BN parameters."""
    lo, skip = f32(lo), f32(skip)
    B, Cc, h, w = lo.shape
    Cs = skip.shape[1]
    y = np.empty((B, Cc, 2 * h, 2 * w), np.float32)
    w_up = f32(sd[prefix + ".up.weight"])
    w_cv = f32(np.asarray(sd[prefix + ".conv.0.weight"]).reshape(Cc, Cs))
    _lib.check(_lib.lib().cf_op_idaup(device, _DT[dtype], ptr(lo), ptr(skip), ptr(w_up), ptr(_bn4(sd, prefix + ".bn_up")),
                                      ptr(w_cv), ptr(_bn4(sd, prefix + ".conv.1")), float(eps), ptr(y),
                                      B, Cc, Cs, h, w), op=True)
    return y


def heads(x, sd, collapse=False, dtype="fp32", device=0):
    """The four heads (model/centernet.py:247-261) -> dict hm (raw), wh, lm, reg (NCHW)."""
    x = f32(x)
    B, _, h, w = x.shape
    names = ("hm", "wh", "lm", "reg")
    w0 = f32(np.stack([sd[n + ".0.weight"] for n in names]))
    b0 = f32(np.stack([sd[n + ".0.bias"] for n in names]))
    w1 = f32(np.concatenate([np.asarray(sd[n + ".1.weight"]).reshape(-1, 24) for n in names]))
    b1 = f32(np.concatenate([np.asarray(sd[n + ".1.bias"]) for n in names]))
    out = np.empty((B, 15, h, w), np.float32)
    _lib.check(_lib.lib().cf_op_heads(device, _DT[dtype], ptr(x), ptr(w0), ptr(b0), ptr(w1), ptr(b1), ptr(out),
                                      B, h, w, 1 if collapse else 0), op=True)
    return {"hm": out[:, 0:1], "wh": out[:, 1:3], "lm": out[:, 3:13], "reg": out[:, 13:15]}


def shuffle_v2_block(x, sd, inp, oup, mid, ksize, stride, prefix="", dtype="fp32", device=0):
    """ShuffleV2Block(inp, oup, mid, ksize=, stride=).forward in eval mode (model/blocks.py:4-62) from a
    state_dict slice with the reference's key names (branch_main.0/1/3/4/5/6, branch_proj.0/1/2/3): ONE C-ABI call;
    BN fold, channel shuffle and concat all happen behind it."""
    x = f32(x)
    B, _, H, W = x.shape
    pad = ksize // 2
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    y = np.empty((B, oup, Ho, Wo), np.float32)

    def w(key):
        return f32(np.asarray(sd[prefix + key + ".weight"]))
    args = [w("branch_main.0"), _bn4(sd, prefix + "branch_main.1"), w("branch_main.3"), _bn4(sd, prefix + "branch_main.4"),
            w("branch_main.5"), _bn4(sd, prefix + "branch_main.6")]
    if stride == 2:
        args += [w("branch_proj.0"), _bn4(sd, prefix + "branch_proj.1"), w("branch_proj.2"), _bn4(sd, prefix + "branch_proj.3")]
    else:
        args += [None, None, None, None]
    _lib.check(_lib.lib().cf_op_shufflev2(device, _DT[dtype], ptr(x), ptr(y), B, int(inp), int(oup), int(mid), H, W,
                                          int(ksize), int(stride), *[ptr(a) for a in args]), op=True)
    return y


def yuv_to_bgr(frames, fmt="nv12", size=None, device=0):
    """cv2.cvtColor(frame, cv2.COLOR_YUV2BGR_<fmt>) on the device (``cf_op_yuv_to_bgr``), followed by cv2.resize to ``size`` = (H, W)
    when given and different: frames uint8 [B, h*3//2, w] or one [h*3//2, w] frame (OpenCV's single-buffer 4:2:0 layout);
    fmt 'nv12', 'nv21', 'i420' ('yuv420p') or 'yv12'.  Returns uint8 [B, H, W, 3] (or [H, W, 3] for one frame)."""
    x = np.ascontiguousarray(frames, dtype=np.uint8)
    one = x.ndim == 2
    if one:
        x = x[None]
    if x.ndim != 3:
        raise ValueError("frames must be uint8 [B, h*3//2, w] or [h*3//2, w], got %s" % (x.shape,))
    B, rows, w = x.shape
    h = rows * 2 // 3
    if h * 3 // 2 != rows:
        raise ValueError("a 4:2:0 frame has h*3//2 rows for an even h; got %d rows" % rows)
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    out = np.empty((B, H, W, 3), np.uint8)
    _lib.check(_lib.lib().cf_op_yuv_to_bgr(device, _lib.yuv_format(fmt), ptr(x), ptr(out), B, h, w, H, W), op=True)
    return out[0] if one else out


def align_faces(imgs, lms, counts, size=112, template=None, out="u8", rgb=False, mean=0.0, scale=1.0, device=0):
    """Aligned face chips (``cf_op_align_faces``): imgs uint8 [B,h,w,3] BGR, lms [N,10] landmark rows (x0,y0,...,x4,y4 in image pixels),
    image after image, counts [B] (N = their sum).  Every face is warped onto ``template`` ([5][2] chip points; default the ArcFace
    112 x 112 points times size / 112) by the least-squares similarity of its landmarks.  Returns (chips, matrices): chips uint8
    [N,size,size,3] BGR (``out='u8'``) or float32 [N,3,size,size] = ``(u8 - mean) * scale`` (``out='f32'``; RGB planes with ``rgb``),
    matrices float64 [N,6] = the row-major 2x3 chip -> image maps (zero for faces that cannot be aligned)."""
    x = np.ascontiguousarray(imgs, dtype=np.uint8)
    if x.ndim != 4 or x.shape[3] != 3:
        raise ValueError("images must be uint8 [B,h,w,3], got %s" % (x.shape,))
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    lms = np.ascontiguousarray(lms, dtype=np.float32).reshape(-1, 10)
    if counts.shape[0] != x.shape[0] or (counts < 0).any() or int(counts.sum()) != lms.shape[0]:
        raise ValueError("counts must be [B] non-negative and sum to the number of landmark rows")
    o, tm, shape, dtype = _lib.align_opts(size, out, rgb, mean, scale, template)
    N = lms.shape[0]
    chips = np.zeros((N,) + shape, dtype)
    mats = np.zeros((N, 6), np.float64)
    _lib.check(_lib.lib().cf_op_align_faces(device, ptr(x), x.shape[0], x.shape[1], x.shape[2], ptr(lms), ptr(counts), C.byref(o),
                                            ptr(chips), ptr(mats)), op=True)
    return chips, mats


def align_frame(frames, lms, counts, fmt="bgr", size=112, template=None, out="u8", rgb=False, mean=0.0, scale=1.0, max_per_image=0, device=0):
    """Aligned face chips cut from full-resolution frames (``cf_op_align_frame``): ``frames`` as ``cut_tiles`` takes them (BGR uint8
    [B,h,w,3], dense 4:2:0 uint8 [B, h*3//2, w], or per-frame plane tuples of pitched rows: a plane's buffer must hold rows x pitch
    bytes); they are only read, 4:2:0 pixels are converted as ``yuv_to_bgr`` converts them.  lms [N,10] landmark rows in FRAME pixels,
    image after image, counts [B] (N = their sum).  Chip options and the result (chips, matrices) as ``align_faces``; the matrices are
    chip -> frame maps.  The kernel reads dwords: planes whose pitch is not a multiple of 4 are copied into padded rows first."""
    tab, B, h, w, pitch0, pitch1, keep = _lib.frame_planes(frames, fmt, writable=False)
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    lms = np.ascontiguousarray(lms, dtype=np.float32)
    if lms.ndim != 2 or lms.shape[1] != 10:
        raise ValueError("landmarks must be [N,10] rows, got %s" % (lms.shape,))
    if counts.shape[0] != B or (counts < 0).any() or int(counts.sum()) != lms.shape[0]:
        raise ValueError("counts must be [B] non-negative and sum to the number of landmark rows")
    tab, pitch0, pitch1, keep4 = _lib.frames_pitch4(tab, fmt, B, h, w, pitch0, pitch1)
    o, tm, shape, dtype = _lib.align_opts(size, out, rgb, mean, scale, template, max_per_image)
    N = int(np.minimum(counts, max_per_image).sum()) if max_per_image > 0 else lms.shape[0]
    chips = np.zeros((N,) + shape, dtype)
    mats = np.zeros((N, 6), np.float64)
    _lib.check(_lib.lib().cf_op_align_frame(device, _lib.frame_format(fmt), tab, B, h, w, pitch0, pitch1, ptr(lms), ptr(counts), C.byref(o),
                                            ptr(chips), ptr(mats)), op=True)
    del keep, keep4
    return chips, mats


def redact_faces(frames, boxes, counts, net_hw, fmt="bgr", mode="mosaic", shape="ellipse", cell=20, scale=1.3, fill=(0, 0, 0), device=0):
    """Face redaction in the frame (``cf_op_redact``): ``frames`` -- BGR uint8 [B,h,w,3], dense 4:2:0 uint8 [B, h*3//2, w], or a list of
    per-frame plane tuples (pitched rows) -- are modified IN PLACE and returned.  boxes [N,4] x1,y1,x2,y2 in the coordinates of a
    network input of ``net_hw`` = (H, W), image after image, counts [B] (N = their sum).  Every sample that the box grown by ``scale``
    (``shape='rect'``) or the ellipse inscribed in it covers becomes ``fill`` (``mode='solid'``; bytes in the frame's channel order) or
    the mean of its ``cell`` x ``cell`` mosaic cell, a grid anchored at the frame origin."""
    tab, B, h, w, pitch0, pitch1, keep = _lib.frame_planes(frames, fmt)
    boxes, counts = _lib.box_rows(boxes, counts, B)
    o = _lib.redact_opts(mode, shape, cell, scale, fill)
    _lib.check(_lib.lib().cf_op_redact(device, C.byref(o), _lib.frame_format(fmt), tab, B, h, w, pitch0, pitch1, ptr(boxes), ptr(counts),
                                       int(net_hw[0]), int(net_hw[1])), op=True)
    del keep
    return frames


def blur_faces(frames, boxes, counts, net_hw, fmt="bgr", shape="ellipse", radius=0, scale=1.3, device=0):
    """Blur redaction in the frame (``cf_op_blur``): ``frames``, ``boxes``, ``counts`` and ``net_hw`` as ``redact_faces`` takes them; the
    frames are modified IN PLACE and returned.  Every sample that the box grown by ``scale`` (``shape='rect'``) or the ellipse inscribed
    in it covers becomes the box * box * box filtered value (width 2r+1 each, sigma about r) of the untouched frame; ``radius`` = r in
    1..24, or 0 for a per-face r of an eighth of the box's smaller side."""
    tab, B, h, w, pitch0, pitch1, keep = _lib.frame_planes(frames, fmt)
    boxes, counts = _lib.box_rows(boxes, counts, B)
    o = _lib.blur_opts(shape, radius, scale)
    _lib.check(_lib.lib().cf_op_blur(device, C.byref(o), _lib.frame_format(fmt), tab, B, h, w, pitch0, pitch1, ptr(boxes), ptr(counts),
                                     int(net_hw[0]), int(net_hw[1])), op=True)
    del keep
    return frames


def bgr_to_yuv_color(bgr):
    """(Y, U, V) of a (B, G, R) byte triple: integer BT.601 limited range, ``>> 8`` as floor division.  White -> (235, 128, 128),
    black -> (16, 128, 128), the reference's box green (2, 255, 0) -> (145, 55, 34)."""
    b, g, r = (int(v) for v in bgr)
    return (((66 * r + 129 * g + 25 * b + 128) >> 8) + 16, ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128,
            ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128)


def _draw_rows(boxes, scores, counts, B, lms, info):
    boxes, counts = _lib.box_rows(boxes, counts, B)
    N = boxes.shape[0]
    scores = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
    lms = None if lms is None else np.ascontiguousarray(lms, dtype=np.float32).reshape(-1, 10)
    info = None if info is None else np.ascontiguousarray(info, dtype=np.int32).reshape(-1, 3)
    for a, what in ((scores, "scores"), (lms, "lms"), (info, "info")):
        if a is not None and a.shape[0] != N:
            raise ValueError("%s has %d rows, boxes %d" % (what, a.shape[0], N))
    return boxes, scores, counts, lms, info


def draw_faces(frames, boxes, scores, counts, net_hw, fmt="bgr", lms=None, info=None, device=0, **opts):
    """Annotation in the frame (``cf_op_draw``): ``frames`` as ``redact_faces`` takes them are modified IN PLACE and returned.  boxes
    [N,4] x1,y1,x2,y2 and lms [N,10] in the coordinates of a network input of ``net_hw`` = (H, W), scores [N], info [N,3] = id, hits,
    misses (``None``: all rows live), image after image, counts [B].  ``opts``: those of ``_lib.draw_opts`` -- boxes, landmarks,
    thickness, radius, label ('none' | 'score' | 'id'), label_scale, dash_held, scale and the four colours, bytes in the frame's own
    channel order."""
    tab, B, h, w, pitch0, pitch1, keep = _lib.frame_planes(frames, fmt)
    boxes, scores, counts, lms, info = _draw_rows(boxes, scores, counts, B, lms, info)
    o = _lib.draw_opts(**opts)
    _lib.check(_lib.lib().cf_op_draw(device, C.byref(o), _lib.frame_format(fmt), tab, B, h, w, pitch0, pitch1, ptr(boxes), ptr(scores), ptr(lms),
                                     ptr(info), ptr(counts), int(net_hw[0]), int(net_hw[1])), op=True)
    del keep
    return frames


def draw_layout(box, score, frame_hw, net_hw, lms=None, info=None, **opts):
    """One row's integer geometry (``cf_draw_layout``; host only, the code the kernels run): int32 [32] = ok, X1, Y1, X2, Y2, held, plate
    x0, y0, Pw, Ph, n, ten digits, the landmarks' valid bits, Lx0, Ly0 .. Lx4, Ly4."""
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(4)
    lms = None if lms is None else np.ascontiguousarray(lms, dtype=np.float32).reshape(10)
    info = None if info is None else np.ascontiguousarray(info, dtype=np.int32).reshape(3)
    out = np.zeros((32,), np.int32)
    o = _lib.draw_opts(**opts)
    _lib.check(_lib.lib().cf_draw_layout(C.byref(o), ptr(box), float(np.float32(score)), ptr(lms), ptr(info), int(frame_hw[0]), int(frame_hw[1]),
                                         int(net_hw[0]), int(net_hw[1]), ptr(out)), op=True)
    return out


def tile_grid(h, w, tile, overlap, with_full=True):
    """The rectangles of sliced inference (``cf_tile_grid``; host only): int32 [T][4] rows (x0, y0, w, h) covering an h x w frame with
    tiles of ``tile`` = (tile_h, tile_w) or one int, neighbours sharing at least ``overlap`` pixels, row-major; the whole frame is
    appended when ``with_full`` and there is more than one tile.  All values even."""
    th, tw = (int(tile), int(tile)) if np.isscalar(tile) else (int(tile[0]), int(tile[1]))
    n = C.c_int(0)
    L = _lib.lib()
    _lib.check(L.cf_tile_grid(int(h), int(w), th, tw, int(overlap), 1 if with_full else 0, None, 0, C.byref(n)), op=True)
    tab = (_lib.TileRect * max(n.value, 1))()
    _lib.check(L.cf_tile_grid(int(h), int(w), th, tw, int(overlap), 1 if with_full else 0, tab, n.value, C.byref(n)), op=True)
    return np.array([[r.x0, r.y0, r.w, r.h] for r in tab[:n.value]], np.int32).reshape(-1, 4)


def cut_tiles(frames, rects, size, fmt="bgr", device=0):
    """The tile cutter (``cf_op_cut_tiles``): uint8 [Bf, T, H, W, 3] BGR, tile (f, t) = the rectangle ``rects[t]`` = (x0, y0, w, h) of
    frame f, converted to BGR (4:2:0 formats) and resized to ``size`` = (H, W) with the taps clamped at the rectangle's edges.
    ``frames`` as ``redact_faces`` takes them (BGR [B,h,w,3], dense 4:2:0 [B, h*3//2, w], or per-frame plane tuples of pitched rows: a
    plane's buffer must hold rows x pitch bytes); they are only read."""
    tab, B, h, w, pitch0, pitch1, keep = _lib.frame_planes(frames, fmt, writable=False)
    rt, T = _lib.tile_rects(rects)
    H, W = int(size[0]), int(size[1])
    out = np.empty((B, T, H, W, 3), np.uint8)
    _lib.check(_lib.lib().cf_op_cut_tiles(device, _lib.frame_format(fmt), tab, B, h, w, pitch0, pitch1, rt, T, H, W, ptr(out)), op=True)
    del keep
    return out


def merge_tiles(rects, frame_hw, net_hw, dets_net, scores, lms_net, counts, max_out, metric="ios", thresh=0.5, edge=2.0, dets=None, lms=None,
                device=0):
    """The merge of per-tile detections (``cf_op_merge_tiles``): dets_net [Bf, T, rows, 4] box corners, scores [Bf, T, rows], lms_net
    [Bf, T, rows, 10] in the coordinates of a ``net_hw`` = (H, W) network input, counts [Bf, T]; per tile the rows below min(count, rows)
    are filtered by the edge rule, mapped into the ``frame_hw`` = (h, w) frame and de-duplicated per frame by greedy NMS with ``metric``
    ('iou' | 'ios') and ``thresh``.  Returns (dets [Bf, max_out, 5], lms [Bf, max_out, 10], counts [Bf], flags [Bf]); rows at and past
    a frame's count keep the bytes of the ``dets`` / ``lms`` arrays passed in (zeros by default)."""
    rt, T = _lib.tile_rects(rects)
    d = np.ascontiguousarray(dets_net, dtype=np.float32)
    if d.ndim != 4 or d.shape[1] != T or d.shape[3] != 4:
        raise ValueError("dets_net must be [Bf, T=%d, rows, 4], got %s" % (T, d.shape))
    Bf, _, rows, _ = d.shape
    sc = np.ascontiguousarray(scores, dtype=np.float32).reshape(Bf, T, rows)
    lm = np.ascontiguousarray(lms_net, dtype=np.float32).reshape(Bf, T, rows, 10)
    cn = np.ascontiguousarray(counts, dtype=np.int32).reshape(Bf, T)
    max_out = int(max_out)
    od = np.zeros((Bf, max_out, 5), np.float32) if dets is None else np.ascontiguousarray(dets, dtype=np.float32).reshape(Bf, max_out, 5)
    ol = np.zeros((Bf, max_out, 10), np.float32) if lms is None else np.ascontiguousarray(lms, dtype=np.float32).reshape(Bf, max_out, 10)
    oc, fl = np.zeros((Bf,), np.int32), np.zeros((Bf,), np.int32)
    o = _lib.merge_opts(metric, thresh, edge)
    _lib.check(_lib.lib().cf_op_merge_tiles(device, C.byref(o), rt, T, Bf, int(frame_hw[0]), int(frame_hw[1]), int(net_hw[0]), int(net_hw[1]),
                                            ptr(d), ptr(sc), ptr(lm), ptr(cn), rows, max_out, ptr(od), ptr(ol), ptr(oc), ptr(fl)), op=True)
    return od, ol, oc, fl


def fit_geometry(h, w, H, W, anchor="center", upscale=True):
    """The placement of an h x w frame in an H x W canvas with its aspect ratio kept (``cf_fit_geometry``, host only): (rw, rh, dx, dy)."""
    o, g = _lib.fit_opts(anchor, upscale), _lib.FitGeom()
    _lib.check(_lib.lib().cf_fit_geometry(C.byref(o), int(h), int(w), int(H), int(W), C.byref(g)), op=True)
    return g.rw, g.rh, g.dx, g.dy


def fit_frames(frames, size, fmt="bgr", anchor="center", upscale=True, fill=(0, 0, 0), device=0):
    """The fit kernel (``cf_op_fit``): uint8 [B, H, W, 3] BGR canvases of ``size`` = (H, W), frame b converted to BGR (4:2:0 formats),
    resized to (rh, rw) with its aspect ratio kept and pasted at (dy, dx), ``fill`` (B, G, R) elsewhere.  ``frames`` as ``cut_tiles``
    takes them; they are only read.  No accuracy claim is made for letterboxed input."""
    tab, B, h, w, pitch0, pitch1, keep = _lib.frame_planes(frames, fmt, writable=False)
    H, W = int(size[0]), int(size[1])
    o = _lib.fit_opts(anchor, upscale, fill)
    out = np.empty((B, H, W, 3), np.uint8)
    _lib.check(_lib.lib().cf_op_fit(device, C.byref(o), _lib.frame_format(fmt), tab, B, h, w, pitch0, pitch1, H, W, ptr(out)), op=True)
    del keep
    return out


def unfit_rows(frame_hw, net_hw, dets_net, scores, lms_net, counts, max_out, anchor="center", upscale=True, dets=None, lms=None, device=0):
    """The mapping of decoded rows back into frame pixels (``cf_op_unfit``): dets_net [B, rows, 4] box corners, scores [B, rows], lms_net
    [B, rows, 10] in the coordinates of a ``net_hw`` = (H, W) canvas that holds a fitted ``frame_hw`` = (h, w) frame, counts [B]; the rows
    below min(count, rows) whose corners are finite and whose centre lies in the content are mapped and compacted in order.  Returns
    (dets [B, max_out, 5], lms [B, max_out, 10], counts [B], flags [B]); rows at and past an image's count keep the bytes of the
    ``dets`` / ``lms`` arrays passed in (zeros by default)."""
    d = np.ascontiguousarray(dets_net, dtype=np.float32)
    if d.ndim != 3 or d.shape[2] != 4:
        raise ValueError("dets_net must be [B, rows, 4], got %s" % (d.shape,))
    B, rows, _ = d.shape
    sc = np.ascontiguousarray(scores, dtype=np.float32).reshape(B, rows)
    lm = np.ascontiguousarray(lms_net, dtype=np.float32).reshape(B, rows, 10)
    cn = np.ascontiguousarray(counts, dtype=np.int32).reshape(B)
    max_out = int(max_out)
    od = np.zeros((B, max_out, 5), np.float32) if dets is None else np.ascontiguousarray(dets, dtype=np.float32).reshape(B, max_out, 5)
    ol = np.zeros((B, max_out, 10), np.float32) if lms is None else np.ascontiguousarray(lms, dtype=np.float32).reshape(B, max_out, 10)
    oc, fl = np.zeros((B,), np.int32), np.zeros((B,), np.int32)
    o = _lib.fit_opts(anchor, upscale)
    _lib.check(_lib.lib().cf_op_unfit(device, C.byref(o), B, int(frame_hw[0]), int(frame_hw[1]), int(net_hw[0]), int(net_hw[1]),
                                      ptr(d), ptr(sc), ptr(lm), ptr(cn), rows, max_out, ptr(od), ptr(ol), ptr(oc), ptr(fl)), op=True)
    return od, ol, oc, fl


def view_layout(h, w, H, W, tile=None, overlap=None, scales=(1.0,), anchor="center"):
    """The views of multi-scale detection (``cf_view_layout``; host only): int32 [V][8] rows (sx0, sy0, sw, sh, dx, dy, dw, dh) for an
    h x w frame in an H x W canvas.  Tiles first (``tile`` = one int or (tile_h, tile_w), None: no tiles; only when there is more than
    one), each filling the canvas; then one whole-frame level per entry of ``scales`` (fractions of the fitted size, rounded to per
    mille, each within 0.001 .. 1.0), placed by ``anchor`` ('center' | 'topleft').  No accuracy claim is made for any layout."""
    o = _lib.view_opts(tile, overlap, scales, anchor)
    n = C.c_int(0)
    L = _lib.lib()
    _lib.check(L.cf_view_layout(C.byref(o), int(h), int(w), int(H), int(W), None, 0, C.byref(n)), op=True)
    tab = (_lib.View * max(n.value, 1))()
    _lib.check(L.cf_view_layout(C.byref(o), int(h), int(w), int(H), int(W), tab, n.value, C.byref(n)), op=True)
    return np.array([[v.sx0, v.sy0, v.sw, v.sh, v.dx, v.dy, v.dw, v.dh] for v in tab[:n.value]], np.int32).reshape(-1, 8)


def cut_views(frames, views, size, fmt="bgr", fill=(0, 0, 0), device=0):
    """The views cutter (``cf_op_views``): uint8 [Bf, V, H, W, 3] BGR canvases of ``size`` = (H, W); canvas (f, v) is ``fill`` (B, G, R)
    with the source rectangle of ``views[v]`` = (sx0, sy0, sw, sh, dx, dy, dw, dh) of frame f, converted to BGR (4:2:0 formats) and
    resized to (dh, dw) with the taps clamped at the rectangle's edges, pasted at (dy, dx).  ``frames`` as ``cut_tiles`` takes them; they
    are only read."""
    tab, B, h, w, pitch0, pitch1, keep = _lib.frame_planes(frames, fmt, writable=False)
    vt, V = _lib.view_table(views)
    H, W = int(size[0]), int(size[1])
    fb = _lib.fill_bytes(fill)
    out = np.empty((B, V, H, W, 3), np.uint8)
    _lib.check(_lib.lib().cf_op_views(device, _lib.frame_format(fmt), tab, B, h, w, pitch0, pitch1, vt, V, fb, H, W, ptr(out)), op=True)
    del keep
    return out


def merge_views(views, frame_hw, net_hw, dets_net, scores, lms_net, counts, max_out, metric="ios", thresh=0.5, edge=2.0, dets=None, lms=None,
                device=0):
    """The merge of per-view detections (``cf_op_merge_views``): dets_net [Bf, V, rows, 4] box corners, scores [Bf, V, rows], lms_net
    [Bf, V, rows, 10] in the coordinates of a ``net_hw`` = (H, W) canvas, counts [Bf, V]; per view the rows below min(count, rows) are
    filtered (finite corners, centre inside the content, the edge rule at content sides whose source side is interior to the frame),
    mapped into the ``frame_hw`` = (h, w) frame and de-duplicated per frame by greedy NMS with ``metric`` ('iou' | 'ios') and ``thresh``.
    Returns (dets [Bf, max_out, 5], lms [Bf, max_out, 10], counts [Bf], flags [Bf]); rows at and past a frame's count keep the bytes of
    the ``dets`` / ``lms`` arrays passed in (zeros by default)."""
    vt, V = _lib.view_table(views)
    d = np.ascontiguousarray(dets_net, dtype=np.float32)
    if d.ndim != 4 or d.shape[1] != V or d.shape[3] != 4:
        raise ValueError("dets_net must be [Bf, V=%d, rows, 4], got %s" % (V, d.shape))
    Bf, _, rows, _ = d.shape
    sc = np.ascontiguousarray(scores, dtype=np.float32).reshape(Bf, V, rows)
    lm = np.ascontiguousarray(lms_net, dtype=np.float32).reshape(Bf, V, rows, 10)
    cn = np.ascontiguousarray(counts, dtype=np.int32).reshape(Bf, V)
    max_out = int(max_out)
    od = np.zeros((Bf, max_out, 5), np.float32) if dets is None else np.ascontiguousarray(dets, dtype=np.float32).reshape(Bf, max_out, 5)
    ol = np.zeros((Bf, max_out, 10), np.float32) if lms is None else np.ascontiguousarray(lms, dtype=np.float32).reshape(Bf, max_out, 10)
    oc, fl = np.zeros((Bf,), np.int32), np.zeros((Bf,), np.int32)
    o = _lib.merge_opts(metric, thresh, edge)
    _lib.check(_lib.lib().cf_op_merge_views(device, C.byref(o), vt, V, Bf, int(frame_hw[0]), int(frame_hw[1]), int(net_hw[0]), int(net_hw[1]),
                                            ptr(d), ptr(sc), ptr(lm), ptr(cn), rows, max_out, ptr(od), ptr(ol), ptr(oc), ptr(fl)), op=True)
    return od, ol, oc, fl


def pack_views(views, Bf, size, gutter=0):
    """The first-fit shelf packer (``cf_pack_views``; host only): the placements of the ``Bf * V`` (frame, view) pairs, frame-major, in
    canvases of ``size`` = (H, W) with ``gutter`` pixels of fill between contents.  Each view keeps its source rectangle and its
    (dw, dh); its dx, dy are replaced.  Returns (places int32 [Bf * V][10] rows (frame, canvas, sx0, sy0, sw, sh, dx, dy, dw, dh), the
    number of canvases).  A view that fills the canvas gets a canvas of its own.  ``gutter`` = 0 is this project's default; nobody has
    measured it (no trained weights, no labelled set): contents that share an edge share the threshold decode's NMS."""
    vt, V = _lib.view_table(views)
    H, W = int(size[0]), int(size[1])
    n, nc = C.c_int(0), C.c_int(0)
    L = _lib.lib()
    _lib.check(L.cf_pack_views(vt, V, int(Bf), H, W, int(gutter), None, 0, C.byref(n), C.byref(nc)), op=True)
    tab = (_lib.Place * max(n.value, 1))()
    _lib.check(L.cf_pack_views(vt, V, int(Bf), H, W, int(gutter), tab, n.value, C.byref(n), C.byref(nc)), op=True)
    return np.frombuffer(tab, np.int32).reshape(-1, 10)[:n.value].copy(), nc.value


def cut_packed(frames, places, n_canvases, size, fmt="bgr", fill=(0, 0, 0), device=0, rot=0):
    """The packed cutter (``cf_op_packed``): uint8 [N, H, W, 3] BGR canvases of ``size`` = (H, W), N = ``n_canvases``; canvas n is
    ``fill`` (B, G, R) and, inside the content rectangle of every row (frame, canvas, sx0, sy0, sw, sh, dx, dy, dw, dh) of ``places``
    with canvas == n, what ``cut_views`` makes of that view of that frame.  The contents of one canvas must not overlap.  ``frames`` as
    ``cut_views`` takes them; they are only read.  ``rot`` 90, 180 or 270 (``cf_op_packed_rot``): the clockwise turn that makes the
    STORED frames upright; the source rectangles are then in pixels of the upright view (``np.rot90`` of the frame's BGR)."""
    tab, B, h, w, pitch0, pitch1, keep = _lib.frame_planes(frames, fmt, writable=False)
    pt, P = _lib.place_table(places)
    H, W, N = int(size[0]), int(size[1]), int(n_canvases)
    fb = _lib.fill_bytes(fill)
    out = np.empty((max(N, 0), H, W, 3), np.uint8)
    if rot:
        _lib.check(_lib.lib().cf_op_packed_rot(device, int(rot), _lib.frame_format(fmt), tab, B, h, w, pitch0, pitch1, pt, P, N, fb, H, W, ptr(out)), op=True)
    else:
        _lib.check(_lib.lib().cf_op_packed(device, _lib.frame_format(fmt), tab, B, h, w, pitch0, pitch1, pt, P, N, fb, H, W, ptr(out)), op=True)
    del keep
    return out


def merge_packed(places, n_frames, frame_hw, net_hw, dets_net, scores, lms_net, counts, max_out, metric="ios", thresh=0.5, edge=2.0, dets=None,
                 lms=None, device=0, rot=0):
    """The merge of per-canvas detections by placement (``cf_op_merge_packed``): dets_net [N, rows, 4] box corners, scores [N, rows],
    lms_net [N, rows, 10] in the coordinates of a ``net_hw`` = (H, W) canvas, counts [N].  Frame f's candidates are the rows below
    min(count, rows) of the canvas of each of its placements (placement order, then row order), filtered against that placement's
    content by the rules of ``merge_views``, mapped into the ``frame_hw`` = (h, w) frame and de-duplicated per frame by greedy NMS.
    Returns (dets [Bf, max_out, 5], lms [Bf, max_out, 10], counts [Bf], flags [Bf]) with Bf = ``n_frames``; rows at and past a frame's
    count keep the bytes of the ``dets`` / ``lms`` arrays passed in (zeros by default).  ``rot`` 90, 180 or 270
    (``cf_op_merge_packed_rot``): the placements' sources lie in the upright view of the STORED ``frame_hw`` frame, the edge rule tests
    against that view, and the rows come back in the stored frame's pixels (boxes assigned from mapped corners, landmarks in order)."""
    pt, P = _lib.place_table(places)
    d = np.ascontiguousarray(dets_net, dtype=np.float32)
    if d.ndim != 3 or d.shape[2] != 4:
        raise ValueError("dets_net must be [N, rows, 4], got %s" % (d.shape,))
    N, rows, Bf = d.shape[0], d.shape[1], int(n_frames)
    sc = np.ascontiguousarray(scores, dtype=np.float32).reshape(N, rows)
    lm = np.ascontiguousarray(lms_net, dtype=np.float32).reshape(N, rows, 10)
    cn = np.ascontiguousarray(counts, dtype=np.int32).reshape(N)
    max_out = int(max_out)
    shape = (max(Bf, 0), max(max_out, 0))
    od = np.zeros(shape + (5,), np.float32) if dets is None else np.ascontiguousarray(dets, dtype=np.float32).reshape(shape + (5,))
    ol = np.zeros(shape + (10,), np.float32) if lms is None else np.ascontiguousarray(lms, dtype=np.float32).reshape(shape + (10,))
    oc, fl = np.zeros((shape[0],), np.int32), np.zeros((shape[0],), np.int32)
    o = _lib.merge_opts(metric, thresh, edge)
    args = (pt, P, N, Bf, int(frame_hw[0]), int(frame_hw[1]), int(net_hw[0]), int(net_hw[1]), ptr(d), ptr(sc), ptr(lm), ptr(cn), rows, max_out, ptr(od),
            ptr(ol), ptr(oc), ptr(fl))
    if rot:
        _lib.check(_lib.lib().cf_op_merge_packed_rot(device, int(rot), C.byref(o), *args), op=True)
    else:
        _lib.check(_lib.lib().cf_op_merge_packed(device, C.byref(o), *args), op=True)
    return od, ol, oc, fl


def rot_geometry(h, w, H, W, rot, fit=None):
    """The placement of the UPRIGHT view of a stored h x w frame in an H x W canvas (``cf_rot_geometry``, host only): (rw, rh, dx, dy).
    ``rot``: the clockwise turn (0, 90, 180, 270) that makes the frame upright; ``fit`` as ``_lib.rot_opts`` takes it (None: stretch)."""
    o, g = _lib.rot_opts(rot, fit), _lib.FitGeom()
    _lib.check(_lib.lib().cf_rot_geometry(C.byref(o), int(h), int(w), int(H), int(W), C.byref(g)), op=True)
    return g.rw, g.rh, g.dx, g.dy


def rot_frames(frames, size, fmt="bgr", rot=0, fit=None, device=0):
    """The kernel of ``cf_forward_rot`` (``cf_op_rot``): uint8 [B, H, W, 3] BGR canvases of ``size`` = (H, W) from the upright view of the
    stored ``frames`` (as ``fit_frames`` takes them; only read): frame b converted to BGR, turned ``rot`` degrees clockwise, then stretched
    to the canvas (``fit`` = None) or fitted into it (True, or a dict of ``fit_opts`` keywords).  rot = 0 with a fit is ``fit_frames``."""
    tab, B, h, w, pitch0, pitch1, keep = _lib.frame_planes(frames, fmt, writable=False)
    H, W = int(size[0]), int(size[1])
    o = _lib.rot_opts(rot, fit)
    out = np.empty((B, H, W, 3), np.uint8)
    _lib.check(_lib.lib().cf_op_rot(device, C.byref(o), _lib.frame_format(fmt), tab, B, h, w, pitch0, pitch1, H, W, ptr(out)), op=True)
    del keep
    return out


def unrot_rows(frame_hw, net_hw, dets_net, scores, lms_net, counts, max_out, rot=0, fit=None, dets=None, lms=None, device=0):
    """The mapping of decoded rows back into the pixels of the STORED frame (``cf_op_unrot``): ``unfit_rows`` behind a canvas that holds
    the upright view of a ``frame_hw`` = (h, w) frame turned ``rot`` degrees clockwise, stretched (``fit`` = None) or fitted.  Boxes are
    assigned from mapped corners (no min / max); landmarks keep their order."""
    d = np.ascontiguousarray(dets_net, dtype=np.float32)
    if d.ndim != 3 or d.shape[2] != 4:
        raise ValueError("dets_net must be [B, rows, 4], got %s" % (d.shape,))
    B, rows, _ = d.shape
    sc = np.ascontiguousarray(scores, dtype=np.float32).reshape(B, rows)
    lm = np.ascontiguousarray(lms_net, dtype=np.float32).reshape(B, rows, 10)
    cn = np.ascontiguousarray(counts, dtype=np.int32).reshape(B)
    max_out = int(max_out)
    od = np.zeros((B, max_out, 5), np.float32) if dets is None else np.ascontiguousarray(dets, dtype=np.float32).reshape(B, max_out, 5)
    ol = np.zeros((B, max_out, 10), np.float32) if lms is None else np.ascontiguousarray(lms, dtype=np.float32).reshape(B, max_out, 10)
    oc, fl = np.zeros((B,), np.int32), np.zeros((B,), np.int32)
    o = _lib.rot_opts(rot, fit)
    _lib.check(_lib.lib().cf_op_unrot(device, C.byref(o), B, int(frame_hw[0]), int(frame_hw[1]), int(net_hw[0]), int(net_hw[1]),
                                      ptr(d), ptr(sc), ptr(lm), ptr(cn), rows, max_out, ptr(od), ptr(ol), ptr(oc), ptr(fl)), op=True)
    return od, ol, oc, fl


def mirror_batch(x, device=0):
    """The mirror kernel of the flip test (``cf_op_mirror``): ``x`` uint8 [B, H, W, 3] or float32 [B, 3, H, W] with W a multiple of 32 ->
    the same batch with the columns of every image reversed (whole pixels), written on the device as the flip forward writes the
    second half of its 2B input."""
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint8:
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError("uint8 input must be [B, H, W, 3], got %s" % (x.shape,))
        fmt, (B, H, W) = _lib.CF_IN_U8_HWC_BGR, x.shape[:3]
    else:
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError("float input must be [B, 3, H, W], got %s" % (x.shape,))
        fmt, (B, H, W) = _lib.CF_IN_F32_NCHW, (x.shape[0], x.shape[2], x.shape[3])
    out = np.empty_like(x)
    _lib.check(_lib.lib().cf_op_mirror(device, fmt, ptr(x), B, H, W, ptr(out)), op=True)
    return out


def flip_heads(records, B, device=0):
    """The merge kernel of the flip test (``cf_op_flip_heads``): ``records`` float32 [2B, h, w, 16] head records, the B unmirrored
    images first, then their mirrored passes -> (records [B, h, w, 16], hm_plane [B, h*w]) by the statement under ``cf_set_flip_test`` in
    include/centerface_hip.h (heat and wh averaged, landmark x negated with the point pairs 0 <-> 1 and 3 <-> 4 swapped, reg of the
    unmirrored pass)."""
    r = np.ascontiguousarray(records, dtype=np.float32)
    B = int(B)
    if r.ndim != 4 or r.shape[3] != 16 or r.shape[0] != 2 * B:
        raise ValueError("records must be [2B, h, w, 16] with B=%d, got %s" % (B, r.shape))
    h, w = r.shape[1:3]
    out, plane = np.empty((B, h, w, 16), np.float32), np.empty((B, h * w), np.float32)
    _lib.check(_lib.lib().cf_op_flip_heads(device, ptr(r), B, h, w, ptr(out), ptr(plane)), op=True)
    return out, plane


def track_sequence(boxes, scores, lms, counts, dets=None, lms_out=None, info=None, device=0, birth_score=None, weak_iou=None, motion=None, vel=False,
                   **opts):
    """The tracker's update over a whole sequence (``cf_op_track``) with a fresh tracker: boxes [F, S, rows, 4], scores [F, S, rows], lms
    [F, S, rows, 10], counts [F, S] -- frame f of stream s has the rows below min(count, rows), in whatever coordinates they are.
    ``opts``: iou, max_age, min_hits, max_tracks, hold_grow (``_lib.track_opts``).  ``birth_score``: the tracker with two thresholds
    (``cf_op_track_weak``) -- rows with score > birth_score associate as before, the others may only match a confirmed track, at IoU >=
    ``weak_iou`` (0.5 unless given), and are never born; flag bit 1 says that one did.  Returns (dets [F, S, max_tracks, 5], lms
    [F, S, max_tracks, 10], info [F, S, max_tracks, 3] = id, hits, misses, counts [F, S], flags [F, S]) after every frame; rows at and
    past a count keep the bytes of the ``dets`` / ``lms_out`` / ``info`` arrays passed in (zeros by default).
    ``motion``: None, True or dict(gain=, damp=) -- the tracker with constant-velocity prediction (``cf_op_track_ex``; include/centerface_hip.h
    "constant velocity"): rows are matched against the predicted boxes and held boxes coast.  gain 0.5 and damp 1.0 are this project's
    choices; nobody has measured them and no accuracy claim is made.  ``vel=True``: the velocities [F, S, max_tracks, 2] of the output rows
    are returned as a sixth item (an array: it is also the initial content; all zero without ``motion``)."""
    o = _lib.track_opts(**opts)
    if birth_score is None and weak_iou is not None:
        raise ValueError("weak_iou needs birth_score")
    wo = None if birth_score is None else _lib.track_weak_opts(birth_score, 0.5 if weak_iou is None else weak_iou)
    mo = _lib.track_motion_of(motion)
    b = np.ascontiguousarray(boxes, dtype=np.float32)
    if b.ndim != 4 or b.shape[3] != 4:
        raise ValueError("boxes must be [F, S, rows, 4], got %s" % (b.shape,))
    F, S, rows, _ = b.shape
    sc = np.ascontiguousarray(scores, dtype=np.float32).reshape(F, S, rows)
    lm = np.ascontiguousarray(lms, dtype=np.float32).reshape(F, S, rows, 10)
    cn = np.ascontiguousarray(counts, dtype=np.int32).reshape(F, S)
    M = max(int(o.max_tracks), 1)
    od = np.zeros((F, S, M, 5), np.float32) if dets is None else np.ascontiguousarray(dets, dtype=np.float32).reshape(F, S, M, 5)
    ol = np.zeros((F, S, M, 10), np.float32) if lms_out is None else np.ascontiguousarray(lms_out, dtype=np.float32).reshape(F, S, M, 10)
    oi = np.zeros((F, S, M, 3), np.int32) if info is None else np.ascontiguousarray(info, dtype=np.int32).reshape(F, S, M, 3)
    oc, fl = np.zeros((F, S), np.int32), np.zeros((F, S), np.int32)
    tabs = (ptr(b), ptr(sc), ptr(lm), ptr(cn), ptr(od), ptr(ol), ptr(oi), ptr(oc), ptr(fl))
    want_vel = vel is not None and vel is not False
    ov = None
    if want_vel:
        ov = np.zeros((F, S, M, 2), np.float32) if vel is True else np.ascontiguousarray(vel, dtype=np.float32).reshape(F, S, M, 2)
    if mo is not None:
        _lib.check(_lib.lib().cf_op_track_ex(device, C.byref(o), None if wo is None else C.byref(wo), C.byref(mo), S, F, rows, *tabs,
                                             None if ov is None else ptr(ov)), op=True)
    elif wo is None:
        _lib.check(_lib.lib().cf_op_track(device, C.byref(o), S, F, rows, *tabs), op=True)
    else:
        _lib.check(_lib.lib().cf_op_track_weak(device, C.byref(o), C.byref(wo), S, F, rows, *tabs), op=True)
    return (od, ol, oi, oc, fl, ov) if want_vel else (od, ol, oi, oc, fl)


def follow_sequence(boxes, scores, lms, counts, frames, fmt="bgr", space_hw=None, detect=None, *, tiled=False, search=4, max_sad=4096,
                    dets=None, lms_out=None, info=None, moves=None, device=0, motion=None, birth_score=None, weak_iou=None, **opts):
    """``track_sequence`` with the follower behind every frame (``cf_op_follow``): frame f of stream s is ``frames[f * S + s]`` -- F * S host
    frames of one size as ``redact_faces`` takes them (BGR uint8 [F*S,h,w,3], dense 4:2:0 uint8 [F*S, h*3//2, w], or per-frame plane
    tuples of pitched rows), only read.  ``detect`` [F] (default: all): where it is set the update with the frame's rows runs first,
    then the faces are followed in the frame -- block matching of a 16 x 16 cell template within ``search`` cells, a best match above
    ``max_sad`` moves nothing; the two defaults are this project's choices, no accuracy claim is made for them.  ``space_hw``: the (H, W)
    the rows are in, mapped to the frame by w / W, h / H; ``tiled=True``: the rows are in frame pixels (``space_hw`` is the frame's size).
    ``opts`` as ``track_sequence``.  Returns (dets, lms, info, counts, flags, moves [F, S, max_tracks, 4] = px, py, SAD, code
    (``_lib.CF_FOLLOW_*``)) after every frame; rows at and past a count keep the bytes of the arrays passed in (zeros by default).
    ``motion`` (and ``birth_score`` / ``weak_iou``) as ``track_sequence``: the updates are those of that tracker (``cf_op_follow_ex``), and a
    coasted slot is FOLLOWED from its coasted place with the template of its last detection."""
    o, fo = _lib.track_opts(**opts), _lib.follow_opts(search, max_sad)
    if birth_score is None and weak_iou is not None:
        raise ValueError("weak_iou needs birth_score")
    wo = None if birth_score is None else _lib.track_weak_opts(birth_score, 0.5 if weak_iou is None else weak_iou)
    mo = _lib.track_motion_of(motion)
    b = np.ascontiguousarray(boxes, dtype=np.float32)
    if b.ndim != 4 or b.shape[3] != 4:
        raise ValueError("boxes must be [F, S, rows, 4], got %s" % (b.shape,))
    F, S, rows, _ = b.shape
    sc = np.ascontiguousarray(scores, dtype=np.float32).reshape(F, S, rows)
    lm = np.ascontiguousarray(lms, dtype=np.float32).reshape(F, S, rows, 10)
    cn = np.ascontiguousarray(counts, dtype=np.int32).reshape(F, S)
    dt = np.ones((F,), np.uint8) if detect is None else np.ascontiguousarray(np.asarray(detect).astype(bool), dtype=np.uint8).reshape(F)
    tab, B, h, w, pitch0, pitch1, keep = _lib.frame_planes(frames, fmt, writable=False)
    if B != F * S:
        raise ValueError("%d frames for F x S = %d x %d" % (B, F, S))
    H, W = (h, w) if space_hw is None else (int(space_hw[0]), int(space_hw[1]))
    M = max(int(o.max_tracks), 1)
    od = np.zeros((F, S, M, 5), np.float32) if dets is None else np.ascontiguousarray(dets, dtype=np.float32).reshape(F, S, M, 5)
    ol = np.zeros((F, S, M, 10), np.float32) if lms_out is None else np.ascontiguousarray(lms_out, dtype=np.float32).reshape(F, S, M, 10)
    oi = np.zeros((F, S, M, 3), np.int32) if info is None else np.ascontiguousarray(info, dtype=np.int32).reshape(F, S, M, 3)
    om = np.zeros((F, S, M, 4), np.int32) if moves is None else np.ascontiguousarray(moves, dtype=np.int32).reshape(F, S, M, 4)
    oc, fl = np.zeros((F, S), np.int32), np.zeros((F, S), np.int32)
    if wo is None and mo is None:
        _lib.check(_lib.lib().cf_op_follow(device, C.byref(o), C.byref(fo), S, F, rows, ptr(b), ptr(sc), ptr(lm), ptr(cn), ptr(dt), _lib.frame_format(fmt), tab,
                                           h, w, pitch0, pitch1, H, W, 1 if tiled else 0, ptr(od), ptr(ol), ptr(oi), ptr(oc), ptr(fl), ptr(om)), op=True)
    else:
        _lib.check(_lib.lib().cf_op_follow_ex(device, C.byref(o), None if wo is None else C.byref(wo), None if mo is None else C.byref(mo), C.byref(fo), S, F,
                                              rows, ptr(b), ptr(sc), ptr(lm), ptr(cn), ptr(dt), _lib.frame_format(fmt), tab, h, w, pitch0, pitch1, H, W,
                                              1 if tiled else 0, ptr(od), ptr(ol), ptr(oi), ptr(oc), ptr(fl), ptr(om)), op=True)
    del keep
    return od, ol, oi, oc, fl, om


def scene_sequence(frames, fmt, streams, hist=350, grid=640, sigs=False, device=0):
    """The scene check of ``Engine.scene_check`` over a whole sequence, with a fresh ``SceneCuts`` and no tracker (``cf_op_scene``): frame f
    of stream s is ``frames[f * S + s]`` -- F * S host frames of one even size, at least 8 x 8, as ``redact_faces`` takes them (BGR uint8
    [F*S,h,w,3], dense 4:2:0 uint8 [F*S, h*3//2, w], or per-frame plane tuples of pitched rows), only read.  Returns out int32 [F, S, 4] =
    code (``_lib.CF_SCENE_*``), hist, grid, run of every check; with ``sigs`` also the signatures int32 [F, S, 128] (64 bins, 64 cell
    means).  ``hist=350`` and ``grid=640`` are this project's choices; no accuracy claim is made for them."""
    o = _lib.scene_opts(hist, grid)
    S = int(streams)
    tab, B, h, w, pitch0, pitch1, keep = _lib.frame_planes(frames, fmt, writable=False)
    if S < 1 or B % S:
        raise ValueError("%d frames for %d streams" % (B, S))
    F = B // S
    out = np.zeros((F, S, 4), np.int32)
    sg = np.zeros((F, S, 128), np.int32) if sigs else None
    _lib.check(_lib.lib().cf_op_scene(device, C.byref(o), S, F, _lib.frame_format(fmt), tab, h, w, pitch0, pitch1, ptr(out), ptr(sg)), op=True)
    del keep
    return (out, sg) if sigs else out


def lookback_sequence(dets_in, lms_in, info_in, counts_in, push=None, cuts=None, dets=None, lms_out=None, info=None, device=0, **opts):
    """The lookback step of ``Engine.lookback_step`` over a whole sequence, with a fresh ``Lookback`` (``cf_op_lookback``): step f pushes,
    for every stream s, the tracked rows below counts_in[f, s] of dets_in [F, S, rows_in, 5], lms_in [F, S, rows_in, 10] and info_in
    [F, S, rows_in, 3] = id, hits, misses -- what ``track_sequence`` returns -- where ``push`` [F] is set (default: everywhere), and is a
    drain elsewhere.  ``cuts`` [F, S] (default: none): bit 0 = the scene check called the pushed frame a cut, bit 1 = a
    ``Lookback.forget`` of the stream comes before the step.  ``opts``: depth, rows, grow, confirm (``_lib.lookback_opts``; the defaults
    are this project's choices, no accuracy claim is made for them).  Returns (dets [F, S, rows, 5], lms [F, S, rows, 10], info
    [F, S, rows, 3], counts [F, S], state [F, S, 4] = seq, own rows, back-filled rows, flags -- seq -1 where nothing was emitted) after
    every step; rows at and past a count keep the bytes of the ``dets`` / ``lms_out`` / ``info`` arrays passed in (zeros by default)."""
    o = _lib.lookback_opts(**opts)
    d = np.ascontiguousarray(dets_in, dtype=np.float32)
    if d.ndim != 4 or d.shape[3] != 5:
        raise ValueError("dets_in must be [F, S, rows_in, 5], got %s" % (d.shape,))
    F, S, rows_in, _ = d.shape
    lm = np.ascontiguousarray(lms_in, dtype=np.float32).reshape(F, S, rows_in, 10)
    ii = np.ascontiguousarray(info_in, dtype=np.int32).reshape(F, S, rows_in, 3)
    cn = np.ascontiguousarray(counts_in, dtype=np.int32).reshape(F, S)
    pu = np.ones((F,), np.uint8) if push is None else np.ascontiguousarray(np.asarray(push) != 0, dtype=np.uint8).reshape(F)
    cu = None if cuts is None else np.ascontiguousarray(cuts, dtype=np.int32).reshape(F, S)
    R = max(int(o.rows), 1)
    od = np.zeros((F, S, R, 5), np.float32) if dets is None else np.ascontiguousarray(dets, dtype=np.float32).reshape(F, S, R, 5)
    ol = np.zeros((F, S, R, 10), np.float32) if lms_out is None else np.ascontiguousarray(lms_out, dtype=np.float32).reshape(F, S, R, 10)
    oi = np.zeros((F, S, R, 3), np.int32) if info is None else np.ascontiguousarray(info, dtype=np.int32).reshape(F, S, R, 3)
    oc, st = np.zeros((F, S), np.int32), np.zeros((F, S, 4), np.int32)
    _lib.check(_lib.lib().cf_op_lookback(device, C.byref(o), S, F, rows_in, ptr(pu), ptr(d), ptr(lm), ptr(ii), ptr(cn), ptr(cu), ptr(od), ptr(ol), ptr(oi),
                                         ptr(oc), ptr(st)), op=True)
    return od, ol, oi, oc, st


def lookback_trace_sequence(dets_in, lms_in, info_in, counts_in, frames, fmt, space_hw, push=None, cuts=None, *, tiled=False, search=4,
                            max_sad=4096, dets=None, lms_out=None, info=None, moves=None, device=0, **opts):
    """``lookback_sequence`` with a fresh ``Lookback`` that has ``trace(search, max_sad)`` set (``cf_op_lookback_trace``): step f of stream
    s has the frame ``frames[f * S + s]`` -- F * S host frames of one even size as ``follow_sequence`` takes them, only read; the frame of a
    drain is ignored --, whose luma is retained and through which the newborn faces are matched backwards.  ``space_hw``: the (H, W) the
    rows are in, mapped to the frame by w / W, h / H; ``tiled=True``: the rows are in frame pixels (``space_hw`` is the frame's size).
    Returns ``lookback_sequence``'s tuple plus moves [F, S, rows, 4] = PX, PY, SAD, code (``_lib.CF_FOLLOW_*``) of the back-filled rows
    (zeros for own rows); rows at and past a count keep the bytes of the arrays passed in (zeros by default)."""
    o, fo = _lib.lookback_opts(**opts), _lib.follow_opts(search, max_sad)
    d = np.ascontiguousarray(dets_in, dtype=np.float32)
    if d.ndim != 4 or d.shape[3] != 5:
        raise ValueError("dets_in must be [F, S, rows_in, 5], got %s" % (d.shape,))
    F, S, rows_in, _ = d.shape
    lm = np.ascontiguousarray(lms_in, dtype=np.float32).reshape(F, S, rows_in, 10)
    ii = np.ascontiguousarray(info_in, dtype=np.int32).reshape(F, S, rows_in, 3)
    cn = np.ascontiguousarray(counts_in, dtype=np.int32).reshape(F, S)
    pu = np.ones((F,), np.uint8) if push is None else np.ascontiguousarray(np.asarray(push) != 0, dtype=np.uint8).reshape(F)
    cu = None if cuts is None else np.ascontiguousarray(cuts, dtype=np.int32).reshape(F, S)
    tab, B, h, w, pitch0, pitch1, keep = _lib.frame_planes(frames, fmt, writable=False)
    if B != F * S:
        raise ValueError("%d frames for F x S = %d x %d" % (B, F, S))
    H, W = int(space_hw[0]), int(space_hw[1])
    R = max(int(o.rows), 1)
    od = np.zeros((F, S, R, 5), np.float32) if dets is None else np.ascontiguousarray(dets, dtype=np.float32).reshape(F, S, R, 5)
    ol = np.zeros((F, S, R, 10), np.float32) if lms_out is None else np.ascontiguousarray(lms_out, dtype=np.float32).reshape(F, S, R, 10)
    oi = np.zeros((F, S, R, 3), np.int32) if info is None else np.ascontiguousarray(info, dtype=np.int32).reshape(F, S, R, 3)
    om = np.zeros((F, S, R, 4), np.int32) if moves is None else np.ascontiguousarray(moves, dtype=np.int32).reshape(F, S, R, 4)
    oc, st = np.zeros((F, S), np.int32), np.zeros((F, S, 4), np.int32)
    _lib.check(_lib.lib().cf_op_lookback_trace(device, C.byref(o), C.byref(fo), S, F, rows_in, ptr(pu), ptr(d), ptr(lm), ptr(ii), ptr(cn), ptr(cu),
                                               _lib.frame_format(fmt), tab, h, w, pitch0, pitch1, H, W, 1 if tiled else 0, ptr(od), ptr(ol), ptr(oi),
                                               ptr(oc), ptr(st), ptr(om)), op=True)
    del keep
    return od, ol, oi, oc, st, om


def scene_signature(frame, fmt, device=0):
    """The 128 int32 of one frame's signature (``include/centerface_hip.h``: 64 luma bins, 8 x 8 cell means), computed on the device:
    ``frame`` is one BGR uint8 [h,w,3], one dense 4:2:0 uint8 [h*3//2, w], or one plane tuple."""
    one = np.ascontiguousarray(frame)[None] if isinstance(frame, np.ndarray) else [frame]
    return scene_sequence(one, fmt, 1, sigs=True, device=device)[1][0, 0]


def chip_quality(chips, boxes, scores, lms, fx=1.0, fy=1.0, *, min_hits=2, terms=("size", "pose", "score"), device=0):
    """The scoring kernel of the best-shot table alone (``cf_op_chip_quality``): chips uint8 [n, S, S, 3] BGR, their rows boxes [n, 4],
    scores [n], lms [n, 10] and the frame pixels per unit of the rows' space ``fx``, ``fy`` -> (quality int64 [n], parts int32 [n, 4] =
    sharp, size_w, pose_w, score_w).  The formula (``include/centerface_hip.h``) is this project's choice; no accuracy claim is made."""
    ch = np.ascontiguousarray(chips, dtype=np.uint8)
    if ch.ndim != 4 or ch.shape[1] != ch.shape[2] or ch.shape[3] != 3:
        raise ValueError("chips must be [n, S, S, 3], got %s" % (ch.shape,))
    n = ch.shape[0]
    o = _lib.bestshot_opts(ch.shape[1], 1, min_hits, terms)
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(n, 4)
    sc = np.ascontiguousarray(scores, dtype=np.float32).reshape(n)
    lm = np.ascontiguousarray(lms, dtype=np.float32).reshape(n, 10)
    q, parts = np.zeros((n,), np.int64), np.zeros((n, 4), np.int32)
    _lib.check(_lib.lib().cf_op_chip_quality(device, C.byref(o), ptr(ch), ptr(b), ptr(sc), ptr(lm), n, float(fx), float(fy), ptr(q), ptr(parts)), op=True)
    return q, parts


def bestshot_sequence(boxes, scores, lms, info, counts, chips, collect, cap=None, fx=1.0, fy=1.0, chip_counts=None, *, entries=320, min_hits=2,
                      terms=("size", "pose", "score"), out=None, device=0):
    """A whole scripted sequence of offers and collects on a fresh best-shot table (``cf_op_bestshot``), no engine and no tracker: frame f
    of stream s is offered the rows i < counts[f, s] of boxes [F, S, rows, 4], scores [F, S, rows], lms [F, S, rows, 10], info
    [F, S, rows, 3] = id, hits, misses with the chips [F, S, rows, Sz, Sz, 3]; the leading ``chip_counts[f, s]`` rows have a chip (default:
    all rows).  ``collect`` [F]: 0 none, 1 collect, 2 collect with flush, after that frame's offer, ``cap`` rows per stream (default
    ``entries``).  Returns a dict: chips [F, S, cap, Sz, Sz, 3], quality [F, S, cap] int64, records [F, S, cap, 8], dets [F, S, cap, 5],
    lms [F, S, cap, 10], counts / pending / flags [F, S] (zero on frames without a collect), offer_flags [F, S], offer_quality
    [F, S, rows] int64.  ``out``: a dict of arrays for chips / quality / records / dets / lms whose bytes rows at and past a count keep
    (zeros by default)."""
    b = np.ascontiguousarray(boxes, dtype=np.float32)
    if b.ndim != 4 or b.shape[3] != 4:
        raise ValueError("boxes must be [F, S, rows, 4], got %s" % (b.shape,))
    F, S, rows, _ = b.shape
    ch = np.ascontiguousarray(chips, dtype=np.uint8)
    if ch.ndim != 6 or ch.shape[:3] != (F, S, rows) or ch.shape[3] != ch.shape[4] or ch.shape[5] != 3:
        raise ValueError("chips must be [F, S, rows, Sz, Sz, 3], got %s" % (ch.shape,))
    Sz = ch.shape[3]
    o = _lib.bestshot_opts(Sz, entries, min_hits, terms)
    cap = int(o.entries if cap is None else cap)
    sc = np.ascontiguousarray(scores, dtype=np.float32).reshape(F, S, rows)
    lm = np.ascontiguousarray(lms, dtype=np.float32).reshape(F, S, rows, 10)
    nf = np.ascontiguousarray(info, dtype=np.int32).reshape(F, S, rows, 3)
    cn = np.ascontiguousarray(counts, dtype=np.int32).reshape(F, S)
    cc = np.full((F, S), rows, np.int32) if chip_counts is None else np.ascontiguousarray(chip_counts, dtype=np.int32).reshape(F, S)
    co = np.ascontiguousarray(collect, dtype=np.uint8).reshape(F)
    kc = max(cap, 0)
    shapes = {"chips": ((F, S, kc, Sz, Sz, 3), np.uint8), "quality": ((F, S, kc), np.int64), "records": ((F, S, kc, 8), np.int32),
              "dets": ((F, S, kc, 5), np.float32), "lms": ((F, S, kc, 10), np.float32)}
    r = {k: np.zeros(sh, dt) if out is None or k not in out else np.ascontiguousarray(out[k], dtype=dt).reshape(sh) for k, (sh, dt) in shapes.items()}
    for k in ("counts", "pending", "flags", "offer_flags"):
        r[k] = np.zeros((F, S), np.int32)
    r["offer_quality"] = np.zeros((F, S, rows), np.int64)
    _lib.check(_lib.lib().cf_op_bestshot(device, C.byref(o), S, F, rows, ptr(b), ptr(sc), ptr(lm), ptr(nf), ptr(cn), ptr(cc), ptr(ch), ptr(co), cap,
                                         float(fx), float(fy), ptr(r["chips"]), ptr(r["quality"]), ptr(r["records"]), ptr(r["dets"]), ptr(r["lms"]),
                                         ptr(r["counts"]), ptr(r["pending"]), ptr(r["flags"]), ptr(r["offer_flags"]), ptr(r["offer_quality"])), op=True)
    return r


def ctdet_decode(heat, wh, reg=None, K=100, lm=None, device=0):
    """ctdet_decode (centerface_ext.py:52-82): (dets [B,K,6], lms [B,K,10]|None, inds [B,K] int64)."""
    heat, wh, reg, lm = f32(heat), f32(wh), f32(reg), f32(lm)
    B, _, h, w = heat.shape
    dets = np.empty((B, K, 6), np.float32)
    lms = np.empty((B, K, 10), np.float32) if lm is not None else None
    inds = np.empty((B, K), np.int64)
    _lib.check(_lib.lib().cf_op_ctdet_decode(device, ptr(heat), ptr(wh), ptr(reg), ptr(lm), B, h, w, int(K),
                                             ptr(dets), ptr(lms), ptr(inds)), op=True)
    return dets, lms, inds
