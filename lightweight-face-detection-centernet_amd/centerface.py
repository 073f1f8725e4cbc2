"""Drop-in host API: the reference's ``centerface.py`` surface on top of libcenterface_hip.so.

``CenterFace(height, width, landmarks=True)`` / ``__call__(img, threshold)`` / ``transform`` /
``decode`` / ``nms`` keep the reference's names, argument meaning, return types and quirks
(centerface.py:11-151); all arithmetic on the hot path runs in hand-written HIP kernels behind the
C ABI (``include/centerface_hip.h``).  This module only marshals numpy arrays; there is no CPU
compute fallback -- if the library is absent every entry point raises.

Additions over the reference (keyword-only, defaults reproduce the reference):
``weights=`` (checkpoint path or state_dict; default: deterministic synthetic weights because the
reference's ``weight/model_epoch_100.pt`` is not distributed), ``dtype=`` ('fp32' parity mode or
'bf16' throughput mode), ``device=``, ``max_batch=``, ``collapse_heads=``; methods ``forward``,
``detect_batch``, ``decode_topk`` (the ``ctdet_decode`` path of centerface_ext.py:52-82).
"""
import bisect
import collections
import contextlib
import ctypes as C
import os
import threading
import types
import weakref

import numpy as np

from . import _lib
from . import weights as _weights

_DTYPES = {"fp32": _lib.CF_F32, "float32": _lib.CF_F32, "f32": _lib.CF_F32,
           "bf16": _lib.CF_BF16, "bfloat16": _lib.CF_BF16,
           # tolerance mode: fp32 storage, split-bf16 ("bf16x3") GEMM products -- within 1e-3 of the reference like "fp32"
           "fp32_split": _lib.CF_F32_SPLIT, "bf16x3": _lib.CF_F32_SPLIT}


def _grown(cap, run):
    """``run(cap)`` fills buffers of ``cap`` rows and returns (result, rows wanted): the result of the first run whose buffers held all
    it wanted -- when more rows survive than there is room for, the reference keeps them all, so the run is repeated with that many."""
    while True:
        res, want = run(cap)
        if want <= cap:
            return res
        cap = want


class Engine(object):
    """One cf_ctx: one GPU, one stream, fixed (H, W), batch up to ``max_batch``."""

    def __init__(self, height, width, max_batch=1, dtype="fp32", device=0, weights=None,
                 collapse_heads=None, fuse=True, graph=True, uphead=True, neck=True, decode_stream=True, high_priority_streams=False,
                 flip_test=False):
        """``flip_test=True``: CenterNet's flip test (``cf_set_flip_test``): every forward runs the batch and its mirror as one batch
        of 2B and the heads are merged on the device before anything reads them -- about one forward at 2B instead of one at B.  The
        context is created with room for ``2 * max_batch`` images; ``max_batch`` stays the caller's number.  No accuracy claim is made."""
        L = _lib.lib()
        if dtype not in _DTYPES:
            raise ValueError("dtype must be one of %s" % sorted(_DTYPES))
        self.H, self.W, self.max_batch, self.device = int(height), int(width), int(max_batch), int(device)
        self.h, self.w = self.H // 4, self.W // 4
        self.dtype = dtype
        if collapse_heads is None:
            # the head pair conv3x3+b -> conv1x1+b is linear (model/centernet.py:249-256): folding it (in float64)
            # into one 3x3 24->15 conv is exact algebra and 6x fewer flops -- the default in both modes; pass
            # collapse_heads=False for the two-stage kernel that keeps the reference's operation order
            collapse_heads = True
        flags = ((_lib.CF_FLAG_COLLAPSE_HEADS if collapse_heads else 0) | (0 if fuse else _lib.CF_FLAG_NO_FUSE)
                 | (0 if graph else _lib.CF_FLAG_NO_GRAPH) | (0 if uphead else _lib.CF_FLAG_NO_UPHEAD)
                 | (0 if neck else _lib.CF_FLAG_NO_NECK) | (0 if decode_stream else _lib.CF_FLAG_NO_DECODE_STREAM)
                 | (_lib.CF_FLAG_STREAM_HIGH if high_priority_streams else 0))
        handle = C.c_void_p()
        self._flip_room, self._flip = bool(flip_test), False
        _lib.check(L.cf_create(self.device, self.max_batch * (2 if self._flip_room else 1), self.H, self.W, _DTYPES[dtype], flags, C.byref(handle)))
        self._h = handle
        self._L = L
        if self._flip_room:
            self.set_flip_test(True)
        # what the last forward was: its batch (last_B), (frames, tiles per frame) when it was tiled, the batches waiting in an upload or
        # in a lane, the rows the last decode or merge kept (the align forms size their buffers from it), the host arrays kept alive
        self._last = types.SimpleNamespace(B=0, tiles=None, uploaded_B=0, lane_B=0, kept=0, keep=None)
        if weights is None:
            weights = _weights.synthetic_state_dict(0)
        elif isinstance(weights, str):
            weights = _weights.load_checkpoint(weights)
        self.load_state_dict(weights)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.cf_synchronize(self._h)
            for p in getattr(self, "_pinned", []):
                self._L.cf_host_free(self._h, p)
            self._pinned = []
            self._L.cf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, code):
        _lib.check(code, self._h)

    @property
    def last_B(self):
        """The batch of the last forward (tile images after ``forward_tiles_enqueue``)."""
        return self._last.B

    @last_B.setter
    def last_B(self, B):
        self._last.B, self._last.tiles = B, None          # (forward_tiles_enqueue sets the tiles again behind this)

    def load_state_dict(self, sd):
        """Strict load (centerface.py:24)."""
        sd = _weights.validate_state_dict(sd)
        descs = (_lib.TensorDesc * len(sd))()
        keep = []
        for i, (k, v) in enumerate(sd.items()):
            name = k.encode()
            keep.append((name, v))
            descs[i].name = name
            descs[i].data = v.ctypes.data
            descs[i].ndim = v.ndim
            for j, d in enumerate(v.shape):
                descs[i].dims[j] = d
            descs[i].dtype = 1 if v.dtype == np.int64 else 0
        self._chk(self._L.cf_load_weights(self._h, descs, len(sd)))

    # -- forward ----------------------------------------------------------------------------
    def forward_enqueue(self, x, on_device=False, B=None, in_format=None):
        """Enqueue one forward.  ``x``: uint8 [B,H,W,3] BGR or float32 [B,3,H,W] numpy array, or an
        int device pointer with ``on_device=True`` (then ``B`` and ``in_format`` are required)."""
        if on_device:
            p = C.c_void_p(int(x))
        else:
            x = np.ascontiguousarray(x)
            if x.dtype == np.uint8:
                if x.ndim != 4 or x.shape[1:] != (self.H, self.W, 3):
                    raise ValueError("uint8 input must be [B,%d,%d,3], got %s" % (self.H, self.W, x.shape))
                in_format = _lib.CF_IN_U8_HWC_BGR
            else:
                x = np.ascontiguousarray(x, dtype=np.float32)
                if x.ndim != 4 or x.shape[1:] != (3, self.H, self.W):
                    raise ValueError("float input must be [B,3,%d,%d], got %s" % (self.H, self.W, x.shape))
                in_format = _lib.CF_IN_F32_NCHW
            B = x.shape[0]
            self._last.keep = x
            p = _lib.ptr(x)
        self._chk(self._L.cf_forward(self._h, p, int(in_format), 1 if on_device else 0, int(B)))
        self.last_B = int(B)

    def forward_lanes_enqueue(self, prev, x, B, in_format=None):
        """Two-lane schedule (``cf_forward_lanes``; EXPERIMENTS BUILD of the library only -- ``make -C csrc EXP=1`` +
        ``CF_LIB=.../libcenterface_hip_exp.so``; measured slower than EngineRing): enqueue the front of a new batch (device pointer ``x``) on this
        engine and the back half of the batch pending on ``prev`` (another Engine of the same device, or None) underneath its
        mid-size blocks.  Afterwards ``prev`` holds a decodable result; this engine does not until it has been ``prev`` of a
        later call or ``forward_lanes_flush()`` was called."""
        fmt = _lib.CF_IN_U8_HWC_BGR if in_format is None else int(in_format)
        if not hasattr(self._L, "cf_forward_lanes"):
            raise RuntimeError("cf_forward_lanes exists only in an experiments build of the library (make -C csrc EXP=1)")
        self._chk(self._L.cf_forward_lanes(self._h, prev._h if prev is not None else None, C.c_void_p(int(x)), fmt, 1, int(B)))
        self.last_B = 0
        if prev is not None and prev._last.lane_B:
            prev.last_B, prev._last.lane_B = prev._last.lane_B, 0
        self._last.lane_B = int(B)

    def forward_lanes_flush(self):
        self._chk(self._L.cf_forward_lanes_flush(self._h))
        if self._last.lane_B:
            self.last_B, self._last.lane_B = self._last.lane_B, 0

    def forward_resized_enqueue(self, imgs_u8):
        """cv2.resize + forward (centerface.py:30-41): uint8 [B,h,w,3] BGR images of any (common) size are
        stretch-resized on the device to (H, W) and fed to the network."""
        x = np.ascontiguousarray(imgs_u8, dtype=np.uint8)
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError("images must be uint8 [B,h,w,3], got %s" % (x.shape,))
        self._last.keep = x
        self._chk(self._L.cf_forward_resized(self._h, _lib.ptr(x), 0, x.shape[0], x.shape[1], x.shape[2]))
        self.last_B = x.shape[0]

    def forward_yuv_enqueue(self, frames, fmt="nv12", *, on_device=False, h=None, w=None, y_pitch=None, c_pitch=None):
        """4:2:0 video frames -> BGR on the device -> forward (``cf_forward_yuv``): the same results as the frames'
        ``cv2.cvtColor(frame, cv2.COLOR_YUV2BGR_<fmt>)`` through ``forward_enqueue`` (or ``forward_resized_enqueue`` when (h, w) is
        not the network size), at half the bytes of BGR over the link.  ``fmt``: 'nv12', 'nv21', 'i420' ('yuv420p') or 'yv12'.
        ``frames``: uint8 [B, h*3//2, w] (OpenCV's single-buffer layout: one DMA), or a list of [h*3//2, w] arrays of one size (one
        descriptor per frame, no host stacking; page-locked arrays -- ``pinned_empty`` -- are DMA'd directly).  ``on_device=True``:
        a list of (y, c0, c1) device addresses, chroma planes in the format's order (c1 None for NV12 / NV21), with ``h``, ``w`` and
        the row pitches in bytes (default: dense rows; addresses and pitches multiples of 4)."""
        f = _lib.yuv_format(fmt)
        if on_device:
            tab, B, h, w, y_pitch, cp = _lib.device_input_planes("forward_yuv_enqueue", frames, f, h, w, y_pitch, c_pitch)
        else:
            if isinstance(frames, np.ndarray):
                arrs = np.ascontiguousarray(frames)
                if arrs.dtype != np.uint8 or arrs.ndim != 3:
                    raise ValueError("frames must be uint8 [B, h*3//2, w], got %s %s" % (arrs.dtype, arrs.shape))
                shp = arrs.shape[1:]
            else:
                arrs = [np.asarray(a) for a in frames]
                if not arrs:
                    raise ValueError("forward_yuv_enqueue needs at least one frame")
                shp = arrs[0].shape
                for a in arrs:
                    if a.dtype != np.uint8 or a.ndim != 2 or a.shape != shp:
                        raise ValueError("frames must be uint8 [h*3//2, w] arrays of one size, got %s %s (first: %s)" % (a.dtype, a.shape, shp))
                arrs = [a if a.flags["C_CONTIGUOUS"] else np.ascontiguousarray(a) for a in arrs]
            if (shp[0] * 2 // 3) * 3 // 2 != shp[0] or (h is not None and int(h) != shp[0] * 2 // 3) or (w is not None and int(w) != shp[1]):
                raise ValueError("a 4:2:0 frame of h x w is [h*3//2, w] with h even; got %s (h=%s, w=%s)" % (shp, h, w))
            tab, h, w, cp = _lib.dense_planes(f, arrs)
            if (y_pitch is not None and int(y_pitch) != w) or (c_pitch is not None and int(c_pitch) != cp):
                raise ValueError("host frames are dense [h*3//2, w] arrays: y_pitch = w, c_pitch = the chroma row")
            B, self._last.keep = len(arrs), arrs
        self._chk(self._L.cf_forward_yuv(self._h, f, tab, 1 if on_device else 0, B, h, w, w if y_pitch is None else int(y_pitch),
                                         cp if c_pitch is None else int(c_pitch)))
        self.last_B = B

    def forward_images_enqueue(self, images, upload_only=False):
        """The batch as a LIST of uint8 [h,w,3] BGR arrays of one common size (``cf_forward_images``): one asynchronous DMA per
        image, resize on the device when (h, w) is not the network size.  With page-locked arrays (``pinned_empty`` / ``pin``)
        nothing is copied on the host."""
        arrs = [np.asarray(im) for im in images]
        if not arrs:
            raise ValueError("forward_images_enqueue needs at least one image")
        shp = arrs[0].shape
        for a in arrs:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape != shp or a.shape[2] != 3:
                raise ValueError("images must be uint8 [h,w,3] arrays of one common size, got %s %s (first: %s)" % (a.dtype, a.shape, shp))
        arrs = [a if a.flags["C_CONTIGUOUS"] else np.ascontiguousarray(a) for a in arrs]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        self._last.keep = arrs
        self._chk((self._L.cf_upload_images if upload_only else self._L.cf_forward_images)(self._h, ptrs, len(arrs), int(shp[0]), int(shp[1])))
        if upload_only:
            self._last.uploaded_B = len(arrs)
        else:
            self.last_B = len(arrs)

    def _upload_addrs(self, addrs, h, w, keep):
        """``upload_images`` for callers that have validated the batch already (CenterFaceBuckets: one raw size per chunk, page-locked
        uint8 arrays): the host addresses go straight into the pointer table."""
        self._last.keep = keep
        self._chk(self._L.cf_upload_images(self._h, (C.c_void_p * len(addrs))(*addrs), len(addrs), int(h), int(w)))
        self._last.uploaded_B = len(addrs)

    def upload_images(self, images):
        """First half of ``forward_images_enqueue`` (``cf_upload_images``): only the host -> device copies are enqueued."""
        self.forward_images_enqueue(images, upload_only=True)

    def forward_uploaded(self):
        """Second half (``cf_forward_uploaded``): resize + forward on what the last ``upload_images`` brought over."""
        self._chk(self._L.cf_forward_uploaded(self._h))
        self.last_B = self._last.uploaded_B

    def set_rescale(self, scale_h=0.0, scale_w=0.0):
        """centerface.py:55-62 on the device (``cf_set_rescale``): the threshold decodes of this engine return
        ``x // scale_w``, ``y // scale_h``; (0, 0) = off."""
        self._chk(self._L.cf_set_rescale(self._h, float(scale_h), float(scale_w)))

    @property
    def flip_test(self):
        """Whether the forwards of this engine run the flip test (``set_flip_test``)."""
        return self._flip

    def set_flip_test(self, on):
        """Switch CenterNet's flip test on or off for the forwards from now on (``cf_set_flip_test``); the results of the last forward
        stay.  Only an engine built with ``flip_test=True`` has the room for the mirrored half."""
        if not self._flip_room:
            raise ValueError("set_flip_test needs an engine built with flip_test=True (its context holds 2 * max_batch images)")
        self._chk(self._L.cf_set_flip_test(self._h, 1 if on else 0))
        self._flip = bool(on)

    def resized_input(self):
        """The uint8 [B,H,W,3] BGR batch the network read in the last forward_resized_enqueue / forward_yuv_enqueue (for tests)."""
        out = np.empty((self.last_B, self.H, self.W, 3), np.uint8)
        self._chk(self._L.cf_get_resized_input(self._h, _lib.ptr(out), self.last_B))
        return out

    def synchronize(self):
        self._chk(self._L.cf_synchronize(self._h))

    def heads(self, sigmoid_hm=False):
        """The four head maps of the last forward as NCHW float32 (model/centernet.py:277-280)."""
        B, h, w = self.last_B, self.h, self.w
        out = {"hm": np.empty((B, 1, h, w), np.float32), "wh": np.empty((B, 2, h, w), np.float32),
               "lm": np.empty((B, 10, h, w), np.float32), "reg": np.empty((B, 2, h, w), np.float32)}
        sg = np.empty((B, 1, h, w), np.float32) if sigmoid_hm else None
        self._chk(self._L.cf_get_heads(self._h, _lib.ptr(out["hm"]), _lib.ptr(out["wh"]), _lib.ptr(out["lm"]),
                                       _lib.ptr(out["reg"]), _lib.ptr(sg)))
        if sigmoid_hm:
            out["hm_sigmoid"] = sg
        return out

    def forward(self, x):
        """net(x)[0] (centerface.py:41): dict of hm (raw logits), wh, lm, reg."""
        self.forward_enqueue(x)
        return self.heads()

    # -- decode -----------------------------------------------------------------------------
    def decode_topk(self, K=100, use_reg=True, landmarks=True, post=None):
        """ctdet_decode on the last forward's heads: (dets [B,K,6], lms [B,K,10] | None, inds [B,K]).
        ``post=(c, s)`` (centers [B,2], scales [B] or [B,2]) additionally applies ctdet_post_process's
        coordinate mapping (utils/post_process.py:83-90) inside the decode kernel."""
        B = self.last_B
        dets = np.empty((B, K, 6), np.float32)
        lms = np.empty((B, K, 10), np.float32) if landmarks else None
        inds = np.empty((B, K), np.int64)
        if post is None:
            self._chk(self._L.cf_decode_topk(self._h, int(K), 1 if use_reg else 0, _lib.ptr(dets), _lib.ptr(lms),
                                             _lib.ptr(inds), 0))
        else:
            c = np.ascontiguousarray(np.asarray(post[0], np.float32).reshape(B, 2))
            s = np.asarray(post[1], np.float32)
            s = np.ascontiguousarray(np.repeat(s.reshape(B, 1), 2, axis=1) if s.size == B else s.reshape(B, 2))
            self._chk(self._L.cf_decode_topk_post(self._h, int(K), 1 if use_reg else 0, _lib.ptr(c), _lib.ptr(s),
                                                  self.w, self.h, _lib.ptr(dets), _lib.ptr(lms), _lib.ptr(inds), 0))
        return dets, lms, inds

    def decode_topk_device(self, K, dets_ptr, lms_ptr=None, inds_ptr=None, use_reg=True):
        """Same, writing into caller-owned DEVICE buffers (asynchronous)."""
        self._chk(self._L.cf_decode_topk(self._h, int(K), 1 if use_reg else 0, C.c_void_p(int(dets_ptr)),
                                         C.c_void_p(int(lms_ptr)) if lms_ptr else None,
                                         C.c_void_p(int(inds_ptr)) if inds_ptr else None, 1))

    def decode_threshold_enqueue(self, score_thresh=0.3, nms_thresh=0.3, max_out=1024, mode="d1", size=None):
        """Enqueue the threshold decode + NMS kernels of the last forward right behind it (no host wait); a following
        ``decode_threshold`` with the same arguments only waits and copies the results out (``cf_decode_threshold_enqueue``)."""
        ih, iw = (self.H, self.W) if size is None else (int(size[0]), int(size[1]))
        self._chk(self._L.cf_decode_threshold_enqueue(self._h, {"d1": 0, "d2": 1}[mode], float(score_thresh), float(nms_thresh), ih, iw, int(max_out)))

    def decode_threshold(self, score_thresh=0.3, nms_thresh=0.3, max_out=1024, mode="d1", size=None):
        """CenterFace.decode + nms on the last forward: list of (boxes [n,5], lms [n,10]) per image.
        mode "d2" = eval_widerface.decode (eval_widerface.py:92-110): threshold honoured, offsets used.
        ``size`` = (h, w) the boxes are clamped to (default: the engine's input size)."""
        ih, iw = (self.H, self.W) if size is None else (int(size[0]), int(size[1]))
        return self._rows(self.last_B, max_out, lambda cap, dets, lms, counts: self._L.cf_decode_threshold_sized(
            self._h, {"d1": 0, "d2": 1}[mode], float(score_thresh), float(nms_thresh), ih, iw, cap, _lib.ptr(dets), _lib.ptr(lms), _lib.ptr(counts)))

    def _rows(self, B, max_out, call):
        """Per-image (dets [n,5], lms [n,10]) of ``call(cap, dets, lms, counts)`` -- the threshold decode or the tile merge -- on host
        buffers of ``max_out`` rows per image, grown until every image's rows fit; remembers how many rows were kept."""
        def run(cap):
            dets, lms, counts = np.empty((B, cap, 5), np.float32), np.empty((B, cap, 10), np.float32), np.empty((B,), np.int32)
            self._chk(call(cap, dets, lms, counts))
            return (dets, lms, counts), int(counts.max(initial=0))
        dets, lms, counts = _grown(int(max_out), run)
        self._last.kept = int(counts.sum())
        return [(dets[b, :counts[b]].copy(), lms[b, :counts[b]].copy()) for b in range(B)]

    # -- aligned face chips -------------------------------------------------------------------
    def align_faces(self, size=112, *, max_faces=None, out="u8", rgb=False, mean=0.0, scale=1.0, template=None, max_per_image=0):
        """Aligned chips of the faces the preceding ``decode_threshold`` kept (``cf_align_faces``): every face is warped from the
        uint8 batch the network read onto ``template`` ([5][2] chip points; default the ArcFace 112 x 112 points times size / 112) by
        the least-squares similarity of its five landmarks -- in network coordinates, whatever ``set_rescale`` says.  Returns
        (chips [N,size,size,3] uint8 BGR, or [N,3,size,size] float32 = ``(u8 - mean) * scale`` with ``out='f32'``; offsets [B+1]:
        the faces of image b are rows offsets[b]:offsets[b+1], in the decode's keep order; matrices [N,6] float64: the 2x3 chip ->
        network-input maps, zero where a face could not be aligned).  ``max_faces`` caps N (offsets[-1] still tells the number
        wanted); by default the buffers are sized from the decode's counts and grown if that was short."""
        o, tm, shape, dtype = _lib.align_opts(size, out, rgb, mean, scale, template, max_per_image)
        return self._chips(self.last_B, shape, dtype, max_faces, lambda chips, mats, offs, cap: self._L.cf_align_faces(
            self._h, C.byref(o), _lib.ptr(chips), _lib.ptr(mats), _lib.ptr(offs), cap, 0))

    def _chips(self, B, shape, dtype, max_faces, call):
        """(chips, offsets, matrices) of ``call(chips, mats, offs, cap)``: host buffers for ``max_faces`` faces, or sized from the rows
        the last decode or merge kept and grown once the offsets tell that this was short."""
        def run(cap):
            chips, mats, offs = np.empty((max(cap, 1),) + shape, dtype), np.empty((max(cap, 1), 6), np.float64), np.zeros((B + 1,), np.int32)
            self._chk(call(chips, mats, offs, cap))
            n = min(int(offs[-1]), cap)
            return (chips[:n], offs, mats[:n]), 0 if max_faces is not None else int(offs[-1])
        return _grown(self._last.kept if max_faces is None else int(max_faces), run)

    def align_faces_device(self, chips_ptr, offsets_ptr, cap_faces, matrices_ptr=None, size=112, *, out="u8", rgb=False, mean=0.0,
                           scale=1.0, template=None, max_per_image=0):
        """Same, writing into caller-owned DEVICE buffers (chips for ``cap_faces`` faces, 16-byte aligned; offsets [B+1] int32;
        matrices [cap_faces,6] float64 or None): asynchronous on the engine's main stream, no host read of the counts."""
        o, tm, _, _ = _lib.align_opts(size, out, rgb, mean, scale, template, max_per_image)
        self._chk(self._L.cf_align_faces(self._h, C.byref(o), C.c_void_p(int(chips_ptr)), C.c_void_p(int(matrices_ptr)) if matrices_ptr else None,
                                         C.c_void_p(int(offsets_ptr)), int(cap_faces), 1))      # (the template is read during the call)

    def align_faces_frame(self, frames, fmt="bgr", size=112, *, max_faces=None, out="u8", rgb=False, mean=0.0, scale=1.0, template=None,
                          max_per_image=0):
        """Aligned chips cut from the SOURCE frames (``cf_align_faces_frame``, host form): as ``align_faces``, but every face is sampled
        at the resolution it has in ``frames`` -- host arrays as ``redact_faces`` takes them (BGR uint8 [B,h,w,3], dense 4:2:0 uint8
        [B, h*3//2, w], or per-frame plane tuples of pitched rows), only read -- instead of the network-sized batch.  Behind a plain
        forward the faces are those the preceding ``decode_threshold`` kept, their network-coordinate landmarks mapped to the frame by
        w / W, h / H in float64 (whatever ``set_rescale`` says), B the forward's batch; behind ``forward_tiles_enqueue`` +
        ``merge_tiles`` they are the merged rows, B the number of frames.  Returns (chips, offsets [B+1], matrices [N,6] chip -> frame
        pixel maps)."""
        args, keep = _lib.host_frame_args(frames, fmt, writable=False)
        o, tm, shape, dtype = _lib.align_opts(size, out, rgb, mean, scale, template, max_per_image)
        return self._chips(args[3], shape, dtype, max_faces, lambda chips, mats, offs, cap: self._L.cf_align_faces_frame(
            self._h, C.byref(o), *args, _lib.ptr(chips), _lib.ptr(mats), _lib.ptr(offs), cap, 0))

    def align_faces_frame_device(self, plane_ptrs, fmt, B, h, w, pitch0, pitch1, chips_ptr, offsets_ptr, cap_faces, matrices_ptr=None,
                                 size=112, *, out="u8", rgb=False, mean=0.0, scale=1.0, template=None, max_per_image=0):
        """Same, reading DEVICE planes in place -- a decoder's surfaces: ``plane_ptrs`` = B tuples (p0, p1, p2) of device addresses as
        ``redact_faces_device`` takes them (addresses and pitches multiples of 4) -- and writing caller-owned DEVICE buffers as
        ``align_faces_device`` does.  Asynchronous on the engine's main stream behind the decode or the merge; no count is read on
        the host."""
        args = _lib.device_frame_args("align_faces_frame_device", plane_ptrs, fmt, B, h, w, pitch0, pitch1)
        o, tm, _, _ = _lib.align_opts(size, out, rgb, mean, scale, template, max_per_image)
        self._chk(self._L.cf_align_faces_frame(self._h, C.byref(o), *args, C.c_void_p(int(chips_ptr)), C.c_void_p(int(matrices_ptr)) if matrices_ptr else None,
                                               C.c_void_p(int(offsets_ptr)), int(cap_faces), 1))      # (the template is read during the call)

    # -- face redaction in the source frame ------------------------------------------------------
    def redact_faces(self, frames, fmt="bgr", *, mode="mosaic", shape="ellipse", cell=20, scale=1.3, fill=(0, 0, 0)):
        """Blank or pixelate, in ``frames``, the faces the preceding ``decode_threshold`` kept (``cf_redact_faces``, blocking form): the
        host arrays are copied up, redacted on the device and copied back IN PLACE, and returned.  ``frames``: BGR uint8 [B,h,w,3]
        (``fmt='bgr'``), OpenCV's dense 4:2:0 uint8 [B, h*3//2, w] ('nv12', 'nv21', 'i420', 'yv12'), or a list of per-frame plane tuples
        of 2-D uint8 arrays (pitched rows; chroma planes in the format's order) -- of ANY size: the boxes are taken in network
        coordinates, whatever ``set_rescale`` says, and mapped to the frame by w / W, h / H.  B must be the last forward's batch.
        A face's box is grown about its centre by ``scale``; ``shape`` 'rect' covers it, 'ellipse' the ellipse inscribed in it;
        ``mode`` 'solid' writes ``fill`` (bytes in the frame's channel order), 'mosaic' the mean of the ``cell`` x ``cell`` cell of a
        grid anchored at the frame origin, taken from the untouched frame."""
        return self._cover(self._L.cf_redact_faces, _lib.host_frame_args(frames, fmt), lambda: _lib.redact_opts(mode, shape, cell, scale, fill), frames)

    def redact_faces_device(self, plane_ptrs, fmt, B, h, w, pitch0, pitch1=0, *, mode="mosaic", shape="ellipse", cell=20, scale=1.3,
                            fill=(0, 0, 0)):
        """Same, in place on DEVICE planes -- a decoder's surfaces: ``plane_ptrs`` = B tuples (p0, p1, p2) of device addresses (BGR: p0
        only; NV12 / NV21: Y and the interleaved plane; I420 / YV12: three planes), addresses and pitches multiples of 4.  Asynchronous
        on the engine's main stream behind the decode; no count is read on the host."""
        self._cover(self._L.cf_redact_faces, (_lib.device_frame_args("redact_faces_device", plane_ptrs, fmt, B, h, w, pitch0, pitch1), None),
                    lambda: _lib.redact_opts(mode, shape, cell, scale, fill))

    def _cover(self, fn, frame_args, opts, frames=None):
        """The body of the redact and blur pairs: ``frame_args`` = (the frame arguments, what to keep alive) of the host or the device
        planes, then the options struct of ``opts()``, then the one ABI call; returns ``frames``."""
        o = opts()
        self._chk(fn(self._h, C.byref(o), *frame_args[0]))
        return frames

    def blur_faces(self, frames, fmt="bgr", *, shape="ellipse", radius=0, scale=1.3):
        """Blur, in ``frames``, the faces the preceding ``decode_threshold`` kept (``cf_blur_faces``, blocking form): frames, formats and
        faces as ``redact_faces``; copied up, blurred on the device and copied back IN PLACE, and returned.  A covered sample becomes the
        box * box * box filtered value (width 2r+1 each, sigma about r) of the untouched frame; ``radius`` = r in 1..24, or 0 for a
        per-face r of an eighth of the box's smaller side (at most 24)."""
        return self._cover(self._L.cf_blur_faces, _lib.host_frame_args(frames, fmt), lambda: _lib.blur_opts(shape, radius, scale), frames)

    def blur_faces_device(self, plane_ptrs, fmt, B, h, w, pitch0, pitch1=0, *, shape="ellipse", radius=0, scale=1.3):
        """Same, in place on DEVICE planes as ``redact_faces_device`` takes them: asynchronous on the engine's main stream behind the
        decode; no count is read on the host."""
        self._cover(self._L.cf_blur_faces, (_lib.device_frame_args("blur_faces_device", plane_ptrs, fmt, B, h, w, pitch0, pitch1), None),
                    lambda: _lib.blur_opts(shape, radius, scale))

    def draw_faces(self, frames, fmt="bgr", **options):
        """Draw, in ``frames``, the newest face rows -- those ``redact_faces`` would cover: the preceding ``decode_threshold``'s, the
        merged ones, or the tracked ones behind ``track_update`` -- (``cf_draw_faces``, blocking form): box outlines, landmark dots
        and a numeric label, copied up, painted on the device and copied back IN PLACE, and returned.  Frames and formats as
        ``redact_faces``.  ``options``: those of ``_lib.draw_opts`` -- boxes, landmarks, thickness, radius, label ('none' | 'score' |
        'id': the track id, tracked rows only), label_scale, dash_held, scale, box_color, held_color, lm_color, text_color (bytes in
        the frame's own channel order; ``ops.bgr_to_yuv_color`` converts).  Held tracks are drawn in ``held_color``, dashed, without
        dots.  No state of the engine changes: draw after redact."""
        return self._cover(self._L.cf_draw_faces, _lib.host_frame_args(frames, fmt), lambda: _lib.draw_opts(**options), frames)

    def draw_faces_device(self, plane_ptrs, fmt, B, h, w, pitch0, pitch1=0, **options):
        """Same, in place on DEVICE planes as ``redact_faces_device`` takes them: asynchronous on the engine's main stream behind the
        rows' producer; no count is read on the host."""
        self._cover(self._L.cf_draw_faces, (_lib.device_frame_args("draw_faces_device", plane_ptrs, fmt, B, h, w, pitch0, pitch1), None),
                    lambda: _lib.draw_opts(**options))

    def cover_faces(self, frames, fmt="bgr", **options):
        """``blur_faces`` when ``options`` say ``mode='blur'`` (shape, radius, scale), otherwise ``redact_faces``."""
        kind, kw = _lib.split_redact_options(options)
        return self.blur_faces(frames, fmt, **kw) if kind == "blur" else self.redact_faces(frames, fmt, **kw)

    # -- tiled detection of large frames ---------------------------------------------------------
    def forward_tiles_enqueue(self, frames, rects, fmt="bgr", *, on_device=False, h=None, w=None, pitch0=None, pitch1=None):
        """Cut ``rects`` ([T][4] rows (x0, y0, w, h), all even, inside the frame) out of every frame at native resolution, resize each to
        the network size and run the Bf * T tiles as one batch (``cf_forward_tiles``); image f * T + t is tile t of frame f.  ``frames``:
        host arrays as ``redact_faces`` takes them (BGR uint8 [B,h,w,3], dense 4:2:0 uint8 [B, h*3//2, w], or per-frame plane tuples of
        pitched rows) -- only read -- or, with ``on_device=True``, Bf tuples (p0, p1, p2) of device addresses with ``h``, ``w`` and the
        pitches in bytes (default: dense rows; addresses and pitches multiples of 4), read in place.  A ``decode_threshold`` then gives
        the per-tile results and ``merge_tiles`` the per-frame ones."""
        f = _lib.frame_format(fmt)
        rt, T = _lib.tile_rects(rects)
        if on_device:
            tab, B, h, w, pitch0, pitch1 = _lib.device_input_planes("forward_tiles_enqueue", frames, f, h, w, pitch0, pitch1)
        else:
            tab, B, h, w, pitch0, pitch1, self._last.keep = _lib.frame_planes(frames, fmt, writable=False)
        self._chk(self._L.cf_forward_tiles(self._h, f, tab, 1 if on_device else 0, B, h, w, pitch0, pitch1, rt, T))
        self.last_B = B * T
        self._last.tiles = (B, T)

    def merge_tiles(self, metric="ios", thresh=0.5, edge=2.0, max_out=1024):
        """Per-frame detections of the last tiled forward (``cf_merge_tiles``, host form): the rows the preceding ``decode_threshold``
        kept for every tile -- in network coordinates, whatever ``set_rescale`` says -- are mapped into frame pixels and de-duplicated
        on the device.  A row whose box comes within ``edge`` network pixels of a tile side that is not on the frame border is dropped
        first (a face cut by the seam; the neighbouring tile or the whole-frame tile sees it whole); the others go through greedy NMS
        with ``metric`` 'ios' (intersection over the smaller box) or 'iou' at ``thresh``.  Returns (results, flags): a list of (dets
        [n,5], lms [n,10]) per frame and int32 [Bf], bit 0 set where a tile's decode was truncated by its ``max_out``.  IoS 0.5 and
        edge 2 are this project's defaults, not the reference's."""
        Bf = (self._last.tiles or (1, 1))[0]                             # (without a tiled forward the library refuses: CF_ESTATE)
        o = _lib.merge_opts(metric, thresh, edge)
        flags = np.empty((Bf,), np.int32)
        return self._rows(Bf, max_out, lambda cap, dets, lms, counts: self._L.cf_merge_tiles(
            self._h, C.byref(o), cap, _lib.ptr(dets), _lib.ptr(lms), _lib.ptr(counts), _lib.ptr(flags), 0)), flags

    def merge_tiles_device(self, max_out, dets_ptr=None, lms_ptr=None, counts_ptr=None, flags_ptr=None, *, metric="ios", thresh=0.5, edge=2.0):
        """Same, writing into caller-owned DEVICE buffers (dets [Bf,max_out,5], lms [Bf,max_out,10] float32, counts / flags [Bf] int32;
        any may be None): asynchronous on the engine's main stream behind the decode, no count is read on the host.  The context keeps
        the merged rows either way: a following ``redact_faces`` / ``redact_faces_device`` on the full frames uses them."""
        o = _lib.merge_opts(metric, thresh, edge)
        self._chk(self._L.cf_merge_tiles(self._h, C.byref(o), int(max_out), _lib.vp(dets_ptr), _lib.vp(lms_ptr), _lib.vp(counts_ptr), _lib.vp(flags_ptr), 1))

    # -- multi-scale detection: views of one frame --------------------------------------------------
    def forward_views_enqueue(self, frames, views, fmt="bgr", *, fill=(0, 0, 0), on_device=False, h=None, w=None, pitch0=None, pitch1=None):
        """Run ``views`` ([V][8] rows (sx0, sy0, sw, sh, dx, dy, dw, dh): a source rectangle of the frame, all even, and a content
        rectangle of the canvas; ``ops.view_layout`` makes them) of every frame as one batch of Bf * V canvases (``cf_forward_views``);
        image f * V + v is ``fill`` (B, G, R) with the source of view v of frame f resized into its content rectangle.  ``frames`` and the
        ``on_device`` form as ``forward_tiles_enqueue`` takes them; they are only read.  A ``decode_threshold`` then gives the per-view
        results and ``merge_views`` the per-frame ones.  One view per canvas: a half-size level costs a whole forward; ``forward_packed_enqueue``
        packs several levels and frames into one canvas, and its ``rot=`` is where rotated views live.  No accuracy claim is made: the
        argument is geometric."""
        f = _lib.frame_format(fmt)
        vt, V = _lib.view_table(views)
        fb = _lib.fill_bytes(fill)
        if on_device:
            tab, B, h, w, pitch0, pitch1 = _lib.device_input_planes("forward_views_enqueue", frames, f, h, w, pitch0, pitch1)
        else:
            tab, B, h, w, pitch0, pitch1, self._last.keep = _lib.frame_planes(frames, fmt, writable=False)
        self._chk(self._L.cf_forward_views(self._h, f, tab, 1 if on_device else 0, B, h, w, pitch0, pitch1, vt, V, fb))
        self.last_B = B * V
        self._last.tiles = (B, V)

    def merge_views(self, metric="ios", thresh=0.5, edge=2.0, max_out=1024):
        """Per-frame detections of the last views forward (``cf_merge_views``, host form): the rows the preceding ``decode_threshold``
        kept for every view -- in canvas coordinates, whatever ``set_rescale`` says -- whose centre lies in the view's content and whose
        box stays ``edge`` network pixels clear of a content side that is a seam inside the frame, mapped into frame pixels and
        de-duplicated on the device by greedy NMS with ``metric`` 'ios' or 'iou' at ``thresh``.  Returns (results, flags) as
        ``merge_tiles``.  IoS 0.5 and edge 2 are this project's defaults; nobody has measured them."""
        Bf = (self._last.tiles or (1, 1))[0]                             # (without a views forward the library refuses: CF_ESTATE)
        o = _lib.merge_opts(metric, thresh, edge)
        flags = np.empty((Bf,), np.int32)
        return self._rows(Bf, max_out, lambda cap, dets, lms, counts: self._L.cf_merge_views(
            self._h, C.byref(o), cap, _lib.ptr(dets), _lib.ptr(lms), _lib.ptr(counts), _lib.ptr(flags), 0)), flags

    def merge_views_device(self, max_out, dets_ptr=None, lms_ptr=None, counts_ptr=None, flags_ptr=None, *, metric="ios", thresh=0.5, edge=2.0):
        """Same, writing into caller-owned DEVICE buffers as ``merge_tiles_device``: asynchronous on the engine's main stream behind the
        decode, no count is read on the host.  The context keeps the merged rows either way."""
        o = _lib.merge_opts(metric, thresh, edge)
        self._chk(self._L.cf_merge_views(self._h, C.byref(o), int(max_out), _lib.vp(dets_ptr), _lib.vp(lms_ptr), _lib.vp(counts_ptr), _lib.vp(flags_ptr), 1))

    # -- packed views: several levels and frames share one canvas -----------------------------------
    def forward_packed_enqueue(self, frames, places, n_canvases, fmt="bgr", *, fill=(0, 0, 0), on_device=False, h=None, w=None, pitch0=None,
                               pitch1=None, rot=0):
        """Run ``n_canvases`` canvases that hold the placements ``places`` ([P][10] rows (frame, canvas, sx0, sy0, sw, sh, dx, dy, dw, dh):
        one view of one frame in one canvas; ``ops.pack_views`` makes them) as one batch (``cf_forward_packed``): canvas n is ``fill``
        (B, G, R) and, inside the content of every placement with canvas == n, what ``forward_views_enqueue`` makes of that view of that
        frame, byte for byte.  The contents of one canvas must not overlap (sharing an edge is allowed).  ``frames`` and the ``on_device``
        form as ``forward_views_enqueue`` takes them; they are only read.  A ``decode_threshold`` then gives the per-CANVAS results --
        its NMS and its max_out are shared by the frames on a canvas, and boxes of two frames whose contents share an edge can suppress
        each other there; a gutter keeps them apart -- and ``merge_packed`` the per-frame ones.  ``rot`` 90, 180 or 270
        (``cf_forward_packed_rot``): rotated views -- the clockwise turn that makes the STORED frames upright; the source rectangles are
        then in pixels of the upright view (lay them out with ``ops.view_layout(hu, wu, ...)``), and ``merge_packed`` returns the rows
        in the stored frame's pixels.  One rot per call, no mirrored orientations.  No accuracy claim is made: the argument is
        geometric."""
        f = _lib.frame_format(fmt)
        pt, P = _lib.place_table(places)
        fb = _lib.fill_bytes(fill)
        if on_device:
            tab, B, h, w, pitch0, pitch1 = _lib.device_input_planes("forward_packed_enqueue", frames, f, h, w, pitch0, pitch1)
        else:
            tab, B, h, w, pitch0, pitch1, self._last.keep = _lib.frame_planes(frames, fmt, writable=False)
        if rot:
            self._chk(self._L.cf_forward_packed_rot(self._h, int(rot), f, tab, 1 if on_device else 0, B, h, w, pitch0, pitch1, pt, P, int(n_canvases), fb))
        else:
            self._chk(self._L.cf_forward_packed(self._h, f, tab, 1 if on_device else 0, B, h, w, pitch0, pitch1, pt, P, int(n_canvases), fb))
        self.last_B = int(n_canvases)
        self._last.tiles = (B, 1)

    def merge_packed(self, metric="ios", thresh=0.5, edge=2.0, max_out=1024):
        """Per-frame detections of the last packed forward (``cf_merge_packed``, host form): per frame the rows the preceding
        ``decode_threshold`` kept on the canvas of each of its placements whose centre lies in THAT placement's content (a row centred in
        another frame's content comes out in that frame; one centred in the fill belongs to nobody), by the rules of ``merge_views``,
        mapped into frame pixels and de-duplicated on the device.  Returns (results, flags) as ``merge_views``; flag bit 0: a canvas that
        holds one of the frame's placements had more rows than the decode's max_out."""
        Bf = (self._last.tiles or (1, 1))[0]                             # (without a packed forward the library refuses: CF_ESTATE)
        o = _lib.merge_opts(metric, thresh, edge)
        flags = np.empty((Bf,), np.int32)
        return self._rows(Bf, max_out, lambda cap, dets, lms, counts: self._L.cf_merge_packed(
            self._h, C.byref(o), cap, _lib.ptr(dets), _lib.ptr(lms), _lib.ptr(counts), _lib.ptr(flags), 0)), flags

    def merge_packed_device(self, max_out, dets_ptr=None, lms_ptr=None, counts_ptr=None, flags_ptr=None, *, metric="ios", thresh=0.5, edge=2.0):
        """Same, writing into caller-owned DEVICE buffers as ``merge_views_device``: asynchronous on the engine's main stream behind the
        decode, no count is read on the host.  The context keeps the merged rows either way."""
        o = _lib.merge_opts(metric, thresh, edge)
        self._chk(self._L.cf_merge_packed(self._h, C.byref(o), int(max_out), _lib.vp(dets_ptr), _lib.vp(lms_ptr), _lib.vp(counts_ptr), _lib.vp(flags_ptr), 1))

    # -- aspect-preserving (letterbox) input -------------------------------------------------------
    def forward_fit_enqueue(self, frames, fmt="bgr", *, anchor="center", upscale=True, fill=(0, 0, 0), on_device=False, h=None, w=None,
                            pitch0=None, pitch1=None):
        """Fit every frame into the network's (H, W) canvas with its aspect ratio kept -- resized to (rh, rw) = ``ops.fit_geometry``,
        pasted at the centre (``anchor='topleft'``: at the origin), ``fill`` (B, G, R) around it -- and run the B canvases as one batch
        (``cf_forward_fit``).  ``upscale=False`` leaves a frame that is smaller than the canvas at its size.  ``frames`` and the
        ``on_device`` form as ``forward_tiles_enqueue`` takes them, except that BGR frames may have odd sides; they are only read.  A
        ``decode_threshold`` then gives the rows in canvas coordinates and ``unfit_rows`` those in frame pixels.  No accuracy claim is
        made for letterboxed input: the argument is geometric (the reference's data pipeline fits and pads, dataset/dataset.py:114-134)."""
        f = _lib.frame_format(fmt)
        o = _lib.fit_opts(anchor, upscale, fill)
        if on_device:
            tab, B, h, w, pitch0, pitch1 = _lib.device_input_planes("forward_fit_enqueue", frames, f, h, w, pitch0, pitch1)
        else:
            tab, B, h, w, pitch0, pitch1, self._last.keep = _lib.frame_planes(frames, fmt, writable=False)
        self._chk(self._L.cf_forward_fit(self._h, C.byref(o), f, tab, 1 if on_device else 0, B, h, w, pitch0, pitch1))
        self.last_B = B

    def forward_rot_enqueue(self, frames, fmt="bgr", rot=0, *, fit=None, on_device=False, h=None, w=None, pitch0=None, pitch1=None):
        """Detect upright in frames that are STORED turned (a corridor-mode camera, phone video whose turn lives in the container's
        display matrix): fill the network's canvases from the upright view of every frame and run them as one batch
        (``cf_forward_rot``).  ``rot``: the clockwise turn -- 0, 90, 180 or 270 -- that makes the stored frame upright
        (``cv2.ROTATE_90_CLOCKWISE`` for 90).  ``fit`` None: the upright view is stretched to (H, W) like ``forward_resized``; True, or a
        dict with anchor, upscale and / or fill: it is fitted like ``forward_fit_enqueue``.  ``frames`` and the ``on_device`` form as
        there; they are only read.  A ``decode_threshold`` then gives the rows in canvas coordinates and ``unfit_rows`` those in the
        pixels of the STORED frame, where ``redact_faces``, ``draw_faces``, ``align_faces_frame`` and the tracker take them.  One ``rot``
        per call; mirrored orientations are not covered; a single-view path: tiles and levels of a rotated source, a rotated tiled forward
        among them, live in ``forward_packed_enqueue(rot=)``.  No accuracy claim is made: the argument is geometric."""
        f = _lib.frame_format(fmt)
        o = _lib.rot_opts(rot, fit)
        if on_device:
            tab, B, h, w, pitch0, pitch1 = _lib.device_input_planes("forward_rot_enqueue", frames, f, h, w, pitch0, pitch1)
        else:
            tab, B, h, w, pitch0, pitch1, self._last.keep = _lib.frame_planes(frames, fmt, writable=False)
        self._chk(self._L.cf_forward_rot(self._h, C.byref(o), f, tab, 1 if on_device else 0, B, h, w, pitch0, pitch1))
        self.last_B = B

    def unfit_rows(self, max_out=1024):
        """Per-frame detections of the last fitted forward in frame pixels (``cf_unfit_rows``, host form): the rows the preceding
        ``decode_threshold`` kept -- in canvas coordinates, whatever ``set_rescale`` says -- whose corners are finite and whose centre
        lies in the content, mapped back on the device, in the decode's order.  Returns (results, flags): a list of (dets [n,5], lms
        [n,10]) per frame and int32 [B], bit 0 set where the decode was truncated by its ``max_out``.  Until the next forward or decode,
        ``track_update``, ``redact_faces`` / ``blur_faces`` / ``draw_faces`` / ``align_faces_frame`` of this engine use these rows."""
        B = self.last_B
        flags = np.empty((B,), np.int32)
        return self._rows(B, max_out, lambda cap, dets, lms, counts: self._L.cf_unfit_rows(
            self._h, cap, _lib.ptr(dets), _lib.ptr(lms), _lib.ptr(counts), _lib.ptr(flags), 0)), flags

    def unfit_rows_device(self, max_out, dets_ptr=None, lms_ptr=None, counts_ptr=None, flags_ptr=None):
        """Same, writing into caller-owned DEVICE buffers (dets [B,max_out,5], lms [B,max_out,10] float32, counts / flags [B] int32; any
        may be None): asynchronous on the engine's main stream behind the decode, no count is read on the host.  The context keeps the
        mapped rows either way."""
        self._chk(self._L.cf_unfit_rows(self._h, int(max_out), _lib.vp(dets_ptr), _lib.vp(lms_ptr), _lib.vp(counts_ptr), _lib.vp(flags_ptr), 1))

    # -- face tracks across video frames -----------------------------------------------------------
    def track_update(self, tracker, stream0=0):
        """Advance ``tracker`` by one frame with the rows the preceding ``decode_threshold`` kept -- after ``forward_tiles_enqueue``, the
        rows of the preceding ``merge_tiles`` -- (``cf_track_update``, host form): image b is the next frame of stream ``stream0 + b``.
        Returns (results, flags): per image (dets [n,5], lms [n,10], ids [n], hits [n], misses [n]) -- every detection of the frame plus
        the tracks held through a dropout (``misses`` > 0: box grown by ``hold_grow`` per missed frame, last-seen landmarks), in slot
        order -- and int32 [B], bit 0 set where a new face found no free slot and was dropped.  Until the next forward, decode or
        merge, ``redact_faces`` / ``blur_faces`` / ``align_faces_frame`` of this engine use these rows."""
        B = self._last.tiles[0] if self._last.tiles else self.last_B
        M = tracker.max_tracks
        dets = np.empty((B, M, 5), np.float32)
        lms = np.empty((B, M, 10), np.float32)
        info = np.empty((B, M, 3), np.int32)
        counts = np.zeros((B,), np.int32)
        flags = np.zeros((B,), np.int32)
        self._chk(self._L.cf_track_update(self._h, tracker._handle(self), int(stream0), _lib.ptr(dets), _lib.ptr(lms), _lib.ptr(info),
                                          _lib.ptr(counts), _lib.ptr(flags), 0))
        return [(dets[b, :counts[b]].copy(), lms[b, :counts[b]].copy(), info[b, :counts[b], 0].copy(), info[b, :counts[b], 1].copy(),
                 info[b, :counts[b], 2].copy()) for b in range(B)], flags

    def track_update_device(self, tracker, stream0=0, dets_ptr=None, lms_ptr=None, info_ptr=None, counts_ptr=None, flags_ptr=None):
        """Same, writing into caller-owned DEVICE buffers (dets [B,max_tracks,5], lms [B,max_tracks,10] float32, info [B,max_tracks,3],
        counts / flags [B] int32; any may be None): asynchronous on the engine's main stream behind the decode or the merge, nothing is
        read on the host.  The context keeps the tracked rows either way."""
        self._chk(self._L.cf_track_update(self._h, tracker._handle(self), int(stream0), _lib.vp(dets_ptr), _lib.vp(lms_ptr), _lib.vp(info_ptr), _lib.vp(counts_ptr),
                                          _lib.vp(flags_ptr), 1))

    def track_follow(self, frames, fmt, tracker, stream0=0, *, search=4, max_sad=4096):
        """Follow the faces ``tracker`` holds into ``frames`` by block matching, WITHOUT a forward (``cf_track_follow``, host form): frame b
        is the current frame of stream ``stream0 + b`` -- host frames as ``redact_faces`` takes them, only read, of any size when the
        tracker's rows are in network coordinates (mapped by w / W, h / H), of the tiled frames' size when they are in frame pixels.  A
        slot that an update has just filled or matched learns a 16 x 16 cell template of its face; any other is searched within
        ``search`` cells of where it was and, with a best sum of absolute differences of at most ``max_sad``, moved there -- box and
        landmarks, in the tracker's state.  ``search=4`` and ``max_sad=4096`` are this project's choices; no accuracy claim is made for
        them.  Needs one ``track_update`` on the tracker before the first call, and none on this engine.  Returns (dets [B,M,5], lms
        [B,M,10], info [B,M,3] = id, hits, misses, counts [B], moves [B,M,4] = px, py, SAD, code (``_lib.CF_FOLLOW_*``)), M =
        ``max_tracks``, rows below counts[b] valid.  Until the next forward, decode, merge or update on this engine, ``redact_faces`` /
        ``blur_faces`` / ``align_faces_frame`` / ``draw_faces`` use these rows."""
        args, keep = _lib.host_frame_args(frames, fmt, writable=False)
        f, tab, dev, B, h, w, pitch0, pitch1 = args
        M = tracker.max_tracks
        dets, lms = np.zeros((B, M, 5), np.float32), np.zeros((B, M, 10), np.float32)
        info, moves, counts = np.zeros((B, M, 3), np.int32), np.zeros((B, M, 4), np.int32), np.zeros((B,), np.int32)
        o = _lib.follow_opts(search, max_sad)
        self._chk(self._L.cf_track_follow(self._h, tracker._handle(self), int(stream0), B, C.byref(o), f, tab, dev, h, w, pitch0, pitch1,
                                          _lib.ptr(dets), _lib.ptr(lms), _lib.ptr(info), _lib.ptr(counts), _lib.ptr(moves), 0))
        return dets, lms, info, counts, moves

    def track_follow_device(self, plane_ptrs, fmt, B, h, w, pitch0, pitch1, tracker, stream0=0, *, search=4, max_sad=4096, dets_ptr=None,
                            lms_ptr=None, info_ptr=None, counts_ptr=None, moves_ptr=None):
        """Same, reading DEVICE planes in place as ``redact_faces_device`` takes them and writing caller-owned DEVICE buffers (any may
        be None): asynchronous on the engine's main stream behind the tracker's last update or follow; nothing is read on the host.
        The context keeps the followed rows either way."""
        f, tab, dev, B, h, w, pitch0, pitch1 = _lib.device_frame_args("track_follow_device", plane_ptrs, fmt, B, h, w, pitch0, pitch1)
        o = _lib.follow_opts(search, max_sad)
        self._chk(self._L.cf_track_follow(self._h, tracker._handle(self), int(stream0), B, C.byref(o), f, tab, dev, h, w, pitch0, pitch1,
                                          _lib.vp(dets_ptr), _lib.vp(lms_ptr), _lib.vp(info_ptr), _lib.vp(counts_ptr), _lib.vp(moves_ptr), 1))

    # -- scene cuts --------------------------------------------------------------------------------
    def scene_check(self, frames, fmt, scenes, tracker=None, stream0=0, *, codes=True, out_ptr=None):
        """Does frame b continue stream ``stream0 + b`` of ``scenes`` (a ``SceneCuts``)?  (``cf_scene_check``, host form; the statement is
        in ``include/centerface_hip.h``.)  Host frames as ``redact_faces`` takes them, only read, of an even size of at least 8 x 8; no
        forward is needed and the rows this engine holds stay as they are.  With ``tracker`` the tracks of every stream that is CUT are
        freed on the device, as ``Tracker.reset`` frees them: CALL IT BEFORE the frame's ``track_update`` or ``track_follow``.  Returns
        int32 [B, 4] = code (``_lib.CF_SCENE_FIRST`` / ``_SAME`` / ``_CUT``), hist (per mille of pixels that changed luma bin), grid (sum
        of the 64 cell-mean differences), run (SAME checks in a row) and blocks; ``codes=False`` reads nothing back and returns None.
        A flash is reported as a cut, a dissolve is not one cut; the thresholds are this project's choices, no accuracy claim is made.
        ``out_ptr``: a DEVICE int32 [B, 4] buffer that takes the codes instead (for ``lookback_step``); nothing is read back, returns None."""
        args, keep = _lib.host_frame_args(frames, fmt, writable=False)
        f, tab, dev, B, h, w, pitch0, pitch1 = args
        out = np.zeros((B, 4), np.int32) if codes and not out_ptr else None
        self._chk(self._L.cf_scene_check(self._h, scenes._handle(self), tracker._handle(self) if tracker is not None else None, int(stream0), B, f, tab,
                                         dev, h, w, pitch0, pitch1, C.c_void_p(int(out_ptr)) if out_ptr else _lib.ptr(out), 1 if out_ptr else 0))
        del keep
        return out

    def scene_check_device(self, plane_ptrs, fmt, B, h, w, pitch0, pitch1, scenes, tracker=None, stream0=0, out_ptr=None):
        """Same, reading DEVICE planes in place as ``redact_faces_device`` takes them and writing the caller-owned DEVICE buffer ``out_ptr``
        (int32 [B, 4], or None): asynchronous on the engine's main stream behind the last check of ``scenes`` and the last update, follow
        or reset of ``tracker``; nothing is read on the host -- the cut is decided and the tracks are freed by the kernel."""
        f, tab, dev, B, h, w, pitch0, pitch1 = _lib.device_frame_args("scene_check_device", plane_ptrs, fmt, B, h, w, pitch0, pitch1)
        self._chk(self._L.cf_scene_check(self._h, scenes._handle(self), tracker._handle(self) if tracker is not None else None, int(stream0), B, f, tab,
                                         dev, h, w, pitch0, pitch1, C.c_void_p(int(out_ptr)) if out_ptr else None, 1))

    # -- lookback: cover faces in the frames before their first detection ---------------------------
    def lookback_step(self, lb, stream0=0, B=None, push=True, scene=None):
        """One step of the streams ``stream0 .. stream0 + B - 1`` of ``lb`` (a ``Lookback``; default: all from ``stream0`` on)
        (``cf_lookback_step``, host form; the statement is in ``include/centerface_hip.h``).  ``push=True``: the tracked rows this engine
        holds behind a ``track_update`` or ``track_follow`` of B images enter the delay line, image b as the next frame of stream
        ``stream0 + b``; ``scene``: the int32 [B, 4] codes ``scene_check`` returned for these frames -- or the address of a DEVICE buffer
        it wrote them to --, or None.  ``push=False``: a drain, for the end of the video; no forward is needed.  Returns (dets [B,R,5],
        lms [B,R,10], info [B,R,3] = id, hits, misses, counts [B], state [B,4] = seq, own rows, back-filled rows, flags), R = ``lb.rows``,
        rows below counts[b] valid: the tracked rows of the frame ``depth`` steps back plus the first boxes of the tracks born since (hits
        0, misses = the distance, the box grown by ``grow`` per frame).  state[b, 0] == -1: the stream is still warming up (or drained)
        and nothing is due.  Until the next forward, decode, merge, update or follow on this engine ``redact_faces`` / ``blur_faces`` /
        ``draw_faces`` / ``align_faces_frame`` use these rows: GIVE THEM THE FRAMES OF ``depth`` STEPS AGO."""
        B = lb.streams - int(stream0) if B is None else int(B)
        n, R = max(B, 0), lb.rows
        dets, lms, info = np.zeros((n, R, 5), np.float32), np.zeros((n, R, 10), np.float32), np.zeros((n, R, 3), np.int32)
        counts, state = np.zeros((n,), np.int32), np.zeros((n, 4), np.int32)
        on_dev = scene is not None and not isinstance(scene, np.ndarray)
        sc = C.c_void_p(int(scene)) if on_dev else _lib.ptr(None if scene is None else np.ascontiguousarray(scene, dtype=np.int32).reshape(n, 4))
        self._chk(self._L.cf_lookback_step(self._h, lb._handle(self), int(stream0), B, 1 if push else 0, sc, 1 if on_dev else 0, _lib.ptr(dets),
                                           _lib.ptr(lms), _lib.ptr(info), _lib.ptr(counts), _lib.ptr(state), 0))
        return dets, lms, info, counts, state

    def lookback_step_device(self, lb, stream0, B, push=True, scene_ptr=None, dets_ptr=None, lms_ptr=None, info_ptr=None, counts_ptr=None,
                             state_ptr=None):
        """Same, reading the scene codes from the DEVICE buffer ``scene_check_device`` wrote (or None) and writing caller-owned DEVICE
        buffers (dets [B,R,5], lms [B,R,10] float32, info [B,R,3], counts [B], state [B,4] int32; any may be None): asynchronous on the
        engine's main stream behind the last step of ``lb``; no row, count or code is read on the host.  The context keeps the lookback
        rows either way."""
        self._chk(self._L.cf_lookback_step(self._h, lb._handle(self), int(stream0), int(B), 1 if push else 0, _lib.vp(scene_ptr), 1, _lib.vp(dets_ptr), _lib.vp(lms_ptr),
                                           _lib.vp(info_ptr), _lib.vp(counts_ptr), _lib.vp(state_ptr), 1))

    def _lookback_enable(self, lb, h, w):
        """The library object of ``lb`` -- a ``Lookback`` with ``trace()`` set -- enabled for h x w frames on its first use."""
        handle = lb._handle(self)
        if lb._trace is not None and lb._traced_hw is None:
            o = _lib.follow_opts(**lb._trace)
            self._chk(self._L.cf_lookback_trace_enable(self._h, handle, C.byref(o), int(h), int(w)))
            lb._traced_hw = (int(h), int(w))
        return handle

    def lookback_step_frames(self, lb, frames, fmt, stream0=0, B=None, push=True, scene=None):
        """``lookback_step`` of a ``Lookback`` with ``trace()`` set (``cf_lookback_step_frames``, host form): ``frames`` -- host frames as
        ``track_follow`` takes them, only read -- ARE THE FRAMES THE PUSHED ROWS BELONG TO, frame b that of stream ``stream0 + b``.  Their
        luma is retained on the device, every newborn face is matched backwards through the queued frames' luma, and the back-filled
        boxes and landmarks of the emitted frame stand where the walk found the face (then grown as before).  The first call enables
        the library object for the frames' (h, w); every later push must have that size.  ``push=False``: a drain; ``frames`` may be
        None and ``B`` defaults to all streams from ``stream0`` on.  Returns (dets, lms, info, counts, state) as ``lookback_step`` plus
        moves int32 [B,R,4] = PX, PY, SAD, code (``_lib.CF_FOLLOW_*``) of the back-filled rows, zeros for the frame's own rows."""
        if push:
            args, keep = _lib.host_frame_args(frames, fmt, writable=False)
            f, tab, dev, nB, h, w, pitch0, pitch1 = args
            B = nB if B is None else int(B)
            if B != nB:
                raise ValueError("%d frames for B=%d" % (nB, B))
            handle = self._lookback_enable(lb, h, w)
        else:
            f, tab, dev, h, w, pitch0, pitch1, keep = 0, None, 0, 0, 0, 0, 0, None
            B = lb.streams - int(stream0) if B is None else int(B)
            handle = lb._handle(self)
        n, R = max(B, 0), lb.rows
        dets, lms, info = np.zeros((n, R, 5), np.float32), np.zeros((n, R, 10), np.float32), np.zeros((n, R, 3), np.int32)
        counts, state, moves = np.zeros((n,), np.int32), np.zeros((n, 4), np.int32), np.zeros((n, R, 4), np.int32)
        on_dev = scene is not None and not isinstance(scene, np.ndarray)
        sc = C.c_void_p(int(scene)) if on_dev else _lib.ptr(None if scene is None else np.ascontiguousarray(scene, dtype=np.int32).reshape(n, 4))
        self._chk(self._L.cf_lookback_step_frames(self._h, handle, int(stream0), B, 1 if push else 0, sc, 1 if on_dev else 0, f, tab, dev, h, w, pitch0,
                                                  pitch1, _lib.ptr(dets), _lib.ptr(lms), _lib.ptr(info), _lib.ptr(counts), _lib.ptr(state),
                                                  _lib.ptr(moves), 0))
        del keep
        return dets, lms, info, counts, state, moves

    def lookback_step_frames_device(self, lb, plane_ptrs, fmt, B, h, w, pitch0, pitch1, stream0=0, push=True, scene_ptr=None, dets_ptr=None,
                                    lms_ptr=None, info_ptr=None, counts_ptr=None, state_ptr=None, moves_ptr=None):
        """Same, reading DEVICE planes in place as ``track_follow_device`` takes them (``plane_ptrs`` None with ``push=False``) and the
        scene codes from a DEVICE buffer (or None), and writing caller-owned DEVICE buffers (as ``lookback_step_device``, plus moves
        [B,R,4] int32; any may be None): asynchronous on the engine's main stream behind the last step of ``lb``; nothing is read on
        the host.  The context keeps the lookback rows either way."""
        if push:
            f, tab, dev, B, h, w, pitch0, pitch1 = _lib.device_frame_args("lookback_step_frames_device", plane_ptrs, fmt, B, h, w, pitch0, pitch1)
            handle = self._lookback_enable(lb, h, w)
        else:
            f, tab, dev, h, w, pitch0, pitch1 = 0, None, 1, 0, 0, 0, 0
            handle = lb._handle(self)
        self._chk(self._L.cf_lookback_step_frames(self._h, handle, int(stream0), int(B), 1 if push else 0, _lib.vp(scene_ptr), 1, f, tab, dev, h, w,
                                                  pitch0, pitch1, _lib.vp(dets_ptr), _lib.vp(lms_ptr), _lib.vp(info_ptr), _lib.vp(counts_ptr),
                                                  _lib.vp(state_ptr), _lib.vp(moves_ptr), 1))

    # -- best-shot selection: each track's sharpest chip ---------------------------------------------
    def bestshot_offer(self, shots, chips, offsets, hw, stream0=0):
        """Offer ``shots`` (a ``BestShots``) the chips of this frame (``cf_bestshot_offer``, host form): ``chips`` uint8 [N, size, size, 3]
        and ``offsets`` [B+1] as ``align_faces_frame`` (or ``align_faces``) returned them for the tracked rows this engine holds -- behind a
        ``track_update`` or ``track_follow`` --, image b being the next frame of stream ``stream0 + b``; ``hw`` = (h, w) of the frames the
        chips were cut from (the network's (H, W) for ``align_faces``).  Every row with ``misses == 0`` and ``hits >= min_hits`` that has
        a chip is scored, and the table keeps per track id the chip with the highest quality; an id that is gone from the rows finishes
        its entry.  Returns (quality int64 [N]: Q of the chip of an eligible row, -1 otherwise; flags int32 [B]: bit 0 = a new track
        found no free entry).  No state of the engine changes."""
        ch = np.ascontiguousarray(chips, dtype=np.uint8)
        if ch.ndim != 4 or ch.shape[1:] != (shots.size, shots.size, 3):
            raise ValueError("chips must be [N, %d, %d, 3], got %s" % (shots.size, shots.size, ch.shape))
        offs = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        B, N = offs.size - 1, ch.shape[0]
        if N == 0:
            ch = np.zeros((1,) + ch.shape[1:], np.uint8)                      # (an address to name; cap_faces = 0 reads none of it)
        quality, flags = np.full((N,), -1, np.int64), np.zeros((max(B, 0),), np.int32)
        self._chk(self._L.cf_bestshot_offer(self._h, shots._handle(self), int(stream0), B, _lib.ptr(ch), _lib.ptr(offs), N, 0, int(hw[0]), int(hw[1]),
                                            _lib.ptr(quality) if N else None, _lib.ptr(flags), 0))
        return quality, flags

    def bestshot_offer_device(self, shots, chips_ptr, offsets_ptr, cap_faces, B, hw, stream0=0, quality_ptr=None, flags_ptr=None):
        """Same, reading the DEVICE chips and offsets an ``align_faces_frame_device`` wrote (chips for ``cap_faces`` faces, 16-byte
        aligned) and writing caller-owned DEVICE outputs (quality [cap_faces] int64, flags [B] int32; either may be None): asynchronous
        on the engine's main stream behind the align; nothing is read on the host."""
        self._chk(self._L.cf_bestshot_offer(self._h, shots._handle(self), int(stream0), int(B), _lib.vp(chips_ptr), _lib.vp(offsets_ptr), int(cap_faces), 1,
                                            int(hw[0]), int(hw[1]), _lib.vp(quality_ptr), _lib.vp(flags_ptr), 1))

    def bestshot_collect(self, shots, stream0=0, B=None, cap=None, flush=False):
        """The finished entries of the streams ``stream0 .. stream0 + B - 1`` of ``shots`` (default: all from ``stream0`` on), at most
        ``cap`` per stream (default: every entry), in finishing order (``cf_bestshot_collect``, host form); ``flush=True`` first finishes
        every live entry -- the end of the video.  Returns (chips [B, cap, size, size, 3], quality int64 [B, cap], records int32
        [B, cap, 8] = id, best_t, first_t, last_t, n_offered, sharp, size_w | pose_w << 10 | score_w << 20, done_seq; dets [B, cap, 5]
        and lms [B, cap, 10] = the row of the best frame; counts [B]: the valid rows; pending [B]: finished entries that did not fit;
        flags [B]: bit 0 = since the last collect a new track found no free entry).  Needs no forward on this engine."""
        B = shots.streams - int(stream0) if B is None else int(B)
        cap = shots.entries if cap is None else int(cap)
        k, S = max(cap, 0), shots.size
        chips, quality, records = np.zeros((max(B, 0), k, S, S, 3), np.uint8), np.zeros((max(B, 0), k), np.int64), np.zeros((max(B, 0), k, 8), np.int32)
        dets, lms = np.zeros((max(B, 0), k, 5), np.float32), np.zeros((max(B, 0), k, 10), np.float32)
        counts, pending, flags = (np.zeros((max(B, 0),), np.int32) for _ in range(3))
        self._chk(self._L.cf_bestshot_collect(self._h, shots._handle(self), int(stream0), B, cap, 1 if flush else 0, _lib.ptr(chips), _lib.ptr(quality),
                                              _lib.ptr(records), _lib.ptr(dets), _lib.ptr(lms), _lib.ptr(counts), _lib.ptr(pending), _lib.ptr(flags), 0))
        return chips, quality, records, dets, lms, counts, pending, flags

    def bestshot_collect_device(self, shots, stream0, B, cap, flush=False, chips_ptr=None, quality_ptr=None, records_ptr=None, dets_ptr=None,
                                lms_ptr=None, counts_ptr=None, pending_ptr=None, flags_ptr=None):
        """Same, writing caller-owned DEVICE buffers ([B, cap, ...] as above, chips 16-byte aligned; any may be None -- the entries are
        freed all the same): asynchronous on the engine's main stream behind the table's last call."""
        self._chk(self._L.cf_bestshot_collect(self._h, shots._handle(self), int(stream0), int(B), int(cap), 1 if flush else 0, _lib.vp(chips_ptr), _lib.vp(quality_ptr),
                                              _lib.vp(records_ptr), _lib.vp(dets_ptr), _lib.vp(lms_ptr), _lib.vp(counts_ptr), _lib.vp(pending_ptr), _lib.vp(flags_ptr), 1))

    # -- launch plan / layer trace (parity tests) ---------------------------------------------
    def plan(self):
        """The context's launch plan: list of dicts name/kind/C/H/W/fused_away."""
        n = C.c_int()
        self._chk(self._L.cf_plan_size(self._h, C.byref(n)))
        out = []
        for i in range(n.value):
            info = _lib.OpInfo()
            self._chk(self._L.cf_plan_op(self._h, i, C.byref(info)))
            out.append(dict(index=i, name=info.name.decode(), kind=info.kind.decode(), C=info.C, H=info.H, W=info.W,
                            fused_away=bool(info.fused_away)))
        return out

    def trace(self, x, op_index):
        """Run the forward up to plan entry ``op_index`` and return that entry's output as NCHW float32."""
        x = np.ascontiguousarray(x)
        in_format = _lib.CF_IN_U8_HWC_BGR if x.dtype == np.uint8 else _lib.CF_IN_F32_NCHW
        if x.dtype != np.uint8:
            x = np.ascontiguousarray(x, dtype=np.float32)
        op = self.plan()[op_index]
        out = np.empty((x.shape[0], op["C"], op["H"], op["W"]), np.float32)
        self._chk(self._L.cf_forward_trace(self._h, _lib.ptr(x), in_format, 0, x.shape[0], int(op_index), _lib.ptr(out)))
        self.last_B = x.shape[0] if op_index == len(self.plan()) - 1 else 0
        return out

    # -- timing -----------------------------------------------------------------------------
    def event_record(self, slot):
        self._chk(self._L.cf_event_record(self._h, int(slot)))

    def event_elapsed_ms(self, a, b):
        ms = C.c_float()
        self._chk(self._L.cf_event_elapsed_ms(self._h, int(a), int(b), C.byref(ms)))
        return ms.value

    def profile_forward(self, x, on_device=False, B=None, in_format=None, K=0):
        """Per-kernel times of one forward: list of dicts name/kind/ms/algo_bytes/flops."""
        if on_device:
            p = C.c_void_p(int(x))
        else:
            x = np.ascontiguousarray(x)
            in_format = _lib.CF_IN_U8_HWC_BGR if x.dtype == np.uint8 else _lib.CF_IN_F32_NCHW
            B = x.shape[0]
            p = _lib.ptr(x)
        rec = (_lib.OpTime * 64)()
        n = C.c_int()
        self._chk(self._L.cf_profile_forward(self._h, p, int(in_format), 1 if on_device else 0, int(B), int(K),
                                             rec, 64, C.byref(n)))
        self.last_B = int(B)
        return [dict(name=r.name.decode(), kind=r.kind.decode(), kernel=r.kernel.decode(), ms=r.ms, algo_bytes=r.algo_bytes, flops=r.flops)
                for r in rec[:n.value]]

    def streams(self):
        """(main, decode) hipStream_t handles as ints, e.g. for torch.cuda.ExternalStream."""
        a, b = C.c_void_p(), C.c_void_p()
        self._chk(self._L.cf_get_streams(self._h, C.byref(a), C.byref(b)))
        return a.value or 0, b.value or 0

    def shares_queue_with(self, other):
        """True when this context's main stream waits behind ``other``'s (same hardware queue).  Both must be idle."""
        sh = C.c_int(0)
        self._chk(self._L.cf_streams_share_queue(other._h, self._h, C.byref(sh)))
        return bool(sh.value)

    def queue_shared(self, which, other, which_other):
        """The same probe for any pair of streams (``cf_streams_share_queue_ex``): which = 0 main, 1 decode, 2 the device's copy stream."""
        sh = C.c_int(0)
        self._chk(self._L.cf_streams_share_queue_ex(other._h, int(which_other), self._h, int(which), C.byref(sh)))
        return bool(sh.value)

    def reroll_streams(self):
        """Replace the main and decode streams by newly created ones (cf_reroll_streams).  The context must be idle."""
        self._chk(self._L.cf_reroll_streams(self._h))

    def graph_stats(self):
        """(captured forward graphs, keys that fell back to eager launches)."""
        a, b = C.c_int(), C.c_int()
        self._chk(self._L.cf_graph_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def pinned_array(self, shape, dtype=np.uint8):
        """A numpy array in page-locked host memory (cf_host_alloc): forward_enqueue / forward_resized_enqueue from it
        are asynchronous DMA copies.  Freed with the engine (close)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._chk(self._L.cf_host_alloc(self._h, max(n, 1), C.byref(p)))
        if not hasattr(self, "_pinned"):
            self._pinned = []
        self._pinned.append(p)
        buf = (C.c_char * max(n, 1)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def pinned_raw(self, nbytes):
        """(pointer, capacity) of a fresh page-locked host buffer owned by the engine (freed at close or by pinned_free)."""
        p = C.c_void_p()
        self._chk(self._L.cf_host_alloc(self._h, max(int(nbytes), 1), C.byref(p)))
        if not hasattr(self, "_pinned"):
            self._pinned = []
        self._pinned.append(p)
        return p, int(nbytes)

    def pinned_free(self, p):
        """Release one buffer of pinned_array / pinned_raw now (no copy from it may be in flight)."""
        self._pinned = [q for q in getattr(self, "_pinned", []) if q.value != p.value]
        self._L.cf_host_free(self._h, p)

    def device_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self._L.cf_device_alloc(self._h, int(nbytes), C.byref(p)))
        return p.value

    def device_free(self, p):
        self._chk(self._L.cf_device_free(self._h, C.c_void_p(int(p))))

    def memcpy_h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self._L.cf_memcpy_h2d(self._h, C.c_void_p(int(dptr)), _lib.ptr(arr), arr.nbytes))

    def memcpy_d2h(self, arr, dptr):
        """Blocking copy of ``arr.nbytes`` device bytes at ``dptr`` into the C-contiguous numpy array ``arr``."""
        if not arr.flags["C_CONTIGUOUS"]:
            raise ValueError("memcpy_d2h needs a C-contiguous destination")
        self._chk(self._L.cf_memcpy_d2h(self._h, _lib.ptr(arr), C.c_void_p(int(dptr)), arr.nbytes))


class _StreamState(object):
    """What ``Tracker``, ``SceneCuts``, ``Lookback`` and ``BestShots`` share: one object of the library that holds the state of ``streams``
    video streams on one GPU.  A subclass names the library's functions (``_create``, ``_destroy`` and, where there is one, ``_clear``)
    and the noun of the messages, and hands ``_open`` its options struct last in its ``__init__``."""

    _create = _destroy = _clear = _noun = None

    def _open(self, engine_or_device, streams, opts):
        self._L = _lib.lib()
        self._o = opts
        self.streams = int(streams)
        self._h = None
        if isinstance(engine_or_device, Engine):
            self.device = engine_or_device.device
            self._handle(engine_or_device)
        else:
            self.device = int(engine_or_device)
            # refuse bad options now, not at the first call (no context: the library checks the arguments and tells)
            out = C.c_void_p()
            self._make(None, out)
            why = (self._L.cf_op_last_error() or b"").decode(errors="replace")
            if "null context" not in why:
                raise _lib.CenterFaceValueError(-1, why)

    def _make(self, ctx, out):
        """The library's create call with the context handle ``ctx`` (None: only the arguments are checked); returns its code."""
        return getattr(self._L, self._create)(ctx, self.streams, C.byref(self._o), C.byref(out))

    def _handle(self, engine):
        """The library's object, created with ``engine``'s context on first use."""
        if self._h is None:
            if engine.device != self.device:
                raise ValueError("the %s was made for device %d, the engine runs on device %d" % (self._noun, self.device, engine.device))
            out = C.c_void_p()
            _lib.check(self._make(engine._h, out), engine._h)
            self._h = out
        return self._h

    def _clear_stream(self, stream):
        if not -1 <= int(stream) < self.streams:
            raise ValueError("stream %d of a %s with %d" % (stream, self._noun, self.streams))
        if self._h is not None:
            _lib.check(getattr(self._L, self._clear)(self._h, int(stream)), op=True)

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tracker(_StreamState):
    """One cf_tracker: ``streams`` independent video streams on one GPU, ``max_tracks`` slots each (``include/centerface_hip.h`` states
    the update).  ``engine_or_device``: an ``Engine`` (the tracker is created at once on its GPU) or a device index (created by the first
    ``Engine.track_update`` that uses it, which must be on that GPU).  A face that matches a track (IoU >= ``iou``) keeps its id; a track
    seen ``min_hits`` times running is held for up to ``max_age`` frames without a detection, its box growing by ``hold_grow`` of its
    size per missed frame.  A frame with more faces and held tracks than ``max_tracks`` DROPS the surplus new faces (flag bit 0): they are
    not covered.  The defaults are this project's choices; no accuracy claim is made for them.  Engines of one GPU may share a tracker:
    its updates are ordered in call order.

    ``weak_score`` (default None: the tracker above): two thresholds, ``0 < weak_score < birth_score <= 1``.  ``weak_score`` is the
    score threshold the caller -- or the product paths of ``CenterFace``, which read it from here -- DECODES at; the library never sees
    it.  Rows with ``score > birth_score`` associate, are born and are returned as before; the rows between the two thresholds may
    only match a track that was already confirmed (``min_hits``), at IoU >= ``weak_iou``, and are otherwise discarded: the frame in
    which a face scores 0.29 keeps its track alive with the box and the landmarks of THAT frame instead of a held, stale box (flag
    bit 1 of the update says that it happened).  0.1 and 0.5 are ByteTrack's customary values and this project's choice: nobody has
    measured them here, and no accuracy claim is made.

    ``motion`` (default None: no motion model): True, or a dict with ``gain`` and / or ``damp`` -- constant-velocity prediction
    (``include/centerface_hip.h``, "constant velocity").  Every slot keeps a velocity; rows are matched against the box where the face
    is EXPECTED, and a held box coasts with its landmarks by the velocity per missed frame (times ``damp`` after each).  The model cannot
    bootstrap (the second sighting must still match the unpredicted box), only the centre moves, and a coast at ``damp = 1`` carries
    a held box ``max_age * v`` away.  ``gain = 0.5`` and ``damp = 1.0`` (SORT's coast) are this project's choices: there is no labelled
    video here, nobody has measured them, and no accuracy claim is made.  ``Tracker.motion`` is None or the dict of the two numbers;
    every product path reads the model from the tracker it is given."""

    _create, _destroy, _clear, _noun = "cf_track_create", "cf_track_destroy", "cf_track_reset", "tracker"

    def __init__(self, engine_or_device, streams, iou=0.3, max_age=15, min_hits=2, max_tracks=256, hold_grow=0.0, weak_score=None, birth_score=0.3,
                 weak_iou=0.5, motion=None):
        self.max_tracks = int(max_tracks)
        self.motion, self._mo = None, _lib.track_motion_of(motion)
        if self._mo is not None:
            gain, damp = float(self._mo.gain), float(self._mo.damp)
            if not 0.0 < gain <= 1.0:                                                # (a NaN fails every comparison)
                raise ValueError("gain must be finite and in (0, 1], got %r" % (gain,))
            if not 0.0 <= damp <= 1.0:
                raise ValueError("damp must be finite and in [0, 1], got %r" % (damp,))
            self.motion = dict(gain=gain, damp=damp)
        self.weak_score, self.birth_score, self._wo = None, None, None
        if weak_score is not None:
            weak_score, birth_score, weak_iou = float(weak_score), float(birth_score), float(weak_iou)
            if not 0.0 < weak_score < birth_score <= 1.0:                         # (a NaN fails every comparison)
                raise ValueError("a weak tracker needs 0 < weak_score < birth_score <= 1, got weak_score=%r, birth_score=%r" % (weak_score, birth_score))
            if not 0.0 < weak_iou <= 1.0:
                raise ValueError("weak_iou must be in (0, 1], got %r" % (weak_iou,))
            self.weak_score, self.birth_score, self._wo = weak_score, birth_score, _lib.track_weak_opts(birth_score, weak_iou)
        self._open(engine_or_device, streams, _lib.track_opts(iou, max_age, min_hits, max_tracks, hold_grow))

    def _make(self, ctx, out):
        if self._mo is not None:
            return self._L.cf_track_create_ex(ctx, self.streams, C.byref(self._o), None if self._wo is None else C.byref(self._wo), C.byref(self._mo),
                                              C.byref(out))
        if self._wo is None:
            return _StreamState._make(self, ctx, out)
        return self._L.cf_track_create_weak(ctx, self.streams, C.byref(self._o), C.byref(self._wo), C.byref(out))

    def reset(self, stream=-1):
        """A scene cut: drop every track of ``stream`` (-1: of all streams).  ids are not reused."""
        self._clear_stream(stream)


class SceneCuts(_StreamState):
    """One cf_scene: the last frame signature of ``streams`` independent video streams on one GPU (``include/centerface_hip.h`` states the
    signature and the check).  ``engine_or_device``: an ``Engine`` (created at once on its GPU) or a device index (created by the first
    ``Engine.scene_check`` that uses it, which must be on that GPU).  A frame is a CUT when at least ``hist`` per mille of its pixels
    changed luma bin AND the 64 cell means moved by ``grid`` in sum.  A full-frame flash is reported as a cut (the cost: held tracks are
    lost); a dissolve is not one cut.  The defaults are this project's choices: there is no labelled video here, nobody has measured
    them, and no accuracy claim is made.  Engines of one GPU may share an object: its checks are ordered in call order."""

    _create, _destroy, _clear, _noun = "cf_scene_create", "cf_scene_destroy", "cf_scene_forget", "scene object"

    def __init__(self, engine_or_device, streams, hist=350, grid=640):
        self._open(engine_or_device, streams, _lib.scene_opts(hist, grid))

    def forget(self, stream=-1):
        """The next check of ``stream`` (-1: of every stream) is FIRST: a new video begins there."""
        self._clear_stream(stream)


class Lookback(_StreamState):
    """One cf_lookback: a delay line of ``depth`` frames for ``streams`` independent video streams on one GPU (``include/centerface_hip.h``
    states the step).  ``engine_or_device``: an ``Engine`` (created at once on its GPU) or a device index (created by the first
    ``Engine.lookback_step`` that uses it, which must be on that GPU).  A frame leaves the line ``depth`` steps after it entered, with its
    own tracked rows plus the first box of every track born in the meantime -- seen in at least ``confirm`` of the queued frames --,
    grown by ``grow`` of its size per frame of distance: the face is covered BEFORE its first detection, where it was first detected
    (the box is not moved).  ``rows``: the most rows of a frame, pushed or emitted; a surplus of back-filled rows is DROPPED (state flag
    bit 0): those faces are not covered in that frame.  A scene cut (``scene=`` of the step, or ``forget``) is never painted across.  The
    defaults are this project's choices: there is no labelled video here, nobody has measured them, and no accuracy claim is made.
    Engines of one GPU may share an object: its steps are ordered in call order.  For the product paths (``CenterFace.anonymize(...,
    lookback=)``) the object also keeps, per stream, the host copies of the source frames that are still in the line.  ``trace()``
    opts in to back-filled boxes that follow the face through the queued frames."""

    _create, _destroy, _clear, _noun = "cf_lookback_create", "cf_lookback_destroy", "cf_lookback_forget", "lookback object"

    def __init__(self, engine_or_device, streams, depth=8, rows=256, grow=0.05, confirm=1):
        self.depth, self.rows = int(depth), int(rows)
        self._frames = [[] for _ in range(max(int(streams), 0))]             # per stream: the retained source frames, oldest first
        self._codes = None                                                    # (engine, device address): the scene codes of a chunk
        self._trace, self._traced_hw = None, None                             # ``trace()``'s options; the (h, w) the library object is enabled for
        self._open(engine_or_device, streams, _lib.lookback_opts(depth, rows, grow, confirm))

    def trace(self, search=4, max_sad=4096):
        """Opt in, before the object's first use, to back-filled boxes that FOLLOW the face through the queued frames
        (``include/centerface_hip.h``, "lookback with a trace"): the object then keeps the luma of every queued frame on the device
        (``depth + 1`` planes per stream: 16 streams, depth 8, 1080p: 298 MB), and a newborn face is matched backwards through them
        with the follower's block matching -- within ``search`` cells per frame, a best match above ``max_sad`` ends the chain.
        Pushes then go through ``Engine.lookback_step_frames``, whose first call enables the library object for its frames' size; the
        product paths do that by themselves.  The defaults are the follower's, this project's choices; no accuracy claim is made.
        Returns the object."""
        if self._traced_hw is not None or any(self._frames):
            raise ValueError("trace() comes before the %s's first use" % self._noun)
        # refuse bad options now, not at the first step (no context: the library checks the arguments and tells)
        self._L.cf_lookback_trace_enable(None, None, C.byref(_lib.follow_opts(search, max_sad)), 2, 2)
        why = (self._L.cf_op_last_error() or b"").decode(errors="replace")
        if "null context" not in why:
            raise _lib.CenterFaceValueError(-1, why)
        self._trace = dict(search=int(search), max_sad=int(max_sad))
        return self

    def fill(self, stream):
        """The number of source frames of ``stream`` the product paths still hold (0 .. depth)."""
        return len(self._frames[stream])

    def _retain(self, stream0, frames):
        """The product paths': frame b of ``frames`` is the newest source frame of stream ``stream0 + b`` (kept as it is, not copied)."""
        for b, frame in enumerate(frames):
            self._frames[stream0 + b].append(frame)

    def _due(self, stream0, B):
        """The oldest retained frame of each of the streams ``stream0 .. stream0 + B - 1`` as one new array [B, ...]; they are let go."""
        return np.stack([self._frames[stream0 + b].pop(0) for b in range(B)])

    def _scene_codes(self, engine):
        """A device buffer of this object for the scene codes of one chunk of ``engine`` (int32 [max_batch, 4])."""
        if self._codes is None or self._codes[0] is not engine:
            self._free_codes()
            self._codes = (engine, engine.device_alloc(16 * engine.max_batch))
        return self._codes[1]

    def _free_codes(self):
        if self._codes is not None:
            engine, p = self._codes
            self._codes = None
            if getattr(engine, "_h", None):
                engine.device_free(p)

    def forget(self, stream=-1):
        """Nothing pushed from now on is painted back into the frames of ``stream`` (-1: of every stream) that are queued now: for callers
        that reset the tracks themselves (``Tracker.reset``).  The queued frames still come out."""
        self._clear_stream(stream)

    def close(self):
        self._free_codes()
        _StreamState.close(self)                                              # (the luma ring and the trace table are the library object's)
        self._traced_hw = None


class BestShots(_StreamState):
    """One cf_bestshot table: ``streams`` independent video streams on one GPU, ``entries`` entries each -- live tracks plus finished ones
    not yet collected (``include/centerface_hip.h`` states the quality, the offer and the collect).  ``engine_or_device``: an ``Engine``
    (the table is created at once on its GPU) or a device index (created by the first ``Engine.bestshot_offer`` / ``bestshot_collect``
    that uses it, which must be on that GPU).  Per track id the table keeps the chip -- ``size`` x ``size`` uint8 BGR, as
    ``align_faces_frame(size=size)`` cuts it -- with the highest quality: the variance of the Laplacian of its central half, times the
    weights named in ``terms`` ('size': the face's side in the frame against the chip's; 'pose': the nose's offset from the eye-mouth
    axis; 'score': the detector's).  Only rows with ``misses == 0`` and ``hits >= min_hits`` are offered.  A stream with more live
    and uncollected tracks than ``entries`` does NOT ENTER the surplus (flag bit 0) until an entry is free.  The formula and the defaults
    are this project's choices; no accuracy claim is made for them.  Engines of one GPU may share a table: its calls are ordered in call
    order."""

    _create, _destroy, _noun = "cf_bestshot_create", "cf_bestshot_destroy", "table"      # (no clear: entries leave through the collect)

    def __init__(self, engine_or_device, streams, size=112, entries=320, min_hits=2, terms=("size", "pose", "score")):
        self.size, self.entries = int(size), int(entries)
        self._open(engine_or_device, streams, _lib.bestshot_opts(size, entries, min_hits, terms))


class EngineRing(object):
    """``depth`` independent contexts of one geometry used round-robin: batch i runs on context i % depth.

    Inside one context a forward is a chain on one stream.  Its back half -- the project GEMMs on the 40x40 / 20x20 maps
    (HBM-bound, small grids), the up3+heads kernel (memory-latency-bound) and the decode -- leaves the VALU idle, while
    its front half (stem, layer1.x / 2.x: VALU-issue-bound on Swish) leaves HBM idle.  With two batches in flight on two
    contexts (each has its own main / copy / decode streams and buffers) the GPU overlaps the back half of batch i with
    the front half of batch i+1: 44k -> 48k img/s at 64 x 640x640 bf16 (tools/dual_stream_probe.py; depth 3 adds
    nothing).  The reference has no counterpart (centerface.py:39-48 is one synchronous call per image); a C host does
    the same with two cf_ctx handles.  Contexts are independent: results of batch i are on context
    i % depth until batch i + depth is submitted.

        ring = EngineRing(640, 640, max_batch=64, dtype="bf16")
        t0 = ring.submit(batch0, K=100); t1 = ring.submit(batch1, K=100)
        dets, lms, inds = ring.collect(t0)          # waits for batch0 only
    """

    def __init__(self, height, width, depth=2, placement=None, **engine_kwargs):
        if depth < 1:
            raise ValueError("depth must be >= 1")
        # three or more contexts (small batches: BASELINE configs[4] shards of four 1280x1280 images): six streams on HIP's four hardware
        # queues serialise more than they overlap -- the decodes stay on the main streams (CF_FLAG_NO_DECODE_STREAM): 9.5 -> 12.2 k img/s at depth 3
        engine_kwargs.setdefault("decode_stream", depth < 3)
        # Where the ring's streams land decides whether its contexts overlap at all.  HIP folds a process's streams onto four hardware queues
        # PER PRIORITY CLASS and gives a new stream the least-used queue of its class; two main streams on one queue (or on two queues of one
        # dispatch pipe) run their forwards strictly one after the other (48.2 k img/s instead of 54.4 k at 64 x 640x640, and which of the two a
        # ring got depended on every stream the process had created before).
        #   placement="probe" (default): default-priority streams, every pair tested with spin kernels (cf_streams_share_queue_ex, + 16 = the
        #     dispatch-pipe form), cf_spread_streams re-places them all when two clash: 51.0-54.5 k in EVERY process history measured
        #     (tools/queue_order_probe.py, tools/ring_sequence_probe.py), ~15-30 ms at creation.
        #   placement="priority" (round 6): the ring's streams are created in the HIGHEST priority class (CF_FLAG_STREAM_HIGH) and nothing is
        #     probed.  A class of its own is proof against everything the process did in the DEFAULT class -- 54.3-54.5 k with an identical queue
        #     map after 0 / 1 / 2 / 3 / 5 dummy streams or live plain contexts, where default-class streams as created give 48.2-54.4 k -- but not
        #     against this library's own earlier use of the highest class: the device's copy stream lives there, five streams share four queues,
        #     and which two share depends on what was created AND DESTROYED before (a ring created after two plain contexts were closed: 47.5 k;
        #     after two single-context rings: 45.7-47.8 k; with the copy stream in the lowest class instead: 51.7 k always, 4 % under the best).
        #     For a server that creates its ring first and keeps it: the same rate as "probe" with no probe kernel ever launched.
        #   placement="none": streams as the runtime creates them.
        if placement is None:
            placement = os.environ.get("CF_RING_PLACEMENT") or "probe"
        if os.environ.get("CF_RING_PLACE", "1") == "0":        # (round-5 switch: streams as created)
            placement = "none"
        if placement not in ("priority", "probe", "none"):
            raise ValueError("placement must be 'priority', 'probe' or 'none'")
        if placement == "priority":
            engine_kwargs.setdefault("high_priority_streams", True)
        self.placement = placement
        self.engines = [Engine(height, width, **engine_kwargs) for _ in range(int(depth))]
        self.queue_rerolls = 0
        if placement == "probe":
            which = (0, 1) if engine_kwargs["decode_stream"] else (0,)
            streams = [(e, w) for e in self.engines for w in which]
            # (+ 16: the dispatch-pipe probe; two DECODE streams on one pipe are harmless and sometimes all the process's queues allow)
            clash = any(a[0].queue_shared(a[1] + 16, b[0], b[1]) for k, a in enumerate(streams) for b in streams[:k] if not (a[1] == 1 and b[1] == 1))
            if clash:
                hs = (C.c_void_p * len(self.engines))(*[e._h for e in self.engines])
                nd = C.c_int(0)
                self.engines[0]._chk(self.engines[0]._L.cf_spread_streams(hs, len(self.engines), 0, C.byref(nd)))
                self.queue_rerolls = 1
        self.depth = int(depth)
        self._n = 0
        self._out = [None] * self.depth               # per slot: (K, dets_ptr, lms_ptr, inds_ptr, B)

    def next_engine(self):
        """The context the next batch goes to (advances the ring): for callers that drive Engine directly."""
        e = self.engines[self._n % self.depth]
        self._n += 1
        return e

    def submit(self, x, K=100, on_device=False, B=None, in_format=None, use_reg=True):
        """Enqueue forward + top-K decode of one batch on the next context; returns a ticket for ``collect``."""
        slot = self._n % self.depth
        e = self.next_engine()
        e.forward_enqueue(x, on_device=on_device, B=B, in_format=in_format)
        o = self._out[slot]
        if o is None or o[0] < K:
            if o is not None:
                e.synchronize()
                for q in o[4]:
                    e.pinned_free(q)
            nb = e.max_batch
            # the decode's "device" outputs are page-locked HOST buffers (device-visible): the select kernel writes the B x K rows over
            # PCIe itself, and collect() is a wait + three numpy copies instead of three blocking device -> pageable transfers
            raw = [e.pinned_raw(nb * K * 6 * 4)[0], e.pinned_raw(nb * K * 10 * 4)[0], e.pinned_raw(nb * K * 8)[0]]
            o = (int(K), raw[0].value, raw[1].value, raw[2].value, raw)
        self._out[slot] = o
        e.decode_topk_device(K, o[1], o[2], o[3], use_reg=use_reg)
        return (slot, int(K), e.last_B)

    def collect(self, ticket):
        """(dets [B,K,6], lms [B,K,10], inds [B,K]) of a submitted batch (host arrays; waits for that context only)."""
        slot, K, B = ticket
        e, o = self.engines[slot], self._out[slot]
        # the decode wrote compact [B][K] rows (the K of its call) at the start of the slot's buffers
        e.synchronize()

        def host(addr, shape, dtype):
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return np.frombuffer((C.c_char * n).from_address(addr), dtype=dtype).reshape(shape).copy()
        return host(o[1], (B, K, 6), np.float32), host(o[2], (B, K, 10), np.float32), host(o[3], (B, K), np.int64)

    def load_state_dict(self, sd):
        for e in self.engines:
            e.load_state_dict(sd)

    def synchronize(self):
        for e in self.engines:
            e.synchronize()

    def close(self):
        for slot, e in enumerate(self.engines):
            self._out[slot] = None                # (the page-locked output buffers belong to the engine: freed with it)
            e.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_RESCALE, _UNFIT, _MERGE, _VIEWS, _PACKED = "rescale", "unfit", "merge", "views", "packed"      # how a plan's rows reach frame space: the five cases of ``_Plan.rows``
_Frames = collections.namedtuple("_Frames", "array fmt options")        # the cover, draw and follow steps: the array a chunk's slice of which they work on
_Scene = collections.namedtuple("_Scene", "scenes array fmt")           # the scene check: the ``SceneCuts`` and the array it looks at
_Best = collections.namedtuple("_Best", "shots array fmt template flush sink")      # the best shots: where the chips are cut, where the collect goes
_Late = collections.namedtuple("_Late", "lookback flush ready")         # the lookback: the ``Lookback``, drain at the end, the lists the call returns
_Plan = collections.namedtuple("_Plan", (
    "frames",        # the source the forward reads, sliced per chunk: an array or a list of frames
    "forward",       # the enqueue that takes any slice of ``frames``
    "per",           # frames per chunk
    "rows",          # how the rows reach frame space: _RESCALE (the decode rescales), _UNFIT (``Engine.unfit_rows``), _MERGE, _VIEWS or _PACKED
    "merge",         # (metric, thresh, edge) of ``Engine.merge_tiles`` for _MERGE, of ``Engine.merge_views`` for _VIEWS, of ``Engine.merge_packed`` for _PACKED
    "out",           # the output copy that is returned with the results, or None
    "tracker",       # the ``Tracker`` that every detected chunk advances, or None
    "scene",         # _Scene: every chunk is first checked for scene cuts, which frees the tracks of a cut stream
    "follow",        # _Frames: the tracker's faces are followed in the chunk right behind the update
    "detect",        # False: no forward, decode or update except in a key chunk; the results are the followed rows
    "cover",         # _Frames: the chunk's slice of the array is covered (``Engine.cover_faces``)
    "draw",          # _Frames: the chunk's slice of the array is annotated (``Engine.draw_faces``)
    "chips",         # chips(i, j) cuts the chips of frames i:j, which join the results
    "best",          # _Best: the chips of the tracked rows are offered per chunk, ONE collect follows the last
    "lookback",      # _Late: the chunk's frames are retained and its rows pushed; the frames that become due are covered or drawn instead
), defaults=(_RESCALE, None, None, None, None, None, True, None, None, None, None, None))
"""What one call asks of the chunk loop (``CenterFace._run``)."""


class CenterFace(object):
    """Same construction and call surface as the reference class (centerface.py:11-66)."""
    mean = np.array([0.408, 0.447, 0.470], dtype=np.float32).reshape(1, 1, 3)   # centerface.py:12-13
    std = np.array([0.289, 0.274, 0.278], dtype=np.float32).reshape(1, 1, 3)    # centerface.py:14-15

    def __init__(self, height, width, landmarks=True, *, weights=None, dtype="fp32", device=0,
                 max_batch=1, collapse_heads=None, nms_thresh=0.3, max_dets=1024, flip_test=False):
        """``flip_test=True``: every forward of every path runs the batch and its mirror and merges the heads on the device
        (``Engine(flip_test=True)``): about twice the network time; no accuracy claim is made."""
        self.landmarks = landmarks
        self.src_hw = (int(height), int(width))                                  # the frame size detect_yuv takes
        self.img_h_new, self.img_w_new, self.scale_h, self.scale_w = self.transform(height, width)
        self.nms_thresh = nms_thresh
        self.max_dets = max_dets
        self.device = device
        # (threshold decodes run on the main stream: these contexts never need a decode stream of their own)
        self._engine_kw = dict(max_batch=max_batch, dtype=dtype, device=device, weights=weights, collapse_heads=collapse_heads, decode_stream=False,
                               flip_test=flip_test)
        self.engine = Engine(self.img_h_new, self.img_w_new, **self._engine_kw)
        self._engine2 = None                      # second context of detect_stream, created on first use

    def close(self):
        self.engine.close()
        if self._engine2 is not None:
            self._engine2.close()
            self._engine2 = None

    # centerface.py:68-71
    def transform(self, h, w):
        img_h_new, img_w_new = int(np.ceil(h / 32) * 32), int(np.ceil(w / 32) * 32)
        scale_h, scale_w = img_h_new / h, img_w_new / w
        return img_h_new, img_w_new, scale_h, scale_w

    @staticmethod
    def _floordiv(a, scale):
        """``a // scale`` for a float32 array and a Python float exactly as numpy evaluates it (float32 operands, result the
        mathematically exact floor of the quotient), computed as floor of the float64 quotient: two float32 values whose
        ratio is not an integer differ from it by far more than a double's rounding, so the results are identical
        (tests/test_abi.py::test_fast_floor_division_equals_numpy_floor_divide, adversarial near-multiples included) --
        and numpy's own float32 floor_divide (an fmod per element) is 12x slower, which made this rescale half of the
        host time of a VGA-bucket batch."""
        return np.floor(a.astype(np.float64) / np.float64(np.float32(scale))).astype(np.float32)

    def _postprocess(self, dets, lms, rescaled=False):
        # centerface.py:55-62: floor-division rescale (``rescaled``: already done by the decode kernel, Engine.set_rescale),
        # empty -> [0,5] / [0,10]
        if len(dets) > 0 and rescaled:
            pass
        elif len(dets) > 0:
            dets[:, 0:4:2], dets[:, 1:4:2] = self._floordiv(dets[:, 0:4:2], self.scale_w), self._floordiv(dets[:, 1:4:2], self.scale_h)
            if self.landmarks:
                lms[:, 0:10:2], lms[:, 1:10:2] = self._floordiv(lms[:, 0:10:2], self.scale_w), self._floordiv(lms[:, 1:10:2], self.scale_h)
        else:
            dets = np.empty(shape=[0, 5], dtype=np.float32)
            if self.landmarks:
                lms = np.empty(shape=[0, 10], dtype=np.float32)
        return (dets, lms) if self.landmarks else dets

    def _postprocess_many(self, results, rescaled=False):
        """_postprocess for a list of (dets, lms) that share one (scale_h, scale_w): ONE floor division over the
        concatenated rows (elementwise, so identical to per-image calls), then split again.  ``rescaled``: the decode kernel
        has divided already (Engine.set_rescale) -- only the reference's empty-result shapes are left to do."""
        if rescaled:
            return [self._postprocess(d, l, True) for d, l in results]
        n = [len(d) for d, _ in results]
        if sum(n) == 0:
            return [self._postprocess(d, l) for d, l in results]
        dets = np.concatenate([d for d, _ in results if len(d)])
        lms = np.concatenate([l for d, l in results if len(d)])
        dets, lms = self._postprocess(dets, lms) if self.landmarks else (self._postprocess(dets, lms), None)
        out, o = [], 0
        for k in n:
            if k == 0:
                out.append(self._postprocess(np.empty((0, 5), np.float32), np.empty((0, 10), np.float32)))
            else:
                out.append((dets[o:o + k], lms[o:o + k]) if self.landmarks else dets[o:o + k])
            o += k
        return out

    def __call__(self, img, threshold=0.2):
        """img: BGR uint8 HWC (what cv2.imread returns).  Returns (dets [N,5], lms [N,10]) or dets."""
        return self.detect_batch([img], threshold)[0]

    def detect_batch(self, imgs, threshold=0.2):
        """Batched ``__call__`` (the shape of eval_widerface.get_detections, :76-90).  The reference's
        decode ignores ``threshold`` and uses 0.3 (centerface.py:77); so does this."""
        del threshold
        return self._run(self._plain(imgs))

    def _input_form(self, eng, imgs, fmt=None):
        """(frames, forward): the form in which ``eng`` takes ``imgs`` and the enqueue that takes any slice of them -- 4:2:0 frames
        (``fmt``) are converted on the device, page-locked images go up as they are (one DMA each, no host copy), a network-sized batch
        runs as it is, and anything else passes the device's cv2.resize stand-in."""
        if fmt is not None:
            return self._yuv_frames(imgs), lambda chunk: eng.forward_yuv_enqueue(chunk, fmt)
        imgs = [np.asarray(im, dtype=np.uint8) for im in imgs]
        direct = all(is_pinned(im) for im in imgs)
        batch = imgs if direct else np.stack(imgs)                           # one common (h, w) per instance
        identity = batch[0].shape[:2] == (self.img_h_new, self.img_w_new)
        return batch, eng.forward_images_enqueue if direct else eng.forward_enqueue if identity else eng.forward_resized_enqueue

    def _decode(self, eng, score=0.3):
        """The results of the forward last enqueued on ``eng``; the rescale (centerface.py:55-62) was done by the decode kernel."""
        return self._postprocess_many(eng.decode_threshold(score, self.nms_thresh, self.max_dets), rescaled=True)

    def _follow(self, follow, detect, tracker, frames, fmt):
        """The ``follow`` / ``detect`` arguments of the product paths -> the ``follow`` of a plan: None, or (array, fmt, options of
        ``Engine.track_follow``).  ``follow``: None / False, True (the defaults) or a dict with search and / or max_sad;
        ``detect=False`` follows in any case.  Both need a tracker."""
        if detect and not follow:
            return None
        if tracker is None:
            raise ValueError("follow= and detect=False need tracker=")
        o = dict(follow) if isinstance(follow, dict) else {}
        if set(o) - {"search", "max_sad"}:
            raise ValueError("follow takes search and max_sad, got %s" % sorted(o))
        return _Frames(frames, fmt, o)

    def _followed(self, dets, lms, counts, hw, tiled):
        """The per-frame results of a chunk that was only followed: the tracked rows mapped from the tracker's space to frame pixels in
        float64 (w / W, h / H of the network input; rows of a tiled path are in frame pixels already), not floored."""
        fx, fy = (1.0, 1.0) if tiled else (float(hw[1]) / float(self.img_w_new), float(hw[0]) / float(self.img_h_new))
        out = []
        for b, n in enumerate(counts):
            d, l = dets[b, :n].astype(np.float64), lms[b, :n].astype(np.float64)
            d[:, 0:4:2] *= fx
            d[:, 1:4:2] *= fy
            l[:, 0::2] *= fx
            l[:, 1::2] *= fy
            out.append((d, l) if self.landmarks else d)
        return out

    def _scene(self, scenes, tracker, frames, fmt):
        """The ``scenes`` argument of the product paths -> the ``scene`` of a plan: None, or (scenes, array, fmt).  Needs a tracker."""
        if scenes is None:
            return None
        if tracker is None:
            raise ValueError("scenes= needs tracker=")
        return _Scene(scenes, frames, fmt)

    def _lookback(self, lookback, flush, tracker, n):
        """The ``lookback`` / ``flush`` arguments of the product paths -> the ``lookback`` of a plan: None, or (lookback, flush, ready)
        with ``ready`` the n lists the call returns.  Needs a tracker, and the n streams of the call at one fill level: otherwise one
        step would be due for some of its images and not for others.  Refused before any engine call."""
        if lookback is None:
            if flush:
                raise ValueError("flush= needs lookback=")
            return None
        if tracker is None:
            raise ValueError("lookback= needs tracker=")
        if n > lookback.streams:
            raise ValueError("%d images for a lookback object with %d streams" % (n, lookback.streams))
        fills = [lookback.fill(k) for k in range(n)]
        if len(set(fills)) > 1:
            raise ValueError("the streams of this call stand at different fill levels of the lookback object: %s" % (fills,))
        return _Late(lookback, bool(flush), [[] for _ in range(n)])

    def _plan(self, frames, fmt, take, *, tiled=False, tile=None, overlap=None, with_full=True, merge=("ios", 0.5, 2.0), fit=None, tracker=None,
              follow=None, detect=True, scenes=None, lookback=None, flush=False, cover=None, draw=None, rotate=0, views=None):
        """The plan of a public product method from the keyword arguments they share (``fit``: what ``_fit_options`` made of it;
        ``views``: what ``_views_options`` made of it;
        ``cover`` / ``draw``: the options of that step; ``rotate``: the clockwise turn that makes the stored frames upright, 0 = none).  ``fmt`` None: BGR images.  ``take`` says what the steps in frame space work on:
        'copy' -- a new array, which the call returns (the inputs stay untouched); 'array' -- the frames as one uint8 array of the size
        this instance was built for, unless they are fitted or tiled; 'given' -- the frames as they are (fitted or tiled only).  The
        forward reads that array too, except on the untiled path of 'copy', which takes the input in ``_input_form``.  Refuses, in this
        order and before any engine call: what ``_lookback`` refuses, frames of the wrong form, a source that cannot be had (the
        instance's size, ``max_batch`` below the tiles of a frame), what ``_follow`` and ``_scene`` refuse."""
        rotate = self._rotation(rotate, tiled) if rotate else 0                  # (0: the plan of before, nothing of it is reached)
        eng = self.engine
        late = self._lookback(lookback, flush, tracker, len(frames))
        fmt_, plain, per, rows = "bgr" if fmt is None else fmt, not tiled and fit is None and not rotate and views is None, eng.max_batch, _RESCALE
        if take == "copy" and plain and fmt is not None:                          # 4:2:0 frames of the instance's size go up as they are
            src, forward = self._input_form(eng, frames, fmt)
            array = np.stack([np.asarray(f) for f in src])                        # a new array: the inputs stay untouched
        elif take == "copy":
            frames = [np.asarray(f, dtype=np.uint8) for f in frames]
            array = np.stack(frames)                                              # a new array: the inputs stay untouched
            # (the copy comes BEFORE the batch that ``_input_form`` stacks: with the two large blocks allocated the other way round the
            # allocator handed out cold pages in every call, and anonymize of 8 VGA frames took 3.0 ms instead of 1.4)
            src, forward = self._input_form(eng, frames) if plain else (array, None)
        elif take == "array":
            bgr, array = _lib.frame_format(fmt) == _lib.CF_FRAME_BGR, np.ascontiguousarray(frames, dtype=np.uint8)
            if array.ndim != (4 if bgr else 3):
                raise ValueError("frames must be uint8 [B,h,w,3] (bgr) or [B, h*3//2, w] (4:2:0), got %s" % (array.shape,))
        else:
            array = frames
        if views is not None:
            (forward, per), src = self._views_form(array, fmt_, views, cover is not None or draw is not None), array
            rows = _PACKED if views.get("pack") or views.get("rotate") else _VIEWS      # (rotated views always go through the packed forward)
            merge = (views["metric"], views["thresh"], views["edge"])
        elif rotate:                                                              # (fit None: the upright view is stretched)
            src, forward, rows = array, lambda chunk: eng.forward_rot_enqueue(chunk, fmt_, rotate, fit=fit), _UNFIT
        elif fit is not None:
            src, forward, rows = array, lambda chunk: eng.forward_fit_enqueue(chunk, fmt_, **fit), _UNFIT
        elif tiled:
            (forward, per), src, rows = self._tiled_form(array, fmt_, tile, overlap, with_full, cover is not None or draw is not None), array, _MERGE
        elif take == "array":
            want = self.src_hw + (3,) if bgr else (self.src_hw[0] * 3 // 2, self.src_hw[1])
            if array.shape[1:] != want:
                raise ValueError("frames must be %s per frame (this instance was built for %dx%d), got %s" % ((want,) + self.src_hw + (array.shape[1:],)))
            src, forward = array, eng.forward_resized_enqueue if bgr else lambda chunk: eng.forward_yuv_enqueue(chunk, fmt)
        step = lambda options: None if options is None else _Frames(array, fmt_, options)      # noqa: E731
        return _Plan(src, forward, per, rows, merge, array if take == "copy" else None, tracker, follow=self._follow(follow, detect, tracker, array, fmt_),
                     scene=self._scene(scenes, tracker, array, fmt_), detect=detect, cover=step(cover), draw=step(draw), lookback=late)

    def _plain(self, imgs, fmt=None, **steps):
        """The plan of the paths that only detect: the input in ``_input_form``, the decode rescales."""
        return _Plan(*self._input_form(self.engine, imgs, fmt), self.engine.max_batch, **steps)

    @contextlib.contextmanager
    def _rescaled(self, plan, on):
        """centerface.py:55-62 inside the decode kernel while the block runs -- where ``on`` and the plan's rows reach frame space that
        way --, switched off again whatever happens in it."""
        on = on and plan.rows == _RESCALE
        if on:
            self.engine.set_rescale(self.scale_h, self.scale_w)
        try:
            yield
        finally:
            if on:
                self.engine.set_rescale(0.0, 0.0)

    def _run(self, plan):
        """The chunk loop of every product path.  Per chunk of ``plan.per`` frames, image b of the chunk at frame i being stream i + b:
        the scene check; the detection (``_detect_chunk``) -- of every chunk with ``detect``, else of a key chunk, in which a frame is a
        stream's FIRST or a CUT --; the steps behind it (``_chunk_steps``): follow, best-shot offer, lookback step, cover, draw, chips.
        Behind the last chunk ``_finish``.  The decode rescales for the whole call with ``detect``, else around a key chunk's detection.
        Returns the lookback's lists, (the output copy, the per-frame results) or the per-frame results."""
        eng, res = self.engine, []
        with self._rescaled(plan, plan.detect):
            for i in range(0, len(plan.frames), plan.per):
                codes, key, sc = None, plan.detect, plan.scene
                if sc is not None and plan.lookback is not None and plan.detect:      # the codes go to the step in a device buffer
                    codes = plan.lookback.lookback._scene_codes(eng)
                    eng.scene_check(sc.array[i:i + plan.per], sc.fmt, sc.scenes, plan.tracker, i, codes=False, out_ptr=codes)
                elif sc is not None:
                    codes = eng.scene_check(sc.array[i:i + plan.per], sc.fmt, sc.scenes, plan.tracker, i, codes=not plan.detect)
                    key = plan.detect or bool((codes[:, 0] != _lib.CF_SCENE_SAME).any())
                res.extend(self._chunk_steps(plan, i, self._detect_chunk(plan, i) if key else None, codes))
            self._finish(plan)
        return plan.lookback.ready if plan.lookback is not None else res if plan.out is None else (plan.out, res)

    def _detect_chunk(self, plan, i):
        """The detection of the chunk at frame i: forward, decode, the rows to frame space, the tracker's update; the per-frame results."""
        eng = self.engine
        # a tracker with two thresholds: the decode keeps the rows above its weak_score for the update, and the results are the rows
        # above its birth_score -- those a decode at birth_score keeps, in the same order (include/centerface_hip.h, "two thresholds")
        weak = getattr(plan.tracker, "weak_score", None)
        score = 0.3 if weak is None else weak
        with self._rescaled(plan, not plan.detect):
            plan.forward(plan.frames[i:i + plan.per])
            if plan.rows == _RESCALE:
                res = self._decode(eng, score)
            else:
                eng.decode_threshold(score, self.nms_thresh, self.max_dets)
                rows = (eng.unfit_rows(self.max_dets) if plan.rows == _UNFIT else eng.merge_views(*plan.merge, self.max_dets) if plan.rows == _VIEWS
                        else eng.merge_packed(*plan.merge, self.max_dets) if plan.rows == _PACKED else eng.merge_tiles(*plan.merge, self.max_dets))
                res = self._postprocess_many(rows[0], rescaled=True)
            if plan.tracker is not None:
                eng.track_update_device(plan.tracker, i)
        return res if weak is None else self._strong(res, plan.tracker.birth_score)

    def _strong(self, res, birth_score):
        """The per-frame results with only the rows whose score is above ``birth_score`` (float32, strict: the decode's own compare)."""
        out = []
        for r in res:
            d, l = r if self.landmarks else (r, None)
            keep = d[:, 4] > np.float32(birth_score)
            out.append((d[keep], l[keep]) if self.landmarks else d[keep])
        return out

    def _chunk_steps(self, plan, i, res, codes):
        """The steps behind the detection of the chunk at frame i, while the engine still holds its rows: the follow (without ``detect``
        its rows are the results); the chips of the tracked rows offered to the best shots; with a lookback its step -- the chunk's
        frames are retained and the due ones covered and drawn (``_lookback_out``) --, else the chunk's frames covered and drawn; the
        chips, which join the results.  ``codes``: what the scene check left for the lookback step.  Returns the chunk's results."""
        eng, j, follow, best = self.engine, i + plan.per, plan.follow, plan.best
        if follow is not None:
            part = follow.array[i:j]
            d, l, _, n, _ = eng.track_follow(part, follow.fmt, plan.tracker, i, **follow.options)
            if not plan.detect:
                res = self._followed(d, l, n, _lib.frame_planes(part, follow.fmt, writable=False)[2:4], plan.rows != _RESCALE)
        if best is not None:
            part = best.array[i:j]
            cut, offs, _ = eng.align_faces_frame(part, best.fmt, best.shots.size, template=best.template)
            eng.bestshot_offer(best.shots, cut, offs, _lib.frame_planes(part, best.fmt, writable=False)[2:4], i)
        if plan.lookback is not None:
            lb, part = plan.lookback.lookback, (plan.draw if plan.cover is None else plan.cover).array[i:j]
            lb._retain(i, part)
            if getattr(lb, "_trace", None) is not None:                          # the chunk's frames go along: their luma is retained and traced through
                fmt_ = (plan.draw if plan.cover is None else plan.cover).fmt
                rows = eng.lookback_step_frames(lb, part, fmt_, i, len(part), push=True, scene=codes)[:5]
            else:
                rows = eng.lookback_step(lb, i, len(part), push=True, scene=codes)
            self._lookback_out(plan, i, rows)
        else:
            self._paint(plan, lambda array: array[i:j])
        if plan.chips is not None:
            cut, offs, _ = plan.chips(i, j)
            res = [(d, l, cut[offs[b]:offs[b + 1]]) for b, (d, l) in enumerate(res)]
        return res

    def _paint(self, plan, frames_of):
        """Cover, then draw, the faces of the rows the engine holds in ``frames_of(the step's array)``."""
        if plan.cover is not None:
            self.engine.cover_faces(frames_of(plan.cover.array), plan.cover.fmt, **plan.cover.options)
        if plan.draw is not None:
            self.engine.draw_faces(frames_of(plan.draw.array), plan.draw.fmt, **plan.draw.options)

    def _lookback_out(self, plan, i, rows):
        """Behind a step of the streams i .. i + B - 1: where a frame became due, the retained copies of those frames are covered or
        drawn with the lookback rows the engine holds, and (frame, dets, lms, info) joins ``ready`` per stream."""
        dets, lms, info, counts, state = rows
        if not (state[:, 0] >= 0).any():
            return
        due = plan.lookback.lookback._due(i, len(counts))                    # (the streams of a call stand at one fill level: all are due)
        self._paint(plan, lambda array: due)
        for b, n in enumerate(counts):
            plan.lookback.ready[i + b].append((due[b], dets[b, :n].copy(), lms[b, :n].copy(), info[b, :n].copy()))

    def _finish(self, plan):
        """Behind the last chunk: ONE collect of the best shots over the call's streams; with ``flush`` the lookback's streams are
        drained, one step per frame still in the line."""
        eng, n = self.engine, len(plan.frames)
        if plan.best is not None and n:
            plan.best.sink.append(eng.bestshot_collect(plan.best.shots, 0, n, flush=plan.best.flush))
        if plan.lookback is not None and plan.lookback.flush:
            lb = plan.lookback.lookback
            while n and lb.fill(0) > 0:                                           # the end of the video
                for i in range(0, n, plan.per):
                    self._lookback_out(plan, i, eng.lookback_step(lb, i, min(plan.per, n - i), push=False))

    def detect_aligned(self, imgs, size=112, **chip_options):
        """``detect_batch`` plus the aligned chip of every detection: one (dets, lms, chips) per image, dets / lms exactly those of
        ``detect_batch`` (rescale included), chips[k] = the face of dets[k] warped onto the chip template from the network-sized
        frame on the device (``Engine.align_faces``; ``chip_options``: out, rgb, mean, scale, template).  An image without
        detections gives an empty [0, ...] chip array."""
        if not self.landmarks:
            raise ValueError("detect_aligned needs the landmarks: construct CenterFace(..., landmarks=True)")
        return self._run(self._plain(imgs, chips=lambda i, j: self.engine.align_faces(size, **chip_options)))

    def detect_aligned_frames(self, frames, fmt="bgr", size=112, *, tiled=False, tile=None, overlap=None, fit=None, rotate=0, views=None, **chip_options):
        """Detection plus the aligned chip of every detection cut from the FRAME ITSELF (``Engine.align_faces_frame``), not from the
        network-sized batch: one (dets, lms, chips) per frame, dets / lms in frame pixels.  ``frames``: BGR uint8 [B,h,w,3]
        (``fmt='bgr'``) or dense 4:2:0 uint8 [B, h*3//2, w] ('nv12', 'nv21', 'i420', 'yv12') of the (height, width) this instance was
        built for; they go through ``forward_resized`` / ``forward_yuv`` and the results are those of ``detect_batch`` /
        ``detect_yuv`` (floor-divided to frame pixels).  ``tiled=True``: frames of any even size, detected by ``detect_tiled``'s path
        (``tile``, ``overlap``); the chips are those of the merged detections, which are in frame pixels and not floor-divided.
        ``fit``: True, or a dict with anchor, upscale and / or fill: frames of any size, detected by ``detect_fit``'s path instead
        (frame pixels, not floor-divided); not together with ``tiled``.  ``rotate``: as ``anonymize`` -- the similarity is fitted to the
        landmarks, so the chips of a turned frame come out upright.  ``views``: as ``anonymize`` (``detect_views``'s path).  ``chip_options``: out, rgb, mean, scale, template."""
        views = self._views_options(views, tiled, fit, rotate)
        fit = self._fit_options(fit, tiled)
        if not self.landmarks:
            raise ValueError("detect_aligned_frames needs the landmarks: construct CenterFace(..., landmarks=True)")
        plan = self._plan(frames, fmt, "array", tiled=tiled, tile=tile, overlap=overlap, fit=fit, rotate=rotate, views=views)
        return self._run(plan._replace(chips=lambda i, j: self.engine.align_faces_frame(plan.frames[i:j], fmt, size, **chip_options)))

    def _tiled_form(self, frames, fmt, tile, overlap, with_full, writable):
        """(forward, frames per chunk) of the tiled paths: the enqueue that cuts any slice of ``frames`` into the tiles of their size."""
        h, w = _lib.frame_planes(frames, fmt, writable=writable)[2:4]
        th, tw = (self.img_h_new, self.img_w_new) if tile is None else (int(tile), int(tile)) if np.isscalar(tile) else (int(tile[0]), int(tile[1]))
        if overlap is None:
            overlap = (min(th, tw) // 4) & ~1
        from . import ops
        rects = ops.tile_grid(h, w, (th, tw), overlap, with_full)
        per = self.engine.max_batch // len(rects)
        if per < 1:
            raise ValueError("%d tiles per frame need max_batch >= %d (this instance has %d)" % (len(rects), len(rects), self.engine.max_batch))
        return lambda chunk: self.engine.forward_tiles_enqueue(chunk, rects, fmt), per

    def _views_form(self, frames, fmt, views, writable):
        """(forward, frames per chunk) of the views paths: the enqueue that makes the views of any slice of ``frames`` (their size's
        layout, ``ops.view_layout``).  With a turn (``views['rotate']``) the layout is that of the UPRIGHT view (hu, wu) and the forward
        always the packed one: unpacked, the placement list {f, f * V + v, views[v]}."""
        h, w = _lib.frame_planes(frames, fmt, writable=writable)[2:4]
        from . import ops
        rot = views.get("rotate", 0)
        hu, wu = (w, h) if rot in (90, 270) else (h, w)
        table = ops.view_layout(hu, wu, self.img_h_new, self.img_w_new, views["tile"], views["overlap"], views["scales"], views["anchor"])
        if views.get("pack"):
            return self._packed_form(table, len(frames), fmt, views)
        V = len(table)
        per = self.engine.max_batch // V
        if per < 1:
            raise ValueError("%d views per frame need max_batch >= %d (this instance has %d)" % (V, V, self.engine.max_batch))
        if rot:
            def places(Bf):
                t = np.empty((Bf, V, 10), np.int32)
                t[:, :, 0], t[:, :, 1], t[:, :, 2:] = np.arange(Bf)[:, None], np.arange(Bf * V).reshape(Bf, V), table
                return t.reshape(-1, 10)
            return lambda chunk: self.engine.forward_packed_enqueue(chunk, places(len(chunk)), len(chunk) * V, fmt, fill=views["fill"], rot=rot), per
        return lambda chunk: self.engine.forward_views_enqueue(chunk, table, fmt, fill=views["fill"]), per

    def _packed_form(self, table, n_frames, fmt, views):
        """(forward, frames per chunk) of the packed views paths: frames per chunk is the largest Bf whose packed canvas count
        (``ops.pack_views``) fits ``max_batch`` -- the count is monotone in Bf, so the search goes upward -- and every chunk is packed for
        its own length (the last one may be shorter), the layouts cached by length."""
        from . import ops
        size, cap, layouts = (self.img_h_new, self.img_w_new), self.engine.max_batch, {}

        def layout(Bf):
            if Bf not in layouts:
                layouts[Bf] = ops.pack_views(table, Bf, size, views.get("gutter", 0))
            return layouts[Bf]
        if layout(1)[1] > cap:
            raise ValueError("the %d views of one frame pack into %d canvases and need max_batch >= %d (this instance has %d)"
                             % (len(table), layout(1)[1], layout(1)[1], cap))
        per = 1
        while per < n_frames and layout(per + 1)[1] <= cap:
            per += 1
        return lambda chunk: self.engine.forward_packed_enqueue(chunk, *layout(len(chunk)), fmt, fill=views["fill"], rot=views.get("rotate", 0)), per

    @staticmethod
    def _views_options(views, tiled=False, fit=None, rotate=0):
        """The ``views`` argument of the product paths -> None, or the options of ``detect_views``' path with every default filled in:
        ``views`` None / False, True (the defaults) or a dict with scales, tile, overlap, anchor, fill, metric, thresh, edge, pack, gutter
        and / or rotate (``pack``: several views and frames share a canvas, ``ops.pack_views`` with ``gutter`` pixels of fill between
        them; ``rotate``: 0, 90, 180 or 270, the clockwise turn that makes the STORED frames upright -- rotated views: the layout is that
        of the upright view, ``Engine.forward_packed_enqueue(rot=)`` cuts it and the rows come back in the stored frame's pixels).
        ``views`` excludes ``tiled=True``, ``fit`` and the top-level ``rotate``: the layout has its own tiles, its own fit and its own
        ``rotate`` key."""
        if views is None or views is False:
            return None
        for name, on in (("tiled=True", tiled), ("fit=", fit is not None and fit is not False), ("rotate=", bool(rotate))):
            if on:
                raise ValueError("views= and %s exclude each other: the views have their own tiles, their own fit and their own turn (rotated views: "
                                 "the rotate key of the views dict)" % name)
        o = dict(scales=(1.0, 0.5), tile=None, overlap=None, anchor="center", fill=(0, 0, 0), metric="ios", thresh=0.5, edge=2.0)
        given, late = dict(views) if isinstance(views, dict) else {}, {"pack", "gutter", "rotate"}      # (late: in the result only when given)
        if set(given) - set(o) - late:
            raise ValueError("views takes %s, got %s" % (", ".join(sorted(set(o) | late)), sorted(given)))
        o.update(given)
        if "rotate" in o:
            if o["rotate"] not in (0, 90, 180, 270):
                raise ValueError("the rotate key of views must be 0, 90, 180 or 270 (clockwise degrees), got %r" % (o["rotate"],))
            o["rotate"] = int(o["rotate"])
        _lib.view_opts(o["tile"], o["overlap"], o["scales"], o["anchor"])       # refuse bad names and numbers before any work
        _lib.fill_bytes(o["fill"])
        _lib.merge_opts(o["metric"], o["thresh"], o["edge"])
        if "gutter" in o:
            o["gutter"] = int(o["gutter"])
            if o["gutter"] < 0:
                raise ValueError("gutter must not be negative, got %d" % o["gutter"])
            if o["gutter"] and not o.get("pack"):
                raise ValueError("gutter= goes with pack=True")
        return o

    def detect_views(self, frames, fmt="bgr", *, scales=(1.0, 0.5), tile=None, overlap=None, anchor="center", fill=(0, 0, 0), metric="ios",
                     thresh=0.5, edge=2.0, redact=None, tracker=None, follow=None, detect=True, scenes=None, lookback=None, flush=False,
                     pack=False, gutter=0, rotate=0):
        """Multi-scale detection: every frame reaches the network as several VIEWS in one batch -- the aspect-true whole frame at each of
        ``scales`` (fractions of the fitted size; 0.5 shows a face that fills the frame at half the size, where a stride-4 centre
        detector holds together), placed by ``anchor`` on a canvas of ``fill``, and, with ``tile`` (``overlap``: default a fifth of the
        tile, rounded down to even), enlarged tiles in front of them -- and the per-view detections are mapped back and de-duplicated on
        the device (``Engine.merge_views``: ``metric``, ``thresh``, ``edge``).  ``frames`` as ``detect_tiled`` takes them, of any even
        size; ``max_batch`` must hold the views of one frame.  Returns (dets [n,5], lms [n,10]) per frame (``dets`` alone without
        landmarks), in FRAME pixels, not floor-divided.  Without ``pack`` there is one view per canvas: a half-size level costs a whole
        forward for a quarter of a canvas.  ``pack=True`` packs the views of the frames of a chunk into shared canvases
        (``ops.pack_views``, first-fit shelves, ``gutter`` pixels of fill between contents; ``Engine.forward_packed_enqueue`` /
        ``merge_packed``): levels 1.0, 0.5 and 0.25 of a 1080p frame then cost one 640 x 640 canvas per frame instead of three, and
        ``max_batch`` must hold the canvases of one frame.  Packed, the threshold decode's NMS and ``max_dets`` are per canvas and so
        shared by the frames on it, and boxes of two frames whose contents share an edge can suppress each other there: a gutter
        keeps them apart.  ``rotate``: 90, 180 or 270 -- rotated views: the clockwise turn that makes the STORED frames upright; the
        views are laid out in the upright view and cut from the stored frames in place (``Engine.forward_packed_enqueue(rot=)``, packed
        or, without ``pack``, one view per canvas), and the rows come back in the STORED frame's pixels, as behind ``detect_rotated``.
        One turn per call, no mirrored orientations, no probing.  The layout defaults, ``gutter`` = 0 and the
        IoS 0.5 / edge 2 merge are this project's choices and nobody has measured them; no accuracy claim is made.  ``redact``,
        ``tracker``, ``follow``, ``detect``, ``scenes``, ``lookback`` and ``flush``: as ``detect_tiled``."""
        views = self._views_options(dict(scales=scales, tile=tile, overlap=overlap, anchor=anchor, fill=fill, metric=metric, thresh=thresh, edge=edge,
                                         **(dict(pack=True, gutter=gutter) if pack else dict(gutter=gutter) if gutter else {}),
                                         **(dict(rotate=rotate) if rotate else {})))
        if redact is not None:
            _lib.split_redact_options(redact)                                   # refuse what blur does not take before any work
        if lookback is not None and redact is None:
            raise ValueError("lookback= needs redact=")                         # (without it there is nothing to delay)
        return self._run(self._plan(frames, fmt, "given", views=views, tracker=tracker, follow=follow, detect=detect, scenes=scenes, lookback=lookback,
                                    flush=flush, cover=redact))

    @staticmethod
    def _rotation(rotate, tiled=False):
        """The ``rotate`` argument of the product paths: the clockwise turn -- 0, 90, 180 or 270 -- that makes the STORED frames upright
        (``Engine.forward_rot_enqueue``; the rows come back in the stored frame's pixels).  ``rotate`` and ``tiled=True`` exclude each
        other."""
        if rotate not in (0, 90, 180, 270):
            raise ValueError("rotate must be 0, 90, 180 or 270 (clockwise degrees), got %r" % (rotate,))
        if rotate and tiled:
            raise ValueError("rotate= and tiled=True exclude each other: a rotated tiled forward is not covered")
        return int(rotate)

    def _fit_options(self, fit, tiled=False):
        """The ``fit`` argument of the product paths -> None, or the options of ``Engine.forward_fit_enqueue``: ``fit`` None / False,
        True (the defaults) or a dict with anchor, upscale and / or fill.  ``fit`` and ``tiled=True`` exclude each other."""
        if fit is None or fit is False:
            return None
        if tiled:
            raise ValueError("fit= and tiled=True exclude each other: a frame is either letterboxed or cut into tiles")
        o = dict(fit) if isinstance(fit, dict) else {}
        if set(o) - {"anchor", "upscale", "fill"}:
            raise ValueError("fit takes anchor, upscale and fill, got %s" % sorted(o))
        _lib.fit_opts(**o)                                                    # refuse bad names and bytes before any work
        return o

    def detect_fit(self, frames, fmt="bgr", *, anchor="center", upscale=True, fill=(0, 0, 0), redact=None, tracker=None, follow=None, detect=True,
                   scenes=None, lookback=None, flush=False, rotate=0):
        """Detection of frames of another size -- or shape -- than the network input WITHOUT the stretch of ``detect_batch``: every frame
        is resized on the device with its aspect ratio kept and pasted into the network's canvas (``Engine.forward_fit_enqueue``:
        ``anchor``, ``upscale``, ``fill``), and the rows whose centre lies in the content are mapped back (``Engine.unfit_rows``).
        ``frames``: BGR uint8 [B,h,w,3] (``fmt='bgr'``; odd sides allowed), dense 4:2:0 uint8 [B, h*3//2, w], or per-frame plane tuples.
        Returns (dets [n,5], lms [n,10]) per frame (``dets`` alone without landmarks), in FRAME pixels, not floor-divided.  No accuracy
        claim is made: there are no trained weights and no labelled set here; the reference's data pipeline fits and pads likewise
        (dataset/dataset.py:114-134).  ``redact``, ``tracker``, ``follow``, ``detect``, ``scenes``, ``lookback`` and ``flush``: as
        ``detect_tiled``.  ``rotate``: 90, 180 or 270 -- the clockwise turn that makes the STORED frames upright: the upright view is
        fitted (``Engine.forward_rot_enqueue``) and the rows come back in the stored frame's pixels; one turn per call."""
        if redact is not None:
            _lib.split_redact_options(redact)                                   # refuse what blur does not take before any work
        fit = self._fit_options(dict(anchor=anchor, upscale=upscale, fill=fill))
        if lookback is not None and redact is None:
            raise ValueError("lookback= needs redact=")                         # (without it there is nothing to delay)
        return self._run(self._plan(frames, fmt, "given", fit=fit, tracker=tracker, follow=follow, detect=detect, scenes=scenes, lookback=lookback,
                                    flush=flush, cover=redact, rotate=rotate))

    def detect_tiled(self, frames, tile=None, overlap=None, fmt="bgr", *, with_full=True, metric="ios", thresh=0.5, edge=2.0, redact=None,
                     tracker=None, follow=None, detect=True, scenes=None, lookback=None, flush=False):
        """Sliced inference for frames much larger than the network input, whose small faces the stretch-resize of ``detect_batch``
        loses: every frame is cut on the device into overlapping tiles of ``tile`` (default: the network's (H, W)) that share at
        least ``overlap`` pixels (default: a quarter of the tile, rounded down to even), plus the whole frame as one more tile; the
        tiles run as one batch, and the per-tile detections are mapped back and de-duplicated on the device (``Engine.merge_tiles``:
        ``metric``, ``thresh``, ``edge``).  ``frames``: BGR uint8 [B,h,w,3] (``fmt='bgr'``), dense 4:2:0 uint8 [B, h*3//2, w], or
        per-frame plane tuples -- of any even size; ``max_batch`` must hold the tiles of one frame.  Returns (dets [n,5], lms [n,10]) per
        frame (``dets`` alone without landmarks), in FRAME pixels, not floor-divided.  The defaults are this project's choices; no
        accuracy claim is made for them.  ``redact``: options of ``Engine.redact_faces``, or ``mode='blur'`` with those of
        ``Engine.blur_faces``; the frames are then redacted IN PLACE with the merged boxes.  ``tracker``: a ``Tracker`` whose
        stream k the k-th frame of this call continues (frame pixels): it is advanced behind the merge, and the redaction then covers
        the tracked rows -- the merged detections plus the tracks held through a dropout; the detections returned stay the frame's
        own.  A ``Tracker(motion=)`` carries its motion model itself: no argument here, the held rows are the coasted ones.  ``follow``, ``detect`` and ``scenes``: as ``anonymize`` (``redact=`` only; the frames are checked and followed as they are before the
        redaction).  ``lookback`` and ``flush`` (``redact=`` and an array of frames only): as ``anonymize`` -- the frames are then NOT
        redacted in place, the return is the lists of ``anonymize(lookback=)``."""
        if redact is not None:
            _lib.split_redact_options(redact)                                   # refuse what blur does not take before any work
        if lookback is not None and redact is None:
            raise ValueError("lookback= needs redact=")                         # (without it there is nothing to delay)
        return self._run(self._plan(frames, fmt, "given", tiled=True, tile=tile, overlap=overlap, with_full=with_full, merge=(metric, thresh, edge),
                                    tracker=tracker, follow=follow, detect=detect, scenes=scenes, lookback=lookback, flush=flush, cover=redact))

    def anonymize(self, imgs, *, tiled=False, tile=None, overlap=None, fit=None, tracker=None, follow=None, detect=True, scenes=None, lookback=None,
                  flush=False, rotate=0, views=None, **options):
        """``detect_batch`` plus the redaction of every detection: (frames_out, [(dets, lms), ...]) -- frames_out a uint8 [B,h,w,3] COPY of
        ``imgs`` in which every detected face is pixelated or blanked on the device (``Engine.redact_faces``; ``options``: mode, shape,
        cell, scale, fill) or, with ``mode='blur'``, blurred (``Engine.blur_faces``; shape, radius, scale), the detections exactly those of ``detect_batch`` (rescale included).  ``imgs`` are left untouched; an image
        without detections comes back byte for byte.  ``tiled=True``: detection by ``detect_tiled`` (``tile``, ``overlap``) on frames of
        any even size, redaction with the merged boxes; the detections are then in frame pixels.  ``tracker``: a ``Tracker`` (default none: every
        call stands alone) whose stream k the k-th image of this call continues -- a video is fed one call per frame, n cameras n images per
        call; it is advanced between the decode (the merge) and the redaction, which then covers the detections of this frame AND the
        tracks held through a dropout.  The detections returned stay the frame's own.  A tracker with two thresholds
        (``Tracker(weak_score=)``): every product path decodes at its ``weak_score`` instead of 0.3, so that the rows between the
        thresholds reach the update, and returns the rows above its ``birth_score``.  A tracker with a motion model
        (``Tracker(motion=)``) needs no argument here, in ``anonymize_yuv``, ``annotate*``, ``best_shots`` or ``detect_tiled(redact=)``:
        the tracker object carries it, and the held rows that are covered, drawn or cut are then the coasted ones.  ``follow`` (needs ``tracker``): True, or a dict with
        ``search`` and / or ``max_sad`` (``Engine.track_follow``; the defaults 4 and 4096 are this project's choices, no accuracy claim is
        made): right behind the update the tracker's faces are followed in the frame by block matching, so a track held through a dropout
        moves with its face instead of staying where it was last detected.  ``detect=False`` (needs ``tracker``, which a call with
        detection has advanced before): NO FORWARD -- the faces are only followed from where the tracker has them, then covered; the
        results are then the tracked rows (held ones included) mapped to frame pixels in float64, not floored.  Detecting every Nth
        frame and following in between is the throughput lever for video.  ``scenes`` (needs ``tracker``): a ``SceneCuts`` whose stream k the
        k-th image continues; every chunk is first checked for scene cuts on the device (``Engine.scene_check``) and the tracks of a cut
        stream are freed there, so nothing of the previous scene is held, followed or covered.  With ``detect=False`` a chunk in which a
        frame is a stream's first or a cut is detected after all (forward, decode, update, then the follow): ``detect=False`` then means
        "detect only where a scene starts".  A flash counts as a cut, a dissolve is not one; the thresholds are this project's choices, no
        accuracy claim is made.  ``fit``: True, or a dict with anchor, upscale and / or fill: detection by ``detect_fit`` on frames of
        any size -- letterboxed instead of stretched --, redaction with the rows mapped back, which are in frame pixels; not together
        with ``tiled``; no accuracy claim is made for it either.  ``lookback`` (needs ``tracker``): a ``Lookback`` whose stream k the k-th
        image continues: THE OUTPUT IS DELAYED by ``lookback.depth`` calls, and a face is covered in the frames BEFORE its first
        detection too -- with the first box of its track, grown by the distance, where it was first detected (not moved; the defaults
        are this project's choices, no accuracy claim is made).  Each chunk runs [scene check,] forward, decode, update[, follow], then
        ``Engine.lookback_step``; the frame that becomes due -- the object's own copy of the image of ``depth`` calls ago -- is covered
        with the lookback rows.  A ``Lookback`` with ``trace()`` set takes the chunk's frames too (``Engine.lookback_step_frames``; even
        sides): the back-filled boxes then follow the face through the queued frames.  The return is then, per image k of the call, the LIST of (frame, dets [n,5], lms [n,10], info [n,3] = id,
        hits, misses) that became ready: empty while stream k warms up, one item in the steady state, and with ``flush=True`` (the end of
        the video: the stream is drained) up to ``depth + 1``; dets and lms are the covered rows, in the tracker's space, back-filled ones
        with hits 0 and misses = the distance.  The streams of a call must stand at one fill level (ValueError).  With the defaults every
        call does what it did without them.  ``rotate``: 90, 180 or 270 -- the clockwise turn that makes the STORED frames upright (a
        corridor-mode camera, phone video): the network sees the upright view (``Engine.forward_rot_enqueue``; stretched to the network
        input, or fitted with ``fit``), frames of any size; detections and redaction are in the pixels of the stored frame, not
        floor-divided; not together with ``tiled``; one turn per call; no accuracy claim is made.  ``views``: True, or a dict with scales,
        tile, overlap, anchor, fill, metric, thresh, edge, pack, gutter and / or rotate: detection by ``detect_views`` -- several views of every
        frame in one batch, merged on the device -- on frames of any even size, the rows in frame pixels; not together with ``tiled``,
        ``fit`` or the top-level ``rotate`` (rotated views: the ``rotate`` key of the dict, as ``detect_views(rotate=)``; the rows and the
        redaction are then in the pixels of the STORED frame); no accuracy claim is made for it either."""
        return self._anonymize(imgs, None, options, tiled=tiled, tile=tile, overlap=overlap, fit=fit, tracker=tracker, follow=follow, detect=detect,
                               scenes=scenes, lookback=lookback, flush=flush, rotate=rotate, views=views)

    def anonymize_yuv(self, frames, fmt="nv12", *, tiled=False, tile=None, overlap=None, fit=None, tracker=None, follow=None, detect=True,
                      scenes=None, lookback=None, flush=False, rotate=0, views=None, **options):
        """``detect_yuv`` plus the redaction, for 4:2:0 video frames: (frames_out, [(dets, lms), ...]), frames_out a uint8
        [B, height*3//2, width] copy of ``frames`` in the same format with every detected face redacted in the luma and chroma planes.  ``tiled=True``, ``tracker``, ``follow``,
        ``fit``, ``detect``, ``scenes``, ``lookback``, ``flush``, ``rotate`` and ``views``: as ``anonymize``; a ``Tracker(motion=)`` carries its
        motion model itself, as there."""
        return self._anonymize(frames, fmt, options, tiled=tiled, tile=tile, overlap=overlap, fit=fit, tracker=tracker, follow=follow, detect=detect,
                               scenes=scenes, lookback=lookback, flush=flush, rotate=rotate, views=views)

    def _anonymize(self, frames, fmt, options, *, tiled, fit, rotate=0, views=None, **shared):
        """The body of ``anonymize`` (``fmt`` None: BGR images) and ``anonymize_yuv``: the copy of the frames is covered."""
        _lib.split_redact_options(options)                                    # refuse what blur does not take before any work
        views = self._views_options(views, tiled, fit, rotate)
        rotate = self._rotation(rotate, tiled) if rotate else 0
        return self._run(self._plan(frames, fmt, "copy", tiled=tiled, fit=self._fit_options(fit, tiled), cover=options, rotate=rotate, views=views, **shared))

    def best_shots(self, frames, fmt="bgr", *, tracker, shots, tiled=False, tile=None, overlap=None, fit=None, follow=None, detect=True,
                   flush=False, template=None, scenes=None, rotate=0, views=None):
        """One chip per appearance of a person: detection, tracking and best-shot selection of ``frames`` -- BGR uint8 [B,h,w,3]
        (``fmt='bgr'``) or dense 4:2:0 uint8 [B, h*3//2, w] -- where image k of a call is the next frame of stream k of ``tracker`` (a
        ``Tracker``) and of ``shots`` (a ``BestShots``), as in ``anonymize(tracker=)``: a video is fed one call per frame, n cameras n
        images per call.  Per chunk: forward, decode (``tiled=True``: ``detect_tiled``'s path with ``tile``, ``overlap``, on frames of any
        even size), ``track_update``, the follow if asked for (``follow``, ``detect``: as ``anonymize``), then the aligned chips of the
        tracked rows are cut from the frames at ``shots.size`` (``template``: as ``Engine.align_faces_frame``) and offered to the table;
        after the last chunk the finished entries of the call's streams are collected -- ``flush=True`` finishes every live track first
        (the end of the video).  Returns, per stream, the list of finished shots in finishing order: dicts with ``id``, ``quality``,
        ``chip`` [size, size, 3], ``det`` [5], ``lms`` [10] (the row of the best frame, in the tracker's space) and ``record`` (the eight
        int32 of ``Engine.bestshot_collect``).  ``scenes``: as ``anonymize`` -- a cut frees the stream's tracks, so their entries finish.  ``fit``: as ``anonymize`` (``detect_fit``'s path).  ``rotate``: as ``anonymize``; the chips are fitted to the landmarks, so they come out upright.  ``views``: as ``anonymize``.  A ``Tracker(motion=)`` carries its motion model itself (no argument here).  The quality formula is this project's choice; no accuracy claim is made for it."""
        views = self._views_options(views, tiled, fit, rotate)
        fit = self._fit_options(fit, tiled)
        if not self.landmarks:
            raise ValueError("best_shots needs the landmarks: construct CenterFace(..., landmarks=True)")
        if tracker is None or shots is None:
            raise ValueError("best_shots needs tracker= and shots=")
        plan = self._plan(frames, fmt, "array", tiled=tiled, tile=tile, overlap=overlap, fit=fit, tracker=tracker, follow=follow, detect=detect, scenes=scenes,
                          rotate=rotate, views=views)
        sink = []
        self._run(plan._replace(best=_Best(shots, plan.frames, fmt, template, bool(flush), sink)))
        if not sink:
            return []
        chips, quality, records, dets, lms, counts = sink[0][:6]
        return [[{"id": int(records[s, k, 0]), "quality": int(quality[s, k]), "chip": chips[s, k].copy(), "det": dets[s, k].copy(), "lms": lms[s, k].copy(),
                  "record": records[s, k].copy()} for k in range(int(counts[s]))] for s in range(len(plan.frames))]

    def _draw_options(self, options, tracker, yuv):
        """The options of ``annotate`` / ``annotate_yuv`` -> those of ``Engine.draw_faces``: the reference's look (demo.py:15-23: green
        boxes of thickness 1, red dots of radius 2) by default, the track id as the label when there is a tracker, else the score;
        colours are BGR triples, converted for 4:2:0 frames."""
        from . import ops
        o = dict(box_color=(2, 255, 0), lm_color=(0, 0, 255), held_color=(0, 255, 255), text_color=(0, 0, 0), thickness=1, radius=2,
                 label="id" if tracker is not None else "score", label_scale=2, dash_held=True, scale=1.0, landmarks=bool(self.landmarks))
        o.update(options)
        if yuv:
            for k in ("box_color", "lm_color", "held_color", "text_color"):
                o[k] = ops.bgr_to_yuv_color(o[k])
        _lib.draw_opts(**o)                                                   # refuse bad names and colours before any work
        return o

    def annotate(self, imgs, *, tiled=False, tile=None, overlap=None, fit=None, tracker=None, follow=None, detect=True, scenes=None, lookback=None,
                 flush=False, rotate=0, views=None, **options):
        """``detect_batch`` plus the drawing of every detection, what demo.py:15-23 does with cv2 on the host: (frames_out, [(dets, lms),
        ...]) -- frames_out a uint8 [B,h,w,3] COPY of ``imgs`` with box outlines, landmark dots and a label painted on the device
        (``Engine.draw_faces``; ``options`` as there, colours as BGR triples).  ``tiled``, ``tile``, ``overlap`` and ``tracker`` as
        ``anonymize``: with a tracker the label is the track id and the tracks held through a dropout are drawn too, dashed, in
        ``held_color``.  ``fit``, ``follow``, ``detect`` and ``scenes``: as ``anonymize``.  ``lookback`` and ``flush``: as ``anonymize`` --
        the delayed frames are drawn, a back-filled row as a held one (dashed, in ``held_color``), and the return is the lists.
        ``rotate``: as ``anonymize``; the labels are upright in the STORED frame, so a viewer of the upright video sees them turned.
        ``views``: as ``anonymize``.  A ``Tracker(motion=)`` carries its motion model itself (no argument here): the held tracks are
        drawn where they coasted to."""
        return self._annotate(imgs, None, options, tiled=tiled, tile=tile, overlap=overlap, fit=fit, tracker=tracker, follow=follow, detect=detect,
                              scenes=scenes, lookback=lookback, flush=flush, rotate=rotate, views=views)

    def annotate_yuv(self, frames, fmt="nv12", *, tiled=False, tile=None, overlap=None, fit=None, tracker=None, follow=None, detect=True,
                     scenes=None, lookback=None, flush=False, rotate=0, views=None, **options):
        """``annotate`` for 4:2:0 video frames: frames_out a uint8 [B, height*3//2, width] copy of ``frames`` in the same format, drawn
        in the luma and chroma planes; the BGR colours are converted with ``ops.bgr_to_yuv_color``.  ``fit``, ``scenes``, ``lookback`` and
        ``flush``, ``rotate`` and ``views``: as ``annotate``; a ``Tracker(motion=)`` likewise."""
        return self._annotate(frames, fmt, options, tiled=tiled, tile=tile, overlap=overlap, fit=fit, tracker=tracker, follow=follow, detect=detect,
                              scenes=scenes, lookback=lookback, flush=flush, rotate=rotate, views=views)

    def _annotate(self, frames, fmt, options, *, tiled, fit, tracker, rotate=0, views=None, **shared):
        """The body of ``annotate`` (``fmt`` None: BGR images) and ``annotate_yuv``: the copy of the frames is drawn into."""
        views = self._views_options(views, tiled, fit, rotate)
        fit = self._fit_options(fit, tiled)
        rotate = self._rotation(rotate, tiled) if rotate else 0
        return self._run(self._plan(frames, fmt, "copy", tiled=tiled, fit=fit, tracker=tracker, draw=self._draw_options(options, tracker, fmt is not None),
                                    rotate=rotate, views=views, **shared))

    def _yuv_frames(self, frames):
        """The frames of detect_yuv / detect_stream(fmt=...) checked against the instance's (height, width): a [B, height*3//2, width]
        array as it is, anything else as a list of [height*3//2, width] arrays."""
        want = (self.src_hw[0] * 3 // 2, self.src_hw[1])
        if isinstance(frames, np.ndarray) and frames.ndim == 3:
            if frames.dtype != np.uint8 or frames.shape[1:] != want:
                raise ValueError("frames must be uint8 [B, %d, %d] (4:2:0 frames of %dx%d), got %s %s"
                                 % (want + self.src_hw + (frames.dtype, frames.shape)))
            return frames
        frames = [np.asarray(f) for f in frames]
        for f in frames:
            if f.dtype != np.uint8 or f.shape != want:
                raise ValueError("frames must be uint8 [%d, %d] arrays (4:2:0 frames of %dx%d), got %s %s"
                                 % (want + self.src_hw + (f.dtype, f.shape)))
        return frames

    def detect_yuv(self, frames, fmt="nv12"):
        """``detect_batch`` for 4:2:0 video frames -- NV12 / NV21 from hardware decoders, I420 (yuv420p) / YV12 from software ones:
        the same results as ``detect_batch([cv2.cvtColor(f, cv2.COLOR_YUV2BGR_<fmt>) for f in frames])``, with the conversion on the
        device and half the bytes of BGR over the link.  ``frames``: uint8 [B, height*3//2, width] or a list of [height*3//2, width]
        arrays, (height, width) = the size this instance was built for (ValueError otherwise)."""
        return self._run(self._plain(frames, fmt))

    def detect_stream(self, imgs, threshold=0.2, *, fmt=None):
        """``__call__`` over an iterable of same-sized images, results yielded in order (the loop of demo.py:30-38 /
        eval_widerface.py:76-90).  The reference runs one synchronous call per image; here two contexts alternate, the
        forward of chunk i+1 (``max_batch`` images) is enqueued before the host waits for the decode of chunk i, so the GPU
        works on one chunk while the host decodes and rescales the other.  Same results as ``__call__`` (tests).
        ``fmt`` ('nv12', 'nv21', 'i420', 'yv12'): the items are 4:2:0 video frames of the instance's size, as ``detect_yuv`` takes
        them -- a decoder's output, converted on the device."""
        del threshold
        if self._engine2 is None:
            self._engine2 = Engine(self.img_h_new, self.img_w_new, **self._engine_kw)
            if self._engine2.shares_queue_with(self.engine):     # keep the two main streams on different hardware queues (see EngineRing)
                hs = (C.c_void_p * 2)(self.engine._h, self._engine2._h)
                self.engine._chk(self.engine._L.cf_spread_streams(hs, 2, 0, None))
        engs = (self.engine, self._engine2)
        nb = self.engine.max_batch

        def enqueue(e, chunk):
            chunk = [np.asarray(im, dtype=np.uint8) for im in chunk]
            e.set_rescale(self.scale_h, self.scale_w)
            try:
                frames, forward = self._input_form(e, chunk, fmt)
                forward(frames)
            except BaseException:
                e.set_rescale(0.0, 0.0)                  # the rescale is per-context state: a failed enqueue must not leave it behind
                raise

        def finish(e):
            try:
                return self._decode(e)
            finally:
                e.set_rescale(0.0, 0.0)
        it, k, pending = iter(imgs), 0, None
        while True:
            chunk = []
            for im in it:
                chunk.append(im)
                if len(chunk) == nb:
                    break
            if chunk:
                enqueue(engs[k & 1], chunk)
            if pending is not None:
                for r in finish(pending):
                    yield r
            if not chunk:
                return
            pending = engs[k & 1]
            k += 1

    def forward(self, x):
        return self.engine.forward(x)

    def decode_topk(self, K=100):
        return self.engine.decode_topk(K)

    # centerface.py:73-109 on explicit arrays
    def decode(self, heatmap, scale, offset, landmark, size, threshold=0.1):
        del offset, threshold       # read but unused / ignored by the reference (:77,:86-88)
        L = _lib.lib()
        hm = _lib.f32(np.asarray(heatmap).reshape((1, 1) + np.squeeze(heatmap).shape))
        h, w = hm.shape[2:]
        wh = _lib.f32(scale)
        lm = _lib.f32(landmark) if landmark is not None else np.zeros((1, 10, h, w), np.float32)
        def run(cap):
            dets, lms, cnt = np.empty((1, cap, 5), np.float32), np.empty((1, cap, 10), np.float32), np.zeros((1,), np.int32)
            _lib.check(L.cf_op_decode_threshold(self.device, _lib.ptr(hm), _lib.ptr(wh), _lib.ptr(lm), 1, h, w,
                                                int(size[0]), int(size[1]), 0.3, float(self.nms_thresh), cap,
                                                _lib.ptr(dets), _lib.ptr(lms), _lib.ptr(cnt)), op=True)
            return (dets, lms, int(cnt[0])), int(cnt[0])
        dets, lms, n = _grown(max(1, min(h * w, 4096)), run)
        if n == 0:
            return ([], []) if self.landmarks else []
        return (dets[0, :n].copy(), lms[0, :n].copy()) if self.landmarks else dets[0, :n].copy()

    # centerface.py:111-151
    def nms(self, boxes, scores, nms_thresh):
        L = _lib.lib()
        boxes, scores = _lib.f32(boxes), _lib.f32(scores)
        n = boxes.shape[0]
        keep = np.empty((max(n, 1),), np.int32)
        nk = C.c_int32()
        _lib.check(L.cf_op_nms(self.device, _lib.ptr(boxes), _lib.ptr(scores), n, float(nms_thresh),
                               _lib.ptr(keep), C.byref(nk)), op=True)
        return [int(k) for k in keep[:nk.value]]


# ---- page-locked caller memory ------------------------------------------------------------------------------------------
# Round 6.  Round 5 page-locked numpy HEAP memory in place (hipHostRegister on `im.copy()`, and on an aligned window of an np.empty
# array for pinned_empty).  That is what killed the driver's GPU run of round 5: the C library grows, trims and reuses its heap
# underneath a live registration, the registration's pages stop being the ones the GPU was given, and a later DMA from the array
# faults ("Memory access fault by GPU ... on address <heap address>": SIGABRT from the HSA runtime's event thread, no Python
# exception possible).  tools/diag/pin_churn_probe.py reproduces it in under a minute of allocation churn: 6 faults in 22 runs from heap
# memory, 1 in 6 even from whole pages inside a heap array, none from mmap regions or hipHostMalloc memory.  Hence:
#   * pinned_empty / pinned_copy hand out hipHostMalloc memory (cf_pinned_alloc) -- the library never registers numpy's heap;
#   * pin() only accepts whole pages of a mapping of its own (np.memmap / mmap / shared memory: a frame pool) and refuses the heap.
_pin_lock = threading.Lock()
_pin_bases, _pin_sizes = [], {}          # sorted base addresses / base -> bytes, of every page-locked range handed out or registered
_pin_ids = {}                            # id(array object handed out by pin / pinned_empty) -> its address (the per-image fast path)
_PAGE = 4096


def _track(addr, nbytes):
    with _pin_lock:
        bisect.insort(_pin_bases, addr)
        _pin_sizes[addr] = nbytes


def _untrack(addr):
    with _pin_lock:
        if _pin_sizes.pop(addr, None) is None:
            return False
        _pin_bases.remove(addr)
        return True


def _unregister(addr):
    if not _untrack(addr):
        return
    try:
        _lib.lib().cf_host_unregister(C.c_void_p(addr))
    except Exception:                                              # noqa: BLE001  (interpreter shutdown)
        pass


def _owner(arr):
    """The ndarray at the end of ``arr``'s .base chain: the object whose lifetime bounds the memory ``arr`` views."""
    o = arr
    while isinstance(o.base, np.ndarray):
        o = o.base
    return o


def _heap_range():
    """[lo, hi) of the C library's main heap (the ``[heap]`` line of /proc/self/maps), or None."""
    try:
        with open("/proc/self/maps") as f:
            for ln in f:
                if ln.rstrip().endswith("[heap]"):
                    lo, hi = ln.split()[0].split("-")
                    return int(lo, 16), int(hi, 16)
    except OSError:
        pass
    return None


def pin(arr):
    """Page-lock the memory of a C-contiguous numpy array IN PLACE (``cf_host_register``) and return it: batches taken from it
    reach the GPU by asynchronous DMA with no staging copy (``Engine.forward_images_enqueue``, ``CenterFaceBuckets``).  Only for
    memory that is a mapping of its own -- ``np.memmap``, ``mmap.mmap``, a shared-memory segment: a decoder's frame pool -- in whole
    pages: the address a multiple of 4096, the size too.  Arrays from ``np.empty`` / ``.copy()`` / ``cv2.imread`` live on the C
    library's heap and are REFUSED (ValueError): registering heap memory faults the GPU once the heap has been trimmed and regrown
    (the abort of GPUTEST_r05; see the comment above) -- copy such images into ``pinned_empty`` / ``pinned_copy`` buffers instead.
    ``unpin`` releases the registration; so does the garbage collection of the array that owns the memory (a finalizer on the
    owner unregisters the range before the mapping can go away)."""
    if not isinstance(arr, np.ndarray) or not arr.flags["C_CONTIGUOUS"] or arr.nbytes == 0:
        raise ValueError("pin needs a non-empty C-contiguous numpy array")
    addr, nbytes = arr.ctypes.data, arr.nbytes
    if addr % _PAGE or nbytes % _PAGE:
        raise ValueError("pin needs whole pages of a mapping of its own (address and size multiples of %d; got 0x%x, %d bytes): "
                         "numpy heap arrays cannot be page-locked in place -- use pinned_empty / pinned_copy" % (_PAGE, addr, nbytes))
    heap = _heap_range()
    if heap is not None and addr < heap[1] and addr + nbytes > heap[0]:
        raise ValueError("pin: the array lives on the C library's heap; page-locking heap memory in place faults the GPU when the heap "
                         "is trimmed and regrown -- use pinned_empty / pinned_copy")
    with _pin_lock:
        if addr in _pin_sizes:
            if _pin_sizes[addr] >= nbytes:
                return arr
            raise ValueError("a shorter range at the same address is already pinned")
        k = bisect.bisect_right(_pin_bases, addr) - 1
        lo_clash = k >= 0 and _pin_bases[k] + _pin_sizes[_pin_bases[k]] > addr
        hi_clash = k + 1 < len(_pin_bases) and _pin_bases[k + 1] < addr + nbytes
        if lo_clash or hi_clash:
            raise ValueError("the array overlaps a range that is already pinned (pin the enclosing array once)")
    owner = _owner(arr)
    _lib.check(_lib.lib().cf_host_register(C.c_void_p(addr), nbytes), op=True)
    _track(addr, nbytes)
    weakref.finalize(owner, _unregister, addr)                     # (a no-op after unpin: _unregister forgets the address first)
    _remember(arr)
    return arr


def _remember(arr):
    key = id(arr)
    _pin_ids[key] = arr.ctypes.data
    weakref.finalize(arr, _pin_ids.pop, key, None)


def _direct_addr(im):
    """Address of a page-locked C-contiguous uint8 array, else None (one dict probe for the objects pin / pinned_empty returned)."""
    if type(im) is not np.ndarray or im.dtype != np.uint8:
        return None
    addr = _pin_ids.get(id(im))
    if addr is not None and im.flags.c_contiguous:
        return addr
    return im.ctypes.data if is_pinned(im) else None


def unpin(arr):
    """Release a ``pin`` registration (``pinned_empty`` memory is released with its last view instead)."""
    _pin_ids.pop(id(arr), None)
    _unregister(arr.ctypes.data)


class _PinnedBlock(object):
    """One hipHostMalloc allocation (``cf_pinned_alloc``) exposed through the array interface; freed when the last numpy view of it
    is gone (numpy keeps this object as the .base of every view)."""

    def __init__(self, nbytes):
        p = C.c_void_p()
        _lib.check(_lib.lib().cf_pinned_alloc(int(nbytes), C.byref(p)), op=True)
        self.addr, self.nbytes = p.value, int(nbytes)
        self.__array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.addr, False), "version": 3}
        _track(self.addr, self.nbytes)

    def __del__(self):
        addr, self.addr = getattr(self, "addr", None), None
        if addr:
            _untrack(addr)
            try:
                _lib.lib().cf_pinned_free(C.c_void_p(addr))
            except Exception:                                      # noqa: BLE001  (interpreter shutdown)
                pass


def pinned_empty(shape, dtype=np.uint8):
    """``np.empty`` in page-locked host memory (hipHostMalloc through ``cf_pinned_alloc``; released when the array and its views are
    gone): images written here reach the GPU by asynchronous DMA with no staging copy."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    block = _PinnedBlock(max(n, 1))
    out = np.asarray(block)[:n].view(dtype).reshape(shape)
    _remember(out)
    return out


def pinned_copy(arr):
    """A copy of ``arr`` in page-locked memory (``pinned_empty`` + one host copy): for images that arrive in pageable memory
    (``cv2.imread``, a decoder) and are used more than once."""
    arr = np.asarray(arr)
    out = pinned_empty(arr.shape, arr.dtype)
    np.copyto(out, arr)
    return out


def is_pinned(arr):
    """True when the array's bytes lie inside a range registered by ``pin`` or handed out by ``pinned_empty``."""
    if not isinstance(arr, np.ndarray) or not arr.flags["C_CONTIGUOUS"]:
        return False
    addr = arr.ctypes.data
    with _pin_lock:
        k = bisect.bisect_right(_pin_bases, addr) - 1
        return k >= 0 and addr + arr.nbytes <= _pin_bases[k] + _pin_sizes[_pin_bases[k]]


_copy_pool, _copy_pool_lock = None, threading.Lock()


def _stage_copy_begin(stage, images, background=False):
    """Host images -> rows of a page-locked staging array; returns a function that waits for the copy.  The copy is the largest
    host cost of a mixed-size batch (118 MB for 128 VGA images: 5 of 9 ms on one core).  numpy releases the GIL while it copies,
    so a few worker threads (one task per worker: a submit costs ~25 us of Python) move it faster -- and, with ``background``,
    entirely off the calling thread, which collects the results of an earlier chunk meanwhile.  Small jobs are copied at once."""
    global _copy_pool
    total = sum(int(np.asarray(im).nbytes) for im in images)
    workers = min(int(os.environ.get("CF_STAGE_THREADS", "4")), os.cpu_count() or 1, len(images))
    if total < (4 << 20) or workers < 2:
        for k, im in enumerate(images):
            np.copyto(stage[k], np.asarray(im, dtype=np.uint8))
        return lambda: None
    with _copy_pool_lock:
        if _copy_pool is None:
            from concurrent.futures import ThreadPoolExecutor
            _copy_pool = ThreadPoolExecutor(max_workers=max(2, min(int(os.environ.get("CF_STAGE_THREADS", "4")), os.cpu_count() or 1)),
                                            thread_name_prefix="cf-stage")

    def copy_slice(k0):
        for k in range(k0, len(images), workers):
            np.copyto(stage[k], np.asarray(images[k], dtype=np.uint8))
    futs = [_copy_pool.submit(copy_slice, k0) for k0 in range(0 if background else 1, workers)]
    if not background:
        copy_slice(0)                                              # the calling thread takes a share

    def wait():
        for f in futs:
            f.result()                                             # re-raises a worker's exception (shape mismatch, ...)
    return wait


class CenterFaceBuckets(object):
    """Variable-size input (BASELINE configs[3]: WIDER-style images of different shapes in one batch).

    The reference builds one ``CenterFace(h, w)`` per image shape (demo.py:76 even per image).  Here images are
    bucketed by their NETWORK shape ``transform(h, w)[:2]`` (multiples of 32, centerface.py:68-71): every bucket
    owns one ``Engine`` (one cf_ctx on the GPU, created on first use, all sharing the same weights, graphs
    reused), so all raw sizes that round up to the same network shape share a context.  Inside a bucket the
    images of one raw size run as full ``forward_resized`` batches (the device resize takes one source size per
    launch); the floor-division rescale uses each image's own ``scale_h`` / ``scale_w``.  Results come back in
    the order of ``imgs``; every image gets exactly what ``CenterFace(h, w)(img)`` returns for it."""

    def __init__(self, landmarks=True, *, weights=None, dtype="fp32", device=0, max_batch=32, max_buckets=8,
                 nms_thresh=0.3, max_dets=1024, collapse_heads=None, flip_test=False):
        self.landmarks, self.dtype, self.device, self.max_batch, self.max_buckets = landmarks, dtype, device, max_batch, max_buckets
        self.flip_test = bool(flip_test)        # every bucket's engine runs the flip test (Engine(flip_test=True))
        self.nms_thresh, self.max_dets, self.collapse_heads = nms_thresh, max_dets, collapse_heads
        self._weights = _weights.synthetic_state_dict(0) if weights is None else (
            _weights.load_checkpoint(weights) if isinstance(weights, str) else weights)
        self._buckets = {}          # network (H, W) -> Engine, in least-recently-used order
        self.created = 0            # contexts created so far (tests: raw sizes sharing a network shape share one)

    def _engine(self, H, W):
        key = (int(H), int(W))
        eng = self._buckets.pop(key, None)
        if eng is None:
            if len(self._buckets) >= self.max_buckets:             # evict the least recently used context
                old = next(iter(self._buckets))
                self._buckets.pop(old).close()
            eng = Engine(H, W, max_batch=self.max_batch, dtype=self.dtype, device=self.device, weights=self._weights, decode_stream=False,
                         collapse_heads=self.collapse_heads, flip_test=self.flip_test)
            self.created += 1
            self._placement_dirty = True
        self._buckets[key] = eng
        return eng

    def _staging(self, eng, n, h, w):
        """Page-locked staging view [n, h, w, 3] into the engine's ONE grow-only pinned buffer (sized to the largest
        n * h * w * 3 seen).  A WIDER-style run has hundreds of distinct raw sizes and tail lengths: one pinned array per
        (n, h, w) would pile up GBs of page-locked memory, each allocation a device-synchronising hipHostMalloc.  Reuse
        is safe: an engine stages one chunk per round and the round ends with its decode_threshold (a synchronise)."""
        need = int(n) * int(h) * int(w) * 3
        st = eng.__dict__.get("_stage")
        if st is None or st[1] < need:
            if st is not None:
                eng.synchronize()
                eng.pinned_free(st[0])
            cap = max(need, int(1.25 * st[1]) if st is not None else need)
            eng.__dict__["_stage"] = st = eng.pinned_raw(cap)
        buf = (C.c_char * need).from_address(st[0].value)
        return np.frombuffer(buf, dtype=np.uint8, count=need).reshape(n, h, w, 3)

    def detect(self, imgs, threshold=0.2):
        del threshold                                              # ignored by the reference's decode (centerface.py:77)
        groups = {}                                                # network shape -> raw shape -> indices
        net = self.__dict__.setdefault("_net_shape", {})           # raw (h, w) -> network (H, W): transform() once per size
        addrs = []                                                 # per image: address if page-locked uint8 (pin / pinned_empty), else None
        for i, im in enumerate(imgs):
            hw = im.shape[:2] if type(im) is np.ndarray else np.asarray(im).shape[:2]
            HW = net.get(hw)
            if HW is None:
                HW = net[hw] = CenterFace.transform(None, hw[0], hw[1])[:2]
            groups.setdefault(HW, {}).setdefault(hw, []).append(i)
            addrs.append(_direct_addr(im))
        out = [None] * len(imgs)
        post = CenterFace.__new__(CenterFace)                      # only for _postprocess (no engine of its own)
        post.landmarks = self.landmarks
        keys = list(groups)
        for g0 in range(0, len(keys), self.max_buckets):           # at most max_buckets contexts alive at a time (LRU eviction)
            self._run_buckets({k: groups[k] for k in keys[g0:g0 + self.max_buckets]}, imgs, out, post, addrs)
        return out

    def _run_buckets(self, groups, imgs, out, post, addrs):
        # one work list per bucket (engine): chunks of one raw size, at most max_batch images
        work = []
        for (H, W), raws in groups.items():
            eng = self._engine(H, W)
            work.append([eng, [((h, w), idx[j:j + eng.max_batch]) for (h, w), idx in raws.items()
                               for j in range(0, len(idx), eng.max_batch)]])
        # New contexts since the last call: put the main streams on dispatch pipes such that contexts used one after the other never share
        # one (cf_spread_streams, window 2).  A process's queues offer three or four pipes; five contexts as the runtime places them had
        # three on one pipe (contexts 0, 3, 4), so the forwards of chunks 3 and 4 took turns kernel by kernel: 31.0 -> 33.9-35.4 k img/s on
        # the configs[3] mix with (0, 3) (1, 4) (2) instead.  Costs ~15 ms, once per new context.
        if self.__dict__.pop("_placement_dirty", False) and len(self._buckets) >= 2:
            engs = list(self._buckets.values())
            hs = (C.c_void_p * len(engs))(*[e._h for e in engs])
            engs[0]._chk(engs[0]._L.cf_spread_streams(hs, len(engs), 2, None))
        # Software pipeline over the chunks, taken round-robin over the buckets, on TWO host threads: this thread copies chunk i into
        # its context's page-locked buffer (with the staging threads) and enqueues it (asynchronous DMA + resize + forward on that
        # context's own streams); a collector thread waits for the oldest chunk in flight (decode_threshold: the wait happens inside
        # the C call, without the GIL), copies its results out and rescales them.  Round 3 did both on one thread and was host-bound
        # (6.3 ms per 128 images of which the device needs 4.2: profiles/r04_depth_sweep.txt).  A context has one staging buffer and
        # one decode state, so its previous chunk is collected before its next one is staged (the future of that chunk).
        order = []
        while any(chunks for _, chunks in work):
            for eng, chunks in work:
                if chunks:
                    order.append((eng,) + chunks.pop(0))

        def collect(item):
            eng, (h, w), idx = item
            pp = CenterFace.__new__(CenterFace)                    # only the reference's empty-result shapes are left to the host
            pp.landmarks = post.landmarks
            try:
                res = pp._postprocess_many(eng.decode_threshold(0.3, self.nms_thresh, self.max_dets), rescaled=True)
            finally:
                eng.set_rescale(0.0, 0.0)
            for i, r in zip(idx, res):
                out[i] = r

        collector = self.__dict__.get("_collector")
        if collector is None:
            from concurrent.futures import ThreadPoolExecutor
            collector = self.__dict__["_collector"] = ThreadPoolExecutor(max_workers=1, thread_name_prefix="cf-collect")
        last, futs = {}, []
        main_exc = None
        # Page-locked chunks are uploaded AHEAD: the copies of the next chunks (one per context at most) are enqueued before the
        # forward of this one, so the device's copy queue holds nothing but copies back to back and never stands behind a forward.
        direct = [all(addrs[i] is not None for i in idx) for _, _, idx in order]
        uploaded, up_next = {}, 0              # id(engine) -> index into ``order`` of the chunk whose copies are enqueued

        def upload_ahead(k):
            # the copies of chunks k, k+1, ... in order, while they are page-locked and their context has no upload waiting
            nonlocal up_next
            up_next = max(up_next, k)
            while up_next < len(order) and up_next <= k + len(work):
                e2, hw2, idx2 = order[up_next]
                if not direct[up_next] or id(e2) in uploaded:
                    return
                # calls on ONE context are serialised by the caller (include/centerface_hip.h): the collector thread may still be inside
                # this context's decode of its previous chunk -- no upload ahead into it until that chunk has been collected
                busy = last.get(id(e2))
                if busy is not None and not busy.done():
                    return
                e2._upload_addrs([addrs[i] for i in idx2], hw2[0], hw2[1], [imgs[i] for i in idx2])
                uploaded[id(e2)] = up_next
                up_next += 1
        try:
            for k, item in enumerate(order):
                eng, (h, w), idx = item
                prev = last.get(id(eng))
                if prev is not None:
                    prev.result()                                  # this context's earlier chunk has been collected
                eng.set_rescale(eng.H / h, eng.W / w)              # this chunk's scale_h, scale_w (centerface.py:68-71)
                if direct[k]:
                    upload_ahead(k)                                # (a no-op when an earlier step has uploaded this chunk already)
                    if uploaded.pop(id(eng), None) != k:
                        raise RuntimeError("CenterFaceBuckets: upload order lost track of chunk %d" % k)
                    eng.forward_uploaded()                         # page-locked images (pin / pinned_empty): DMA straight from them
                    upload_ahead(k + 1)                            # (after the forward: a context holds ONE upload at a time)
                else:
                    chunk = [imgs[i] for i in idx]
                    stage = self._staging(eng, len(idx), h, w)
                    _stage_copy_begin(stage, chunk)()
                    if (h, w) == (eng.H, eng.W):
                        eng.forward_enqueue(stage)
                    else:
                        eng.forward_resized_enqueue(stage)
                eng.decode_threshold_enqueue(0.3, self.nms_thresh, self.max_dets)       # decode + NMS run as soon as the forward is done
                f = collector.submit(collect, item)                # FIFO on one worker: collected in enqueue order
                last[id(eng)] = f
                futs.append(f)
        except BaseException as exc:                               # noqa: BLE001  (re-raised below, after the drain)
            main_exc = exc
        # drain even when staging / enqueue raised: no chunk stays in flight.  The exception of this thread wins; a collector
        # failure is raised only when nothing else is propagating (and is not re-raised a second time when it already surfaced
        # through prev.result() above).
        err = None
        for f in futs:
            try:
                f.result()
            except Exception as exc:                               # noqa: BLE001
                err = err or exc
        if main_exc is not None or err is not None:
            for eng, _ in work:                                    # the rescale is per-context state: never left behind by a failed chunk
                try:
                    eng.set_rescale(0.0, 0.0)
                except Exception:                                  # noqa: BLE001
                    pass
        if main_exc is not None:
            if err is not None and err is not main_exc:
                raise main_exc from err
            raise main_exc
        if err is not None:
            raise err

    __call__ = detect

    def close(self):
        col = self.__dict__.pop("_collector", None)
        if col is not None:
            col.shutdown(wait=True)
        for eng in self.__dict__.get("_buckets", {}).values():
            eng.close()
        self._buckets = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()                                           # the collector thread does not outlive the object
        except Exception:                                          # noqa: BLE001
            pass
