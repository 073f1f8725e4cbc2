/*
 * centerface_hip.h -- C ABI of libcenterface_hip.so: the MI355X (gfx950) CenterFace inference hot path.
 *
 * The reference has no FFI: its boundary is the Python class in centerface.py.  Every entry point
 * below names the reference code it replaces; INTEGRATION.md shows the ctypes stub a maintainer of
 * the reference would add to centerface.py to route through this library.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types cross the boundary (device pointers travel as void*).
 *   - every function returns 0 (CF_OK) or a negative CF_E* code; cf_last_error(ctx) gives the text.
 *     The library never aborts and never falls back to a CPU path.
 *   - one cf_ctx = one GPU + its own HIP streams (forward, decode, input copy), buffers and graphs; calls on a ctx are
 *     serialised by the caller; different ctxs may be driven from different threads / processes (one process per GPU
 *     for multi-GPU; two ctxs on one GPU used alternately keep two batches in flight).
 *   - host outputs are written into CALLER-ALLOCATED buffers; nothing allocated here crosses back.
 *   - activations live in HBM as NHWC (channels contiguous), fp32 or bf16 storage, fp32 accumulate.
 */
#ifndef CENTERFACE_HIP_H
#define CENTERFACE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CF_VERSION 100           /* 0.1.0 */

/* error codes */
#define CF_OK             0
#define CF_EINVAL        -1      /* bad argument (shape not multiple of 32, K > h*w, ...) */
#define CF_ENOMEM        -2
#define CF_EHIP          -3      /* a HIP runtime call failed; see cf_last_error */
#define CF_ESTATE        -4      /* call order violated (forward before load_weights, ...) */
#define CF_ESCHEMA       -5      /* weight set does not match the 94-tensor checkpoint schema */
#define CF_EOVERFLOW     -6      /* candidate capacity exceeded in threshold decode */

/* storage dtype of activations and packed weights (accumulation is always fp32) */
#define CF_F32   0               /* parity mode: fp32 storage, exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) */
#define CF_BF16  1               /* throughput mode: bf16 storage, bf16 MFMA, fp32 accumulate */
#define CF_F32_SPLIT 2           /* tolerance mode: fp32 storage, every GEMM product as a split-bf16 ("bf16x3") product on the bf16
                                  * matrix pipe (hi.hi + lo.hi + hi.lo, fp32 accumulate): within north_star's 1e-3 of the reference
                                  * like CF_F32 (products exact to ~2^-16 relative), several times its speed */

/* network input formats accepted by cf_forward */
#define CF_IN_U8_HWC_BGR  0      /* uint8 [B,H,W,3] BGR, as cv2 gives it; /255, -mean, /std fused
                                    into the stem (replaces centerface.py:32-37) */
#define CF_IN_F32_NCHW    1      /* float [B,3,H,W], already normalised: the tensor the reference
                                    hands to net() at centerface.py:41 / eval_widerface.py:83 */

/* cf_create flags */
#define CF_FLAG_COLLAPSE_HEADS  1u   /* fold each head's conv3x3+b -> conv1x1+b (a linear pair,
                                        model/centernet.py:249-256) into one 3x3 conv 24->15 */
#define CF_FLAG_NO_GRAPH        2u   /* launch kernels eagerly instead of replaying a hipGraph */
#define CF_FLAG_NO_FUSE         4u   /* run every MBConv block as three kernels (expand, dw, project)
                                        instead of the fused kernel that keeps the 6x tensor in LDS */
#define CF_FLAG_NO_UPHEAD       8u   /* keep the last IDAUp stage and the heads as two kernels (bf16 +
                                        collapsed heads fuse them, the neck output stays in LDS) */
#define CF_FLAG_NO_NECK        16u   /* keep conv_last and the first two IDAUp stages as three kernels (bf16 fuses them
                                        into one: the 1/32 and 1/16 neck maps stay in LDS) */
#define CF_FLAG_NO_DECODE_STREAM 32u  /* device-output decodes (cf_decode_topk, cf_gather_topk) run on the context's main stream instead of a
                                      * decode stream of its own.  For hosts that keep THREE OR MORE contexts in flight (small batches):
                                      * HIP has four hardware queues per process, and three main + three decode streams share them
                                      * (configs[4] shard, B = 4: 3 contexts 9.5 k img/s with decode streams, 12.2 k without; 2 contexts 11.3 k) */
#define CF_FLAG_STREAM_HIGH 64u       /* the context's main and decode streams are created in the HIGHEST stream-priority class.  The HIP runtime
                                      * keeps one pool of (four) hardware queues per priority class and gives a new stream the least-used queue of its
                                      * class, so streams in a class of their own are placed independently of everything the process created in the
                                      * default class: 54.3-54.5 k img/s for two contexts from five different process histories, against 48.2-54.4 k
                                      * for default-class streams as created (round 6, tools/queue_order_probe.py).  The class is shared with the
                                      * device's copy stream and with this library's earlier contexts: after contexts have been destroyed in it the
                                      * map is no longer the same (45.7-47.8 k, tools/ring_sequence_probe.py) -- for a host that creates its contexts
                                      * once; cf_streams_share_queue_ex / cf_spread_streams verify and repair a placement in any history. */

typedef struct cf_ctx cf_ctx;

/* One checkpoint tensor, exactly as torch.save(model.state_dict()) holds it (train.py:165):
 * conv weights OIHW float32; num_batches_tracked may be passed (int64) and is ignored. */
typedef struct cf_tensor_desc {
    const char* name;            /* state_dict key, e.g. "layer1.0.conv.1.1.weight" */
    const void* data;            /* host pointer */
    int32_t     ndim;
    int64_t     dims[4];
    int32_t     dtype;           /* 0 = float32, 1 = int64 */
} cf_tensor_desc;

int         cf_version(void);
const char* cf_strerror(int code);
const char* cf_last_error(const cf_ctx* ctx);          /* ctx may be NULL: last create error */
int         cf_device_count(int* n);

/* ---- lifetime: replaces CenterFace.__init__ (centerface.py:16-27) -------------------------- */
/* H, W must be multiples of 32 (CenterFace.transform guarantees it, centerface.py:69). */
int cf_create(int device, int max_batch, int H, int W, int dtype, uint32_t flags, cf_ctx** out);
int cf_destroy(cf_ctx* ctx);
/* strict load of the 94-tensor state_dict (centerface.py:23-24): validates names and shapes,
 * folds BatchNorm (eval mode, centerface.py:25), repacks to kernel layouts, uploads. */
int cf_load_weights(cf_ctx* ctx, const cf_tensor_desc* tensors, int n);

/* ---- training-side pieces that share the detector's tensors (forward evaluation only) ----------------- */
/* CtdetLoss.forward (model/losses.py:347-374: focal loss :142-167 on clamp(sigmoid(hm), 1e-5, 1-1e-5),
 * RegL1Loss :239-250 on wh / reg / lm gathered at ind) evaluated on the head maps of the LAST cf_forward of
 * ctx.  Targets are host arrays as dataset/dataset.py:223-226 returns them: gt_hm [B,1,h,w] f32,
 * reg_mask / lm_mask [B,M] u8, ind / lm_ind [B,M] i64, wh_t / reg_t [B,M,2], lm_t [B,M,10].
 * weights = {hm_w, wh_w, off_w, lm_w} (reference defaults 1, 0.1, 1, 1).  out[5] = loss, hm_loss, wh_loss,
 * off_loss, lm_loss.  Blocking. */
int cf_ctdet_loss(cf_ctx* ctx, const float* gt_hm, const uint8_t* reg_mask, const int64_t* ind, const float* wh_t,
                  const float* reg_t, const uint8_t* lm_mask, const int64_t* lm_ind, const float* lm_t,
                  int max_objs, const float* weights4, float* out5);

/* ---- forward: replaces net(img)[0] (centerface.py:41, eval_widerface.py:83-84) ------------- */
/* `in` is a host pointer (in_on_device = 0; copied H2D on a copy stream into one of two staging buffers, so the
 * copy overlaps the previous forward -- keep the buffer unchanged until a blocking call on this context has
 * returned: cf_synchronize, cf_get_heads or a decode with host outputs) or a device pointer on
 * ctx's GPU (in_on_device = 1; 4-byte aligned -- CF_EINVAL otherwise).  Asynchronous: returns after
 * enqueueing. */
int cf_forward(cf_ctx* ctx, const void* in, int in_format, int in_on_device, int B);
/* cv2.resize + forward in one enqueue (centerface.py:30-41): imgs uint8 [B,h,w,3] BGR of ANY size are
 * stretch-resized on the device to the ctx's (H, W) with OpenCV's fixed-point INTER_LINEAR arithmetic for uint8
 * (11-bit coefficients, int32 passes; csrc/cf_util.hip restates it) and fed to the network.  Pinned to the
 * published algorithm, not to a particular cv2 binary (cv2 is not installable where this was built). */
int cf_forward_resized(cf_ctx* ctx, const void* imgs_u8, int in_on_device, int B, int h, int w);
/* The same for a batch held as B SEPARATE host images, imgs[b] -> uint8 [h,w,3] BGR -- what the loop of eval_widerface.py:76-90
 * has after B cv2.imread calls.  Every image is one asynchronous DMA into the context's buffer ((h, w) == (H, W): straight into
 * the network input, no resize launch).  From page-locked memory (cf_host_alloc, cf_host_register) there is no host-side
 * staging copy at all; pageable pointers work too, but then the call returns only once the runtime has staged them.  The images
 * must stay unchanged until a blocking call on ctx has returned (as for cf_forward). */
int cf_forward_images(cf_ctx* ctx, const void* const* imgs, int B, int h, int w);
/* The two halves of cf_forward_images: cf_upload_images only enqueues the host -> device copies (large batches: on the device's
 * copy streams, shared by every context of the process, in call order), cf_forward_uploaded enqueues resize + forward on what the
 * last cf_upload_images of ctx brought over (CF_ESTATE without one; any other upload or forward on ctx in between replaces it).
 * A host that keeps several contexts in flight issues the uploads of the next batches BEFORE the forwards of the earlier ones, so
 * that the copy queue never stands behind a forward (CenterFaceBuckets: 5 contexts, 128 VGA images, profiles/r05_vga_pipeline.md). */
int cf_upload_images(cf_ctx* ctx, const void* const* imgs, int B, int h, int w);
int cf_forward_uploaded(cf_ctx* ctx);
/* ---- 4:2:0 video frames: cv2.cvtColor(frame, COLOR_YUV2BGR_<fmt>) on the device, then the network ------------------- */
#define CF_YUV_NV12 0            /* Y plane, then one interleaved U,V plane (what hardware decoders emit) */
#define CF_YUV_NV21 1            /* Y plane, then one interleaved V,U plane */
#define CF_YUV_I420 2            /* Y, U, V planes (yuv420p: what software decoders emit) */
#define CF_YUV_YV12 3            /* Y, V, U planes */
#define CF_FRAME_BGR 4           /* uint8 [h,w,3] BGR rows: with CF_YUV_* the one `format` integer of cf_redact_faces (not a cf_forward_yuv format) */
typedef struct cf_yuv_planes {
    const void* y;               /* h rows of y_pitch bytes */
    const void* c0;              /* first chroma plane in the format's order: NV12 / NV21 the interleaved plane, I420 U, YV12 V
                                    (h/2 rows of c_pitch bytes) */
    const void* c1;              /* second chroma plane (I420 V, YV12 U); NULL for NV12 / NV21 */
} cf_yuv_planes;
/* B frames of h x w (both even, >= 2) in format yuv_format (CF_YUV_*), frames[b] = the planes of frame b: converted to uint8 BGR
 * with OpenCV's fixed-point BT.601 limited-range arithmetic (COLOR_YUV2BGR_NV12 / _NV21 / _I420 / _YV12; restated in csrc/cf_yuv.hip
 * from the published algorithm, not pinned to a cv2 binary), stretch-resized to the ctx's (H, W) like cf_forward_resized when
 * (h, w) differs, and fed to the network: every result equals that of the BGR frames through cf_forward / cf_forward_resized.
 * y_pitch >= w, c_pitch >= w (NV12 / NV21) or w/2 (I420 / YV12), in bytes.  Host frames (in_on_device = 0) are copied into a
 * device staging buffer: ONE DMA when the batch is one dense block of OpenCV's [h*3/2, w] frames (y_pitch = w, c_pitch = the
 * chroma row), else one pitched 2-D copy per plane per frame; keep them unchanged until a blocking call on ctx has returned.
 * Device frames (in_on_device = 1) are read in place; their plane addresses and pitches must be multiples of 4.  CF_EINVAL for
 * any bad argument, before anything is enqueued.  Asynchronous. */
int cf_forward_yuv(cf_ctx* ctx, int yuv_format, const cf_yuv_planes* frames, int in_on_device, int B, int h, int w,
                   int y_pitch, int c_pitch);
/* the uint8 [B,H,W,3] BGR batch the network read in the last cf_forward_resized or cf_forward_yuv (resized / converted; tests) */
int cf_get_resized_input(cf_ctx* ctx, void* out_u8, int B);
/* copies the four head maps of the last forward to host as NCHW float32: hm [B,1,h,w] raw logits
 * (what net() returns), wh [B,2,h,w], lm [B,10,h,w], reg [B,2,h,w]; h=H/4, w=W/4 (model/centernet.py
 * :277-280).  Any pointer may be NULL.  hm_sigmoid (optional) receives clamp(sigmoid(hm),1e-4,1-1e-4)
 * (centerface.py:43).  Synchronises. */
int cf_get_heads(cf_ctx* ctx, float* hm, float* wh, float* lm, float* reg, float* hm_sigmoid);

/* ---- decode D3: replaces ctdet_decode / _nms / _topk / _transpose_and_gather_feat
 *      (centerface_ext.py:11-82) on the last forward's heads --------------------------------- */
/* dets [B,K,6] = x1,y1,x2,y2,score,cls in heat-map units; lms [B,K,10] raw landmark rows at the
 * same cells (may be NULL); inds [B,K] flat cell index y*w+x (may be NULL).  Equal scores are
 * ordered lower-index-first (torch.topk leaves it unspecified).  use_reg = 0 gives the +0.5
 * branch (centerface_ext.py:65-67).  out_on_device selects host or device destination buffers.
 * 1 <= K <= h*w, any map size (K > 1024 sorts through global memory: slower, same results). */
int cf_decode_topk(cf_ctx* ctx, int K, int use_reg, float* dets, float* lms, int64_t* inds,
                   int out_on_device);

/* Same, followed by ctdet_post_process (utils/post_process.py:83-100): both box corners are mapped
 * from heat-map coordinates back to source-image coordinates with the inverse affine of
 * get_affine_transform(center, scale, rot=0, (out_w, out_h), inv=1) (utils/image.py:19-66), fused into
 * the decode kernel's epilogue.  centers [B,2] (c[i]), scales [B,2] (s[i]; [0] is used, as the
 * reference does), out_w/out_h = heat-map size.  cv2.getAffineTransform is replaced by a float64
 * 3-point solve. */
int cf_decode_topk_post(cf_ctx* ctx, int K, int use_reg, const float* centers, const float* scales,
                        int out_w, int out_h, float* dets, float* lms, int64_t* inds, int out_on_device);
/* the 2x3 float64 matrix used above (row-major), for callers that want transform_preds themselves */
int cf_affine_from_center_scale(float cx, float cy, float scale_w, int out_w, int out_h, double* trans6);

/* ---- decode D1: replaces CenterFace.decode + nms (centerface.py:73-151) -------------------- */
/* For each image: cells with hm > score_thresh in row-major order, boxes/landmarks with the
 * reference's arithmetic (offsets ignored, x2 = min(x1c + w, W)), greedy IoU >= nms_thresh
 * suppression in descending score order.  dets [B,max_out,5], lms [B,max_out,10] (may be NULL),
 * counts [B] = number of boxes that survive NMS (in the reference's keep order); only the first max_out
 * rows are written, so counts[b] > max_out tells the caller that image b was truncated (call again with a
 * larger max_out).  Any number of cells above the threshold is accepted, as in the reference: the candidate
 * workspace grows to the largest count seen (CF_ENOMEM if that does not fit).  Host buffers.
 * The reference ignores its `threshold` argument and uses 0.3 (centerface.py:77); pass 0.3f. */
int cf_decode_threshold(cf_ctx* ctx, float score_thresh, float nms_thresh, int max_out,
                        float* dets, float* lms, int32_t* counts);

/* mode 0 = the above (D1); mode 1 = D2, eval_widerface.decode (eval_widerface.py:92-110): the threshold
 * argument is honoured and the offsets are added -- reg channel 1 to x and channel 0 to y plus the
 * 0.5, exactly as that file does (:102-104) -- no landmarks; same greedy NMS (:112-152). */
int cf_decode_threshold_ex(cf_ctx* ctx, int mode, float score_thresh, float nms_thresh, int max_out,
                           float* dets, float* lms, int32_t* counts);

/* Same with an explicit clamp size: the reference's get_detections clamps boxes to a hard-coded (640, 640)
 * whatever the input size (eval_widerface.py:88); cf_decode_threshold[_ex] clamp to the context's (H, W). */
int cf_decode_threshold_sized(cf_ctx* ctx, int mode, float score_thresh, float nms_thresh, int img_h, int img_w,
                              int max_out, float* dets, float* lms, int32_t* counts);
/* centerface.py:55-62 on the device: from now on the threshold decodes of ctx write floor(x / scale_w) and floor(y / scale_h) for
 * the box corners and the landmark points (numpy's float32 `//`: the exact floor of the quotient), so the host has nothing left to
 * do per box.  scale_h = scale_w = 0 switches it off (the default: network coordinates).  CF_EINVAL for negative / mixed values. */
int cf_set_rescale(cf_ctx* ctx, float scale_h, float scale_w);
/* Optional asynchronous first half: enqueue the decode kernels right behind the last forward, no host wait.  A later
 * cf_decode_threshold_sized (or _ex / plain, which call it) with the SAME parameters then only waits and copies the results out;
 * with other parameters, or after another forward, it launches its own decode as usual.  For hosts that keep several contexts
 * in flight and collect them later (CenterFaceBuckets): the decode runs when the forward finishes, not when the host gets there. */
int cf_decode_threshold_enqueue(cf_ctx* ctx, int mode, float score_thresh, float nms_thresh, int img_h, int img_w, int max_out);

/* ---- flip test: the batch and its mirror in one forward, the heads merged on the device ---------------------------------------- */
/* The reference trains on mirrored images half of the time (dataset/dataset.py:125-128 mirrors the image, :166-174 the boxes and the
 * landmark x values, and swaps the left and right points 0 <-> 1 and 3 <-> 4) and carries CenterNet's flip test for inference
 * (centerface_ext.py:162-163 concatenates the batch with its mirror; model/losses.py:94-116 flip_tensor / flip_lr / flip_lr_off put the
 * mirrored maps back).  cf_set_flip_test(ctx, 1) switches ctx to it; 0 (the default) switches it off; any other value is CF_EINVAL, as
 * is 1 on a context with max_batch < 2.  No trained weights and no labelled set are on hand: no accuracy claim is made.  The cost is
 * about one forward at 2B instead of one at B, plus the two kernels below.
 *
 * While it is on, every forward entry point -- cf_forward, cf_forward_resized, cf_forward_images / cf_upload_images /
 * cf_forward_uploaded, cf_forward_yuv, cf_forward_tiles (B = the tile count Bf * T), cf_forward_fit, and the forward inside
 * cf_detect_topk -- accepts B <= max_batch / 2 (CF_EINVAL above that, before anything is enqueued) and runs
 *     mirror -> the plan over 2B images -> merge
 * on the context's stream: image B + b of the network input is image b with its columns reversed (csrc/cf_flip.hip writes it on the
 * device; there is no second host-to-device copy), and ONE kernel folds the two halves of the head records into the first before
 * anything reads them.  The context then holds B images (cf_get_heads, every decode, cf_merge_tiles, cf_unfit_rows, the tracker,
 * redact, blur, draw, chips and best shots work unchanged on the merged heads); cf_align_faces and cf_get_resized_input see the
 * unmirrored images.  Results are the same with and without CF_FLAG_NO_GRAPH.  cf_forward_trace and cf_profile_forward (and the
 * experiments build's cf_forward_lanes) return CF_ESTATE while it is on.  A context that never switches it on allocates nothing for it;
 * the first flip forward of a caller's device tensor or a host batch of the network's size allocates a second input buffer.
 *
 * THE MERGE.  All arithmetic is float32, in the order written.  The head records are rec [.][h][w][16] float32:
 *     r[0] = clamp(sigmoid(hm)), r[1..2] = wh, r[3..12] = lm as x, y of points 0 .. 4, r[13..14] = reg, r[15] = the raw hm logit,
 * and hm_plane [.][h * w] is the dense copy of r[0] that the decodes scan.  For b < B and cell (y, x) let
 *     a = rec[b][y][x],   m = rec[B + b][y][w - 1 - x],   p = (1, 0, 2, 4, 3).
 * Then
 *     out[0]      = (a[0] + m[0]) * 0.5f                      the heat, after sigmoid and clamp, as CenterNet averages it
 *     out[1]      = (a[1] + m[1]) * 0.5f
 *     out[2]      = (a[2] + m[2]) * 0.5f                      wh
 *     out[3 + 2j] = (a[3 + 2j] - m[3 + 2 p[j]]) * 0.5f        x of point j = 0 .. 4
 *     out[4 + 2j] = (a[4 + 2j] + m[4 + 2 p[j]]) * 0.5f        y of point j
 *     out[13..14] = a[13..14]                                  reg of the unmirrored pass only, as CenterNet does
 *     out[15]     = (a[15] + m[15]) * 0.5f                    the MEAN LOGIT of the two passes, NOT the logit of out[0]
 * out overwrites rec[b][y][x], and hm_plane[b][y * w + x] = out[0].  A landmark x is an offset from the cell centre in map units: in
 * the unmirrored frame the mirrored pass's point lies at x + 0.5 - lx', hence the minus; the pairs change places because the training
 * data swaps them.
 *
 * Worked example, B = 1, h = 1, w = 2 (every value is exact in float32):
 *     rec[0][0][0] = a  = ( 0.75, 4,  6,   1, -2,   3,  0.5,  -1, 2.5,  5, -3,  0.25,  8,  0.125, 0.875,  1.5)
 *     rec[1][0][1] = m  = ( 0.25, 2, 10,  -3,  4,   2, -1,     7, 0.5,  1.5, -5,  3,   6,  0.5,   0.25,  -0.5)
 *       -> rec[0][0][0] = ( 0.5,  3,  8,  -0.5, -1.5,  3, 2.25,  -4, 1.5,  1, 1.5,  -0.625, 1.5,  0.125, 0.875,  0.5)
 *          e.g. out[3] = (a[3] - m[5]) / 2 = (1 - 2) / 2, out[4] = (a[4] + m[6]) / 2 = (-2 - 1) / 2, out[5] = (a[5] - m[3]) / 2 = (3 + 3) / 2,
 *          out[9] = (a[9] - m[11]) / 2 = (5 - 3) / 2, out[11] = (a[11] - m[9]) / 2 = (0.25 - 1.5) / 2, out[12] = (a[12] + m[10]) / 2 = (8 - 5) / 2
 *     rec[0][0][1] = a' = ( 0.5,  1,  1,   0,  0,   0,  0,   0,  0,   0,  0,   0,   0,  0.25, 0.75,  0)
 *     rec[1][0][0] = m' = ( 0.5,  3,  5,   2,  4,   6,  8,  10, 12,  14, 16,  18,  20,  9,    9,     2)
 *       -> rec[0][0][1] = ( 0.5,  2,  3,  -3,  4,  -1,  2,  -5,  6,  -9, 10,  -7,   8,  0.25, 0.75,  1)
 *     hm_plane[0] = (0.5, 0.5). */
int cf_set_flip_test(cf_ctx* ctx, int on);

/* ---- aligned face chips: the similarity warp of the frame onto a chip template, on the device ---------------------------- */
/* The next stage of a face pipeline (recognition, quality, attributes) takes an aligned crop: the least-squares similarity that maps
 * the detector's five landmarks onto a template (what SimilarityTransform.estimate + cv2.warpAffine do on the host), sampled
 * bilinearly.  Here one kernel writes the chips of every kept face of the batch from data that is still on the device.  The
 * arithmetic is this library's own statement (csrc/cf_align.hip, restated in tests/test_align.py): float64 estimate in a fixed
 * operation order, fixed-point warp (1/32-pixel positions, weights out of 1024, constant border 0 per neighbour).  It is NOT claimed
 * bit-identical to cv2.warpAffine, whose weight table is rounded to 15 bits. */
#define CF_CHIP_U8_HWC_BGR 0     /* uint8 [N,S,S,3] BGR */
#define CF_CHIP_F32_NCHW   1     /* float [N,3,S,S], value ((float)u8 - mean) * scale; planes B,G,R, or R,G,B when rgb != 0 */
typedef struct cf_align_opts {
    int32_t size;                /* S: chip side, a multiple of 4 in [16, 512] */
    int32_t format;              /* CF_CHIP_* */
    int32_t rgb;                 /* CF_CHIP_F32_NCHW only: channel order R,G,B */
    float   mean, scale;         /* CF_CHIP_F32_NCHW only */
    const float* tmpl;           /* [5][2] template points (x, y) in chip pixels, or NULL: the ArcFace 112 x 112 points times S / 112 */
    int32_t max_per_image;       /* at most this many faces per image, in keep order; 0 = all */
} cf_align_opts;
/* Chips of the faces kept by the LAST THRESHOLD DECODE of the last forward of ctx (cf_decode_threshold[_ex | _sized | _enqueue]),
 * sampled from the uint8 BGR batch the network read in that forward -- whichever entry point put it there (cf_forward with
 * CF_IN_U8_HWC_BGR from host or device, cf_forward_resized, cf_forward_images / _uploaded, cf_forward_yuv); a device input of
 * cf_forward must still be unchanged.  Landmarks are taken in NETWORK coordinates whatever cf_set_rescale says, so the chips are
 * cut from the network-sized batch (cf_align_faces_frame below samples the full-resolution source instead).  Face
 * n = offsets[b] + i is keep position i of image b; offsets [B + 1] = exclusive prefix sum of min(counts[b], the decode's max_out,
 * max_per_image).  Only faces n < cap_faces are written; offsets[B] is the number WANTED, so offsets[B] > cap_faces tells the
 * caller of the truncation (call again with more room).  chips: [cap_faces] chips in opts->format; matrices (may be NULL):
 * [cap_faces][6] float64, the row-major 2x3 chip -> source map that was sampled (all zero for a face that cannot be aligned:
 * non-finite or coincident landmarks, or a scale beyond the fixed-point range; its chip is that of an all-zero source).
 * out_on_device = 1: chips / matrices / offsets are device buffers (chips 16-byte aligned), the call is asynchronous on the stream
 * that carried the decode and reads no count on the host; 0: host buffers, blocking.  CF_EINVAL for any bad argument before any GPU
 * work; CF_ESTATE without a threshold decode behind the last forward, after a CF_IN_F32_NCHW forward, or once another upload or
 * forward was started on ctx. */
int cf_align_faces(cf_ctx* ctx, const cf_align_opts* opts, void* chips, double* matrices, int32_t* offsets, int cap_faces, int out_on_device);
/* The same chips cut from the SOURCE FRAMES instead of the network-sized batch: the read-side twin of cf_redact_faces.  A 1080p frame
 * behind a 640 x 640 context keeps three times the resolution of the face that cf_align_faces would upscale.  frames[b] (b < B, all
 * h x w in `format`: CF_YUV_* with the planes of cf_yuv_planes, or CF_FRAME_BGR with the [h][pitch0] pixel rows in .y), pitches and
 * in_on_device exactly as for cf_forward_tiles, except that BGR frames may have odd sides: sides 2..8192, even for 4:2:0; device
 * planes and pitches multiples of 4, read in place; host frames are copied up first (row bytes only).  The frames are named by the
 * caller, so it does not matter which entry point fed the forward (a CF_IN_F32_NCHW forward is fine: the network batch is not read).
 * Which faces -- as cf_redact_faces:
 *   * after cf_forward_tiles: the merged rows of the last cf_merge_tiles, whose landmarks are in frame pixels already; B must be Bf and
 *     (h, w) the tiled frame's (CF_EINVAL otherwise); CF_ESTATE without a merge;
 *   * otherwise: the rows the last threshold decode kept, in NETWORK coordinates whatever cf_set_rescale says; every value is mapped
 *     X = (double)x * ((double)w / (double)W), Y = (double)y * ((double)h / (double)H) and kept as a double, and the similarity is
 *     fitted to the mapped points (the map is anisotropic when h / H != w / W); B must equal the last forward's batch.
 * The source pixel at (sy, sx) is the three bytes at p0 + sy * pitch0 + 3 * sx (BGR), or the BT.601 conversion of cf_forward_yuv
 * applied to Y[sy][sx] and the chroma sample at (sy >> 1, sx >> 1): the chip equals, bit for bit, the chip cf_op_align_faces cuts
 * from the frame converted by cf_op_yuv_to_bgr at (H, W) = (h, w).  Estimate, fixed-point warp, border rule, the alignable rule and
 * the all-zero matrix / all-zero-source chip of an unalignable face are those of cf_align_faces (restated in tests/test_align.py);
 * `matrices` are chip -> FRAME pixel maps.  Sampling is bilinear at a point: a face much larger than the chip is not area-filtered
 * (neither is cv2.warpAffine's).  opts, chips, matrices, offsets ([B + 1]; offsets[B] = the number wanted), cap_faces,
 * max_per_image and out_on_device are exactly as for cf_align_faces.  With device frames and device outputs nothing is read on the
 * host and the call is asynchronous on the stream that carried the decode or the merge; with host frames or host outputs it blocks.
 * CF_EINVAL for every bad argument before any GPU work (ctx == NULL: the arguments are still checked, cf_op_last_error names the
 * cause); CF_ESTATE without a threshold decode behind the last forward, or once another upload or forward was started on ctx.  The
 * call changes no state of ctx: a cf_redact_faces, cf_align_faces or second cf_align_faces_frame behind it behaves as before. */
int cf_align_faces_frame(cf_ctx* ctx, const cf_align_opts* opts, int format, const cf_yuv_planes* frames, int in_on_device,
                         int B, int h, int w, int pitch0, int pitch1,
                         void* chips, double* matrices, int32_t* offsets, int cap_faces, int out_on_device);

/* ---- face redaction: blank or pixelate every kept face IN THE SOURCE FRAME, on the device ------------------------------------ */
/* Anonymising video: every face the detector kept is covered in the full-resolution frame -- BGR or 4:2:0, a decoder's surface in
 * place -- and the frame goes on to an encoder; no box and no pixel crosses to the host.  The arithmetic is this library's own
 * statement (csrc/cf_redact.hip, restated in tests/test_redact.py; device and restatement are equal bit for bit).  Integers
 * throughout, except the box mapping: float64 in the order written, no FMA contraction.
 *   Per face: box (x1, y1, x2, y2) float32 in NETWORK coordinates (as the threshold decode computed it, BEFORE cf_set_rescale),
 *   frame h x w, context H x W, options below.
 *   1. Box to frame.  cx = ((double)x1 + (double)x2) * 0.5;  hw = ((double)x2 - (double)x1) * 0.5 * (double)scale;
 *      fx = (double)w / (double)W;  X1 = floor((cx - hw) * fx), X2 = ceil((cx + hw) * fx); likewise y with h / H.  The face is
 *      skipped when one of the four inputs is not finite or hw / hh is not > 0.  Each result is clamped to [-8192, 16384] as a
 *      double, converted to int, then X1, Y1 are rounded DOWN to even and X2, Y2 UP to even (every format: a mask means the same
 *      pixels in BGR and in 4:2:0).  Frames are at most 8192 a side, so no int64 product below overflows.
 *   2. Coverage, in half-pixel units: a BGR pixel / luma sample (x, y) has the point (U, V) = (2x+1, 2y+1), a chroma sample (i, j)
 *      the point (4i+2, 4j+2).  RECT: 2*X1 <= U < 2*X2 and 2*Y1 <= V < 2*Y2.  ELLIPSE: A = X2-X1, Bv = Y2-Y1, du = U-(X1+X2),
 *      dv = V-(Y1+Y2): (du*Bv)^2 + (dv*A)^2 <= (A*Bv)^2 in int64.  Only samples inside the frame are written; a sample is redacted
 *      when ANY face of its image covers it.
 *   3. Value.  SOLID: fill[channel].  MOSAIC: the grid is anchored at the FRAME origin: cell (gx, gy) of a BGR / luma plane is
 *      [gx*m, min((gx+1)*m, w)) x [gy*m, min((gy+1)*m, h)), of a chroma plane the same index with m/2, w/2, h/2 (the two interleaved
 *      channels of NV12 / NV21 separately); its value is (sum + n/2) / n over ALL n samples of the cell in the frame AS IT WAS BEFORE
 *      THE CALL, per channel, and a covered sample takes its cell's value -- so the result depends neither on the order of the faces
 *      nor on their overlap.  On the device: one launch that only reads the frame writes the means of every cell a face's clipped
 *      box touches into a scratch of one entry per cell, a second launch only writes covered samples.
 * Bytes outside the masks -- pitch padding, the corners of an ELLIPSE box -- are not written at all. */
#define CF_REDACT_SOLID   0
#define CF_REDACT_MOSAIC  1
#define CF_REDACT_RECT    0
#define CF_REDACT_ELLIPSE 1
typedef struct cf_planes_rw {
    void* p0;                    /* BGR: the [h][pitch0] pixel rows; 4:2:0: the Y plane */
    void* p1;                    /* 4:2:0: first chroma plane in the format's order (as cf_yuv_planes.c0), h/2 rows of pitch1 bytes; BGR: unused */
    void* p2;                    /* I420 / YV12: second chroma plane; otherwise unused */
} cf_planes_rw;
typedef struct cf_redact_opts {
    int32_t mode;                /* CF_REDACT_SOLID | CF_REDACT_MOSAIC */
    int32_t shape;               /* CF_REDACT_RECT | CF_REDACT_ELLIPSE */
    int32_t cell;                /* MOSAIC: m, even, 2 <= m <= 256 (ignored for SOLID) */
    float   scale;               /* the box is grown about its centre by this factor, 0.25 <= scale <= 4 */
    uint8_t fill[4];             /* SOLID: bytes in the frame's own channel order (B,G,R or Y,U,V); [3] unused */
} cf_redact_opts;
/* Redacts, in frames[b] (b < B, all h x w in `format`: CF_YUV_* or CF_FRAME_BGR), the faces that the LAST THRESHOLD DECODE of the last
 * forward of ctx kept for image b: rows i < min(counts[b], the decode's max_out), as cf_align_faces.  The frames are named by the
 * caller, so it does not matter which entry point fed the forward (a CF_IN_F32_NCHW forward is fine: the input batch is not read).
 * pitch0 >= 3w (BGR) or >= w (Y), pitch1 as c_pitch of cf_forward_yuv (ignored for BGR), in bytes.
 * on_device = 1: in place on the caller's device planes (addresses and pitches multiples of 4), asynchronous on the stream that
 * carried the decode, no count is read on the host; on_device = 0: host frames are copied up, redacted and copied back, blocking.
 * B must equal the last forward's batch.  CF_EINVAL, before any GPU work, for: format / mode / shape out of range, an odd or
 * out-of-range cell (MOSAIC), scale out of range or not finite, odd h or w for 4:2:0, h or w of 0 or above 8192, a pitch that is too
 * small, a misaligned device plane or pitch, a NULL required plane.  CF_ESTATE without a threshold decode behind the last forward, or
 * once another upload or forward was started on ctx. */
int cf_redact_faces(cf_ctx* ctx, const cf_redact_opts* opts, int format, const cf_planes_rw* frames, int on_device, int B, int h, int w,
                    int pitch0, int pitch1);

/* ---- blur redaction: the same faces covered with a Gaussian-like blur of the frame ---------------------------------------------- */
/* The third look of a face anonymiser beside SOLID and MOSAIC, as its own entry point with its own options (cf_redact_opts and its
 * modes stay as they are).  The arithmetic is this library's own statement (csrc/cf_blur.hip, restated in tests/test_blur.py; device
 * and restatement are equal bit for bit).  Integers throughout, except the box mapping, which is cf_redact_faces'.
 *   1. Faces, boxes, coverage: steps 1 and 2 of cf_redact_faces, exactly -- the kept rows of the last threshold decode or the merged
 *      rows after cf_merge_tiles, the box grown by `scale`, X1, Y1 snapped down and X2, Y2 up to even, the RECT / ELLIPSE half-pixel
 *      point tests with chroma samples at (4i+2, 4j+2).
 *   2. Filter of strength r, 1 <= r <= 24.  b = 2r+1; the 1-D taps t are the integer sequence box_b * box_b * box_b (three discrete
 *      convolutions of b ones): 6r+1 taps, radius R = 3r, sum b^3, variance r(r+1), so sigma is about r; r = 1: 1 3 6 7 6 3 1.  The
 *      taps come from integer convolution, never from exp.  For a sample (x, y) of a plane of cw x ch samples, per channel:
 *        S = sum_j sum_i t[j] * t[i] * src[clamp(y+j-R, 0, ch-1)][clamp(x+i-R, 0, cw-1)]
 *        value = (S + D/2) / D,  D = b^6, in 64-bit integers  (S <= 255 * 49^6; the row sums fit int32)
 *      One rounding only, so a separable evaluation equals the 2-D one.  src is the plane AS IT WAS BEFORE THE CALL; border samples
 *      replicate.  The three bytes of BGR are filtered separately, as are the two interleaved channels of NV12 / NV21 (stride 2
 *      bytes).  Chroma planes use r_c = (r+1)/2 (integer division) on their w/2 x h/2 grid.
 *   3. Which r.  radius in 1..24: that r for every face.  radius == 0: per face, with A = X2-X1 and Bv = Y2-Y1 of the snapped,
 *      unclipped box, r_f = clamp(min(A, Bv) / 8, 1, 24) (integer division); a covered sample takes the value computed with
 *      r* = max r_f over the faces of its image that cover THAT sample (the sample's own point test: the chroma one for chroma;
 *      (r+1)/2 is monotonic, so the chroma radius is that of r*).  The value depends only on (plane, x, y, r*) and the untouched
 *      frame, so the result depends neither on the order of the faces nor on their overlap.
 *   4. Writes.  Only covered samples inside the frame, never by read-modify-write; pitch padding, the corners of an ELLIPSE box and
 *      uncovered bytes are not touched.  On the device: one launch that only reads the frame writes the value of every covered
 *      sample into a context-owned scratch that mirrors the planes, a second launch only writes covered samples -- so the call runs
 *      in place on a decoder's surface. */
typedef struct cf_blur_opts {
    int32_t shape;               /* CF_REDACT_RECT | CF_REDACT_ELLIPSE */
    int32_t radius;              /* r, 1..24; 0 = per face from the box size */
    float   scale;               /* the box is grown about its centre by this factor, 0.25 <= scale <= 4 */
} cf_blur_opts;
/* Frames, formats, pitches, alignment, on_device, the faces (after cf_merge_tiles: the merged rows), B and the state rules are those
 * of cf_redact_faces.  CF_EINVAL, before any GPU work, for: format / shape out of range, radius outside 0..24, scale out of range or
 * not finite, odd h or w for 4:2:0, h or w of 0 or above 8192, a pitch that is too small, a misaligned device plane or pitch, a NULL
 * required plane.  CF_ESTATE as cf_redact_faces.  The scratch grows to the largest B x frame seen (outside any graph). */
int cf_blur_faces(cf_ctx* ctx, const cf_blur_opts* opts, int format, const cf_planes_rw* frames, int on_device, int B, int h, int w,
                  int pitch0, int pitch1);

/* ---- tiled detection of large frames (sliced inference) ------------------------------------
 * A frame much larger than the network input loses its small faces in the stretch-resize of every other entry point.  Here the frame
 * is cut into overlapping rectangles at or near native resolution, the rectangles run as one batch, and the per-tile detections are
 * mapped back into frame pixels and de-duplicated, all on the device:
 *   cf_tile_grid (host) -> cf_forward_tiles -> cf_decode_threshold* (unchanged, per tile image) -> cf_merge_tiles [-> cf_redact_faces]
 * The defaults the Python layer uses (IoS 0.5, edge 2) are this project's choices, not the reference's; no accuracy claim is made. */
typedef struct cf_tile_rect { int32_t x0, y0, w, h; } cf_tile_rect;
#define CF_MERGE_IOU 0           /* suppress when inter / union >= thresh (the decode's own measure) */
#define CF_MERGE_IOS 1           /* suppress when inter / min(area, area) >= thresh: removes a partial box lying inside a full one */
typedef struct cf_merge_opts {
    int32_t metric;              /* CF_MERGE_IOU | CF_MERGE_IOS */
    float   thresh;
    float   edge;                /* network pixels; 0 = no edge rule */
} cf_merge_opts;
/* The rectangles of an h x w frame for tiles of tile_h x tile_w with at least `overlap` pixels shared by neighbours (all even,
 * 0 <= overlap < min(tile_h, tile_w)); host only.  Per axis: rw = min(tile_w, w); nx = 1 when rw == w, else
 * ceil((w - overlap) / (rw - overlap)); x0_i = ((i * (w - rw)) / (nx - 1)) & ~1 (integer division).  Row-major, y outer; the
 * whole-frame rectangle (0, 0, w, h) is appended when with_full and nx * ny > 1.  The rectangles cover the frame, the last one ends
 * at w / h.  *n = the number wanted; only the first `cap` are written.  1920 x 1080, tile 640, overlap 128: 4 x 2 + 1 = 9. */
int cf_tile_grid(int h, int w, int tile_h, int tile_w, int overlap, int with_full, cf_tile_rect* rects, int cap, int* n);
/* Bf frames of h x w in `format` (CF_YUV_* with the planes of cf_yuv_planes, or CF_FRAME_BGR with the [h][pitch0] pixel rows in .y)
 * and T rectangles shared by the frames -> the network batch of Bf * T images, image f * T + t = resize(bgr(frame f)[rectangle t],
 * (H, W)) with the conversion of cf_forward_yuv and the resize of cf_forward_resized applied to the crop (taps clamp at the
 * rectangle's edges) -> forward.  x0, y0, w, h of every rectangle even, w, h >= 2, inside the frame; frame h, w even, <= 8192;
 * 1 <= T, Bf * T <= max_batch.  pitch0 >= 3w (BGR) or w (Y), pitch1 as c_pitch of cf_forward_yuv.  in_on_device = 1: the planes
 * are read in place (addresses and pitches multiples of 4); 0: host frames, copied up first (only the row bytes are read).
 * CF_EINVAL before anything is enqueued, the offending rectangle named in cf_last_error.  The context remembers the rectangles and
 * the frame size for cf_merge_tiles; every other forward or upload forgets them.  cf_get_resized_input returns the tile batch;
 * cf_align_faces works per tile image; cf_align_faces_frame, after cf_merge_tiles, per frame on the merged rows. */
int cf_forward_tiles(cf_ctx* ctx, int format, const cf_yuv_planes* frames, int in_on_device, int Bf, int h, int w,
                     int pitch0, int pitch1, const cf_tile_rect* rects, int T);
/* Merges the rows the LAST THRESHOLD DECODE kept for the Bf * T tile images of the last cf_forward_tiles, per frame.  Per tile the rows
 * i < min(counts, the decode's max_out), in network coordinates whatever cf_set_rescale says:
 *   * a row is dropped when a corner is not finite, or when the box comes within opts->edge network pixels of a side of its rectangle
 *     that is not on the frame border (x1 < edge, x2 > W - edge, y1 < edge, y2 > H - edge; float32);
 *   * the others are mapped, X = (float)((double)x * ((double)rw / (double)W) + (double)x0), y likewise (corners and landmarks);
 *   * greedy NMS over the frame's candidates in (tile, row) order with opts->metric and opts->thresh: score descending, the higher
 *     candidate index first among equals, float32 "+1" areas as the decode's.
 * dets [Bf][max_out][5], lms [Bf][max_out][10] in frame pixels, counts [Bf] (may exceed max_out: only max_out rows are written),
 * flags [Bf] (bit 0: a tile of the frame had more rows than the decode's max_out).  Any of the four may be NULL; the context's own
 * merged rows are written in any case (cf_redact_faces reads them).  out_on_device = 1: device buffers, asynchronous on the decode's
 * stream, no count read on the host; 0: host buffers, blocking.  CF_ESTATE unless the last forward was cf_forward_tiles with a
 * threshold decode behind it; CF_ENOMEM, before any launch, when the suppression bits of Bf x (T * the decode's max_out) candidates
 * would exceed 256 MiB.  After a merge, cf_redact_faces takes the merged boxes: its B must be Bf and its (h, w) the frame's
 * (CF_EINVAL otherwise); after a tiled forward without a merge it returns CF_ESTATE. */
int cf_merge_tiles(cf_ctx* ctx, const cf_merge_opts* opts, int max_out, float* dets, float* lms, int32_t* counts, int32_t* flags,
                   int out_on_device);

/* ---- aspect-preserving (letterbox) input: fit frames on the device, map rows back ------------
 * cf_forward_resized, cf_forward_yuv and the whole-frame tile of a tiled forward STRETCH a frame of another size to (H, W): a 1920 x 1080
 * frame behind a 640 x 640 context reaches the network with every face squashed to 56 % of its width.  The reference's data pipeline
 * fits the image with its aspect ratio kept and the border left black (dataset/dataset.py:114-134: s = max(h, w), get_affine_transform,
 * cv2.warpAffine with the zero border), and its CenterFace(h, w) builds the network for the frame's size, so neither distorts.  Here
 * the frame is resized with its aspect ratio kept, pasted into a filled (H, W) canvas, and the decode's rows are mapped back into frame
 * pixels, all on the device:
 *   cf_forward_fit -> cf_decode_threshold* (unchanged, per canvas) -> cf_unfit_rows [-> cf_track_update | cf_redact_faces | ...]
 * No trained weights and no labelled set are on hand: no accuracy claim is made for cf_forward_fit; the argument is geometric.
 *
 * Geometry of an h x w frame in an H x W canvas (integers, 64-bit products):
 *   upscale == 0 and h <= H and w <= W:   rw = w, rh = h
 *   else w * H <= h * W (height-limited): rh = H, rw = max(1, (2 * w * H + h) / (2 * h))
 *   else:                                 rw = W, rh = max(1, (2 * h * W + w) / (2 * w))
 *   CF_FIT_CENTER: dx = (W - rw) / 2, dy = (H - rh) / 2;  CF_FIT_TOPLEFT: dx = dy = 0.
 *   1080 x 1920 in 640 x 640: rw 640, rh 360, dy 140.  40 x 120 in 64 x 96: rw 96, rh 32, dy 16.  120 x 40 in 64 x 96: rh 64, rw 21, dx 37.
 * Canvas: image b = fill everywhere, except canvas[dy : dy + rh, dx : dx + rw] = resize(bgr(frame b), (rh, rw)) with the conversion of
 * cf_forward_yuv (the identity for CF_FRAME_BGR) and the resize of cf_forward_resized from (h, w) to (rh, rw): "resize, then pad".
 * rw == w and rh == h reproduce the source bytes.  rw, rh, dx, dy may be odd. */
#define CF_FIT_CENTER  0
#define CF_FIT_TOPLEFT 1
typedef struct cf_fit_opts {
    int32_t anchor;              /* CF_FIT_CENTER | CF_FIT_TOPLEFT */
    int32_t upscale;             /* 1: a frame smaller than the canvas is enlarged until one side fills it; 0: it keeps its size */
    uint8_t fill[4];             /* B, G, R of the padding, unused */
} cf_fit_opts;                   /* 12 bytes */
typedef struct cf_fit_geom { int32_t rw, rh, dx, dy; } cf_fit_geom;
/* The geometry above; host only.  CF_EINVAL (cf_op_last_error names the value) for NULL opts or g, an anchor or upscale outside {0, 1},
 * h or w outside 2..8192, H or W below 1; *g is written on success only. */
int cf_fit_geometry(const cf_fit_opts* opts, int h, int w, int H, int W, cf_fit_geom* g);
/* B frames of h x w in `format` -> the network batch of B canvases as stated above -> forward.  Formats, planes, pitches, in_on_device
 * and the alignment rule of device planes exactly as for cf_forward_tiles, except that BGR frames may have odd sides: sides 2..8192,
 * even for 4:2:0.  The fit is one launch (per 64 frames); every tap lies inside the frame, pitch padding is never read; the frames are
 * not modified.  CF_EINVAL before any GPU work, the offending value named in cf_last_error, for: NULL opts, frame table or required
 * plane, an anchor or upscale outside {0, 1}, a bad format, side, pitch or alignment, B < 1 or B > max_batch (ctx == NULL: the arguments
 * are still checked first, cf_op_last_error names the cause).  The context remembers the geometry and the frame size for cf_unfit_rows
 * until any other forward or upload.  cf_get_resized_input returns the padded batch; cf_align_faces works per image on the padded
 * batch; cf_merge_tiles behind it is CF_ESTATE (it is not a tiled forward). */
int cf_forward_fit(cf_ctx* ctx, const cf_fit_opts* opts, int format, const cf_yuv_planes* frames, int in_on_device, int B, int h, int w,
                   int pitch0, int pitch1);
/* Maps the rows the LAST THRESHOLD DECODE kept for the B images of the last cf_forward_fit back into frame pixels.  Per image the rows
 * i < min(count, the decode's max_out), in keep order, in network coordinates whatever cf_set_rescale says:
 *   * a row is dropped when a corner is not finite, or when its centre cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f (float32) lies
 *     outside the content: it is kept iff dx <= cx < dx + rw and dy <= cy < dy + rh;
 *   * the others are mapped, X = (float)(((double)x - (double)dx) * ((double)w / (double)rw)), Y likewise with dy and h / rh (the four
 *     corners and the ten landmark values; float64 in this order, no contraction); the score is copied.  No clamping, no second NMS.
 * The kept rows are compacted in order (a prefix sum: deterministic).  dets [B][max_out][5], lms [B][max_out][10] in frame pixels,
 * counts [B] (may exceed max_out: only max_out rows are written), flags [B] (bit 0: the image had more rows than the decode's max_out).
 * Any of the four may be NULL; out_on_device as for cf_merge_tiles.  The context's own frame-space rows are written in any case and the
 * context is left in the state behind a merge: cf_track_update, cf_track_follow, cf_redact_faces, cf_blur_faces, cf_draw_faces,
 * cf_align_faces_frame and the best-shot offer take them with B frames of (h, w), as after cf_merge_tiles; before cf_unfit_rows they
 * return CF_ESTATE.  CF_EINVAL for max_out < 1 (ctx == NULL: checked first, cf_op_last_error names the cause); CF_ESTATE unless the
 * last forward was cf_forward_fit with a threshold decode behind it. */
int cf_unfit_rows(cf_ctx* ctx, int max_out, float* dets, float* lms, int32_t* counts, int32_t* flags, int out_on_device);

/* ---- rotated sources: detect upright in frames stored a quarter or half turn away ------------
 * Every forward above takes the stored frame for upright.  A corridor-mode camera (the sensor mounted a quarter turn, the stream still
 * 1920 x 1080) and phone video (the turn kept in the container's display matrix, the hardware decoder handing out the surface as stored)
 * break that: the network, trained on upright faces (the reference mirrors its training images and never turns them,
 * dataset/dataset.py:125-128), sees sideways ones.  cf_forward_rot fills the canvases from the UPRIGHT view of the stored frames and
 * cf_unfit_rows maps the decode's rows back into the STORED frame's pixels, so cover, draw and chip calls work in place on the
 * decoder's surface as they do behind cf_forward_fit; cf_align_faces_frame fits a similarity to the landmarks, so its chips of a turned
 * frame come out upright as they are:
 *   cf_forward_rot -> cf_decode_threshold* (unchanged, per canvas) -> cf_unfit_rows [-> cf_track_update | cf_redact_faces | ...]
 * No trained weights and no labelled set are on hand: no accuracy claim is made; the argument is geometric, as for the fit.
 *
 * rot in {0, 90, 180, 270} is the CLOCKWISE turn that makes the stored frame F (h x w) upright: a display-matrix rotation,
 * cv2.ROTATE_90_CLOCKWISE for 90.  The upright view U has (hu, wu):
 *   rot   0: (h, w)  U[y][x] = F[y][x]                    numpy: F
 *   rot  90: (w, h)  U[y][x] = F[h-1-x][y]                numpy: np.rot90(F, -1)
 *   rot 180: (h, w)  U[y][x] = F[h-1-y][w-1-x]            numpy: np.rot90(F, 2)
 *   rot 270: (w, h)  U[y][x] = F[x][w-1-y]                numpy: np.rot90(F, 1)
 * Canvas: canvas_b is what the statements above make of bgr(U_b), with bgr() the conversion of cf_forward_yuv applied to F, before the
 * turn (the identity for CF_FRAME_BGR):
 *   stretch == 0: the fit of cf_forward_fit with the geometry cf_fit_geometry(&fit, hu, wu, H, W): resize to (rh, rw), then pad;
 *   stretch == 1: rw = W, rh = H, dx = dy = 0: the resize of cf_forward_resized from (hu, wu) to (H, W), no padding.
 * Rows back (cf_unfit_rows behind cf_forward_rot): kept or dropped exactly as behind cf_forward_fit -- finite corners and the float32
 * centre inside the content, in canvas coordinates.  With, in float64, in this order and without contraction,
 *   ux(x) = ((double)x - dx) * ((double)wu / rw),   uy(y) = ((double)y - dy) * ((double)hu / rh),
 * a point (x, y) of the canvas maps to (X, Y) of the stored frame; the difference is taken in float64 and rounded to float32 once:
 *   rot   0: X = ux(x)            Y = uy(y)
 *   rot  90: X = uy(y)            Y = (h-1) - ux(x)
 *   rot 180: X = (w-1) - ux(x)    Y = (h-1) - uy(y)
 *   rot 270: X = (w-1) - uy(y)    Y = ux(x)
 * (h-1 and w-1 are the index map above; the decode's own "+1" widths treat coordinates as pixel indices).  The five landmarks are
 * mapped point by point in their order: a rotation keeps handedness, left and right are not swapped.  The box is an ASSIGNMENT of
 * mapped corners, never a min / max, so a signed zero or an inverted box of untrained weights cannot make the result ambiguous:
 *   rot  90: X1 = X(., y1)  Y1 = Y(x2, .)  X2 = X(., y2)  Y2 = Y(x1, .)
 *   rot 180: X1 = X(x2, .)  Y1 = Y(., y2)  X2 = X(x1, .)  Y2 = Y(., y1)
 *   rot 270: X1 = X(., y2)  Y1 = Y(x1, .)  X2 = X(., y1)  Y2 = Y(x2, .)
 * The score is copied; compaction, counts and flags as behind cf_forward_fit.  With rot == 0 and stretch == 0 the canvases and the rows
 * are those of cf_forward_fit + cf_unfit_rows, bit for bit (the same kernels).
 * Not covered: mirrored orientations (the other four EXIF codes; they need the landmark swap of the flip merge); a rot per frame within
 * one call (one camera, one mount: group the frames per call); probing the orientation.  This call stays a single-view path: tiles
 * and levels of a rotated source, a rotated tiled forward among them, live in cf_forward_packed_rot further down.  The labels
 * cf_draw_faces paints are upright in the STORED frame, so a viewer of the upright video sees them turned. */
typedef struct cf_rot_opts {
    int32_t rot;                 /* 0 | 90 | 180 | 270: the clockwise turn that makes the stored frame upright */
    int32_t stretch;             /* 1: the upright view is stretched to (H, W) and `fit` is only validated; 0: it is fitted by `fit` */
    cf_fit_opts fit;
} cf_rot_opts;                   /* 20 bytes */
/* The geometry of the upright view in the canvas, as stated above; host only.  CF_EINVAL (cf_op_last_error names the value) for NULL
 * opts or g, a rot outside the four, a stretch outside {0, 1}, and whatever cf_fit_geometry refuses; *g is written on success only. */
int cf_rot_geometry(const cf_rot_opts* opts, int h, int w, int H, int W, cf_fit_geom* g);
/* B stored frames of h x w in `format` -> the B canvases stated above -> forward.  Formats, planes, pitches, in_on_device, alignment and
 * the staging of host frames exactly as for cf_forward_fit, and every check of it, plus CF_EINVAL before any GPU work, the value named
 * in cf_last_error, for a rot outside the four or a stretch outside {0, 1} (ctx == NULL: the arguments are still checked first,
 * cf_op_last_error names the cause).  A quarter turn is one launch (per 64 frames) whose taps coalesce along the stored rows; every tap
 * lies inside the frame, pitch padding is never read; the frames are not modified.  The context remembers rot, the geometry and the
 * stored frame's size for cf_unfit_rows until any other forward or upload; cf_unfit_rows then leaves "B frames of (h, w)" for the
 * consumers with the same state rules and the same CF_ESTATE answers as behind cf_forward_fit.  cf_set_flip_test, cf_get_resized_input
 * and cf_align_faces see the canvases; cf_merge_tiles behind it is CF_ESTATE. */
int cf_forward_rot(cf_ctx* ctx, const cf_rot_opts* opts, int format, const cf_yuv_planes* frames, int in_on_device, int B, int h, int w,
                   int pitch0, int pitch1);

/* ---- multi-scale detection: tiles and reduced frame copies, merged on the device -------------
 * Every forward above shows the network each face at ONE size, set by how the frame is mapped into the canvas: the stretch or the fit of
 * the whole frame, a turned whole frame, or tiles, which enlarge and cover the small end.  Nothing covers the large end: a face that fills
 * a phone or video-call frame is about 300 network pixels wide after the fit into 640 x 640, where a stride-4 centre detector is known to
 * break up.  CenterNet's test code answers with test_scales -- the frame run at several sizes, the results merged -- the other half of
 * the test-time pair whose flip test is cf_set_flip_test.  Here ONE batch holds different VIEWS of the same frame -- enlarged tiles, the
 * aspect-true whole frame, the whole frame at half and quarter size -- and ONE merge runs over it, all on the device:
 *   cf_view_layout (host) -> cf_forward_views -> cf_decode_threshold* (unchanged, per view image) -> cf_merge_views [-> cf_track_update | ...]
 * No trained weights and no labelled set are on hand: no accuracy claim is made; the argument is geometric, as for tiles and the fit.
 * The layout defaults of the Python layer (levels 1.0 and 0.5) and its merge (IoS 0.5, edge 2) are this project's choices; nobody has
 * measured them.
 *
 * A VIEW is a source rectangle of the frame and a content rectangle of the canvas.
 * Canvas: image f * V + v is `fill` everywhere, except
 *   canvas[dy : dy + dh, dx : dx + dw] = resize(bgr(frame f)[sy0 : sy0 + sh, sx0 : sx0 + sw], (dh, dw))
 * with the conversion of cf_forward_yuv (the identity for CF_FRAME_BGR) and the fixed-point resize of cf_forward_resized applied to the
 * crop: the taps clamp at the source rectangle's edges.  A view with (dx, dy, dw, dh) = (0, 0, W, H) is the tile of cf_forward_tiles,
 * byte for byte; a view with the whole frame as source and the rectangle of cf_fit_geometry as content is the canvas of cf_forward_fit,
 * byte for byte; a source of exactly the content's size reproduces the source bytes.
 * Limits, plainly: cf_forward_views puts one view per canvas -- a half-size level costs a whole forward for a quarter of a canvas;
 * the packing of several levels and frames into one canvas is cf_forward_packed below; it takes the stored frame for upright: rotated
 * views live in cf_forward_packed_rot (cf_forward_rot stays a single-view path). */
typedef struct cf_view {
    int32_t sx0, sy0, sw, sh;    /* frame pixels; all even, sw, sh >= 2, inside the frame */
    int32_t dx, dy, dw, dh;      /* canvas pixels; dw, dh >= 1, inside (H, W); may be odd */
} cf_view;                       /* 32 bytes */
typedef struct cf_view_opts {
    int32_t tile_h, tile_w, overlap;   /* 0, 0: no tiles */
    int32_t anchor;              /* CF_FIT_CENTER | CF_FIT_TOPLEFT, for the levels */
    int32_t n_levels;            /* 0..8 */
    int32_t scale_pm[8];         /* per mille of the fitted size, 1..1000 */
} cf_view_opts;                  /* 52 bytes */
/* The views of an h x w frame in an H x W canvas; host only.  Tiles first: the rectangles of cf_tile_grid(h, w, tile_h, tile_w, overlap,
 * with_full = 0), each with the whole canvas (0, 0, W, H) as content, and only when there is more than one (tile_h = tile_w = 0: none,
 * overlap is not looked at).  Then one view per level, in the order given: the whole frame (0, 0, w, h) as source and the content
 *   dw = max(1, (rw * pm + 500) / 1000), dh = max(1, (rh * pm + 500) / 1000)      (integer division)
 * with (rw, rh) of cf_fit_geometry with upscale = 1; CF_FIT_CENTER: dx = (W - dw) / 2, dy = (H - dh) / 2; CF_FIT_TOPLEFT: dx = dy = 0.
 * 1080 x 1920 in 640 x 640, tile 640, overlap 128, levels 1000 and 500: 8 tiles, then 640 x 360 at y = 140, then 320 x 180 at
 * (160, 230): V = 10.  *n = the number wanted; only the first `cap` are written.  CF_EINVAL (cf_op_last_error names the cause) for NULL
 * opts or n, an anchor outside {0, 1}, n_levels outside 0..8, a scale outside 1..1000, when the result would be empty, and for whatever
 * cf_tile_grid (tiles asked for) or cf_fit_geometry refuse.  A frame with an odd side gets levels with an odd source, which
 * cf_forward_views refuses as it refuses the frame. */
int cf_view_layout(const cf_view_opts* opts, int h, int w, int H, int W, cf_view* views, int cap, int* n);
/* Bf frames of h x w in `format` and V views shared by the frames -> the network batch of Bf * V canvases stated above, fill = B, G, R
 * of the padding (3 bytes) -> forward.  Frames, formats, pitches, the staging of host frames, the alignment of device planes and the
 * even-sides rule exactly as for cf_forward_tiles; 1 <= V, Bf * V <= max_batch.  The cutter is one launch (per 64 frames); rows and
 * columns of the padding are written without touching the source; every tap lies inside the source rectangle, pitch padding is never
 * read; the frames are not modified.  CF_EINVAL before anything is enqueued, the offending view named by its index in cf_last_error,
 * for: a source value that is odd, smaller than 2 or outside the frame, dw or dh below 1, a content outside (H, W), V < 1, NULL views
 * or fill, a bad format, side, pitch or alignment, Bf * V > max_batch (ctx == NULL: the arguments are still checked first, the content
 * only for dx, dy >= 0 and dw, dh >= 1 as there is no canvas, and cf_op_last_error names the cause).  The context remembers the views
 * and the frame size for cf_merge_views until any other forward or upload.  Under cf_set_flip_test it behaves as cf_forward_tiles does
 * (Bf * V <= max_batch / 2, the mirrors behind the batch).  cf_get_resized_input returns the view batch; cf_align_faces works per view
 * image; cf_merge_tiles and cf_unfit_rows behind it are CF_ESTATE. */
int cf_forward_views(cf_ctx* ctx, int format, const cf_yuv_planes* frames, int in_on_device, int Bf, int h, int w, int pitch0, int pitch1,
                     const cf_view* views, int V, const uint8_t* fill);
/* Merges the rows the LAST THRESHOLD DECODE kept for the Bf * V view images of the last cf_forward_views, per frame.  The candidates are
 * the rows i < min(count, the decode's max_out) of each view image, walked in (view, row) order, in network coordinates whatever
 * cf_set_rescale says.  A row is dropped when any of these holds:
 *   * a corner is not finite;
 *   * its float32 centre (x1 + x2) * 0.5f, (y1 + y2) * 0.5f lies outside [dx, dx + dw) x [dy, dy + dh) (the rule of cf_unfit_rows);
 *   * its box comes within opts->edge of a content side whose SOURCE side is interior to the frame, four float32 compares:
 *       x1 < (float)dx + edge  when sx0 > 0;   x2 > (float)(dx + dw) - edge  when sx0 + sw < w;   the same two in y
 *     (for a tile view these are the compares of cf_merge_tiles, bit for bit; a whole-frame level has no interior side).
 * A kept row is mapped, X = (float)(((double)x - (double)dx) * ((double)sw / (double)dw) + (double)sx0), Y likewise with dy, sh / dh
 * and sy0 (the four corners and the ten landmark values; float64 in this order, no contraction; for a tile view the bits of
 * cf_merge_tiles); the score is copied.  Then the greedy NMS of cf_merge_tiles over the frame's candidates: the same metric, threshold,
 * order and ties, the same dets / lms / counts / flags (bit 0: a view image of the frame had more rows than the decode's max_out), the
 * same out_on_device forms and the same CF_ENOMEM refusal above 256 MiB of suppression bits (Bf x (V * the decode's max_out)
 * candidates).  The compaction is a prefix sum: deterministic.  Afterwards the context is in the state behind a merge: cf_track_update,
 * cf_track_follow, cf_redact_faces, cf_blur_faces, cf_draw_faces, cf_align_faces_frame, the lookback and the best-shot offer take the
 * rows with Bf frames of (h, w), unchanged; before cf_merge_views they return CF_ESTATE.  CF_ESTATE unless the last forward was
 * cf_forward_views with a threshold decode behind it. */
int cf_merge_views(cf_ctx* ctx, const cf_merge_opts* opts, int max_out, float* dets, float* lms, int32_t* counts, int32_t* flags,
                   int out_on_device);

/* ---- packed views: several levels and frames share one canvas ---------------------------------
 * cf_forward_views spends a whole canvas on every view: levels 1.0, 0.5 and 0.25 of a 1080p frame in 640 x 640 are three canvases per
 * frame, the third one 1/16 full.  A PLACEMENT puts one view of one frame into one canvas, and a canvas may hold many:
 *   cf_pack_views (host) -> cf_forward_packed -> cf_decode_threshold* (unchanged, per canvas) -> cf_merge_packed [-> cf_track_update | ...]
 * Canvas n of a packed batch of N canvases is `fill` everywhere; inside the content rectangle of every placement with canvas == n it is
 * the cf_forward_views image of that view of frame `frame`, byte for byte: the same conversion, the same fixed-point resize of the crop,
 * taps clamped at the source rectangle.  The contents of one canvas must not overlap (sharing an edge is allowed); a canvas without a
 * placement is all fill.  The placement list {f, f * V + v, views[v]} for f < Bf, v < V reproduces cf_forward_views byte for byte and
 * cf_merge_views bit for bit.
 * Limits, plainly: the threshold decode's own NMS and its max_out are per CANVAS, so they are shared by the frames on that canvas; boxes
 * of two frames whose contents share an edge can suppress each other in that NMS when they overlap -- a gutter keeps them apart;
 * cf_align_faces behind a packed forward works per canvas image; the stored frame is taken for upright (rotated views live in
 * cf_forward_packed_rot below); all frames of a call have one size.  The gutter
 * default of the Python layer (0) is this project's choice; nobody has measured it (no trained weights, no labelled set). */
typedef struct cf_place {
    int32_t frame, canvas;       /* frame in [0, Bf), canvas in [0, N) */
    cf_view view;                /* the source rectangle of the frame and the content rectangle in that canvas */
} cf_place;                      /* 40 bytes */
/* First-fit shelf packer; host only.  Items are the Bf * V (frame, view) pairs, frame-major (f ascending, then v ascending); an item
 * carries its view's (dw, dh), the view's own dx, dy are replaced.  Canvases are kept in creation order; a canvas has shelves
 * (y, height, x_next) in creation order and a y_next.  For each item, go through the canvases in order:
 *   1. through the canvas's shelves in order: if dh <= height and x_next + dw <= W, place the item at (x_next, y), x_next += dw + gutter;
 *   2. otherwise, if y_next + dh <= H, open a shelf y = y_next, height = dh, x_next = dw + gutter: the item at (0, y),
 *      y_next = y + dh + gutter;
 *   3. if no canvas takes the item, open a new canvas with the item at (0, 0) (its first shelf, by rule 2).
 * A view whose content is the whole canvas (a tile view) therefore gets a canvas of its own.  places[k] is item k (frame = k / V, view
 * k % V).  1080 x 1920 frames, 640 x 640 canvas, levels 1000, 500 and 250, Bf = 2, gutter 0, as (canvas, dx, dy):
 *   frame 0: (0, 0, 0), (0, 0, 360), (0, 320, 360); frame 1: (1, 0, 0), (1, 0, 360), (0, 480, 360); two canvases;
 *   gutter 16: (0, 0, 0), (0, 0, 376), (0, 336, 376), (1, 0, 0), (1, 0, 376), (1, 336, 376).
 * *n_places = Bf * V and *n_canvases are the numbers wanted; only the first `cap` placements are written.  CF_EINVAL, cf_op_last_error
 * naming the cause, for NULL views, n_places or n_canvases (or places with cap > 0), V < 1, Bf < 1, gutter < 0, cap < 0, H or W below 1,
 * a view with dw > W or dh > H, dw or dh below 1.  gutter = fill between contents. */
int cf_pack_views(const cf_view* views, int V, int Bf, int H, int W, int gutter, cf_place* places, int cap, int* n_places, int* n_canvases);
/* Bf frames of h x w in `format` and P placements -> the network batch of N canvases stated above -> forward.  Frames, formats, pitches,
 * the staging of host frames, the alignment of device planes and the even-sides rule exactly as for cf_forward_views; 1 <= N <=
 * max_batch (half of it under the flip test), 1 <= P, frame in [0, Bf), canvas in [0, N); every view passes the checks of
 * cf_forward_views' view table (the placement named by its index); two overlapping contents on one canvas are CF_EINVAL with both
 * placement indices in cf_last_error.  Every refusal comes before anything is enqueued; with ctx == NULL the arguments are still checked
 * (the content only for dx, dy >= 0 and dw, dh >= 1 as there is no canvas) and cf_op_last_error names the cause.  The cutter is ONE
 * launch that writes all N canvases, one writer per byte; a canvas tile no placement touches is stored as fill without reading a frame;
 * every tap lies inside its placement's source rectangle, pitch padding is never read; the frames are not modified.  The context
 * remembers the placements for cf_merge_packed until any other forward or upload.  Under cf_set_flip_test it mirrors whole canvases, as
 * cf_forward_views does.  cf_get_resized_input returns the N canvases.  cf_merge_views, cf_merge_tiles and cf_unfit_rows behind it are
 * CF_ESTATE. */
int cf_forward_packed(cf_ctx* ctx, int format, const cf_yuv_planes* frames, int in_on_device, int Bf, int h, int w, int pitch0, int pitch1,
                      const cf_place* places, int P, int N, const uint8_t* fill);
/* Merges the rows the LAST THRESHOLD DECODE kept for the N canvases of the last cf_forward_packed, per frame.  Frame f's candidates are
 * the rows i < min(count, the decode's max_out) of the canvas of each of its placements, walked in (placement index ascending, row
 * ascending) order.  Each row is tested against THAT placement's content with the three drop rules of cf_merge_views and mapped by the
 * same float64 expression; the greedy NMS of cf_merge_tiles then runs unchanged.  A row whose centre lies in another frame's content
 * fails this placement's centre rule and is picked up when that other placement is walked; a row whose centre lies in the fill belongs
 * to nobody.  flags bit 0 of frame f: a canvas that holds one of its placements had more rows than the decode's max_out.  The
 * compaction is a prefix sum: no atomics, deterministic.  The candidate capacity per frame is (most placements of any frame) x the
 * decode's max_out, and the CF_ENOMEM bound of cf_merge_views applies to it.  Outputs and out_on_device forms as cf_merge_views.
 * Afterwards the context is in the state behind a merge, with Bf frames of (h, w): every consumer takes the rows unchanged; before
 * cf_merge_packed they return CF_ESTATE.  CF_ESTATE unless the last forward was cf_forward_packed with a threshold decode behind it. */
int cf_merge_packed(cf_ctx* ctx, const cf_merge_opts* opts, int max_out, float* dets, float* lms, int32_t* counts, int32_t* flags,
                    int out_on_device);

/* ---- rotated sources through views and packed canvases: tiles and levels of a turned frame ----
 * cf_forward_rot puts ONE fitted or stretched whole frame on a canvas; cf_forward_views and cf_forward_packed take the stored frame for
 * upright.  A corridor-mode camera stores 1920 x 1080 and means 1080 x 1920: fitted upright into 640 x 640 that is a 360 x 640 content,
 * the faces down the corridor a handful of network pixels wide -- the case tiles and levels exist for.  cf_forward_packed_rot is
 * cf_forward_packed whose placements cut the UPRIGHT view U of the stored frame F, so a turned source gets tiles, levels and packing in
 * one batch, and the cf_merge_packed behind it returns the rows in the STORED frame's pixels: tracker, follower, redact, blur, draw,
 * frame chips, lookback and best shots keep working in place on the decoder's surface, as they do behind cf_forward_rot:
 *   cf_view_layout(hu, wu) + cf_pack_views (host, unchanged) -> cf_forward_packed_rot -> cf_decode_threshold* -> cf_merge_packed [-> ...]
 * rot in {0, 90, 180, 270} is the clockwise turn that makes F (h x w) upright, U is (hu, wu) = (h, w) for 0 and 180, (w, h) for 90 and
 * 270, and the index maps are those stated for cf_forward_rot.  Every placement's source rectangle is in pixels of U; the unpacked
 * form is the placement list {f, f * V + v, views[v]}.
 * Canvas: canvas n is `fill` everywhere, except inside each placement's content, where it is
 *   resize(bgr(U_f)[sy0 : sy0 + sh, sx0 : sx0 + sw], (dh, dw))
 * with bgr() taken per STORED pixel before the turn (a 4:2:0 pixel's chroma is that of its own 2 x 2 block in F) and the fixed-point
 * resize of cf_forward_views, taps clamped at the source rectangle.  rot == 0 IS cf_forward_packed: the same launch, the same bytes.
 * Merge: cf_merge_packed keeps its prototype and recognises a cf_forward_packed_rot behind the decode.  Per placement row it applies the
 * three drop rules of cf_merge_views in canvas coordinates, unchanged, except that "source side interior to the frame" is tested against
 * U: sx0 > 0, sx0 + sw < wu, sy0 > 0, sy0 + sh < hu.  A kept point (x, y) goes to the upright view first, in float64, in this order and
 * without contraction,
 *   ux(x) = ((double)x - dx) * ((double)sw / dw) + sx0,   uy(y) = ((double)y - dy) * ((double)sh / dh) + sy0,
 * then to the stored frame by the table of cf_unfit_rows, the difference taken in float64 and rounded to float32 once:
 *   rot  90: X = uy(y)            Y = (h-1) - ux(x)
 *   rot 180: X = (w-1) - ux(x)    Y = (h-1) - uy(y)
 *   rot 270: X = (w-1) - uy(y)    Y = ux(x)
 * Landmarks are mapped point by point in their order (no left / right swap); the box is the ASSIGNMENT of mapped corners stated for
 * cf_unfit_rows behind cf_forward_rot, never a min / max; the score is copied.  The greedy NMS of cf_merge_tiles then runs unchanged on
 * the stored-frame boxes; counts, flags, the truncated-canvas rule, the out_on_device forms and the CF_ENOMEM bound are cf_merge_packed's.
 * Afterwards the context is in the state behind a merge with Bf frames of (h, w) STORED.  rot 0 gives the bits of cf_merge_packed.
 * A single whole-frame placement with the rectangle of cf_rot_geometry reproduces the canvas of cf_forward_rot byte for byte; its rows
 * equal those of cf_unfit_rows behind cf_forward_rot in VALUE, not always in bits: the "+ sx0" adds + 0.0, which turns -0.0 into +0.0,
 * and this merge runs an NMS that the unfit does not.
 * Limits, plainly: no mirrored orientations (the other four EXIF codes); one rot per call (one camera, one mount: group the frames per
 * call); no probing of the orientation; the labels cf_draw_faces paints stay upright in the STORED frame; the threshold decode's NMS and
 * max_out are per canvas and so shared by the frames on it, as stated for packed views.  No trained weights and no labelled set are on hand: no accuracy
 * claim is made.
 *
 * Bf stored frames of h x w and P placements whose sources lie in the upright view -> N canvases -> forward.  Every check of
 * cf_forward_packed, with the source rectangles checked against (hu, wu), plus CF_EINVAL, the value named, for a rot outside the four;
 * h and w must be even for every format (an even rectangle of U is then an even rectangle of F).  Every refusal comes before anything is
 * enqueued; with ctx == NULL the arguments are still checked and cf_op_last_error names the cause.  rot 180 keeps the packed cutter's
 * layout with mirrored taps; a quarter turn transposes on the output side (a wave's lanes run along canvas rows, so its taps run along
 * stored rows and coalesce).  One launch writes all N canvases, one writer per byte; a canvas tile no placement touches is stored as
 * fill without reading a frame; every tap lies inside its placement's source rectangle mapped into F, pitch padding is never read; the
 * frames are not modified.  The context remembers rot, the placements and (h, w) until any other forward or upload; cf_merge_views,
 * cf_merge_tiles and cf_unfit_rows behind it are CF_ESTATE.  Under cf_set_flip_test it mirrors whole canvases, as cf_forward_packed does
 * (N <= max_batch / 2).  cf_get_resized_input returns the N canvases. */
int cf_forward_packed_rot(cf_ctx* ctx, int rot, int format, const cf_yuv_planes* frames, int in_on_device, int Bf, int h, int w,
                          int pitch0, int pitch1, const cf_place* places, int P, int N, const uint8_t* fill);

/* ---- face tracks across video frames: cover faces through detection dropouts -----------------
 * Every entry point above treats a frame as if it were the only one: the frame in which a face scores just under the threshold goes out
 * uncovered.  A cf_tracker associates the rows of each frame with the tracks of the frames before, on the device, and hands the
 * redaction the detections of the frame PLUS the tracks that were seen min_hits times running and then missed at most max_age frames:
 *   cf_forward* -> cf_decode_threshold* [-> cf_merge_tiles] -> cf_track_update -> cf_redact_faces | cf_blur_faces | cf_align_faces_frame
 * The defaults the Python layer uses are this project's choices; no accuracy claim is made for them.
 *
 * A tracker holds n_streams independent video streams on one device; stream s has max_tracks slots.  A slot holds: alive, id, hits,
 * misses, box[4], score, lms[10] (float32); the stream holds next_id (starts at 1, never reused).  One update of stream s with the rows
 * i < n = min(count, rows the decode / the merge wrote per image), in row order (the keep order):
 *   1. A row with a non-finite corner is skipped: it neither matches nor is born.
 *   2. Match.  For each remaining row in row order, over the slots that were alive when the update began and are not yet matched in this
 *      update: the decode's float32 "+1" IoU (areas (x2-x1+1)*(y2-y1+1), inter / (area_t + area_d - inter), float32 throughout, no
 *      FMA contraction).  The largest wins, ties go to the lowest slot, a NaN never wins.  A winner >= iou_thresh takes the row's box,
 *      score and landmarks as they are, hits = min(hits + 1, 1 << 30), misses = 0.  Otherwise the row is new.
 *   3. Age.  Every slot alive at the start and unmatched: hits < min_hits -> freed at once (a tentative track is never held);
 *      otherwise misses += 1, freed when misses > max_age.
 *   4. Birth.  New rows, in row order, take the lowest free slot (free after step 3): id = next_id++, hits = 1, misses = 0.  With no
 *      free slot the row is DROPPED and bit 0 of flags[s] is set: THAT FACE IS NOT IN THE OUTPUT AND WILL NOT BE COVERED.  Size
 *      max_tracks for the most faces a frame can show plus the tracks held through dropouts (80 bytes of device state per slot).
 *   5. Output.  The alive slots in ascending slot order are rows k < counts[s] <= max_tracks: dets[k] = box, score; lms[k]; info[k] =
 *      id, hits, misses (int32).  misses == 0: the box bit for bit.  misses > 0 (held): the box grown about its centre, in float64:
 *      cx = ((double)x1 + (double)x2) * 0.5; hw = ((double)x2 - (double)x1) * 0.5 * (1.0 + (double)hold_grow * (double)misses);
 *      x1' = (float)(cx - hw), x2' = (float)(cx + hw); y likewise.  THE LANDMARKS OF A HELD ROW ARE THE LAST ONES SEEN (not grown, not
 *      moved): chips cut from them by cf_align_faces_frame show whatever is at that place now.  (cf_track_follow, below, moves both.)
 * Coordinates are whatever the rows are in: network coordinates after an ordinary forward (whatever cf_set_rescale says), frame pixels
 * after cf_merge_tiles.  The tracker latches that space -- (not tiled, H, W), or (tiled, h, w) -- on its first update and refuses
 * another with CF_EINVAL. */
typedef struct cf_tracker cf_tracker;
typedef struct cf_track_opts {
    float   iou_thresh;   /* finite, in (0, 1] */
    int32_t max_age;      /* 0..1000 frames a confirmed track is held */
    int32_t min_hits;     /* 1..1000 */
    int32_t max_tracks;   /* 1..1024 per stream */
    float   hold_grow;    /* finite, 0..1 per missed frame */
} cf_track_opts;
/* ctx names the device (and carries the error text); 1..4096 streams.  CF_EINVAL for a bad option or count before any GPU work (ctx ==
 * NULL: the arguments are still checked first, cf_op_last_error names the cause).  *out is written on success only. */
int cf_track_create(cf_ctx* ctx, int n_streams, const cf_track_opts* opts, cf_tracker** out);
/* Waits for the tracker's last update, then frees it.  NULL: CF_OK. */
int cf_track_destroy(cf_tracker* trk);
/* A scene cut: frees every track of `stream` (-1: of all streams), ordered behind the updates issued so far and before those issued
 * later.  ids are not reused; the latched coordinate space stays.  CF_EINVAL for a stream outside -1 .. n_streams - 1. */
int cf_track_reset(cf_tracker* trk, int stream);
/* One update with the rows of the LAST THRESHOLD DECODE of the last forward of ctx (network coordinates); after cf_forward_tiles, with
 * the merged rows of the last cf_merge_tiles (frame pixels).  Image (frame) b is the next frame of stream stream0 + b; stream0 + B <=
 * n_streams.  dets [B][max_tracks][5], lms [B][max_tracks][10], info [B][max_tracks][3], counts [B], flags [B]; any may be NULL.
 * out_on_device as for cf_merge_tiles: device buffers are asynchronous on the stream that carried the decode or the merge, host buffers
 * block (rows at and past the largest count of the batch are not written).
 * CF_ESTATE without a decode (or, tiled, without a merge), once another upload or forward was started on ctx, and on a second update
 * behind the same decode / merge (time would advance twice).  CF_EINVAL, before any GPU work, for a stream range outside the tracker, a
 * tracker of another device, or a changed coordinate space.
 * The output rows live in buffers owned by the CONTEXT, the state in the tracker: a ring of contexts can share one tracker.  The
 * tracker keeps one event; every update first makes its stream wait for the previous update's event, then records a new one, so the
 * updates of one tracker are ordered across contexts in call order.
 * After a successful update, and until the next forward, upload, threshold decode or merge on ctx, cf_redact_faces, cf_blur_faces and
 * cf_align_faces_frame take the TRACKED rows (held ones included) instead of the decode's or the merge's; their B and (h, w) rules
 * are those of the rows the update consumed.  Without an update they do exactly what they did before. */
int cf_track_update(cf_ctx* ctx, cf_tracker* trk, int stream0, float* dets, float* lms, int32_t* info,
                    int32_t* counts, int32_t* flags, int out_on_device);

/* ---- two thresholds: a second association pass for low-score rows ----------------------------
 * A held box is stale: the face that scored 0.29 instead of 0.31 was seen by the detector, box and landmarks at the right place, and the
 * row was thrown away before the tracker could look at it.  A tracker created with two more numbers takes the rows of a decode at a
 * LOWER score threshold, lets the low-score rows match tracks that already exist, and lets them do nothing else (the association of
 * ByteTrack and its descendants; the defaults the Python layer uses are its customary values, nobody has measured them here and no
 * accuracy claim is made):
 *   birth_score: float32, finite, in (0, 1];   weak_iou: float32, finite, in (0, 1].
 * A row is STRONG when score > birth_score -- strict and in float32, because the threshold decodes keep cells with hm > score_thresh:
 * the strong rows of a decode at a lower threshold are then exactly the rows of a decode at birth_score (the NMS is greedy in descending
 * score order and keeps that order, cf_unfit_rows is a filter, cf_merge_tiles removes duplicates greedily by score; this holds as long
 * as no stage is cut by its max_out or its candidate limit).  Every other row is WEAK, a NaN score and score == birth_score included.
 * One update of a stream becomes:
 *   1.  Unchanged: a row with a non-finite corner is skipped, strong or weak.
 *   2a. Strong pass.  Step 2 above over the strong rows only, in row order.  A strong row without a winner >= iou_thresh is NEW.
 *   2b. Weak pass, after the strong pass has seen every strong row, over the weak rows in row order.  Eligible are the slots that were
 *       alive when the update began, are not yet matched in this update by either pass, and had hits >= min_hits when the update began:
 *       confirmed tracks, live or held; a tentative track is never matched by a weak row.  The measure, the arg-max, the tie rule (lowest
 *       slot) and the NaN rule are step 2's.  A winner with iou >= weak_iou takes the row's box, score and landmarks as they are, hits =
 *       min(hits + 1, 1 << 30), misses = 0 -- exactly what a strong match does.  Otherwise the row is DISCARDED: it is not new, it is
 *       never born, and it never sets flag bit 0.
 *   3 to 5. Unchanged, so a weak match stops the ageing and the row comes out ungrown, bit for bit.  Bit 1 (value 2) of flags[s] is set
 *       for a stream in whose update at least one weak row matched; bit 0 keeps its meaning.
 * A tracker created without the two numbers does what it did before, bit for bit.  What follows for the other objects:
 *   * cf_track_follow LEARNS a new template behind a weak match, because the box changed.
 *   * The lookback back-fills only strong births, because weak rows are never born.
 *   * The best-shot offer sees a weak-matched row as any live row (misses == 0); its score term already weighs it down.
 * The library never sees the threshold the caller decodes at; cf_track_update, cf_track_follow, cf_track_reset, the scene check and the
 * lookback take such a tracker unchanged. */
typedef struct cf_track_weak_opts {
    float birth_score;    /* finite, in (0, 1]: a row is strong when score > birth_score */
    float weak_iou;       /* finite, in (0, 1]: the match threshold of the weak pass */
} cf_track_weak_opts;
/* cf_track_create with the two numbers; weak == NULL is cf_track_create.  CF_EINVAL for a bad value before any GPU work, the cause in
 * cf_last_error (ctx == NULL: the arguments are still checked first, cf_op_last_error names the cause). */
int cf_track_create_weak(cf_ctx* ctx, int n_streams, const cf_track_opts* opts, const cf_track_weak_opts* weak, cf_tracker** out);

/* ---- constant velocity: tracks are matched where the face is expected, held boxes coast with it ----
 * A track above does not know that its face is moving: a held box stands where the face WAS, and the next detection is measured against
 * last frame's box, so a fast face that drops out for one frame comes back under a new id while the old track covers an empty place.  A
 * tracker created with cf_track_motion_opts keeps, per slot, vel = (vx, vy) in float32 beside the record (the motion model that SORT and
 * ByteTrack put in front of the association, reduced to the centre):
 *   gain: float32, finite, in (0, 1];   damp: float32, finite, in [0, 1].
 * All new arithmetic is float32, every operation rounded, no FMA contraction.  One update of a stream becomes:
 *   1'. Skip.  Step 1 as it is; in addition a row with a corner of magnitude above 16777216 (2^24) is skipped too.  This keeps every
 *       later quantity finite.
 *   P.  Predict.  For every slot alive when the update began, with stored box o and velocity v:
 *       P = (o.x1 + vx, o.y1 + vy, o.x2 + vx, o.y2 + vy).
 *   2'. Match.  Steps 2, 2a and 2b measure the IoU of P and the row, not of the stored box and the row.  The measure, the arg-max, the
 *       tie rule, the NaN rule, the thresholds and the eligibility (including "confirmed when the update began") are unchanged.  A winner
 *       takes the row's box d, score and landmarks as they are, as before.  Its velocity is updated from the values BEFORE the take --
 *       the stored box o, g = misses, hb = hits:
 *         cdx = (d.x1 + d.x2) * 0.5f;  cox = (o.x1 + o.x2) * 0.5f;  rx = (cdx - cox) - vx;
 *         a = hb == 1 ? 1.0f : gain;   vx' = vx + a * (rx / (float)(g + 1));        y likewise.
 *       hb == 1 is the track's second sighting: its velocity is still the 0 of birth, so the first measured displacement is taken whole.
 *   3'. Age.  Freeing tentative tracks and counting misses are unchanged.  A slot that stays alive unmatched (a held track) COASTS: every
 *       x of its box and of its ten landmarks becomes x + vx, every y becomes y + vy; then vel = (vx * damp, vy * damp).  If a coasted
 *       corner's magnitude exceeds 2^24 the slot is freed instead.
 *       Follower records: if the tracker has follower records, and the slot's tpl_id == id, and tpl_box equals the box before the coast bit
 *       for bit, then tpl_box takes the coasted box.  The next cf_track_follow then FOLLOWS from the coasted place with the template of
 *       the last detection; without this write it would LEARN whatever stands there.
 *   4'. Birth.  As it is, with vel = (0, 0): a reused slot never inherits a velocity.
 *   5.  Output.  Unchanged: the held row is the coasted box, grown by hold_grow, with its landmarks coasted with it.
 * What follows for the other objects:
 *   * cf_track_follow leaves vel alone.  It still LEARNS behind any match, because the box changed; behind a coast it now follows about
 *     the predicted centre.
 *   * With the follower running between updates, v is the motion per update that the follower has not already put into the box.
 *   * Lookback, best shots, redact, blur, draw and chips take the rows unchanged.
 *   * cf_track_reset and a scene cut need no word about velocities, because birth zeroes them.
 *   * Device state per slot becomes 88 bytes for a motion tracker.
 * THE LIMITS.  The model cannot bootstrap: a face so fast that its SECOND sighting misses iou_thresh against the unpredicted box is reborn
 * every frame, as before.  Only the centre moves; size is not predicted.  A wrong match yields a wrong velocity for a few frames.
 * Coasting at damp = 1 carries a held box max_age * v away.  gain = 0.5 and damp = 1.0 (SORT's coast) are this project's choices: there
 * is no labelled video here, nobody has measured them, and no accuracy claim is made.
 * A tracker created without these options runs the update it ran before, bit for bit. */
typedef struct cf_track_motion_opts {
    float gain;           /* finite, in (0, 1]: the share of a measured residual that the velocity takes from the third sighting on */
    float damp;           /* finite, in [0, 1]: what is left of the velocity after each coasted frame */
} cf_track_motion_opts;
/* cf_track_create with the weak and the motion options, each of which may be NULL; motion == NULL is cf_track_create_weak (with its
 * refusals, under its name).  CF_EINVAL for a bad value before any GPU work, after the plain and the weak checks: "gain must be finite
 * and in (0, 1]", "damp must be finite and in [0, 1]" (ctx == NULL: the arguments are still checked first, cf_op_last_error names the
 * cause). */
int cf_track_create_ex(cf_ctx* ctx, int n_streams, const cf_track_opts* opts, const cf_track_weak_opts* weak,
                       const cf_track_motion_opts* motion, cf_tracker** out);

/* ---- follow tracked faces between detections: block matching in the frame, on the device -----
 * cf_track_update leaves two holes: a held track does not move (hold_grow only inflates its box blindly, and its landmarks stay where
 * the face was), and every frame needs a forward, because the tracker advances only behind a decode.  cf_track_follow measures, from
 * the pixels of a new frame and WITHOUT A FORWARD, where every tracked face went, and moves the tracker's state there:
 *   key frame:       cf_forward* -> cf_decode_threshold* [-> cf_merge_tiles] -> cf_track_update -> cf_track_follow -> cf_redact_faces | ...
 *   frames between:                                                                                cf_track_follow -> cf_redact_faces | ...
 * The arithmetic is this library's own statement (csrc/cf_follow.hip; restated in tests/follow_cases.py; device and restatement are
 * equal bit for bit).  Integers throughout, except the box geometry and the move: float64 in the order written, no FMA contraction.
 * The defaults the Python layer uses (search 4, max_sad 4096) are this project's choices; no accuracy claim is made for them.
 *
 * P = 16 is the template side in cells, R = opts->search.  A tracker that was followed at least once holds, per slot, a follower record
 * (allocated by the first follow, 280 bytes per slot, all zero at first): tpl[16][16] uint8, tpl_c, tpl_id, tpl_box[4] = the bit
 * patterns of the slot's box as the follower last left it.
 *   Luma.  Of a 4:2:0 frame: the sample's Y byte.  Of a BGR frame: (29*B + 150*G + 77*R + 128) >> 8.
 *   Geometry.  Frames of h x w; the tracker's latched row space is H x W.  Network space: fx = (double)w / (double)W, fy = (double)h /
 *   (double)H.  Frame space (rows of cf_merge_tiles): fx = fy = 1, and (h, w) must be the latched size.  For every alive slot of the
 *   streams stream0 .. stream0 + B - 1, with the slot's box (x1, y1, x2, y2) as the state holds it (not grown):
 *     side = max(((double)x2 - (double)x1) * fx, ((double)y2 - (double)y1) * fy).  The slot is skipped, code NONE, when a corner is not
 *     finite or side is not > 0.
 *     cx = ((double)x1 + (double)x2) * 0.5 * fx clamped to [-8192, 16384], CX = (int)floor(cx); CY likewise with y and fy.
 *     S = (int)ceil(side clamped to [1, 8192]); cell size c = (S + 15) / 16 (integer division; 1..512).
 *   Cell (i, j) about (CX, CY), i and j possibly negative, covers the pixels [CX + i*c, CX + (i+1)*c) x [CY + j*c, CY + (j+1)*c), their
 *   coordinates clamped into the frame (the border replicates); its value is (sum of luma + c*c/2) / (c*c) (the sum fits int32).
 *   Learn or follow, decided per slot on the device:
 *     LEARN when tpl_id != id or the box differs in any bit from tpl_box -- the slot is new, or an update matched a detection into it.
 *       tpl = the cells i, j in [-8, 8) of this frame, tpl_c = c, tpl_id = id, tpl_box = the box.  Code LEARNED, moves 0, 0, 0.
 *     FOLLOW otherwise, with c = tpl_c.  Window: the cells i, j in [-8-R, 8+R) about the CURRENT (CX, CY).  For every (dx, dy) in
 *       [-R, R]^2: SAD = sum over the 256 template cells of |win[j+dy][i+dx] - tpl[j][i]|.  The best displacement has the smallest SAD,
 *       then the smallest dx*dx + dy*dy, then the smallest dy, then the smallest dx; px = dx*c, py = dy*c.
 *       SAD > max_sad: code LOST, nothing moves (moves = px, py, SAD of the best displacement all the same).
 *       Otherwise every x of the box and of the ten landmarks becomes (float)((double)x + (double)px / fx), every y
 *       (float)((double)y + (double)py / fy); the state and tpl_box take the new box; code MOVED.
 *       THE TEMPLATE IS NOT REFRESHED BY A FOLLOW: it stays that of the last detection, so the quantisation to c pixels does not add up.
 *   hits, misses, ids and flags are untouched: a followed frame is not a detection opportunity, max_age keeps counting detections.
 *   Output.  The context's tracked rows are written again from the state by step 5 of cf_track_update (alive slots in slot order, held
 *   boxes grown by hold_grow, info = id, hits, misses), and moves[B][max_tracks][4] int32 = px, py, SAD, code in the same row order.
 * So: at a key frame (update, then follow) the matched and the newborn slots learn and the held slots move with their face; between
 * key frames every slot moves; a slot reused under a new id learns again; cf_track_reset needs no word about the follower.
 * On the device: one workgroup per (slot, stream) and a second launch of one wave per stream for the rows.  THE COST GROWS WITH THE
 * FACE'S AREA: c*c pixels per cell, (16 + 2R)^2 cells per followed face. */
#define CF_FOLLOW_NONE    0
#define CF_FOLLOW_LEARNED 1
#define CF_FOLLOW_MOVED   2
#define CF_FOLLOW_LOST    3
typedef struct cf_follow_opts {
    int32_t search;       /* R, 1..8 cells */
    int32_t max_sad;      /* 0..65280: a best match above it is LOST */
} cf_follow_opts;
/* Follows the streams stream0 .. stream0 + B - 1 of trk in frames[b] (b < B; frame b is the current frame of stream stream0 + b).
 * Frames, formats, pitches, alignment and on_device are those of cf_redact_faces; the frames are only read (host frames are copied up,
 * never back).  IT NEEDS NO FORWARD ON ctx: everything comes from the tracker, so a chunk loop or a ring of contexts can follow any
 * streams on any context of the tracker's device.  The call orders itself on the tracker's event exactly as cf_track_update does.
 * dets [B][max_tracks][5], lms [B][max_tracks][10], info [B][max_tracks][3], counts [B], moves [B][max_tracks][4]; any may be NULL;
 * out_on_device as for cf_track_update.
 * CF_ESTATE when the tracker was never updated (it has no row space yet).  CF_EINVAL, before any GPU work, for: bad options, a stream
 * range outside the tracker, B outside 1..max_batch, a tracker of another device, in frame space an (h, w) that is not the latched one,
 * and every geometry and plane error of the redaction (ctx == NULL: the options and the geometry are still checked first,
 * cf_op_last_error names the cause).  CF_ENOMEM, before any launch, when the follower records do not fit.
 * Afterwards, and until the next forward, threshold decode, merge or update on ctx, cf_redact_faces, cf_blur_faces,
 * cf_align_faces_frame and cf_draw_faces (CF_DRAW_LABEL_ID included) take THESE rows: their B is the follow's B, their coordinates the
 * tracker's space.  Calls that name the decode's own rows -- cf_align_faces, cf_merge_tiles -- and the refusal of a second
 * cf_track_update behave as before. */
int cf_track_follow(cf_ctx* ctx, cf_tracker* trk, int stream0, int B, const cf_follow_opts* opts, int format, const cf_planes_rw* frames,
                    int on_device, int h, int w, int pitch0, int pitch1, float* dets, float* lms, int32_t* info, int32_t* counts,
                    int32_t* moves, int out_on_device);

/* ---- scene cuts: found in the luma on the device, the cut streams' tracks reset without a host round trip -------------------------
 * Tracks, the follower, the best shots and the annotation all assume that frame n + 1 continues frame n.  At an edit point of a video it
 * does not: held tracks keep covering the places where the previous scene's faces stood, the follower matches old templates against
 * unrelated pixels, and follow-only frames cover nothing that is new.  cf_track_reset is the remedy, but a host call the caller has to
 * time by hand.  cf_scene_check measures whether a frame continues its stream and, where it does not, frees the stream's tracks on the
 * device:
 *   frame -> cf_scene_check [resets the cut streams' tracks] -> (cf_forward* -> decode -> cf_track_update)? -> cf_track_follow -> ...
 * CALL IT BEFORE THE FRAME'S UPDATE OR FOLLOW.  The arithmetic is this library's own statement (csrc/cf_scene.hip; restated in
 * tests/scene_cases.py; device and restatement are equal bit for bit).  All integers.  The defaults the Python layer uses (hist 350,
 * grid 640) are this project's choices: there is no labelled video here, nobody has measured them, and no accuracy claim is made.
 *
 *   Luma.  The follower's: of a 4:2:0 frame the sample's Y byte, of a BGR frame (29*B + 150*G + 77*R + 128) >> 8.
 *   Signature of an h x w frame, 128 int32:
 *     bins[k], k < 64: the number of pixels with luma >> 2 == k.
 *     mean[8*j + i], i, j < 8: cell (i, j) covers x in [(i*w)/8, ((i+1)*w)/8) and y in [(j*h)/8, ((j+1)*h)/8) (integer division; the
 *       cells differ in size when 8 does not divide the side).  With n pixels in the cell the value is (sum of luma + n/2) / n.  A cell
 *       sum stays below 2^31 for every allowed frame size.
 *     Pitch padding bytes never count.
 *   State per stream of a cf_scene: the last signature, the (h, w) it was taken at, valid, run; all zero at first.
 *   One check of stream s with a frame, N = h*w:
 *     FIRST when the state is not valid or its (h, w) differ from the frame's: hist = grid = 0, run = 0.  Nothing is reset.
 *     Otherwise A = sum_k |bins[k] - prev.bins[k]| (int64), hist = (A * 1000) / (2 * N), in 0..1000: the per mille of pixels that
 *       changed bin; grid = sum_k |mean[k] - prev.mean[k]|, in 0..16320.
 *       CUT when hist >= hist_thresh && grid >= grid_thresh; run = 0.
 *       SAME otherwise; run = min(run + 1, 1 << 30).
 *     After any code the state takes the frame's signature and (h, w), valid = 1.
 *     Output: out[b][4] int32 = code, hist, grid, run.
 *     On CUT with a tracker given every slot of stream s is freed exactly as cf_track_reset(trk, s) frees it: the slots' meta words
 *     become zero, next_id is untouched (ids are not reused), the latched space stays, the follower records need no word.  This is
 *     decided and done by the kernel; no count or code is read on the host.
 * Both conditions must hold: a pan changes the cell means but not the histogram, a face-sized object entering changes neither much.
 * TWO LIMITS.  A full-frame brightness jump (a flash) changes both measures and is reported as a cut; the cost is lost held tracks, not
 * uncovered detections.  A dissolve is not one cut: no pair of neighbouring frames differs enough.
 * On the device: one bandwidth-bound pass over the luma (many workgroups per frame, each leaving 72 int32 partials) and one wave per
 * stream that finishes the sums, decides, resets and stores the signature. */
#define CF_SCENE_FIRST 0
#define CF_SCENE_SAME  1
#define CF_SCENE_CUT   2
typedef struct cf_scene cf_scene;
typedef struct cf_scene_opts {
    int32_t hist_thresh;  /* 0..1000 per mille */
    int32_t grid_thresh;  /* 0..16320 */
} cf_scene_opts;
/* ctx names the device (and carries the error text); 1..4096 streams.  CF_EINVAL for a bad option or count before any GPU work (ctx ==
 * NULL: the arguments are still checked first, cf_op_last_error names the cause).  *out is written on success only. */
int cf_scene_create(cf_ctx* ctx, int n_streams, const cf_scene_opts* opts, cf_scene** out);
/* Waits for the object's last check, then frees it.  NULL: CF_OK. */
int cf_scene_destroy(cf_scene* scn);
/* The next check of `stream` (-1: of every stream) is FIRST; ordered behind the checks issued so far and before those issued later.
 * CF_EINVAL for a stream outside -1 .. n_streams - 1. */
int cf_scene_forget(cf_scene* scn, int stream);
/* Checks the streams stream0 .. stream0 + B - 1 of scn with frames[b] (frame b is the current frame of stream stream0 + b) and, with trk
 * not NULL, resets the tracks of the streams that are CUT.  Frames, formats, pitches, alignment, on_device and the h / w rules are those
 * of cf_track_follow (h and w even, at most 8192; the frames are only read, host frames are copied up, never back); in addition h, w >=
 * 8, so that every cell holds a pixel.  IT NEEDS NO FORWARD ON ctx, does not touch the rows ctx holds and does not change which rows the
 * redaction, the blur, the chips or the annotation take.  A cf_scene owns its state, a stream and an event, like a cf_tracker: a check
 * makes the context's stream wait for the event of the check before it and records a new one, and with trk does the same on the tracker's
 * event, so a ring of contexts can share both objects in call order.  out [B][4] (may be NULL); out_on_device = 1: a device buffer,
 * asynchronous on the context's stream, nothing is read on the host; 0: a host buffer, the call blocks.
 * CF_EINVAL, before any GPU work, for: a stream range outside scn or trk, B outside 1..max_batch, an object of another device, and every
 * geometry and plane error of the follower (ctx == NULL: the geometry is still checked first, cf_op_last_error names the cause). */
int cf_scene_check(cf_ctx* ctx, cf_scene* scn, cf_tracker* trk, int stream0, int B, int format, const cf_planes_rw* frames,
                   int on_device, int h, int w, int pitch0, int pitch1, int32_t* out, int out_on_device);

/* ---- lookback: cover faces in the frames BEFORE their first detection -----------------------------------------------------------
 * cf_track_update, cf_track_follow and cf_scene_check close holes that lie behind a detection.  The hole in front of it is still open: a
 * face that enters the picture, turns to the camera or comes into focus is visible for several frames before it first scores above the
 * threshold, and those frames go out uncovered.  The tracker knows only the past, and a tentative track is never held (min_hits): an
 * onset that flickers hit, miss, hit leaves the middle frame bare.  A cf_lookback delays the output by `depth` frames and paints a
 * track's first box backwards: it keeps the last frames' tracked rows per stream on the device and hands out the rows of the frame
 * `depth` steps back PLUS the first boxes of every track born since, grown by the distance:
 *   ... -> cf_track_update [-> cf_track_follow] -> cf_lookback_step -> cf_redact_faces | cf_blur_faces | cf_draw_faces (ON THE FRAME OF
 *   `depth` STEPS AGO, which the caller keeps)
 * No row, count or code crosses to the host.  The defaults the Python layer uses (depth 8, grow 0.05, confirm 1) are this project's
 * choices: there is no labelled video here, nobody has measured them, and no accuracy claim is made.
 *
 * A cf_lookback holds n_streams independent streams on one device.  A stream holds: a queue of at most depth + 1 entries, oldest first;
 * max_id, seq_next, pending_cut, all 0 at first.  An entry holds seq, cut, n and n rows; a row holds box[4], score, lms[10] (float32),
 * id, hits, misses (int32) and born.  One step of stream s (image b of the call):
 *   1. Push, when push != 0.  n = min(max(count, 0), the stride of the pushed rows, rows).  A new entry takes the image's tracked rows
 *      i < n bit for bit: dets, lms and info = id, hits, misses as step 5 of cf_track_update or cf_track_follow left them.  seq =
 *      seq_next++.  cut = pending_cut || (scene codes given && code[b][0] != CF_SCENE_SAME); then pending_cut = 0.  born[i] = id[i] >
 *      max_id with max_id as it was before this step; then max_id becomes the largest id seen.  The entry is appended.
 *   2. Emit.  After a push: when the queue holds depth + 1 entries.  Without a push (a drain): when the queue is not empty.  Otherwise
 *      nothing is emitted: counts[b] = 0 and state[b] = -1, 0, 0, 0.
 *   3. An emit takes the oldest entry t out of the queue; e_1 .. e_m (m <= depth) are the entries that remain, oldest first.
 *      Own rows.  The output rows k < n_t are t's rows, bit for bit, in order.
 *      Back-filled rows.  For j = 1 .. m in order, STOPPING at the first e_j with cut set (it and everything behind it belong to another
 *      scene; a cut on t itself stops nothing): the rows i of e_j in row order with born set are eligible when (a) their four corners
 *      are finite and (b) their id occurs in at least `confirm` of the entries e_j .. e_m, counted up to but not including the next
 *      entry with cut set.  While fewer than `rows` rows are written an eligible row is appended; otherwise it is DROPPED and bit 0 of
 *      the flags is set: THAT FACE IS NOT COVERED IN THIS FRAME.  The appended row: the box grown about its centre in float64 by g = 1.0
 *      + (double)grow * (double)j -- cx = ((double)x1 + (double)x2) * 0.5; hw = ((double)x2 - (double)x1) * 0.5 * g; x1' = (float)(cx -
 *      hw), x2' = (float)(cx + hw); y likewise (the order of the tracker's held rows, no contraction) --, score and landmarks as
 *      stored, info = id, 0, j.  THE LANDMARKS OF A BACK-FILLED ROW ARE THOSE OF THE TRACK'S FIRST FRAME (not grown, not moved), and so
 *      is the box's place: the face is covered where it was FIRST SEEN, j frames later.  With hits = 0 and misses = j > 0
 *      cf_draw_faces draws the row as a held one and the best-shot offer never scores it.
 *      state[b] = seq_t, n_t, rows appended, flags.
 * On the device: one launch per step, one workgroup per stream; the queue is a rotating array whose head and fill live in device
 * memory (80 bytes per row, (depth + 1) * rows rows per stream). */
typedef struct cf_lookback cf_lookback;
typedef struct cf_lookback_opts {
    int32_t depth;        /* 1..32 frames of delay */
    int32_t rows;         /* 1..1024: capacity of an entry AND of an output image; the stride of every output table */
    float   grow;         /* finite, 0..1 per frame of distance */
    int32_t confirm;      /* 1..depth + 1 queued frames that must show a new id before it is back-filled (at most depth entries are
                           * counted, e_j .. e_m: depth + 1 is never met and back-fills nothing) */
} cf_lookback_opts;
/* ctx names the device (and carries the error text); 1..4096 streams.  CF_EINVAL for a bad option or count before any GPU work (ctx ==
 * NULL: the arguments are still checked first, cf_op_last_error names the cause); CF_ENOMEM when the queues do not fit.  *out is written
 * on success only. */
int cf_lookback_create(cf_ctx* ctx, int n_streams, const cf_lookback_opts* opts, cf_lookback** out);
/* Waits for the object's last step, then frees it.  NULL: CF_OK. */
int cf_lookback_destroy(cf_lookback* lb);
/* Sets pending_cut of `stream` (-1: of every stream): nothing pushed later is painted back into what is queued now.  For callers that
 * reset tracks themselves (cf_track_reset).  Ordered like cf_track_reset: behind the steps issued so far, before those issued later.
 * CF_EINVAL for a stream outside -1 .. n_streams - 1. */
int cf_lookback_forget(cf_lookback* lb, int stream);
/* One step of the streams stream0 .. stream0 + B - 1 (image b is stream stream0 + b).  push != 0: ctx must hold tracked rows that no step
 * has consumed -- the tracked rows behind a cf_track_update or the followed rows behind a cf_track_follow -- of B images, else CF_ESTATE;
 * a second push behind the same rows is CF_ESTATE (time would advance twice).  push == 0 (a drain, the end of the video) needs no
 * forward, only an object that was pushed into before (CF_ESTATE otherwise: its rows have no coordinate space yet).  scene: [B][4]
 * exactly as cf_scene_check wrote it (scene_on_device: a device buffer, read on ctx's stream; else a host table, copied up before the call returns), or NULL.
 * The object latches the row space -- (not tiled, H, W) or (tiled, h, w) -- and the stride of the pushed rows (<= rows) on its first push;
 * another space or stride later is CF_EINVAL.  CF_EINVAL also, before any GPU work, for B outside 1..max_batch, a stream range outside
 * the object and an object of another device (ctx == NULL: B is still checked first, cf_op_last_error names the cause).
 * dets [B][rows][5], lms [B][rows][10], info [B][rows][3], counts [B], state [B][4]; any may be NULL; out_on_device as for
 * cf_track_update (host buffers block; rows at and past the largest count of the batch are not written).
 * After a successful step, and until the next forward, upload, threshold decode, merge, update or follow on ctx, cf_redact_faces,
 * cf_blur_faces, cf_draw_faces and cf_align_faces_frame take the LOOKBACK ROWS, with the step's B and the latched space: GIVE THEM THE
 * FRAMES OF `depth` STEPS AGO.  cf_align_faces, cf_merge_tiles, cf_unfit_rows and the refusal of a second cf_track_update behave as
 * before.  The rows live in buffers owned by the CONTEXT, the queues in the object: a ring of contexts can share one object; it keeps one
 * event and orders its steps across contexts exactly as a tracker orders its updates. */
int cf_lookback_step(cf_ctx* ctx, cf_lookback* lb, int stream0, int B, int push, const int32_t* scene, int scene_on_device,
                     float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* state, int out_on_device);

/* ---- lookback with a trace: the back-filled boxes follow the face through the queued frames (opt-in) ---------------------------------
 * cf_lookback_step paints a back-filled box where the face was first detected.  A person who walks into the picture is not there in the
 * frames before: at 12 pixels per frame the face is 96 pixels from its birth box at distance 8.  With cf_lookback_trace_enable the
 * object also keeps the LUMA of every queued frame on the device, a pushing step matches every newborn face BACKWARDS through those
 * planes with the follower's block matching (cell means, a 16 x 16 cell template, SAD search, one 64-bit min key: see "follow tracked
 * faces between detections"), and the emit moves the back-filled box to where the walk found the face.  cf_follow_opts is the
 * follower's (search R in 1..8, max_sad in 0..65280); the defaults the Python layer uses (4, 4096) are this project's choices:
 * no accuracy claim is made.  WITHOUT THE CALL EVERYTHING ABOVE HOLDS AS IT STANDS, bit for bit.
 *
 * cf_lookback_trace_enable allocates, for an object nothing was pushed into yet, the luma ring -- per stream depth + 1 planes of h rows
 * of (w + 15) & ~15 bytes: 16 streams, depth 8, 1920 x 1080: 298 MB -- and the trace table -- per queue entry rows x depth x 4 int32.
 * CF_ESTATE when the object was pushed into already (an entry without luma cannot be traced through) or is enabled already.  CF_EINVAL,
 * before any GPU work, for bad options (the follower's texts), h or w odd, below 2 or above 8192, and an object of another device (ctx
 * == NULL: the arguments are still checked first, cf_op_last_error names the cause).  CF_ENOMEM when the ring does not fit.
 *
 * Once enabled: cf_lookback_step with push != 0 is CF_ESTATE (the frame is missing); with push == 0 it stays allowed and emits what
 * cf_lookback_step_frames with push == 0 emits.  cf_lookback_step_frames on an object that is not enabled is CF_ESTATE; a pushed (h, w)
 * other than the enabled one is CF_EINVAL.  Frames, formats, pitches, alignment and on_device are those of cf_track_follow (the frames
 * are only read; host frames are copied up, never back); every state rule -- which rows a push takes, the refusal of a second push, which
 * calls take the lookback rows afterwards, the ordering on the object's event -- is cf_lookback_step's.  With push == 0, frames may be
 * NULL and the frame arguments are ignored.
 *
 * A step with push, per stream; frames[b] MUST be the frame the pushed rows belong to.
 *   1. Retain.  The luma of frames[b] -- the follower's: the Y byte, or (29*B + 150*G + 77*R + 128) >> 8 -- is stored in the ring plane of
 *      the entry the push fills, which is decided from the queue's words on the device: no head or fill is read on the host.
 *   2. Push.  As step 1 of cf_lookback_step.
 *   3. Trace.  After the push the queue is q_0 (oldest) .. q_m = E (the new entry), m <= depth; L_k is the retained luma of q_k.  Rows
 *      in network space: fx = w / W, fy = h / H in float64; rows in frame space: fx = fy = 1 and (h, w) must be the latched size; which
 *      of the two is what the object latched on its first push.  For every row i of E with born set and four finite corners:
 *        Learn.  The follower's geometry from the row's box as stored: side, CX, CY, S, c = (S + 15) / 16.  When side is not > 0 the
 *          row's trace is 0, 0, 0, CF_FOLLOW_NONE at every distance.  Otherwise tpl = the cells i, j in [-8, 8) about (CX, CY) in L_m,
 *          and PX = PY = 0.
 *        Walk, for d = 1 .. m:  (a) if q_(m-d+1) has cut set (for d = 1 that is E itself) the chain ends; those distances are never
 *          read by an emit.  (b) Window = the cells [-8-R, 8+R) of size c about (CX + PX, CY + PY) in L_(m-d).  (c) The best (dx, dy) in
 *          [-R, R]^2 by the follower's key: smallest SAD, then dx*dx + dy*dy, then dy, then dx.  (d) SAD > max_sad: T[i][d] = PX, PY,
 *          SAD, CF_FOLLOW_LOST; the chain ends, and every further distance takes the same four words.  (e) Otherwise PX += dx*c, PY +=
 *          dy*c and T[i][d] = PX, PY, SAD, CF_FOLLOW_MOVED.
 *        The template is that of the birth frame throughout: nothing is refreshed, nothing is kept past the step.  Integers throughout.
 *   4. Emit.  As steps 2 and 3 of cf_lookback_step -- eligibility, confirm, the stop at a cut, the `rows` capacity with its flag bit and
 *      the order are unchanged -- except for the appended back-filled rows: a row of e_j at distance j reads (PX, PY, SAD, code) =
 *      T[row][j] of e_j's table.  PX == 0 and PY == 0: the row is appended exactly as by cf_lookback_step.  Otherwise every x of the box
 *      and of the ten landmarks becomes (float)((double)x + (double)PX / fx), every y (float)((double)y + (double)PY / fy) (the
 *      follower's formula), and THEN the moved box is grown by g = 1 + grow * j in the order stated above.  info = id, 0, j as before.
 *      moves[b][rows][4] = PX, PY, SAD, code for the back-filled rows and 0, 0, 0, CF_FOLLOW_NONE for own rows; rows at and past the
 *      largest count of the batch are not written.
 * So: on a sequence in which displacement 0 is always the best match -- identical frames, by the smallest-move tie rule -- the output
 * equals that of cf_lookback_step bit for bit.  A LOST chain leaves the box where the walk last had the face.
 * On the device: a bandwidth-bound retain pass per pushed frame (16-byte loads and stores; 48 BGR bytes give 16 lumas), one workgroup
 * per (pushed row, stream) for the trace, which leaves at once for a row that is not born, and the one launch of cf_lookback_step. */
int cf_lookback_trace_enable(cf_ctx* ctx, cf_lookback* lb, const cf_follow_opts* opts, int h, int w);
/* dets [B][rows][5], lms [B][rows][10], info [B][rows][3], counts [B], state [B][4], moves [B][rows][4]; any may be NULL; out_on_device as
 * for cf_lookback_step.  CF_EINVAL, before any GPU work, for B below 1 and, with push != 0, every geometry and plane error of
 * cf_track_follow (ctx == NULL: these are still checked first, cf_op_last_error names the cause). */
int cf_lookback_step_frames(cf_ctx* ctx, cf_lookback* lb, int stream0, int B, int push, const int32_t* scene, int scene_on_device,
                            int format, const cf_planes_rw* frames, int on_device, int h, int w, int pitch0, int pitch1,
                            float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* state, int32_t* moves, int out_on_device);

/* ---- best-shot selection: each track's sharpest chip, kept on the device -----------------------------------------------------
 * cf_track_update / cf_track_follow give every face an identity, cf_align_faces_frame cuts a chip of every tracked row: a track that
 * lives 200 frames yields 200 chips.  A cf_bestshot table is offered the chips of each frame, scores them, and keeps PER TRACK ID the
 * chip with the highest quality; when the id disappears from the tracked rows the entry is finished, and cf_bestshot_collect hands the
 * finished entries out in finishing order -- one chip per appearance of a person.  In the device form no chip, box or count crosses to
 * the host:
 *   ... -> cf_track_update [-> cf_track_follow] -> cf_align_faces_frame (chips, offsets) -> cf_bestshot_offer ...  cf_bestshot_collect
 * The arithmetic is this library's own statement (csrc/cf_bestshot.hip; restated in tests/bestshot_cases.py; device and restatement are
 * equal bit for bit): integers throughout, except a few float64 terms in the order written, no FMA contraction.  THE QUALITY FORMULA IS
 * THIS PROJECT'S CHOICE; no accuracy claim is made for it.
 *
 * Quality of one chip.  Inputs: a uint8 [S][S][3] BGR chip, its row (x1, y1, x2, y2), score, lms[10] (float32), and fx, fy (float64).
 *   1. Luma.  L = (29*B + 150*G + 77*R + 128) >> 8 (the follower's luma).
 *   2. Sharpness.  The window is the central half: a = S/4, b = 3*S/4, pixels a <= x, y < b, N = (S/2)*(S/2).
 *      lap = 4*L[y][x] - L[y-1][x] - L[y+1][x] - L[y][x-1] - L[y][x+1] (the neighbours exist because a >= 4).
 *      S1 = sum lap, S2 = sum lap*lap (int64); V = N*S2 - S1*S1; sharp = V / (N*N).  V >= 0: the division needs no sign rule.  Range
 *      0 .. 1 040 400; at S = 512, N*S2 <= 4.5e15 and S1*S1 <= 4.5e15 fit int64.  This is the variance of the 4-neighbour Laplacian; it
 *      leaves out the chip border, where the warp's zero border would count as an edge.
 *   3. size_w: 256 when CF_BEST_SIZE is off.  wx = ((double)x2 - (double)x1) * fx, wy = ((double)y2 - (double)y1) * fy.
 *      !(wx > 0) || !(wy > 0): 0.  Otherwise side = wx < wy ? wx : wy, side_i = side >= (double)S ? S : (int)floor(side),
 *      size_w = side_i * 256 / S.  (A face larger than the chip gains nothing more: the chip is point-sampled.)
 *   4. pose_w: 256 when CF_BEST_POSE is off; 0 when any of the ten landmark values is not finite.
 *      Pj = ((double)lms[2j] * fx, (double)lms[2j+1] * fy); ex = (P0x + P1x) * 0.5, ey = (P0y + P1y) * 0.5; mx = (P3x + P4x) * 0.5,
 *      my = (P3y + P4y) * 0.5; ax = mx - ex, ay = my - ey; dx = P2x - ex, dy = P2y - ey; cr = ax*dy - ay*dx; len2 = ax*ax + ay*ay.
 *      !(len2 > 0): 0.  Otherwise t = fabs(cr) / len2 * 512.0, pose_w = !(t < 256.0) ? 0 : 256 - (int)floor(t).  (The nose's sideways
 *      offset from the eye-mouth axis, in units of that axis: 0.5 or more gives 0.)
 *   5. score_w: 256 when CF_BEST_SCORE is off.  t = (double)score * 256.0; score_w = !(t > 0) ? 0 : (t >= 256.0 ? 256 : (int)floor(t)).
 *   6. Q = (int64)sharp * size_w * pose_w * score_w (at most 1.8e13); parts = sharp, size_w, pose_w, score_w.
 *   (A flat chip gives sharp 0; grey columns alternating 100 / 110 give 400; a grey 0 / 255 checkerboard gives 1 040 400.)
 *
 * The table.  Each stream has E entries, each FREE, LIVE or DONE.  An entry holds id, Q, parts, best_t, first_t, last_t, n_offered,
 * done_seq, det[5] and lms[10] (the row of the best frame, bit for bit) and the chip.  Each stream also holds an offer counter t and a
 * finish counter seq, both starting at 0, and sticky flags.
 *
 * One offer of stream s.  The rows are the context's newest TRACKED rows of image b: i < n = min(count, rows per image), with
 * info = id, hits, misses.  The caller's chips and offsets[B+1] are as cf_align_faces_frame writes them.  Row i has chip
 * c = offsets[b] + i iff 0 <= offsets[b] <= offsets[b+1], i < offsets[b+1] - offsets[b] and c < cap_faces; anything else is "no chip",
 * never an out-of-range read.  (Offsets as the align calls write them never name a chip twice; should malformed ones do, the chip is
 * that of the lowest image naming it and the others' rows have no chip.)
 *   1. A row COUNTS if id >= 1 and no earlier row of the image has the same id.
 *   2. Every LIVE entry, in ascending entry order: its id is among the counted rows -> last_t = t; otherwise the entry becomes DONE
 *      with done_seq = seq++.
 *   3. Counted rows in row order.  A row is eligible iff misses == 0 && hits >= min_hits and it has a chip.  (A row held through a
 *      dropout shows whatever is at that place now, so it is never offered; its id is still present, so its entry stays alive.)  For an
 *      eligible row, compute Q:
 *        a LIVE entry holds the id: n_offered = min(n_offered + 1, 1 << 30); if Q > entry.Q (strictly: the earlier frame wins a tie)
 *          the entry takes Q, parts, best_t = t, det, lms and the chip.
 *        no entry holds it: the lowest FREE entry (DONE entries are not free) becomes LIVE with first_t = best_t = last_t = t,
 *          n_offered = 1, and Q, parts, det, lms and the chip.
 *        there is none: the row is not entered; bit 0 is set in this offer's flags and in the stream's sticky flags.  It may enter on
 *          a later frame.
 *   4. t += 1.
 *
 * Collect of stream s with cap and flush.
 *   1. flush: every LIVE entry becomes DONE, in ascending entry order with consecutive seqs (the end of the video).
 *   2. The DONE entries in ascending done_seq: the first min(n_done, cap) are output as rows k and become FREE.
 *   3. counts[s] is that number, pending[s] what stays DONE.  4. flags[s] = the sticky flags, which are then cleared.
 *   5. records[k] = id, best_t, first_t, last_t, n_offered, sharp, size_w | pose_w << 10 | score_w << 20, done_seq (int32).
 *   6. Rows at and past counts[s] are not written.
 *
 * On the device an offer is three launches (score: one workgroup per chip; decide: one per stream; copy) and a collect two. */
#define CF_BEST_SIZE  1
#define CF_BEST_POSE  2
#define CF_BEST_SCORE 4
typedef struct cf_bestshot_opts {
    int32_t size;      /* S: chip side, a multiple of 4 in [16, 512]; chips are CF_CHIP_U8_HWC_BGR */
    int32_t entries;   /* E: 1..2048 table entries per stream (live tracks + finished ones not yet collected) */
    int32_t min_hits;  /* 1..1000: a row is offered only with hits >= min_hits */
    int32_t terms;     /* 0..7: which of the three weights take part (CF_BEST_*); sharpness always does */
} cf_bestshot_opts;   /* 16 bytes */
typedef struct cf_bestshot cf_bestshot;
/* A table of n_streams (1..4096) streams on ctx's device: n_streams * E * (3*S*S + 128) bytes of device state.  CF_EINVAL for bad options
 * or a NULL out, before any GPU work (ctx == NULL: the options are still checked first, cf_op_last_error names the cause, as
 * cf_track_create does); CF_ENOMEM, before anything is allocated, when the state does not fit the device's free memory. */
int cf_bestshot_create(cf_ctx* ctx, int n_streams, const cf_bestshot_opts* opts, cf_bestshot** out);
/* Waits for the table's last call, then frees it.  NULL gives CF_OK. */
int cf_bestshot_destroy(cf_bestshot* bs);
/* One offer of the streams stream0 .. stream0 + B - 1: image b of ctx's newest tracked rows is stream stream0 + b; B must be the B of
 * those rows.  chips [cap_faces][S][S][3] uint8 and offsets [B+1] as cf_align_faces / cf_align_faces_frame wrote them (on_device: device
 * addresses, chips 16-byte aligned; otherwise host arrays, which are copied up, and the call blocks).  (h, w) is the frame the chips were
 * cut from: rows in network space, any 2..8192, fx = (double)w / (double)W, fy = (double)h / (double)H (chips of cf_align_faces: pass
 * (H, W)); rows in frame space (after cf_merge_tiles), (h, w) must be the tiled frame's and fx = fy = 1.
 * quality [cap_faces] (Q of the chip of an eligible row, -1 otherwise) and flags [B] may be NULL; out_on_device says where they are.
 * With device chips and device outputs the call is asynchronous on the context's main stream behind the align, and reads nothing on
 * the host.  It changes no state of ctx.
 * CF_ESTATE when the newest rows of ctx are not tracked rows (no cf_track_update / cf_track_follow behind them), or once another
 * forward or upload was started.  CF_EINVAL, before any GPU work, for: a stream range outside the table, B outside 1..max_batch or not
 * the rows' B, cap_faces < 0, bad h / w, device chips not 16-byte aligned, a table on another device, NULL chips / offsets / table
 * (ctx == NULL: the arguments are still checked first, cf_op_last_error names the cause).
 * Ordering: the table keeps one event, used exactly as the tracker uses its own -- every offer or collect first makes its stream wait
 * for the previous call's event, then records a new one -- so a ring of contexts can share one table in call order. */
int cf_bestshot_offer(cf_ctx* ctx, cf_bestshot* bs, int stream0, int B, const void* chips, const int32_t* offsets, int cap_faces,
                      int on_device, int h, int w, int64_t* quality, int32_t* flags, int out_on_device);
/* Collect of the streams stream0 .. stream0 + B - 1 (any range inside the table, cap in 0..E).  Outputs, any may be NULL (entries are freed all
 * the same): chips [B][cap][S][S][3] (16-byte aligned on the device), quality [B][cap], records [B][cap][8], dets [B][cap][5],
 * lms [B][cap][10], counts [B], pending [B], flags [B].  It needs no forward on ctx.  The host form blocks. */
int cf_bestshot_collect(cf_ctx* ctx, cf_bestshot* bs, int stream0, int B, int cap, int flush, void* chips, int64_t* quality,
                        int32_t* records, float* dets, float* lms, int32_t* counts, int32_t* pending, int32_t* flags, int out_on_device);

/* ---- annotation: box outlines, landmark dots and a numeric label IN THE SOURCE FRAME, on the device --------------------------- */
/* What demo.py:15-23, 40-51 does with a detection -- cv2.rectangle(frame, .., (2, 255, 0), 1) per box, cv2.circle(frame, .., 2,
 * (0, 0, 255), -1) per landmark -- for frames that stay on the device: BGR or 4:2:0, pitched, a decoder's surface in place, behind the
 * decode, the merge or the tracker, whose work it makes visible (held tracks in their own colour, dashed, with their id).  The
 * arithmetic is this library's own statement (csrc/cf_drawmath.h, shared by the host and the kernels of csrc/cf_draw.hip; restated in
 * tests/draw_cases.py; device and restatement are equal bit for bit).  Integers throughout, except the point mapping: float64 in the
 * order written, no FMA contraction.
 *   Frame h x w, the rows' coordinate space H x W, fx = (double)w / (double)W, fy = (double)h / (double)H (after a merge H x W is the
 *   frame itself: fx = fy = 1).  Options t = thickness, r = radius, k = label_scale.
 *   1. Points.  P(v, f) = (int)min(max(floor(v * f), -8192.0), 16384.0) for a double v.
 *      Box: cx = ((double)x1 + (double)x2) * 0.5, hw = ((double)x2 - (double)x1) * 0.5 * (double)scale, X1 = P(cx - hw, fx),
 *      X2 = P(cx + hw, fx); y likewise.  A row is skipped entirely when a corner is not finite or hw / hh is not > 0, as in the
 *      redaction.  Both corners are inclusive: the box is [X1..X2] x [Y1..Y2].  There is no snapping to even.
 *      Landmark j: (Lx, Ly) = (P((double)lx, fx), P((double)ly, fy)); skipped when either value is not finite.
 *   2. Primitives of a row, as sets of frame pixels (x, y), clipped to the frame:
 *      Outline (CF_DRAW_BOX): pixels inside the box with x < X1 + t || x > X2 - t || y < Y1 + t || y > Y2 - t.  With t = 1 these are
 *        exactly the pixels cv2.rectangle(.., thickness=1) names for the same integer corners.  A held row (misses > 0) with dash_held
 *        keeps only pixels with ((x + y) % (8 * t)) < 4 * t: x, y >= 0 inside the frame, so the pattern is anchored at the frame origin.
 *      Dot (CF_DRAW_LANDMARKS): pixels with dx*dx + dy*dy <= r*r + r about each of the five (Lx, Ly), live rows only (a held row's
 *        landmarks are the last ones seen and are not drawn).  r = 2 is the 5 x 5 square without its corners, 21 pixels; r = 0 one pixel.
 *      Label (label != NONE).  SCORE: value p = (int)floor((double)score * 100.0) clamped to [0, 100]; no label when score is not
 *        finite.  ID: the row's track id; no label when id <= 0.  Digits: the decimal digits of the value without leading zeros, n of
 *        them (1..10).  Plate: Pw = k * (6n + 1), Ph = 9k, x0 = X1, y0 = Y1 - Ph when that is >= 0, else Y1 + t; the plate is
 *        [x0, x0 + Pw) x [y0, y0 + Ph).  Ink: with u = (x - x0) / k, v = (y - y0) / k, the pixel is ink when 1 <= v <= 7, u >= 1,
 *        q = (u - 1) / 6 < n, col = (u - 1) % 6 < 5 and bit 4 - col of GLYPH[digit q][v - 1] is set.
 *        GLYPH, rows top to bottom, 5 bits each, MSB = left column:
 *          0: 0E 11 13 15 19 11 0E    1: 04 0C 04 04 04 04 0E    2: 0E 11 01 02 04 08 1F    3: 1F 02 04 02 01 11 0E
 *          4: 02 06 0A 12 1F 02 02    5: 1F 10 1E 01 01 11 0E    6: 06 08 10 1E 11 11 0E    7: 1F 01 02 04 08 08 08
 *          8: 0E 11 11 0E 11 11 0E    9: 0E 11 11 0F 01 02 0C
 *   3. Layers.  Each primitive pixel has a layer, and the layer fixes the colour: 1 held_color: outline and plate of held rows;
 *      2 box_color: outline and plate of live rows; 3 text_color: ink; 4 lm_color: dots.  A frame pixel takes the colour of the HIGHEST
 *      layer that any row of its image puts on it and is not written at all when there is none -- so the result depends neither on the
 *      order of the rows nor on their overlap.
 *   4. Planes.  BGR: the three bytes of the pixel.  4:2:0: the luma sample takes byte 0 of the colour; a chroma sample (i, j) takes
 *      bytes 1 and 2 of the colour of the highest layer over its four luma pixels (2i..2i+1, 2j..2j+1) and is untouched when none of
 *      the four is drawn; chroma is in memory order for NV21 / YV12, as cf_redact_faces places `fill`.  No byte that is not drawn is
 *      ever read-modify-written: pitch padding and every undrawn byte keep their values.
 * On the device this is a gather (one launch writes a record per row, one launch of a workgroup per 64 x 16 tile paints): every byte
 * has one writer, the frame is never read. */
#define CF_DRAW_BOX        1     /* `what` bits */
#define CF_DRAW_LANDMARKS  2
#define CF_DRAW_LABEL_NONE  0    /* `label` */
#define CF_DRAW_LABEL_SCORE 1
#define CF_DRAW_LABEL_ID    2
typedef struct cf_draw_opts {
    int32_t what;                /* CF_DRAW_BOX | CF_DRAW_LANDMARKS; what == 0 with label == 0 is CF_EINVAL */
    int32_t thickness;           /* t, 1..16: the outline grows INWARDS from the box */
    int32_t radius;              /* r, 0..16: landmark dot */
    int32_t label;               /* CF_DRAW_LABEL_* */
    int32_t label_scale;         /* k, 1..8: pixels per glyph cell */
    int32_t dash_held;           /* 0 | 1: outlines of held rows (misses > 0) are dashed */
    float   scale;               /* box grown about its centre, 0.25..4 (1 = the detection itself) */
    uint8_t box_color[4], held_color[4], lm_color[4], text_color[4];   /* bytes in the frame's own channel order (B,G,R or Y,U,V), [3] unused -- as cf_redact_opts.fill */
} cf_draw_opts;                  /* 44 bytes */
/* Which rows, B, (h, w), pitches, alignment, on_device, the stream and the CF_ESTATE / CF_EINVAL rules are those of cf_redact_faces:
 * the tracked rows behind a cf_track_update, else the merged rows of a tiled forward, else the decode's, in network coordinates
 * whatever cf_set_rescale says.  misses and id come from the tracked rows' info; untracked rows are all live, and CF_DRAW_LABEL_ID on
 * them is CF_ESTATE.  The call changes no state of ctx, as cf_align_faces_frame promises: a redact, blur, align or second draw behind it
 * behaves as before (draw-after-redact is the expected order).  BGR frames may have odd sides (h, w in 1..8192).  on_device = 1: in
 * place, asynchronous on the stream that carried the rows' producer, no count is read on the host.  CF_EINVAL, before any GPU work,
 * for: `what` outside 0..3 or `label` outside 0..2, nothing to draw, thickness, radius or label_scale out of range, dash_held not
 * 0 / 1, scale out of range or not finite, and every geometry and plane error of the redaction.  A scratch of one record per row
 * grows to the largest B x rows seen (outside any graph). */
int cf_draw_faces(cf_ctx* ctx, const cf_draw_opts* opts, int format, const cf_planes_rw* frames, int on_device, int B, int h, int w,
                  int pitch0, int pitch1);

/* ---- fused convenience: forward + D3 decode in one enqueue (eval_widerface.py:76-90 shape) -- */
int cf_detect_topk(cf_ctx* ctx, const void* in, int in_format, int in_on_device, int B, int K,
                   float* dets, float* lms, int64_t* inds, int out_on_device);

/* ---- multi-GPU: one process (or thread) per GPU, batch sharded by rank, final boxes gathered over RCCL / xGMI -- */
/* The only exchange of the data path (images are independent end to end): an all-gather of the fixed-size
 * detection records.  The reference has no counterpart (train.py:11,17 import torch.distributed without using
 * it).  librccl is loaded on first use.  Rendezvous is the caller's: rank 0 calls cf_comm_unique_id and ships the
 * 128 bytes to the other ranks by any means (file, socket, MPI, torch.distributed store), then every rank calls
 * cf_comm_create (collective: returns when all `world` ranks have joined). */
#define CF_COMM_ID_BYTES 128
typedef struct cf_comm cf_comm;
int cf_comm_unique_id(void* id, int bytes);
/* ONE communicator per rank (= per GPU), whatever the number of contexts on that GPU: it owns the rank's single gather
 * stream, and every all-gather of every context of the rank is enqueued there in call order -- all ranks then see the same
 * collective order as long as they call cf_gather_topk in the same order (concurrent communicators on free-running streams
 * have no such guarantee and may deadlock).  `ctx` only names the device. */
int cf_comm_create(cf_ctx* ctx, int rank, int world, const void* id, cf_comm** out);
/* Single process / single thread that owns one context per GPU: the n ncclCommInitRank calls inside one
 * ncclGroupStart/End (un-grouped, the first call would block forever waiting for the others).  out[i] = rank i = ctxs[i]. */
int cf_comm_create_all(cf_ctx** ctxs, int n, cf_comm** out);
/* Dry run of a `world`-rank gather on ONE GPU, without RCCL: the process plays the ranks in turn.  cf_comm_loopback_rank(comm, r)
 * names the rank whose cf_gather_topk comes next; that call decodes the context's last forward (rank r's shard), writes the slot
 * header and copies the slot into rank r's place of the landing area (the stand-in for the all-gather).  The call of the LAST rank
 * of a step (every rank exactly once, any order) runs the header check + unpack and fills `records` [world * B, K, 16]; the calls
 * before it write nothing.  Everything else -- slot sizes, shard agreement, header protocol, step numbers, the rank-major unpack
 * arithmetic, the mismatch latch -- is the code of the real gather: a deployment checks its shard math for 2 / 4 / 8 ranks on one
 * GPU (tests/test_multigpu.py asserts the 8-rank result equals the unsharded order bit for bit). */
int cf_comm_create_loopback(cf_ctx* ctx, int world, cf_comm** out);
int cf_comm_loopback_rank(cf_comm* comm, int rank);
int cf_comm_destroy(cf_comm* comm);
/* Give up on a communicator whose collective does not complete (ncclCommAbort: in-flight RCCL kernels exit), then release
 * it.  cf_comm_query: 0 = everything enqueued on the gather stream (shard agreement, gathers) has completed, 1 = still
 * running, CF_EINVAL = the agreement or a slot header found unequal (B, K) or unequal step numbers on the ranks (latched;
 * text from cf_comm_last_error).  Never blocks -- a host polls it against its own deadline and aborts instead of hanging.
 * cf_comm_synchronize waits by polling cf_comm_query, so the latch ends the wait too. */
int cf_comm_abort(cf_comm* comm);
int cf_comm_query(cf_comm* comm);
int cf_comm_synchronize(cf_comm* comm);
const char* cf_comm_last_error(cf_comm* comm);
/* Declare the largest shard every rank gathers: B images x K records (= the fixed slot size of every later gather).  Collective by
 * contract: every rank calls it with the same values at the same point of its call sequence (the first cf_gather_topk of a
 * communicator calls it implicitly; call it again on every rank to change the geometry).  It enqueues the ONLY extra
 * collective of the gather path -- a 2-int all-gather of each rank's (B, K) plus a device-side compare that latches a
 * mismatch -- and returns without waiting; poll cf_comm_query (0 = agreed, CF_EINVAL = unequal shards) against a deadline.
 * The first gather of the geometry reads that verdict (waiting for it if the host has not) BEFORE it enqueues a record
 * gather, so an all-gather with per-rank-unequal counts is never launched. */
int cf_comm_set_shard(cf_comm* comm, int B, int K);
/* Test hooks.  what = 0: park the gather stream behind a spin kernel of `value` ms (a collective that does not complete in
 * time); what = 1: the header of the next gather's slot carries B + value (the mismatch path on a single rank). */
int cf_comm_debug(cf_comm* comm, int what, int value);
void* cf_comm_stream(cf_comm* comm);                    /* the gather stream (hipStream_t) */
/* D3 decode of the last forward (as cf_decode_topk) followed by the all-gather: records [world * B, K, 16] =
 * x1,y1,x2,y2,score,cls,lm0..lm9 per detection, rank-major = exactly the batch order of the unsharded run.  Every rank
 * must pass the same B and K.  ONE collective per call: each rank sends a fixed-size slot = a 64-byte header {magic, B, K,
 * step number} + its B x K x 16 records; behind the all-gather a device kernel checks every rank's header against THIS
 * rank's (B, K) and step count and strips the headers into `records`.  The slot agreed by cf_comm_set_shard is a CAPACITY:
 * any (B, K) with B x K no larger than the agreed product -- the ragged last batch of a run, a smaller K -- is gathered in
 * the same slot without another agreement, as long as it is the same on every rank.  A rank whose shard does not fit
 * still sends a full-size slot (carrying its real B, K) and returns CF_EINVAL; a rank whose (B, K) differs from the
 * others' is found by every rank's header check: the counts and the collective sequence stay identical on all ranks,
 * every rank latches the mismatch, nobody hangs.  A latched mismatch
 * is reported by the blocking form itself, and by cf_comm_query / cf_comm_synchronize / the next cf_gather_topk for the
 * asynchronous form.  The decode runs on the context's decode stream, the all-gather on the communicator's stream behind
 * it, both underneath the next forward.  out_on_device = 1: `records` is a device buffer, the call never waits on the host
 * once the shard is agreed (cf_comm_query / cf_comm_synchronize before reading it); 0: host buffer, blocking. */
int cf_gather_topk(cf_ctx* ctx, cf_comm* comm, int K, int use_reg, float* records, int out_on_device);

/* ---- stream / timing plumbing -------------------------------------------------------------- */
int cf_synchronize(cf_ctx* ctx);
/* HIP events on the ctx stream (the stream the kernels are launched on). slot in [0, 64). */
int cf_event_record(cf_ctx* ctx, int slot);
int cf_event_elapsed_ms(cf_ctx* ctx, int slot_begin, int slot_end, float* ms);
/* Per-kernel timing of one forward (+ optional top-K decode when K > 0): runs the launches eagerly
 * with an event pair around each, returns up to `cap` records.  Replaces the datetime prints at
 * centerface.py:38,47,49. */
typedef struct cf_op_time {
    char    name[48];            /* e.g. "layer1.0.dw" */
    char    kind[16];            /* stem | pw | dw | head | decode */
    char    kernel[160];         /* demangled kernel symbol, as rocprofv3 --kernel-trace prints it */
    float   ms;
    double  algo_bytes;          /* algorithmic HBM bytes of this launch: unpadded in + out */
    double  flops;               /* 2 * MACs */
} cf_op_time;
int cf_profile_forward(cf_ctx* ctx, const void* in, int in_format, int in_on_device, int B, int K,
                       cf_op_time* out, int cap, int* n_out);
/* The launch plan of a context (model/centernet.py:263-280 as kernels) and a layer-by-layer trace for parity
 * tests: cf_forward_trace runs the forward eagerly up to and including plan entry `op_index` and copies that
 * entry's output to the host as NCHW float32 [B, C, H, W] (the head entry: C = 16 record channels hm_sigmoid,
 * wh0-1, lm0-9, reg0-1, hm_raw).  Entries with fused_away != 0 are not launched (their work happens inside the
 * next entry) and cannot be traced.  Blocking. */
typedef struct cf_op_info {
    char    name[48];            /* e.g. "layer1.0.mbconv" */
    char    kind[16];            /* stem0 | mbconv | expdw | pw | dw | head | stem */
    int32_t C, H, W;             /* output tensor */
    int32_t fused_away;
} cf_op_info;
int cf_plan_size(cf_ctx* ctx, int* n);
int cf_plan_op(cf_ctx* ctx, int i, cf_op_info* out);
int cf_forward_trace(cf_ctx* ctx, const void* in, int in_format, int in_on_device, int B, int op_index, float* out_nchw);
/* The context's HIP streams as opaque hipStream_t values: `main_stream` carries the forward (and the
 * host-output decodes), `decode_stream` the device-output top-K decode.  For callers that chain their own
 * device work (e.g. an RCCL all-gather of the decoded boxes on another stream) with stream/event waits
 * instead of cf_synchronize(). */
int cf_get_streams(cf_ctx* ctx, void** main_stream, void** decode_stream);
/* Two contexts with a batch in flight on each overlap their forwards on the GPU -- unless their MAIN streams were folded
 * onto the same hardware queue (HIP maps a process's streams onto 4 queues; which one a new stream gets depends on every
 * stream the process created before): then the two forwards run strictly one after the other (42 k instead of 46 k img/s
 * at 64 x 640x640).  cf_streams_share_queue tells (a ~0.3 ms spin on a's main stream, an empty kernel on b's, both contexts
 * idle); cf_reroll_streams replaces the context's main and decode streams by new ones (new streams are created BEFORE the
 * old ones are destroyed; the context must be idle; captured graphs stay valid).  Re-rolling helps in a fresh process; where it keeps
 * landing on the same queue, cf_spread_streams (below) is the tool.  What EngineRing calls at construction when its streams clash. */
int cf_streams_share_queue(cf_ctx* a, cf_ctx* b, int* shared);
/* The same probe for any pair of the contexts' streams: which = 0 main, 1 decode, 2 the device's copy stream (a == b allowed).
 * + 16 on either selector: the DISPATCH-PIPE probe -- the first stream runs a kernel whose grid cannot be resident at once (its pipe stays busy
 * launching workgroups), so streams on different queues of one pipe are caught too: such a pair costs a ring of two contexts its overlap
 * just like a shared queue (49-51 k instead of 53-54 k img/s; tools/queue_order_probe.py). */
int cf_streams_share_queue_ex(cf_ctx* a, int which_a, cf_ctx* b, int which_b, int* shared);
/* Put the main streams (and the decode streams of contexts created without CF_FLAG_NO_DECODE_STREAM) of n idle contexts of one device on
 * pairwise different hardware queues: candidates are created and probed one after the other, those that land on a used queue are kept as
 * ballast until the end, so the runtime's fewest-streams-first placement moves on (a create-then-destroy re-roll can come back to the same
 * queue forever in a process with unevenly loaded queues).  Main streams first; at most four queues exist.  window = 0: all pairwise different;
 * window = w > 0: a main stream only differs from those of the w contexts before it in ctxs (more contexts than pipes, used round-robin in
 * that order).  Decode streams may end up sharing with each other, never with a main stream.  *n_distinct (may be NULL) =
 * streams placed on a queue of their own.  Captured graphs stay valid.  Call it only when streams clash as created: the placement the runtime
 * gives the first contexts of a process measured 4 % faster than a fresh one (54.1 against 51.9 k img/s, no queue shared in either). */
int cf_spread_streams(cf_ctx** ctxs, int n, int window, int* n_distinct);
int cf_reroll_streams(cf_ctx* ctx);
/* hipGraph replay state: number of captured forward graphs held by the context, and how many
 * (input, format, batch) keys could not be captured and run as eager launches instead. */
int cf_graph_stats(cf_ctx* ctx, int* n_graphs, int* n_uncapturable);
/* page-locked host memory: a batch staged here is copied by DMA, asynchronously, underneath the previous forward
 * (cf_forward from pageable memory stages through the driver and blocks the caller for the copy) */
int cf_host_alloc(cf_ctx* ctx, uint64_t bytes, void** hptr);
int cf_host_free(cf_ctx* ctx, void* hptr);
/* The same without a context (any device may DMA from it; hipHostMalloc, portable): for a host's frame pool. */
int cf_pinned_alloc(uint64_t bytes, void** hptr);
int cf_pinned_free(void* hptr);
/* Page-lock / release memory the caller owns (no context needed; any device may then DMA from it).  For buffers that are reused:
 * registering costs a page-table walk (~0.1 ms per MB).  Errors: cf_op_last_error().
 * CONTRACT (round 6): `hptr` is page-aligned (4096), `bytes` a multiple of the page size, and the range is a mapping OF ITS OWN
 * (mmap, shm, a device driver's buffer) -- NOT memory from malloc / new / numpy.  Registration works on pages and on the kernel's
 * view of the mapping; the C library grows, trims and reuses its heap (brk) underneath live registrations, and the GPU then faults on
 * a page it was told is locked ("Memory access fault by GPU ... Reason: Unknown", SIGABRT from the HSA runtime's event thread).
 * Measured on MI355X / ROCm 7 (tools/diag/pin_churn_probe.py, 45 s of allocation churn per run): heap memory 6 faults in 22 runs,
 * whole pages inside a heap array 1 in 6, mmap regions 0 in 6, cf_pinned_alloc memory 0 in 6.  An unaligned pointer or size is
 * CF_EINVAL; whose mapping it is cannot be checked here (cfa.pin refuses the [heap] segment).  Prefer cf_pinned_alloc. */
int cf_host_register(void* hptr, uint64_t bytes);
int cf_host_unregister(void* hptr);
/* device memory helpers so a host language without a GPU allocator can keep inputs resident */
int cf_device_alloc(cf_ctx* ctx, uint64_t bytes, void** dptr);
int cf_device_free(cf_ctx* ctx, void* dptr);
int cf_memcpy_h2d(cf_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int cf_memcpy_d2h(cf_ctx* ctx, void* dst, const void* src, uint64_t bytes);

/* ---- per-op entry points (tests; host pointers; NCHW float32 like the torch ops they replace) */
const char* cf_op_last_error(void);      /* text of the last failing cf_op_* call on this thread */
/* Demangled symbol (as rocprofv3 prints it) of the kernel the last cf_op_* call on this thread selected; the layout converters
 * around it set none, so after cf_op_pwconv it names the GEMM instance.  Lets a test assert WHICH variant it checked. */
const char* cf_op_last_kernel(void);
/* ConvReLU depthwise / ShuffleV2 dw: pad -> conv2d(groups=C, bias=False) -> act.
 * x [B,C,H,W], w [C,1,k,k], y [B,C,Ho,Wo]; pad_lo/pad_hi as ZeroPad2d (model/centernet.py:63,68-70;
 * model/blocks.py:28); act: 0 none, 1 swish.  bias may be NULL (folded BN shift, blocks.py:29).
 * C a multiple of 8; k 3 or 5; stride 1 or 2; act 0 or 1; the padded input at least k x k (so Ho, Wo >= 1); one image (H x W x C in the
 * storage type) smaller than 4 GiB (CF_EINVAL otherwise, before any GPU work: y is not written). */
int cf_op_dwconv(int device, int dtype, const float* x, const float* w, const float* bias, float* y,
                 int B, int C, int H, int W, int k, int stride, int pad_lo, int pad_hi, int act);
/* Which kernel instance cf_op_dwconv (and the engine's and the ShuffleV2 block's standalone depthwise) would launch for a shape, and
 * with what: the host half of the launcher only, no device, no launch.  out = {ok, strip (1 dw_strip_kernel, 0 dw_lds_kernel), k,
 * stride, tile rows, tile columns, Cc (channels per chunk), nchunk, cpp (16-byte groups per pixel of a chunk), threads per workgroup,
 * dynamic LDS bytes, ntx, nty (tiles across / down one image), workgroups, Ho, Wo}; tag (may be NULL; tag_len bytes) receives the
 * symbol cf_op_last_kernel reports after that launch.  ok = 0 (all zeros, empty tag, CF_OK) for a shape cf_op_dwconv refuses.
 * CF_EINVAL only for an unknown dtype, B < 1, a null out or tag_len < 1 with a tag. */
int cf_op_dw_pick(int dtype, int B, int C, int H, int W, int k, int stride, int pad_lo, int pad_hi, int act, int has_bias,
                  int out[16], char* tag, int tag_len);
/* 1x1 conv [+bias] [+act] [+residual]: x [B,Cin,H,W], w [Cout,Cin], y [B,Cout,H,W]
 * (model/centernet.py:109-110,117-118,134-137,179-184; blocks.py:22-24,31-33). act 0/1 swish/2 relu */
int cf_op_pwconv(int device, int dtype, const float* x, const float* w, const float* bias,
                 const float* residual, float* y, int B, int Cin, int Cout, int H, int W, int act);
/* The same with the kernel's pixel-block addressing ([m / 32][C / P][m % 32][P], P channels per 16 bytes, buffers padded to whole
 * 32-pixel blocks as the engine's are) switched on per operand: layout bit 0 = x, bit 1 = y, bit 2 = residual.  The caller still
 * passes and receives NCHW float32; the reordering happens on the device around the kernel.  layout = 0 is cf_op_pwconv.
 * Unknown bits, or bit 2 without a residual: CF_EINVAL before any GPU work.  The output is filled with 0xFF bytes before the
 * launch, so an element the kernel does not write comes back as NaN. */
int cf_op_pwconv_ex(int device, int dtype, const float* x, const float* w, const float* bias,
                    const float* residual, float* y, int B, int Cin, int Cout, int H, int W, int act, int layout);
/* MBConvBlock.forward, se=False (model/centernet.py:89-140) as ONE fused kernel: x [B,Cin,H,W],
 * w_exp [hid,Cin], w_dw [hid,1,k,k], w_proj [Cout,hid]; residual when Cin==Cout and stride==1.
 * Returns CF_EINVAL for shapes the fused kernel does not cover (t == 1, Cout > 96, Cin > 96, a hid no serving family's hidden
 * chunk divides -- in bf16 that includes hid = 32 / 96 at Cin >= 56: cf_op_mbconv_pick tells), before any GPU work.  Like cf_op_pwconv_ex,
 * cf_op_mbconv / cf_op_expand_dw / cf_op_dwconv fill the output with 0xFF bytes before the launch: a skipped element is a NaN. */
int cf_op_mbconv(int device, int dtype, const float* x, const float* w_exp, const float* w_dw,
                 const float* w_proj, float* y, int B, int Cin, int hid, int Cout, int H, int W,
                 int k, int stride);
/* Which kernel family and table row cf_op_mbconv / cf_op_expand_dw (and the engine) would pick for a block shape: the geometry
 * function only, no device, no launch.  out = {ok, kind (MbKind: 0 tile, 1 px, 2 expdw px, 4 expdw mx, 5 mx, 6 mx2, 7 f32,
 * 8 expdw f32, 9 sp), HC, nq, JX, NBO, HALF, KG}; ok = 0 (and CF_OK) for a shape the entry point refuses.  CF_EINVAL only for an
 * unknown dtype or a null out. */
int cf_op_mbconv_pick(int dtype, int Cin, int hid, int Cout, int k, int stride, int out[8]);
int cf_op_expand_dw_pick(int dtype, int Cin, int hid, int k, int stride, int out[8]);
/* The first two thirds of MBConvBlock.forward (model/centernet.py:109-114): expand 1x1 + Swish, depthwise
 * k x k (stride, `_get_padding`) + Swish, as ONE kernel (bf16 storage only; the path the engine uses for
 * the blocks whose Cout is too wide to fuse the project conv as well).  y [B,hid,Ho,Wo].
 * Returns CF_EINVAL for shapes / dtypes the kernel does not cover. */
int cf_op_expand_dw(int device, int dtype, const float* x, const float* w_exp, const float* w_dw, float* y,
                    int B, int Cin, int hid, int H, int W, int k, int stride);
/* CtdetLoss.forward on explicit NCHW head maps (hm as logits), same targets as cf_ctdet_loss. */
int cf_op_ctdet_loss(int device, const float* hm_raw, const float* wh, const float* reg, const float* lm,
                     int B, int h, int w, const float* gt_hm, const uint8_t* reg_mask, const int64_t* ind,
                     const float* wh_t, const float* reg_t, const uint8_t* lm_mask, const int64_t* lm_ind,
                     const float* lm_t, int max_objs, const float* weights4, float* out5);
/* Target maps of dataset/dataset.py:160-217 for boxes [B,M,4] / landmarks [B,M,10] given in OUTPUT-MAP
 * coordinates (after the affine of :172-179), counts [B]: Gaussian heat map (utils/image.py:95-141, radius in
 * float64), wh, reg, ind, reg_mask, landmarks, lm_ind, lm_mask -- all [B,M,...] except hm [B,1,h,w]. */
int cf_op_encode_targets(int device, const float* boxes, const float* lms, const int32_t* counts, int B, int h, int w,
                         int max_objs, float* hm, float* wh, float* reg, int64_t* ind, uint8_t* reg_mask,
                         float* landmarks, int64_t* lm_ind, uint8_t* lm_mask);
/* ShuffleV2Block.forward in eval mode (model/blocks.py:4-62) as ONE entry point: x [B, 2*inp, H, W] (stride 1) or
 * [B, inp, H, W] (stride 2) -> y [B, oup, Ho, Wo].  Weights as the reference's state_dict holds them: m_w0
 * [mid, inp] (branch_main.0), m_wdw [mid,1,k,k] (.3), m_w5 [oup-inp, mid] (.5); p_wdw [inp,1,k,k] (branch_proj.0),
 * p_w2 [inp, inp] (.2) for stride 2 (NULL otherwise); every *_bn* is 4 rows [C]: weight, bias, running_mean,
 * running_var (eps 1e-5), folded here.  The channel shuffle (:56-62) and the concat (:50,54) are channel
 * addressing inside the kernels.  inp, mid, oup-inp multiples of 8. */
int cf_op_shufflev2(int device, int dtype, const float* x, float* y, int B, int inp, int oup, int mid, int H, int W,
                    int ksize, int stride, const float* m_w0, const float* m_bn1, const float* m_wdw, const float* m_bn4,
                    const float* m_w5, const float* m_bn6, const float* p_wdw, const float* p_bn1, const float* p_w2,
                    const float* p_bn3);
/* stem: ConvReLU(3,32,3,stride 2) on a normalised float NCHW tensor or a uint8 HWC BGR image
 * (model/centernet.py:224 ; centerface.py:32-37). y [B,32,H/2,W/2] */
int cf_op_stem(int device, int dtype, const void* x, int in_format, const float* w, float* y,
               int B, int H, int W);
/* IDAUp.forward (model/centernet.py:200-204) with raw (unfolded) BN parameters, 5 floats rows:
 * bn_up[4][C] / bn_cv[4][C] = weight, bias, running_mean, running_var. lo [B,C,h,w], skip [B,Cs,2h,2w] */
int cf_op_idaup(int device, int dtype, const float* lo, const float* skip, const float* w_up,
                const float* bn_up, const float* w_cv, const float* bn_cv, float eps, float* y,
                int B, int C, int Cs, int h, int w);
/* the four heads (model/centernet.py:247-261,277-279) on x [B,24,h,w]; weights concatenated in
 * head order hm,wh,lm,reg: w0 [4][24,24,3,3], b0 [4][24], w1 [15,24], b1 [15].
 * out [B,15,h,w] = hm(raw),wh(2),lm(10),reg(2).  collapse != 0 uses the folded 3x3 24->15 conv. */
int cf_op_heads(int device, int dtype, const float* x, const float* w0, const float* b0,
                const float* w1, const float* b1, float* out, int B, int h, int w, int collapse);
/* ctdet_decode (centerface_ext.py:52-82) on explicit maps: heat [B,1,h,w] (already sigmoid'ed),
 * wh [B,2,h,w], reg [B,2,h,w] or NULL, lm [B,10,h,w] or NULL. */
int cf_op_ctdet_decode(int device, const float* heat, const float* wh, const float* reg,
                       const float* lm, int B, int h, int w, int K,
                       float* dets, float* lms, int64_t* inds);
/* CenterFace.decode + nms (centerface.py:73-151) on explicit maps for ONE image size (H,W). */
int cf_op_decode_threshold(int device, const float* hm, const float* wh, const float* lm,
                           int B, int h, int w, int img_h, int img_w, float score_thresh,
                           float nms_thresh, int max_out, float* dets, float* lms, int32_t* counts);
int cf_op_decode_threshold_ex(int device, int mode, const float* hm, const float* wh, const float* reg,
                              const float* lm, int B, int h, int w, int img_h, int img_w, float score_thresh,
                              float nms_thresh, int max_out, float* dets, float* lms, int32_t* counts);
/* ctdet_post_process's coordinate part on explicit detections dets [B,K,dim] (in place, host array) */
int cf_op_ctdet_post_process(int device, float* dets, const float* centers, const float* scales, int B, int K,
                             int dim, int out_w, int out_h);
/* The conversion kernel of cf_forward_yuv alone, on host arrays: dense frames [B][h*3/2][w] (OpenCV's single-buffer layout, what
 * cv2.cvtColor(bgr, COLOR_BGR2YUV_I420) returns) -> bgr [B][H][W][3].  (H, W) == (h, w): the conversion only; otherwise followed
 * by cv2.resize to (H, W).  h, w, W even. */
int cf_op_yuv_to_bgr(int device, int yuv_format, const uint8_t* frames, uint8_t* bgr, int B, int h, int w, int H, int W);
/* The kernel of cf_align_faces alone, on host arrays: imgs uint8 [B,h,w,3] BGR (w >= 2), lms [N,10] landmark rows in image pixels,
 * image after image, counts [B] (>= 0, N = their sum): chips [N] in opts->format, matrices [N,6] float64 (may be NULL). */
int cf_op_align_faces(int device, const uint8_t* imgs, int B, int h, int w, const float* lms, const int32_t* counts,
                      const cf_align_opts* opts, void* chips, double* matrices);
/* The kernel of cf_align_faces_frame alone, on host frames (every plane holds rows x pitch bytes; all of them are copied up, so the
 * padding bytes are on the device beside the pixels; pitches multiples of 4): lms [N,10] float32 landmark rows in FRAME pixels, image
 * after image, counts [B] (>= 0, N = their sum): chips [N] in opts->format, matrices [N,6] float64 (may be NULL).  The same validation
 * as cf_align_faces_frame, before any device is touched. */
int cf_op_align_frame(int device, int format, const cf_yuv_planes* host_frames, int B, int h, int w, int pitch0, int pitch1,
                      const float* lms, const int32_t* counts, const cf_align_opts* opts, void* chips, double* matrices);
/* The kernels of cf_redact_faces alone, on host frames (modified in place): boxes [sum counts][4] x1,y1,x2,y2 in the coordinates of an
 * H x W network input, image after image, counts [B] (>= 0).  The same validation as cf_redact_faces, before any device is touched. */
int cf_op_redact(int device, const cf_redact_opts* opts, int format, const cf_planes_rw* host_frames, int B, int h, int w, int pitch0,
                 int pitch1, const float* boxes, const int32_t* counts, int H, int W);
/* The kernels of cf_blur_faces alone, on host frames (modified in place): boxes, counts, H, W and the validation as cf_op_redact. */
int cf_op_blur(int device, const cf_blur_opts* opts, int format, const cf_planes_rw* host_frames, int B, int h, int w, int pitch0,
               int pitch1, const float* boxes, const int32_t* counts, int H, int W);
/* The tile cutter of cf_forward_tiles alone, on host frames (every plane holds rows x pitch bytes; all of them are copied up, so the
 * padding bytes are on the device beside the pixels): tiles [Bf * T][H][W][3].  W % 4 == 0.  The same validation, before any device is
 * touched. */
int cf_op_cut_tiles(int device, int format, const cf_yuv_planes* host_frames, int Bf, int h, int w, int pitch0, int pitch1,
                    const cf_tile_rect* rects, int T, int H, int W, uint8_t* tiles);
/* The merge of cf_merge_tiles alone, on host tables: dets_net [Bf * T][rows][4], scores [Bf * T][rows], lms_net [Bf * T][rows][10],
 * counts [Bf * T] -> dets [Bf][max_out][5], lms [Bf][max_out][10], out_counts [Bf], flags [Bf].  dets and lms are copied up first, so
 * rows the kernels do not write come back as the caller filled them. */
int cf_op_merge_tiles(int device, const cf_merge_opts* opts, const cf_tile_rect* rects, int T, int Bf, int h, int w, int H, int W,
                      const float* dets_net, const float* scores, const float* lms_net, const int32_t* counts, int rows, int max_out,
                      float* dets, float* lms, int32_t* out_counts, int32_t* flags);
/* The cutter of cf_forward_views alone, on host frames (every plane holds rows x pitch bytes; all of them are copied up, so the padding
 * bytes are on the device beside the pixels): canvases [Bf * V][H][W][3].  W % 4 == 0, Bf * V * H * W * 3 < 2^31.  The same validation,
 * before any device is touched; nothing is written on refusal. */
int cf_op_views(int device, int format, const cf_yuv_planes* host_frames, int Bf, int h, int w, int pitch0, int pitch1,
                const cf_view* views, int V, const uint8_t* fill, int H, int W, uint8_t* canvases);
/* The merge of cf_merge_views alone, on host tables: dets_net [Bf * V][rows][4], scores [Bf * V][rows], lms_net [Bf * V][rows][10],
 * counts [Bf * V] -> dets [Bf][max_out][5], lms [Bf][max_out][10], out_counts [Bf], flags [Bf].  dets and lms are copied up first, so
 * rows the kernels do not write come back as the caller filled them.  The views are checked against the h x w frame and the H x W
 * canvas as cf_forward_views checks them. */
int cf_op_merge_views(int device, const cf_merge_opts* opts, const cf_view* views, int V, int Bf, int h, int w, int H, int W,
                      const float* dets_net, const float* scores, const float* lms_net, const int32_t* counts, int rows, int max_out,
                      float* dets, float* lms, int32_t* out_counts, int32_t* flags);
/* The cutter of cf_forward_packed alone, on host frames (every plane holds rows x pitch bytes; all of them are copied up): canvases
 * [N][H][W][3].  W % 4 == 0, N * H * W * 3 < 2^31.  The same validation, before any device is touched; nothing is written on refusal. */
int cf_op_packed(int device, int format, const cf_yuv_planes* host_frames, int Bf, int h, int w, int pitch0, int pitch1,
                 const cf_place* places, int P, int N, const uint8_t* fill, int H, int W, uint8_t* canvases);
/* The merge of cf_merge_packed alone, on host tables: dets_net [N][rows][4], scores [N][rows], lms_net [N][rows][10], counts [N] ->
 * dets [Bf][max_out][5], lms [Bf][max_out][10], out_counts [Bf], flags [Bf].  dets and lms are copied up first, so rows the kernels do
 * not write come back as the caller filled them.  The placements are checked as cf_forward_packed checks them. */
int cf_op_merge_packed(int device, const cf_merge_opts* opts, const cf_place* places, int P, int N, int Bf, int h, int w, int H, int W,
                       const float* dets_net, const float* scores, const float* lms_net, const int32_t* counts, int rows, int max_out,
                       float* dets, float* lms, int32_t* out_counts, int32_t* flags);
/* The cutter of cf_forward_packed_rot and the merge behind it alone: cf_op_packed and cf_op_merge_packed with the turn `rot` (h x w is
 * the STORED frame, the sources of the placements lie in its upright view, the rows come back in its pixels), the same shapes, limits
 * and copies; the checks of cf_forward_packed_rot before any device is touched; nothing is written on refusal.  rot == 0: those two. */
int cf_op_packed_rot(int device, int rot, int format, const cf_yuv_planes* host_frames, int Bf, int h, int w, int pitch0, int pitch1,
                     const cf_place* places, int P, int N, const uint8_t* fill, int H, int W, uint8_t* canvases);
int cf_op_merge_packed_rot(int device, int rot, const cf_merge_opts* opts, const cf_place* places, int P, int N, int Bf, int h, int w,
                           int H, int W, const float* dets_net, const float* scores, const float* lms_net, const int32_t* counts,
                           int rows, int max_out, float* dets, float* lms, int32_t* out_counts, int32_t* flags);
/* The fit kernel of cf_forward_fit alone, on host frames (every plane holds rows x pitch bytes; all of them are copied up, so the
 * padding bytes are on the device beside the pixels): canvas [B][H][W][3] uint8.  W % 4 == 0, B * H * W * 3 < 2^31.  The same
 * validation, before any device is touched; nothing is written on refusal. */
int cf_op_fit(int device, const cf_fit_opts* opts, int format, const cf_yuv_planes* host_frames, int B, int h, int w, int pitch0,
              int pitch1, int H, int W, uint8_t* canvas);
/* The mapper of cf_unfit_rows alone, on host tables, with the geometry of (opts, h, w, H, W): dets_net [B][rows][4], scores [B][rows],
 * lms_net [B][rows][10], counts [B] -> dets [B][max_out][5], lms [B][max_out][10], out_counts [B], flags [B].  dets and lms are copied
 * up first, so rows the kernel does not write come back as the caller filled them.  No pointer may be NULL; B, rows, max_out >= 1,
 * B * max(rows, max_out) <= 2^24; the option and size checks of cf_fit_geometry, before any device is touched; nothing is written on
 * refusal. */
int cf_op_unfit(int device, const cf_fit_opts* opts, int B, int h, int w, int H, int W, const float* dets_net, const float* scores,
                const float* lms_net, const int32_t* counts, int rows, int max_out, float* dets, float* lms, int32_t* out_counts,
                int32_t* flags);
/* The kernels of cf_forward_rot and of the cf_unfit_rows behind it alone, on host frames and host tables: cf_op_fit and cf_op_unfit with
 * the turn and the stretch of `opts` (h x w is the STORED frame), the same shapes, limits and copies; the checks of cf_forward_rot and
 * cf_rot_geometry before any device is touched; nothing is written on refusal. */
int cf_op_rot(int device, const cf_rot_opts* opts, int format, const cf_yuv_planes* host_frames, int B, int h, int w, int pitch0,
              int pitch1, int H, int W, uint8_t* canvas);
int cf_op_unrot(int device, const cf_rot_opts* opts, int B, int h, int w, int H, int W, const float* dets_net, const float* scores,
                const float* lms_net, const int32_t* counts, int rows, int max_out, float* dets, float* lms, int32_t* out_counts,
                int32_t* flags);
/* The mirror kernel of the flip test alone (cf_set_flip_test), on a host batch: x holds B network inputs of in_format (CF_IN_U8_HWC_BGR:
 * uint8 [B][H][W][3]; CF_IN_F32_NCHW: float32 [B][3][H][W]), out the same with the columns of every image reversed (whole pixels, not
 * bytes).  The kernel runs as the flip forward of a caller's tensor runs it -- one launch that writes the unmirrored and the mirrored
 * half of a 2B batch -- and the mirrored half comes back.  CF_EINVAL, before any device is touched, for a NULL pointer, B < 1, H < 1,
 * W not a positive multiple of 32, an unknown format, or 2^31 bytes and more. */
int cf_op_mirror(int device, int in_format, const void* x, int B, int H, int W, void* out);
/* The merge kernel of the flip test alone, on host records: records_2B [2B][h][w][16] float32 (B unmirrored images, then the B
 * mirrored passes) -> records_out [B][h][w][16] and hm_plane_out [B][h * w], by the statement under cf_set_flip_test.  CF_EINVAL, before
 * any device is touched, for a NULL pointer, B, h or w below 1, or 2^31 bytes and more. */
int cf_op_flip_heads(int device, const float* records_2B, int B, int h, int w, float* records_out, float* hm_plane_out);
/* The update kernel of cf_track_update over a whole sequence, on host tables, with a fresh tracker of n_streams streams: frame f of
 * stream s has the rows i < min(counts_in[f][s], rows) of boxes [F][S][rows][4], scores [F][S][rows], lms_in [F][S][rows][10] ->
 * dets [F][S][max_tracks][5], lms [F][S][max_tracks][10], info [F][S][max_tracks][3], counts [F][S], flags [F][S] after each frame.
 * dets, lms and info are copied up first, so rows the kernel does not write come back as the caller filled them.  No pointer may be
 * NULL; n_frames, rows >= 1, n_frames * n_streams * max(rows, max_tracks) <= 2^24; counts_in >= 0.  The same option checks as
 * cf_track_create, before any device is touched. */
int cf_op_track(int device, const cf_track_opts* opts, int n_streams, int n_frames, int rows, const float* boxes,
                const float* scores, const float* lms_in, const int32_t* counts_in,
                float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* flags);
/* cf_op_track with the tracker of cf_track_create_weak: the same tables, limits and checks, plus the option checks of
 * cf_track_create_weak, before any device is touched.  flags [F][S] carry bit 1 where a weak row matched.  weak == NULL is cf_op_track. */
int cf_op_track_weak(int device, const cf_track_opts* opts, const cf_track_weak_opts* weak, int n_streams, int n_frames, int rows,
                     const float* boxes, const float* scores, const float* lms_in, const int32_t* counts_in,
                     float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* flags);
/* The kernels of cf_track_update and cf_track_follow over a whole sequence, on host tables and host frames, with a fresh tracker of
 * n_streams streams whose row space is space_h x space_w (tiled = 0: network space, fx = w / space_w, fy = h / space_h; tiled = 1:
 * frame space, (space_h, space_w) must be (h, w)).  Frame f of stream s: where detect[f] is not 0 the update with the rows
 * i < min(counts_in[f][s], rows) of boxes [F][S][rows][4], scores [F][S][rows], lms_in [F][S][rows][10] (as cf_op_track) runs first;
 * then the follow on frames[f * S + s] (F * S host frames of h x w in `format`, pitches as cf_redact_faces; only read).  Outputs after
 * each frame: dets [F][S][max_tracks][5], lms [F][S][max_tracks][10], info [F][S][max_tracks][3], counts [F][S], flags [F][S] (0 where
 * no update ran), moves [F][S][max_tracks][4]; rows at and past a count keep the caller's bytes.  All pointers host, none NULL.  The
 * option checks of cf_track_create and cf_track_follow, the geometry and plane checks of cf_redact_faces and the limits of cf_op_track,
 * before any device is touched; nothing is written on refusal. */
int cf_op_follow(int device, const cf_track_opts* opts, const cf_follow_opts* fopts, int n_streams, int n_frames, int rows,
                 const float* boxes, const float* scores, const float* lms_in, const int32_t* counts_in, const uint8_t* detect,
                 int format, const cf_planes_rw* frames, int h, int w, int pitch0, int pitch1, int space_h, int space_w, int tiled,
                 float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* flags, int32_t* moves);
/* cf_op_track_weak with the tracker of cf_track_create_ex ("constant velocity"): the same tables, limits and checks, plus the motion option
 * checks, before any device is touched and after the plain and the weak ones.  weak and motion may each be NULL; motion == NULL is
 * cf_op_track_weak (vel is then left alone).  vel: NULL, or [F][S][max_tracks][2] = vx, vy of the output rows, in output-row order,
 * after every frame; copied up first like dets, so rows at and past the count keep the caller's bytes. */
int cf_op_track_ex(int device, const cf_track_opts* opts, const cf_track_weak_opts* weak, const cf_track_motion_opts* motion,
                   int n_streams, int n_frames, int rows, const float* boxes, const float* scores, const float* lms_in,
                   const int32_t* counts_in, float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* flags, float* vel);
/* cf_op_follow with the tracker of cf_track_create_ex: the update of every detect frame is that tracker's, and a coast moves the follower
 * records' tpl_box along.  The option checks come in the order plain, weak, motion, follow.  weak == NULL and motion == NULL is
 * cf_op_follow. */
int cf_op_follow_ex(int device, const cf_track_opts* opts, const cf_track_weak_opts* weak, const cf_track_motion_opts* motion,
                    const cf_follow_opts* fopts, int n_streams, int n_frames, int rows,
                    const float* boxes, const float* scores, const float* lms_in, const int32_t* counts_in, const uint8_t* detect,
                    int format, const cf_planes_rw* frames, int h, int w, int pitch0, int pitch1, int space_h, int space_w, int tiled,
                    float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* flags, int32_t* moves);
/* The kernels of cf_scene_check over a whole sequence of host frames, with a fresh cf_scene of n_streams streams and no tracker: frame
 * f of stream s is frames[f * S + s] (F * S host frames of h x w in `format`, pitches as cf_redact_faces; only read).  out [F][S][4] =
 * code, hist, grid, run of every check; sigs [F][S][128] (or NULL) = the signature of every frame.  The option and count checks of
 * cf_scene_create, the geometry and plane checks of cf_scene_check, n_frames >= 1 and at most 2^24 frames, before any device is touched;
 * nothing is written on refusal. */
int cf_op_scene(int device, const cf_scene_opts* opts, int n_streams, int n_frames, int format, const cf_planes_rw* frames, int h, int w,
                int pitch0, int pitch1, int32_t* out, int32_t* sigs);
/* The kernel of cf_lookback_step over a whole sequence of host tables, with a fresh cf_lookback of n_streams streams: step f is a push of
 * the streams 0 .. S - 1 when push[f] != 0 -- the rows i < counts_in[f][s] of dets_in [F][S][rows_in][5], lms_in [F][S][rows_in][10],
 * info_in [F][S][rows_in][3] --, else a drain.  cuts [F][S] (or NULL): bit 0 = the scene code of the pushed frame is CF_SCENE_CUT (else
 * CF_SCENE_SAME), bit 1 = a cf_lookback_forget of the stream comes before the step.  After each step: dets [F][S][rows][5], lms
 * [F][S][rows][10], info [F][S][rows][3], counts [F][S], state [F][S][4]; rows at and past a count keep the caller's bytes.  All other
 * pointers host, none NULL.  The option and count checks of cf_lookback_create, n_steps >= 1, 1 <= rows_in <= opts->rows and
 * n_steps * n_streams * rows <= 2^24, before any device is touched; nothing is written on refusal. */
int cf_op_lookback(int device, const cf_lookback_opts* opts, int n_streams, int n_steps, int rows_in, const uint8_t* push,
                   const float* dets_in, const float* lms_in, const int32_t* info_in, const int32_t* counts_in, const int32_t* cuts,
                   float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* state);
/* cf_op_lookback with a fresh cf_lookback that is enabled for tracing (cf_lookback_trace_enable with fopts, h, w): every step has a frame,
 * frames[f * S + s] (F * S host frames of h x w in `format`, pitches as cf_redact_faces; only read; the frame of a drain is ignored),
 * and the rows are in the space space_h x space_w (tiled = 0: network space, fx = w / space_w, fy = h / space_h; tiled = 1: frame space,
 * (space_h, space_w) must be (h, w)), as for cf_op_follow.  Adds moves [F][S][rows][4]; rows at and past a count keep the caller's bytes.
 * The checks of cf_op_lookback, cf_lookback_trace_enable and cf_op_follow's frame table, before any device is touched; nothing is
 * written on refusal. */
int cf_op_lookback_trace(int device, const cf_lookback_opts* opts, const cf_follow_opts* fopts, int n_streams, int n_steps, int rows_in,
                         const uint8_t* push, const float* dets_in, const float* lms_in, const int32_t* info_in, const int32_t* counts_in,
                         const int32_t* cuts, int format, const cf_planes_rw* frames, int h, int w, int pitch0, int pitch1, int space_h,
                         int space_w, int tiled, float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* state, int32_t* moves);
/* The scoring kernel of cf_bestshot_offer alone, on host tables: chips [n][S][S][3] uint8, boxes [n][4], scores [n], lms [n][10]
 * (n in 1..65536; every row counts and is eligible) -> quality [n] int64, parts [n][4] int32 = sharp, size_w, pose_w, score_w.  fx, fy
 * finite and > 0.  Every bad argument is CF_EINVAL with a cf_op_last_error that names it, before any device is touched. */
int cf_op_chip_quality(int device, const cf_bestshot_opts* opts, const uint8_t* chips, const float* boxes, const float* scores,
                       const float* lms, int n, double fx, double fy, int64_t* quality, int32_t* parts);
/* The kernels of cf_bestshot_offer and cf_bestshot_collect over a whole scripted sequence on host tables, with a fresh table of n_streams
 * streams and no engine and no tracker.  Frame f of stream s is offered the rows i < min(counts[f][s], rows) of boxes [F][S][rows][4],
 * scores [F][S][rows], lms [F][S][rows][10], info [F][S][rows][3] = id, hits, misses; the leading min(chip_counts[f][s], rows) rows
 * have a chip (as max_per_image truncates), chips [F][S][rows][Sz][Sz][3].  collect [F] uint8: 0 none, 1 collect, 2 collect with flush,
 * of all streams with `cap` (0..entries), after that frame's offer.  Outputs per frame: out_chips [F][S][cap][Sz][Sz][3], out_quality
 * [F][S][cap], out_records [F][S][cap][8], out_dets [F][S][cap][5], out_lms [F][S][cap][10] (rows at and past a count keep the caller's
 * bytes), out_counts, out_pending, out_flags [F][S] (zero on frames without a collect), offer_flags [F][S], offer_quality [F][S][rows]
 * (-1 for a row without a chip).  All pointers host, none NULL.  rows in 1..1024, n_frames >= 1, counts and chip_counts >= 0, fx, fy
 * finite and > 0, and the option checks of cf_bestshot_create; every bad argument is CF_EINVAL with a cf_op_last_error that names it,
 * before any device is touched; nothing is written on refusal. */
int cf_op_bestshot(int device, const cf_bestshot_opts* opts, int n_streams, int n_frames, int rows, const float* boxes,
                   const float* scores, const float* lms, const int32_t* info, const int32_t* counts, const int32_t* chip_counts,
                   const uint8_t* chips, const uint8_t* collect, int cap, double fx, double fy, uint8_t* out_chips,
                   int64_t* out_quality, int32_t* out_records, float* out_dets, float* out_lms, int32_t* out_counts,
                   int32_t* out_pending, int32_t* out_flags, int32_t* offer_flags, int64_t* offer_quality);
/* The kernels of cf_draw_faces alone, on host frames (modified in place): boxes [N][4] x1,y1,x2,y2 in the coordinates of an H x W
 * network input, scores [N], lms [N][10] or NULL, info [N][3] = id, hits, misses or NULL (all live), image after image, counts [B]
 * (>= 0, N = their sum).  The same validation as cf_draw_faces, before any device is touched; NULL lms with CF_DRAW_LANDMARKS and
 * NULL info with CF_DRAW_LABEL_ID are CF_EINVAL. */
int cf_op_draw(int device, const cf_draw_opts* opts, int format, const cf_planes_rw* host_frames, int B, int h, int w, int pitch0,
               int pitch1, const float* boxes, const float* scores, const float* lms, const int32_t* info, const int32_t* counts,
               int H, int W);
/* HOST ONLY: the integer geometry of one row in an h x w frame, computed by the code the kernels run (csrc/cf_drawmath.h), so that
 * the shared statement can be checked with no GPU.  lms [10] and info [3] may be NULL.  out[32]:
 *   [0] ok (0 = the row is skipped; every other value is then 0)   [1..4] X1, Y1, X2, Y2   [5] held (misses > 0)
 *   [6..9] plate x0, y0, Pw, Ph (0 without a label)   [10] n, the digits of the label (0 = none)   [11..20] the digits, most
 *   significant first, 0 past n   [21] bit j set: landmark j is finite   [22..31] Lx0, Ly0 .. Lx4, Ly4 (0 where not finite).
 * Returns CF_EINVAL for options cf_draw_faces refuses, NULL opts / box / out, or h, w, H, W outside 1..8192 (H, W: below 1). */
int cf_draw_layout(const cf_draw_opts* opts, const float* box, float score, const float* lms, const int32_t* info, int h, int w,
                   int H, int W, int32_t* out);
/* CenterFace.nms alone (centerface.py:111-151): keep[] receives kept indices in keep order. */
int cf_op_nms(int device, const float* boxes, const float* scores, int n, float nms_thresh,
              int32_t* keep, int32_t* n_keep);
/* bbox_overlap (eval_widerface.py:48-74: the "+1" IoU of every detection against every annotation, float32 arithmetic as numpy
 * computes it for float32 inputs) and the two counts evaluate (:195-206) takes from it, for n_img images in one call: rows of
 * box_stride / query_stride floats (x1,y1,x2,y2 first), concatenated; box_off / query_off [n_img + 1] = first row of each image.
 * overlaps (optional): the dense [N_i][K_i] float64 matrices back to back.  counts (optional) [n_img][2]: detections whose best
 * overlap exceeds thresh (evaluate's "detected_num"), annotations whose best overlap does ("true_positives"). */
int cf_op_box_match(int device, int n_img, const float* boxes, int box_stride, const int32_t* box_off, const float* query,
                    int query_stride, const int32_t* query_off, float thresh, double* overlaps, int32_t* counts);

#ifdef __cplusplus
}
#endif
#endif /* CENTERFACE_HIP_H */
