// Host-callable launchers for the gfx950 kernels + weight packers.  dtype: 0 = fp32, 1 = bf16, 2 = fp32 storage with split-bf16
// GEMM products (sp32_t, cf_common.h): storage, layouts and sizes of 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include "centerface_hip.h"
#include "cf_frame.h"

struct sp32_t;

namespace cf {

// Demangled symbol of the kernel the last launch_* call on this thread selected, in the form
// rocprofv3 prints it -- lets cf_profile_forward attribute times to kernel symbols.
const char* last_kernel_tag();
void set_kernel_tag(const char* fmt, ...);
template <typename T> inline const char* type_tag() { return sizeof(T) == 4 ? "float" : "unsigned short"; }
template <> inline const char* type_tag<sp32_t>() { return "sp32_t"; }

inline size_t elem_size(int dtype) { return dtype == 1 ? 2 : 4; }
inline int per16(int dtype) { return dtype == 1 ? 8 : 4; }

// ------------------------------------------------------------------ pointwise (1x1) conv, MFMA
// y[m][n] = act( sum_k x[m][k] * w[n][k] + bias[n] ) (+ residual[m][n]) (+ IDAUp up-branch)
struct PwParams {
    const void* x;        // [M][K]  T
    const void* wp;       // packed weights, see pw_pack_weights
    const float* bias;    // [N] fp32 or nullptr
    const void* res;      // [M][N] T residual (added after act) or nullptr
    void* y;              // [M][N] T
    long long M;
    int K, N;
    int act;              // 0 none, 1 swish, 2 relu
    // IDAUp fusion (model/centernet.py:200-204): y += relu(low[b][y/2][x/2][n] * upw[tap][n] + upb[n])
    const void* low;      // [B][Ho/2][Wo/2][N] T or nullptr
    const float* upw;     // [4][N]  deconv tap * BN scale
    const float* upb;     // [N]     BN shift
    int Ho, Wo;           // spatial dims of y per image (IDAUp fusion; the map size also picks pw_ksplit_kernel, cf_pw.hip)
    // channel-addressed output (ShuffleV2 concat, model/blocks.py:47-54): y rows have ldy elements and this conv
    // writes channels [yoff, yoff + N) of them; ldy = 0 means a dense [M][N] output.  Plain pw_kernel only.
    int ldy, yoff;
    // x in PIXEL-BLOCK order (bf16 only): [m / 32][K / 8][m % 32][8 channels], what expdw_px_kernel writes with
    // MbParams::yblock -- the 32 lanes of a wave half then read one contiguous 512-byte run per k-step instead of 32 rows
    int xblock;
    int yblock;           // y written in pixel-block order [m / 32][N / 8][m % 32][8] (bf16; dense output only)
    int resblock;         // res read in pixel-block order
};
// out[m][c] = x[m][2 c + phase], c < C: the pass-through half of channel_shuffle (model/blocks.py:56-62) written
// straight into its slice of the block output (rows of ldy elements, channel offset yoff)
hipError_t launch_shuffle_copy(hipStream_t s, int dtype, const void* x, void* y, long long M, int C, int phase, int ldy, int yoff);
size_t pw_packed_bytes(int dtype, int K, int N);
void pw_pack_weights(int dtype, const float* w /*[N][K]*/, int K, int N, void* out_host);
hipError_t launch_pw(hipStream_t s, int dtype, const PwParams& p);

// ------------------------------------------------------------------ depthwise k x k conv
struct DwParams {
    const void* x;        // [B][H][W][C] T
    const float* w;       // [k][k][C] fp32 (tap-major, channel contiguous)
    const float* bias;    // [C] fp32 or nullptr
    void* y;              // [B][Ho][Wo][C] T
    int B, C, H, W, Ho, Wo;
    int k, s, pad_lo;     // pad_hi is implied by Ho/Wo
    int act;              // 0 none, 1 swish
};
void dw_pack_weights(const float* w /*[C][1][k][k]*/, int C, int k, float* out_host /*[k][k][C]*/);
hipError_t launch_dw(hipStream_t s, int dtype, const DwParams& p);
// What launch_dw does for p, from the host alone (no device, no launch; of p it reads the sizes, k, s, pad_lo, act and WHETHER bias is set): the
// instance (strip = dw_strip_kernel, else dw_lds_kernel; its k, s and tile), its symbol as cf_op_last_kernel reports it after the launch, the channel
// chunk, the chunks per image, the 16-byte groups per pixel of a chunk, threads per workgroup, dynamic LDS bytes, the tile grid and the number of
// workgroups.  hipErrorInvalidValue where launch_dw refuses.  launch_dw launches exactly this (one function computes both: dw_plan, cf_dw.hip).
struct DwChoice {
    char tag[160];
    int strip, k, s, th, tw;
    int Cc, nchunk, cpp, threads, ntx, nty;
    long long nwg;
    size_t lds_bytes;
};
hipError_t dw_choose(int dtype, const DwParams& p, DwChoice& c);

// ------------------------------------------------------------------ fused MBConv block
// The kernel families.  The values are kernel arguments (MbParams::kind) and appear in tool output: they never change (3 is unused).
// A family = one row of kMbFamilies (cf_mbconv.hip: how it packs and launches) + its place in mb_geometry / expdw_geometry (when it is
// chosen) + an answer to each predicate below.
enum MbKind : int {
    MB_TILE = 0,          // cf_mbconv.hip: E tile in LDS as bf16 / fp32, every dtype
    MB_PX = 1,            // cf_mbconv2.hip: fp16 pixel-pair tile, bf16 storage only
    XD_PX = 2,            // cf_mbconv2.hip: expand + depthwise only (project stays a GEMM launch), bf16
    XD_MX = 4,            // cf_mbconv3.hip: expand + depthwise on the matrix cores, stride 1, bf16
    MB_MX = 5,            // cf_mbconv3.hip: fully fused block, matrix-core depthwise, stride 1, bf16
    MB_MX2 = 6,           // cf_mbconv3.hip: the same for the stride-2 blocks
    MB_F32 = 7,           // cf_mbconv4.hip: the fp32-storage modes' fused block, second generation
    XD_F32 = 8,           // cf_mbconv5.hip: expand + depthwise for the fp32-storage modes
    MB_SP = 9,            // cf_mbconv6.hip: the split mode's fused block for Cout <= 32
    MB_SP_DIRECT = 10,    // experiments/cf_mbconv7.hip (experiments build only)
};
// can the family write its block output in pixel-block order (MbParams::yblock)?  The bf16 fused kernels, and cf_mbconv.hip's fp32-tile
// kernel (layer3.1 in the split mode)
inline bool mb_writes_blocked(MbKind kind, int dtype) {
    return kind == MB_PX || kind == MB_MX || kind == MB_MX2 || (kind == MB_TILE && dtype != 1);
}
struct MbGeom {
    bool ok;              // false: this block shape is not supported by the fused kernel
    int HC, nq;           // hidden-channel chunk and number of chunks (hid = HC * nq)
    int NBE, JX, HALF, NBO, rowb;
    size_t lds_bytes, wexp_bytes, wdw_floats, wproj_bytes;
    MbKind kind; int S;   // kind: the kernel family that serves the block (MbKind above)
    int KG;               // k-groups of the project loop (fp32 / split kernels: the wave groups that split a hidden chunk's k-steps);
                          // the split mode packs the project fragments in pairs per k-group (split_pairs_inplace)
};
MbGeom mb_geometry(int dtype, int Cin, int hid, int Cout, int k, int s);
void mb_pack_weights(int dtype, const MbGeom& g, int Cin, int hid, int Cout, int k,
                     const float* we /*[hid][Cin]*/, const float* wd /*[hid][k*k]*/, const float* wp /*[Cout][hid]*/,
                     void* wexp_host, float* wdw_host, void* wproj_host);
struct MbParams {
    const void* x;        // [B][Hin][Win][Cin] T
    void* y;              // [B][Hout][Wout][Cout] T
    const void* wexp; const float* wdw; const void* wproj;
    int B, Hin, Win, Hout, Wout, Cin, hid, Cout;
    int k, s, pad_lo, residual;
    int HC, nq, NBE, JX, HALF, rowb;
    size_t lds_bytes;
    int nw;               // mbconv_px_kernel: 1 = XCD-aware tile order (set by the launcher)
    MbKind kind;          // MbGeom::kind
    int yblock;           // y (expdw: the depthwise tensor; mbconv_px: the block output) in pixel-block order
                          // [m / 32][C / 8][m % 32][8], m = linear pixel index over the batch (PwParams::xblock)
    int xblock;           // expdw_px_kernel: x in pixel-block order
    void* dbg;            // -DCF_X5_TIMING builds only: per-wave phase cycle sums (tools/x5_timing.py); nullptr otherwise
};
hipError_t launch_mbconv(hipStream_t s, int dtype, const MbParams& p);
// the MbParams fields that come from the geometry
inline void mb_fill(MbParams& p, const MbGeom& g) {
    p.HC = g.HC; p.nq = g.nq; p.NBE = g.NBE; p.JX = g.JX; p.HALF = g.HALF; p.rowb = g.rowb; p.lds_bytes = g.lds_bytes; p.kind = g.kind;
}
// expand + depthwise only (XD_PX [2], XD_MX [4], XD_F32 [8]): y = depthwise output [B][Hout][Wout][hid]; packs with mb_pack_weights(wproj = nullptr)
MbGeom expdw_geometry(int dtype, int Cin, int hid, int k, int s);
// What one family's translation unit calls of another's (everything else of a family is reached through kMbFamilies and mb_geometry,
// cf_mbconv.hip, and declared there):
// cf_mbconv3.hip: depthwise on the matrix cores (v_mfma_f32_4x4x4_16b_f16, Toeplitz operands), stride 1, bf16 storage.
// XD_MX [4] = expand + depthwise (project stays a GEMM launch)
MbGeom expdw_mx_geometry(int dtype, int Cin, int hid, int k, int s);
// cf_mbconv5.hip: expand + depthwise for the fp32-storage modes (XD_F32 [8], split-bf16 tolerance mode): register-window
// depthwise on an x-quad-cell tile, packed taps; y = depthwise output in NHWC or pixel-block order; MbGeom::HALF = hidden chunks
// per workgroup.  Expand fragments as cf_mbconv.hip, taps [chunk][group of 4 channels][tap][4] (mb_pack_weights)
MbGeom expdw_f32_geometry(int dtype, int Cin, int hid, int k, int s);
// cf_mbconv6.hip: the split mode's fused block for Cout <= 32 (MB_SP [9]): cf_mbconv5.hip's register-window depthwise + project
// MFMAs from an LDS tile of the depthwise output (experiments/cf_mbconv7.hip packs its expand fragments and taps with it)
void mb6_pack(int dtype, const MbGeom& g, int Cin, int hid, int Cout, int k, const float* we, const float* wd, const float* wp,
              void* wexp_host, float* wdw_host, void* wproj_host);

// ------------------------------------------------------------------ stem 3x3 s2 3->32 + Swish
struct StemParams {
    const void* x;        // u8 [B][H][W][3] (BGR) or f32 [B][3][H][W]
    int in_format;        // CF_IN_U8_HWC_BGR / CF_IN_F32_NCHW
    const void* w;        // packed MFMA fragments, see stem_pack_weights
    void* y;              // [B][H/2][W/2][32] T
    int B, H, W;
};
size_t stem_packed_bytes(int dtype);
void stem_pack_weights(int dtype, const float* w /*[32][3][3][3]*/, void* out_host);
hipError_t launch_stem(hipStream_t s, int dtype, const StemParams& p);

// ------------------------------------------------------------------ fused stem + layer0 (dw 3x3 + project 32->16)
struct Stem0Params {
    const void* x;        // u8 [B][H][W][3] (BGR) or f32 [B][3][H][W]
    int in_format;
    const float* lut;     // [3][256] normalisation table (u8 input only)
    const void* wstem;    // stem_pack_weights
    const float* wdw;     // [9][32] fp32
    const void* wproj;    // stem0_pack_proj
    void* y;              // [B][H/2][W/2][16] T
    int B, H, W;
    int kind;             // 0: stem0_kernel; else a set of the bits below
};
// bits of Stem0Params::kind (kernel argument: the values never change)
enum : int {
    STEM0_PX = 1,         // stem0_px_kernel (bf16 storage; weights from stem0px_pack)
    STEM0_XCD = 2,        // XCD-aware tile order
    STEM0_MX = 4,         // depthwise on the matrix cores (weights from stem0mx_pack)
};
size_t stem0px_wstem_bytes();
size_t stem0px_wdw_dwords();
void stem0px_pack(const float* ws /*[32][3][3][3]*/, const float* wd /*[32][9]*/, const float* wp /*[16][32]*/,
                  void* wstem_out, uint32_t* wdw_out, void* wproj_out);
size_t stem0mx_wdw_dwords();
void stem0mx_pack(const float* ws, const float* wd, const float* wp, void* wstem_out, uint32_t* wdw_out, void* wproj_out);     // STEM0_MX
void stem0_lut(float* lut /*[3][256]*/);
size_t stem0_proj_bytes(int dtype);
void stem0_pack_proj(int dtype, const float* wp /*[16][32]*/, void* out_host);
hipError_t launch_stem0(hipStream_t s, int dtype, const Stem0Params& p);

// ------------------------------------------------------------------ heads: 3x3 conv (MFMA) + 1x1
struct HeadParams {
    const void* x;        // [B][h][w][24] T
    const void* w0p;      // packed 3x3 weights (96 or 16 output slots), see head_pack_weights
    const float* b0;      // [96] (two-stage) or [16] (collapsed)
    const float* w1d;     // [96][16] dense second-stage table (two-stage only)
    const float* b1;      // [16]
    float* heads;         // [B][h][w][16] fp32: hm_sigmoid, wh0, wh1, lm0..9, reg0, reg1, hm_raw
    float* hm_plane;      // optional dense [B][h][w] copy of hm_sigmoid for the peak test (coalesced reads)
    int B, h, w;
    int collapsed;
};
size_t head_packed_bytes(int dtype, int collapsed);
// w0 [4][24][24][3][3], b0 [4][24], w1 [15][24] (rows: hm, wh0, wh1, lm0..9, reg0, reg1), b1 [15]
void head_pack_weights(int dtype, int collapsed, const float* w0, const float* b0, const float* w1,
                       const float* b1, void* w0p_host, float* b0_host /*[96]|[16]*/,
                       float* w1d_host /*[96][16]*/, float* b1_host /*[16]*/);
hipError_t launch_heads(hipStream_t s, int dtype, const HeadParams& p);

// ------------------------------------------------------------------ detection loss + target encoder (cf_loss.hip)
struct LossParams {
    const float* heads;   // [B][h][w][16] head records of a forward (used when the explicit maps are null)
    const float* hm_raw;  // explicit NCHW maps (op-level entry): hm logits [B,1,h,w], wh [B,2,h,w], reg [B,2,h,w], lm [B,10,h,w]
    const float* wh; const float* reg; const float* lm;
    const float* gt_hm;   // [B][h][w]
    const unsigned char* reg_mask; const long long* ind; const float* wh_t; const float* reg_t;   // [B][M](,2)
    const unsigned char* lm_mask; const long long* lm_ind; const float* lm_t;                     // [B][M](,10)
    int B, h, w, M;
    float hm_w, wh_w, off_w, lm_w;
};
hipError_t launch_ctdet_loss(hipStream_t s, const LossParams& p, double* ws /*[3 * nblocks + 6]*/, int nblocks, float* out_dev /*[5]*/);
struct EncodeParams {
    const float* boxes;   // [B][M][4] x1,y1,x2,y2 in output-map coordinates
    const float* lms;     // [B][M][10], lms[.][0] < 0: no landmarks
    const int* counts;    // [B] objects per image (<= M)
    float* hm; float* wh; float* reg; long long* ind; unsigned char* reg_mask;
    float* landmarks; long long* lm_ind; unsigned char* lm_mask;
    int B, h, w, M;
};
hipError_t launch_encode_targets(hipStream_t s, const EncodeParams& p);

// ------------------------------------------------------------------ IDAUp stage 3 + heads fused (bf16, collapsed heads)
struct UpHeadParams {
    const void* skip;     // [B][h][w][24] T: the IDAUp skip input (layer1 output)
    const void* low;      // [B][h/2][w/2][24] T: previous IDAUp stage
    const void* wcv;      // pw_pack_weights(24 -> 24, BN folded)
    const float* bias;    // [24] BN shift of the 1x1 conv
    const float* upw;     // [4][24] deconv tap * BN scale
    const float* upb;     // [24]
    const void* w0p;      // head_pack_weights(collapsed)
    const float* b0;      // [16]
    float* heads;         // [B][h][w][16] fp32
    float* hm_plane;      // [B][h][w] or nullptr
    int B, h, w;
    int xcd;              // 1 = XCD-aware tile order (set by the launcher)
};
hipError_t launch_uphead(hipStream_t s, int dtype, const UpHeadParams& p);

// conv_last + up1 + up2 as one kernel (cf_neck.hip, bf16): the 1/32 and 1/16 neck maps exist only in LDS
struct NeckParams {
    const void* x;        // layer6 output [B][h][w][320] bf16 (rows, or pixel-block order with x_blk)
    const void* skip1;    // layer4 output [B][2h][2w][96]
    const void* skip2;    // layer2 output [B][4h][4w][32]
    int x_blk, skip1_blk, skip2_blk;
    const void* w0; const float* b0;                                      // conv_last: pw_pack_weights(320 -> 24, BN folded), shift
    const void* w1; const float* b1; const float* upw1; const float* upb1; // up1: conv (96 -> 24), [4][24] tap * scale, [24] shift
    const void* w2; const float* b2; const float* upw2; const float* upb2; // up2: conv (32 -> 24)
    void* y;              // up2 output [B][4h][4w][24] bf16 rows
    int B, h, w;          // h, w: the 1/32 map
};
hipError_t launch_neck(hipStream_t s, int dtype, const NeckParams& p);

// ------------------------------------------------------------------ decode
// D3: 3x3 peak test + top-K (radix select + bitonic sort) + gather: a multi-workgroup collect kernel + one select
// workgroup per image (cf_decode.hip).
struct TopkParams {
    const float* heads;   // [B][h*w][16]
    const float* hm_plane; // optional dense [B][h*w] heat map (else channel 0 of the records is used)
    unsigned long long* scratch;   // [B][h*w] composite keys of the cells whose kept score is not +0 (the peak list)
    int* count;           // [B * kTopkCountStride] list lengths, one per 128-byte line: zero before the launch, zero again after it
    unsigned long long* big;       // K > 1024 only: [B][big_stride] sort buffer + final order (topk_big_stride(K))
    size_t big_stride;
    int B, h, w, K, use_reg;
    float* dets;          // [B][K][6] or nullptr
    float* lms;           // [B][K][10] or nullptr
    long long* inds;      // [B][K] or nullptr
    float* rec16;         // [B][K][16] or nullptr: x1,y1,x2,y2,score,cls,lm0..9 -- the record the multi-GPU gather ships
    const double* trans;  // optional [B][6]: row-major 2x3 affine (heat-map -> source image) applied to both box corners
};
constexpr int kTopkCountStride = 32;   // ints between two images' list counters (each on its own cache line)
size_t topk_big_stride(int K);
hipError_t launch_peak_topk(hipStream_t s, const TopkParams& p);

// D1: threshold compaction (row-major) + box/landmark arithmetic + greedy NMS
struct ThreshParams {
    const float* heads;   // [B][h*w][16]
    const float* hm_plane; // optional dense [B][h*w] copy of channel 0 (coalesced threshold scan), else nullptr
    int B, h, w, img_h, img_w;
    float score_thresh, nms_thresh;
    int cap;              // candidate capacity per image
    int mode;             // 0 = D1 CenterFace.decode (centerface.py:73-109), 1 = D2 eval_widerface.decode (:92-110)
    // workspace (device)
    float* cand;          // [B][cap][16]: x1,y1,x2,y2,score, lm[10], pad
    int* cand_count;      // [B]
    int* order;           // [B][cap] candidate indices sorted by score desc
    unsigned long long* mask;   // [B][cap][cap/64]
    // outputs (device)
    int max_out;
    float* dets;          // [B][max_out][5]
    float* lms;           // [B][max_out][10] or nullptr
    float* lms_net;       // optional [B][max_out][10]: the same rows in network coordinates whatever rs_h / rs_w say (cf_align_faces reads them)
    float* dets_net;      // optional [B][max_out][4]: the box corners likewise, before the rescale (cf_redact_faces reads them)
    int* counts;          // [B]
    int* overflow;        // [1] largest candidate count seen when some image exceeded cap (else untouched)
    float rs_h, rs_w;     // > 0: emit floor(y / rs_h), floor(x / rs_w) (centerface.py:55-62); 0 = network coordinates
    int* host_counts;     // optional page-locked HOST mirrors, written by the sweep kernel over PCIe ([B] counts, [1] the final overflow word):
    int* host_overflow;   // with dets / lms in page-locked memory too the host needs no copy command at all, only an event wait
    int metric;           // suppression measure of the mask stage: 0 = IoU (inter / union), 1 = IoS (inter / the smaller area; cf_tiles.hip)
};
hipError_t launch_decode_threshold(hipStream_t s, const ThreshParams& p);
// apply per-image 2x3 affines to the (x1,y1),(x2,y2) corners of dets [B][K][stride] in place (utils/post_process.py:83-90)
hipError_t launch_affine_boxes(hipStream_t s, float* dets, const double* trans, int B, int K, int stride);
// rank + suppression matrix + greedy sweep only (candidates already collected)
hipError_t launch_nms_stages(hipStream_t s, const ThreshParams& p);

// bbox_overlap + the two match counts of evaluate (eval_widerface.py:48-74, 172-211); images concatenated, one workgroup each
struct OverlapParams {
    const float* boxes;   // detections, rows of box_stride floats (x1,y1,x2,y2,...)
    const float* query;   // annotations, rows of query_stride floats
    const int* box_off;   // [n_img + 1] first row of each image in boxes
    const int* query_off; // [n_img + 1]
    int n_img, box_stride, query_stride;
    float thresh;
    double* overlaps;     // optional: per image a dense [N][K] block at overlaps_off[img]
    const long long* overlaps_off;
    int* counts;          // optional [n_img][2] (zeroed): detections with a best overlap > thresh, annotations with one
};
hipError_t launch_box_match(hipStream_t s, const OverlapParams& p);

// bilinear stretch-resize of uint8 HWC images (cv2.resize(img, (W, H)) at centerface.py:30; half-pixel centres)
hipError_t launch_resize_u8(hipStream_t s, const uint8_t* src, uint8_t* dst, int B, int h, int w, int H, int W);
// B page-locked host images (device-visible addresses, 16-byte aligned, `bytes` each) -> dst [B][bytes], read over PCIe by a kernel
hipError_t launch_upload_images(hipStream_t s, const void* const* imgs, uint8_t* dst, int B, long long bytes);
// 4:2:0 frames (fmt = CF_YUV_*; planes = B x {y, c0, c1} device addresses, c1 unused for NV12 / NV21) -> uint8 BGR dst [B][H][W][3]:
// cv2.cvtColor(COLOR_YUV2BGR_<fmt>), then cv2.resize to (H, W) when (H, W) != (h, w) (cf_yuv.hip).  h, w, W even; plane addresses
// and pitches multiples of 4
hipError_t launch_yuv_to_bgr(hipStream_t s, int fmt, const void* const* planes, int B, int h, int w, int y_pitch, int c_pitch,
                             uint8_t* dst, int H, int W);

// Aligned face chips (cf_align.hip): similarity estimate from five landmarks + fixed-point bilinear warp of the uint8 BGR batch,
// one launch for every kept face of the batch.  Face n = off[b] + i (image b, keep position i), off = exclusive prefix sum of
// min(counts[b], rows_cap, max_per_image); its landmark row is lms[b * lms_stride + i], or -- lms_stride == 0 -- row
// (prefix sum of counts)[b] + i of a packed table.  Only faces n < cap_faces are written; offsets[B] = the number wanted.
struct AlignParams {
    const uint8_t* img;   // [B][H][W][3] uint8 BGR, 4-byte aligned
    size_t img_dwords;    // readable dwords at img (>= B*H*W*3 / 4, rounded up)
    int B, H, W;
    const float* lms;     // landmark rows of 10 floats, network-input pixels
    int lms_stride;       // rows per image, or 0 = packed
    const int* counts;    // [B]
    int rows_cap;         // rows the producer wrote per image at most
    int max_per_image;    // 0 = all
    int S, format, rgb;   // chip size; 0 = uint8 [N,S,S,3] BGR, 1 = float32 [N,3,S,S] ((u8 - mean) * scale; RGB planes when rgb)
    float mean, scale;
    double tmpl[10];      // template points in chip pixels
    void* chips;          // 4-byte (uint8) / 16-byte (float) aligned
    double* mats;         // [cap_faces][6] chip -> source, or nullptr
    int* offsets;         // [B + 1] or nullptr
    int cap_faces;
};
// chip options -> p (size, format, rgb, mean, scale, template: [5][2] floats or nullptr = ArcFace 112 points * S / 112); host only,
// returns nullptr or what is wrong
const char* align_params_set(AlignParams& p, int size, int format, int rgb, float mean, float scale, const float* tmpl, int max_per_image);
size_t align_chip_bytes(int size, int format);
hipError_t launch_align_faces(hipStream_t s, const AlignParams& p);

// Face redaction in the source frame (cf_redact.hip): every sample of a BGR or 4:2:0 frame that the scaled box (RECT) or its inscribed
// ellipse of some kept face covers is overwritten, by a fill colour (SOLID) or by the mean of its frame-anchored mosaic cell (MOSAIC: a
// first launch writes the cell means of the untouched frame to `cells`, a second one writes the samples).  Frames, plane table and faces:
// cf_frame.h; the launches are sized for B x faces_cap faces and read counts on the device.
struct RedactParams {
    FrameGeo g;           // pitches multiples of 4
    FaceList f;
    int mode, shape, cell;   // CF_REDACT_SOLID / _MOSAIC, CF_REDACT_RECT / _ELLIPSE, the mosaic cell m
    float scale;
    uint8_t fill[3];      // in the frame's channel order (B,G,R or Y,U,V)
    const void* const* planes;   // HOST table of B x {p0, p1, p2} DEVICE addresses (cf_frame.h), all 4-byte aligned
    uint32_t* cells;      // MOSAIC: [B][ceil(h / m)][ceil(w / m)] cell means, one dword each (else unused)
};
// nullptr, or what is wrong with the options / geometry (host only; no device is touched)
const char* redact_check(int format, int mode, int shape, int cell, float scale, int B, int h, int w, int pitch0, int pitch1);
// the same for a B x {p0, p1, p2} plane table: required planes present; device planes and pitches multiples of 4
const char* redact_check_planes(int format, const void* const* planes, int B, int on_device, int pitch0, int pitch1);
size_t redact_cells(int B, int h, int w, int cell);      // dwords of RedactParams::cells
hipError_t launch_redact_faces(hipStream_t s, const RedactParams& p);

// Blur redaction in the source frame (cf_blur.hip): every sample that a kept face covers (frames, faces and coverage as RedactParams)
// becomes the box_b * box_b * box_b filtered value of the untouched frame.  A first launch only reads the frame and writes the value of
// every covered sample into `scratch`, which mirrors the planes in the layout of redact_stage_layout (B * one bytes); a second launch
// only writes the frame.
constexpr int kBlurMaxRadius = 24;
struct BlurParams {
    FrameGeo g;
    FaceList f;
    int shape;
    int radius;           // 1..24: that r for every face; 0: per face, clamp(min(A, Bv) / 8, 1, 24)
    float scale;
    const void* const* planes;   // as RedactParams::planes
    uint8_t* scratch;     // blur_scratch_bytes(format, B, h, w) bytes on the device
};
// nullptr, or what is wrong with the options / geometry (host only): redact_check's words plus the radius
const char* blur_check(int format, int shape, int radius, float scale, int B, int h, int w, int pitch0, int pitch1);
size_t blur_scratch_bytes(int format, int B, int h, int w);
hipError_t launch_blur_faces(hipStream_t s, const BlurParams& p);

// Annotation of the source frame (cf_draw.hip): outlines, landmark dots and a numeric label of every face row, painted by a gather -- a
// prep launch writes one record per (image, row) to `recs`, a paint launch of one workgroup per 64 x 16 tile takes, per pixel, the highest
// layer over the records that touch its tile.  The arithmetic: cf_drawmath.h.
struct DrawRec;
struct DrawGeoOpts;
// the rows of B images: image b has the rows b * stride + i, i < min(counts[b], rows_cap) (rows_cap <= stride), of boxes [.][4] (the
// coordinates of an H x W network input), scores[row * score_step], lms [.][10] (nullptr: none) and info [.][3] = id, hits, misses
// (nullptr: untracked rows, all live)
struct DrawRows { const float* boxes; const float* scores; int score_step; const float* lms; const int32_t* info; const int* counts; int stride, rows_cap, H, W; };
struct DrawParams {
    FrameGeo g;           // pitches multiples of 4
    DrawRows r;
    cf_draw_opts o;
    const void* const* planes;   // as RedactParams::planes
    DrawRec* recs;        // draw_scratch_bytes(B, rows_cap) bytes on the device
};
// nullptr, or what is wrong with the options / geometry (host only; no device is touched)
const char* draw_check(const cf_draw_opts* o, int format, int B, int h, int w, int pitch0, int pitch1);
DrawGeoOpts draw_geo_opts(const cf_draw_opts* o);
size_t draw_scratch_bytes(int B, int rows_cap);
hipError_t launch_draw_faces(hipStream_t s, const DrawParams& p);

// Aligned face chips cut from the caller's frames (cf_align_frame.hip): the estimate, warp and outputs of AlignParams (a.img, a.img_dwords,
// a.H, a.W unused; a.B = the number of frames), sampling B pitched frames of h x w in `format` instead of the network batch.  A landmark
// value x (y) of a.lms is taken as (double)x * sx ((double)y * sy): sx = w / W, sy = h / H for network-coordinate rows, 1.0 for rows
// that are in frame pixels already.  4:2:0 pixels are converted by cf_yuvmath.h as they are read.
struct AlignFrameParams {
    AlignParams a;
    int format;                  // CF_YUV_NV12 .. CF_YUV_YV12, CF_FRAME_BGR
    const void* const* planes;   // HOST table of B x {p0, p1, p2} DEVICE addresses (cf_frame.h; read only), 4-byte aligned
    int h, w, pitch0, pitch1;    // pitches in bytes, multiples of 4
    double sx, sy;
};
// geometry and chip options of cf_align_faces_frame / cf_op_align_frame: nullptr, or what is wrong (host only; fills p.a's options,
// the format and the geometry).  on_device: the planes are read where they are (alignment rules), else they will be staged.
const char* align_frame_check(AlignFrameParams& p, int size, int chip_format, int rgb, float mean, float scale, const float* tmpl,
                              int max_per_image, int format, const void* const* planes, int on_device, int B, int h, int w, int pitch0, int pitch1);
hipError_t launch_align_frame(hipStream_t s, const AlignFrameParams& p);
// sets the text cf_op_last_error returns (cf_ops.hip): for a refusal that has no context to carry it
void op_error_set(const char* text);

// Tiled detection (cf_tiles.hip).  The cutter writes dst [Bf * T][H][W][3] uint8 BGR: image f * T + t = the rectangle rects[t] of frame f,
// converted (4:2:0) and resized to (H, W) as launch_yuv_to_bgr / launch_resize_u8 would the cropped frame.  planes: HOST table of
// Bf x {p0, p1, p2} DEVICE addresses (cf_frame.h; read only); rects: T rectangles on the DEVICE.
// tile_grid: the rectangles of cf_tile_grid (host only).  tiles_check: nullptr, or what is wrong (the text lives in `why`; host only).
int tile_grid(int h, int w, int tile_h, int tile_w, int overlap, int with_full, cf_tile_rect* rects, int cap, int* n);
const char* tiles_check(std::string& why, int format, int Bf, int h, int w, int pitch0, int pitch1, const cf_tile_rect* rects, int T, int H, int W);
hipError_t launch_cut_tiles(hipStream_t s, int format, const void* const* planes, int Bf, int pitch0, int pitch1, const cf_tile_rect* rects,
                            int T, uint8_t* dst, int H, int W);

// Aspect-preserving input (cf_fit.hip; the statement is that file's header).  fit_geometry: the placement of an h x w frame in an H x W
// canvas (host only; CF_EINVAL for an unknown anchor / upscale, a null g or a size below 1).  fit_check: nullptr, or what is wrong with the
// options and the frames (the text lives in `why`; host only).  The fit writes dst [B][H][W][3] uint8 BGR: the frame converted (4:2:0),
// resized to (g.rh, g.rw) and pasted at (g.dy, g.dx), `fill` (B, G, R) elsewhere.  planes: HOST table of B x {p0, p1, p2} DEVICE addresses
// (cf_frame.h; read only).
int fit_geometry(int anchor, int upscale, int h, int w, int H, int W, cf_fit_geom* g);
const char* fit_check(std::string& why, const cf_fit_opts* o, int format, int B, int h, int w, int pitch0, int pitch1, int H, int W);
// rot: the clockwise turn (0, 90, 180, 270) that makes the stored h x w frames upright; g then places the UPRIGHT view (rot_geometry).
// 90 and 270 go to the quarter-turn kernel of cf_rot.hip (launch_rot_quarter: one launch over nb <= kFitFrames checked frames).
constexpr int kFitFrames = 64;                       // frames per launch: 3 x 64 pointers = 1.5 KB of kernel arguments
hipError_t launch_fit_frames(hipStream_t s, int rot, int format, const void* const* planes, int B, int h, int w, int pitch0, int pitch1,
                             const cf_fit_geom& g, const uint8_t* fill, uint8_t* dst, int H, int W);
void launch_rot_quarter(hipStream_t s, int rot, int format, const FramePtrs<kFitFrames>& tab, int nb, uint8_t* dst, const cf_fit_geom& g, uint32_t fill,
                        int h, int w, int pitch0, int pitch1, int H, int W);
// The rows of a threshold decode over B fitted images mapped back into the h x w frames: rows i < min(counts[b], rows) of dets_net
// [B][rows][4], scores[(b * rows + i) * score_stride], lms_net [B][rows][10] are filtered (non-finite corners, centre outside the
// content), mapped and compacted per image in order.
struct UnfitParams {
    cf_fit_geom g; int h, w, B;
    const float* dets_net; const float* scores; int score_stride; const float* lms_net; const int* counts; int rows;
    // outputs (device), frame pixels
    int max_out;
    float* dets;          // [B][max_out][5]
    float* lms;           // [B][max_out][10]
    float* corners;       // [B][max_out][4]: the box rows FaceList::boxes takes with (H, W) = (h, w)
    int* out_counts;      // [B], may exceed max_out
    int* flags;           // [B]: bit 0 = the image had counts > rows
};
hipError_t launch_unfit_rows(hipStream_t s, const UnfitParams& p);

// Rotated sources (cf_rot.hip; the statement is in include/centerface_hip.h).  rot_geometry: the placement of the UPRIGHT view of an
// h x w frame (host only; o has passed rot_check).  rot_check: nullptr, or what is wrong with the turn, the options and the frames.
// The fit of the upright views is launch_fit_frames with the turn.
// launch_unrot_rows (cf_fit.hip): the unfit behind it, p.g from rot_geometry, p.h x p.w the stored frame; rot == 0 is launch_unfit_rows.
int rot_geometry(const cf_rot_opts* o, int h, int w, int H, int W, cf_fit_geom* g);
const char* rot_check(std::string& why, const cf_rot_opts* o, int format, int B, int h, int w, int pitch0, int pitch1, int H, int W);
hipError_t launch_unrot_rows(hipStream_t s, const UnfitParams& p, int rot);

// Multi-scale views (cf_views.hip; the statement is in include/centerface_hip.h).  view_layout: the views of cf_view_layout (host only).
// views_check: nullptr, or what is wrong with the frames and the view table (the text lives in `why` and names the view; host only);
// views_table_check: its view-table part alone.  The cutter writes dst [Bf * V][H][W][3] uint8 BGR: image f * V + v = `fill` (B, G, R)
// with the source rectangle of views[v] of frame f, converted (4:2:0) and resized, pasted at its content rectangle.  planes: HOST table
// of Bf x {p0, p1, p2} DEVICE addresses (cf_frame.h; read only); views: V views on the DEVICE.
int view_layout(const cf_view_opts* o, int h, int w, int H, int W, cf_view* views, int cap, int* n);
const char* views_table_check(std::string& why, int h, int w, const cf_view* views, int V, int H, int W);
const char* views_check(std::string& why, int format, int Bf, int h, int w, int pitch0, int pitch1, const cf_view* views, int V, int H, int W);
hipError_t launch_cut_views(hipStream_t s, int format, const void* const* planes, int Bf, int pitch0, int pitch1, const cf_view* views, int V,
                            const uint8_t* fill, uint8_t* dst, int H, int W);

// Packed views (cf_views.hip; the statement is in include/centerface_hip.h).  pack_views: the shelf packer of cf_pack_views (host only;
// the arguments have been checked).  pack_check: nullptr, or what is wrong with P placements of Bf frames of h x w in N canvases of
// H x W -- ranges, every view by views_table_check's rules, two overlapping contents on one canvas (both indices named; host only).
// pack_table: the ONE device blob of a packed batch, built on the host: the placements sorted by canvas (stable), the CSR of that order
// by canvas [N + 1], the CSR by frame [Bf + 1] with, per frame, the sorted positions of its placements in placement-index order [P], and
// the plane addresses 3 x Bf (YV12's chroma planes swapped: the I420 kernel serves both).  PackDev: the blob's parts on the device.
int pack_views(const cf_view* views, int V, int Bf, int H, int W, int gutter, cf_place* places, int cap, int* n_canvases);
const char* pack_check(std::string& why, int h, int w, const cf_place* places, int P, int N, int Bf, int H, int W);
struct PackHost { std::vector<unsigned char> blob; size_t off_cv, off_fr, off_idx, off_planes; int most; };      // most: placements of any frame, at most
PackHost pack_table(const cf_place* places, int P, int N, int Bf, const void* const* planes, int format);
struct PackDev { const cf_place* places; const int* cv_off; const int* fr_off; const int* fr_idx; const uint8_t* const* planes; };
inline PackDev pack_dev(const PackHost& t, const void* dev) {
    const unsigned char* b = (const unsigned char*)dev;
    return PackDev{(const cf_place*)b, (const int*)(b + t.off_cv), (const int*)(b + t.off_fr), (const int*)(b + t.off_idx), (const uint8_t* const*)(b + t.off_planes)};
}
// dst [N][H][W][3] uint8 BGR, every byte written once by one launch; the caller has run views_check's frame part and pack_check
// rot: the clockwise turn (0, 90, 180, 270) that makes the stored h x w frames upright (the placements' sources are then rectangles of
// the upright view, cf_views_rot.hip)
hipError_t launch_cut_packed(hipStream_t s, int rot, int format, const PackDev& t, int N, int h, int w, int pitch0, int pitch1, const uint8_t* fill,
                             uint8_t* dst, int H, int W);

// Rotated sources through packed views (cf_views_rot.hip; the statement is in include/centerface_hip.h).  rot: the clockwise turn (0, 90,
// 180, 270) that makes the stored h x w frames upright; the placements' sources are rectangles of the upright view.  pack_rot_check:
// nullptr, or what is wrong with the turn or with the placements (pack_check against the upright view's size; host only).
// launch_cut_packed_quarter: launch_cut_packed's rot 90 / 270 (the arguments have been checked).
const char* pack_rot_check(std::string& why, int rot, int h, int w, const cf_place* places, int P, int N, int Bf, int H, int W);
void launch_cut_packed_quarter(hipStream_t s, int rot, int format, const PackDev& t, int N, uint8_t* dst, uint32_t fill, int h, int w, int pitch0, int pitch1,
                               int H, int W);

// The merge of the rows of a threshold decode over the images of a tiled, views or packed forward (cf_tiles.hip, cf_collect.h): rows
// i < min(counts[img], rows) of dets_net [.][rows][4], scores[(img * rows + i) * score_stride], lms_net [.][rows][10] are filtered
// (non-finite corners; the edge rule; behind views and placements the centre rule), mapped into the STORED h x w frame and collected per
// frame in (source, row) order; then rank / mask / sweep with `metric` and `thresh`.  kind names the sources of a frame:
//   MERGE_TILES   rects [V]: image f * V + t is rectangle t stretched over the H x W canvas
//   MERGE_VIEWS   views [V]: image f * V + v is view v
//   MERGE_PLACED  pack: the placements of the frame, image = the placement's canvas; V = PackHost::most; rot = the turn (0, 90, 180, 270)
//                 that makes the stored frames upright, the placements' sources being rectangles of the upright view
enum { MERGE_TILES = 0, MERGE_VIEWS = 1, MERGE_PLACED = 2 };
struct MergeParams {
    int kind;
    const cf_tile_rect* rects;   // device
    const cf_view* views;        // device
    PackDev pack;
    int V, Bf, h, w, H, W, rot;  // (H, W: MERGE_TILES only; rot: MERGE_PLACED only, else 0)
    const float* dets_net; const float* scores; int score_stride; const float* lms_net; const int* counts; int rows;
    int metric; float thresh, edge;
    // workspace (device), cap = V * rows candidates per frame
    float* cand;          // [Bf][cap][16]
    int* cand_count;      // [Bf]
    int* order;           // [Bf][cap]
    unsigned long long* mask;    // [Bf][cap][ceil(cap / 64)]: merge_mask_bytes
    // outputs (device), frame pixels
    int max_out;
    float* dets;          // [Bf][max_out][5]
    float* lms;           // [Bf][max_out][10]
    float* corners;       // [Bf][max_out][4]: the box rows FaceList::boxes takes with (H, W) = (h, w)
    int* out_counts;      // [Bf], may exceed max_out
    int* flags;           // [Bf]: bit 0 = some image of the frame had counts > rows
};
size_t merge_mask_bytes(int Bf, int V, int rows);
constexpr size_t kMergeMaskLimit = (size_t)256 << 20;      // refused with CF_ENOMEM above this, before any launch
hipError_t launch_merge(hipStream_t s, const MergeParams& p);

// Flip test (cf_flip.hip; the statement is in include/centerface_hip.h).  mirror_check: nullptr, or what is wrong with the format and sizes
// of a batch to mirror (the text lives in `why`; host only).  launch_mirror_batch: dst holds 2B network inputs of in_format (uint8
// [.][H][W][3] or float32 [.][3][H][W]; 16-byte aligned); images B .. 2B-1 become images 0 .. B-1 of src with their columns reversed and,
// when src != dst, images 0 .. B-1 of dst become those of src in the same launch.  src == dst mirrors the first half of dst into its
// second.  src is 4-byte aligned at least.  launch_flip_heads: rec [2B][h][w][16] float32 -> the merged records in rec [0 .. B) and their
// heat in hm_plane [B][h * w], in place.
const char* mirror_check(std::string& why, int in_format, int B, int H, int W);
hipError_t launch_mirror_batch(hipStream_t s, int in_format, const void* src, void* dst, int B, int H, int W);
hipError_t launch_flip_heads(hipStream_t s, float* rec, float* hm_plane, int B, int h, int w);

// Face tracks across video frames (cf_track.hip; the statement is that file's header).  One update of the streams stream0 .. stream0 + B - 1
// with the rows i < min(counts[b], rows) of image b: boxes [B][rows][4], scores[(b * rows + i) * score_stride], lms [B][rows][10].
// All pointers are device-visible; boxes rows are 16-byte aligned.
constexpr int kTrackMaxSlots = 1024, kTrackMaxStreams = 4096;
struct TrackParams {
    const float* boxes; const float* scores; int score_stride; const float* lms; const int* counts; int rows, B;
    float iou_thresh; int max_age, min_hits, max_tracks; float hold_grow;
    // two thresholds (cf_track_create_weak): weak != 0 runs the second pass for the rows with !(score > birth_score)
    int weak; float birth_score, weak_iou;
    void set_weak(const cf_track_weak_opts* w) { weak = w ? 1 : 0; birth_score = w ? w->birth_score : 0.f; weak_iou = w ? w->weak_iou : 0.f; }
    // state (device), owned by the tracker: n_streams x max_tracks slots
    int stream0;
    int* meta;            // [S][max_tracks][4]: alive, id, hits, misses
    float* rec;           // [S][max_tracks][16]: box, score, lms[10], 0
    int* next_id;         // [S]
    // outputs (device): the alive slots of every stream, compacted in slot order
    float* dets;          // [B][max_tracks][5]
    float* lms_out;       // [B][max_tracks][10]
    int* info;            // [B][max_tracks][3]: id, hits, misses
    float* corners;       // [B][max_tracks][4]: the box rows FaceList::boxes takes, as MergeParams::corners
    int* out_counts;      // [B], <= max_tracks
    int* flags;           // [B]: bit 0 = a new row found no free slot and was dropped; bit 1 = a weak row matched
    // constant velocity (cf_track_create_ex), behind everything else so that the kernel arguments of the other trackers lie where they lay:
    // motion != 0 matches against the predicted boxes, learns `vel` from every match and coasts the held slots
    int motion; float gain, damp;
    void set_motion(const cf_track_motion_opts* m) { motion = m ? 1 : 0; gain = m ? m->gain : 0.f; damp = m ? m->damp : 0.f; }
    float* vel;           // state [S][max_tracks][2]: vx, vy -- motion trackers only, else nullptr (never read)
    int* tmeta;           // the follower's FollowParams::tmeta [S][max_tracks][6], or nullptr before the first follow: a coast moves tpl_box along
    float* vel_out;       // output [B][max_tracks][2] in output-row order, or nullptr (motion trackers only)
};
// nullptr, or what is wrong with the options / the number of streams (host only); the weak and the motion options may be null (a plain tracker)
const char* track_check(const cf_track_opts* o, int n_streams);
const char* track_weak_check(const cf_track_weak_opts* w);
const char* track_motion_check(const cf_track_motion_opts* m);
hipError_t launch_track_update(hipStream_t s, const TrackParams& p);

// The follower (cf_follow.hip; the statement is in include/centerface_hip.h): block matching of every alive slot of the streams
// stream0 .. stream0 + g.B - 1 in the luma of the g.B frames, then the rows of TrackParams' step 5 again, from the moved state.
constexpr int kFollowSide = 16, kFollowMaxSearch = 8, kFollowMaxSad = 255 * kFollowSide * kFollowSide;
constexpr size_t kFollowSlotBytes = kFollowSide * kFollowSide + 6 * sizeof(int);      // tpl | tpl_c, tpl_id, tpl_box[4]
struct FollowParams {
    FrameGeo g;                  // pitch0 a multiple of 4; only plane 0 (BGR rows or the Y plane) is read
    const void* const* planes;   // HOST table of g.B x {p0, p1, p2} DEVICE addresses (cf_frame.h), p0 4-byte aligned
    int search, max_sad;
    double fx, fy;               // frame pixels per unit of the rows' space: w / W, h / H, or 1.0 for rows in frame pixels
    int stream0, max_tracks; float hold_grow;
    // state (device), owned by the tracker: TrackParams' meta and rec, and the follower records of all n_streams x max_tracks slots
    int* meta; float* rec;
    uint8_t* tpl;                // [S][max_tracks][16][16]
    int* tmeta;                  // [S][max_tracks][6]: tpl_c, tpl_id, the bits of tpl_box
    int* slot_moves;             // scratch [g.B][max_tracks][4]: px, py, SAD, code per SLOT
    // outputs (device), as TrackParams', plus moves [g.B][max_tracks][4] in the same row order
    float* dets; float* lms_out; int* info; float* corners; int* out_counts; int* moves;
};
// nullptr, or what is wrong with the options / geometry (host only; no device is touched)
const char* follow_check(const cf_follow_opts* o, int format, int B, int h, int w, int pitch0, int pitch1);
hipError_t launch_track_follow(hipStream_t s, const FollowParams& p);

// Scene cuts (cf_scene.hip; the statement is in include/centerface_hip.h): the signature of g.B frames, the check of the streams
// stream0 .. stream0 + g.B - 1 against their last signature and, on CUT with `meta`, the reset of the stream's track slots.
constexpr int kSceneSig = 128, kScenePart = 72, kSceneRows = 16;      // int32 of a signature / of a workgroup's partials; rows of a workgroup
struct SceneParams {
    FrameGeo g;                  // pitch0 a multiple of 4; only plane 0 (BGR rows or the Y plane) is read
    const void* const* planes;   // HOST table of g.B x {p0, p1, p2} DEVICE addresses (cf_frame.h), p0 4-byte aligned
    int hist_thresh, grid_thresh, stream0;
    // state (device), owned by the scene object
    int* sig;                    // [S][128]: bins, cell means
    int* st;                     // [S][4]: h, w, valid, run
    // the tracker's TrackParams::meta (max_tracks slots per stream), or nullptr: nothing is reset
    int* meta; int max_tracks;
    int* part;                   // scratch, scene_part_bytes(g.B, g.h)
    int* out;                    // [g.B][4] (device): code, hist, grid, run
    int* sig_out;                // [g.B][128] (device) or nullptr: the frames' signatures
};
// nullptr, or what is wrong with the options / geometry (host only; no device is touched)
const char* scene_check(const cf_scene_opts* o, int format, int B, int h, int w, int pitch0, int pitch1);
size_t scene_part_bytes(int B, int h);
hipError_t launch_scene_check(hipStream_t s, const SceneParams& p);

// Lookback (cf_lookback.hip; the statement is in include/centerface_hip.h): one step of the streams stream0 .. stream0 + B - 1 -- with
// push != 0 the tracked rows of image b (in_dets [B][in_stride][5], in_lms [.][.][10], in_info [.][.][3], in_counts [B]; scene [B][4] as
// SceneParams::out, or nullptr) enter the queue of stream stream0 + b; then the due entry leaves it with the back-filled rows behind its own.
constexpr int kLookbackMaxDepth = 32, kLookbackMaxRows = 1024;
struct LookbackParams {
    int depth, rows, confirm; float grow;
    int stream0, B, push;
    const float* in_dets; const float* in_lms; const int* in_info; const int* in_counts; int in_stride;
    const int* scene;
    // state (device), owned by the object: n_streams queues of depth + 1 entries of `rows` rows
    int* qmeta;           // [S][4]: head, fill, max_id, seq_next
    int* pend;            // [S]: pending_cut
    int* emeta;           // [S][depth + 1][4]: seq, cut, n, 0
    float* rec;           // [S][depth + 1][rows][16]: box, score, lms[10], 0
    int* info;            // [S][depth + 1][rows][4]: id, hits, misses, born
    // outputs (device), stride `rows` per image; corners may be nullptr
    float* dets; float* lms; int* out_info; float* corners; int* counts; int* state;
    // the trace of an enabled object (cf_lookback_trace_enable), nullptr otherwise: a back-filled row of e_j is moved by trace[e_j][row][j - 1]
    const int* trace;     // [S][depth + 1][rows][depth][4]: PX, PY, SAD, code at the distances 1 .. depth
    double fx, fy;        // frame pixels per unit of the rows' space (FollowParams)
    int* moves;           // output [B][rows][4], or nullptr
};
// nullptr, or what is wrong with the options / the number of streams (host only)
const char* lookback_check(const cf_lookback_opts* o, int n_streams);
hipError_t launch_lookback_step(hipStream_t s, const LookbackParams& p);

// The lookback's trace (cf_lookback.hip; the statement is in include/centerface_hip.h, "a step with push"): ahead of a pushing step of an
// enabled object, the luma of the g.B frames goes into the ring plane of the entry the push will fill (retain), and every row the push
// will call born is matched backwards through the retained planes of the queued entries (trace).  Both read the queue's words as the
// step before left them; the step kernel behind them advances the queue and reads the trace.
constexpr int kLookbackLumaAlign = 16;
__host__ __device__ inline int lookback_luma_pitch(int w) { return (w + kLookbackLumaAlign - 1) & ~(kLookbackLumaAlign - 1); }
struct LookbackTraceParams {
    FrameGeo g;                  // pitch0 a multiple of 4; only plane 0 (BGR rows or the Y plane) is read
    const void* const* planes;   // HOST table of g.B x {p0, p1, p2} DEVICE addresses (cf_frame.h), p0 4-byte aligned
    int search, max_sad;
    double fx, fy;
    uint8_t* luma;               // [S][depth + 1][g.h][lookback_luma_pitch(g.w)]
    int* trace;                  // as LookbackParams::trace
    LookbackParams step;         // the step this goes ahead of (push != 0): its options, inputs and queue words
};
hipError_t launch_lookback_trace(hipStream_t s, const LookbackTraceParams& p);

// Best-shot selection (cf_bestshot.hip; the statement is in include/centerface_hip.h).  The table's device state, per stream and entry:
// erec kBestRecInts int32 (state, id, best_t, first_t, last_t, n_offered, done_seq, parts[4], -, Q as int64, -, -), erow kBestRowFloats
// float32 (det[5], lms[10], -), the chip; per stream smeta kBestStreamInts int32 (t, seq, sticky flags, -).  All zero at first.
constexpr int kBestMaxEntries = 2048, kBestMaxRows = kTrackMaxSlots, kBestRecInts = 16, kBestRowFloats = 16, kBestStreamInts = 4, kBestScratchInts = 6;
struct BestTable { int size, entries, min_hits, terms; int32_t* erec; float* erow; uint8_t* chips; int32_t* smeta; };
// the rows of B images: boxes [B][rows][4], scores (stride score_stride floats per row), lms [B][rows][10], info [B][rows][3], counts [B]
struct BestRows { const float* boxes; const float* scores; int score_stride; const float* lms; const int32_t* info; const int* counts; int rows; };
struct BestOffer {
    BestTable t; BestRows r;
    int stream0, B;
    const uint8_t* chips;        // [cap_faces][S][S][3], 16-byte aligned
    const int* offsets;          // [B + 1]
    int cap_faces;
    double fx, fy;
    long long* q;                // [cap_faces]: Q of the chip of an eligible row, else -1 (the caller's `quality`, or scratch)
    int32_t* sc;                 // scratch [cap_faces][kBestScratchInts]: parts[4], the row b * rows + i whose image names the chip or -1, -
    int32_t* jobs;               // scratch [B][rows][2]: chip -> entry (of all streams), or -1
    int32_t* flags;              // [B] or nullptr
};
struct BestCollect {
    BestTable t;
    int stream0, B, cap, flush;
    void* chips; long long* quality; int32_t* records; float* dets; float* lms; int32_t* counts; int32_t* pending; int32_t* flags;      // [B][cap]... / [B]; any may be nullptr
    int32_t* jobs;               // scratch [B][cap][2]
};
// nullptr, or what is wrong with the options / the number of streams (host only)
const char* best_check(const cf_bestshot_opts* o, int n_streams);
size_t best_chip_bytes(int size);
hipError_t launch_best_score(hipStream_t s, const BestOffer& p);       // the score kernel alone: t.size, t.min_hits, t.terms, r, chips, offsets, q, sc
hipError_t launch_best_offer(hipStream_t s, const BestOffer& p);       // score, decide, copy
hipError_t launch_best_collect(hipStream_t s, const BestCollect& p);   // collect, copy

// layout converters used by cf_get_heads and the per-op test entry points
hipError_t launch_nchw_to_nhwc(hipStream_t s, int dtype, const float* src /*f32 NCHW*/, void* dst /*T NHWC*/,
                               int B, int C, int H, int W);
hipError_t launch_blocked_to_nchw(hipStream_t s, int dtype, const void* src /*pixel-block order*/, float* dst /*f32 NCHW*/, int B, int C, int H, int W);
hipError_t launch_nchw_to_blocked(hipStream_t s, int dtype, const float* src /*f32 NCHW*/, void* dst /*pixel-block order, whole 32-pixel blocks*/, int B, int C, int H, int W);
hipError_t launch_nhwc_to_nchw(hipStream_t s, int dtype, const void* src /*T NHWC*/, float* dst /*f32 NCHW*/,
                               int B, int C, int H, int W);

}  // namespace cf
