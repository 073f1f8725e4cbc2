// Rotated sources through packed views: the canvases of cf_forward_packed filled from the UPRIGHT view of frames that are stored a
// quarter, a half or three quarters of a turn away from it, and the merge that maps the rows back into the STORED frame.  The statement
// is in include/centerface_hip.h (cf_forward_packed_rot); in short, for a stored frame F of h x w and rot = the clockwise turn that makes
// it upright, the upright view U of hu x wu is
//   rot  90: (w, h)  U[y][x] = F[h-1-x][y]         rot 180: (h, w)  U[y][x] = F[h-1-y][w-1-x]         rot 270: (w, h)  U[y][x] = F[x][w-1-y]
// every placement's source rectangle is in pixels of U, and inside a content the canvas is
//   resize(bgr(U_f)[sy0 : sy0 + sh, sx0 : sx0 + sw], (dh, dw))
// with bgr() taken per STORED pixel (a 4:2:0 pixel's chroma is that of its own 2 x 2 block in F) and the fixed-point resize of
// cf_cvresize.h, taps clamped at the source rectangle: the kernels read F through the index map and never build U.  rot 0 is
// launch_cut_packed / launch_merge_packed of cf_views.hip: the same code, the same bytes.
//
// CUT, rot 180.  cut_packed_kernel (cf_views.hip) with mirrored taps: adjacent canvas columns are still adjacent stored columns, so its
// layout carries over -- an LDS placement list per 128 x (8 * kViewRows) canvas tile, a lane owns four adjacent canvas columns and
// kViewRows rows, three dword stores per row.
//
// CUT, rot 90 / 270.  Adjacent canvas COLUMNS are adjacent stored ROWS: with that layout every tap of a wave would be a cache line of its
// own.  Here the transposition of rot_quarter_kernel (cf_rot.hip) sits under the placement list of cut_packed_kernel: a workgroup owns a
// canvas tile of kQTY rows x kQTX columns and lists the placements that touch it in rounds of kPackList (ballot, the four wave counts
// through LDS, placement order: the list cannot overflow, a canvas with more placements takes more rounds).  A wave's 64 lanes run along
// the tile's canvas ROWS, so for one canvas column their taps run along ONE stored row (two: the bilinear pair) and coalesce; a lane's
// row coefficients are computed once per placement, the tile's column coefficients once per placement and workgroup (LDS).  A lane keeps
// its eight pixels in registers across the list, `fill` where no placement wrote, and packs them into an LDS tile whose row pitch of 25
// dwords is odd; the tile leaves as whole-row dword stores.
//
// Both: one writer per byte; a tile no placement touches stores fill and reads no frame; every tap lies inside the placement's source
// rectangle mapped into F, pitch padding is never read; frames are never written; one launch covers all N canvases and all frames (the
// plane table of the blob reaches every frame).
//
// MERGE.  packed_collect_kernel (cf_views.hip) with the turn: the three drop rules in canvas coordinates, unchanged, except that "source
// side interior to the frame" is tested against U (hu, wu); a kept point goes to U first,
//   ux(x) = ((double)x - dx) * ((double)sw / dw) + sx0,   uy(y) = ((double)y - dy) * ((double)sh / dh) + sy0
// (float64 in this order, no contraction: the file is built with -ffp-contract=off), then to F by the table of cf_unfit_rows, the
// difference taken in float64 and rounded to float32 once; landmarks point by point, the box an ASSIGNMENT of mapped corners.  The NMS
// stages of cf_decode.hip then run on the stored-frame boxes.  The compaction is a prefix sum: the order is deterministic.
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_cvresize.h"
#include "cf_yuvmath.h"
#include "cf_fitpx.h"
#include <cstdio>
#include <string>

namespace cf {
namespace {

constexpr int kViewRows = 4;                                 // rot 180: canvas rows per lane, as cf_views.hip
constexpr int kPackTileW = 128, kPackTileH = 8 * kViewRows;  // rot 180: the canvas tile of a workgroup, as cut_packed_kernel
constexpr int kPackList = 256;                               // placements per list round: one per thread
constexpr int kQTY = 64, kQTX = 32;                          // rot 90 / 270: the canvas tile of a workgroup (rows = the lanes of a wave), as cf_rot.hip
constexpr int kQRowDw = kQTX * 3 / 4;                        // 24 dwords of pixels per tile row ...
constexpr int kQPitch = kQRowDw + 1;                         // ... at an odd pitch

// The pixel U[yu][xu] of the upright view, read from the stored frame and converted there -> B | G << 8 | R << 16.
// SRC: 0 = BGR rows, 1 = one interleaved chroma plane (NV12 / NV21), 2 = two chroma planes (I420; YV12 on a swapped table);
// VF: V first in the interleaved pairs (NV21); ROT: 1 = 90, 2 = 180, 3 = 270
template <int SRC, bool VF, int ROT>
__device__ __forceinline__ uint32_t turned_tap(const uint8_t* p0, const uint8_t* p1, const uint8_t* p2, int pitch0, int pitch1, int h, int w, int yu, int xu) {
    const int y = ROT == 1 ? h - 1 - xu : ROT == 2 ? h - 1 - yu : xu;
    const int x = ROT == 1 ? yu : ROT == 2 ? w - 1 - xu : w - 1 - yu;
    if constexpr (SRC == 0) {
        const uint8_t* q = p0 + (size_t)y * pitch0 + 3 * x;
        return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    } else {
        return yuv_px(p0[(size_t)y * pitch0 + x], chroma_at<SRC == 1, VF>(p1, p2, pitch1, y >> 1, x >> 1));
    }
}

// one canvas pixel from its four taps: the horizontal pass in the upright view first, then the vertical one (cf_cvresize.h)
template <int SRC, bool VF, int ROT>
__device__ __forceinline__ uint32_t turned_pixel(const uint8_t* p0, const uint8_t* p1, const uint8_t* p2, int pitch0, int pitch1, int h, int w,
                                                 int y0, int y1, int b0, int b1, int x0, int x1, int a0, int a1) {
    const uint32_t t00 = turned_tap<SRC, VF, ROT>(p0, p1, p2, pitch0, pitch1, h, w, y0, x0);
    const uint32_t t01 = turned_tap<SRC, VF, ROT>(p0, p1, p2, pitch0, pitch1, h, w, y0, x1);
    const uint32_t t10 = turned_tap<SRC, VF, ROT>(p0, p1, p2, pitch0, pitch1, h, w, y1, x0);
    const uint32_t t11 = turned_tap<SRC, VF, ROT>(p0, p1, p2, pitch0, pitch1, h, w, y1, x1);
    uint32_t ch[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int s = 8 * c;
        const int h0 = (int)((t00 >> s) & 255) * a0 + (int)((t01 >> s) & 255) * a1;
        const int h1 = (int)((t10 >> s) & 255) * a0 + (int)((t11 >> s) & 255) * a1;
        ch[c] = (uint32_t)cv_linear_vpass(b0, b1, h0, h1);
    }
    return pack_bgr(ch[0], ch[1], ch[2]);
}

// One round of the placement list of a tile [tx0, tx0 + tw) x [ty0, ty0 + th) of canvas n: thread tid tests placement base + tid, the
// hits go to s_list in placement order.  Returns their number (uniform); the caller synchronises before the next round.
__device__ __forceinline__ int list_round(const PackDev& t, int base, int k1, int tx0, int ty0, int tw, int th, int* s_list, int* s_cnt) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cand = base + tid;
    bool hit = false;
    if (cand < k1) {
        const cf_view r = t.places[cand].view;
        hit = r.dx < tx0 + tw && r.dx + r.dw > tx0 && r.dy < ty0 + th && r.dy + r.dh > ty0;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int at = 0, cnt = 0;
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) { if (w2 < wave) at += s_cnt[w2]; cnt += s_cnt[w2]; }
    if (hit) s_list[at + __popcll(m & ((1ull << lane) - 1ull))] = cand;
    __syncthreads();
    return cnt;
}

// rot 180: cut_packed_kernel with mirrored taps (hu = h, wu = w)
template <int SRC, bool VF>
__global__ void __launch_bounds__(256) cut_packed_half_kernel(PackDev t, uint8_t* dst, uint32_t fill, int h, int w, int pitch0, int pitch1, int H, int W,
                                                              int tiles_x) {
    __shared__ int s_list[kPackList];
    __shared__ int s_cnt[4];
    const int tid = (int)threadIdx.x, n = (int)blockIdx.y;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int tx0 = tx * kPackTileW, ty0 = ty * kPackTileH;
    const int X0 = tx0 + 4 * (tid & 31), Y0 = ty0 + kViewRows * (tid >> 5);
    const bool live = X0 < W && Y0 < H;                   // (W % 4 == 0: a live lane's four columns are inside)
    uint32_t px[kViewRows][4];
#pragma unroll
    for (int i = 0; i < kViewRows; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) px[i][k] = fill;
    const int k0 = t.cv_off[n], k1 = t.cv_off[n + 1];
    for (int base = k0; base < k1; base += kPackList) {   // uniform trip count
        const int cnt = list_round(t, base, k1, tx0, ty0, kPackTileW, kPackTileH, s_list, s_cnt);
        if (live)
            for (int j = 0; j < cnt; ++j) {
                const cf_place& pl = t.places[__builtin_amdgcn_readfirstlane(s_list[j])];
                const cf_view r = pl.view;
                if (X0 + 4 <= r.dx || X0 >= r.dx + r.dw || Y0 + kViewRows <= r.dy || Y0 >= r.dy + r.dh) continue;      // not this lane's pixels
                bool in[4];
                int x0[4], x1[4], a0[4], a1[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = X0 + k - r.dx;
                    in[k] = x >= 0 && x < r.dw;
                    cv_linear_coeffs(min(max(x, 0), r.dw - 1), r.sw, r.dw, true, x0[k], x1[k], a0[k], a1[k]);      // a foreign column: the edge's taps, not used
                    x0[k] += r.sx0; x1[k] += r.sx0;
                }
                const uint8_t* p0 = t.planes[3 * pl.frame];
                const uint8_t* p1 = t.planes[3 * pl.frame + 1];
                const uint8_t* p2 = t.planes[3 * pl.frame + 2];
#pragma unroll
                for (int i = 0; i < kViewRows; ++i) {
                    const int y = Y0 + i - r.dy;
                    if (y < 0 || y >= r.dh) continue;          // (inside the content, so inside the canvas)
                    int y0, y1, b0, b1;
                    cv_linear_coeffs(y, r.sh, r.dh, false, y0, y1, b0, b1);
                    y0 += r.sy0; y1 += r.sy0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t v = turned_pixel<SRC, VF, 2>(p0, p1, p2, pitch0, pitch1, h, w, y0, y1, b0, b1, x0[k], x1[k], a0[k], a1[k]);
                        if (in[k]) px[i][k] = v;
                    }
                }
            }
        __syncthreads();                                      // s_list and s_cnt are rewritten by the next round
    }
    if (!live) return;
    uint8_t* out = dst + (((size_t)n * H + Y0) * W + X0) * 3;
#pragma unroll
    for (int i = 0; i < kViewRows; ++i)
        if (Y0 + i < H) fit_store(out + (size_t)i * W * 3, px[i]);
}

// rot 90 (ROT 1) / 270 (ROT 3): grid (tiles of a canvas, canvases); thread = (wave, lane): lane -> the tile's canvas row, wave -> eight
// of its columns as two groups of four (three dwords each, as fit_store packs them)
template <int SRC, bool VF, int ROT>
__global__ void __launch_bounds__(256) cut_packed_quarter_kernel(PackDev t, uint8_t* dst, uint32_t fill, int h, int w, int pitch0, int pitch1, int H, int W,
                                                                 int tiles_x) {
    __shared__ uint32_t tile[kQTY * kQPitch];
    __shared__ int4 colc[kQTX];
    __shared__ int s_list[kPackList];
    __shared__ int s_cnt[4];
    const int tid = (int)threadIdx.x, ly = tid & 63, wave = tid >> 6, n = (int)blockIdx.y;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int TX0 = tx * kQTX, TY0 = ty * kQTY;
    const int Y = TY0 + ly, XW = TX0 + 8 * wave;          // the lane's canvas row, the wave's first canvas column
    uint32_t px[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) px[k] = fill;
    const int k0 = t.cv_off[n], k1 = t.cv_off[n + 1];
    for (int base = k0; base < k1; base += kPackList) {   // uniform trip count
        const int cnt = list_round(t, base, k1, TX0, TY0, kQTX, kQTY, s_list, s_cnt);
        for (int j = 0; j < cnt; ++j) {                    // (uniform: the barriers below are reached by every thread)
            const cf_place& pl = t.places[__builtin_amdgcn_readfirstlane(s_list[j])];
            const cf_view r = pl.view;
            if (tid < kQTX) {                              // the tile's column coefficients for this placement, once per workgroup
                int x0, x1, a0, a1;
                cv_linear_coeffs(min(max(TX0 + tid - r.dx, 0), r.dw - 1), r.sw, r.dw, true, x0, x1, a0, a1);      // a foreign column: the edge's taps, not used
                colc[tid] = make_int4(x0 + r.sx0, x1 + r.sx0, a0, a1);
            }
            __syncthreads();
            const int y = Y - r.dy;
            if (y >= 0 && y < r.dh && XW < r.dx + r.dw && XW + 8 > r.dx) {      // (a row of the content is a row of the canvas: Y < H)
                int y0, y1, b0, b1;
                cv_linear_coeffs(y, r.sh, r.dh, false, y0, y1, b0, b1);
                y0 += r.sy0; y1 += r.sy0;
                const uint8_t* p0 = t.planes[3 * pl.frame];
                const uint8_t* p1 = t.planes[3 * pl.frame + 1];
                const uint8_t* p2 = t.planes[3 * pl.frame + 2];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int x = XW + k - r.dx;           // (uniform over the wave)
                    if (x >= 0 && x < r.dw) {
                        const int4 c = colc[8 * wave + k];
                        px[k] = turned_pixel<SRC, VF, ROT>(p0, p1, p2, pitch0, pitch1, h, w, y0, y1, b0, b1, c.x, c.y, c.z, c.w);
                    }
                }
            }
            __syncthreads();                                  // colc is rewritten by the next placement, s_list by the next round
        }
        __syncthreads();                                      // (cnt == 0: s_cnt has been read by everyone)
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        uint32_t* o = tile + ly * kQPitch + (wave * 2 + j) * 3;
        o[0] = px[4 * j] | (px[4 * j + 1] << 24);
        o[1] = (px[4 * j + 1] >> 8) | (px[4 * j + 2] << 16);
        o[2] = (px[4 * j + 2] >> 16) | (px[4 * j + 3] << 8);
    }
    __syncthreads();
    // the tile's rows out, dword by dword: W % 4 == 0, so a row of the canvas ends on a dword of the tile row
    const int row_dw = min(kQRowDw, (W - TX0) * 3 / 4), rows = min(kQTY, H - TY0);
    uint32_t* out = reinterpret_cast<uint32_t*>(dst + (((size_t)n * H + TY0) * W + TX0) * 3);
    const size_t out_pitch = (size_t)W * 3 / 4;
    for (int i = tid; i < kQTY * kQRowDw; i += 256) {
        const int rr = i / kQRowDw, c = i - rr * kQRowDw;
        if (rr < rows && c < row_dw) out[rr * out_pitch + c] = tile[rr * kQPitch + c];
    }
}

// packed_collect_kernel (cf_views.hip) with the turn.  ROT: 1 = 90, 2 = 180, 3 = 270; p.h x p.w is the STORED frame, the sources of the
// placements are rectangles of its upright view of hu x wu.
template <int ROT>
__global__ void __launch_bounds__(1024) packed_collect_rot_kernel(ViewMergeParams p, PackDev t) {
    __shared__ uint32_t wave_cnt[16];
    __shared__ int truncated;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = t.fr_off[f], items = (t.fr_off[f + 1] - q0) * p.rows;
    const int hu = (ROT & 1) ? p.w : p.h, wu = (ROT & 1) ? p.h : p.w;
    float* cand = p.cand + (size_t)f * p.V * p.rows * 16;
    if (tid == 0) truncated = 0;
    __syncthreads();
    uint32_t base = 0;
    for (int j0 = 0; j0 < items; j0 += 1024) {
        const int j = j0 + tid;
        bool keep = false;
        int img = 0, row = 0;
        float c[4] = {0.f, 0.f, 0.f, 0.f};
        cf_view r = {0, 0, 2, 2, 0, 0, 1, 1};
        if (j < items) {
            const int q = j / p.rows;
            row = j - q * p.rows;
            const cf_place& pl = t.places[t.fr_idx[q0 + q]];
            img = pl.canvas;
            const int n = p.counts[img];
            if (row == 0 && n > p.rows) truncated = 1;                    // (every writer stores the same value)
            if (row < min(n, p.rows)) {
                r = pl.view;
                const float4 b4 = *reinterpret_cast<const float4*>(p.dets_net + ((size_t)img * p.rows + row) * 4);
                c[0] = b4.x; c[1] = b4.y; c[2] = b4.z; c[3] = b4.w;
                keep = isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(c[3]);
                const float xlo = (float)r.dx, xhi = (float)(r.dx + r.dw), ylo = (float)r.dy, yhi = (float)(r.dy + r.dh);
                const float cx = (c[0] + c[2]) * 0.5f, cy = (c[1] + c[3]) * 0.5f;
                if (!(cx >= xlo && cx < xhi && cy >= ylo && cy < yhi)) keep = false;
                if (r.sx0 > 0 && c[0] < xlo + p.edge) keep = false;       // interior to the UPRIGHT view
                if (r.sx0 + r.sw < wu && c[2] > xhi - p.edge) keep = false;
                if (r.sy0 > 0 && c[1] < ylo + p.edge) keep = false;
                if (r.sy0 + r.sh < hu && c[3] > yhi - p.edge) keep = false;
            }
        }
        const unsigned long long bal = __ballot(keep);
        __syncthreads();                                                  // the counts of the round before have been read
        if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = 0, total = 0;
        for (int w2 = 0; w2 < 16; ++w2) { if (w2 < wave) off += wave_cnt[w2]; total += wave_cnt[w2]; }
        if (keep) {
            const uint32_t pos = base + off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            const size_t src = (size_t)img * p.rows + row;
            const double sx = (double)r.sw / (double)r.dw, sy = (double)r.sh / (double)r.dh;
            const double dx = (double)r.dx, dy = (double)r.dy, ox = (double)r.sx0, oy = (double)r.sy0;
            // a point of the canvas -> the stored frame: the upright view's pixel first, then the index map of the turn; the difference is
            // taken in float64 and rounded once
            auto turn = [&](float x, float y, float& X, float& Y) {
                const double ux = ((double)x - dx) * sx + ox, uy = ((double)y - dy) * sy + oy;
                if constexpr (ROT == 1) { X = (float)uy; Y = (float)((double)(p.h - 1) - ux); }
                else if constexpr (ROT == 2) { X = (float)((double)(p.w - 1) - ux); Y = (float)((double)(p.h - 1) - uy); }
                else { X = (float)((double)(p.w - 1) - uy); Y = (float)ux; }
            };
            float o[16];
            if constexpr (ROT == 2) {                    // the box is an assignment of mapped corners, never a min / max
                turn(c[2], c[3], o[0], o[1]); turn(c[0], c[1], o[2], o[3]);
            } else if constexpr (ROT == 1) {
                turn(c[2], c[1], o[0], o[1]); turn(c[0], c[3], o[2], o[3]);
            } else {
                turn(c[0], c[3], o[0], o[1]); turn(c[2], c[1], o[2], o[3]);
            }
            o[4] = p.scores[src * p.score_stride];
            const float* l = p.lms_net + src * 10;
#pragma unroll
            for (int k = 0; k < 5; ++k) turn(l[2 * k], l[2 * k + 1], o[5 + 2 * k], o[6 + 2 * k]);      // point by point, order kept
            o[15] = 0.0f;
            float4* d = reinterpret_cast<float4*>(cand + (size_t)pos * 16);
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        }
        base += total;
    }
    __syncthreads();
    if (tid == 0) { p.cand_count[f] = (int)base; p.flags[f] = truncated; }
}

template <int ROT>
void launch_quarter(hipStream_t s, int format, dim3 grid, const PackDev& t, uint8_t* dst, uint32_t fv, int h, int w, int pitch0, int pitch1, int H, int W,
                    int tiles_x) {
    switch (format) {
        case CF_YUV_NV12: hipLaunchKernelGGL((cut_packed_quarter_kernel<1, false, ROT>), grid, dim3(256), 0, s, t, dst, fv, h, w, pitch0, pitch1, H, W, tiles_x); break;
        case CF_YUV_NV21: hipLaunchKernelGGL((cut_packed_quarter_kernel<1, true, ROT>), grid, dim3(256), 0, s, t, dst, fv, h, w, pitch0, pitch1, H, W, tiles_x); break;
        case CF_YUV_I420: case CF_YUV_YV12: hipLaunchKernelGGL((cut_packed_quarter_kernel<2, false, ROT>), grid, dim3(256), 0, s, t, dst, fv, h, w, pitch0, pitch1, H, W, tiles_x); break;
        default: hipLaunchKernelGGL((cut_packed_quarter_kernel<0, false, ROT>), grid, dim3(256), 0, s, t, dst, fv, h, w, pitch0, pitch1, H, W, tiles_x); break;
    }
}

}  // namespace

const char* pack_rot_check(std::string& why, int rot, int h, int w, const cf_place* places, int P, int N, int Bf, int H, int W) {
    char b[160];
    if (rot != 0 && rot != 90 && rot != 180 && rot != 270) {
        snprintf(b, sizeof b, "rot=%d must be 0, 90, 180 or 270 (clockwise degrees)", rot);
        why = b;
        return why.c_str();
    }
    const bool quarter = rot == 90 || rot == 270;
    if (!pack_check(why, quarter ? w : h, quarter ? h : w, places, P, N, Bf, H, W)) return nullptr;
    if (quarter) {
        snprintf(b, sizeof b, " -- rot=%d: the sources are rectangles of the UPRIGHT view, %d x %d, of the stored %d x %d frame", rot, h, w, w, h);
        why += b;
    }
    return why.c_str();
}

hipError_t launch_cut_packed_rot(hipStream_t s, int rot, int format, const PackDev& t, int N, int h, int w, int pitch0, int pitch1, const uint8_t* fill,
                                 uint8_t* dst, int H, int W) {
    if (rot == 0) return launch_cut_packed(s, format, t, N, pitch0, pitch1, fill, dst, H, W);
    if ((rot != 90 && rot != 180 && rot != 270) || format < CF_YUV_NV12 || format > CF_FRAME_BGR || !t.places || !t.cv_off || !t.planes || !fill || !dst ||
        N < 1 || N > 65535 || H < 1 || W < 4 || (W & 3) || h < 2 || w < 2 || ((h | w) & 1))
        return hipErrorInvalidValue;
    const uint32_t fv = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
    if (rot == 180) {
        const int tiles_x = (W + kPackTileW - 1) / kPackTileW, tiles_y = (H + kPackTileH - 1) / kPackTileH;
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)N);
        switch (format) {
            case CF_YUV_NV12: hipLaunchKernelGGL((cut_packed_half_kernel<1, false>), grid, dim3(256), 0, s, t, dst, fv, h, w, pitch0, pitch1, H, W, tiles_x); break;
            case CF_YUV_NV21: hipLaunchKernelGGL((cut_packed_half_kernel<1, true>), grid, dim3(256), 0, s, t, dst, fv, h, w, pitch0, pitch1, H, W, tiles_x); break;
            case CF_YUV_I420: case CF_YUV_YV12: hipLaunchKernelGGL((cut_packed_half_kernel<2, false>), grid, dim3(256), 0, s, t, dst, fv, h, w, pitch0, pitch1, H, W, tiles_x); break;
            default: hipLaunchKernelGGL((cut_packed_half_kernel<0, false>), grid, dim3(256), 0, s, t, dst, fv, h, w, pitch0, pitch1, H, W, tiles_x); break;
        }
    } else {
        const int tiles_x = (W + kQTX - 1) / kQTX, tiles_y = (H + kQTY - 1) / kQTY;
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)N);
        if (rot == 90) launch_quarter<1>(s, format, grid, t, dst, fv, h, w, pitch0, pitch1, H, W, tiles_x);
        else launch_quarter<3>(s, format, grid, t, dst, fv, h, w, pitch0, pitch1, H, W, tiles_x);
    }
    return hipGetLastError();
}

hipError_t launch_merge_packed_rot(hipStream_t s, int rot, const ViewMergeParams& p, const PackDev& t) {
    if (rot == 0) return launch_merge_packed(s, p, t);
    if ((rot != 90 && rot != 180 && rot != 270) || p.Bf < 1 || p.V < 1 || p.rows < 1 || p.max_out < 1 || (long long)p.V * p.rows > INT_MAX / 16 || p.h < 1 ||
        p.w < 1 || p.score_stride < 1 || (p.metric != CF_MERGE_IOU && p.metric != CF_MERGE_IOS) || !t.places || !t.fr_off || !t.fr_idx || !p.dets_net ||
        !p.scores || !p.lms_net || !p.counts || !p.cand || !p.cand_count || !p.order || !p.mask || !p.dets || !p.lms || !p.corners || !p.out_counts || !p.flags)
        return hipErrorInvalidValue;
    if (rot == 90) hipLaunchKernelGGL(packed_collect_rot_kernel<1>, dim3(p.Bf), dim3(1024), 0, s, p, t);
    else if (rot == 180) hipLaunchKernelGGL(packed_collect_rot_kernel<2>, dim3(p.Bf), dim3(1024), 0, s, p, t);
    else hipLaunchKernelGGL(packed_collect_rot_kernel<3>, dim3(p.Bf), dim3(1024), 0, s, p, t);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ThreshParams q{};
    q.B = p.Bf; q.cap = p.V * p.rows; q.nms_thresh = p.thresh; q.metric = p.metric;
    q.cand = p.cand; q.cand_count = p.cand_count; q.order = p.order; q.mask = p.mask;
    q.max_out = p.max_out; q.dets = p.dets; q.lms = p.lms; q.dets_net = p.corners; q.counts = p.out_counts;
    return launch_nms_stages(s, q);
}

}  // namespace cf
