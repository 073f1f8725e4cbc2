// The pixel vocabulary of the cutters (cf_tiles.hip, cf_fit.hip, cf_rot.hip, cf_views.hip, cf_views_rot.hip): one source tap, one
// bilinear pixel, one pack of a pixel and of four pixels, the column set-up and the lane of the padded canvases, the write-out of
// the quarter-turn tiles, the placement list of the packed canvases, and the host's switch over the frame format.  The files that
// include it are built with -ffp-contract=off (cf_cvresize.h's coordinate arithmetic).
#pragma once
#include "cf_kernels.h"
#include "cf_cvresize.h"
#include "cf_yuvmath.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace cf {

// One stored frame: BGR rows (p0) or 4:2:0 planes, pitched, h x w as STORED (read by the turned taps only).
struct SrcPlanes { const uint8_t *p0, *p1, *p2; int pitch0, pitch1, h, w; };

// The pixel U[yu][xu] of the upright view, read from the stored frame and converted there -> B | G << 8 | R << 16.
// SRC: 0 = BGR rows, 1 = one interleaved chroma plane (NV12 / NV21), 2 = two chroma planes (I420; YV12 on a swapped table);
// VF: V first in the interleaved pairs (NV21); ROT: 0 = as stored, 1 = 90, 2 = 180, 3 = 270 (clockwise, the index maps of cf_rot.hip)
template <int SRC, bool VF, int ROT = 0>
__device__ __forceinline__ uint32_t src_tap(const SrcPlanes& s, int yu, int xu) {
    const int y = ROT == 0 ? yu : ROT == 1 ? s.h - 1 - xu : ROT == 2 ? s.h - 1 - yu : xu;
    const int x = ROT == 0 ? xu : ROT == 1 ? yu : ROT == 2 ? s.w - 1 - xu : s.w - 1 - yu;
    if constexpr (SRC == 0) {
        const uint8_t* q = s.p0 + (size_t)y * s.pitch0 + 3 * x;
        return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    } else {
        return yuv_px(s.p0[(size_t)y * s.pitch0 + x], chroma_at<SRC == 1, VF>(s.p1, s.p2, s.pitch1, y >> 1, x >> 1));
    }
}

// Three values 0..255 -> B | G << 8 | R << 16 by byte selection from whole dwords (two v_perm_b32).  Written as shifts and ORs, the
// clamp of cv_linear_vpass next to the packing is selected as gfx950's v_ashr_pk_u8_i32, whose result came back from the device with
// foreign bits above bit 15 in the fit kernel (they reach R and the next pixel's B); a byte selection takes bits 7:0 of each value and
// nothing else.
__device__ __forceinline__ uint32_t pack_bgr(uint32_t b, uint32_t g, uint32_t r) {
    const uint32_t bg = __builtin_amdgcn_perm(g, b, 0x0c0c0400u);       // byte 0 = b[7:0], byte 1 = g[7:0], bytes 2, 3 = 0
    return __builtin_amdgcn_perm(r, bg, 0x0c040100u);                   // bytes 0, 1 = bg[15:0], byte 2 = r[7:0], byte 3 = 0
}

// one output pixel from its four taps: the horizontal pass in the upright view first, then the vertical one (cf_cvresize.h)
template <int SRC, bool VF, int ROT = 0>
__device__ __forceinline__ uint32_t bilinear_px(const SrcPlanes& s, int y0, int y1, int b0, int b1, int x0, int x1, int a0, int a1) {
    const uint32_t t00 = src_tap<SRC, VF, ROT>(s, y0, x0);
    const uint32_t t01 = src_tap<SRC, VF, ROT>(s, y0, x1);
    const uint32_t t10 = src_tap<SRC, VF, ROT>(s, y1, x0);
    const uint32_t t11 = src_tap<SRC, VF, ROT>(s, y1, x1);
    uint32_t ch[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int sh = 8 * c;
        const int h0 = (int)((t00 >> sh) & 255) * a0 + (int)((t01 >> sh) & 255) * a1;
        const int h1 = (int)((t10 >> sh) & 255) * a0 + (int)((t11 >> sh) & 255) * a1;
        ch[c] = (uint32_t)cv_linear_vpass(b0, b1, h0, h1);
    }
    return pack_bgr(ch[0], ch[1], ch[2]);
}

// four adjacent pixels -> the three dwords of their twelve bytes
__device__ __forceinline__ void quad_pack(const uint32_t (&p)[4], uint32_t (&o)[3]) {
    o[0] = p[0] | (p[1] << 24);
    o[1] = (p[1] >> 8) | (p[2] << 16);
    o[2] = (p[2] >> 16) | (p[3] << 8);
}

__device__ __forceinline__ void quad_store(uint8_t* row, const uint32_t (&p)[4]) {
    uint32_t o[3];
    quad_pack(p, o);
    uint32_t* d = reinterpret_cast<uint32_t*>(row);
    d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
}

// The canvas columns X .. X + 3 against the content of view r: in[k] = the column is content; its taps (columns of the upright view)
// and coefficients.  A padding column beside content gets the edge column's taps, which the caller drops.
__device__ __forceinline__ void col_coeffs(const cf_view& r, int X, bool (&in)[4], int (&x0)[4], int (&x1)[4], int (&a0)[4], int (&a1)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = X + k - r.dx;
        in[k] = x >= 0 && x < r.dw;
        cv_linear_coeffs(min(max(x, 0), r.dw - 1), r.sw, r.dw, true, x0[k], x1[k], a0[k], a1[k]);
        x0[k] += r.sx0; x1[k] += r.sx0;
    }
}

// The lane of a padded canvas: columns X0 .. X0 + 3 of the rows [Y0, Yend) of the canvas at `canvas` (W columns) = the content of view
// r, `fill` elsewhere; each row leaves as three dword stores.  Rows wholly in the padding, and lanes whose four columns are, are
// written as fill without touching the source.
template <int SRC, bool VF, int ROT>
__device__ __forceinline__ void padded_lane(const cf_view& r, const SrcPlanes& s, uint8_t* canvas, int W, int X0, int Y0, int Yend, uint32_t fill) {
    uint8_t* out = canvas + (size_t)X0 * 3;
    bool in[4];
    int x0[4], x1[4], a0[4], a1[4];
    col_coeffs(r, X0, in, x0, x1, a0, a1);
    const uint32_t pad[4] = {fill, fill, fill, fill};
    if (!(in[0] || in[1] || in[2] || in[3]) || Yend <= r.dy || Y0 >= r.dy + r.dh) {
        for (int Y = Y0; Y < Yend; ++Y) quad_store(out + (size_t)Y * W * 3, pad);
        return;
    }
    for (int Y = Y0; Y < Yend; ++Y) {
        uint32_t p[4] = {fill, fill, fill, fill};
        const int y = Y - r.dy;
        if (y >= 0 && y < r.dh) {
            int y0, y1, b0, b1;
            cv_linear_coeffs(y, r.sh, r.dh, false, y0, y1, b0, b1);
            y0 += r.sy0; y1 += r.sy0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t v = bilinear_px<SRC, VF, ROT>(s, y0, y1, b0, b1, x0[k], x1[k], a0[k], a1[k]);
                if (in[k]) p[k] = v;
            }
        }
        quad_store(out + (size_t)Y * W * 3, p);
    }
}

// The quarter-turn cutters (rot_quarter_kernel, cut_packed_quarter_kernel): a workgroup owns a canvas tile of kQTY rows x kQTX columns,
// a wave's lanes run along its rows; the pixels go through an LDS tile whose row pitch of 25 dwords is odd, so the 32 lanes of a write
// group hit 32 banks.
constexpr int kQTY = 64, kQTX = 32;
constexpr int kQRowDw = kQTX * 3 / 4;                // 24 dwords of pixels per tile row ...
constexpr int kQPitch = kQRowDw + 1;                 // ... at an odd pitch

// the LDS tile's rows out to the canvas at `canvas` (H x W), dword by dword: W % 4 == 0, so a row of the canvas ends on a dword of the
// tile row
__device__ __forceinline__ void tile_rows_out(const uint32_t* tile, uint8_t* canvas, int H, int W, int TX0, int TY0) {
    const int row_dw = min(kQRowDw, (W - TX0) * 3 / 4), rows = min(kQTY, H - TY0);
    uint32_t* out = reinterpret_cast<uint32_t*>(canvas + ((size_t)TY0 * W + TX0) * 3);
    const size_t out_pitch = (size_t)W * 3 / 4;
    for (int i = (int)threadIdx.x; i < kQTY * kQRowDw; i += 256) {
        const int r = i / kQRowDw, c = i - r * kQRowDw;
        if (r < rows && c < row_dw) out[r * out_pitch + c] = tile[r * kQPitch + c];
    }
}

// One round of the placement list of a tile [tx0, tx0 + tw) x [ty0, ty0 + th) of a packed canvas (256 threads): thread tid tests
// placement base + tid < k1, the hits go to s_list in placement order (ballot, the four wave counts through LDS: a prefix sum).  Returns
// their number (uniform); the caller synchronises before the next round.
constexpr int kPackList = 256;                       // placements per list round: one per thread
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

// fn(SRC, VF) with the std::integral_constants of the frame format's tap (YV12: the I420 tap on a swapped plane table)
template <class F>
inline void with_format(int format, F&& fn) {
    switch (format) {
        case CF_YUV_NV12: fn(std::integral_constant<int, 1>{}, std::false_type{}); break;
        case CF_YUV_NV21: fn(std::integral_constant<int, 1>{}, std::true_type{}); break;
        case CF_YUV_I420: case CF_YUV_YV12: fn(std::integral_constant<int, 2>{}, std::false_type{}); break;
        default: fn(std::integral_constant<int, 0>{}, std::false_type{}); break;
    }
}

}  // namespace cf
