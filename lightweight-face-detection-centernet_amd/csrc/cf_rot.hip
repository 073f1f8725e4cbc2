// Rotated sources: the network's canvases from the UPRIGHT view of frames that are stored a quarter, a half or three quarters of a turn
// away from it (corridor-mode cameras; phone video whose turn lives in the container's display matrix while the decoder hands out the
// surface as stored).  The statement is in include/centerface_hip.h (cf_forward_rot); in short, for a stored frame F of h x w and
// rot = the clockwise turn that makes it upright, the upright view U of hu x wu is
//   rot  90: (w, h)  U[y][x] = F[h-1-x][y]         rot 180: (h, w)  U[y][x] = F[h-1-y][w-1-x]         rot 270: (w, h)  U[y][x] = F[x][w-1-y]
// and canvas_b = what cf_fit.hip makes of bgr(U_b) with the geometry g of (hu, wu) in (H, W) -- or, stretched, g = {W, H, 0, 0}: the
// resize of cf_forward_resized.  bgr() is taken per STORED pixel (a 4:2:0 pixel's chroma is that of its own 2 x 2 block in F), so the
// kernels read F through the index map and never build U.  The rows come back through unfit_rows_kernel<ROT> (cf_fit.hip).
//
// rot 0 is launch_fit_frames: the same code, the same bytes.  rot 180 keeps that kernel's lane layout -- a lane owns four adjacent canvas
// columns whose taps lie in one source row, mirrored -- because adjacent canvas columns are still adjacent source columns.
//
// rot 90 / 270 is where the layout matters: adjacent canvas COLUMNS are adjacent source ROWS, so with the fit's layout every tap of a wave
// would be a cache line of its own.  Here the transpose happens on the output side, whose footprint does not depend on the scale: a
// workgroup owns a canvas tile of kRotTY rows x kRotTX columns; a wave's 64 lanes run along the canvas ROWS of the tile, so for one canvas
// column their taps run along ONE source row (two: the bilinear pair) and coalesce; a lane's row coefficients are computed once, the
// tile's column coefficients once per workgroup (LDS); the pixels go into an LDS tile whose row pitch of 25 dwords is odd, so the 32 lanes
// of a write group hit 32 banks; the tile leaves as whole-row dword stores, 96 contiguous bytes per canvas row.  Padding rows and columns
// are written as fill without touching the source; every tap lies inside the frame, pitch padding is never read.
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_cvresize.h"
#include "cf_yuvmath.h"
#include "cf_fitpx.h"
#include <string>

namespace cf {
namespace {

constexpr int kRotFrames = 64;                       // frames per launch, as the fit's
constexpr int kRotRows = 4;                          // rot 180: canvas rows per lane, as kFitRows
constexpr int kRotTY = 64, kRotTX = 32;              // rot 90 / 270: the canvas tile of a workgroup (rows = the lanes of a wave)
constexpr int kRotRowDw = kRotTX * 3 / 4;            // 24 dwords of pixels per tile row ...
constexpr int kRotPitch = kRotRowDw + 1;             // ... at an odd pitch
using RotPtrs = FramePtrs<kRotFrames>;

// The pixel U[yu][xu] of the upright view, read from the stored frame at (y, x) and converted there -> B | G << 8 | R << 16.
// SRC: 0 = BGR rows, 1 = one interleaved chroma plane (NV12 / NV21), 2 = two chroma planes (I420; YV12 on a swapped table);
// VF: V first in the interleaved pairs (NV21); ROT: 1 = 90, 2 = 180, 3 = 270
template <int SRC, bool VF, int ROT>
__device__ __forceinline__ uint32_t rot_tap(const uint8_t* p0, const uint8_t* p1, const uint8_t* p2, int pitch0, int pitch1, int h, int w, int yu, int xu) {
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
__device__ __forceinline__ uint32_t rot_pixel(const uint8_t* p0, const uint8_t* p1, const uint8_t* p2, int pitch0, int pitch1, int h, int w,
                                              int y0, int y1, int b0, int b1, int x0, int x1, int a0, int a1) {
    const uint32_t t00 = rot_tap<SRC, VF, ROT>(p0, p1, p2, pitch0, pitch1, h, w, y0, x0);
    const uint32_t t01 = rot_tap<SRC, VF, ROT>(p0, p1, p2, pitch0, pitch1, h, w, y0, x1);
    const uint32_t t10 = rot_tap<SRC, VF, ROT>(p0, p1, p2, pitch0, pitch1, h, w, y1, x0);
    const uint32_t t11 = rot_tap<SRC, VF, ROT>(p0, p1, p2, pitch0, pitch1, h, w, y1, x1);
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

// rot 180: fit_frames_kernel with mirrored taps (hu = h, wu = w)
template <int SRC, bool VF>
__global__ void __launch_bounds__(256) rot_half_kernel(RotPtrs tab, uint8_t* dst, cf_fit_geom g, uint32_t fill, int h, int w, int pitch0,
                                                       int pitch1, int H, int W) {
    const int f = blockIdx.y;
    const int gw = W >> 2, ng = (H + kRotRows - 1) / kRotRows;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ng * gw) return;
    const int grp = i / gw, X0 = (i - grp * gw) << 2;
    uint8_t* out = dst + ((size_t)f * H * W + X0) * 3;
    const int Y0 = grp * kRotRows, Yend = min(H, Y0 + kRotRows);
    const uint32_t pad[4] = {fill, fill, fill, fill};
    bool in[4];
    int x0[4], x1[4], a0[4], a1[4];
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = X0 + k - g.dx;
        in[k] = x >= 0 && x < g.rw;
        cv_linear_coeffs(min(max(x, 0), g.rw - 1), w, g.rw, true, x0[k], x1[k], a0[k], a1[k]);
        any = any || in[k];
    }
    if (!any || Yend <= g.dy || Y0 >= g.dy + g.rh) {
        for (int Y = Y0; Y < Yend; ++Y) fit_store(out + (size_t)Y * W * 3, pad);
        return;
    }
    const uint8_t* p0 = tab.p0[f];
    const uint8_t* p1 = tab.p1[f];
    const uint8_t* p2 = tab.p2[f];
    for (int Y = Y0; Y < Yend; ++Y) {
        const int y = Y - g.dy;
        if (y < 0 || y >= g.rh) { fit_store(out + (size_t)Y * W * 3, pad); continue; }
        int y0, y1, b0, b1;
        cv_linear_coeffs(y, h, g.rh, false, y0, y1, b0, b1);
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t v = rot_pixel<SRC, VF, 2>(p0, p1, p2, pitch0, pitch1, h, w, y0, y1, b0, b1, x0[k], x1[k], a0[k], a1[k]);
            p[k] = in[k] ? v : fill;
        }
        fit_store(out + (size_t)Y * W * 3, p);
    }
}

// rot 90 (ROT 1) / 270 (ROT 3): grid (W tiles, H tiles, frames); thread = (wave, lane): lane -> the tile's canvas row, wave -> eight of
// its columns as two groups of four (three dwords each, as fit_store packs them)
template <int SRC, bool VF, int ROT>
__global__ void __launch_bounds__(256) rot_quarter_kernel(RotPtrs tab, uint8_t* dst, cf_fit_geom g, uint32_t fill, int h, int w, int pitch0,
                                                          int pitch1, int H, int W) {
    __shared__ uint32_t tile[kRotTY * kRotPitch];
    __shared__ int4 colc[kRotTX];
    const int f = blockIdx.z, TX0 = blockIdx.x * kRotTX, TY0 = blockIdx.y * kRotTY;
    const int tid = threadIdx.x, ly = tid & 63, wave = tid >> 6;
    const int hu = w, wu = h;
    // (uniform) the tile lies wholly in the padding: no coefficients, no source
    const bool content = TX0 < g.dx + g.rw && TX0 + kRotTX > g.dx && TY0 < g.dy + g.rh && TY0 + kRotTY > g.dy;
    if (content && tid < kRotTX) {
        int x0, x1, a0, a1;
        cv_linear_coeffs(min(max(TX0 + tid - g.dx, 0), g.rw - 1), wu, g.rw, true, x0, x1, a0, a1);
        colc[tid] = make_int4(x0, x1, a0, a1);
    }
    __syncthreads();
    const int y = TY0 + ly - g.dy;
    const bool row_in = content && TY0 + ly < H && y >= 0 && y < g.rh;
    int y0 = 0, y1 = 0, b0 = 0, b1 = 0;
    if (row_in) cv_linear_coeffs(y, hu, g.rh, false, y0, y1, b0, b1);
    const uint8_t* p0 = tab.p0[f];
    const uint8_t* p1 = tab.p1[f];
    const uint8_t* p2 = tab.p2[f];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cg = wave * 2 + j;                      // the column group: canvas columns TX0 + 4 cg .. + 3
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = TX0 + cg * 4 + k - g.dx;        // (uniform over the wave)
            p[k] = fill;
            if (row_in && x >= 0 && x < g.rw) {
                const int4 c = colc[cg * 4 + k];
                p[k] = rot_pixel<SRC, VF, ROT>(p0, p1, p2, pitch0, pitch1, h, w, y0, y1, b0, b1, c.x, c.y, c.z, c.w);
            }
        }
        uint32_t* o = tile + ly * kRotPitch + cg * 3;
        o[0] = p[0] | (p[1] << 24);
        o[1] = (p[1] >> 8) | (p[2] << 16);
        o[2] = (p[2] >> 16) | (p[3] << 8);
    }
    __syncthreads();
    // the tile's rows out, dword by dword: W % 4 == 0, so a row of the canvas ends on a dword of the tile row
    const int row_dw = min(kRotRowDw, (W - TX0) * 3 / 4), rows = min(kRotTY, H - TY0);
    uint32_t* out = reinterpret_cast<uint32_t*>(dst + (((size_t)f * H + TY0) * W + TX0) * 3);
    const size_t out_pitch = (size_t)W * 3 / 4;
    for (int i = tid; i < kRotTY * kRotRowDw; i += 256) {
        const int r = i / kRotRowDw, c = i - r * kRotRowDw;
        if (r < rows && c < row_dw) out[r * out_pitch + c] = tile[r * kRotPitch + c];
    }
}

template <int ROT>
void launch_quarter(hipStream_t s, int format, dim3 grid, const RotPtrs& tab, uint8_t* out, const cf_fit_geom& g, uint32_t fv, int h, int w,
                    int pitch0, int pitch1, int H, int W) {
    switch (format) {
        case CF_YUV_NV12: hipLaunchKernelGGL((rot_quarter_kernel<1, false, ROT>), grid, dim3(256), 0, s, tab, out, g, fv, h, w, pitch0, pitch1, H, W); break;
        case CF_YUV_NV21: hipLaunchKernelGGL((rot_quarter_kernel<1, true, ROT>), grid, dim3(256), 0, s, tab, out, g, fv, h, w, pitch0, pitch1, H, W); break;
        case CF_YUV_I420: case CF_YUV_YV12: hipLaunchKernelGGL((rot_quarter_kernel<2, false, ROT>), grid, dim3(256), 0, s, tab, out, g, fv, h, w, pitch0, pitch1, H, W); break;
        default: hipLaunchKernelGGL((rot_quarter_kernel<0, false, ROT>), grid, dim3(256), 0, s, tab, out, g, fv, h, w, pitch0, pitch1, H, W); break;
    }
}

}  // namespace

const char* rot_check(std::string& why, const cf_rot_opts* o, int format, int B, int h, int w, int pitch0, int pitch1, int H, int W) {
    char b[160];
    auto say = [&](const char* s) { why = s; return why.c_str(); };
    if (!o) return say("null options");
    if (o->rot != 0 && o->rot != 90 && o->rot != 180 && o->rot != 270) { snprintf(b, sizeof b, "rot=%d must be 0, 90, 180 or 270 (clockwise degrees)", o->rot); return say(b); }
    if (o->stretch != 0 && o->stretch != 1) { snprintf(b, sizeof b, "stretch=%d must be 0 or 1", o->stretch); return say(b); }
    return fit_check(why, &o->fit, format, B, h, w, pitch0, pitch1, H, W);
}

int rot_geometry(const cf_rot_opts* o, int h, int w, int H, int W, cf_fit_geom* g) {
    if (!o || !g || h < 1 || w < 1 || H < 1 || W < 1) return CF_EINVAL;
    const bool quarter = o->rot == 90 || o->rot == 270;
    if (o->stretch) { *g = cf_fit_geom{W, H, 0, 0}; return CF_OK; }
    return fit_geometry(o->fit.anchor, o->fit.upscale, quarter ? w : h, quarter ? h : w, H, W, g);
}

// planes: B x {p0, p1, p2} device addresses (HOST table); the caller has run rot_check and rot_geometry
hipError_t launch_rot_frames(hipStream_t s, int rot, int format, const void* const* planes, int B, int h, int w, int pitch0, int pitch1,
                             const cf_fit_geom& g, const uint8_t* fill, uint8_t* dst, int H, int W) {
    if (rot == 0) return launch_fit_frames(s, format, planes, B, h, w, pitch0, pitch1, g, fill, dst, H, W);
    if ((rot != 90 && rot != 180 && rot != 270) || format < CF_YUV_NV12 || format > CF_FRAME_BGR || !planes || !dst || !fill || B < 1 || H < 1 || W < 4 ||
        (W & 3) || h < 1 || w < 1 || g.rw < 1 || g.rh < 1 || g.dx < 0 || g.dy < 0 || g.dx > W - g.rw || g.dy > H - g.rh)
        return hipErrorInvalidValue;
    const uint32_t fv = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
    const long long n = (long long)((H + kRotRows - 1) / kRotRows) * (W >> 2);
    for (int f0 = 0; f0 < B; f0 += kRotFrames) {
        const int nb = B - f0 < kRotFrames ? B - f0 : kRotFrames;
        const RotPtrs tab = frame_ptrs<kRotFrames>(planes, format, f0, nb, true);      // YV12: the I420 kernel on swapped planes
        uint8_t* out = dst + (size_t)f0 * H * W * 3;
        if (rot == 180) {
            const dim3 grid((unsigned)((n + 255) / 256), (unsigned)nb);
            switch (format) {
                case CF_YUV_NV12: hipLaunchKernelGGL((rot_half_kernel<1, false>), grid, dim3(256), 0, s, tab, out, g, fv, h, w, pitch0, pitch1, H, W); break;
                case CF_YUV_NV21: hipLaunchKernelGGL((rot_half_kernel<1, true>), grid, dim3(256), 0, s, tab, out, g, fv, h, w, pitch0, pitch1, H, W); break;
                case CF_YUV_I420: case CF_YUV_YV12: hipLaunchKernelGGL((rot_half_kernel<2, false>), grid, dim3(256), 0, s, tab, out, g, fv, h, w, pitch0, pitch1, H, W); break;
                default: hipLaunchKernelGGL((rot_half_kernel<0, false>), grid, dim3(256), 0, s, tab, out, g, fv, h, w, pitch0, pitch1, H, W); break;
            }
        } else {
            const dim3 grid((unsigned)((W + kRotTX - 1) / kRotTX), (unsigned)((H + kRotTY - 1) / kRotTY), (unsigned)nb);
            if (rot == 90) launch_quarter<1>(s, format, grid, tab, out, g, fv, h, w, pitch0, pitch1, H, W);
            else launch_quarter<3>(s, format, grid, tab, out, g, fv, h, w, pitch0, pitch1, H, W);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace cf
