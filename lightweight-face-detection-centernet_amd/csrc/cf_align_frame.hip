// Aligned face chips cut from the SOURCE frame (cf_align_faces_frame, cf_op_align_frame): the read-side twin of cf_redact.hip.  The
// faces are those of cf_align.hip -- the rows the last threshold decode kept, or the merged rows of a tiled forward -- but the chip is
// sampled from the full-resolution frames the caller names, BGR rows or 4:2:0 planes, pitched, read in place: one launch, nothing
// crosses to the host.
//
// The arithmetic is that of cf_align.hip, unchanged (cf_alignmath.h holds the one statement of it; this file too is compiled with
// -ffp-contract=off), with two additions:
//   * Landmarks.  A row in network coordinates (H x W) is mapped to the frame (h x w) value by value, in float64, and the estimate is
//     fitted to the MAPPED points (the map is anisotropic when h / H != w / W: a network-space fit cannot be scaled afterwards):
//       X = (double)x * ((double)w / (double)W),  Y = (double)y * ((double)h / (double)H)     -- kept as doubles
//     Rows that are in frame pixels already (the merged rows of cf_merge_tiles, cf_op_align_frame) take the factor 1.0, which
//     changes no bit.  The alignable rule (max |linear| * S + max |t| < 2^20) is unchanged: it holds for frames of 8192 a side.
//   * Source pixels.  The pixel at (sy, sx) of a frame is
//       BGR:   the three bytes at p0 + sy * pitch0 + 3 * sx
//       4:2:0: yuv_px(Y[sy][sx], chroma at (sy >> 1, sx >> 1)) of cf_yuvmath.h
//     so a chip equals, bit for bit, the chip cut from the frame converted by cf_forward_yuv's conversion at (H, W) = (h, w).
//     Neighbours outside the h x w frame contribute 0 (per neighbour), as in cf_align.hip.
//
// Loads.  Every load lies inside [plane, plane + rows * pitch) of a plane the caller named; the caller's allocation may end there.
//   BGR: the six bytes of columns cx, cx + 1 (0 <= cx <= w - 2) of a row come from three aligned dwords (fetch_pair); the second and
//   third are clamped to the last dword of THAT FRAME'S plane (h * pitch0 / 4 - 1: address and pitch are multiples of 4).  A dword may
//   hold padding bytes or the next pixel; only the six pixel bytes are extracted, and a clamped dword is never one that holds them.
//   4:2:0: byte loads of samples inside the w x h luma and w/2 x h/2 chroma extents only: padding is not even read.  The two columns
//   share a chroma sample when cx is even, the two rows when r0 >> 1 == r1 >> 1: a shared sample is loaded and converted once.
//
// Point sampling: a face much larger than the chip is sampled without an area filter, as the cv2 recipe this mirrors does.
#include <limits.h>
#include <math.h>

#include "centerface_hip.h"
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_alignmath.h"
#include "cf_yuvmath.h"

namespace cf {
namespace {

constexpr int kAlignFrames = 64;                     // frames per launch: 3 x 64 plane addresses by value = 1.5 KB of kernel arguments
using AlignFramePtrs = FramePtrs<kAlignFrames>;
struct AlignFrameGeo { int f0, nb, h, w, pitch0, pitch1; double sx, sy; };

// SRC: 0 = BGR rows, 1 = one interleaved chroma plane (NV12 / NV21), 2 = two chroma planes (I420; YV12 on a swapped table);
// VF: V first in the interleaved pairs (NV21).  The four neighbours of one tap -> B | G << 8 | R << 16 each.
template <int SRC, bool VF>
__device__ __forceinline__ void frame_fetch(const uint8_t* p0, const uint8_t* p1, const uint8_t* p2, const AlignFrameGeo& g, size_t last0,
                                            const AlignTap& t, uint32_t& a0, uint32_t& a1, uint32_t& c0, uint32_t& c1) {
    if constexpr (SRC == 0) {
        const uint32_t* img = reinterpret_cast<const uint32_t*>(p0);
        fetch_pair(img, (size_t)t.r0 * g.pitch0 + 3 * t.cx, last0, a0, a1);
        fetch_pair(img, (size_t)t.r1 * g.pitch0 + 3 * t.cx, last0, c0, c1);
    } else {
        const uint8_t* y0 = p0 + (size_t)t.r0 * g.pitch0 + t.cx;
        const uint8_t* y1 = p0 + (size_t)t.r1 * g.pitch0 + t.cx;
        const int cr0 = t.r0 >> 1, cr1 = t.r1 >> 1, cc0 = t.cx >> 1, cc1 = (t.cx + 1) >> 1;
        const Chroma k00 = chroma_at<SRC == 1, VF>(p1, p2, g.pitch1, cr0, cc0);
        const Chroma k01 = cc1 != cc0 ? chroma_at<SRC == 1, VF>(p1, p2, g.pitch1, cr0, cc1) : k00;
        const Chroma k10 = cr1 != cr0 ? chroma_at<SRC == 1, VF>(p1, p2, g.pitch1, cr1, cc0) : k00;
        const Chroma k11 = cr1 != cr0 ? (cc1 != cc0 ? chroma_at<SRC == 1, VF>(p1, p2, g.pitch1, cr1, cc1) : k10) : k01;
        a0 = yuv_px(y0[0], k00); a1 = yuv_px(y0[1], k01);
        c0 = yuv_px(y1[0], k10); c1 = yuv_px(y1[1], k11);
    }
}

// One workgroup = one face x one band of chip pixels, as align_chips_kernel.  A launch serves the frames [g.f0, g.f0 + g.nb): every
// workgroup walks all B counts (the face numbering is global), the ones whose face lies in another launch's frames leave.
template <int SRC, bool VF>
__global__ void __launch_bounds__(256) align_frame_kernel(AlignParams p, AlignFrameGeo g, AlignFramePtrs ptrs) {
    __shared__ int tab[4 * kAlignMaxS];                     // ad | bd | X0 | Y0
    const int S = p.S, q4 = S >> 2, items = S * q4;
    const int bands = (items + kAlignItems - 1) / kAlignItems;
    const int n = (int)(blockIdx.x / (unsigned)bands), band = (int)(blockIdx.x - (unsigned)n * bands);
    const int tid = threadIdx.x;
    int b;
    size_t row;
    if (!align_find_face(p, n, b, row)) return;                                // uniform: before any barrier
    if (b < g.f0 || b >= g.f0 + g.nb) return;
    double l[10];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        l[2 * j] = (double)p.lms[row * 10 + 2 * j] * g.sx;
        l[2 * j + 1] = (double)p.lms[row * 10 + 2 * j + 1] * g.sy;
    }
    const Similarity sim = estimate_inverse(l, p.tmpl, S);
    if (band == 0 && tid == 0 && p.mats) {
#pragma unroll
        for (int j = 0; j < 6; ++j) p.mats[(size_t)n * 6 + j] = sim.M[j];
    }
    align_fill_tables(tab, sim, S);
    __syncthreads();
    const uint8_t* p0 = ptrs.p0[b - g.f0];
    const uint8_t* p1 = ptrs.p1[b - g.f0];
    const uint8_t* p2 = ptrs.p2[b - g.f0];
    const size_t last0 = (size_t)g.h * g.pitch0 / 4 - 1;   // last dword of this frame's BGR plane
#pragma unroll 1
    for (int it = 0; it < kAlignItems / 256; ++it) {
        const int item = band * kAlignItems + it * 256 + tid;
        if (item >= items) break;
        const int y = item / q4, x0 = (item - y * q4) << 2;
        const int X0 = tab[2 * kAlignMaxS + y], Y0 = tab[3 * kAlignMaxS + y];
        uint32_t px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const AlignTap t = align_tap((X0 + tab[x0 + k]) >> 5, (Y0 + tab[kAlignMaxS + x0 + k]) >> 5, g.h, g.w, sim.ok);
            uint32_t v = 0;
            if (align_tap_live(t)) {
                uint32_t a0, a1, c0, c1;
                frame_fetch<SRC, VF>(p0, p1, p2, g, last0, t, a0, a1, c0, c1);
                v = align_blend(t, a0, a1, c0, c1);
            }
            px[k] = v;
        }
        align_store4(p, n, y, x0, px);
    }
}

}  // namespace

const char* align_frame_check(AlignFrameParams& p, int size, int chip_format, int rgb, float mean, float scale, const float* tmpl,
                              int max_per_image, int format, const void* const* planes, int on_device, int B, int h, int w, int pitch0, int pitch1) {
    if (const char* why = align_params_set(p.a, size, chip_format, rgb, mean, scale, tmpl, max_per_image)) return why;
    if (const char* why = frame_geometry_check(FrameGeo{format, B, h, w, pitch0, pitch1}, 2, false)) return why;
    if (const char* why = redact_check_planes(format, planes, B, on_device, pitch0, pitch1)) return why;
    p.format = format; p.a.B = B; p.h = h; p.w = w; p.pitch0 = pitch0; p.pitch1 = pitch1;
    return nullptr;
}

hipError_t launch_align_frame(hipStream_t s, const AlignFrameParams& p) {
    const AlignParams& a = p.a;
    if (frame_geometry_check(FrameGeo{p.format, a.B, p.h, p.w, p.pitch0, p.pitch1}, 2, false) ||
        redact_check_planes(p.format, p.planes, a.B, 1, p.pitch0, p.pitch1) || !a.counts || a.cap_faces < 0 ||
        a.S < 16 || a.S > kAlignMaxS || (a.S & 3) || (reinterpret_cast<uintptr_t>(a.chips) & (a.format == 0 ? 3 : 15)) ||
        !(p.sx > 0.0) || !(p.sy > 0.0))
        return hipErrorInvalidValue;
    const long long bands = ((long long)a.S * (a.S >> 2) + kAlignItems - 1) / kAlignItems;
    const long long grid = (long long)(a.cap_faces > 0 ? a.cap_faces : 1) * bands;      // one workgroup at least: it writes the offsets
    if (grid > INT_MAX) return hipErrorInvalidValue;
    for (int f0 = 0; f0 < a.B; f0 += kAlignFrames) {
        AlignFrameGeo g{};
        g.f0 = f0; g.nb = a.B - f0 < kAlignFrames ? a.B - f0 : kAlignFrames;
        g.h = p.h; g.w = p.w; g.pitch0 = p.pitch0; g.pitch1 = p.pitch1; g.sx = p.sx; g.sy = p.sy;
        const AlignFramePtrs tab = frame_ptrs<kAlignFrames>(p.planes, p.format, f0, g.nb, true);      // YV12: the I420 kernel on swapped planes
        AlignParams q = a;
        if (f0 > 0) q.offsets = nullptr;                    // the first launch has written them
        const dim3 gr((unsigned)grid);
        switch (p.format) {
            case CF_YUV_NV12: hipLaunchKernelGGL((align_frame_kernel<1, false>), gr, dim3(256), 0, s, q, g, tab); break;
            case CF_YUV_NV21: hipLaunchKernelGGL((align_frame_kernel<1, true>), gr, dim3(256), 0, s, q, g, tab); break;
            case CF_YUV_I420: case CF_YUV_YV12: hipLaunchKernelGGL((align_frame_kernel<2, false>), gr, dim3(256), 0, s, q, g, tab); break;
            default: hipLaunchKernelGGL((align_frame_kernel<0, false>), gr, dim3(256), 0, s, q, g, tab); break;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace cf
