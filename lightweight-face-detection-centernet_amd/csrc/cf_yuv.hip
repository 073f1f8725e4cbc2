// 4:2:0 video frames -> uint8 BGR HWC on the device: cv2.cvtColor(frame, COLOR_YUV2BGR_<NV12 | NV21 | I420 | YV12>), and for a frame
// of another size than the network's the cv2.resize (centerface.py:30) behind it, in one kernel.
//
// The conversion is OpenCV's fixed-point BT.601 limited-range statement, restated from OpenCV 4.x
// modules/imgproc/src/color_yuv.simd.hpp (the scalar path).  cv2 is not installable where this was built, so -- as for the resize
// (cf_cvresize.h) -- parity is pinned to the published algorithm and to known answers (tests/test_yuv_input.py), NOT to a cv2 binary:
//   uu = U - 128, vv = V - 128, y = max(0, Y - 16) * 1220542
//   B = sat8((y + (1 << 19) + 2116026 * uu) >> 20)
//   G = sat8((y + (1 << 19) - 852492 * vv - 409993 * uu) >> 20)
//   R = sat8((y + (1 << 19) + 1673527 * vv) >> 20)
// Each 2x2 block of luma shares the chroma sample at (y/2, x/2) (no chroma interpolation); >> is an arithmetic shift; the largest
// intermediate stays below 0.6e9 (int32).  A frame of another size is converted at source resolution, then resized (cvtColor followed
// by cv2.resize): the convert+resize kernel converts the four source taps of an output pixel and applies cf_cvresize.h's bilinear step.
//
// Planes (cf_yuv_planes, include/centerface_hip.h): y = h rows of y_pitch bytes; c0 = the first chroma plane in the format's order
// (NV12 / NV21: the interleaved UV / VU plane; I420: U; YV12: V), c1 = the second (I420: V; YV12: U), h/2 rows of c_pitch bytes each.
// Per-frame plane addresses travel by value in a table of kYuvFrames entries per launch (the UploadPtrs pattern of cf_util.hip).
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_cvresize.h"
#include "cf_yuvmath.h"

namespace cf {
namespace {

constexpr int kYuvFrames = 64;                       // frames per launch: 3 x 64 pointers = 1.5 KB of kernel arguments
struct YuvPtrs { const uint8_t* y[kYuvFrames]; const uint8_t* c0[kYuvFrames]; const uint8_t* c1[kYuvFrames]; };

__device__ __forceinline__ uint2 ld8(const uint8_t* p) {             // 8 bytes at a 4-byte aligned address
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    return make_uint2(q[0], q[1]);
}

// Identity size, w % 8 == 0 (every network width): a lane converts a 2 x 8 block -- one chroma row serves both luma rows.  Loads are
// dwords (plane pointers and pitches are multiples of 4), lane-contiguous; the 2 x 24 output bytes go out as 8-byte stores (8-byte
// aligned: w % 8 == 0), lane-contiguous as well.  No LDS: the pass is memory-bound (1.5 bytes in, 3 out per pixel).
template <bool IL, bool VF>
__global__ void __launch_bounds__(256) yuv_bgr_identity8_kernel(YuvPtrs tab, uint8_t* dst, int h, int w, int y_pitch, int c_pitch) {
    const int f = blockIdx.y;
    const int gw = w >> 3;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (h >> 1) * gw) return;
    const int cy = i / gw, x = (i - cy * gw) << 3;
    const uint8_t* yp = tab.y[f] + (size_t)(2 * cy) * y_pitch + x;
    const uint2 yr[2] = {ld8(yp), ld8(yp + y_pitch)};
    Chroma ch[4];
    if (IL) {
        const uint2 c = ld8(tab.c0[f] + (size_t)cy * c_pitch + x);    // 4 (first, second) pairs
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t d = (k < 2 ? c.x : c.y) >> (16 * (k & 1));
            const int a = d & 255, b = (d >> 8) & 255;
            ch[k] = VF ? chroma_terms(b, a) : chroma_terms(a, b);
        }
    } else {
        const size_t o = (size_t)cy * c_pitch + (x >> 1);
        const uint32_t ca = *reinterpret_cast<const uint32_t*>(tab.c0[f] + o), cb = *reinterpret_cast<const uint32_t*>(tab.c1[f] + o);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int a = (ca >> (8 * k)) & 255, b = (cb >> (8 * k)) & 255;
            ch[k] = VF ? chroma_terms(b, a) : chroma_terms(a, b);
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint32_t p[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = yuv_px(((k < 4 ? yr[r].x : yr[r].y) >> (8 * (k & 3))) & 255, ch[k >> 1]);
        uint2* o = reinterpret_cast<uint2*>(dst + (((size_t)f * h + 2 * cy + r) * w + x) * 3);
        o[0] = make_uint2(p[0] | (p[1] << 24), (p[1] >> 8) | (p[2] << 16));
        o[1] = make_uint2((p[2] >> 16) | (p[3] << 8), p[4] | (p[5] << 24));
        o[2] = make_uint2((p[5] >> 8) | (p[6] << 16), (p[6] >> 16) | (p[7] << 8));
    }
}

// Identity size, any even w (the test entry point's small frames): a lane converts a 2 x 2 block, 2-byte loads and stores.
template <bool IL, bool VF>
__global__ void __launch_bounds__(256) yuv_bgr_identity2_kernel(YuvPtrs tab, uint8_t* dst, int h, int w, int y_pitch, int c_pitch) {
    const int f = blockIdx.y;
    const int gw = w >> 1;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (h >> 1) * gw) return;
    const int cy = i / gw, x = (i - cy * gw) << 1;
    const Chroma ch = chroma_at<IL, VF>(tab.c0[f], tab.c1[f], c_pitch, cy, x >> 1);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t yy = *reinterpret_cast<const uint16_t*>(tab.y[f] + (size_t)(2 * cy + r) * y_pitch + x);
        const uint32_t p0 = yuv_px(yy & 255, ch), p1 = yuv_px(yy >> 8, ch);
        uint16_t* o = reinterpret_cast<uint16_t*>(dst + (((size_t)f * h + 2 * cy + r) * w + x) * 3);
        o[0] = (uint16_t)(p0 & 0xffff);
        o[1] = (uint16_t)((p0 >> 16) | ((p1 & 255) << 8));
        o[2] = (uint16_t)(p1 >> 8);
    }
}

// Any other size: cvtColor at source resolution followed by cv2.resize to (H, W).  A lane writes PX adjacent output pixels of one row
// (PX = 4: three dword stores, 4-byte aligned when W % 4 == 0 -- every network width; PX = 2: three 2-byte stores).  Each output
// pixel converts its four source taps (luma + the chroma sample of each tap's 2 x 2 block) and runs the fixed-point bilinear step on
// the converted bytes, exactly as cv2.resize would on cvtColor's output.
template <bool IL, bool VF, int PX>
__global__ void __launch_bounds__(256) yuv_bgr_resize_kernel(YuvPtrs tab, uint8_t* dst, int h, int w, int y_pitch, int c_pitch, int H, int W) {
    const int f = blockIdx.y;
    const int gw = W / PX;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * gw) return;
    const int Y = i / gw, X0 = (i - Y * gw) * PX;
    int y0, y1, b0, b1;
    cv_linear_coeffs(Y, h, H, false, y0, y1, b0, b1);
    const uint8_t* r0 = tab.y[f] + (size_t)y0 * y_pitch;
    const uint8_t* r1 = tab.y[f] + (size_t)y1 * y_pitch;
    const uint8_t* c0 = tab.c0[f];
    const uint8_t* c1 = tab.c1[f];
    uint32_t p[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        int x0, x1, a0, a1;
        cv_linear_coeffs(X0 + k, w, W, true, x0, x1, a0, a1);
        const uint32_t t00 = yuv_px(r0[x0], chroma_at<IL, VF>(c0, c1, c_pitch, y0 >> 1, x0 >> 1));
        const uint32_t t01 = yuv_px(r0[x1], chroma_at<IL, VF>(c0, c1, c_pitch, y0 >> 1, x1 >> 1));
        const uint32_t t10 = yuv_px(r1[x0], chroma_at<IL, VF>(c0, c1, c_pitch, y1 >> 1, x0 >> 1));
        const uint32_t t11 = yuv_px(r1[x1], chroma_at<IL, VF>(c0, c1, c_pitch, y1 >> 1, x1 >> 1));
        uint32_t v = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int s = 8 * c;
            const int h0 = (int)((t00 >> s) & 255) * a0 + (int)((t01 >> s) & 255) * a1;
            const int h1 = (int)((t10 >> s) & 255) * a0 + (int)((t11 >> s) & 255) * a1;
            v |= (uint32_t)cv_linear_vpass(b0, b1, h0, h1) << s;
        }
        p[k] = v;
    }
    uint8_t* out = dst + (((size_t)f * H + Y) * W + X0) * 3;
    if constexpr (PX == 4) {
        uint32_t* o = reinterpret_cast<uint32_t*>(out);
        o[0] = p[0] | (p[1] << 24);
        o[1] = (p[1] >> 8) | (p[2] << 16);
        o[2] = (p[2] >> 16) | (p[3] << 8);
    } else {
        uint16_t* o = reinterpret_cast<uint16_t*>(out);
        o[0] = (uint16_t)(p[0] & 0xffff);
        o[1] = (uint16_t)((p[0] >> 16) | ((p[1] & 255) << 8));
        o[2] = (uint16_t)(p[1] >> 8);
    }
}

template <bool IL, bool VF>
hipError_t launch_fmt(hipStream_t s, const YuvPtrs& tab, int nb, uint8_t* dst, int h, int w, int y_pitch, int c_pitch, int H, int W) {
    if (H == h && W == w) {
        const bool wide = (w & 7) == 0;
        const long long n = (long long)(h >> 1) * (w >> (wide ? 3 : 1));
        const dim3 grid((unsigned)((n + 255) / 256), nb);
        if (wide) hipLaunchKernelGGL((yuv_bgr_identity8_kernel<IL, VF>), grid, dim3(256), 0, s, tab, dst, h, w, y_pitch, c_pitch);
        else hipLaunchKernelGGL((yuv_bgr_identity2_kernel<IL, VF>), grid, dim3(256), 0, s, tab, dst, h, w, y_pitch, c_pitch);
    } else {
        const bool quad = (W & 3) == 0;
        const long long n = (long long)H * (W / (quad ? 4 : 2));
        const dim3 grid((unsigned)((n + 255) / 256), nb);
        if (quad) hipLaunchKernelGGL((yuv_bgr_resize_kernel<IL, VF, 4>), grid, dim3(256), 0, s, tab, dst, h, w, y_pitch, c_pitch, H, W);
        else hipLaunchKernelGGL((yuv_bgr_resize_kernel<IL, VF, 2>), grid, dim3(256), 0, s, tab, dst, h, w, y_pitch, c_pitch, H, W);
    }
    return hipGetLastError();
}

}  // namespace

// planes: B x {y, c0, c1} device addresses; the caller has validated format, sizes, pitches and (for dword loads) 4-byte alignment
hipError_t launch_yuv_to_bgr(hipStream_t s, int fmt, const void* const* planes, int B, int h, int w, int y_pitch, int c_pitch,
                             uint8_t* dst, int H, int W) {
    for (int f0 = 0; f0 < B; f0 += kYuvFrames) {
        const int nb = B - f0 < kYuvFrames ? B - f0 : kYuvFrames;
        // YV12 is I420 with the two chroma planes swapped: it runs the I420 kernels on a swapped table.  (A value-level swap,
        // yuv_bgr_resize_kernel<false, true, 4>, produced wrong bytes on gfx950 in ~12 % of the pixels while the same source with
        // <false, false, 4>, <false, true, 2> and the identity kernels was exact; that instance is not built.)
        const bool swap = fmt == 3;
        YuvPtrs tab{};
        for (int k = 0; k < nb; ++k) {
            tab.y[k] = (const uint8_t*)planes[3 * (f0 + k)];
            tab.c0[k] = (const uint8_t*)planes[3 * (f0 + k) + (swap ? 2 : 1)];
            tab.c1[k] = (const uint8_t*)planes[3 * (f0 + k) + (swap ? 1 : 2)];
        }
        uint8_t* out = dst + (size_t)f0 * H * W * 3;
        hipError_t e;
        switch (fmt) {
            case 0: e = launch_fmt<true, false>(s, tab, nb, out, h, w, y_pitch, c_pitch, H, W); break;      // NV12
            case 1: e = launch_fmt<true, true>(s, tab, nb, out, h, w, y_pitch, c_pitch, H, W); break;       // NV21
            case 2: case 3: e = launch_fmt<false, false>(s, tab, nb, out, h, w, y_pitch, c_pitch, H, W); break;   // I420, YV12
            default: return hipErrorInvalidValue;
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace cf
