// Small shared pieces: kernel-symbol tags for the profiler and the NCHW<->NHWC converters used at
// the test boundary (cf_get_heads / cf_op_*).
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_cvresize.h"
#include <cstdarg>
#include <cstdio>

namespace cf {

static thread_local char g_kernel_tag[160] = "";
const char* last_kernel_tag() { return g_kernel_tag; }
void set_kernel_tag(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_kernel_tag, sizeof g_kernel_tag, fmt, ap); va_end(ap);
}

// ---------------------------------------------------------------- bilinear resize (centerface.py:30)
// cv2.resize's fixed-point INTER_LINEAR for uint8: the coefficients and the vertical pass are stated once, in cf_cvresize.h
__global__ void resize_u8_kernel(const uint8_t* src, uint8_t* dst, int B, int h, int w, int H, int W) {
    const long long n = (long long)B * H * W;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int X = (int)(i % W); const long long t = i / W;
    const int Y = (int)(t % H); const int b = (int)(t / H);
    int x0, x1, a0, a1, y0, y1, b0, b1;
    cv_linear_coeffs(X, w, W, true, x0, x1, a0, a1);
    cv_linear_coeffs(Y, h, H, false, y0, y1, b0, b1);
    const uint8_t* p00 = src + (((size_t)b * h + y0) * w + x0) * 3;
    const uint8_t* p01 = src + (((size_t)b * h + y0) * w + x1) * 3;
    const uint8_t* p10 = src + (((size_t)b * h + y1) * w + x0) * 3;
    const uint8_t* p11 = src + (((size_t)b * h + y1) * w + x1) * 3;
    uint8_t* d = dst + (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int r0 = (int)p00[c] * a0 + (int)p01[c] * a1;
        const int r1 = (int)p10[c] * a0 + (int)p11[c] * a1;
        d[c] = (uint8_t)cv_linear_vpass(b0, b1, r0, r1);
    }
}
// ---- host images -> HBM by a kernel (zero-copy reads of page-locked host memory over PCIe) -------------------------------------
// One launch moves up to 64 separately allocated images: the DMA engines need one command per image (8-10 us of idle link between
// two ~22 us copies of a VGA image) and ~0.3 ms from the end of a copy to the start of a kernel that waits for it on another stream
// (profiles/r05_vga_pipeline.md); a kernel has neither.  blockIdx.y = image, 16-byte loads, UNR in flight per lane: 48 workgroups x
// 256 lanes x 4 x 16 B = 786 KB in flight covers the link's bandwidth-delay product many times.
struct UploadPtrs { const uint8_t* src[64]; };
template <int UNR>
__global__ void __launch_bounds__(256) upload_images_kernel(UploadPtrs tab, uint8_t* dst, long long bytes) {
    const uint8_t* src = tab.src[blockIdx.y];
    uint8_t* out = dst + (size_t)blockIdx.y * bytes;
    const long long nvec = bytes >> 4;                                   // both ends 16-byte aligned (checked by the launcher)
    const long long stride = (long long)gridDim.x * 256;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4* s4 = reinterpret_cast<const u32x4*>(src);
    u32x4* d4 = reinterpret_cast<u32x4*>(out);
    for (; i + (UNR - 1) * stride < nvec; i += UNR * stride) {
        u32x4 v[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) v[u] = __builtin_nontemporal_load(s4 + i + u * stride);
#pragma unroll
        for (int u = 0; u < UNR; ++u) d4[i + u * stride] = v[u];
    }
    for (; i < nvec; i += stride) d4[i] = __builtin_nontemporal_load(s4 + i);
    if (blockIdx.x == 0 && threadIdx.x < (bytes & 15)) out[(nvec << 4) + threadIdx.x] = src[(nvec << 4) + threadIdx.x];
}
// imgs: DEVICE-visible addresses of B page-locked host images of `bytes` each; dst: [B][bytes] on the device (16-byte aligned)
hipError_t launch_upload_images(hipStream_t s, const void* const* imgs, uint8_t* dst, int B, long long bytes) {
    if (B <= 0 || bytes <= 0) return hipSuccess;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int nb = B - b0 < 64 ? B - b0 : 64;
        UploadPtrs tab{};
        for (int b = 0; b < nb; ++b) tab.src[b] = (const uint8_t*)imgs[b0 + b];
        int gx = (int)((bytes / 16 + 256 * 4 - 1) / (256 * 4));
        const int want = (96 + nb - 1) / nb;                             // ~96 workgroups per launch: the link, not the CUs, is the limit
        if (gx > want) gx = want;
        if (gx < 1) gx = 1;
        hipLaunchKernelGGL(upload_images_kernel<4>, dim3(gx, nb), dim3(256), 0, s, tab, dst + (size_t)b0 * bytes, bytes);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_resize_u8(hipStream_t s, const uint8_t* src, uint8_t* dst, int B, int h, int w, int H, int W) {
    const long long n = (long long)B * H * W;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(resize_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, B, h, w, H, W);
    return hipGetLastError();
}

// ---------------------------------------------------------------- layout converters (test boundary)
template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* src, T* dst, int B, int C, int H, int W) {
    const long long n = (long long)B * C * H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        int c = (int)(i % C); long long t = i / C;
        int x = (int)(t % W); t /= W;
        int y = (int)(t % H); int b = (int)(t / H);
        float v = src[(((size_t)b * C + c) * H + y) * W + x];
        if constexpr (sizeof(T) == 4) dst[i] = v;
        else dst[i] = (T)(pack_bf16x2(v, 0.0f) & 0xffffu);
    }
}
template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* src, float* dst, int B, int C, int H, int W) {
    const long long n = (long long)B * C * H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        int x = (int)(i % W); long long t = i / W;
        int y = (int)(t % H); t /= H;
        int c = (int)(t % C); int b = (int)(t / C);
        T v = src[(((size_t)b * H + y) * W + x) * C + c];
        if constexpr (sizeof(T) == 4) dst[i] = v;
        else dst[i] = bf16_to_f32(v);
    }
}
// pixel-block order [m / 32][C / P][m % 32][P] (P = channels per 16 bytes: 8 bf16 / 4 fp32), m = (b H + y) W + x  ->  NCHW float32
template <typename T>
__global__ void blocked_to_nchw_kernel(const T* src, float* dst, int B, int C, int H, int W) {
    constexpr int P = 16 / (int)sizeof(T);
    const long long n = (long long)B * C * H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        int x = (int)(i % W); long long t = i / W;
        int y = (int)(t % H); t /= H;
        int c = (int)(t % C); int b = (int)(t / C);
        const size_t m = ((size_t)b * H + y) * W + x;
        const T v = src[(((m >> 5) * (size_t)(C / P) + (size_t)(c / P)) * 32 + (m & 31)) * P + (c % P)];
        if constexpr (sizeof(T) == 4) dst[i] = v;
        else dst[i] = bf16_to_f32(v);
    }
}
// NCHW float32 -> pixel-block order (the inverse of blocked_to_nchw_kernel); dst holds whole 32-pixel blocks, the pixels past
// B H W of the last one are left as the caller filled them
template <typename T>
__global__ void nchw_to_blocked_kernel(const float* src, T* dst, int B, int C, int H, int W) {
    constexpr int P = 16 / (int)sizeof(T);
    const long long n = (long long)B * C * H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        int x = (int)(i % W); long long t = i / W;
        int y = (int)(t % H); t /= H;
        int c = (int)(t % C); int b = (int)(t / C);
        const size_t m = ((size_t)b * H + y) * W + x;
        const float v = src[i];
        T* d = dst + (((m >> 5) * (size_t)(C / P) + (size_t)(c / P)) * 32 + (m & 31)) * P + (c % P);
        if constexpr (sizeof(T) == 4) *d = v;
        else *d = (T)(pack_bf16x2(v, 0.0f) & 0xffffu);
    }
}
static unsigned conv_grid(long long n) { long long g = (n + 255) / 256; return (unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g)); }

hipError_t launch_nchw_to_nhwc(hipStream_t s, int dtype, const float* src, void* dst, int B, int C, int H, int W) {
    long long n = (long long)B * C * H * W;
    if (n == 0) return hipSuccess;
    if (dtype != 1) hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, dim3(conv_grid(n)), dim3(256), 0, s, src, (float*)dst, B, C, H, W);
    else hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16_t>, dim3(conv_grid(n)), dim3(256), 0, s, src, (bf16_t*)dst, B, C, H, W);
    return hipGetLastError();
}
hipError_t launch_blocked_to_nchw(hipStream_t s, int dtype, const void* src, float* dst, int B, int C, int H, int W) {
    long long n = (long long)B * C * H * W;
    if (n == 0) return hipSuccess;
    if (dtype != 1) hipLaunchKernelGGL(blocked_to_nchw_kernel<float>, dim3(conv_grid(n)), dim3(256), 0, s, (const float*)src, dst, B, C, H, W);
    else hipLaunchKernelGGL(blocked_to_nchw_kernel<bf16_t>, dim3(conv_grid(n)), dim3(256), 0, s, (const bf16_t*)src, dst, B, C, H, W);
    return hipGetLastError();
}
hipError_t launch_nchw_to_blocked(hipStream_t s, int dtype, const float* src, void* dst, int B, int C, int H, int W) {
    long long n = (long long)B * C * H * W;
    if (n == 0) return hipSuccess;
    if (dtype != 1) hipLaunchKernelGGL(nchw_to_blocked_kernel<float>, dim3(conv_grid(n)), dim3(256), 0, s, src, (float*)dst, B, C, H, W);
    else hipLaunchKernelGGL(nchw_to_blocked_kernel<bf16_t>, dim3(conv_grid(n)), dim3(256), 0, s, src, (bf16_t*)dst, B, C, H, W);
    return hipGetLastError();
}
hipError_t launch_nhwc_to_nchw(hipStream_t s, int dtype, const void* src, float* dst, int B, int C, int H, int W) {
    long long n = (long long)B * C * H * W;
    if (n == 0) return hipSuccess;
    if (dtype != 1) hipLaunchKernelGGL(nhwc_to_nchw_kernel<float>, dim3(conv_grid(n)), dim3(256), 0, s, (const float*)src, dst, B, C, H, W);
    else hipLaunchKernelGGL(nhwc_to_nchw_kernel<bf16_t>, dim3(conv_grid(n)), dim3(256), 0, s, (const bf16_t*)src, dst, B, C, H, W);
    return hipGetLastError();
}

}  // namespace cf
