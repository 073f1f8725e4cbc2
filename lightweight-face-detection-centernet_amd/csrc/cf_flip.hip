// Flip test: the mirrored half of the network input, and the fold of the two halves of the head records into the first.  The statement
// (which value of which record goes where, in which float32 order) is in include/centerface_hip.h under cf_set_flip_test; both kernels
// move every byte once and compute next to nothing, so what they are written for is the shape of their memory accesses.
//
// MIRROR.  dst holds 2B network inputs; image B + b becomes image b of src with its columns reversed, and when src is not dst already
// (the caller's device tensor, a host-input slot) the same launch stores image b itself into dst: the forward reads one contiguous batch.
//   * uint8 [.][H][W][3]: a row is W * 3 bytes and W % 32 == 0, so a row is a whole number of 48-byte groups of 16 pixels, and groups
//     are 16-byte aligned whenever the image is.  A lane loads one group (three 16-byte loads; twelve dword loads when src is only
//     4-byte aligned, the caller's tensor -- written as dwords, so the compiler claims no more than that alignment), reverses the order of its sixteen 3-byte pixels -- four blocks of four pixels = three dwords
//     each: the blocks change places and each is reversed by four v_perm_b32 -- and stores it as three 16-byte stores at the mirrored
//     group of the row.  Consecutive lanes read consecutive groups; the stores of a wave cover the same bytes of the mirrored rows.
//   * float32 [.][3][H][W]: a lane owns four floats of a plane row (one 16-byte load, or four dwords), and stores them reversed at the
//     mirrored place (one 16-byte store).
// dst is context-owned (or the op's own allocation): always 16-byte aligned, as is every image in it (3 * H * W is a multiple of 3072).
//
// MERGE.  rec [2B][h][w][16] float32, in place.  Four lanes share a cell, lane q owning floats 4q .. 4q + 3 of the record: one 16-byte
// load of its part of a = rec[b][y][x], two 16-byte loads of the 8-float half of m = rec[B + b][y][w - 1 - x] that holds everything its
// part needs (the point pairs 0 <-> 1 and 3 <-> 4 change places, which crosses 16-byte parts but not 32-byte halves), one 16-byte store
// over its part of a.  The four lanes are the only readers and the only writers of that cell; m lies in the second half of the batch,
// which nothing writes.  Lane 0 of the four also stores the heat into hm_plane.  Consecutive lanes read and write consecutive 16 bytes
// of the first half; the m loads of a wave walk whole 64-byte records downwards.
#include "cf_common.h"
#include "cf_kernels.h"
#include <cstdint>
#include <cstdio>
#include <string>

namespace cf {
namespace {

// v_perm_b32: byte i of the result is picked by byte i of sel, 0 .. 3 = bytes of lo, 4 .. 7 = bytes of hi
__device__ __forceinline__ uint32_t bperm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

// Four pixels in three dwords, bytes 0 .. 11 = p0 b g r | p1 b g r | p2 b g r | p3 b g r  ->  p3 | p2 | p1 | p0:
// o0 = bytes 9 10 11 6, o1 = bytes 7 8 3 4, o2 = bytes 5 0 1 2
__device__ __forceinline__ void reverse_px4(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t& o0, uint32_t& o1, uint32_t& o2) {
    o0 = bperm(d2, d1, 0x02070605u);                       // d2.1 d2.2 d2.3 d1.2
    const uint32_t t = bperm(d2, d1, 0x000c0403u);         // d1.3 d2.0  0   d1.0
    o1 = bperm(d0, t, 0x03070100u);                        //  t.0  t.1 d0.3  t.3
    o2 = bperm(d1, d0, 0x02010005u);                       // d1.1 d0.0 d0.1 d0.2
}

// A16: src is 16-byte aligned; COPY: dst is another buffer than src and receives the unmirrored images as well.
// One lane per 48-byte group; ng = W / 16 groups per row, n = B * H * ng groups.
template <bool A16, bool COPY>
__global__ void __launch_bounds__(256) mirror_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long n, int ng, long long half) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long row = i / ng;
    const int g = (int)(i - row * ng);
    uint32_t d[12];
    if constexpr (A16) {
        const uint4* p = reinterpret_cast<const uint4*>(src + i * 48);
#pragma unroll
        for (int k = 0; k < 3; ++k) { const uint4 v = p[k]; d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w; }
    } else {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(src + i * 48);
#pragma unroll
        for (int k = 0; k < 12; ++k) d[k] = p[k];
    }
    if constexpr (COPY) {
        uint4* o = reinterpret_cast<uint4*>(dst + i * 48);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = make_uint4(d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]);
    }
    uint32_t r[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) reverse_px4(d[9 - 3 * k], d[10 - 3 * k], d[11 - 3 * k], r[3 * k], r[3 * k + 1], r[3 * k + 2]);
    uint4* o = reinterpret_cast<uint4*>(dst + half + (row * ng + (ng - 1 - g)) * 48);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = make_uint4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
}

// One lane per four floats; ng = W / 4 groups per plane row, n = B * 3 * H * ng groups, half = B * 3 * H * W floats
template <bool A16, bool COPY>
__global__ void __launch_bounds__(256) mirror_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n, int ng, long long half) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long row = i / ng;
    const int g = (int)(i - row * ng);
    float4 v;
    if constexpr (A16) v = *reinterpret_cast<const float4*>(src + i * 4);
    else { const float* p = src + i * 4; v = make_float4(p[0], p[1], p[2], p[3]); }
    if constexpr (COPY) *reinterpret_cast<float4*>(dst + i * 4) = v;
    *reinterpret_cast<float4*>(dst + half + (row * ng + (ng - 1 - g)) * 4) = make_float4(v.w, v.z, v.y, v.x);
}

// n = B * h * w * 4 lanes; hw = h * w; half = B * hw cells
__global__ void __launch_bounds__(256) flip_heads_kernel(float* __restrict__ rec, float* __restrict__ hm_plane, long long n, int w, long long half) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long cell = i >> 2;
    const int q = (int)(i & 3);
    const long long row = cell / w;                        // (b * h + y)
    const int x = (int)(cell - row * w);
    float4* mine = reinterpret_cast<float4*>(rec) + i;
    const float4 a = *mine;
    const float4* mp = reinterpret_cast<const float4*>(rec) + (half + row * w + (w - 1 - x)) * 4 + (q & 2);
    const float4 m0 = mp[0], m1 = mp[1];                   // floats 0 .. 7 (q = 0, 1) or 8 .. 15 (q = 2, 3) of the mirrored pass's record
    float4 o;
    switch (q) {
        case 0:  // heat, wh, x of point 0 <- point 1
            o = make_float4((a.x + m0.x) * 0.5f, (a.y + m0.y) * 0.5f, (a.z + m0.z) * 0.5f, (a.w - m1.y) * 0.5f);
            hm_plane[cell] = o.x;
            break;
        case 1:  // y of point 0 <- 1, x y of point 1 <- 0, x of point 2
            o = make_float4((a.x + m1.z) * 0.5f, (a.y - m0.w) * 0.5f, (a.z + m1.x) * 0.5f, (a.w - m1.w) * 0.5f);
            break;
        case 2:  // y of point 2, x y of point 3 <- 4, x of point 4 <- 3
            o = make_float4((a.x + m0.x) * 0.5f, (a.y - m0.w) * 0.5f, (a.z + m1.x) * 0.5f, (a.w - m0.y) * 0.5f);
            break;
        default: // y of point 4 <- 3, reg of the unmirrored pass, the mean logit
            o = make_float4((a.x + m0.z) * 0.5f, a.y, a.z, (a.w + m1.w) * 0.5f);
            break;
    }
    *mine = o;
}

}  // namespace

const char* mirror_check(std::string& why, int in_format, int B, int H, int W) {
    char b[160];
    auto say = [&](const char* s) { why = s; return why.c_str(); };
    if (in_format != CF_IN_U8_HWC_BGR && in_format != CF_IN_F32_NCHW) { snprintf(b, sizeof b, "unknown input format %d", in_format); return say(b); }
    if (B < 1) { snprintf(b, sizeof b, "B=%d must be at least 1", B); return say(b); }
    if (H < 1 || W < 32 || (W % 32)) { snprintf(b, sizeof b, "H=%d, W=%d: W must be a positive multiple of 32 and H at least 1", H, W); return say(b); }
    return nullptr;
}

hipError_t launch_mirror_batch(hipStream_t s, int in_format, const void* src, void* dst, int B, int H, int W) {
    std::string why;
    if (mirror_check(why, in_format, B, H, W) || !src || !dst || (reinterpret_cast<uintptr_t>(src) & 3) || (reinterpret_cast<uintptr_t>(dst) & 15))
        return hipErrorInvalidValue;
    const bool a16 = (reinterpret_cast<uintptr_t>(src) & 15) == 0, copy = src != dst;
    if (in_format == CF_IN_U8_HWC_BGR) {
        const int ng = W / 16;
        const long long n = (long long)B * H * ng, half = (long long)B * H * W * 3;
        const dim3 grid((unsigned)((n + 255) / 256));
        const uint8_t* in = (const uint8_t*)src; uint8_t* out = (uint8_t*)dst;
        if (a16 && copy) hipLaunchKernelGGL((mirror_u8_kernel<true, true>), grid, dim3(256), 0, s, in, out, n, ng, half);
        else if (a16) hipLaunchKernelGGL((mirror_u8_kernel<true, false>), grid, dim3(256), 0, s, in, out, n, ng, half);
        else if (copy) hipLaunchKernelGGL((mirror_u8_kernel<false, true>), grid, dim3(256), 0, s, in, out, n, ng, half);
        else return hipErrorInvalidValue;                  // (src == dst is 16-byte aligned)
    } else {
        const int ng = W / 4;
        const long long n = (long long)B * 3 * H * ng, half = (long long)B * 3 * H * W;
        const dim3 grid((unsigned)((n + 255) / 256));
        const float* in = (const float*)src; float* out = (float*)dst;
        if (a16 && copy) hipLaunchKernelGGL((mirror_f32_kernel<true, true>), grid, dim3(256), 0, s, in, out, n, ng, half);
        else if (a16) hipLaunchKernelGGL((mirror_f32_kernel<true, false>), grid, dim3(256), 0, s, in, out, n, ng, half);
        else if (copy) hipLaunchKernelGGL((mirror_f32_kernel<false, true>), grid, dim3(256), 0, s, in, out, n, ng, half);
        else return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_flip_heads(hipStream_t s, float* rec, float* hm_plane, int B, int h, int w) {
    if (!rec || !hm_plane || B < 1 || h < 1 || w < 1 || (reinterpret_cast<uintptr_t>(rec) & 15)) return hipErrorInvalidValue;
    const long long half = (long long)B * h * w, n = half * 4;
    hipLaunchKernelGGL(flip_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rec, hm_plane, n, w, half);
    return hipGetLastError();
}

}  // namespace cf
