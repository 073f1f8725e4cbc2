// The per-pixel arithmetic of the 4:2:0 -> BGR conversion (OpenCV's fixed-point BT.601 limited-range statement, see cf_yuv.hip), shared
// by the whole-frame conversion kernels (cf_yuv.hip) and the tile cutter (cf_tiles.hip): ONE statement of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cf {

// the chroma half of the three channel sums, rounding constant included
struct Chroma { int b, g, r; };
__device__ __forceinline__ Chroma chroma_terms(int U, int V) {
    const int uu = U - 128, vv = V - 128;
    return {(1 << 19) + 2116026 * uu, (1 << 19) - 852492 * vv - 409993 * uu, (1 << 19) + 1673527 * vv};
}
__device__ __forceinline__ uint32_t sat8(int v) { return (uint32_t)min(max(v >> 20, 0), 255); }
// one pixel -> B | G << 8 | R << 16
__device__ __forceinline__ uint32_t yuv_px(int Y, const Chroma& c) {
    const int y = max(Y - 16, 0) * 1220542;
    return sat8(y + c.b) | (sat8(y + c.g) << 8) | (sat8(y + c.r) << 16);
}
// IL: one interleaved chroma plane (NV12 / NV21), else two (c0 = U, c1 = V); VF: V comes first in the interleaved pairs (NV21)
template <bool IL, bool VF>
__device__ __forceinline__ Chroma chroma_at(const uint8_t* c0, const uint8_t* c1, int c_pitch, int cy, int cx) {
    int a, b;
    if (IL) { const uint8_t* p = c0 + (size_t)cy * c_pitch + 2 * cx; a = p[0]; b = p[1]; }
    else { a = c0[(size_t)cy * c_pitch + cx]; b = c1[(size_t)cy * c_pitch + cx]; }
    return VF ? chroma_terms(b, a) : chroma_terms(a, b);
}

}  // namespace cf
