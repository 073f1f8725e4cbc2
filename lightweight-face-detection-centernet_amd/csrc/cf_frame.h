// The caller's source frames -- BGR rows or 4:2:0 planes (NV12 / NV21 / I420 / YV12), pitched, on the host or the device -- as the face
// redaction (cf_redact.hip), the blur (cf_blur.hip), the chips cut from the frame (cf_align_frame.hip) and the tile cutter (cf_tiles.hip)
// see them: the formats, the geometry and its rules, the face list, the plane-address table of one launch, and the staging of host frames.
// (cf_yuv.hip, on the forward path, keeps its own table.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "centerface_hip.h"

namespace cf {

constexpr int kRedactMaxSide = 8192;
__host__ __device__ inline bool frame_is_il(int format) { return format == CF_YUV_NV12 || format == CF_YUV_NV21; }     // one interleaved chroma plane
__host__ __device__ inline int frame_planes(int format) { return format == CF_FRAME_BGR ? 1 : frame_is_il(format) ? 2 : 3; }
__host__ __device__ inline bool frame_swaps_chroma(int format) { return format == CF_YUV_NV21 || format == CF_YUV_YV12; }     // memory order V, U

// B frames of h x w in `format` (CF_YUV_NV12 .. CF_YUV_YV12, CF_FRAME_BGR); pitches in bytes (pitch1: the chroma planes)
struct FrameGeo { int format, B, h, w, pitch0, pitch1; };
// The faces of B images: image b uses the box rows boxes[b * box_stride + i] (4 floats x1,y1,x2,y2 in the coordinates of an H x W network
// input), i < min(counts[b], rows_cap); rows_cap = the rows the producer wrote per image at most, faces_cap = the faces per image the
// launches are sized for (>= 1)
struct FaceList { const float* boxes; int box_stride; const int* counts; int rows_cap, faces_cap, H, W; };

// nullptr, or what is wrong with the geometry (host only).  min_side: 1 or 2; even_always: h and w must be even for BGR frames too
inline const char* frame_geometry_check(const FrameGeo& g, int min_side, bool even_always) {
    const bool bgr = g.format == CF_FRAME_BGR, odd = (g.h | g.w) & 1;
    if (g.format < CF_YUV_NV12 || g.format > CF_FRAME_BGR) return "unknown format (0..3: NV12, NV21, I420, YV12; 4: BGR)";
    if (g.B < 1) return "B must be at least 1";
    const bool size = g.h < min_side || g.w < min_side || g.h > kRedactMaxSide || g.w > kRedactMaxSide;
    if (even_always && (size || odd)) return "h and w must be even and in [2, 8192]";
    if (size) return min_side < 2 ? "h and w must be in [1, 8192]" : "h and w must be in [2, 8192]";
    if (!bgr && odd) return "a 4:2:0 frame has even h and w";
    if (g.pitch0 < (bgr ? 3 * g.w : g.w)) return "pitch0 is below the row size (3w bytes for BGR, w for a Y plane)";
    if (!bgr && g.pitch1 < (frame_is_il(g.format) ? g.w : g.w / 2)) return "pitch1 is below the chroma row size (w bytes for NV12 / NV21, w/2 for I420 / YV12)";
    return nullptr;
}

// The planes of the (at most N) frames of one launch, by value in the kernel arguments.  Every caller names its frames by a HOST table of
// B x {p0, p1, p2} DEVICE addresses (p1 / p2 as the format needs); frame_ptrs takes the frames [f0, f0 + nb) of it, uv_order: the chroma
// planes of YV12 come out U first (an I420 kernel then serves both).
template <int N> struct FramePtrs { uint8_t* p0[N]; uint8_t* p1[N]; uint8_t* p2[N]; };
template <int N> inline FramePtrs<N> frame_ptrs(const void* const* planes, int format, int f0, int nb, bool uv_order) {
    const bool swap = uv_order && format == CF_YUV_YV12;
    FramePtrs<N> t{};
    for (int k = 0; k < nb; ++k) {
        t.p0[k] = (uint8_t*)planes[3 * (f0 + k)];
        t.p1[k] = (uint8_t*)planes[3 * (f0 + k) + (swap ? 2 : 1)];
        t.p2[k] = (uint8_t*)planes[3 * (f0 + k) + (swap ? 1 : 2)];
    }
    return t;
}

// Host frames of the blocking forms: B frames back to back in one device buffer of B * one bytes, every plane at a 4-byte aligned
// offset with a pitch rounded up to 4; the copies move the row bytes only, so the host's own padding is neither read nor written
struct RedactStage { int row0, row1, pitch0, pitch1, rows1; size_t off1, off2, one; };
inline RedactStage redact_stage_layout(int format, int h, int w) {
    RedactStage st{};
    const bool bgr = format == CF_FRAME_BGR, il = frame_is_il(format);
    st.row0 = bgr ? 3 * w : w; st.row1 = bgr ? 0 : il ? w : w / 2;
    st.pitch0 = (st.row0 + 3) & ~3; st.pitch1 = (st.row1 + 3) & ~3;
    st.rows1 = bgr ? 0 : h / 2;
    st.off1 = (size_t)st.pitch0 * h; st.off2 = st.off1 + (size_t)st.pitch1 * st.rows1;
    st.one = bgr ? st.off1 : il ? st.off2 : st.off2 + (size_t)st.pitch1 * st.rows1;
    return st;
}
// the plane table of B frames staged at `base` (nullptr: a table of nullptrs)
inline std::vector<const void*> stage_table(const RedactStage& st, const uint8_t* base, int format, int B) {
    std::vector<const void*> dev((size_t)3 * B, nullptr);
    const size_t off[3] = {0, st.off1, st.off2};
    for (int b = 0; b < B && base; ++b)
        for (int k = 0; k < frame_planes(format); ++k) dev[3 * b + k] = base + (size_t)b * st.one + off[k];
    return dev;
}
inline hipError_t redact_stage_copy(hipStream_t s, const RedactStage& st, int format, const void* const* host_planes, int B, int h, int pitch0,
                                    int pitch1, uint8_t* dev, bool to_device) {
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < frame_planes(format); ++k) {
            uint8_t* d = dev + (size_t)b * st.one + (k == 0 ? 0 : k == 1 ? st.off1 : st.off2);
            void* hp = const_cast<void*>(host_planes[3 * b + k]);
            const size_t dp = k == 0 ? st.pitch0 : st.pitch1, hpitch = k == 0 ? pitch0 : pitch1, row = k == 0 ? st.row0 : st.row1;
            const size_t rows = k == 0 ? h : st.rows1;
            const hipError_t e = to_device ? hipMemcpy2DAsync(d, dp, hp, hpitch, row, rows, hipMemcpyHostToDevice, s)
                                           : hipMemcpy2DAsync(hp, hpitch, d, dp, row, rows, hipMemcpyDeviceToHost, s);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

}  // namespace cf
