// What the redaction (cf_redact.hip) and the blur (cf_blur.hip) share on the device: the float64 box mapping of step 1 and the
// half-pixel point tests of step 2 of the statement in include/centerface_hip.h, the face of a workgroup, the walk over the planes of
// its clipped box and the masked store.  Both files are compiled with -ffp-contract=off, so the mapping rounds every operation as
// tests/test_redact.py restates it.
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "cf_frame.h"

namespace cf {

constexpr int kRedactFrames = 32;                     // frames per launch: 3 x 32 plane addresses by value = 768 bytes of kernel arguments
constexpr int kRedactGridTarget = 32768;              // workgroups per launch aimed at when choosing the slices per face
using RedactPtrs = FramePtrs<kRedactFrames>;

struct FaceBox { int X1, Y1, X2, Y2; bool ok; };

__device__ __forceinline__ int snap(double v) { return (int)fmin(fmax(v, -8192.0), 16384.0); }

__device__ __forceinline__ FaceBox face_box(const float* bx, float scale, int h, int w, int H, int W) {
    const double x1 = (double)bx[0], y1 = (double)bx[1], x2 = (double)bx[2], y2 = (double)bx[3], s = (double)scale;
    const double cx = (x1 + x2) * 0.5, cy = (y1 + y2) * 0.5;
    const double hw = (x2 - x1) * 0.5 * s, hh = (y2 - y1) * 0.5 * s;
    const double fx = (double)w / (double)W, fy = (double)h / (double)H;
    FaceBox f;
    f.ok = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && hw > 0.0 && hh > 0.0;
    if (!f.ok) { f.X1 = f.Y1 = f.X2 = f.Y2 = 0; return f; }
    f.X1 = snap(floor((cx - hw) * fx)) & ~1;
    f.Y1 = snap(floor((cy - hh) * fy)) & ~1;
    f.X2 = (snap(ceil((cx + hw) * fx)) + 1) & ~1;
    f.Y2 = (snap(ceil((cy + hh) * fy)) + 1) & ~1;
    return f;
}

// The point test of a sample at the half-pixel point (U, V) against one snapped box: RECT 2*X1 <= U < 2*X2 and 2*Y1 <= V < 2*Y2;
// ELLIPSE (du*Bv)^2 + (dv*A)^2 <= (A*Bv)^2 in int64.  U, V of a sample inside a frame of at most 8192 a side: no product overflows.
__device__ __forceinline__ bool face_covers(int X1, int Y1, int X2, int Y2, bool ellipse, int U, int V) {
    if (!ellipse) return 2 * X1 <= U && U < 2 * X2 && 2 * Y1 <= V && V < 2 * Y2;
    const long long A = X2 - X1, Bv = Y2 - Y1;
    const long long tu = (long long)(U - (X1 + X2)) * Bv, tv = (long long)(V - (Y1 + Y2)) * A;
    return tu * tu + tv * tv <= (A * Bv) * (A * Bv);
}

// the face of this workgroup (blockIdx.x = image * faces_cap + keep position) and its box clipped to the frame; false = nothing to do.
// Uniform over the workgroup.
struct Clip { int b, X1, Y1, X2, Y2, cx1, cy1, cx2, cy2; };
__device__ __forceinline__ bool face_clip(const FrameGeo& g, const FaceList& l, float scale, Clip& c) {
    const int n = (int)blockIdx.x;
    c.b = n / l.faces_cap;
    const int i = n - c.b * l.faces_cap;
    if (c.b >= g.B || i >= min(l.counts[c.b], l.rows_cap)) return false;
    const FaceBox f = face_box(l.boxes + ((size_t)c.b * l.box_stride + i) * 4, scale, g.h, g.w, l.H, l.W);
    if (!f.ok) return false;
    c.X1 = f.X1; c.Y1 = f.Y1; c.X2 = f.X2; c.Y2 = f.Y2;
    c.cx1 = max(f.X1, 0); c.cy1 = max(f.Y1, 0); c.cx2 = min(f.X2, g.w); c.cy2 = min(f.Y2, g.h);
    return c.cx1 < c.cx2 && c.cy1 < c.cy2;
}

// Plane `ps` of a frame as a face's workgroup walks it: bytes per sample position (3 BGR, 1 planar, 2 interleaved chroma), whether its
// samples are chroma samples, its pitch, the clipped box in its samples [sx0, sx1) x [sy0, sy1) (4:2:0: the clipped box is even on every
// side) and the aligned dwords [d0, d0 + nd) of a row that hold them.
struct PlanePass {
    bool chroma;
    int bps, pitch, sx0, sx1, sy0, sy1, d0, nd;
    __device__ __forceinline__ int point(int s) const { return chroma ? 4 * s + 2 : 2 * s + 1; }      // sample index -> half-pixel units
};
__device__ __forceinline__ PlanePass plane_pass(const FrameGeo& g, int ps, const Clip& c) {
    PlanePass p;
    p.chroma = ps > 0;
    p.bps = g.format == CF_FRAME_BGR ? 3 : (frame_is_il(g.format) && ps == 1) ? 2 : 1;
    p.pitch = p.chroma ? g.pitch1 : g.pitch0;
    p.sx0 = p.chroma ? c.cx1 >> 1 : c.cx1; p.sx1 = p.chroma ? c.cx2 >> 1 : c.cx2;
    p.sy0 = p.chroma ? c.cy1 >> 1 : c.cy1; p.sy1 = p.chroma ? c.cy2 >> 1 : c.cy2;
    p.d0 = (p.bps * p.sx0) >> 2; p.nd = ((p.bps * p.sx1 + 3) >> 2) - p.d0;
    return p;
}

// The bytes k of the aligned dword at q with bit k of mask set become those of val: the whole dword when all four are, single bytes
// otherwise -- never a read-modify-write.
__device__ __forceinline__ void store_masked_dword(uint8_t* q, uint32_t val, int mask) {
    if (mask == 15) {
        *reinterpret_cast<uint32_t*>(q) = val;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (mask & (1 << k)) q[k] = (uint8_t)(val >> (8 * k));
    }
}

}  // namespace cf
