// The face geometry that the redaction (cf_redact.hip) and the blur (cf_blur.hip) share: the float64 box mapping of step 1 and the
// half-pixel point tests of step 2 of the statement in include/centerface_hip.h.  Both files are compiled with -ffp-contract=off, so the
// mapping rounds every operation as tests/test_redact.py restates it.
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace cf {

constexpr int kRedactFrames = 32;                     // frames per launch: 3 x 32 plane addresses by value = 768 bytes of kernel arguments
constexpr int kRedactGridTarget = 32768;              // workgroups per launch aimed at when choosing the slices per face
struct RedactPtrs { uint8_t* p0[kRedactFrames]; uint8_t* p1[kRedactFrames]; uint8_t* p2[kRedactFrames]; };

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

}  // namespace cf
