// OpenCV's fixed-point INTER_LINEAR coefficients for uint8 (cv2.resize at centerface.py:30), shared by resize_u8_kernel
// (cf_util.hip) and the YUV convert+resize kernel (cf_yuv.hip): ONE statement of the arithmetic.  Every translation unit that
// includes it is built with -ffp-contract=off (Makefile): the coordinates must round like the numpy statement of them.
//
// cv2.resize(img, (W, H)) with the default INTER_LINEAR on uint8 is FIXED-POINT in OpenCV (third-party code, not
// vendored and not installable here; algorithm restated from OpenCV 4.x modules/imgproc/src/resize.cpp,
// the generic path all SIMD paths are bit-exact with):
//   * per destination column: fx = (float)((dx + 0.5) * scale_x - 0.5) with scale_x = 1.0 / ((double)W / w),
//     sx = floor(fx), fx -= sx; sx < 0 -> (sx, fx) = (0, 0); sx >= w - 1 -> (w - 1, 0);
//     coefficients as shorts with 11 fractional bits: a0 = cvRound((1.f - fx) * 2048), a1 = cvRound(fx * 2048);
//   * rows likewise (fy, sy, b0, b1), except that out-of-range rows are CLAMPED (sy + k -> [0, h - 1]) and the
//     coefficients kept;
//   * horizontal pass in int32: r = S[sx] * a0 + S[sx + 1] * a1;
//   * vertical pass (VResizeLinear<uchar, int, short, FixedPtCast<int, uchar, 22>>):
//     dst = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2.
// cvRound = round-half-to-even (rintf).  Parity with an actual cv2 build is UNPINNED (no cv2 anywhere we can run);
// the oracle restates the same published algorithm and the known answers in the tests (identity, exact 2x
// patterns) are derived by hand from it.
#pragma once
#include <hip/hip_runtime.h>

namespace cf {

__device__ __forceinline__ void cv_linear_coeffs(int d, int src, int dst, bool clamp_coeff, int& s0, int& s1, int& c0, int& c1) {
    const double scale = 1.0 / ((double)dst / (double)src);
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int si = (int)floorf(f);
    f -= (float)si;
    if (clamp_coeff) {                                   // columns: coefficient reset at the borders
        if (si < 0) { f = 0.0f; si = 0; }
        if (si >= src - 1) { f = 0.0f; si = src - 1; }
        s0 = si; s1 = min(si + 1, src - 1);
    } else {                                             // rows: indices clamped, coefficients kept
        s0 = min(max(si, 0), src - 1); s1 = min(max(si + 1, 0), src - 1);
    }
    c0 = (int)rintf((1.0f - f) * 2048.0f);
    c1 = (int)rintf(f * 2048.0f);
}
// the vertical pass of one channel (r0, r1: the horizontal passes of the two source rows), saturated to uint8
__device__ __forceinline__ int cv_linear_vpass(int b0, int b1, int r0, int r1) {
    const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
    return min(max(v, 0), 255);
}

}  // namespace cf
