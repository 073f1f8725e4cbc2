// Aligned face chips: for every kept detection, the least-squares similarity that maps its five landmarks onto a chip template
// (the ArcFace 112 x 112 points by default) and the S x S bilinear warp of the uint8 BGR network input under it -- one launch for
// the whole batch, no host round trip (cf_align_faces, cf_op_align_faces).
//
// The arithmetic is this project's own statement, restated in numpy in tests/test_align.py; kernel and restatement are equal bit
// for bit.  It has the same optimum as the common SimilarityTransform.estimate + cv2.warpAffine recipe and the structure of
// OpenCV's warpAffine (1/32-pixel positions, weights out of 1024), but it is NOT bit-identical to cv2.warpAffine: cv2 reads its
// bilinear weights from a rounded 15-bit table, here they are the exact products (32 - fx)(32 - fy), ... .
//
// Estimate, float64, no FMA contraction (this file is compiled with -ffp-contract=off), operation order as written:
//   p[0..4] landmarks (float32 -> double), q[0..4] template points in chip pixels
//   pm = ((((p0 + p1) + p2) + p3) + p4) / 5.0, qm likewise; pc = p - pm, qc = q - qm
//   den += pcx*pcx + pcy*pcy;  na += pcx*qcx + pcy*qcy;  nb += pcx*qcy - pcy*qcx      (i = 0..4, from 0.0)
//   a = na / den, b = nb / den;  tx = qmx - (a*pmx - b*pmy), ty = qmy - (b*pmx + a*pmy)
// Inverse (chip -> source): D = a*a + b*b, ia = a / D, ib = b / D,
//   M = [ia, ib, -(ia*tx + ib*ty), -ib, ia, -(-ib*tx + ia*ty)]
// Alignable: ten finite landmark values, den > 0, D > 0, M finite and max(|M0|,|M1|,|M3|,|M4|) * S + max(|M2|,|M5|) < 2^20 (every
// fixed-point coordinate below then fits int32).  Otherwise M = 0 and the chip is that of an all-zero source.
// Warp, integers:
//   ad[x] = rint(M0*x*1024), bd[x] = rint(M3*x*1024), X0[y] = rint((M1*y + M2)*1024) + 16, Y0[y] = rint((M4*y + M5)*1024) + 16
//   X = (X0[y] + ad[x]) >> 5, Y = (Y0[y] + bd[x]) >> 5;  sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31   (arithmetic shifts)
//   neighbours (sy,sx) (sy,sx+1) (sy+1,sx) (sy+1,sx+1), weights (32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx*fy; a neighbour outside
//   the image contributes 0 (constant border 0, per neighbour);  out = (sum w*pix + 512) >> 10 per channel
#include <limits.h>
#include <math.h>

#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_alignmath.h"

namespace cf {
namespace {

// One workgroup = one face x one band of kAlignItems groups of 4 adjacent chip pixels.  Every workgroup finds its (image, keep
// position) from the per-image counts (B is at most the context's max_batch: a short uniform loop) and recomputes the face's
// estimate (about a hundred double operations, wave-uniform); the per-column and per-row fixed-point terms go through LDS.
// A thread's 4 pixels leave as three dword stores (uint8 HWC) or one float4 per channel (float NCHW): S is a multiple of 4.
__global__ void __launch_bounds__(256) align_chips_kernel(AlignParams p) {
    __shared__ int tab[4 * kAlignMaxS];                     // ad | bd | X0 | Y0
    const int S = p.S, q4 = S >> 2, items = S * q4;
    const int bands = (items + kAlignItems - 1) / kAlignItems;
    const int n = (int)(blockIdx.x / (unsigned)bands), band = (int)(blockIdx.x - (unsigned)n * bands);
    const int tid = threadIdx.x;
    int b;
    size_t row;
    if (!align_find_face(p, n, b, row)) return;                                // uniform: before any barrier
    double l[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) l[j] = (double)p.lms[row * 10 + j];
    const Similarity sim = estimate_inverse(l, p.tmpl, S);
    if (band == 0 && tid == 0 && p.mats) {
#pragma unroll
        for (int j = 0; j < 6; ++j) p.mats[(size_t)n * 6 + j] = sim.M[j];
    }
    align_fill_tables(tab, sim, S);
    __syncthreads();
    const int H = p.H, W = p.W;
    const uint32_t* img = reinterpret_cast<const uint32_t*>(p.img);
    const size_t last = p.img_dwords - 1;
    const size_t img0 = (size_t)b * H * W;
#pragma unroll 1
    for (int it = 0; it < kAlignItems / 256; ++it) {
        const int item = band * kAlignItems + it * 256 + tid;
        if (item >= items) break;
        const int y = item / q4, x0 = (item - y * q4) << 2;
        const int X0 = tab[2 * kAlignMaxS + y], Y0 = tab[3 * kAlignMaxS + y];
        uint32_t px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const AlignTap t = align_tap((X0 + tab[x0 + k]) >> 5, (Y0 + tab[kAlignMaxS + x0 + k]) >> 5, H, W, sim.ok);
            uint32_t v = 0;
            if (align_tap_live(t)) {
                uint32_t a0, a1, c0, c1;
                fetch_pair(img, (img0 + (size_t)t.r0 * W + t.cx) * 3, last, a0, a1);
                fetch_pair(img, (img0 + (size_t)t.r1 * W + t.cx) * 3, last, c0, c1);
                v = align_blend(t, a0, a1, c0, c1);
            }
            px[k] = v;
        }
        align_store4(p, n, y, x0, px);
    }
}

}  // namespace

// the five ArcFace points of the 112 x 112 chip
static const double kArcFace112[10] = {38.2946, 51.6963, 73.5318, 51.5014, 56.0252, 71.7366, 41.5493, 92.3655, 70.7299, 92.2041};

const char* align_params_set(AlignParams& p, int size, int format, int rgb, float mean, float scale, const float* tmpl, int max_per_image) {
    if (size < 16 || size > kAlignMaxS || (size & 3)) return "size must be a multiple of 4 in [16, 512]";
    if (format != 0 && format != 1) return "unknown chip format (0 = CF_CHIP_U8_HWC_BGR, 1 = CF_CHIP_F32_NCHW)";
    if (max_per_image < 0) return "max_per_image must be 0 (all) or positive";
    p.S = size; p.format = format; p.rgb = rgb != 0; p.mean = mean; p.scale = scale; p.max_per_image = max_per_image;
    for (int j = 0; j < 10; ++j) p.tmpl[j] = tmpl ? (double)tmpl[j] : kArcFace112[j] * ((double)size / 112.0);
    return nullptr;
}

size_t align_chip_bytes(int size, int format) { return (size_t)size * size * 3 * (format == 0 ? 1 : sizeof(float)); }

hipError_t launch_align_faces(hipStream_t s, const AlignParams& p) {
    if (p.B < 1 || p.H < 1 || p.W < 2 || p.cap_faces < 0 || p.img_dwords < 2 || (reinterpret_cast<uintptr_t>(p.img) & 3) ||
        (size_t)p.B * p.H * p.W * 3 > p.img_dwords * 4 || p.S < 16 || p.S > kAlignMaxS || (p.S & 3) ||
        (reinterpret_cast<uintptr_t>(p.chips) & (p.format == 0 ? 3 : 15)))
        return hipErrorInvalidValue;
    const long long bands = ((long long)p.S * (p.S >> 2) + kAlignItems - 1) / kAlignItems;
    const long long grid = (long long)(p.cap_faces > 0 ? p.cap_faces : 1) * bands;      // one workgroup at least: it writes the offsets
    if (grid > INT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(align_chips_kernel, dim3((unsigned)grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace cf
