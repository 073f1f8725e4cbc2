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

namespace cf {
namespace {

constexpr int kAlignMaxS = 512;
constexpr int kAlignItems = 1024;      // groups of 4 chip pixels per workgroup: 4 per thread

struct Similarity { double M[6]; bool ok; };

__device__ __forceinline__ Similarity estimate_inverse(const float* l, const double* q, int S) {
    double px[5], py[5];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        px[i] = (double)l[2 * i]; py[i] = (double)l[2 * i + 1];
        finite = finite && isfinite(px[i]) && isfinite(py[i]);
    }
    const double pmx = ((((px[0] + px[1]) + px[2]) + px[3]) + px[4]) / 5.0, pmy = ((((py[0] + py[1]) + py[2]) + py[3]) + py[4]) / 5.0;
    const double qmx = ((((q[0] + q[2]) + q[4]) + q[6]) + q[8]) / 5.0, qmy = ((((q[1] + q[3]) + q[5]) + q[7]) + q[9]) / 5.0;
    double den = 0.0, na = 0.0, nb = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const double pcx = px[i] - pmx, pcy = py[i] - pmy, qcx = q[2 * i] - qmx, qcy = q[2 * i + 1] - qmy;
        den += pcx * pcx + pcy * pcy;
        na += pcx * qcx + pcy * qcy;
        nb += pcx * qcy - pcy * qcx;
    }
    const double a = na / den, b = nb / den;
    const double tx = qmx - (a * pmx - b * pmy), ty = qmy - (b * pmx + a * pmy);
    const double D = a * a + b * b, ia = a / D, ib = b / D;
    Similarity r;
    r.M[0] = ia; r.M[1] = ib; r.M[2] = -(ia * tx + ib * ty);
    r.M[3] = -ib; r.M[4] = ia; r.M[5] = -(-ib * tx + ia * ty);
    bool ok = finite && den > 0.0 && D > 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) ok = ok && isfinite(r.M[j]);
    if (ok) {
        const double lin = fmax(fmax(fabs(r.M[0]), fabs(r.M[1])), fmax(fabs(r.M[3]), fabs(r.M[4])));
        ok = lin * (double)S + fmax(fabs(r.M[2]), fabs(r.M[5])) < 1048576.0;
    }
    if (!ok) {
#pragma unroll
        for (int j = 0; j < 6; ++j) r.M[j] = 0.0;
    }
    r.ok = ok;
    return r;
}

// the pixels at columns cx and cx + 1 of one row (six contiguous bytes at byte address A) as B | G << 8 | R << 16 each: three
// aligned dword loads funnel-shifted by the address's low bits.  `last` = index of the buffer's last dword (the third load may lie
// past the six bytes, never past the buffer).
__device__ __forceinline__ void fetch_pair(const uint32_t* img, size_t A, size_t last, uint32_t& p0, uint32_t& p1) {
    const size_t i0 = A >> 2;
    const int sh = (int)(A & 3) * 8;
    const uint32_t d0 = img[i0], d1 = img[min(i0 + 1, last)], d2 = img[min(i0 + 2, last)];
    const uint32_t lo = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh), hi = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
    p0 = lo & 0xffffffu;
    p1 = (lo >> 24) | ((hi & 0xffffu) << 8);
}

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
    int off = 0, raw = 0, b = -1, i = 0, row0 = 0;
    for (int k = 0; k < p.B; ++k) {
        const int c = max(p.counts[k], 0);
        int m = min(c, p.rows_cap);
        if (p.max_per_image > 0) m = min(m, p.max_per_image);
        if (b < 0 && n < off + m) { b = k; i = n - off; row0 = raw; }
        if (blockIdx.x == 0 && tid == 0 && p.offsets) p.offsets[k] = off;
        off += m; raw += c;
    }
    if (blockIdx.x == 0 && tid == 0 && p.offsets) p.offsets[p.B] = off;       // the number wanted, whatever cap_faces is
    if (b < 0 || n >= p.cap_faces) return;                                     // uniform: before any barrier
    const size_t row = p.lms_stride > 0 ? (size_t)b * p.lms_stride + i : (size_t)row0 + i;
    const Similarity sim = estimate_inverse(p.lms + row * 10, p.tmpl, S);
    if (band == 0 && tid == 0 && p.mats) {
#pragma unroll
        for (int j = 0; j < 6; ++j) p.mats[(size_t)n * 6 + j] = sim.M[j];
    }
    for (int t = tid; t < S; t += 256) {
        const double v = (double)t;
        tab[t] = (int)rint(sim.M[0] * v * 1024.0);
        tab[kAlignMaxS + t] = (int)rint(sim.M[3] * v * 1024.0);
        tab[2 * kAlignMaxS + t] = (int)rint((sim.M[1] * v + sim.M[2]) * 1024.0) + 16;
        tab[3 * kAlignMaxS + t] = (int)rint((sim.M[4] * v + sim.M[5]) * 1024.0) + 16;
    }
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
            const int X = (X0 + tab[x0 + k]) >> 5, Y = (Y0 + tab[kAlignMaxS + x0 + k]) >> 5;
            const int sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31;
            const int wl = (sx >= 0 && sx < W) ? 32 - fx : 0, wr = (sx >= -1 && sx < W - 1) ? fx : 0;
            const int wt = (sim.ok && sy >= 0 && sy < H) ? 32 - fy : 0, wb = (sim.ok && sy >= -1 && sy < H - 1) ? fy : 0;
            // the six bytes fetched are columns cx, cx + 1; the left neighbour is one of them (or outside), so is the right one
            const int cx = min(max(sx, 0), W - 2);
            const int w0 = (sx == cx ? wl : 0) + (sx + 1 == cx ? wr : 0), w1 = (sx == cx + 1 ? wl : 0) + (sx == cx ? wr : 0);
            uint32_t v = 0;
            if ((wt | wb) != 0 && (w0 | w1) != 0) {
                const int r0 = min(max(sy, 0), H - 1), r1 = min(max(sy + 1, 0), H - 1);
                uint32_t a0, a1, c0, c1;
                fetch_pair(img, (img0 + (size_t)r0 * W + cx) * 3, last, a0, a1);
                fetch_pair(img, (img0 + (size_t)r1 * W + cx) * 3, last, c0, c1);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int s = 8 * c;
                    const int top = w0 * (int)((a0 >> s) & 255) + w1 * (int)((a1 >> s) & 255);
                    const int bot = w0 * (int)((c0 >> s) & 255) + w1 * (int)((c1 >> s) & 255);
                    v |= (uint32_t)((wt * top + wb * bot + 512) >> 10) << s;
                }
            }
            px[k] = v;
        }
        if (p.format == 0) {                                // CF_CHIP_U8_HWC_BGR
            uint32_t* o = reinterpret_cast<uint32_t*>((uint8_t*)p.chips + (((size_t)n * S + y) * S + x0) * 3);
            o[0] = px[0] | (px[1] << 24);
            o[1] = (px[1] >> 8) | (px[2] << 16);
            o[2] = (px[2] >> 16) | (px[3] << 8);
        } else {                                            // CF_CHIP_F32_NCHW: ((float)u8 - mean) * scale, two rounded float32 operations
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int s = 8 * c, plane = p.rgb ? 2 - c : c;
                float4 f;
                f.x = ((float)((px[0] >> s) & 255) - p.mean) * p.scale;
                f.y = ((float)((px[1] >> s) & 255) - p.mean) * p.scale;
                f.z = ((float)((px[2] >> s) & 255) - p.mean) * p.scale;
                f.w = ((float)((px[3] >> s) & 255) - p.mean) * p.scale;
                *reinterpret_cast<float4*>((float*)p.chips + (((size_t)n * 3 + plane) * S + y) * S + x0) = f;
            }
        }
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
