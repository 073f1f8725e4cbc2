// The arithmetic of the aligned face chips (see cf_align.hip for the statement), shared by the chips cut from the network batch
// (cf_align.hip) and the chips cut from the caller's full-resolution frames (cf_align_frame.hip): ONE statement of the similarity
// estimate, of the fixed-point tables, of the bilinear blend and of the chip stores.  Both files are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cf_kernels.h"

namespace cf {

constexpr int kAlignMaxS = 512;
constexpr int kAlignItems = 1024;      // groups of 4 chip pixels per workgroup: 4 per thread

struct Similarity { double M[6]; bool ok; };

// l: the ten landmark values (x, y) x 5 as doubles, in the pixels of the image that is sampled; q: the template points in chip pixels
__device__ __forceinline__ Similarity estimate_inverse(const double* l, const double* q, int S) {
    double px[5], py[5];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        px[i] = l[2 * i]; py[i] = l[2 * i + 1];
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

// The face of workgroup n (n = blockIdx.x / bands): image b, keep position i, and its landmark row.  Every workgroup walks the
// per-image counts (a short uniform loop); workgroup 0 writes the offsets.  false: there is no such face (uniform).
__device__ __forceinline__ bool align_find_face(const AlignParams& p, int n, int& b, size_t& row) {
    const int tid = threadIdx.x;
    int off = 0, raw = 0, i = 0, row0 = 0;
    b = -1;
    for (int k = 0; k < p.B; ++k) {
        const int c = max(p.counts[k], 0);
        int m = min(c, p.rows_cap);
        if (p.max_per_image > 0) m = min(m, p.max_per_image);
        if (b < 0 && n < off + m) { b = k; i = n - off; row0 = raw; }
        if (blockIdx.x == 0 && tid == 0 && p.offsets) p.offsets[k] = off;
        off += m; raw += c;
    }
    if (blockIdx.x == 0 && tid == 0 && p.offsets) p.offsets[p.B] = off;       // the number wanted, whatever cap_faces is
    if (b < 0 || n >= p.cap_faces) return false;
    row = p.lms_stride > 0 ? (size_t)b * p.lms_stride + i : (size_t)row0 + i;
    return true;
}

// the per-column and per-row fixed-point terms of one face: tab = ad | bd | X0 | Y0, kAlignMaxS entries each (LDS); the caller
// synchronises
__device__ __forceinline__ void align_fill_tables(int* tab, const Similarity& sim, int S) {
    for (int t = threadIdx.x; t < S; t += 256) {
        const double v = (double)t;
        tab[t] = (int)rint(sim.M[0] * v * 1024.0);
        tab[kAlignMaxS + t] = (int)rint(sim.M[3] * v * 1024.0);
        tab[2 * kAlignMaxS + t] = (int)rint((sim.M[1] * v + sim.M[2]) * 1024.0) + 16;
        tab[3 * kAlignMaxS + t] = (int)rint((sim.M[4] * v + sim.M[5]) * 1024.0) + 16;
    }
}

// One chip pixel's taps in an H x W image: the two columns fetched are cx, cx + 1 (both inside the image: W >= 2) with weights w0, w1,
// the two rows r0, r1 with weights wt, wb.  A neighbour outside the image has weight 0; the weights of one axis sum to at most 32.
struct AlignTap { int cx, r0, r1, w0, w1, wt, wb; };
__device__ __forceinline__ AlignTap align_tap(int X, int Y, int H, int W, bool ok) {
    const int sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31;
    const int wl = (sx >= 0 && sx < W) ? 32 - fx : 0, wr = (sx >= -1 && sx < W - 1) ? fx : 0;
    AlignTap t;
    t.wt = (ok && sy >= 0 && sy < H) ? 32 - fy : 0; t.wb = (ok && sy >= -1 && sy < H - 1) ? fy : 0;
    // the left neighbour is one of the two columns fetched (or outside), so is the right one
    t.cx = min(max(sx, 0), W - 2);
    t.w0 = (sx == t.cx ? wl : 0) + (sx + 1 == t.cx ? wr : 0); t.w1 = (sx == t.cx + 1 ? wl : 0) + (sx == t.cx ? wr : 0);
    t.r0 = min(max(sy, 0), H - 1); t.r1 = min(max(sy + 1, 0), H - 1);
    return t;
}
__device__ __forceinline__ bool align_tap_live(const AlignTap& t) { return (t.wt | t.wb) != 0 && (t.w0 | t.w1) != 0; }

// the four neighbours (B | G << 8 | R << 16 each; a = row r0, c = row r1) -> the chip pixel
__device__ __forceinline__ uint32_t align_blend(const AlignTap& t, uint32_t a0, uint32_t a1, uint32_t c0, uint32_t c1) {
    uint32_t v = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int s = 8 * c;
        const int top = t.w0 * (int)((a0 >> s) & 255) + t.w1 * (int)((a1 >> s) & 255);
        const int bot = t.w0 * (int)((c0 >> s) & 255) + t.w1 * (int)((c1 >> s) & 255);
        v |= (uint32_t)((t.wt * top + t.wb * bot + 512) >> 10) << s;
    }
    return v;
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

// 4 adjacent chip pixels (x0 .. x0 + 3 of row y of chip n) leave as three dword stores (uint8 HWC) or one float4 per channel (float
// NCHW): S is a multiple of 4
__device__ __forceinline__ void align_store4(const AlignParams& p, int n, int y, int x0, const uint32_t* px) {
    const int S = p.S;
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

}  // namespace cf
