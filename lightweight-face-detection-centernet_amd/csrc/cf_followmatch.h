// The block matching that the follower (cf_follow.hip: follow_kernel) and the lookback's backward trace (cf_lookback.hip: lookback_trace_kernel)
// share, as device functions for one workgroup of 256 threads: the cell means of a window of the luma (phase 1 of the follower's
// statement in include/centerface_hip.h), and the SADs of a 16 x 16 cell template against it with the best displacement's key (phases
// 2 and 3).  Integers throughout.  Both kernels call these very functions, so the two agree in every bit by construction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cf_kernels.h"

namespace cf {

constexpr int kMatchThreads = 256;
constexpr int kWin = kFollowSide + 2 * kFollowMaxSearch;          // 32 cells
constexpr int kWinPitch = kWin / 4 + 1;                            // dwords per window row: the byte-aligning read names one dword past the 32 cells

__device__ inline int luma_bgr(int b, int g, int r) { return (29 * b + 150 * g + 77 * r + 128) >> 8; }

// the luma sum of the pixels x0 .. x0 + n - 1 of a Y row (4-byte aligned), all inside the frame
__device__ inline int run_y(const uint8_t* row, int x0, int n) {
    unsigned s = 0;
    int x = x0;
    const int e = x0 + n;
    for (; x < e && (x & 3); ++x) s += row[x];
    for (; x + 4 <= e; x += 4) s = __builtin_amdgcn_sad_u8(*reinterpret_cast<const uint32_t*>(row + x), 0u, s);
    for (; x < e; ++x) s += row[x];
    return (int)s;
}
// the same of a BGR row: the bytes 3 * x0 .. 3 * (x0 + n) - 1, each dword that holds some of them loaded once and no other
__device__ inline int run_bgr(const uint8_t* row, int x0, int n) {
    const uint32_t* d = reinterpret_cast<const uint32_t*>(row);
    int s = 0, k = 3 * x0, have = -1;
    uint32_t wd = 0;
    for (int i = 0; i < n; ++i) {
        int ch[3];
        for (int q = 0; q < 3; ++q, ++k) {
            if ((k >> 2) != have) { have = k >> 2; wd = d[have]; }
            ch[q] = (int)((wd >> (8 * (k & 3))) & 255u);
        }
        s += luma_bgr(ch[0], ch[1], ch[2]);
    }
    return s;
}

// 1. The rounded cell means of the n x n cells (n <= 32) of c x c pixels whose first pixel is (X0, Y0), in plane 0 of an h x w frame (pitch
//    a multiple of 4, p0 4-byte aligned; bgr: BGR rows, else a Y plane; kMayBgr = false: the caller has Y planes only and passes bgr =
//    false), coordinates clamped into the frame: one byte per cell in s_win, window rows of kWinPitch dwords, the bytes past n zero.
//    A work item is one frame row of one cell; the partial sums are added into s_sum (integer addition: the order does not show).
//    Called by every thread of the workgroup with the same arguments; s_win is complete behind the call.
template <bool kMayBgr>
__device__ inline void match_cell_means(int t, const uint8_t* p0, int pitch0, int h, int w, bool bgr, int X0, int Y0, int n, int c, int* s_sum,
                                        uint32_t* s_win) {
    for (int i = t; i < kWin * kWin; i += kMatchThreads) s_sum[i] = 0;
    for (int i = t; i < kWin * kWinPitch; i += kMatchThreads) s_win[i] = 0;
    __syncthreads();
    const int items = n * c * n;                                   // <= 32 * 512 * 32
    for (int it = t; it < items; it += kMatchThreads) {
        const int r = it / n, ci = it - r * n;
        const int y = min(max(Y0 + r, 0), h - 1), x0 = X0 + ci * c;
        const uint8_t* row = p0 + (size_t)y * pitch0;
        int s = 0;
        if (x0 >= 0 && x0 + c <= w) s = kMayBgr && bgr ? run_bgr(row, x0, c) : run_y(row, x0, c);
        else
            for (int i = 0; i < c; ++i) {
                const int x = min(max(x0 + i, 0), w - 1);
                s += kMayBgr && bgr ? luma_bgr(row[3 * x], row[3 * x + 1], row[3 * x + 2]) : row[x];
            }
        atomicAdd(&s_sum[(r / c) * kWin + ci], s);
    }
    __syncthreads();
    uint8_t* wb = reinterpret_cast<uint8_t*>(s_win);
    const int cc = c * c;
    for (int i = t; i < n * n; i += kMatchThreads) {
        const int j = i / n, ci = i - j * n;
        wb[j * (kWinPitch * 4) + ci] = (uint8_t)((s_sum[j * kWin + ci] + cc / 2) / cc);
    }
    __syncthreads();
}

// 2. + 3. The (2R + 1)^2 <= 289 SADs of the template s_tpl (16 rows of 4 dwords) against the window s_win of 16 + 2R cells, one candidate
//    per thread -- per template row four v_sad_u8 on four packed cells each, the window's bytes brought to the template's alignment by
//    v_alignbyte_b32 --, and the smallest 64-bit key (SAD, dx^2 + dy^2, dy + R, dx + R): xor butterfly in the wave, four keys through
//    s_key.  Called by every thread of the workgroup; EVERY thread returns the workgroup's key (the four words are read by all: a
//    broadcast).  s_key is free again behind the caller's next barrier.
__device__ inline unsigned long long match_best_key(int t, int R, const uint32_t* s_win, const uint32_t* s_tpl, unsigned long long* s_key) {
    const int D = 2 * R + 1;
    unsigned long long best = ~0ull;
    for (int cand = t; cand < D * D; cand += kMatchThreads) {
        const int oy = cand / D, ox = cand - oy * D;               // dy + R, dx + R
        const unsigned shift = ox & 3;
        unsigned sad = 0;
        for (int j = 0; j < kFollowSide; ++j) {
            const uint32_t* wr = s_win + (j + oy) * kWinPitch + (ox >> 2);
            uint32_t lo = wr[0];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t hi = wr[q + 1];                     // (ox >> 2) + 4 <= 8: the row's ninth dword, used only with shift 0, i.e. not at all
                sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, shift), s_tpl[j * 4 + q], sad);
                lo = hi;
            }
        }
        const int dx = ox - R, dy = oy - R;
        const unsigned long long key = ((unsigned long long)sad << 32) | ((unsigned long long)(dx * dx + dy * dy) << 16) | (unsigned)(oy << 8) | (unsigned)ox;
        best = key < best ? key : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned ohi = __shfl_xor((unsigned)(best >> 32), off), olo = __shfl_xor((unsigned)best, off);
        const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
        best = o < best ? o : best;
    }
    if ((t & 63) == 0) s_key[t >> 6] = best;
    __syncthreads();
    best = s_key[0];
#pragma unroll
    for (int q = 1; q < kMatchThreads / 64; ++q) best = s_key[q] < best ? s_key[q] : best;
    return best;
}

// the displacement of a key, in cells
__device__ inline int match_key_sad(unsigned long long key) { return (int)(key >> 32); }
__device__ inline int match_key_dx(unsigned long long key, int R) { return (int)(key & 255) - R; }
__device__ inline int match_key_dy(unsigned long long key, int R) { return (int)((key >> 8) & 255) - R; }

}  // namespace cf
