// Last IDAUp stage + the four heads as ONE kernel (bf16 storage, collapsed heads): the 24-channel
// stride-4 neck output lives only in LDS.
//
// Replaces, fused: IDAUp.forward for up3 (model/centernet.py:200-204: relu(bn(conv1x1(skip))) +
// relu(bn_up(deconv2x2(low)))), called at :274) and, per head, Conv2d(24,24,3,padding=1) -> Conv2d(24,c,1)
// (:247-261, :277-279) + the sigmoid/clamp on hm (centerface.py:43).  Layer by layer the neck output is
// written once (79 MB per batch of 64) and read back ~1.5-2x through the 3x3 window; here a workgroup
// computes it for an 8x32 tile plus a one-pixel halo straight into LDS (exactly the bf16 values the
// unfused kernel would store, pixels outside the map = the 3x3 conv's zero padding) and the head conv
// reads its 3 x 72 contiguous elements per output pixel from there.  Same arithmetic, same operation
// order as cf_pw.hip (IDAUp epilogue) followed by cf_head.hip (collapsed), so results are bit-identical
// to the two-kernel path.
#include "cf_exp.h"
#include "cf_common.h"
#include "cf_kernels.h"
#include <algorithm>
#include <atomic>
#include <cstdlib>

namespace cf {

typedef __attribute__((ext_vector_type(8))) __bf16 mfma_bf16x8;

constexpr int UH_TW = 32, UH_IW = UH_TW + 2;      // tile width; the tile height TH and the wave count NW are template parameters

// T = bf16_t (benchmarked mode), sp32_t (tolerance mode: fp32 tile, split-bf16 products) or float (exact fp32 MFMA).
// TH x 32 output tile (TH + 2 halo rows: 10 x 34 = 340 pixels at TH = 8, 18 x 34 = 612 at TH = 16), NW waves; NT: the head
// records (105 MB per batch of 64, read back only at the K decoded cells) are stored non-temporally.
template <typename T, int UH_TH, int NW>
struct Uh {
    static constexpr int P = Elem<T>::PER16;
    static constexpr int PIT = 24 * (int)sizeof(T);                 // bytes per tile pixel: 24 channels
    static constexpr int NC = PIT / 16, NCH = (NC + 1) / 2;        // 1x1 conv: chunks per pixel row / per lane half (k-steps)
    static constexpr int CPD = 3 * NC, SPD = (CPD + 1) / 2;        // head conv: chunks per kernel row (3 pixels) / steps per lane half
    static constexpr int G = 16 / P;                                // channel groups of P per lane (16 output channels)
    static constexpr int IH = UH_TH + 2, IPX = IH * UH_IW, NIB = (IPX + 31) / 32, MAXB = (NIB + NW - 1) / NW;
    static constexpr int T3B = NIB * 32 * PIT, WHB = 3 * SPD * 1024, RSB = NW * 2048;
    static constexpr int LDS = T3B + WHB + RSB;
};

template <typename T, bool COALESCE, int UH_TH = 8, int NW = 4, bool NT = false>
__global__ __launch_bounds__(NW * 64) void uphead_kernel(UpHeadParams p) {
    typedef Uh<T, UH_TH, NW> U;
    constexpr int P = U::P, PIT = U::PIT, NC = U::NC, NCH = U::NCH, CPD = U::CPD, SPD = U::SPD, G = U::G;
    constexpr int UH_IPX = U::IPX, UH_NIB = U::NIB, MAXB = U::MAXB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* T3 = smem;                       // neck tile incl. halo, storage type T
    char* Wh = smem + U::T3B;              // head weight fragments
    char* Rs = Wh + U::WHB;                // one row of 32 records per wave, staged for full-line stores
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pl = lane & 31, h = lane >> 5;
    unsigned tbx = blockIdx.x, tby = blockIdx.y, tbz = blockIdx.z;
    if (p.xcd) xcd_tile_order(tbx, tby, tbz);       // the 3x3 halo rows and the half-resolution `low` rows are shared by neighbours
    const int ox0 = tbx * UH_TW, oy0 = tby * UH_TH, b = tbz;

    // head weights -> LDS by DMA; lands under phase A, fenced by the barrier
    for (int c = wave; c < U::WHB / 1024; c += NW)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)((const char*)p.w0p + c * 1024 + lane * 16),
                                         (__attribute__((address_space(3))) void*)(Wh + c * 1024), 16, 0, 0);

    // ---- phase A: up3 on the halo tile.  1x1 conv 24 -> 24 as in cf_pw.hip (lane half h owns chunks h NCH .. of the pixel row; a
    // chunk past the row meets a zeroed operand), epilogue bias + ReLU, + ReLU(low * tap weight + shift), storage type -> LDS
    u32x4 wc[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) wc[j] = ld16((const char*)p.wcv + (size_t)(j * 64 + lane) * 16);
    // All global loads of this wave's halo blocks are issued before the first result is consumed; padding selects are applied
    // afterwards, on the registers.
    u32x4 xs[MAXB][NCH], lw[MAXB][G];
    bool valid[MAXB]; int tapv[MAXB];
#pragma unroll
    for (int t = 0; t < MAXB; ++t) {
        const int ib = wave + NW * t;
        const int ip = ib * 32 + pl;
        const int ipc = ip < UH_IPX ? ip : UH_IPX - 1;
        const int ty = ipc / UH_IW, tx = ipc - ty * UH_IW;
        const int gy = oy0 - 1 + ty, gx = ox0 - 1 + tx;
        valid[t] = ib < UH_NIB && ip < UH_IPX && (unsigned)gy < (unsigned)p.h && (unsigned)gx < (unsigned)p.w;
        const int cy = min(max(gy, 0), p.h - 1), cx = min(max(gx, 0), p.w - 1);
        const char* xrow = (const char*)p.skip + (((size_t)b * p.h + cy) * p.w + cx) * PIT;
#pragma unroll
        for (int j = 0; j < NCH; ++j) xs[t][j] = ld16(xrow + min(h * NCH + j, NC - 1) * 16);      // a chunk past the row: zeroed below
        const size_t low_row = ((size_t)b * (p.h >> 1) + (cy >> 1)) * (p.w >> 1) + (cx >> 1);
        tapv[t] = ((cy & 1) << 1) | (cx & 1);
#pragma unroll
        for (int g = 0; g < G; ++g) lw[t][g] = ld16((const char*)p.low + (low_row * 24 + min(h * 16 + g * P, 24 - P)) * sizeof(T));
    }
#pragma unroll
    for (int t = 0; t < MAXB; ++t) {
        const int ib = wave + NW * t;
        if (ib >= UH_NIB) break;
        const int ip = ib * 32 + pl;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        mma_chain<T, NCH>(acc, [&](int j) { return wc[j]; }, [&](int j) { return (h * NCH + j) < NC ? xs[t][j] : zero16(); });
        const int tap = tapv[t];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int ch = h * 16 + g * P;
            if (ch >= 24) break;
            float v[P], r[P];
#pragma unroll
            for (int e = 0; e < P; ++e) v[e] = relu_f(acc[g * P + e] + p.bias[ch + e]);
            unpack16<T>(lw[t][g], r);
#pragma unroll
            for (int e = 0; e < P; ++e) v[e] += relu_f(r[e] * p.upw[tap * 24 + ch + e] + p.upb[ch + e]);
            u32x4 o = pack16<T>(v);
            if (!valid[t]) o = zero16();
            st16(T3 + ip * PIT + ch * (int)sizeof(T), o);
        }
    }
    cf_sync_lds_dma();            // the tile is complete and the head weights (LDS-DMA) have landed for every wave

    // ---- phase B: collapsed 3x3 head conv from the LDS tile (cf_head.hip: kernel row dy = 72 contiguous elements = CPD chunks;
    // lane half h owns chunks h SPD ..)
    for (int ob = wave; ob < UH_TH * UH_TW / 32; ob += NW) {
        const int o = ob * 32 + pl;
        const int oy = o / UH_TW, ox = o - oy * UH_TW;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const char* row = T3 + ((oy + dy) * UH_IW + ox) * PIT;
            mma_chain<T, SPD>(acc, [&](int j) { return ld16(Wh + ((dy * SPD + j) * 64 + lane) * 16); },
                              [&](int j) { const int c = h * SPD + j; u32x4 xc = ld16(row + (c < CPD ? c : CPD - 1) * 16);
                                           if (c >= CPD) xc = zero16(); return xc; });
        }
        const int gy = oy0 + oy, gx = ox0 + ox;
        if constexpr (!COALESCE) { if (gy >= p.h || gx >= p.w) continue; }
        // head_pack_weights(collapsed = 2): MFMA row = record slot, so lane half h holds slots 4h..4h+3 (acc 0-3) and
        // 8+4h..8+4h+3 (acc 4-7) of its pixel: every lane stores two 16-byte pieces and a 64-byte record is written by
        // two store instructions of the wave instead of four half-empty ones.  Slot 15 = the raw hm logit (slot 0's
        // weights again: identical arithmetic), slot 0 = its clamped sigmoid.
        float out[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) { out[r] = acc[r] + p.b0[h * 4 + r]; out[4 + r] = acc[4 + r] + p.b0[8 + h * 4 + r]; }
        const size_t m = ((size_t)b * p.h + gy) * p.w + gx;
        const bool inmap = gy < p.h && gx < p.w;
        if (h == 0) {
            // centerface.py:43: clamp(sigmoid(hm), 1e-4, 1 - 1e-4); precise exp + IEEE divide
            float sg = 1.0f / (1.0f + expf(-out[0]));
            sg = fminf(fmaxf(sg, 1e-4f), 1.0f - 1e-4f);
            out[0] = sg;
            if (p.hm_plane && inmap) p.hm_plane[m] = sg;
        }
        if constexpr (COALESCE) {
            // a pixel block is one tile row of 32 cells = 2 KB of consecutive records: staged through LDS so that every store
            // instruction of the wave writes 1 KB of consecutive bytes instead of 64 16-byte pieces 64 bytes apart
            char* rs = Rs + wave * 2048;
            st16(rs + pl * 64 + h * 16, pack16<float>(&out[0]));
            st16(rs + pl * 64 + 32 + h * 16, pack16<float>(&out[4]));
            __builtin_amdgcn_wave_barrier();
            if (gy < p.h) {                                                     // wave-uniform (oy is)
                char* row0 = (char*)(p.heads + (((size_t)b * p.h + gy) * p.w + ox0) * 16);
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int q = lane + 64 * k;                                // 16-byte piece q of the row: record q / 4
                    const u32x4 v = ld16(rs + q * 16);
                    if (ox0 + (q >> 2) < p.w) {
                        if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(row0 + q * 16));
                        else st16(row0 + q * 16, v);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if constexpr (!COALESCE) {
            float* dst = p.heads + m * 16 + h * 4;
            st16(dst, pack16<float>(&out[0]));
            st16(dst + 8, pack16<float>(&out[4]));
        }
    }
}

// ---- bf16 (the benchmarked mode): a workgroup walks a RUN of 16 x 32 tiles instead of one.  Tiles are numbered image -> tile column ->
// tile row, workgroup w of G owns tiles [w T / G, (w + 1) T / G): consecutive tiles of a run are vertically adjacent except where a
// column or an image ends.  Once per workgroup: the head-weight DMA, the 1x1 conv fragments, the per-lane tile coordinates (tile origins
// are multiples of 16 / 32, so a lane's (ty, tx), its deconv tap and its LDS cell are the same for every tile) and the bias / tap / shift
// tables, which live in LDS (as neck_kernel's Tb) instead of being read from global memory behind the MFMA.  Per tile: the global loads of
// tile k + 1 are issued before phase B of tile k and consumed by phase A of tile k + 1, so the memory round trip runs under the head conv
// and its record stores; where tile k + 1 lies directly below tile k, its halo rows 0-1 are tile k's rows 16-17 and are copied inside LDS
// instead of being fetched and computed again.  The arithmetic of a pixel is that of uphead_kernel<bf16_t, true, 16, 8, true>, operation
// for operation.
struct UhRuns {
    typedef Uh<bf16_t, 16, 8> U;
    static constexpr int NW = 8, TH = 16, IH = TH + 2;
    static constexpr int TBF = 24 + 96 + 24 + 16;                  // floats: bias | upw[4][24] | upb | b0
    static constexpr int TB_OFF = U::LDS, WC_OFF = TB_OFF + TBF * 4, LDS = WC_OFF + 2048;          // the tables; the 1x1 conv fragments
    static constexpr int ROW_B = UH_IW * U::PIT;                   // one tile row in LDS
    static constexpr int SHARED_CHUNKS = 2 * ROW_B / 16;           // rows 16-17 -> rows 0-1
    static_assert(U::MAXB == 3 && U::NIB == 20 && U::NCH == 2 && U::G == 2 && U::SPD == 5 && U::CPD == 9, "written out for this geometry");
    static_assert(SHARED_CHUNKS <= NW * 64 && WC_OFF % 16 == 0 && TB_OFF % 16 == 0, "one chunk per thread; 16-byte LDS reads");
};

// LDS-only barrier: every LDS access of this wave has completed, then s_barrier.  (The workgroup fence of __syncthreads() may also wait
// for the vector-memory counter, and the prefetch loads and record stores are exactly what must stay in flight across the barrier.)
__device__ __forceinline__ void uh_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Buffer access with the hardware range check as the predicate: an offset at or past the descriptor's byte count reads zeros / stores
// nothing, and the instruction is issued all the same (uphead_runs_kernel relies on fixed instruction counts per tile).
typedef __amdgpu_buffer_rsrc_t uh_rsrc_t;
constexpr unsigned UH_OOB = 0x80000000u;
__device__ __forceinline__ uh_rsrc_t uh_rsrc(const void* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
typedef __attribute__((ext_vector_type(4))) unsigned int uh_v4u;
__device__ __forceinline__ u32x4 uh_bload(uh_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}
__device__ __forceinline__ void uh_bstore_nt(const u32x4& v, uh_rsrc_t r, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uh_v4u, v), r, (int)off, 0, 2);      // aux 2 = nt
}
__device__ __forceinline__ void uh_bstore32(unsigned v, uh_rsrc_t r, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b32(v, r, (int)off, 0, 0);
}

__global__ __launch_bounds__(UhRuns::NW * 64) __attribute__((amdgpu_waves_per_eu(4)))
void uphead_runs_kernel(UpHeadParams p, int TX, int TY, unsigned tq, unsigned tr) {
    typedef UhRuns R;
    typedef R::U U;
    typedef bf16_t T;
    constexpr int PIT = U::PIT, NW = R::NW, UH_TH = R::TH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* T3 = smem;
    char* Wh = smem + U::T3B;
    char* Rs = Wh + U::WHB;
    float* Tb = reinterpret_cast<float*>(smem + R::TB_OFF);
    char* Wc = smem + R::WC_OFF;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pl = lane & 31, h = lane >> 5;

    // this workgroup's run: tiles [t, t1) = [floor(w T / G), floor((w + 1) T / G)) with T = tq G + tr
    const unsigned G = gridDim.x, wg = blockIdx.x;
    unsigned t = wg * tq + wg * tr / G;
    const unsigned t1 = (wg + 1) * tq + (wg + 1) * tr / G;
    int b, col, row;
    { const unsigned per = (unsigned)(TX * TY), bi = t / per, rem = t - bi * per, ci = rem / (unsigned)TY;
      b = (int)bi; col = (int)ci; row = (int)(rem - ci * (unsigned)TY); }

    // per lane, the same for every tile: halo pixel (ty, tx) of its three blocks (a block past the tile gets ty >= 18: never valid); its
    // offsets from the pixel above-left of the tile origin in skip and in low and its deconv tap follow from it
    int tyx[3];
    const int wl = p.w >> 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ip = (wave + NW * k) * 32 + pl;
        const int ty = ip / UH_IW, tx = ip - ty * UH_IW;
        tyx[k] = (ty << 8) | tx;
    }
    const int cell0 = (wave * 32 + pl) * PIT;                      // block k: + k * NW * 32 * PIT
    const char* brow = T3 + (wave * UH_IW + pl) * PIT + h * (U::SPD * 16);       // phase B: output row `wave` (+ 8), lane half's chunks

    u32x4 xs[3][2], lw[3][2];
    // the halo rows / columns of tile (col, row) that lie inside the map
    auto bounds = [&](int col_, int row_, int& ylo, int& ynum, int& xlo, int& xnum) {
        const int oy0 = row_ * UH_TH, ox0 = col_ * UH_TW;
        ylo = oy0 == 0 ? 1 : 0; ynum = min(R::IH, p.h - oy0 + 1) - ylo;
        xlo = ox0 == 0 ? 1 : 0; xnum = min(UH_IW, p.w - ox0 + 1) - xlo;
    };
    // All global loads of a tile, as buffer loads through a descriptor of the tile's window: a lane with nothing to fetch (a pixel outside
    // the map, the chunk past the row, a block the previous tile already holds, no tile at all) gets an offset past the window, which
    // the range check answers with zeros without touching memory.  Every wave therefore issues the same twelve instructions for every
    // tile and the compiler's vmcnt waits in phase A are exact counts that leave the record stores behind them in flight.
    // `shared`: rows 0-1 come from the previous tile (blocks 0 and 1 are those rows only)
    auto issue = [&](int b_, int col_, int row_, bool shared, bool any) {
        int ylo, ynum, xlo, xnum; bounds(col_, row_, ylo, ynum, xlo, xnum);
        const int oy0 = row_ * UH_TH, ox0 = col_ * UH_TW;
        // the window starts at the pixel above-left of the tile origin; that may lie before the tensor, a valid lane's offset leads inside
        const long long sb = (((long long)b_ * p.h + oy0 - 1) * p.w + ox0 - 1) * PIT;
        const long long lb = (((long long)b_ * (p.h >> 1) + (oy0 >> 1) - 1) * wl + (ox0 >> 1) - 1) * PIT;
        const uh_rsrc_t sk = uh_rsrc((const char*)p.skip + sb, any ? (R::IH * p.w + UH_IW) * PIT : 0);
        const uh_rsrc_t lo = uh_rsrc((const char*)p.low + lb, any ? ((R::IH / 2 + 1) * wl + UH_IW / 2 + 1) * PIT : 0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int ty = tyx[k] >> 8, tx = tyx[k] & 255;
            const bool ok = (unsigned)(ty - ylo) < (unsigned)ynum && (unsigned)(tx - xlo) < (unsigned)xnum && !(shared && wave + NW * k < 2);
            // lane half h: chunks 2h, 2h + 1 (chunk 3 does not exist)
            const unsigned xo = ok ? (unsigned)((ty * p.w + tx) * PIT + h * 32) : UH_OOB;
            const unsigned lo_ = ok ? (unsigned)((((ty + 1) >> 1) * wl + ((tx + 1) >> 1)) * PIT + h * 32) : UH_OOB;
            xs[k][0] = uh_bload(sk, xo); lw[k][0] = uh_bload(lo, lo_);
            xs[k][1] = uh_bload(sk, h == 0 ? xo + 16 : UH_OOB); lw[k][1] = uh_bload(lo, h == 0 ? lo_ + 16 : UH_OOB);
        }
    };
    // ---- phase A (uphead_kernel's, from the prefetched registers and the LDS tables)
    auto phase_a = [&](int col_, int row_, bool shared) {
        int ylo, ynum, xlo, xnum; bounds(col_, row_, ylo, ynum, xlo, xnum);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int ib = wave + NW * k;
            if (ib >= U::NIB) break;
            if (shared && ib < 2) continue;
            const int ty = tyx[k] >> 8, tx = tyx[k] & 255;
            const bool valid = (unsigned)(ty - ylo) < (unsigned)ynum && (unsigned)(tx - xlo) < (unsigned)xnum;
            const bool keep = !(shared && ty < 2);             // block 2 holds four pixels of row 1
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            mma_chain<T, 2>(acc, [&](int j) { return ld16(Wc + (j * 64 + lane) * 16); }, [&](int j) { return xs[k][j]; });
            const int tap = (((ty + 1) & 1) << 1) | ((tx + 1) & 1);       // parity of the map row / column (origins are even)
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const int ch = h * 16 + g * 8;
                if (ch >= 24) break;
                float v[8], r[8];
                unpack16<T>(lw[k][g], r);
#pragma unroll
                for (int q = 0; q < 8; q += 4) {               // the tables four channels at a time: twelve registers, not twenty-four
                    float bs[4], uw[4], ub[4];
                    unpack16<float>(ld16(Tb + ch + q), bs);
                    unpack16<float>(ld16(Tb + 24 + tap * 24 + ch + q), uw);
                    unpack16<float>(ld16(Tb + 120 + ch + q), ub);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[q + e] = relu_f(acc[g * 8 + q + e] + bs[e]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[q + e] += relu_f(r[q + e] * uw[e] + ub[e]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                u32x4 o = pack16<T>(v);
                if (!valid) o = zero16();
                if (keep) st16(T3 + cell0 + k * (NW * 32 * PIT) + ch * (int)sizeof(T), o);
            }
        }
    };

    // the first tile's loads go out first, the once-per-workgroup pieces behind them: head weights and conv fragments by LDS-DMA, the tables
    issue(b, col, row, false, true);
    for (int c = wave; c < U::WHB / 1024; c += NW)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)((const char*)p.w0p + c * 1024 + lane * 16),
                                         (__attribute__((address_space(3))) void*)(Wh + c * 1024), 16, 0, 0);
    if (wave < 2)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)((const char*)p.wcv + wave * 1024 + lane * 16),
                                         (__attribute__((address_space(3))) void*)(Wc + wave * 1024), 16, 0, 0);
    if (tid < R::TBF) Tb[tid] = tid < 24 ? p.bias[tid] : tid < 120 ? p.upw[tid - 24] : tid < 144 ? p.upb[tid - 120] : p.b0[tid - 144];

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // this wave's LDS-DMAs have landed (phase A is about to wait for the loads anyway)
    uh_lds_barrier();
    phase_a(col, row, false);
    for (;;) {
        uh_lds_barrier();                                          // the tile is complete

        // ---- the next tile of the run: its loads go out now and come back under phase B
        const bool more = t + 1 < t1;
        int nb = b, ncol = col, nrow = row + 1;
        bool nshared = more;
        if (nrow == TY) { nrow = 0; nshared = false; if (++ncol == TX) { ncol = 0; ++nb; } }
        issue(nb, ncol, nrow, nshared, more);

        // ---- phase B (uphead_kernel's): output rows `wave` and `wave + 8` of the tile, one block of 32 cells each
        const int ox0 = col * UH_TW, oy0 = row * UH_TH;
        const int wcells = min(UH_TW, p.w - ox0);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int oy = wave + NW * i;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const char* rp = brow + (NW * i + dy) * R::ROW_B;
                // the tenth chunk (upper lane half, j = 4) does not exist: what is read there (inside T3) is replaced by zeros
                mma_chain<T, 5>(acc, [&](int j) { return ld16(Wh + ((dy * 5 + j) * 64 + lane) * 16); },
                                [&](int j) { u32x4 xc = ld16(rp + j * 16); if (j == 4 && h) xc = zero16(); return xc; });
            }
            const int gy = oy0 + oy;
            float b0a[4], b0b[4], out[8];
            unpack16<float>(ld16(Tb + 144 + h * 4), b0a); unpack16<float>(ld16(Tb + 152 + h * 4), b0b);
#pragma unroll
            for (int r = 0; r < 4; ++r) { out[r] = acc[r] + b0a[r]; out[4 + r] = acc[4 + r] + b0b[r]; }
            if (h == 0) {
                float sg = 1.0f / (1.0f + expf(-out[0]));
                sg = fminf(fmaxf(sg, 1e-4f), 1.0f - 1e-4f);
                out[0] = sg;
            }
            // the stores go through descriptors of this map row's cells inside the tile (none when the row is below the map): the range
            // check drops the rest, and the store count per tile is the same for every wave
            const size_t mrow = ((size_t)b * p.h + gy) * p.w + ox0;
            const int ncell = gy < p.h ? wcells : 0;
            uh_bstore32(__float_as_uint(out[0]), uh_rsrc(p.hm_plane + mrow, p.hm_plane ? ncell * 4 : 0), h == 0 ? (unsigned)(pl * 4) : UH_OOB);
            char* rs = Rs + wave * 2048;
            st16(rs + pl * 64 + h * 16, pack16<float>(&out[0]));
            st16(rs + pl * 64 + 32 + h * 16, pack16<float>(&out[4]));
            __builtin_amdgcn_wave_barrier();
            const uh_rsrc_t hr = uh_rsrc(p.heads + mrow * 16, ncell * 64);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int q = lane + 64 * k;                                // 16-byte piece q of the row: record q / 4
                uh_bstore_nt(ld16(rs + q * 16), hr, (unsigned)(q * 16));
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (!more) break;
        u32x4 keep2 = zero16();
        const bool copies = nshared && tid < R::SHARED_CHUNKS;
        if (copies) keep2 = ld16(T3 + (R::IH - 2) * R::ROW_B + tid * 16);
        uh_lds_barrier();                                          // every wave is done reading the tile
        if (copies) st16(T3 + tid * 16, keep2);
        b = nb; col = ncol; row = nrow; ++t;
        phase_a(col, row, nshared);
    }
}

template <typename T, bool CO, int TH, int NW, bool NT>
static hipError_t uphead_launch_t(hipStream_t s, const UpHeadParams& q) {
    typedef Uh<T, TH, NW> U;
    dim3 grid((q.w + UH_TW - 1) / UH_TW, (q.h + TH - 1) / TH, q.B), blk(NW * 64);
    set_kernel_tag("void cf::uphead_kernel<%s, %s, %d, %d, %s>(cf::UpHeadParams)", type_tag<T>(), CO ? "true" : "false", TH, NW, NT ? "true" : "false");
    return launch_lds<uphead_kernel<T, CO, TH, NW, NT>>(grid, blk, U::LDS, s, q);
}

// Workgroups of uphead_runs_kernel the device holds at once: two per CU (61.6 KB of LDS and 8 waves of <= 128 VGPRs each).  The CU count
// is asked once per device.
static int uphead_slots() {
    static std::atomic<int> cus[32];
    int dev = 0; (void)hipGetDevice(&dev);
    std::atomic<int>& slot = cus[dev & 31];
    int n = slot.load(std::memory_order_relaxed);
    if (n <= 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 1;
        slot.store(n, std::memory_order_relaxed);
    }
    return 2 * std::min(n, 16384);
}

// G = min(T, slots) workgroups, workgroup w walks tiles [w T / G, (w + 1) T / G): with T <= slots every workgroup has one tile and every
// tile its own workgroup (single images and small batches lose no CUs), above that the runs differ by at most one tile.
static hipError_t uphead_runs_launch(hipStream_t s, const UpHeadParams& q) {
    const int TX = (q.w + UH_TW - 1) / UH_TW, TY = (q.h + UhRuns::TH - 1) / UhRuns::TH;
    const long long T = (long long)TX * TY * q.B;
    if (T > 0x7fffffffLL) return hipErrorInvalidValue;
    const unsigned G = (unsigned)std::min<long long>(T, uphead_slots());
    set_kernel_tag("cf::uphead_runs_kernel(cf::UpHeadParams, int, int, unsigned int, unsigned int)");
    return launch_lds<uphead_runs_kernel>(dim3(G), dim3(UhRuns::NW * 64), UhRuns::LDS, s, q, TX, TY, (unsigned)(T / G), (unsigned)(T % G));
}

hipError_t launch_uphead(hipStream_t s, int dtype, const UpHeadParams& p) {
    if (p.B <= 0) return hipSuccess;
    static const bool xcd_on = cf_ab_int("CF_UH_XCD", 0) >= 1;      // A/B only: 0.090 -> 0.094 ms with it
    UpHeadParams q = p; q.xcd = xcd_on ? 1 : 0;
#include CF_EXP_INC(cf_uphead_0)
    // bf16: 16 x 32 tiles on eight waves, non-temporal record stores, a run of tiles per workgroup (uphead_runs_kernel: 115 VGPRs, no
    // scratch, 65,152 B of LDS, two workgroups per CU).  B = 64, 640x640, same box and session, parent build against this one: rocprofv3
    // 72.7 -> 58.5 us per launch (23 launches each), HIP events 76.1 -> 61.9 us, bench step 1.1714 / 1.1714 -> 1.1619 / 1.1606 ms
    // (profiles/r08_uphead_runs.md).  The one-tile geometry before it was chosen on HIP events: 8x32 / 4 waves 79.0 us, + non-temporal
    // 78.1, 16x32 / 8 waves 73.2, + non-temporal 72.3; 16x32 / 4 waves 84.9, 32x32 / 8 waves 86.4, 8x32 / 8 waves 91.4.  Every variant is
    // bit-identical to the two-kernel path (test_fused_up3_heads_..., tests/test_uphead_runs.py).  XCD-aware tile order of the one-tile
    // kernel was measured slower (0.090 -> 0.094 ms) and is not offered for the runs.
    if (dtype == 1) return uphead_runs_launch(s, q);
    // fp32 tile (twice the LDS per pixel): 8 x 32 tiles on eight waves, 77.8 KB = two workgroups per CU.  B = 64, 640x640: 0.132 ms
    // (four waves 0.154, 16x32 / 8 waves 0.159, 4x32 / 4 waves 0.187) against 0.103 + 0.149 for the two launches
    if (dtype == 2) return uphead_launch_t<sp32_t, true, 8, 8, true>(s, q);
    return uphead_launch_t<float, true, 8, 4, true>(s, q);
}

}  // namespace cf
