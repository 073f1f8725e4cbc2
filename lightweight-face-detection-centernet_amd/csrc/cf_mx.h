// Matrix-core depthwise building blocks shared by cf_mbconv3.hip and cf_stem0.hip (see the header comment of cf_mbconv3.hip):
// quad-cell tile E[halo quad][channel][4 x fp16], Toeplitz A operands on v_mfma_f32_4x4x4_16b_f16, the lane -> output-quad
// table that keeps ds_read_b128 conflict-free, compiler-visible bf16 packing for MFMA operands.
#pragma once
#include "cf_common.h"

namespace cf {

typedef __attribute__((ext_vector_type(8))) __bf16 mfma_bf16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 mfma_f16x4;
static constexpr float kNegLog2e3 = -1.44269504088896341f, kNegLn23 = -0.69314718055994531f;

// two fp32 -> packed bf16x2 (RNE) through the compiler's own v_cvt_pk_bf16_f32 selection, NOT the inline-asm pack_bf16x2 of
// cf_common.h: here the packed dwords are MFMA operands a few instructions later, and hipcc pads no VALU-write -> MFMA-read
// wait states for a register written inside an asm statement (seen as stale project operands on ~half the waves)
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_v;
__device__ __forceinline__ uint32_t packb(float lo, float hi) {
    f32x2 v; v.x = lo; v.y = hi;
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_v));
}
__device__ __forceinline__ u32x4 pack16b(const float* f) {
    u32x4 c; c.x = packb(f[0], f[1]); c.y = packb(f[2], f[3]); c.z = packb(f[4], f[5]); c.w = packb(f[6], f[7]); return c;
}

__device__ __forceinline__ f32x2 swish2_pre(f32x2 u) {      // u = -log2(e) x  ->  u / (1 + 2^u) = -log2(e) swish(x)
    f32x2 e; e.x = __builtin_amdgcn_exp2f(u.x); e.y = __builtin_amdgcn_exp2f(u.y);
    const f32x2 den = e + 1.0f;
    f32x2 r; r.x = __builtin_amdgcn_rcpf(den.x); r.y = __builtin_amdgcn_rcpf(den.y);
    return u * r;
}

// ---- the vocabulary of the matrix-core kernels (expdw_mx_kernel, mbconv_mx_kernel, mbconv_mx2_kernel, stem0_mx_kernel and the
// experiments variants): every block is the text its callers used to carry, inlined; profiles/mx_vocab_refactor.md compares the assembly

// one quad cell: four fp32 (= -log2(e) x) -> Swish -> fp16 round-toward-zero -> one 8-byte LDS store; swish = false only under CF_ABLATION
__device__ __forceinline__ void mx_cell_store(char* dst, float a0, float a1, float a2, float a3, bool swish = true) {
    f32x2 y0, y1; y0.x = a0; y0.y = a1; y1.x = a2; y1.y = a3;
    if (swish) { y0 = swish2_pre(y0); y1 = swish2_pre(y1); }
    u32x2 d;
    d.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(y0.x, y0.y));
    d.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(y1.x, y1.y));
    *reinterpret_cast<u32x2*>(dst) = d;
}
// the four cells of expand block ib in linear pixel order: D rows (r & 3) + 8 (r >> 2) + 4 h, so register quad tq of lane (channel pl,
// half h) is halo quad ib * 8 + 2 tq + h
template <int CP>
__device__ __forceinline__ void mx_block_store(char* E, int ib, int h, int pl, const f32x16& a, bool swish = true) {
    char* ecell = E + (unsigned)(ib * 8 + h) * (unsigned)CP + pl * 8;
#pragma unroll
    for (int tq = 0; tq < 4; ++tq) mx_cell_store(ecell + 2 * tq * CP, a[4 * tq], a[4 * tq + 1], a[4 * tq + 2], a[4 * tq + 3], swish);
}

// Swish over the depthwise accumulators acc[NG][4] (= -log2(e) x); SCALE: the leftover factor out again (a consumer with plain weights).
// expdw_mx_kernel keeps its own text of the SCALE form: through this function all 36 of its instances come out with other assembly
template <int NG, bool SCALE = false>
__device__ __forceinline__ void mx_swish_acc(f32x4* acc) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
            f32x2 u; u.x = acc[g][i]; u.y = acc[g][i + 1];
            f32x2 y = swish2_pre(u);
            if constexpr (SCALE) y = y * kNegLn23;
            acc[g][i] = y.x; acc[g][i + 1] = y.y;
        }
}

// the lane's eight (four) channels of output pixel i as bf16: a 16-byte store or a project MFMA B fragment
__device__ __forceinline__ u32x4 mx_pack8(const f32x4* acc, int i) {
    u32x4 d;
    d.x = packb(acc[0][i], acc[1][i]); d.y = packb(acc[2][i], acc[3][i]);
    d.z = packb(acc[4][i], acc[5][i]); d.w = packb(acc[6][i], acc[7][i]);
    return d;
}
__device__ __forceinline__ u32x2 mx_pack4(const f32x4* acc, int i) {
    u32x2 d; d.x = packb(acc[0][i], acc[1][i]); d.y = packb(acc[2][i], acc[3][i]);
    return d;
}

// BYTES (whole KiB) from global memory straight into LDS, the KiB chunks dealt over the caller's NW waves (global_load_lds, 16 bytes
// per lane; uses the caller's wave and lane).  A macro: as a function the loop is canonicalised before it is inlined, without the
// caller's ranges of wave and lane, and all 40 kernels of cf_mbconv3.hip come out with other assembly (the fused ones two lines longer)
#define CF_MX_STAGE(SRC, DST, BYTES)                                                                                              \
    do {                                                                                                                          \
        char* stage_dst = (DST);                                                                                                  \
        const char* stage_src = (SRC);                                                                                            \
        for (int c = wave; c < (BYTES) / 1024; c += NW)                                                                           \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(stage_src + c * 1024 + lane * 16),   \
                                             (__attribute__((address_space(3))) void*)(stage_dst + c * 1024), 16, 0, 0);          \
    } while (0)

// (The expand block -- a zeroed f32x16 and the JX-long chain of v_mfma_f32_32x32x16_bf16 against weight fragments in LDS -- stays
// written out in every kernel: as a function, with either form of the fragment address or a callable for it, the nine
// expdw_mx_kernel<5, 4, 10, 40, 8> instances gain 24 to 46 instructions and both layer1.1 instances of mbconv_mx_kernel come out with
// other assembly, the general ones included, which no test at small shapes can reach: profiles/mx_vocab_refactor.md.)

// N register-resident Toeplitz operand pairs (a [2][KS][2], [KS][2] or [KS][KSTEPS] array, flat), 64 lanes apart; at = table + lane
template <int N>
__device__ __forceinline__ void mx_load_taps(u32x2* A, const u32x2* at) {
#pragma unroll
    for (int n = 0; n < N; ++n) A[n] = at[n * 64];
}

// Swish + cell stores of expand block t of wave w under HaloDeal<KS> (cf_common.h); a = the block's 32x32 expand accumulators (lane =
// channel pl of lane half h, register quad tq = rows 8 tq + 4 h ..).  Every cell the depthwise reads is written, every round: the dead
// column pair of a 3x3 halo's quad 4 as ZERO, never left to what the workgroup before had in those bytes (the depthwise multiplies it
// by a zero weight, and 0 * NaN is NaN).  Register quads without a cell are neither activated nor stored; every test is on w, t, tq.
template <int KS, int CP>
__device__ __forceinline__ void halo_deal_store(char* E, int w, int t, int h, int pl, const f32x16& a) {
    typedef HaloDeal<KS> D;
    constexpr int RP = 2 * D::IWQ * CP;                             // bytes from a row pair to the next
    auto full = [&](int tq, char* dst) { mx_cell_store(dst, a[4 * tq], a[4 * tq + 1], a[4 * tq + 2], a[4 * tq + 3]); };
    auto half = [&](float ux, float uy, char* dst) {
        f32x2 u; u.x = ux; u.y = uy;
        const f32x2 y = swish2_pre(u);
        u32x2 d;
        d.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(y.x, y.y));
        d.y = 0u;
        *reinterpret_cast<u32x2*>(dst) = d;
    };
    // ONE vector base for all blocks (row h of row pair 0, quad 0, the lane's channel) + the block's wave-uniform byte offset, added
    // where it is used: a base per block, hoisted out of the round loop, costs the fused kernels their occupancy step
    char* const lane0 = E + h * (D::IWQ * CP) + pl * 8;
    auto at = [&](int so) -> char* { asm volatile("" : "+s"(so)); return lane0 + so; };
    if (t < 2 || (KS == 5 && t == 2 && w < 2)) {
        char* e = at((4 * t + w) * RP);
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) full(tq, e + tq * CP);
    } else if constexpr (KS == 3) {
        if (w < 2) {
            char* e = at(8 * RP + 2 * w * CP);
            full(0, e); full(1, e + CP);
        } else {
            const int np = D::side_pairs(w);
            char* e = at(4 * (w - 2) * RP + 4 * CP);
#pragma unroll
            for (int tq = 0; tq < 4; ++tq) {
                if (2 * tq >= np) break;
                half(a[4 * tq], a[4 * tq + 1], e + 2 * tq * RP);
                if (2 * tq + 1 < np) half(a[4 * tq + 2], a[4 * tq + 3], e + (2 * tq + 1) * RP);
            }
        }
    } else if (t == 2) {
        char* e = at(4 * (w - 2) * RP + 4 * CP);
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) full(tq, e + tq * RP);
    } else if (w >= 2) {
        full(0, at((6 + w) * RP + 4 * CP));
    }
}

// lane & 15 -> output quad of a set (entry: bit 15 = no quad, bits 6.. = oy, bits 0-5 = x-quad)
template <int TOH, int TOW, int IWQ, int S = 1>
struct SetMap {
    static constexpr int OWQ = TOW / 4, NOQ = TOH * OWQ, NSET = (NOQ + 15) / 16, NSLOT = NSET * 16;
    static_assert(OWQ <= 64 && TOH <= 256, "entry packing");
    uint16_t v[NSLOT];
    constexpr SetMap() : v() {
        int bucket[16][NOQ] = {}; int cnt[16] = {}, used[16] = {};
        for (int r = 0; r < NOQ; ++r) { const int b = (S * (r / OWQ) * IWQ + (r % OWQ)) & 15; bucket[b][cnt[b]++] = r; }     // class of the quad's first INPUT cell (stride 2: rows keep even x-quads first, so cell = x-quad / 2)
        int slot[NSLOT] = {};
        for (int s = 0; s < NSET; ++s)
            for (int q = 0; q < 16; ++q) {
                const int b = ((q >> 2) + 4 * (q & 3)) & 15;                     // slot (pg, j) wants class pg + 4 j
                slot[s * 16 + q] = used[b] < cnt[b] ? bucket[b][used[b]++] : -1;
            }
        for (int b = 0; b < 16; ++b)                                            // uneven classes: leftovers fill the holes
            while (used[b] < cnt[b]) {
                int s = 0; while (slot[s] >= 0) ++s;
                slot[s] = bucket[b][used[b]++];
            }
        for (int s = 0; s < NSLOT; ++s) {
            const int r = slot[s] >= 0 ? slot[s] : 0;
            v[s] = (uint16_t)((slot[s] < 0 ? 0x8000 : 0) | ((r / OWQ) << 6) | (r % OWQ));
        }
    }
};

#define CF_MX_MFMA(ACC, AV, BV, ABID) ACC = __builtin_amdgcn_mfma_f32_4x4x4f16(AV, BV, ACC, 2, ABID, 0)

// one k-step of channel g of a lane's eight: bq = its 64 contiguous bytes of a cell row (channel g = dwords 2 g, 2 g + 1), a = the
// Toeplitz operands of channel quad g >> 2 (abid = g & 3 picks the channel inside the quad).  The callers keep the loop over g and
// pick the operand pair there: with the loop in here (both pairs as arguments) the LDS forms issue the table reads behind the cell
// reads and wait for all of them at once -- other assembly for all 29 instances that hold the table in LDS
__device__ __forceinline__ void mx_mfma8(f32x4* acc, int g, u32x2 a, const u32x4* bq) {
    const mfma_f16x4 av = __builtin_bit_cast(mfma_f16x4, a);
    u32x2 b2;
    b2.x = (g & 1) ? bq[g >> 1].z : bq[g >> 1].x;
    b2.y = (g & 1) ? bq[g >> 1].w : bq[g >> 1].y;
    const mfma_f16x4 bv = __builtin_bit_cast(mfma_f16x4, b2);
    switch (g & 3) {
        case 0: CF_MX_MFMA(acc[g], av, bv, 0); break;
        case 1: CF_MX_MFMA(acc[g], av, bv, 1); break;
        case 2: CF_MX_MFMA(acc[g], av, bv, 2); break;
        default: CF_MX_MFMA(acc[g], av, bv, 3); break;
    }
}
// the same for four channels: b0, b1 = the lane's 32 contiguous bytes
__device__ __forceinline__ void mx_mfma4(f32x4* acc, u32x2 a, u32x4 b0, u32x4 b1) {
    const mfma_f16x4 av = __builtin_bit_cast(mfma_f16x4, a);
    u32x2 t0, t1, t2, t3;
    t0.x = b0.x; t0.y = b0.y; t1.x = b0.z; t1.y = b0.w; t2.x = b1.x; t2.y = b1.y; t3.x = b1.z; t3.y = b1.w;
    CF_MX_MFMA(acc[0], av, __builtin_bit_cast(mfma_f16x4, t0), 0);
    CF_MX_MFMA(acc[1], av, __builtin_bit_cast(mfma_f16x4, t1), 1);
    CF_MX_MFMA(acc[2], av, __builtin_bit_cast(mfma_f16x4, t2), 2);
    CF_MX_MFMA(acc[3], av, __builtin_bit_cast(mfma_f16x4, t3), 3);
}

// depthwise of one set (16 output quads x 32 channels): acc[g][i] = output pixel i of this lane's quad, channel kg*8 + g
template <int KS, int IWQ, int CP>
__device__ __forceinline__ void mx_depthwise(const char* bb, const u32x2 (*A)[KS][2], f32x4* acc) {
    constexpr int NSTEP = KS * 2;
#pragma unroll
    for (int g = 0; g < 8; ++g) acc[g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    u32x4 bq[2][4];
#pragma unroll
    for (int g2 = 0; g2 < 4; ++g2) bq[0][g2] = ld16(bb + g2 * 16);
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {
        if (st + 1 < NSTEP) {
            const int ky = (st + 1) >> 1, ks = (st + 1) & 1;
#pragma unroll
            for (int g2 = 0; g2 < 4; ++g2) bq[(st + 1) & 1][g2] = ld16(bb + (ky * IWQ + ks) * CP + g2 * 16);
        }
        __builtin_amdgcn_sched_barrier(0);        // keep the next group's reads in flight under this group's MFMAs
#pragma unroll
        for (int g = 0; g < 8; ++g) mx_mfma8(acc, g, A[g >> 2][st >> 1][st & 1], bq[st & 1]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the same with the Toeplitz operands read from an LDS copy of the round's table ([2][KS][2][64 lanes] x 8 B) one step ahead
// instead of living in 24 / 40 VGPRs for the whole kernel
template <int KS, int IWQ, int CP>
__device__ __forceinline__ void mx_depthwise_lds(const char* bb, const char* at /* table + lane * 8 */, f32x4* acc) {
    constexpr int NSTEP = KS * 2;
#pragma unroll
    for (int g = 0; g < 8; ++g) acc[g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    u32x4 bq[2][4];
    u32x2 aq[2][2];
#pragma unroll
    for (int g2 = 0; g2 < 4; ++g2) bq[0][g2] = ld16(bb + g2 * 16);
    aq[0][0] = *reinterpret_cast<const u32x2*>(at);
    aq[0][1] = *reinterpret_cast<const u32x2*>(at + NSTEP * 512);
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {
        if (st + 1 < NSTEP) {
            const int ky = (st + 1) >> 1, ks = (st + 1) & 1;
#pragma unroll
            for (int g2 = 0; g2 < 4; ++g2) bq[(st + 1) & 1][g2] = ld16(bb + (ky * IWQ + ks) * CP + g2 * 16);
            aq[(st + 1) & 1][0] = *reinterpret_cast<const u32x2*>(at + (st + 1) * 512);
            aq[(st + 1) & 1][1] = *reinterpret_cast<const u32x2*>(at + (NSTEP + st + 1) * 512);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 8; ++g) mx_mfma8(acc, g, aq[st & 1][g >> 2], bq[st & 1]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// single-buffered form (16 VGPRs less): the reads of a step are issued and consumed in place; for kernels that run four waves per
// SIMD, where the other waves cover the LDS latency
template <int KS, int IWQ, int CP>
__device__ __forceinline__ void mx_depthwise_lds1(const char* bb, const char* at, f32x4* acc) {
    constexpr int NSTEP = KS * 2;
#pragma unroll
    for (int g = 0; g < 8; ++g) acc[g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {
        const int ky = st >> 1, ks = st & 1;
        u32x4 bq[4];
#pragma unroll
        for (int g2 = 0; g2 < 4; ++g2) bq[g2] = ld16(bb + (ky * IWQ + ks) * CP + g2 * 16);
        u32x2 aq[2];
        aq[0] = *reinterpret_cast<const u32x2*>(at + st * 512);
        aq[1] = *reinterpret_cast<const u32x2*>(at + (NSTEP + st) * 512);
#pragma unroll
        for (int g = 0; g < 8; ++g) mx_mfma8(acc, g, aq[g >> 2], bq);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Half a set's channels (g = 4 half .. 4 half + 3: 32 contiguous bytes of a cell row) for the stride-2 blocks, where a wave is
// (set, channel half); KSTEPS k-steps per kernel row (stride 2: inputs x .. x + 10 of an output quad = three quads); the Toeplitz
// operand table in LDS is [2 channel quads][KS][KSTEPS][64 lanes] x 8 B, `at` points at this half's quad + lane * 8
template <int KS, int KSTEPS, int IWQ, int CP>
__device__ __forceinline__ void mx_depthwise_half(const char* bb, const char* at, f32x4* acc) {
    constexpr int NSTEP = KS * KSTEPS;
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    u32x4 bq[2][2];
    u32x2 aq[2];
    bq[0][0] = ld16(bb); bq[0][1] = ld16(bb + 16);
    aq[0] = *reinterpret_cast<const u32x2*>(at);
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {
        if (st + 1 < NSTEP) {
            const int ky = (st + 1) / KSTEPS, ks = (st + 1) % KSTEPS;
            constexpr int HQ = (IWQ + 1) / 2;                      // cell rows: even x-quads, then odd ones
            bq[(st + 1) & 1][0] = ld16(bb + (ky * IWQ + (ks & 1) * HQ + (ks >> 1)) * CP);
            bq[(st + 1) & 1][1] = ld16(bb + (ky * IWQ + (ks & 1) * HQ + (ks >> 1)) * CP + 16);
            aq[(st + 1) & 1] = *reinterpret_cast<const u32x2*>(at + (st + 1) * 512);
        }
        __builtin_amdgcn_sched_barrier(0);
        mx_mfma4(acc, aq[st & 1], bq[st & 1][0], bq[st & 1][1]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the same with this half's Toeplitz operands resident in registers (KS x KSTEPS pairs)
template <int KS, int KSTEPS, int IWQ, int CP>
__device__ __forceinline__ void mx_depthwise_half_reg(const char* bb, const u32x2 (*A)[KSTEPS], f32x4* acc) {
    constexpr int NSTEP = KS * KSTEPS;
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    u32x4 bq[2][2];
    bq[0][0] = ld16(bb); bq[0][1] = ld16(bb + 16);
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {
        if (st + 1 < NSTEP) {
            const int ky = (st + 1) / KSTEPS, ks = (st + 1) % KSTEPS;
            constexpr int HQ = (IWQ + 1) / 2;
            bq[(st + 1) & 1][0] = ld16(bb + (ky * IWQ + (ks & 1) * HQ + (ks >> 1)) * CP);
            bq[(st + 1) & 1][1] = ld16(bb + (ky * IWQ + (ks & 1) * HQ + (ks >> 1)) * CP + 16);
        }
        __builtin_amdgcn_sched_barrier(0);
        mx_mfma4(acc, A[st / KSTEPS][st % KSTEPS], bq[st & 1][0], bq[st & 1][1]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Toeplitz A operands of nq rounds of 32 channels: [round][channel quad q][ky][k-step][lane (kg, pg, i)] = 4 fp16 (cf_mbconv3.hip)
// tap of output offset i against input k of k-step ks: w[ky][4 ks + k - stride * i]
void mx_pack_taps(int nq, int k, const float* wd /*[channels][k*k]*/, uint32_t* out, int stride = 1, int ksteps = 2);

}  // namespace cf
