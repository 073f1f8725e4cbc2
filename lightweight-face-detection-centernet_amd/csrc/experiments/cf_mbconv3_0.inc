// experiments build only (make EXP=1): cut out of cf_mbconv3.hip -- rounds-persistent variant: measured slower (profiles/r03_mfma_depthwise.md), experiments build only
// The same with the workgroup walking R rounds of its tile (grid.y = rounds / R): launch + first-DMA latency once per R rounds, the
// next round's weights and operand table streaming into a second LDS stage under the current round's depthwise
template <int KS, int JX, int TOH, int TOW, int NW, int R>
__global__ __launch_bounds__(NW * 64) void expdw_mxr_kernel(MbParams p) {
    constexpr bool ALDS = true;
    typedef Mx<KS, JX, TOH, TOW, NW, true> G;
    constexpr int IWQ = G::IWQ, IWP = G::IWP, IPX = G::IPX, NIB = G::NIB, CP = G::CP, NSET = G::NSET, WXB = G::WXB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* E = smem;
    char* Wst = smem + G::EBYTES;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pl = lane & 31, h = lane >> 5;
    const int tiles_x = (p.Wout + TOW - 1) / TOW;
    const int tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
    const int ox0 = txi * TOW, oy0 = tyi * TOH, b = blockIdx.z;
    const int grp = blockIdx.y;

    // round r of this workgroup = hidden-channel round grp * R + r; expand weights and the operand table of round r + 1 are DMA'd
    // into the other LDS stage while round r's depthwise runs
    constexpr int STG = WXB + G::ATB;
    auto stage = [&](int r) {
        char* dst = Wst + (r & 1) * STG;
        const char* srcx = (const char*)p.wexp + (size_t)(grp * R + r) * WXB;
        CF_MX_STAGE(srcx, dst, WXB);
        const char* srca = (const char*)p.wdw + (size_t)(grp * R + r) * G::ATB;
        CF_MX_STAGE(srca, dst + WXB, G::ATB);
        asm volatile("" ::: "memory");
    };
    stage(0);
    asm volatile("" ::: "memory");
    const char* xbase = (const char*)p.x + (size_t)b * p.Hin * p.Win * p.Cin * 2;
    const unsigned rowbytes = (unsigned)p.Cin * 2;
    auto load_x = [&](int ib, u32x4* xf) -> bool {
        const int ip = ib * 32 + pl;
        const int ipc = ip < IPX ? ip : IPX - 1;
        const int iy = ipc / IWP, ix = ipc - iy * IWP;
        const int gy = oy0 - p.pad_lo + iy, gx = ox0 - p.pad_lo + ix;
        const int cy = min(max(gy, 0), p.Hin - 1), cx = min(max(gx, 0), p.Win - 1);
        if (p.xblock) {
            const char* xb = (const char*)p.x + blk_off(((size_t)b * p.Hin + cy) * p.Win + cx, p.Cin / 8, h * JX);
#pragma unroll
            for (int j = 0; j < JX; ++j) xf[j] = ld16(xb + j * 512);
        } else {
            const unsigned off = ((unsigned)cy * (unsigned)p.Win + (unsigned)cx) * rowbytes + (unsigned)(h * JX * 16);
#pragma unroll
            for (int j = 0; j < JX; ++j) xf[j] = ld16(xbase + off + j * 16);
        }
        return ip < IPX && (unsigned)gy < (unsigned)p.Hin && (unsigned)gx < (unsigned)p.Win;
    };
    auto mask_x = [&](u32x4* xf, bool valid) {
#pragma unroll
        for (int j = 0; j < JX; ++j) {
            xf[j].x = valid ? xf[j].x : 0u; xf[j].y = valid ? xf[j].y : 0u; xf[j].z = valid ? xf[j].z : 0u; xf[j].w = valid ? xf[j].w : 0u;
        }
    };
    const int abl = 0;
    static constexpr SetMap<TOH, TOW, IWQ> kSets{};
    const int kg = lane >> 4;
#pragma unroll 1
    for (int r = 0; r < R; ++r) {
    const char* Wr = Wst + (r & 1) * STG;
    const char* Ats = Wr + WXB;
    u32x4 xa[JX];
    bool va = false;
    if (wave < NIB) va = load_x(wave, xa);
    static_assert(NIB >= NW, "every wave issues the X loads the wait below keeps in flight");
    cf_sync_lds_dma_keep<JX>();      // previous round's depthwise done with E; this round's weights / table (DMA, issued earlier) landed
    mask_x(xa, va);

    // ---- phase 1: expand + Swish -> quad cells.  D rows (r & 3) + 8 (r >> 2) + 4 h: register quad t = halo quad ib*8 + 2t + h
    for (int ib = wave; ib < NIB; ib += NW) {
        u32x4 xn[JX];
        const bool more = ib + NW < NIB;
        bool vn = false;
        if (more) { if (abl & 8) { for (int j = 0; j < JX; ++j) xn[j] = xa[j]; vn = va; } else vn = load_x(ib + NW, xn); }
        f32x16 a;
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = 0.0f;
        const char* wb = Wr + lane * 16;
#pragma unroll
        for (int j = 0; j < JX; ++j) {
            const u32x4 wv = ld16(wb + j * 1024);
            a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(mfma_bf16x8, xa[j]),
                                                        __builtin_bit_cast(mfma_bf16x8, wv), a, 0, 0, 0);
        }
        mx_block_store<CP>(E, ib, h, pl, a, !(abl & 4));
        if (more) {
#pragma unroll
            for (int j = 0; j < JX; ++j) xa[j] = xn[j];
            mask_x(xa, vn);
        }
    }
    __syncthreads();
    if (r + 1 < R) stage(r + 1);

    // ---- phase 2: depthwise on the matrix cores + Swish, 16 output quads x 32 channels per wave step
    for (int set = wave; set < NSET; set += NW) {
        const uint32_t e = kSets.v[set * 16 + (lane & 15)];
        const int oy = (e >> 6) & 0x1ff, oxq = e & 63;
        const bool live = (e & 0x8000u) == 0;
        f32x4 acc[8];
        const char* bb = E + (unsigned)(oy * IWQ + oxq) * (unsigned)CP + kg * 64;
        if (abl & 1) {
#pragma unroll
            for (int g = 0; g < 8; ++g) acc[g] = f32x4{(float)oy, (float)oxq, (float)g, 1.0f};
        } else {
        mx_depthwise_lds<KS, IWQ, CP>(bb, Ats + lane * 8, acc);
        }
        // a = -log2(e) * depthwise output -> Swish, leftover factor out again (the project GEMM has plain weights)
        if (!(abl & 2)) mx_swish_acc<8, true>(acc);
        const int gy = oy0 + oy, gx0 = ox0 + 4 * oxq;
        if (!live || gy >= p.Hout || ((abl & 16) && acc[0][0] != 123.0f)) continue;
        const size_t opix0 = ((size_t)b * p.Hout + gy) * p.Wout + gx0;
        const int chunk = (grp * R + r) * 4 + kg;                     // 8-channel chunk of the depthwise tensor
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (gx0 + i >= p.Wout) break;
            const u32x4 o = mx_pack8(acc, i);
            const size_t opix = opix0 + i;
            st16((char*)p.y + (p.yblock ? blk_off(opix, p.hid / 8, chunk) : (opix * p.hid + (size_t)chunk * 8) * 2), o);
        }
    }
    }
}

// Tile-persistent variant (VERDICT r04 next-4): a workgroup walks T consecutive tile units (tile x image) of ITS round of 32 hidden
// channels: expand weights and the Toeplitz table are DMA'd once, and the first X fragments of unit t + 1 are loaded into registers
// while the depthwise of unit t runs (the plain kernel starts every tile with a weight DMA + an exposed X load).
template <int KS, int JX, int TOH, int TOW, int NW, int T>
__global__ __launch_bounds__(NW * 64) void expdw_mxt_kernel(MbParams p) {
    typedef Mx<KS, JX, TOH, TOW, NW, true> G;
    constexpr int IWQ = G::IWQ, IWP = G::IWP, IPX = G::IPX, NIB = G::NIB, CP = G::CP, NSET = G::NSET, WXB = G::WXB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* E = smem;
    char* Wst = smem + G::EBYTES;
    char* Ats = Wst + WXB;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pl = lane & 31, h = lane >> 5;
    const int tiles_x = (p.Wout + TOW - 1) / TOW, tiles = tiles_x * ((p.Hout + TOH - 1) / TOH);
    const int units = tiles * p.B;
    const int grp = blockIdx.y;
    const int unit0 = blockIdx.x * T;
    {
        const char* srcx = (const char*)p.wexp + (size_t)grp * WXB;
        CF_MX_STAGE(srcx, Wst, WXB);
        const char* srca = (const char*)p.wdw + (size_t)grp * G::ATB;
        CF_MX_STAGE(srca, Ats, G::ATB);
    }
    asm volatile("" ::: "memory");
    auto load_x = [&](int b, int oy0, int ox0, int ib, u32x4* xf) -> bool {
        const int ip = ib * 32 + pl;
        const int ipc = ip < IPX ? ip : IPX - 1;
        const int iy = ipc / IWP, ix = ipc - iy * IWP;
        const int gy = oy0 - p.pad_lo + iy, gx = ox0 - p.pad_lo + ix;
        const int cy = min(max(gy, 0), p.Hin - 1), cx = min(max(gx, 0), p.Win - 1);
        if (p.xblock) {
            const char* xb = (const char*)p.x + blk_off(((size_t)b * p.Hin + cy) * p.Win + cx, p.Cin / 8, h * JX);
#pragma unroll
            for (int j = 0; j < JX; ++j) xf[j] = ld16(xb + j * 512);
        } else {
            const char* xbase = (const char*)p.x + (size_t)b * p.Hin * p.Win * p.Cin * 2;
            const unsigned off = ((unsigned)cy * (unsigned)p.Win + (unsigned)cx) * ((unsigned)p.Cin * 2) + (unsigned)(h * JX * 16);
#pragma unroll
            for (int j = 0; j < JX; ++j) xf[j] = ld16(xbase + off + j * 16);
        }
        return ip < IPX && (unsigned)gy < (unsigned)p.Hin && (unsigned)gx < (unsigned)p.Win;
    };
    auto mask_x = [&](u32x4* xf, bool valid) {
#pragma unroll
        for (int j = 0; j < JX; ++j) {
            xf[j].x = valid ? xf[j].x : 0u; xf[j].y = valid ? xf[j].y : 0u; xf[j].z = valid ? xf[j].z : 0u; xf[j].w = valid ? xf[j].w : 0u;
        }
    };
    auto unit_origin = [&](int unit, int& b, int& oy0, int& ox0) {
        b = unit / tiles;
        const int tile = unit - b * tiles;
        const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
        oy0 = tyi * TOH; ox0 = txi * TOW;
    };
    static_assert(NIB >= NW, "every wave issues the X loads the wait below keeps in flight");
    static constexpr SetMap<TOH, TOW, IWQ> kSets{};
    const int kg = lane >> 4;

    u32x4 xa[JX];
    bool va = false;
    int b, oy0, ox0;
    if (unit0 >= units) return;
    unit_origin(unit0, b, oy0, ox0);
    va = load_x(b, oy0, ox0, wave, xa);
    cf_sync_lds_dma_keep<JX>();              // weights / table landed for every wave
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        const int unit = unit0 + t;
        if (unit >= units) break;
        mask_x(xa, va);
        // ---- phase 1: expand + Swish -> quad cells
        for (int ib = wave; ib < NIB; ib += NW) {
            u32x4 xn[JX];
            const bool more = ib + NW < NIB;
            bool vn = false;
            if (more) vn = load_x(b, oy0, ox0, ib + NW, xn);
            f32x16 a;
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = 0.0f;
            const char* wb = Wst + lane * 16;
#pragma unroll
            for (int j = 0; j < JX; ++j) {
                const u32x4 wv = ld16(wb + j * 1024);
                a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(mfma_bf16x8, xa[j]),
                                                            __builtin_bit_cast(mfma_bf16x8, wv), a, 0, 0, 0);
            }
            mx_block_store<CP>(E, ib, h, pl, a);
            if (more) {
#pragma unroll
                for (int j = 0; j < JX; ++j) xa[j] = xn[j];
                mask_x(xa, vn);
            }
        }
        __syncthreads();
        // the next unit's first X fragments travel while this unit's depthwise runs
        const int bc = b, oyc = oy0, oxc = ox0;
        if (t + 1 < T && unit + 1 < units) {
            unit_origin(unit + 1, b, oy0, ox0);
            va = load_x(b, oy0, ox0, wave, xa);
        }
        // ---- phase 2: depthwise on the matrix cores + Swish
        for (int set = wave; set < NSET; set += NW) {
            const uint32_t e = kSets.v[set * 16 + (lane & 15)];
            const int oy = (e >> 6) & 0x1ff, oxq = e & 63;
            const bool live = (e & 0x8000u) == 0;
            f32x4 acc[8];
            const char* bb = E + (unsigned)(oy * IWQ + oxq) * (unsigned)CP + kg * 64;
            mx_depthwise_lds<KS, IWQ, CP>(bb, Ats + lane * 8, acc);
            mx_swish_acc<8, true>(acc);
            const int gy = oyc + oy, gx0 = oxc + 4 * oxq;
            if (!live || gy >= p.Hout) continue;
            const size_t opix0 = ((size_t)bc * p.Hout + gy) * p.Wout + gx0;
            const int chunk = grp * 4 + kg;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (gx0 + i >= p.Wout) break;
                const u32x4 o = mx_pack8(acc, i);
                const size_t opix = opix0 + i;
                st16((char*)p.y + (p.yblock ? blk_off(opix, p.hid / 8, chunk) : (opix * p.hid + (size_t)chunk * 8) * 2), o);
            }
        }
        __syncthreads();                      // every wave is done reading E before the next unit's expand overwrites it
    }
}
