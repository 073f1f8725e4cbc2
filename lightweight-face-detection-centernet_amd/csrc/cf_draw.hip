// Annotation of the source frame: box outlines, landmark dots and a numeric label (score or track id) of every kept face row are
// painted into a BGR or 4:2:0 frame that stays on the device (cf_draw_faces, cf_op_draw).  The arithmetic is the statement in
// include/centerface_hip.h, written once in cf_drawmath.h for the host and the kernels and restated in numpy in tests/draw_cases.py;
// kernel and restatement are equal byte for byte.  Integers throughout, except the point mapping, which is float64 in the order written
// with no FMA contraction (this file is compiled with -ffp-contract=off).
//
// Why a gather.  A frame pixel takes the colour of the HIGHEST layer that any row of its image puts on it (1 held outline / plate, 2 live
// outline / plate, 3 ink, 4 dot), so the result depends neither on the order of the rows nor on their overlap.  A scatter per face, as
// redact_write_kernel's, would have two workgroups store different colours to one byte where a dot of one face lies on the outline of
// another, and the winner would be a matter of timing.  Here every byte has exactly one writer, which looks at all rows:
//   draw_prep_kernel   one thread per (image, row) below min(counts[b], rows_cap) -- the counts are read on the device, the grid is sized
//                      from capacities -- writes the row's DrawFace record and the bounding rectangle of its primitives to a scratch.
//   draw_paint_kernel  one 256-thread workgroup per 64 x 16 tile of the luma / BGR plane and frame.  Its lanes test the image's records
//                      against the tile, 256 rows per step; the hits are compacted into an LDS list (ballot + prefix inside a wave, one
//                      LDS add per wave); a thread owns 4 pixels of a tile row and keeps the highest layer over the listed records.  A
//                      tile that no record touches leaves after the scan: the common case, and the whole cost of a frame without faces.
//                      Otherwise the thread stores its pixels' bytes as aligned dwords (store_masked_dword: whole when all four bytes
//                      are drawn, single bytes otherwise), leaves the layers in LDS, and the first 128 threads paint the tile's 32 x 8
//                      chroma samples from the 2 x 2 rule.  No atomics on the frame, no scratch image, and the frame is never read.
// Undrawn bytes -- pitch padding included -- are not written at all.
#include <limits.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <string>

#include "centerface_hip.h"
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_drawmath.h"
#include "cf_redactmath.h"

namespace cf {
namespace {

constexpr int kDrawTileW = 64, kDrawTileH = 16;       // luma / BGR pixels; even, so the chroma tile is its half

struct DrawArgs {
    FrameGeo g;           // g.B: the frames of this launch
    DrawGeoOpts o;
    uint32_t color[5];    // [layer]: the three bytes in PLANE order (BGR; Y, first chroma channel in memory order, second)
    const DrawRec* recs;  // [g.B][rows_cap]
    const int* counts;
    int rows_cap, tiles_x;
};

__global__ void __launch_bounds__(256) draw_prep_kernel(DrawRows r, DrawGeoOpts o, int B, int h, int w, DrawRec* recs) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = (int)(gid / r.rows_cap), i = (int)(gid - (long long)b * r.rows_cap);
    if (b >= B || i >= min(r.counts[b], r.rows_cap)) return;
    const size_t row = (size_t)b * r.stride + i;
    DrawRec out;
    out.f = draw_face(o, r.boxes + row * 4, r.scores[row * r.score_step], r.lms ? r.lms + row * 10 : nullptr, r.info ? r.info + row * 3 : nullptr,
                      h, w, r.H, r.W);
    out.b = draw_bounds(out.f, o, h, w);
    recs[(size_t)b * r.rows_cap + i] = out;
}

__global__ void __launch_bounds__(256) draw_paint_kernel(DrawArgs a, RedactPtrs t) {
    __shared__ int s_list[256];
    __shared__ int s_n;
    __shared__ __align__(4) uint8_t s_layer[kDrawTileH][kDrawTileW];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const int x0 = tx * kDrawTileW, y0 = ty * kDrawTileH, w = a.g.w, h = a.g.h;
    const int n = min(a.counts[b], a.rows_cap);
    const DrawRec* recs = a.recs + (size_t)b * a.rows_cap;
    const int px = x0 + 4 * (tid & 15), py = y0 + (tid >> 4);      // this thread's pixels: (px .. px + 3, py)
    int layer[4] = {0, 0, 0, 0};
    bool any = false;
    for (int base = 0; base < n; base += 256) {                    // uniform trip count
        if (tid == 0) s_n = 0;
        __syncthreads();
        const int row = base + tid;
        bool hit = false;
        if (row < n) {
            const DrawRect r = recs[row].b;
            hit = r.x0 < r.x1 && r.y0 < r.y1 && r.x0 < x0 + kDrawTileW && r.x1 > x0 && r.y0 < y0 + kDrawTileH && r.y1 > y0;
        }
        const unsigned long long m = __ballot(hit);
        if (m) {
            const int lane = tid & 63;
            int at = 0;
            if (lane == 0) at = atomicAdd(&s_n, __popcll(m));
            at = __shfl(at, 0);
            if (hit) s_list[at + __popcll(m & ((1ull << lane) - 1ull))] = row;
        }
        __syncthreads();
        const int cnt = s_n;
        any = any || cnt > 0;
        if (py < h)
            for (int k = 0; k < cnt; ++k) {
                const DrawRec& rec = recs[__builtin_amdgcn_readfirstlane(s_list[k])];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (px + j < w && layer[j] < 4) layer[j] = max(layer[j], draw_layer(rec.f, a.o, px + j, py));
            }
        __syncthreads();                                           // s_list is rewritten by the next step
    }
    if (!any) return;                                              // uniform: s_n was the same for every thread in every step
    const bool bgr = a.g.format == CF_FRAME_BGR;
    if (py < h && (layer[0] | layer[1] | layer[2] | layer[3])) {
        if (bgr) {
            uint8_t* q = t.p0[b] + (size_t)py * a.g.pitch0 + (size_t)px * 3;       // 12 bytes: three aligned dwords
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                uint32_t val = 0;
                int mask = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int byte = 4 * d + k, j = byte / 3, ch = byte - 3 * j;
                    if (!layer[j]) continue;
                    val |= ((a.color[layer[j]] >> (8 * ch)) & 255u) << (8 * k);
                    mask |= 1 << k;
                }
                if (mask) store_masked_dword(q + 4 * d, val, mask);
            }
        } else {
            uint32_t val = 0;
            int mask = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (layer[j]) { val |= (a.color[layer[j]] & 255u) << (8 * j); mask |= 1 << j; }
            store_masked_dword(t.p0[b] + (size_t)py * a.g.pitch0 + px, val, mask);
        }
    }
    if (bgr) return;
    // 4:2:0: chroma sample (i, j) takes bytes 1 and 2 of the colour of the highest layer over its luma pixels (2i..2i+1, 2j..2j+1)
    *reinterpret_cast<uint32_t*>(&s_layer[tid >> 4][4 * (tid & 15)]) =
        (uint32_t)layer[0] | (uint32_t)layer[1] << 8 | (uint32_t)layer[2] << 16 | (uint32_t)layer[3] << 24;
    __syncthreads();
    if (tid >= 128) return;
    const bool il = frame_is_il(a.g.format);
    const int cw = w >> 1, chh = h >> 1, cx0 = x0 >> 1, cy0 = y0 >> 1;
    auto top = [&](int i, int j) {       // tile-local chroma sample -> layer
        return max(max((int)s_layer[2 * j][2 * i], (int)s_layer[2 * j][2 * i + 1]), max((int)s_layer[2 * j + 1][2 * i], (int)s_layer[2 * j + 1][2 * i + 1]));
    };
    uint32_t val = 0;
    int mask = 0;
    if (il) {                            // 64 bytes per tile row = 16 dwords of two (c0, c1) samples, 8 rows
        const int j = tid >> 4, d = tid & 15;
        if (cy0 + j >= chh) return;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = 2 * d + s;
            const int l = cx0 + i < cw ? top(i, j) : 0;
            if (l) { val |= ((a.color[l] >> 8) & 0xFFFFu) << (16 * s); mask |= 3 << (2 * s); }
        }
        if (mask) store_masked_dword(t.p1[b] + (size_t)(cy0 + j) * a.g.pitch1 + (size_t)(cx0 + 2 * d) * 2, val, mask);
    } else {                             // per plane 32 bytes per tile row = 8 dwords of four samples, 8 rows; threads 0..63 plane 1, 64..127 plane 2
        const int pl = tid >> 6, j = (tid & 63) >> 3, d = tid & 7;
        if (cy0 + j >= chh) return;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int i = 4 * d + s;
            const int l = cx0 + i < cw ? top(i, j) : 0;
            if (l) { val |= ((a.color[l] >> (8 * (1 + pl))) & 255u) << (8 * s); mask |= 1 << s; }
        }
        if (mask) store_masked_dword((pl ? t.p2[b] : t.p1[b]) + (size_t)(cy0 + j) * a.g.pitch1 + (cx0 + 4 * d), val, mask);
    }
}

}  // namespace

const char* draw_check(const cf_draw_opts* o, int format, int B, int h, int w, int pitch0, int pitch1) {
    const char* geo = frame_geometry_check(FrameGeo{format, B, h, w, pitch0, pitch1}, 1, false);
    if (format < CF_YUV_NV12 || format > CF_FRAME_BGR) return geo;             // the format is refused first, then the options
    if (o->what < 0 || o->what > (CF_DRAW_BOX | CF_DRAW_LANDMARKS)) return "unknown `what` bits (1 = CF_DRAW_BOX, 2 = CF_DRAW_LANDMARKS)";
    if (o->label < CF_DRAW_LABEL_NONE || o->label > CF_DRAW_LABEL_ID) return "unknown label (0 = CF_DRAW_LABEL_NONE, 1 = _SCORE, 2 = _ID)";
    if (o->what == 0 && o->label == CF_DRAW_LABEL_NONE) return "nothing to draw (what == 0 and no label)";
    if (o->thickness < 1 || o->thickness > 16) return "thickness must be in [1, 16]";
    if (o->radius < 0 || o->radius > 16) return "radius must be in [0, 16]";
    if (o->label_scale < 1 || o->label_scale > 8) return "label_scale must be in [1, 8]";
    if (o->dash_held != 0 && o->dash_held != 1) return "dash_held must be 0 or 1";
    if (!(o->scale >= 0.25f && o->scale <= 4.0f)) return "scale must be in [0.25, 4]";
    return geo;
}

DrawGeoOpts draw_geo_opts(const cf_draw_opts* o) {
    return DrawGeoOpts{o->what, o->thickness, o->radius, o->label, o->label_scale, o->dash_held, o->scale};
}

size_t draw_scratch_bytes(int B, int rows_cap) { return (size_t)B * rows_cap * sizeof(DrawRec); }

hipError_t launch_draw_faces(hipStream_t s, const DrawParams& p) {
    const FrameGeo& g = p.g;
    if (draw_check(&p.o, g.format, g.B, g.h, g.w, g.pitch0, g.pitch1) || redact_check_planes(g.format, p.planes, g.B, 1, g.pitch0, g.pitch1) ||
        p.r.H < 1 || p.r.W < 1 || !p.r.boxes || !p.r.scores || !p.r.counts || p.r.stride < 1 || p.r.rows_cap < 1 || p.r.rows_cap > p.r.stride ||
        p.r.score_step < 1 || !p.recs || ((p.o.what & CF_DRAW_LANDMARKS) && !p.r.lms) || (p.o.label == CF_DRAW_LABEL_ID && !p.r.info))
        return hipErrorInvalidValue;
    const long long rows = (long long)g.B * p.r.rows_cap;
    if (rows > (1ll << 30)) return hipErrorInvalidValue;
    const DrawGeoOpts o = draw_geo_opts(&p.o);
    hipLaunchKernelGGL(draw_prep_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, p.r, o, g.B, g.h, g.w, p.recs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const bool swap = frame_swaps_chroma(g.format);
    DrawArgs a{};
    a.g = g; a.o = o; a.rows_cap = p.r.rows_cap;
    const uint8_t* col[5] = {nullptr, p.o.held_color, p.o.box_color, p.o.text_color, p.o.lm_color};
    for (int l = 1; l < 5; ++l) a.color[l] = (uint32_t)col[l][0] | ((uint32_t)col[l][swap ? 2 : 1] << 8) | ((uint32_t)col[l][swap ? 1 : 2] << 16);
    a.tiles_x = (g.w + kDrawTileW - 1) / kDrawTileW;
    const int tiles = a.tiles_x * ((g.h + kDrawTileH - 1) / kDrawTileH);
    for (int f0 = 0; f0 < g.B; f0 += kRedactFrames) {
        const int nb = std::min(g.B - f0, kRedactFrames);
        const RedactPtrs tab = frame_ptrs<kRedactFrames>(p.planes, g.format, f0, nb, false);
        a.g.B = nb;
        a.recs = p.recs + (size_t)f0 * p.r.rows_cap;
        a.counts = p.r.counts + f0;
        hipLaunchKernelGGL(draw_paint_kernel, dim3((unsigned)tiles, (unsigned)nb), dim3(256), 0, s, a, tab);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace cf

// One row's DrawFace record, by the code draw_prep_kernel runs (host only; here, because this file is compiled without FMA contraction).
int cf_draw_layout(const cf_draw_opts* o, const float* box, float score, const float* lms, const int32_t* info, int h, int w, int H, int W,
                   int32_t* out) {
    const char* why = !o || !box || !out ? "null options, box or out" : cf::draw_check(o, CF_FRAME_BGR, 1, h, w, 3 * w, 0);
    if (!why && (H < 1 || W < 1)) why = "H / W below 1";
    if (why) { cf::op_error_set((std::string("cf_draw_layout: ") + why).c_str()); return CF_EINVAL; }
    const cf::DrawFace f = cf::draw_face(cf::draw_geo_opts(o), box, score, lms, info, h, w, H, W);
    memcpy(out, &f, sizeof f);
    return CF_OK;
}
