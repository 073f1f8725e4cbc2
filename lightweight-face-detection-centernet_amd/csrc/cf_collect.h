// The row collection behind the merges (cf_tiles.hip) and the unfit (cf_fit.hip): the order-keeping compaction of a 1024-thread
// workgroup, the index map of a rotated source, and the one collect kernel of launch_merge with the three ways an item finds its image
// and its view.  The files that include it are built with -ffp-contract=off: the mappings are float64 in a fixed order.
#pragma once
#include "cf_kernels.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cf {

// One compaction round of a 1024-thread workgroup: keep flag, ballot, the 16 wave counts through LDS, a prefix sum, so the order
// is the items' and deterministic.  Returns the position of this thread's item (meaningful when keep) and moves base past the round's items.
__device__ __forceinline__ uint32_t compact_pos(bool keep, uint32_t& base) {
    __shared__ uint32_t wave_cnt[16];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const unsigned long long bal = __ballot(keep);
    __syncthreads();                                                      // the counts of the round before have been read
    if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t off = 0, total = 0;
    for (int w2 = 0; w2 < 16; ++w2) { if (w2 == wave) off = total; total += wave_cnt[w2]; }      // off: the counts of the waves before this one
    const uint32_t pos = base + off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    base += total;
    return pos;
}

// A point (ux, uy) of the upright view -> the stored h x w frame by the index map of the turn (ROT: 0 = as stored, 1 = 90, 2 = 180,
// 3 = 270 clockwise); the difference is taken in float64 and rounded once.
template <int ROT>
__device__ __forceinline__ void turn_point(double ux, double uy, int h, int w, float& X, float& Y) {
    if constexpr (ROT == 0) { X = (float)ux; Y = (float)uy; }
    else if constexpr (ROT == 1) { X = (float)uy; Y = (float)((double)(h - 1) - ux); }
    else if constexpr (ROT == 2) { X = (float)((double)(w - 1) - ux); Y = (float)((double)(h - 1) - uy); }
    else { X = (float)((double)(w - 1) - uy); Y = (float)ux; }
}

// A row through the turn: the box is an ASSIGNMENT of mapped corners, never a min / max; the landmarks go point by point, order kept.
// map(x, y, X, Y) takes a point of the canvas to the stored frame.
template <int ROT, class Map>
__device__ __forceinline__ void turn_box(const float (&c)[4], Map&& map, float* o) {
    if constexpr (ROT == 0) { map(c[0], c[1], o[0], o[1]); map(c[2], c[3], o[2], o[3]); }
    else if constexpr (ROT == 2) { map(c[2], c[3], o[0], o[1]); map(c[0], c[1], o[2], o[3]); }
    else if constexpr (ROT == 1) { map(c[2], c[1], o[0], o[1]); map(c[0], c[3], o[2], o[3]); }
    else { map(c[0], c[3], o[0], o[1]); map(c[2], c[1], o[2], o[3]); }
}
template <class Map>
__device__ __forceinline__ void turn_landmarks(const float* l, Map&& map, float* o) {
#pragma unroll
    for (int k = 0; k < 5; ++k) map(l[2 * k], l[2 * k + 1], o[2 * k], o[2 * k + 1]);
}

// Items: how source q of frame f finds its image and its view, how many sources a frame has, and whether a row whose centre lies
// outside the content is dropped.
struct TileItems {                                   // image f * V + q, the whole canvas the content of rectangle q
    static constexpr bool kCentre = false;           // (a tile has no padding: the edge rule alone decides)
    const MergeParams& p;
    __device__ int sources(int) const { return p.V; }
    __device__ int img(int f, int q) const { return f * p.V + q; }
    __device__ cf_view view(int, int q) const { const cf_tile_rect r = p.rects[q]; return cf_view{r.x0, r.y0, r.w, r.h, 0, 0, p.W, p.H}; }
};
struct ViewItems {                                   // image f * V + q, view q
    static constexpr bool kCentre = true;
    const MergeParams& p;
    __device__ int sources(int) const { return p.V; }
    __device__ int img(int f, int q) const { return f * p.V + q; }
    __device__ cf_view view(int, int q) const { return p.views[q]; }
};
struct PlacedItems {                                 // the placements of frame f in placement-index order (the CSR by frame); image = canvas
    static constexpr bool kCentre = true;
    const MergeParams& p;
    __device__ const cf_place& at(int f, int q) const { return p.pack.places[p.pack.fr_idx[p.pack.fr_off[f] + q]]; }
    __device__ int sources(int f) const { return p.pack.fr_off[f + 1] - p.pack.fr_off[f]; }
    __device__ int img(int f, int q) const { return at(f, q).canvas; }
    __device__ cf_view view(int f, int q) const { return at(f, q).view; }
};

// One workgroup per frame walks its (source, row) items in order, 1024 at a time, and fills the frame's candidate table
// [p.V * p.rows][16].  Per row i < min(counts[img], rows) of a view with source (sx0, sy0, sw, sh) and content (dx, dy, dw, dh), dropped
// when a corner is not finite; when (Items::kCentre) its centre cx = (x1 + x2) * 0.5f, cy likewise, lies outside the content; or when
// its box comes within `edge` of a content side whose SOURCE side is interior to the upright view (hu x wu): x1 < (float)dx + edge when
// sx0 > 0, x2 > (float)(dx + dw) - edge when sx0 + sw < wu, the same two in y (float32).  A kept point goes to the upright view,
//   ux(x) = ((double)x - dx) * ((double)sw / dw) + sx0,   uy(y) = ((double)y - dy) * ((double)sh / dh) + sy0
// then to the stored p.h x p.w frame by turn_point<ROT>; the score is copied.
template <class Items, int ROT>
__global__ void __launch_bounds__(1024) collect_rows_kernel(MergeParams p) {
    __shared__ int truncated;
    const Items it{p};
    const int f = blockIdx.x, tid = threadIdx.x;
    const int items = it.sources(f) * p.rows;
    const int hu = (ROT & 1) ? p.w : p.h, wu = (ROT & 1) ? p.h : p.w;
    float* cand = p.cand + (size_t)f * p.V * p.rows * 16;
    if (tid == 0) truncated = 0;
    __syncthreads();
    uint32_t base = 0;
    for (int j0 = 0; j0 < items; j0 += 1024) {           // (items is uniform over the workgroup: so is the trip count)
        const int j = j0 + tid;
        bool keep = false;
        int img = 0, row = 0;
        float c[4] = {0.f, 0.f, 0.f, 0.f};
        cf_view r = {0, 0, 2, 2, 0, 0, 1, 1};
        if (j < items) {
            const int q = j / p.rows;
            row = j - q * p.rows;
            img = it.img(f, q);
            const int n = p.counts[img];
            if (row == 0 && n > p.rows) truncated = 1;                    // (every writer stores the same value)
            if (row < min(n, p.rows)) {
                r = it.view(f, q);
                const float4 b4 = *reinterpret_cast<const float4*>(p.dets_net + ((size_t)img * p.rows + row) * 4);
                c[0] = b4.x; c[1] = b4.y; c[2] = b4.z; c[3] = b4.w;
                keep = isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(c[3]);
                const float xlo = (float)r.dx, xhi = (float)(r.dx + r.dw), ylo = (float)r.dy, yhi = (float)(r.dy + r.dh);
                if constexpr (Items::kCentre) {
                    const float cx = (c[0] + c[2]) * 0.5f, cy = (c[1] + c[3]) * 0.5f;
                    if (!(cx >= xlo && cx < xhi && cy >= ylo && cy < yhi)) keep = false;
                }
                if (r.sx0 > 0 && c[0] < xlo + p.edge) keep = false;
                if (r.sx0 + r.sw < wu && c[2] > xhi - p.edge) keep = false;
                if (r.sy0 > 0 && c[1] < ylo + p.edge) keep = false;
                if (r.sy0 + r.sh < hu && c[3] > yhi - p.edge) keep = false;
            }
        }
        const uint32_t pos = compact_pos(keep, base);
        if (keep) {
            const size_t src = (size_t)img * p.rows + row;
            const double sx = (double)r.sw / (double)r.dw, sy = (double)r.sh / (double)r.dh;
            const double dx = (double)r.dx, dy = (double)r.dy, ox = (double)r.sx0, oy = (double)r.sy0;
            auto map = [&](float x, float y, float& X, float& Y) {
                turn_point<ROT>(((double)x - dx) * sx + ox, ((double)y - dy) * sy + oy, p.h, p.w, X, Y);
            };
            float o[16];
            turn_box<ROT>(c, map, o);
            o[4] = p.scores[src * p.score_stride];
            turn_landmarks(p.lms_net + src * 10, map, o + 5);
            o[15] = 0.0f;
            float4* d = reinterpret_cast<float4*>(cand + (size_t)pos * 16);
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        }
    }
    __syncthreads();
    if (tid == 0) { p.cand_count[f] = (int)base; p.flags[f] = truncated; }
}

}  // namespace cf
