// Tiled detection of large frames (sliced inference): the tile cutter and the merge of the per-tile detections.
//
// CUT.  One launch writes the network's uint8 input batch [Bf * T][H][W][3] BGR from Bf full-resolution frames (BGR rows or 4:2:0
// planes, pitched, read in place) and a table of T rectangles shared by the frames; image f * T + t is tile t of frame f:
//   tile(f, t) = resize(bgr(frame_f)[y0 : y0 + rh, x0 : x0 + rw], (H, W))
// with bgr() the fixed-point BT.601 conversion of cf_yuvmath.h (the identity for BGR frames) and resize the fixed-point INTER_LINEAR
// of cf_cvresize.h applied to the crop: the taps clamp at the rectangle's edges, not at the frame's.  x0, y0, rw, rh are even, so a
// 2 x 2 luma block and its chroma sample are never split and convert-then-crop equals crop-then-convert.  A rectangle of exactly
// (W, H) pixels gets the coefficients 2048 / 0 and reproduces the source bytes.
// A lane owns four adjacent output columns: their taps and coefficients are computed once and serve kCutRows output rows, each row
// going out as three dword stores (W % 4 == 0), lane-contiguous.  Source rows start at arbitrary even offsets: the taps are byte loads.
// Every tap lies inside the rectangle, hence inside the row extents of the planes; pitch padding is never read.
//
// MERGE (launch_merge: here for the tiles, the views and the placements alike; its kernel, collect_rows_kernel<Items, ROT>, is
// cf_collect.h's).  It fills the per-frame candidate table [Bf][cap = T * rows][16] (the record of ThreshParams::cand) from the per-tile
// results of a threshold decode, in order (tile ascending, keep position ascending), and the NMS stages of cf_decode.hip run on it.  Per row of tile (x0, y0, rw, rh), i < min(counts, rows):
//   * dropped when a corner is not finite, or when its network-coordinate box comes within `edge` pixels of an INTERIOR side of the
//     rectangle (one that is not on the frame border): x1 < edge, x2 > W - edge, y1 < edge, y2 > H - edge (float32 compares);
//   * else X = (float)((double)x * ((double)rw / (double)W) + (double)x0), Y likewise with rh / H and y0, for the four corners and the
//     ten landmark values (float64 in this order, no contraction: the file is built with -ffp-contract=off); the score is copied.
// The compaction is a prefix sum over the flattened (tile, row) items, never an atomic: the order is deterministic.
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_cutpx.h"
#include "cf_collect.h"
#include <string>

namespace cf {
namespace {

constexpr int kCutFrames = 64;                       // frames per launch: 3 x 64 pointers = 1.5 KB of kernel arguments
constexpr int kCutRows = 8;                          // output rows per lane (one set of column coefficients)
using CutPtrs = FramePtrs<kCutFrames>;

// (a loop of its own, not the padded lane of cf_cutpx.h: a tile has no padding, so no lane tests for it)
template <int SRC, bool VF>
__global__ void __launch_bounds__(256) cut_tiles_kernel(CutPtrs tab, const cf_tile_rect* __restrict__ rects, uint8_t* dst, int T, int pitch0,
                                                        int pitch1, int H, int W) {
    const int t = blockIdx.y, f = blockIdx.z;
    const int gw = W >> 2, ng = (H + kCutRows - 1) / kCutRows;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ng * gw) return;
    const int g = i / gw, X0 = (i - g * gw) << 2;
    const cf_tile_rect r = rects[t];
    const SrcPlanes src{tab.p0[f], tab.p1[f], tab.p2[f], pitch0, pitch1, 0, 0};
    int x0[4], x1[4], a0[4], a1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cv_linear_coeffs(X0 + k, r.w, W, true, x0[k], x1[k], a0[k], a1[k]);
        x0[k] += r.x0; x1[k] += r.x0;
    }
    uint8_t* out = dst + (((size_t)f * T + t) * H * W + X0) * 3;
    const int Yend = min(H, (g + 1) * kCutRows);
    for (int Y = g * kCutRows; Y < Yend; ++Y) {
        int y0, y1, b0, b1;
        cv_linear_coeffs(Y, r.h, H, false, y0, y1, b0, b1);
        y0 += r.y0; y1 += r.y0;
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = bilinear_px<SRC, VF>(src, y0, y1, b0, b1, x0[k], x1[k], a0[k], a1[k]);
        quad_store(out + (size_t)Y * W * 3, p);
    }
}

}  // namespace

int tile_grid(int h, int w, int tile_h, int tile_w, int overlap, int with_full, cf_tile_rect* rects, int cap, int* n) {
    if (!n || cap < 0 || (cap > 0 && !rects)) return CF_EINVAL;
    if (h < 2 || w < 2 || tile_h < 2 || tile_w < 2 || overlap < 0 || ((h | w | tile_h | tile_w | overlap) & 1)) return CF_EINVAL;
    if (overlap >= std::min(tile_h, tile_w)) return CF_EINVAL;
    const int rw = std::min(tile_w, w), rh = std::min(tile_h, h);
    const int nx = rw == w ? 1 : (w - overlap + (rw - overlap) - 1) / (rw - overlap);
    const int ny = rh == h ? 1 : (h - overlap + (rh - overlap) - 1) / (rh - overlap);
    int k = 0;
    auto put = [&](int x0, int y0, int ww, int hh) { if (k < cap) rects[k] = {x0, y0, ww, hh}; ++k; };
    for (int iy = 0; iy < ny; ++iy)
        for (int ix = 0; ix < nx; ++ix) {
            const int x0 = nx == 1 ? 0 : (int)(((long long)ix * (w - rw)) / (nx - 1)) & ~1;
            const int y0 = ny == 1 ? 0 : (int)(((long long)iy * (h - rh)) / (ny - 1)) & ~1;
            put(x0, y0, rw, rh);
        }
    if (with_full && nx * ny > 1) put(0, 0, w, h);
    *n = k;
    return CF_OK;
}

const char* tiles_check(std::string& why, int format, int Bf, int h, int w, int pitch0, int pitch1, const cf_tile_rect* rects, int T, int H, int W) {
    auto say = [&](const std::string& s) { why = s; return why.c_str(); };
    if (Bf < 1 || T < 1) return say("Bf and T must be at least 1");
    if (H < 1 || W < 4 || (W & 3)) return say("W must be a multiple of 4 and H at least 1");
    if (const char* geo = frame_geometry_check(FrameGeo{format, Bf, h, w, pitch0, pitch1}, 2, true)) return say(geo);
    if (!rects) return say("null rectangle table");
    for (int t = 0; t < T; ++t) {
        const cf_tile_rect& r = rects[t];
        const char* bad = nullptr;
        if ((r.x0 | r.y0 | r.w | r.h) & 1) bad = "has an odd value";
        else if (r.w < 2 || r.h < 2) bad = "is smaller than 2 x 2";
        else if (r.x0 < 0 || r.y0 < 0 || r.x0 > w - r.w || r.y0 > h - r.h) bad = "does not lie inside the frame";
        if (bad) {
            char b[192];
            snprintf(b, sizeof b, "rectangle %d (x0=%d, y0=%d, w=%d, h=%d) %s (%d x %d)", t, r.x0, r.y0, r.w, r.h, bad, w, h);
            return say(b);
        }
    }
    return nullptr;
}

// planes: Bf x {p0, p1, p2} device addresses (HOST table); rects: T rectangles on the DEVICE; the caller has run tiles_check
hipError_t launch_cut_tiles(hipStream_t s, int format, const void* const* planes, int Bf, int pitch0, int pitch1, const cf_tile_rect* rects,
                            int T, uint8_t* dst, int H, int W) {
    if (format < CF_YUV_NV12 || format > CF_FRAME_BGR || !planes || !rects || !dst || Bf < 1 || T < 1 || T > 65535 || H < 1 || W < 4 || (W & 3))
        return hipErrorInvalidValue;
    const long long n = (long long)((H + kCutRows - 1) / kCutRows) * (W >> 2);
    for (int f0 = 0; f0 < Bf; f0 += kCutFrames) {
        const int nb = Bf - f0 < kCutFrames ? Bf - f0 : kCutFrames;
        const CutPtrs tab = frame_ptrs<kCutFrames>(planes, format, f0, nb, true);      // YV12: the I420 kernel on swapped planes (as launch_yuv_to_bgr)
        const dim3 grid((unsigned)((n + 255) / 256), (unsigned)T, (unsigned)nb);
        uint8_t* out = dst + (size_t)f0 * T * H * W * 3;
        with_format(format, [&](auto SRC, auto VF) {
            hipLaunchKernelGGL((cut_tiles_kernel<SRC, VF>), grid, dim3(256), 0, s, tab, rects, out, T, pitch0, pitch1, H, W);
        });
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

size_t merge_mask_bytes(int Bf, int V, int rows) {
    const size_t cap = (size_t)V * rows;
    return (size_t)Bf * cap * ((cap + 63) / 64) * sizeof(unsigned long long);
}

hipError_t launch_merge(hipStream_t s, const MergeParams& p) {
    const bool sources = p.kind == MERGE_TILES ? p.rects && p.H >= 1 && p.W >= 1 && p.rot == 0
                       : p.kind == MERGE_VIEWS ? p.views && p.rot == 0
                       : p.kind == MERGE_PLACED && p.pack.places && p.pack.fr_off && p.pack.fr_idx && (p.rot == 0 || p.rot == 90 || p.rot == 180 || p.rot == 270);
    if (!sources || p.Bf < 1 || p.V < 1 || p.rows < 1 || p.max_out < 1 || (long long)p.V * p.rows > INT_MAX / 16 || p.h < 1 || p.w < 1 || p.score_stride < 1 ||
        (p.metric != CF_MERGE_IOU && p.metric != CF_MERGE_IOS) || !p.dets_net || !p.scores || !p.lms_net || !p.counts || !p.cand || !p.cand_count ||
        !p.order || !p.mask || !p.dets || !p.lms || !p.corners || !p.out_counts || !p.flags)
        return hipErrorInvalidValue;
    const dim3 grid(p.Bf), block(1024);
    if (p.kind == MERGE_TILES) hipLaunchKernelGGL((collect_rows_kernel<TileItems, 0>), grid, block, 0, s, p);
    else if (p.kind == MERGE_VIEWS) hipLaunchKernelGGL((collect_rows_kernel<ViewItems, 0>), grid, block, 0, s, p);
    else if (p.rot == 0) hipLaunchKernelGGL((collect_rows_kernel<PlacedItems, 0>), grid, block, 0, s, p);
    else if (p.rot == 90) hipLaunchKernelGGL((collect_rows_kernel<PlacedItems, 1>), grid, block, 0, s, p);
    else if (p.rot == 180) hipLaunchKernelGGL((collect_rows_kernel<PlacedItems, 2>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((collect_rows_kernel<PlacedItems, 3>), grid, block, 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ThreshParams q{};
    q.B = p.Bf; q.cap = p.V * p.rows; q.nms_thresh = p.thresh; q.metric = p.metric;
    q.cand = p.cand; q.cand_count = p.cand_count; q.order = p.order; q.mask = p.mask;
    q.max_out = p.max_out; q.dets = p.dets; q.lms = p.lms; q.dets_net = p.corners; q.counts = p.out_counts;
    return launch_nms_stages(s, q);
}

}  // namespace cf
