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
// MERGE.  A collect kernel fills the per-frame candidate table [Bf][cap = T * rows][16] (the record of ThreshParams::cand) from the
// per-tile results of a threshold decode, in order (tile ascending, keep position ascending), and the NMS stages of cf_decode.hip run
// on it.  Per row of tile (x0, y0, rw, rh), i < min(counts, rows):
//   * dropped when a corner is not finite, or when its network-coordinate box comes within `edge` pixels of an INTERIOR side of the
//     rectangle (one that is not on the frame border): x1 < edge, x2 > W - edge, y1 < edge, y2 > H - edge (float32 compares);
//   * else X = (float)((double)x * ((double)rw / (double)W) + (double)x0), Y likewise with rh / H and y0, for the four corners and the
//     ten landmark values (float64 in this order, no contraction: the file is built with -ffp-contract=off); the score is copied.
// The compaction is a prefix sum over the flattened (tile, row) items, never an atomic: the order is deterministic.
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_cvresize.h"
#include "cf_yuvmath.h"
#include <string>

namespace cf {
namespace {

constexpr int kCutFrames = 64;                       // frames per launch: 3 x 64 pointers = 1.5 KB of kernel arguments
constexpr int kCutRows = 8;                          // output rows per lane (one set of column coefficients)
using CutPtrs = FramePtrs<kCutFrames>;

// SRC: 0 = BGR rows, 1 = one interleaved chroma plane (NV12 / NV21), 2 = two chroma planes (I420; YV12 on a swapped table);
// VF: V first in the interleaved pairs (NV21).  One source pixel -> B | G << 8 | R << 16
template <int SRC, bool VF>
__device__ __forceinline__ uint32_t cut_tap(const uint8_t* p0, const uint8_t* p1, const uint8_t* p2, int pitch0, int pitch1, int y, int x) {
    if constexpr (SRC == 0) {
        const uint8_t* q = p0 + (size_t)y * pitch0 + 3 * x;
        return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    } else {
        return yuv_px(p0[(size_t)y * pitch0 + x], chroma_at<SRC == 1, VF>(p1, p2, pitch1, y >> 1, x >> 1));
    }
}

template <int SRC, bool VF>
__global__ void __launch_bounds__(256) cut_tiles_kernel(CutPtrs tab, const cf_tile_rect* __restrict__ rects, uint8_t* dst, int T, int pitch0,
                                                        int pitch1, int H, int W) {
    const int t = blockIdx.y, f = blockIdx.z;
    const int gw = W >> 2, ng = (H + kCutRows - 1) / kCutRows;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ng * gw) return;
    const int g = i / gw, X0 = (i - g * gw) << 2;
    const cf_tile_rect r = rects[t];
    const uint8_t* p0 = tab.p0[f];
    const uint8_t* p1 = tab.p1[f];
    const uint8_t* p2 = tab.p2[f];
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
        for (int k = 0; k < 4; ++k) {
            const uint32_t t00 = cut_tap<SRC, VF>(p0, p1, p2, pitch0, pitch1, y0, x0[k]);
            const uint32_t t01 = cut_tap<SRC, VF>(p0, p1, p2, pitch0, pitch1, y0, x1[k]);
            const uint32_t t10 = cut_tap<SRC, VF>(p0, p1, p2, pitch0, pitch1, y1, x0[k]);
            const uint32_t t11 = cut_tap<SRC, VF>(p0, p1, p2, pitch0, pitch1, y1, x1[k]);
            uint32_t v = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int s = 8 * c;
                const int h0 = (int)((t00 >> s) & 255) * a0[k] + (int)((t01 >> s) & 255) * a1[k];
                const int h1 = (int)((t10 >> s) & 255) * a0[k] + (int)((t11 >> s) & 255) * a1[k];
                v |= (uint32_t)cv_linear_vpass(b0, b1, h0, h1) << s;
            }
            p[k] = v;
        }
        uint32_t* o = reinterpret_cast<uint32_t*>(out + (size_t)Y * W * 3);
        o[0] = p[0] | (p[1] << 24);
        o[1] = (p[1] >> 8) | (p[2] << 16);
        o[2] = (p[2] >> 16) | (p[3] << 8);
    }
}

// One workgroup per frame walks the T * rows (tile, row) items in order, 1024 at a time: keep flag, ballot, the 16 wave counts through
// LDS, write at base + prefix.
__global__ void __launch_bounds__(1024) merge_collect_kernel(MergeParams p) {
    __shared__ uint32_t wave_cnt[16];
    __shared__ int truncated;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = p.T * p.rows;
    float* cand = p.cand + (size_t)f * cap * 16;
    if (tid == 0) truncated = 0;
    __syncthreads();
    const float W = (float)p.W, H = (float)p.H;
    uint32_t base = 0;
    for (int j0 = 0; j0 < cap; j0 += 1024) {
        const int j = j0 + tid;
        bool keep = false;
        int t = 0, row = 0;
        float c[4] = {0.f, 0.f, 0.f, 0.f};
        cf_tile_rect r = {0, 0, 2, 2};
        if (j < cap) {
            t = j / p.rows; row = j - t * p.rows;
            const int img = f * p.T + t;
            const int n = p.counts[img];
            if (row == 0 && n > p.rows) truncated = 1;                    // (every writer stores the same value)
            if (row < min(n, p.rows)) {
                r = p.rects[t];
                const float4 q = *reinterpret_cast<const float4*>(p.dets_net + ((size_t)img * p.rows + row) * 4);
                c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
                keep = isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(c[3]);
                if (r.x0 > 0 && c[0] < p.edge) keep = false;
                if (r.x0 + r.w < p.w && c[2] > W - p.edge) keep = false;
                if (r.y0 > 0 && c[1] < p.edge) keep = false;
                if (r.y0 + r.h < p.h && c[3] > H - p.edge) keep = false;
            }
        }
        const unsigned long long bal = __ballot(keep);
        __syncthreads();                                                  // the counts of the round before have been read
        if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = 0, total = 0;
        for (int w2 = 0; w2 < 16; ++w2) { if (w2 < wave) off += wave_cnt[w2]; total += wave_cnt[w2]; }
        if (keep) {
            const uint32_t pos = base + off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            const size_t src = (size_t)(f * p.T + t) * p.rows + row;
            const double sx = (double)r.w / (double)p.W, sy = (double)r.h / (double)p.H;
            const double ox = (double)r.x0, oy = (double)r.y0;
            float o[16];
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (float)((double)c[k] * ((k & 1) ? sy : sx) + ((k & 1) ? oy : ox));
            o[4] = p.scores[src * p.score_stride];
            const float* l = p.lms_net + src * 10;
#pragma unroll
            for (int k = 0; k < 10; ++k) o[5 + k] = (float)((double)l[k] * ((k & 1) ? sy : sx) + ((k & 1) ? oy : ox));
            o[15] = 0.0f;
            float4* d = reinterpret_cast<float4*>(cand + (size_t)pos * 16);
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        }
        base += total;
    }
    __syncthreads();
    if (tid == 0) { p.cand_count[f] = (int)base; p.flags[f] = truncated; }
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
        switch (format) {
            case CF_YUV_NV12: hipLaunchKernelGGL((cut_tiles_kernel<1, false>), grid, dim3(256), 0, s, tab, rects, out, T, pitch0, pitch1, H, W); break;
            case CF_YUV_NV21: hipLaunchKernelGGL((cut_tiles_kernel<1, true>), grid, dim3(256), 0, s, tab, rects, out, T, pitch0, pitch1, H, W); break;
            case CF_YUV_I420: case CF_YUV_YV12: hipLaunchKernelGGL((cut_tiles_kernel<2, false>), grid, dim3(256), 0, s, tab, rects, out, T, pitch0, pitch1, H, W); break;
            default: hipLaunchKernelGGL((cut_tiles_kernel<0, false>), grid, dim3(256), 0, s, tab, rects, out, T, pitch0, pitch1, H, W); break;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

size_t merge_mask_bytes(int Bf, int T, int rows) {
    const size_t cap = (size_t)T * rows;
    return (size_t)Bf * cap * ((cap + 63) / 64) * sizeof(unsigned long long);
}

hipError_t launch_merge_tiles(hipStream_t s, const MergeParams& p) {
    if (p.Bf < 1 || p.T < 1 || p.rows < 1 || p.max_out < 1 || (long long)p.T * p.rows > INT_MAX / 16 || p.H < 1 || p.W < 1 || p.score_stride < 1 ||
        (p.metric != CF_MERGE_IOU && p.metric != CF_MERGE_IOS) || !p.rects || !p.dets_net || !p.scores || !p.lms_net || !p.counts || !p.cand ||
        !p.cand_count || !p.order || !p.mask || !p.dets || !p.lms || !p.corners || !p.out_counts || !p.flags)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(merge_collect_kernel, dim3(p.Bf), dim3(1024), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ThreshParams q{};
    q.B = p.Bf; q.cap = p.T * p.rows; q.nms_thresh = p.thresh; q.metric = p.metric;
    q.cand = p.cand; q.cand_count = p.cand_count; q.order = p.order; q.mask = p.mask;
    q.max_out = p.max_out; q.dets = p.dets; q.lms = p.lms; q.dets_net = p.corners; q.counts = p.out_counts;
    return launch_nms_stages(s, q);
}

}  // namespace cf
