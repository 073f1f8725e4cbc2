// Multi-scale detection: one batch whose images are different VIEWS of the same frames -- enlarged tiles, the aspect-true whole frame,
// the whole frame at reduced sizes -- and one merge over the per-view detections.  The statement is in include/centerface_hip.h.
//
// A view is a source rectangle of the frame (sx0, sy0, sw, sh: even, inside the frame) and a content rectangle of the canvas (dx, dy,
// dw, dh: inside (H, W), may be odd).
//
// CUT.  One launch writes the network's uint8 input batch [Bf * V][H][W][3] BGR from Bf full-resolution frames (BGR rows or 4:2:0
// planes, pitched, read in place) and a table of V views shared by the frames; image f * V + v is `fill` everywhere, except
//   canvas[dy : dy + dh, dx : dx + dw] = resize(bgr(frame_f)[sy0 : sy0 + sh, sx0 : sx0 + sw], (dh, dw))
// with bgr() the fixed-point BT.601 conversion of cf_yuvmath.h (the identity for BGR frames) and resize the fixed-point INTER_LINEAR of
// cf_cvresize.h applied to the crop: the taps clamp at the source rectangle's edges.  (dx, dy, dw, dh) = (0, 0, W, H) is the tile of
// cf_tiles.hip; the whole frame as source with the rectangle of fit_geometry as content is the canvas of cf_fit.hip.
// A lane owns four adjacent CANVAS columns -- each of them content or padding on its own -- whose taps and coefficients are computed
// once and serve kViewRows canvas rows, each row going out as three dword stores (W % 4 == 0), lane-contiguous.  Rows wholly in the
// padding, and lanes whose four columns are, are written as fill without touching the source (a quarter-size level: 15/16 of the
// canvas); a padding column beside content computes the edge column's taps and drops them.  The taps are byte loads; every tap lies
// inside the source rectangle, pitch padding is never read.
//
// MERGE.  A collect kernel fills the per-frame candidate table [Bf][cap = V * rows][16] (the record of ThreshParams::cand) from the
// per-view results of a threshold decode, in order (view ascending, keep position ascending), and the NMS stages of cf_decode.hip run
// on it.  Per row of view v, i < min(counts, rows), dropped when
//   * a corner is not finite, or
//   * its centre cx = (x1 + x2) * 0.5f, cy likewise (float32) lies outside the content: kept iff dx <= cx < dx + dw and
//     dy <= cy < dy + dh (the unfit's rule), or
//   * its box comes within `edge` of a content side whose SOURCE side is interior to the frame: x1 < (float)dx + edge when sx0 > 0,
//     x2 > (float)(dx + dw) - edge when sx0 + sw < w, the same two in y (float32; a tile view: the compares of cf_tiles.hip);
//   * else X = (float)(((double)x - (double)dx) * ((double)sw / (double)dw) + (double)sx0), Y likewise, for the four corners and the
//     ten landmark values (float64 in this order, no contraction: the file is built with -ffp-contract=off); the score is copied.
// The compaction is a prefix sum over the flattened (view, row) items, never an atomic: the order is deterministic.
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_cvresize.h"
#include "cf_yuvmath.h"
#include "cf_fitpx.h"
#include <string>
#include <vector>

namespace cf {
namespace {

constexpr int kViewFrames = 64;                      // frames per launch: 3 x 64 pointers = 1.5 KB of kernel arguments
constexpr int kViewRows = 4;                         // canvas rows per lane (one set of column coefficients): the fit's figure, cf_fit.hip says why not 8
using ViewPtrs = FramePtrs<kViewFrames>;

// SRC: 0 = BGR rows, 1 = one interleaved chroma plane (NV12 / NV21), 2 = two chroma planes (I420; YV12 on a swapped table);
// VF: V first in the interleaved pairs (NV21).  One source pixel -> B | G << 8 | R << 16
template <int SRC, bool VF>
__device__ __forceinline__ uint32_t view_tap(const uint8_t* p0, const uint8_t* p1, const uint8_t* p2, int pitch0, int pitch1, int y, int x) {
    if constexpr (SRC == 0) {
        const uint8_t* q = p0 + (size_t)y * pitch0 + 3 * x;
        return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    } else {
        return yuv_px(p0[(size_t)y * pitch0 + x], chroma_at<SRC == 1, VF>(p1, p2, pitch1, y >> 1, x >> 1));
    }
}

template <int SRC, bool VF>
__global__ void __launch_bounds__(256) cut_views_kernel(ViewPtrs tab, const cf_view* __restrict__ views, uint8_t* dst, int V, uint32_t fill,
                                                        int pitch0, int pitch1, int H, int W) {
    const int v = blockIdx.y, f = blockIdx.z;
    const int gw = W >> 2, ng = (H + kViewRows - 1) / kViewRows;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ng * gw) return;
    const int grp = i / gw, X0 = (i - grp * gw) << 2;
    const cf_view r = views[v];
    uint8_t* out = dst + (((size_t)f * V + v) * H * W + X0) * 3;
    const int Y0 = grp * kViewRows, Yend = min(H, Y0 + kViewRows);
    const uint32_t pad[4] = {fill, fill, fill, fill};
    bool in[4];
    int x0[4], x1[4], a0[4], a1[4];
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = X0 + k - r.dx;
        in[k] = x >= 0 && x < r.dw;
        cv_linear_coeffs(min(max(x, 0), r.dw - 1), r.sw, r.dw, true, x0[k], x1[k], a0[k], a1[k]);      // a padding column beside content: the edge's taps, not used
        x0[k] += r.sx0; x1[k] += r.sx0;
        any = any || in[k];
    }
    if (!any || Yend <= r.dy || Y0 >= r.dy + r.dh) {     // the lane's columns, or all of its rows, are padding: the source is not touched
        for (int Y = Y0; Y < Yend; ++Y) fit_store(out + (size_t)Y * W * 3, pad);
        return;
    }
    const uint8_t* p0 = tab.p0[f];
    const uint8_t* p1 = tab.p1[f];
    const uint8_t* p2 = tab.p2[f];
    for (int Y = Y0; Y < Yend; ++Y) {
        const int y = Y - r.dy;
        if (y < 0 || y >= r.dh) { fit_store(out + (size_t)Y * W * 3, pad); continue; }
        int y0, y1, b0, b1;
        cv_linear_coeffs(y, r.sh, r.dh, false, y0, y1, b0, b1);
        y0 += r.sy0; y1 += r.sy0;
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t t00 = view_tap<SRC, VF>(p0, p1, p2, pitch0, pitch1, y0, x0[k]);
            const uint32_t t01 = view_tap<SRC, VF>(p0, p1, p2, pitch0, pitch1, y0, x1[k]);
            const uint32_t t10 = view_tap<SRC, VF>(p0, p1, p2, pitch0, pitch1, y1, x0[k]);
            const uint32_t t11 = view_tap<SRC, VF>(p0, p1, p2, pitch0, pitch1, y1, x1[k]);
            uint32_t ch[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int s = 8 * c;
                const int h0 = (int)((t00 >> s) & 255) * a0[k] + (int)((t01 >> s) & 255) * a1[k];
                const int h1 = (int)((t10 >> s) & 255) * a0[k] + (int)((t11 >> s) & 255) * a1[k];
                ch[c] = (uint32_t)cv_linear_vpass(b0, b1, h0, h1);
            }
            p[k] = in[k] ? pack_bgr(ch[0], ch[1], ch[2]) : fill;
        }
        fit_store(out + (size_t)Y * W * 3, p);
    }
}

// One workgroup per frame walks the V * rows (view, row) items in order, 1024 at a time: keep flag, ballot, the 16 wave counts through
// LDS, write at base + prefix (as merge_collect_kernel).
__global__ void __launch_bounds__(1024) views_collect_kernel(ViewMergeParams p) {
    __shared__ uint32_t wave_cnt[16];
    __shared__ int truncated;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = p.V * p.rows;
    float* cand = p.cand + (size_t)f * cap * 16;
    if (tid == 0) truncated = 0;
    __syncthreads();
    uint32_t base = 0;
    for (int j0 = 0; j0 < cap; j0 += 1024) {
        const int j = j0 + tid;
        bool keep = false;
        int v = 0, row = 0;
        float c[4] = {0.f, 0.f, 0.f, 0.f};
        cf_view r = {0, 0, 2, 2, 0, 0, 1, 1};
        if (j < cap) {
            v = j / p.rows; row = j - v * p.rows;
            const int img = f * p.V + v;
            const int n = p.counts[img];
            if (row == 0 && n > p.rows) truncated = 1;                    // (every writer stores the same value)
            if (row < min(n, p.rows)) {
                r = p.views[v];
                const float4 q = *reinterpret_cast<const float4*>(p.dets_net + ((size_t)img * p.rows + row) * 4);
                c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
                keep = isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(c[3]);
                const float xlo = (float)r.dx, xhi = (float)(r.dx + r.dw), ylo = (float)r.dy, yhi = (float)(r.dy + r.dh);
                const float cx = (c[0] + c[2]) * 0.5f, cy = (c[1] + c[3]) * 0.5f;
                if (!(cx >= xlo && cx < xhi && cy >= ylo && cy < yhi)) keep = false;
                if (r.sx0 > 0 && c[0] < xlo + p.edge) keep = false;
                if (r.sx0 + r.sw < p.w && c[2] > xhi - p.edge) keep = false;
                if (r.sy0 > 0 && c[1] < ylo + p.edge) keep = false;
                if (r.sy0 + r.sh < p.h && c[3] > yhi - p.edge) keep = false;
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
            const size_t src = (size_t)(f * p.V + v) * p.rows + row;
            const double sx = (double)r.sw / (double)r.dw, sy = (double)r.sh / (double)r.dh;
            const double dx = (double)r.dx, dy = (double)r.dy, ox = (double)r.sx0, oy = (double)r.sy0;
            float o[16];
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (float)(((double)c[k] - ((k & 1) ? dy : dx)) * ((k & 1) ? sy : sx) + ((k & 1) ? oy : ox));
            o[4] = p.scores[src * p.score_stride];
            const float* l = p.lms_net + src * 10;
#pragma unroll
            for (int k = 0; k < 10; ++k) o[5 + k] = (float)(((double)l[k] - ((k & 1) ? dy : dx)) * ((k & 1) ? sy : sx) + ((k & 1) ? oy : ox));
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

int view_layout(const cf_view_opts* o, int h, int w, int H, int W, cf_view* views, int cap, int* n) {
    if (!o || !n || cap < 0 || (cap > 0 && !views)) return CF_EINVAL;
    if ((o->anchor != CF_FIT_CENTER && o->anchor != CF_FIT_TOPLEFT) || o->n_levels < 0 || o->n_levels > 8) return CF_EINVAL;
    for (int l = 0; l < o->n_levels; ++l) if (o->scale_pm[l] < 1 || o->scale_pm[l] > 1000) return CF_EINVAL;
    if (h < 2 || w < 2 || h > kRedactMaxSide || w > kRedactMaxSide || H < 1 || W < 1) return CF_EINVAL;
    int k = 0;
    auto put = [&](const cf_view& v) { if (k < cap) views[k] = v; ++k; };
    if (o->tile_h != 0 || o->tile_w != 0) {
        int T = 0;
        if (tile_grid(h, w, o->tile_h, o->tile_w, o->overlap, 0, nullptr, 0, &T)) return CF_EINVAL;
        if (T > 1) {                                     // (one tile is the whole frame stretched: a level says that better)
            std::vector<cf_tile_rect> rects((size_t)T);
            if (tile_grid(h, w, o->tile_h, o->tile_w, o->overlap, 0, rects.data(), T, &T)) return CF_EINVAL;
            for (const cf_tile_rect& r : rects) put(cf_view{r.x0, r.y0, r.w, r.h, 0, 0, W, H});
        }
    }
    if (o->n_levels > 0) {
        cf_fit_geom g{};
        if (fit_geometry(CF_FIT_CENTER, 1, h, w, H, W, &g)) return CF_EINVAL;
        for (int l = 0; l < o->n_levels; ++l) {
            const int dw = (int)std::max(1LL, ((long long)g.rw * o->scale_pm[l] + 500) / 1000);
            const int dh = (int)std::max(1LL, ((long long)g.rh * o->scale_pm[l] + 500) / 1000);
            const bool mid = o->anchor == CF_FIT_CENTER;
            put(cf_view{0, 0, w, h, mid ? (W - dw) / 2 : 0, mid ? (H - dh) / 2 : 0, dw, dh});
        }
    }
    if (k == 0) return CF_EINVAL;
    *n = k;
    return CF_OK;
}

const char* views_table_check(std::string& why, int h, int w, const cf_view* views, int V, int H, int W) {
    auto say = [&](const std::string& s) { why = s; return why.c_str(); };
    if (V < 1) return say("V must be at least 1");
    if (!views) return say("null view table");
    for (int v = 0; v < V; ++v) {
        const cf_view& r = views[v];
        const char* bad = nullptr;
        if ((r.sx0 | r.sy0 | r.sw | r.sh) & 1) bad = "has an odd source value";
        else if (r.sw < 2 || r.sh < 2) bad = "has a source smaller than 2 x 2";
        else if (r.sx0 < 0 || r.sy0 < 0 || r.sx0 > w - r.sw || r.sy0 > h - r.sh) bad = "has a source that does not lie inside the frame";
        else if (r.dw < 1 || r.dh < 1) bad = "has an empty content (dw, dh must be at least 1)";
        else if (r.dx < 0 || r.dy < 0 || r.dx > W - r.dw || r.dy > H - r.dh) bad = "has a content that does not lie inside the canvas";
        if (bad) {
            char b[320];
            snprintf(b, sizeof b, "view %d (source x0=%d, y0=%d, w=%d, h=%d; content x=%d, y=%d, w=%d, h=%d) %s (frame %d x %d, canvas %d x %d)", v, r.sx0,
                     r.sy0, r.sw, r.sh, r.dx, r.dy, r.dw, r.dh, bad, w, h, W, H);
            return say(b);
        }
    }
    return nullptr;
}

const char* views_check(std::string& why, int format, int Bf, int h, int w, int pitch0, int pitch1, const cf_view* views, int V, int H, int W) {
    auto say = [&](const std::string& s) { why = s; return why.c_str(); };
    if (Bf < 1) return say("Bf must be at least 1");
    if (V < 1) return say("V must be at least 1");
    if (H < 1 || W < 4 || (W & 3)) return say("W must be a multiple of 4 and H at least 1");
    if (const char* geo = frame_geometry_check(FrameGeo{format, Bf, h, w, pitch0, pitch1}, 2, true)) return say(geo);
    return views_table_check(why, h, w, views, V, H, W);
}

// planes: Bf x {p0, p1, p2} device addresses (HOST table); views: V views on the DEVICE; the caller has run views_check
hipError_t launch_cut_views(hipStream_t s, int format, const void* const* planes, int Bf, int pitch0, int pitch1, const cf_view* views, int V,
                            const uint8_t* fill, uint8_t* dst, int H, int W) {
    if (format < CF_YUV_NV12 || format > CF_FRAME_BGR || !planes || !views || !fill || !dst || Bf < 1 || V < 1 || V > 65535 || H < 1 || W < 4 || (W & 3))
        return hipErrorInvalidValue;
    const uint32_t fv = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
    const long long n = (long long)((H + kViewRows - 1) / kViewRows) * (W >> 2);
    for (int f0 = 0; f0 < Bf; f0 += kViewFrames) {
        const int nb = Bf - f0 < kViewFrames ? Bf - f0 : kViewFrames;
        const ViewPtrs tab = frame_ptrs<kViewFrames>(planes, format, f0, nb, true);      // YV12: the I420 kernel on swapped planes (as launch_cut_tiles)
        const dim3 grid((unsigned)((n + 255) / 256), (unsigned)V, (unsigned)nb);
        uint8_t* out = dst + (size_t)f0 * V * H * W * 3;
        switch (format) {
            case CF_YUV_NV12: hipLaunchKernelGGL((cut_views_kernel<1, false>), grid, dim3(256), 0, s, tab, views, out, V, fv, pitch0, pitch1, H, W); break;
            case CF_YUV_NV21: hipLaunchKernelGGL((cut_views_kernel<1, true>), grid, dim3(256), 0, s, tab, views, out, V, fv, pitch0, pitch1, H, W); break;
            case CF_YUV_I420: case CF_YUV_YV12: hipLaunchKernelGGL((cut_views_kernel<2, false>), grid, dim3(256), 0, s, tab, views, out, V, fv, pitch0, pitch1, H, W); break;
            default: hipLaunchKernelGGL((cut_views_kernel<0, false>), grid, dim3(256), 0, s, tab, views, out, V, fv, pitch0, pitch1, H, W); break;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_merge_views(hipStream_t s, const ViewMergeParams& p) {
    if (p.Bf < 1 || p.V < 1 || p.rows < 1 || p.max_out < 1 || (long long)p.V * p.rows > INT_MAX / 16 || p.h < 1 || p.w < 1 || p.score_stride < 1 ||
        (p.metric != CF_MERGE_IOU && p.metric != CF_MERGE_IOS) || !p.views || !p.dets_net || !p.scores || !p.lms_net || !p.counts || !p.cand ||
        !p.cand_count || !p.order || !p.mask || !p.dets || !p.lms || !p.corners || !p.out_counts || !p.flags)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(views_collect_kernel, dim3(p.Bf), dim3(1024), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ThreshParams q{};
    q.B = p.Bf; q.cap = p.V * p.rows; q.nms_thresh = p.thresh; q.metric = p.metric;
    q.cand = p.cand; q.cand_count = p.cand_count; q.order = p.order; q.mask = p.mask;
    q.max_out = p.max_out; q.dets = p.dets; q.lms = p.lms; q.dets_net = p.corners; q.counts = p.out_counts;
    return launch_nms_stages(s, q);
}

}  // namespace cf
