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
// MERGE (collect_rows_kernel<ViewItems, 0> of cf_collect.h, launched by cf_tiles.hip's launch_merge).  It fills the candidate table [Bf][cap = V * rows][16] (the record of ThreshParams::cand) from the
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
//
// PACKED VIEWS (further down).  A placement (cf_place) puts one view of one frame into one canvas, so several levels and frames share a
// canvas: cut_packed_kernel writes all canvases in one launch, one writer per byte, and the collect kernel walks a frame's placements
// (PlacedItems).
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_cutpx.h"
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

namespace cf {
namespace {

constexpr int kViewFrames = 64;                      // frames per launch: 3 x 64 pointers = 1.5 KB of kernel arguments
constexpr int kViewRows = 4;                         // canvas rows per lane (one set of column coefficients): the fit's figure, cf_fit.hip says why not 8
using ViewPtrs = FramePtrs<kViewFrames>;

// the padded lane of cf_cutpx.h on view blockIdx.y of the device's table
template <int SRC, bool VF>
__global__ void __launch_bounds__(256) cut_views_kernel(ViewPtrs tab, const cf_view* __restrict__ views, uint8_t* dst, int V, uint32_t fill,
                                                        int pitch0, int pitch1, int H, int W) {
    const int v = blockIdx.y, f = blockIdx.z;
    const int gw = W >> 2, ng = (H + kViewRows - 1) / kViewRows;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ng * gw) return;
    const int grp = i / gw, X0 = (i - grp * gw) << 2, Y0 = grp * kViewRows;
    padded_lane<SRC, VF, 0>(views[v], SrcPlanes{tab.p0[f], tab.p1[f], tab.p2[f], pitch0, pitch1, 0, 0}, dst + ((size_t)f * V + v) * H * W * 3, W, X0, Y0,
                            min(H, Y0 + kViewRows), fill);
}

// PACKED VIEWS.  A placement puts one view of one frame into one canvas; a canvas holds any number of them, disjoint.
//
// CUT.  One launch writes all N canvases, every byte once.  A workgroup owns a kPackTileW x kPackTileH tile of canvas blockIdx.y; its
// lanes keep the shape of cut_views_kernel (four adjacent canvas columns, kViewRows rows, three dword stores per row), 32 lanes across
// and 8 down.  The placements are sorted by canvas on the host (t.cv_off: the CSR).  In rounds of kPackList placements of its canvas,
// every thread tests one against the tile and the hits are compacted into an LDS list (list_round, cf_cutpx.h); a list can therefore
// not overflow, a canvas with more placements takes more rounds.  Every lane then walks the list: a placement that reaches into its
// 4 x kViewRows pixels gets its column taps and coefficients computed once (col_coeffs) and serves the lane's rows (bilinear_px); the
// pixels live in registers from the first round to the stores at the end, `fill` where no placement wrote.  A tile no placement touches
// stores fill and reads no frame.  Taps inside the placement's source rectangle.  ROT: 0 = frames as stored; 2 = rot 180 (h x w the
// stored frame), the same layout on mirrored taps: adjacent canvas columns are still adjacent stored columns.
constexpr int kPackTileW = 128, kPackTileH = 8 * kViewRows;

template <int SRC, bool VF, int ROT>
__global__ void __launch_bounds__(256) cut_packed_kernel(PackDev t, uint8_t* dst, uint32_t fill, int h, int w, int pitch0, int pitch1, int H, int W,
                                                         int tiles_x) {
    __shared__ int s_list[kPackList];
    __shared__ int s_cnt[4];
    const int tid = (int)threadIdx.x, n = (int)blockIdx.y;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int tx0 = tx * kPackTileW, ty0 = ty * kPackTileH;
    const int X0 = tx0 + 4 * (tid & 31), Y0 = ty0 + kViewRows * (tid >> 5);
    const bool live = X0 < W && Y0 < H;                   // (W % 4 == 0: a live lane's four columns are inside)
    uint32_t px[kViewRows][4];
#pragma unroll
    for (int i = 0; i < kViewRows; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) px[i][k] = fill;
    const int k0 = t.cv_off[n], k1 = t.cv_off[n + 1];
    for (int base = k0; base < k1; base += kPackList) {   // uniform trip count
        const int cnt = list_round(t, base, k1, tx0, ty0, kPackTileW, kPackTileH, s_list, s_cnt);
        if (live)
            for (int j = 0; j < cnt; ++j) {
                const cf_place& pl = t.places[__builtin_amdgcn_readfirstlane(s_list[j])];
                const cf_view r = pl.view;
                if (X0 + 4 <= r.dx || X0 >= r.dx + r.dw || Y0 + kViewRows <= r.dy || Y0 >= r.dy + r.dh) continue;      // not this lane's pixels
                bool in[4];
                int x0[4], x1[4], a0[4], a1[4];
                col_coeffs(r, X0, in, x0, x1, a0, a1);
                const SrcPlanes src{t.planes[3 * pl.frame], t.planes[3 * pl.frame + 1], t.planes[3 * pl.frame + 2], pitch0, pitch1, h, w};
#pragma unroll
                for (int i = 0; i < kViewRows; ++i) {
                    const int y = Y0 + i - r.dy;
                    if (y < 0 || y >= r.dh) continue;          // (inside the content, so inside the canvas)
                    int y0, y1, b0, b1;
                    cv_linear_coeffs(y, r.sh, r.dh, false, y0, y1, b0, b1);
                    y0 += r.sy0; y1 += r.sy0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t v = bilinear_px<SRC, VF, ROT>(src, y0, y1, b0, b1, x0[k], x1[k], a0[k], a1[k]);
                        if (in[k]) px[i][k] = v;
                    }
                }
            }
        __syncthreads();                                      // s_list and s_cnt are rewritten by the next round
    }
    if (!live) return;
    uint8_t* out = dst + (((size_t)n * H + Y0) * W + X0) * 3;
#pragma unroll
    for (int i = 0; i < kViewRows; ++i)
        if (Y0 + i < H) quad_store(out + (size_t)i * W * 3, px[i]);
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
        with_format(format, [&](auto SRC, auto VF) {
            hipLaunchKernelGGL((cut_views_kernel<SRC, VF>), grid, dim3(256), 0, s, tab, views, out, V, fv, pitch0, pitch1, H, W);
        });
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The first-fit shelf packer of cf_pack_views (the rule is stated in include/centerface_hip.h and restated in tests/pack_cases.py).
int pack_views(const cf_view* views, int V, int Bf, int H, int W, int gutter, cf_place* places, int cap, int* n_canvases) {
    struct Shelf { long long y, height, x_next; };
    struct Canvas { std::vector<Shelf> shelves; long long y_next; };
    std::vector<Canvas> cvs;
    long long k = 0;
    for (int f = 0; f < Bf; ++f)
        for (int v = 0; v < V; ++v, ++k) {
            const long long dw = views[v].dw, dh = views[v].dh;
            int at = -1;
            long long x = 0, y = 0;
            for (size_t c = 0; c < cvs.size() && at < 0; ++c) {
                Canvas& cv = cvs[c];
                for (Shelf& s : cv.shelves)
                    if (dh <= s.height && s.x_next + dw <= W) { x = s.x_next; y = s.y; s.x_next += dw + gutter; at = (int)c; break; }
                if (at < 0 && cv.y_next + dh <= H) {
                    x = 0; y = cv.y_next;
                    cv.shelves.push_back(Shelf{y, dh, dw + gutter});
                    cv.y_next = y + dh + gutter;
                    at = (int)c;
                }
            }
            if (at < 0) {
                cvs.push_back(Canvas{{Shelf{0, dh, dw + gutter}}, dh + gutter});
                at = (int)cvs.size() - 1;
            }
            if (k < cap) {
                cf_place& p = places[k];
                p.frame = f; p.canvas = at; p.view = views[v];
                p.view.dx = (int)x; p.view.dy = (int)y;
            }
        }
    *n_canvases = (int)cvs.size();
    return CF_OK;
}

const char* pack_check(std::string& why, int h, int w, const cf_place* places, int P, int N, int Bf, int H, int W) {
    auto say = [&](const std::string& s) { why = s; return why.c_str(); };
    char b[400];
    if (P < 1) return say("P must be at least 1");
    if (N < 1) return say("N must be at least 1");
    if (!places) return say("null placement table");
    for (int k = 0; k < P; ++k) {
        const cf_place& p = places[k];
        if (p.frame < 0 || p.frame >= Bf) { snprintf(b, sizeof b, "placement %d names frame %d outside [0, %d)", k, p.frame, Bf); return say(b); }
        if (p.canvas < 0 || p.canvas >= N) { snprintf(b, sizeof b, "placement %d names canvas %d outside [0, %d)", k, p.canvas, N); return say(b); }
        std::string text;
        if (views_table_check(text, h, w, &p.view, 1, H, W)) { snprintf(b, sizeof b, "placement %d: %s", k, text.c_str()); return say(b); }
    }
    // overlaps: per canvas a sweep down the contents' top rows
    std::vector<int> idx((size_t)P);
    for (int k = 0; k < P; ++k) idx[k] = k;
    std::sort(idx.begin(), idx.end(), [&](int a, int c) {
        const cf_place &p = places[a], &q = places[c];
        return p.canvas != q.canvas ? p.canvas < q.canvas : p.view.dy != q.view.dy ? p.view.dy < q.view.dy : a < c;
    });
    for (int i = 0; i < P; ++i) {
        const cf_place& p = places[idx[i]];
        for (int j = i + 1; j < P; ++j) {
            const cf_place& q = places[idx[j]];
            if (q.canvas != p.canvas || q.view.dy >= p.view.dy + p.view.dh) break;
            if (q.view.dx < p.view.dx + p.view.dw && p.view.dx < q.view.dx + q.view.dw) {
                snprintf(b, sizeof b, "the contents of placements %d and %d overlap on canvas %d", std::min(idx[i], idx[j]), std::max(idx[i], idx[j]), p.canvas);
                return say(b);
            }
        }
    }
    return nullptr;
}

PackHost pack_table(const cf_place* places, int P, int N, int Bf, const void* const* planes, int format) {
    PackHost t{};
    std::vector<int> idx((size_t)P), pos((size_t)P);
    for (int k = 0; k < P; ++k) idx[k] = k;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int c) { return places[a].canvas < places[c].canvas; });
    t.off_cv = (size_t)P * sizeof(cf_place);
    t.off_fr = t.off_cv + (size_t)(N + 1) * sizeof(int);
    t.off_idx = t.off_fr + (size_t)(Bf + 1) * sizeof(int);
    t.off_planes = (t.off_idx + (size_t)P * sizeof(int) + 7) & ~(size_t)7;
    t.blob.assign(t.off_planes + (size_t)3 * Bf * sizeof(void*), 0);
    cf_place* sp = (cf_place*)t.blob.data();
    int* cv = (int*)(t.blob.data() + t.off_cv);
    int* fr = (int*)(t.blob.data() + t.off_fr);
    int* fi = (int*)(t.blob.data() + t.off_idx);
    const void** pl = (const void**)(t.blob.data() + t.off_planes);
    for (int k = 0; k < P; ++k) { sp[k] = places[idx[k]]; pos[idx[k]] = k; ++cv[sp[k].canvas + 1]; ++fr[sp[k].frame + 1]; }
    for (int n = 0; n < N; ++n) cv[n + 1] += cv[n];
    for (int f = 0; f < Bf; ++f) { t.most = std::max(t.most, fr[f + 1]); fr[f + 1] += fr[f]; }
    std::vector<int> next(fr, fr + Bf);
    for (int k = 0; k < P; ++k) fi[next[places[k].frame]++] = pos[k];          // placement-index order inside a frame
    const bool swap = format == CF_YUV_YV12;                                    // the I420 kernel on swapped planes (as launch_cut_views)
    for (int f = 0; f < Bf && planes; ++f) {
        pl[3 * f] = planes[3 * f];
        pl[3 * f + 1] = planes[3 * f + (swap ? 2 : 1)];
        pl[3 * f + 2] = planes[3 * f + (swap ? 1 : 2)];
    }
    return t;
}

// rot 90 / 270 go to the quarter-turn kernel of cf_views_rot.hip
hipError_t launch_cut_packed(hipStream_t s, int rot, int format, const PackDev& t, int N, int h, int w, int pitch0, int pitch1, const uint8_t* fill,
                             uint8_t* dst, int H, int W) {
    if ((rot != 0 && rot != 90 && rot != 180 && rot != 270) || format < CF_YUV_NV12 || format > CF_FRAME_BGR || !t.places || !t.cv_off || !t.planes || !fill ||
        !dst || N < 1 || N > 65535 || H < 1 || W < 4 || (W & 3) || (rot != 0 && (h < 2 || w < 2 || ((h | w) & 1))))
        return hipErrorInvalidValue;
    const uint32_t fv = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
    if (rot == 90 || rot == 270) launch_cut_packed_quarter(s, rot, format, t, N, dst, fv, h, w, pitch0, pitch1, H, W);
    else {
        const int tiles_x = (W + kPackTileW - 1) / kPackTileW, tiles_y = (H + kPackTileH - 1) / kPackTileH;
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)N);
        with_format(format, [&](auto SRC, auto VF) {
            if (rot == 0) hipLaunchKernelGGL((cut_packed_kernel<SRC, VF, 0>), grid, dim3(256), 0, s, t, dst, fv, h, w, pitch0, pitch1, H, W, tiles_x);
            else hipLaunchKernelGGL((cut_packed_kernel<SRC, VF, 2>), grid, dim3(256), 0, s, t, dst, fv, h, w, pitch0, pitch1, H, W, tiles_x);
        });
    }
    return hipGetLastError();
}

}  // namespace cf
