// Aspect-preserving (letterbox) input: the fit of source frames into the network's canvas and the mapping of the decode's rows back
// into frame pixels.
//
// GEOMETRY (fit_geometry; integers, 64-bit products).  An h x w frame in an H x W canvas keeps its size when upscale == 0 and it fits
// (rw = w, rh = h); else, height-limited (w * H <= h * W): rh = H, rw = max(1, (2 * w * H + h) / (2 * h)); else rw = W,
// rh = max(1, (2 * h * W + w) / (2 * w)).  CF_FIT_CENTER: dx = (W - rw) / 2, dy = (H - rh) / 2; CF_FIT_TOPLEFT: dx = dy = 0.
//
// FIT.  One launch writes the network's uint8 input batch [B][H][W][3] BGR from B full-resolution frames (BGR rows or 4:2:0 planes,
// pitched, read in place):
//   canvas_b[dy : dy + rh, dx : dx + rw] = resize(bgr(frame_b), (rh, rw)),   every other pixel = fill
// with bgr() the fixed-point BT.601 conversion of cf_yuvmath.h (the identity for BGR frames) and resize the fixed-point INTER_LINEAR of
// cf_cvresize.h from (h, w) to (rh, rw): "resize, then pad".  rw == w and rh == h give the coefficients 2048 / 0: the source bytes.
// fit_frames_kernel<SRC, VF, ROT> runs the padded lane of cf_cutpx.h on this one geometry (ROT 2: the rot 180 of cf_rot.hip, mirrored
// taps): a lane owns four adjacent CANVAS columns -- each of them content or padding on its own, dx and dx + rw are no multiples of 4 -- whose
// taps and coefficients are computed once and serve kFitRows canvas rows, each row going out as three dword stores (W % 4 == 0),
// lane-contiguous.  Rows wholly in the padding, and lanes whose four columns are, are written as fill without touching the source; a
// padding column beside content computes the edge column's taps and drops them.  The taps are byte loads; every tap lies inside the
// frame, pitch padding is never read.
//
// UNFIT.  One workgroup per image walks the rows the threshold decode kept, i < min(count, rows), in keep order:
//   * dropped when a corner is not finite, or when its centre cx = (x1 + x2) * 0.5f, cy likewise (float32) lies outside the content:
//     kept iff dx <= cx < dx + rw and dy <= cy < dy + rh;
//   * else X = (float)(((double)x - (double)dx) * ((double)w / (double)rw)), Y likewise with dy and h / rh, for the four corners and the
//     ten landmark values (float64 in this order, no contraction: the file is built with -ffp-contract=off); the score is copied.
// The compaction (compact_pos, cf_collect.h) is a prefix sum, never an atomic: the order is the decode's.  Behind a rotated forward (cf_rot.hip) the same kernel maps
// through the turn as well: unfit_rows_kernel<ROT>, whose ROT == 0 instance is the map above.
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_cutpx.h"
#include "cf_collect.h"
#include <string>

namespace cf {
namespace {

// canvas rows per lane (one set of column coefficients).  The cutter's 8 left 16 frames of 1080p with 3 waves per SIMD, 44 % of them
// storing fill only: 35 / 55 us (NV12 / BGR) against 23 / 32 us with 4; 2 and 1 measured the same as 4 (profiles/fit.md)
constexpr int kFitRows = 4;
using FitPtrs = FramePtrs<kFitFrames>;

// The padded lane of cf_cutpx.h on one geometry: the whole upright view is the source, g its content.  ROT: 0 = as stored, 2 = rot 180,
// the same lane layout on mirrored taps (adjacent canvas columns are still adjacent stored columns; hu = h, wu = w).
template <int SRC, bool VF, int ROT>
__global__ void __launch_bounds__(256) fit_frames_kernel(FitPtrs tab, uint8_t* dst, cf_fit_geom g, uint32_t fill, int h, int w, int pitch0,
                                                         int pitch1, int H, int W) {
    const int f = blockIdx.y;
    const int gw = W >> 2, ng = (H + kFitRows - 1) / kFitRows;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ng * gw) return;
    const int grp = i / gw, X0 = (i - grp * gw) << 2, Y0 = grp * kFitRows;
    padded_lane<SRC, VF, ROT>(cf_view{0, 0, w, h, g.dx, g.dy, g.rw, g.rh}, SrcPlanes{tab.p0[f], tab.p1[f], tab.p2[f], pitch0, pitch1, h, w},
                              dst + (size_t)f * H * W * 3, W, X0, Y0, min(H, Y0 + kFitRows), fill);
}

// One workgroup per image walks its rows in order, 1024 at a time, and compacts the kept ones (compact_pos).  ROT: the quarter turns of a
// rotated forward (cf_rot.hip has the statement); p.h x p.w is the STORED frame, the content of the canvas its upright view of hu x wu.
// ROT == 0 is the unfit above.  (The upright point has no source offset to add: a sum with 0.0 would turn a -0.0 into +0.0.)
template <int ROT>
__global__ void __launch_bounds__(1024) unfit_rows_kernel(UnfitParams p) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int count = p.counts[b], n = min(max(count, 0), p.rows);
    const float xlo = (float)p.g.dx, xhi = (float)(p.g.dx + p.g.rw), ylo = (float)p.g.dy, yhi = (float)(p.g.dy + p.g.rh);
    const int hu = (ROT & 1) ? p.w : p.h, wu = (ROT & 1) ? p.h : p.w;
    const double sx = (double)wu / (double)p.g.rw, sy = (double)hu / (double)p.g.rh;
    const double ox = (double)p.g.dx, oy = (double)p.g.dy;
    auto map = [&](float x, float y, float& X, float& Y) { turn_point<ROT>(((double)x - ox) * sx, ((double)y - oy) * sy, p.h, p.w, X, Y); };
    uint32_t base = 0;
    for (int j0 = 0; j0 < n; j0 += 1024) {               // (n is uniform over the workgroup: so is the trip count)
        const int row = j0 + tid;
        bool keep = false;
        float c[4] = {0.f, 0.f, 0.f, 0.f};
        const size_t src = (size_t)b * p.rows + row;
        if (row < n) {
            const float4 q = *reinterpret_cast<const float4*>(p.dets_net + src * 4);
            c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
            keep = isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(c[3]);
            const float cx = (c[0] + c[2]) * 0.5f, cy = (c[1] + c[3]) * 0.5f;
            if (!(cx >= xlo && cx < xhi && cy >= ylo && cy < yhi)) keep = false;
        }
        const uint32_t pos = compact_pos(keep, base);
        if (keep && pos < (uint32_t)p.max_out) {
            const size_t d = (size_t)b * p.max_out + pos;
            float o[4];
            turn_box<ROT>(c, map, o);
            *reinterpret_cast<float4*>(p.corners + d * 4) = make_float4(o[0], o[1], o[2], o[3]);
            float* dd = p.dets + d * 5;
            dd[0] = o[0]; dd[1] = o[1]; dd[2] = o[2]; dd[3] = o[3];
            dd[4] = p.scores[src * p.score_stride];
            turn_landmarks(p.lms_net + src * 10, map, p.lms + d * 10);
        }
    }
    if (tid == 0) { p.out_counts[b] = (int)base; p.flags[b] = count > p.rows ? 1 : 0; }
}

}  // namespace

int fit_geometry(int anchor, int upscale, int h, int w, int H, int W, cf_fit_geom* g) {
    if (!g || (anchor != CF_FIT_CENTER && anchor != CF_FIT_TOPLEFT) || (upscale != 0 && upscale != 1) || h < 1 || w < 1 || H < 1 || W < 1) return CF_EINVAL;
    long long rw, rh;
    if (!upscale && h <= H && w <= W) { rw = w; rh = h; }
    else if ((long long)w * H <= (long long)h * W) { rh = H; rw = std::max(1LL, (2LL * w * H + h) / (2LL * h)); }
    else { rw = W; rh = std::max(1LL, (2LL * h * W + w) / (2LL * w)); }
    g->rw = (int)rw; g->rh = (int)rh;
    g->dx = anchor == CF_FIT_CENTER ? (W - (int)rw) / 2 : 0;
    g->dy = anchor == CF_FIT_CENTER ? (H - (int)rh) / 2 : 0;
    return CF_OK;
}

const char* fit_check(std::string& why, const cf_fit_opts* o, int format, int B, int h, int w, int pitch0, int pitch1, int H, int W) {
    char b[224];
    auto say = [&](const char* s) { why = s; return why.c_str(); };
    if (!o) return say("null options");
    if (o->anchor != CF_FIT_CENTER && o->anchor != CF_FIT_TOPLEFT) { snprintf(b, sizeof b, "unknown anchor %d (0 = CF_FIT_CENTER, 1 = CF_FIT_TOPLEFT)", o->anchor); return say(b); }
    if (o->upscale != 0 && o->upscale != 1) { snprintf(b, sizeof b, "upscale=%d must be 0 or 1", o->upscale); return say(b); }
    if (H < 1 || W < 4 || (W & 3)) { snprintf(b, sizeof b, "H=%d, W=%d: W must be a multiple of 4 and H at least 1", H, W); return say(b); }
    if (const char* geo = frame_geometry_check(FrameGeo{format, B, h, w, pitch0, pitch1}, 2, false)) {
        snprintf(b, sizeof b, "%s (format=%d, B=%d, h=%d, w=%d, pitch0=%d, pitch1=%d)", geo, format, B, h, w, pitch0, pitch1);
        return say(b);
    }
    return nullptr;
}

// planes: B x {p0, p1, p2} device addresses (HOST table); the caller has run fit_check / rot_check and fit_geometry / rot_geometry
hipError_t launch_fit_frames(hipStream_t s, int rot, int format, const void* const* planes, int B, int h, int w, int pitch0, int pitch1,
                             const cf_fit_geom& g, const uint8_t* fill, uint8_t* dst, int H, int W) {
    if ((rot != 0 && rot != 90 && rot != 180 && rot != 270) || format < CF_YUV_NV12 || format > CF_FRAME_BGR || !planes || !dst || !fill || B < 1 || H < 1 ||
        W < 4 || (W & 3) || h < 1 || w < 1 || g.rw < 1 || g.rh < 1 || g.dx < 0 || g.dy < 0 || g.dx > W - g.rw || g.dy > H - g.rh)
        return hipErrorInvalidValue;
    const uint32_t fv = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
    const long long n = (long long)((H + kFitRows - 1) / kFitRows) * (W >> 2);
    for (int f0 = 0; f0 < B; f0 += kFitFrames) {
        const int nb = B - f0 < kFitFrames ? B - f0 : kFitFrames;
        const FitPtrs tab = frame_ptrs<kFitFrames>(planes, format, f0, nb, true);      // YV12: the I420 kernel on swapped planes (as launch_cut_tiles)
        const dim3 grid((unsigned)((n + 255) / 256), (unsigned)nb);
        uint8_t* out = dst + (size_t)f0 * H * W * 3;
        if (rot == 90 || rot == 270) launch_rot_quarter(s, rot, format, tab, nb, out, g, fv, h, w, pitch0, pitch1, H, W);
        else with_format(format, [&](auto SRC, auto VF) {
            if (rot == 0) hipLaunchKernelGGL((fit_frames_kernel<SRC, VF, 0>), grid, dim3(256), 0, s, tab, out, g, fv, h, w, pitch0, pitch1, H, W);
            else hipLaunchKernelGGL((fit_frames_kernel<SRC, VF, 2>), grid, dim3(256), 0, s, tab, out, g, fv, h, w, pitch0, pitch1, H, W);
        });
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_unfit_rows(hipStream_t s, const UnfitParams& p) { return launch_unrot_rows(s, p, 0); }

// rot: 0, 90, 180, 270 (checked by the caller); p.g places the UPRIGHT view of the p.h x p.w frames
hipError_t launch_unrot_rows(hipStream_t s, const UnfitParams& p, int rot) {
    if ((rot != 0 && rot != 90 && rot != 180 && rot != 270) || p.B < 1 || p.rows < 1 || p.max_out < 1 || p.h < 1 || p.w < 1 || p.g.rw < 1 || p.g.rh < 1 ||
        p.score_stride < 1 || !p.dets_net || !p.scores || !p.lms_net || !p.counts || !p.dets || !p.lms || !p.corners || !p.out_counts || !p.flags)
        return hipErrorInvalidValue;
    switch (rot) {
        case 90: hipLaunchKernelGGL(unfit_rows_kernel<1>, dim3(p.B), dim3(1024), 0, s, p); break;
        case 180: hipLaunchKernelGGL(unfit_rows_kernel<2>, dim3(p.B), dim3(1024), 0, s, p); break;
        case 270: hipLaunchKernelGGL(unfit_rows_kernel<3>, dim3(p.B), dim3(1024), 0, s, p); break;
        default: hipLaunchKernelGGL(unfit_rows_kernel<0>, dim3(p.B), dim3(1024), 0, s, p); break;
    }
    return hipGetLastError();
}

}  // namespace cf
