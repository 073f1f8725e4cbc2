// Rotated sources: the network's canvases from the UPRIGHT view of frames that are stored a quarter, a half or three quarters of a turn
// away from it (corridor-mode cameras; phone video whose turn lives in the container's display matrix while the decoder hands out the
// surface as stored).  The statement is in include/centerface_hip.h (cf_forward_rot); in short, for a stored frame F of h x w and
// rot = the clockwise turn that makes it upright, the upright view U of hu x wu is
//   rot  90: (w, h)  U[y][x] = F[h-1-x][y]         rot 180: (h, w)  U[y][x] = F[h-1-y][w-1-x]         rot 270: (w, h)  U[y][x] = F[x][w-1-y]
// and canvas_b = what cf_fit.hip makes of bgr(U_b) with the geometry g of (hu, wu) in (H, W) -- or, stretched, g = {W, H, 0, 0}: the
// resize of cf_forward_resized.  bgr() is taken per STORED pixel (a 4:2:0 pixel's chroma is that of its own 2 x 2 block in F), so the
// kernels read F through the index map and never build U.  The rows come back through unfit_rows_kernel<ROT> (cf_fit.hip).
//
// rot 0 and rot 180 are fit_frames_kernel<.., ROT> of cf_fit.hip: rot 180 keeps that kernel's lane layout -- a lane owns four adjacent
// canvas columns whose taps lie in one source row, mirrored -- because adjacent canvas columns are still adjacent source columns.
//
// rot 90 / 270 is where the layout matters: adjacent canvas COLUMNS are adjacent source ROWS, so with the fit's layout every tap of a wave
// would be a cache line of its own.  Here the transpose happens on the output side, whose footprint does not depend on the scale: a
// workgroup owns a canvas tile of kQTY rows x kQTX columns (cf_cutpx.h); a wave's 64 lanes run along the canvas ROWS of the tile, so for
// one canvas column their taps run along ONE source row (two: the bilinear pair) and coalesce; a lane's row coefficients are computed
// once, the tile's column coefficients once per workgroup (LDS); the pixels go into an LDS tile whose row pitch of 25 dwords is odd, so
// the 32 lanes of a write group hit 32 banks; the tile leaves as whole-row dword stores, 96 contiguous bytes per canvas row.  Padding rows
// and columns are written as fill without touching the source; every tap lies inside the frame, pitch padding is never read.
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_cutpx.h"
#include <string>

namespace cf {
namespace {

// rot 90 (ROT 1) / 270 (ROT 3): grid (W tiles, H tiles, frames); thread = (wave, lane): lane -> the tile's canvas row, wave -> eight of
// its columns as two groups of four (three dwords each: quad_pack)
template <int SRC, bool VF, int ROT>
__global__ void __launch_bounds__(256) rot_quarter_kernel(FramePtrs<kFitFrames> tab, uint8_t* dst, cf_fit_geom g, uint32_t fill, int h, int w, int pitch0,
                                                          int pitch1, int H, int W) {
    __shared__ uint32_t tile[kQTY * kQPitch];
    __shared__ int4 colc[kQTX];
    const int f = blockIdx.z, TX0 = blockIdx.x * kQTX, TY0 = blockIdx.y * kQTY;
    const int tid = threadIdx.x, ly = tid & 63, wave = tid >> 6;
    const int hu = w, wu = h;
    // (uniform) the tile lies wholly in the padding: no coefficients, no source
    const bool content = TX0 < g.dx + g.rw && TX0 + kQTX > g.dx && TY0 < g.dy + g.rh && TY0 + kQTY > g.dy;
    if (content && tid < kQTX) {
        int x0, x1, a0, a1;
        cv_linear_coeffs(min(max(TX0 + tid - g.dx, 0), g.rw - 1), wu, g.rw, true, x0, x1, a0, a1);
        colc[tid] = make_int4(x0, x1, a0, a1);
    }
    __syncthreads();
    const int y = TY0 + ly - g.dy;
    const bool row_in = content && TY0 + ly < H && y >= 0 && y < g.rh;
    int y0 = 0, y1 = 0, b0 = 0, b1 = 0;
    if (row_in) cv_linear_coeffs(y, hu, g.rh, false, y0, y1, b0, b1);
    const SrcPlanes src{tab.p0[f], tab.p1[f], tab.p2[f], pitch0, pitch1, h, w};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cg = wave * 2 + j;                      // the column group: canvas columns TX0 + 4 cg .. + 3
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = TX0 + cg * 4 + k - g.dx;        // (uniform over the wave)
            p[k] = fill;
            if (row_in && x >= 0 && x < g.rw) {
                const int4 c = colc[cg * 4 + k];
                p[k] = bilinear_px<SRC, VF, ROT>(src, y0, y1, b0, b1, c.x, c.y, c.z, c.w);
            }
        }
        uint32_t o[3];
        quad_pack(p, o);
        uint32_t* t = tile + ly * kQPitch + cg * 3;
        t[0] = o[0]; t[1] = o[1]; t[2] = o[2];
    }
    __syncthreads();
    tile_rows_out(tile, dst + (size_t)f * H * W * 3, H, W, TX0, TY0);
}

}  // namespace

const char* rot_check(std::string& why, const cf_rot_opts* o, int format, int B, int h, int w, int pitch0, int pitch1, int H, int W) {
    char b[160];
    auto say = [&](const char* s) { why = s; return why.c_str(); };
    if (!o) return say("null options");
    if (o->rot != 0 && o->rot != 90 && o->rot != 180 && o->rot != 270) { snprintf(b, sizeof b, "rot=%d must be 0, 90, 180 or 270 (clockwise degrees)", o->rot); return say(b); }
    if (o->stretch != 0 && o->stretch != 1) { snprintf(b, sizeof b, "stretch=%d must be 0 or 1", o->stretch); return say(b); }
    return fit_check(why, &o->fit, format, B, h, w, pitch0, pitch1, H, W);
}

int rot_geometry(const cf_rot_opts* o, int h, int w, int H, int W, cf_fit_geom* g) {
    if (!o || !g || h < 1 || w < 1 || H < 1 || W < 1) return CF_EINVAL;
    const bool quarter = o->rot == 90 || o->rot == 270;
    if (o->stretch) { *g = cf_fit_geom{W, H, 0, 0}; return CF_OK; }
    return fit_geometry(o->fit.anchor, o->fit.upscale, quarter ? w : h, quarter ? h : w, H, W, g);
}

// rot: 90 or 270; one launch over the nb frames of tab (launch_fit_frames has checked the arguments)
void launch_rot_quarter(hipStream_t s, int rot, int format, const FramePtrs<kFitFrames>& tab, int nb, uint8_t* dst, const cf_fit_geom& g, uint32_t fill,
                        int h, int w, int pitch0, int pitch1, int H, int W) {
    const dim3 grid((unsigned)((W + kQTX - 1) / kQTX), (unsigned)((H + kQTY - 1) / kQTY), (unsigned)nb);
    with_format(format, [&](auto SRC, auto VF) {
        if (rot == 90) hipLaunchKernelGGL((rot_quarter_kernel<SRC, VF, 1>), grid, dim3(256), 0, s, tab, dst, g, fill, h, w, pitch0, pitch1, H, W);
        else hipLaunchKernelGGL((rot_quarter_kernel<SRC, VF, 3>), grid, dim3(256), 0, s, tab, dst, g, fill, h, w, pitch0, pitch1, H, W);
    });
}

}  // namespace cf
