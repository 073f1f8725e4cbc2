// Rotated sources through packed views: the canvases of cf_forward_packed filled from the UPRIGHT view of frames that are stored a
// quarter, a half or three quarters of a turn away from it, and the merge that maps the rows back into the STORED frame.  The statement
// is in include/centerface_hip.h (cf_forward_packed_rot); in short, for a stored frame F of h x w and rot = the clockwise turn that makes
// it upright, the upright view U of hu x wu is
//   rot  90: (w, h)  U[y][x] = F[h-1-x][y]         rot 180: (h, w)  U[y][x] = F[h-1-y][w-1-x]         rot 270: (w, h)  U[y][x] = F[x][w-1-y]
// every placement's source rectangle is in pixels of U, and inside a content the canvas is
//   resize(bgr(U_f)[sy0 : sy0 + sh, sx0 : sx0 + sw], (dh, dw))
// with bgr() taken per STORED pixel (a 4:2:0 pixel's chroma is that of its own 2 x 2 block in F) and the fixed-point resize of
// cf_cvresize.h, taps clamped at the source rectangle: the kernels read F through the index map and never build U.  The turn is an
// argument of launch_cut_packed (cf_views.hip) and a field of MergeParams; this file holds the quarter-turn cutter.
//
// CUT, rot 180.  cut_packed_kernel<SRC, VF, 2> (cf_views.hip): the unturned kernel on mirrored taps -- adjacent canvas columns are still
// adjacent stored columns, so its layout carries over.
//
// CUT, rot 90 / 270.  Adjacent canvas COLUMNS are adjacent stored ROWS: with that layout every tap of a wave would be a cache line of its
// own.  Here the transposition of rot_quarter_kernel (cf_rot.hip) sits under the placement list of cut_packed_kernel: a workgroup owns a
// canvas tile of kQTY rows x kQTX columns and lists the placements that touch it in rounds of kPackList (list_round, cf_cutpx.h: placement
// order; the list cannot overflow, a canvas with more placements takes more rounds).  A wave's 64 lanes run along
// the tile's canvas ROWS, so for one canvas column their taps run along ONE stored row (two: the bilinear pair) and coalesce; a lane's
// row coefficients are computed once per placement, the tile's column coefficients once per placement and workgroup (LDS).  A lane keeps
// its eight pixels in registers across the list, `fill` where no placement wrote, and packs them into an LDS tile whose row pitch of 25
// dwords is odd; the tile leaves as whole-row dword stores.
//
// Both: one writer per byte; a tile no placement touches stores fill and reads no frame; every tap lies inside the placement's source
// rectangle mapped into F, pitch padding is never read; frames are never written; one launch covers all N canvases and all frames (the
// plane table of the blob reaches every frame).
//
// MERGE.  collect_rows_kernel<PlacedItems, ROT> (cf_collect.h, launched by cf_tiles.hip's launch_merge): the three drop rules in canvas
// coordinates, unchanged, except that "source side interior to the frame" is tested against U (hu, wu); a kept point goes to U first,
//   ux(x) = ((double)x - dx) * ((double)sw / dw) + sx0,   uy(y) = ((double)y - dy) * ((double)sh / dh) + sy0
// (float64 in this order, no contraction: the file is built with -ffp-contract=off), then to F by the table of cf_unfit_rows, the
// difference taken in float64 and rounded to float32 once; landmarks point by point, the box an ASSIGNMENT of mapped corners.  The NMS
// stages of cf_decode.hip then run on the stored-frame boxes.  The compaction is a prefix sum: the order is deterministic.
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_cutpx.h"
#include <cstdio>
#include <string>

namespace cf {
namespace {

// rot 90 (ROT 1) / 270 (ROT 3): grid (tiles of a canvas, canvases); thread = (wave, lane): lane -> the tile's canvas row, wave -> eight
// of its columns as two groups of four (three dwords each: quad_pack)
template <int SRC, bool VF, int ROT>
__global__ void __launch_bounds__(256) cut_packed_quarter_kernel(PackDev t, uint8_t* dst, uint32_t fill, int h, int w, int pitch0, int pitch1, int H, int W,
                                                                 int tiles_x) {
    __shared__ uint32_t tile[kQTY * kQPitch];
    __shared__ int4 colc[kQTX];
    __shared__ int s_list[kPackList];
    __shared__ int s_cnt[4];
    const int tid = (int)threadIdx.x, ly = tid & 63, wave = tid >> 6, n = (int)blockIdx.y;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int TX0 = tx * kQTX, TY0 = ty * kQTY;
    const int Y = TY0 + ly, XW = TX0 + 8 * wave;          // the lane's canvas row, the wave's first canvas column
    uint32_t px[2][4] = {{fill, fill, fill, fill}, {fill, fill, fill, fill}};      // the wave's eight columns as two groups of four
    const int k0 = t.cv_off[n], k1 = t.cv_off[n + 1];
    for (int base = k0; base < k1; base += kPackList) {   // uniform trip count
        const int cnt = list_round(t, base, k1, TX0, TY0, kQTX, kQTY, s_list, s_cnt);
        for (int j = 0; j < cnt; ++j) {                    // (uniform: the barriers below are reached by every thread)
            const cf_place& pl = t.places[__builtin_amdgcn_readfirstlane(s_list[j])];
            const cf_view r = pl.view;
            if (tid < kQTX) {                              // the tile's column coefficients for this placement, once per workgroup
                int x0, x1, a0, a1;
                cv_linear_coeffs(min(max(TX0 + tid - r.dx, 0), r.dw - 1), r.sw, r.dw, true, x0, x1, a0, a1);      // a foreign column: the edge's taps, not used
                colc[tid] = make_int4(x0 + r.sx0, x1 + r.sx0, a0, a1);
            }
            __syncthreads();
            const int y = Y - r.dy;
            if (y >= 0 && y < r.dh && XW < r.dx + r.dw && XW + 8 > r.dx) {      // (a row of the content is a row of the canvas: Y < H)
                int y0, y1, b0, b1;
                cv_linear_coeffs(y, r.sh, r.dh, false, y0, y1, b0, b1);
                y0 += r.sy0; y1 += r.sy0;
                const SrcPlanes src{t.planes[3 * pl.frame], t.planes[3 * pl.frame + 1], t.planes[3 * pl.frame + 2], pitch0, pitch1, h, w};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int x = XW + k - r.dx;           // (uniform over the wave)
                    if (x >= 0 && x < r.dw) {
                        const int4 c = colc[8 * wave + k];
                        px[k >> 2][k & 3] = bilinear_px<SRC, VF, ROT>(src, y0, y1, b0, b1, c.x, c.y, c.z, c.w);
                    }
                }
            }
            __syncthreads();                                  // colc is rewritten by the next placement, s_list by the next round
        }
        __syncthreads();                                      // (cnt == 0: s_cnt has been read by everyone)
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        uint32_t o[3];
        quad_pack(px[j], o);
        uint32_t* d = tile + ly * kQPitch + (wave * 2 + j) * 3;
        d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
    }
    __syncthreads();
    tile_rows_out(tile, dst + (size_t)n * H * W * 3, H, W, TX0, TY0);
}

}  // namespace

const char* pack_rot_check(std::string& why, int rot, int h, int w, const cf_place* places, int P, int N, int Bf, int H, int W) {
    char b[160];
    if (rot != 0 && rot != 90 && rot != 180 && rot != 270) {
        snprintf(b, sizeof b, "rot=%d must be 0, 90, 180 or 270 (clockwise degrees)", rot);
        why = b;
        return why.c_str();
    }
    const bool quarter = rot == 90 || rot == 270;
    if (!pack_check(why, quarter ? w : h, quarter ? h : w, places, P, N, Bf, H, W)) return nullptr;
    if (quarter) {
        snprintf(b, sizeof b, " -- rot=%d: the sources are rectangles of the UPRIGHT view, %d x %d, of the stored %d x %d frame", rot, h, w, w, h);
        why += b;
    }
    return why.c_str();
}

// rot: 90 or 270 (launch_cut_packed has checked the arguments)
void launch_cut_packed_quarter(hipStream_t s, int rot, int format, const PackDev& t, int N, uint8_t* dst, uint32_t fill, int h, int w, int pitch0, int pitch1,
                               int H, int W) {
    const int tiles_x = (W + kQTX - 1) / kQTX, tiles_y = (H + kQTY - 1) / kQTY;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)N);
    with_format(format, [&](auto SRC, auto VF) {
        if (rot == 90) hipLaunchKernelGGL((cut_packed_quarter_kernel<SRC, VF, 1>), grid, dim3(256), 0, s, t, dst, fill, h, w, pitch0, pitch1, H, W, tiles_x);
        else hipLaunchKernelGGL((cut_packed_quarter_kernel<SRC, VF, 3>), grid, dim3(256), 0, s, t, dst, fill, h, w, pitch0, pitch1, H, W, tiles_x);
    });
}

}  // namespace cf
