// Face redaction in the source frame: every sample that the scaled box of a kept face (RECT) or the ellipse inscribed in it (ELLIPSE)
// covers is overwritten -- with a fill colour (SOLID) or with the mean of its mosaic cell (MOSAIC) -- in a BGR or 4:2:0 frame that
// stays on the device (cf_redact_faces, cf_op_redact).
//
// The arithmetic is this project's own statement, restated in numpy in tests/test_redact.py; kernel and restatement are equal bit for
// bit.  Everything is integer arithmetic except the box mapping, which is float64 in the order written with no FMA contraction (this
// file is compiled with -ffp-contract=off).
//
// Per face: box (x1, y1, x2, y2) float32 in network coordinates (the threshold decode's values before cf_set_rescale), frame h x w,
// context H x W; options mode (SOLID | MOSAIC), shape (RECT | ELLIPSE), cell m (even, 2..256), scale s (0.25..4), fill[3].
// 1. Box to frame:
//      cx = ((double)x1 + (double)x2) * 0.5,  hw = ((double)x2 - (double)x1) * 0.5 * (double)s,  fx = (double)w / (double)W
//      X1 = floor((cx - hw) * fx),  X2 = ceil((cx + hw) * fx);  the same for y with h / H
//    skipped (nothing written) when one of the four inputs is not finite or hw / hh is not > 0.  Each result is clamped to
//    [-8192, 16384] as a double, converted to int, then X1, Y1 are rounded down to even and X2, Y2 up to even -- in every format, so a
//    mask means the same pixels in BGR and in 4:2:0.  Frames are at most 8192 a side: |du| <= 49152, axes <= 24576, and the sum of
//    the two squares below stays under 2^62.
// 2. Coverage, in half-pixel units: a BGR pixel / luma sample (x, y) is the point (U, V) = (2x+1, 2y+1), a chroma sample (i, j) the
//    point (4i+2, 4j+2).
//      RECT:    2*X1 <= U < 2*X2 and 2*Y1 <= V < 2*Y2
//      ELLIPSE: A = X2-X1, Bv = Y2-Y1, du = U-(X1+X2), dv = V-(Y1+Y2):  (du*Bv)^2 + (dv*A)^2 <= (A*Bv)^2   (int64)
//    Only samples inside the frame are written; a sample is redacted when any face of its image covers it.
// 3. Value: SOLID fill[channel].  MOSAIC: the grid is anchored at the frame origin, not at the box: cell (gx, gy) of a BGR / luma plane
//    is [gx*m, min((gx+1)*m, w)) x [gy*m, min((gy+1)*m, h)), of a chroma plane the same index with m/2, w/2, h/2 (the two interleaved
//    channels of NV12 / NV21 averaged separately); value = (sum + n/2) / n over all n samples of the cell in the frame as it was
//    before the call, per channel.  A covered sample takes its cell's value.
// Grid and means belong to the frame, not to a face, so the result depends neither on face order nor on overlap.  On the device that
// takes two launches in stream order: redact_means_kernel only READS the frame and writes the means of every cell that some face's
// clipped box touches into a scratch of one dword per cell ([B][ceil(h/m)][ceil(w/m)]: B | G << 8 | R << 16, or Y | c0 << 8 | c1 << 16
// in plane order; two faces that touch one cell write the same dword); redact_write_kernel only WRITES covered samples.  SOLID
// takes the second launch alone.
//
// Stores: a thread owns one aligned dword of a plane row.  When all four bytes are covered it stores the dword, otherwise it stores the
// covered bytes one by one -- never a read-modify-write, so bytes outside the masks (pitch padding, the corners of an ELLIPSE box, a
// neighbouring face's workgroup's bytes) are not touched.  Both launches are sized from capacities (B x faces_cap faces x a few
// slices) and read the per-image counts on the device; a workgroup whose face does not exist leaves at once.
#include <limits.h>
#include <math.h>
#include <algorithm>

#include "centerface_hip.h"
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_redactmath.h"

namespace cf {
namespace {

constexpr int kRedactMaxSlices = 64;

struct RedactArgs {
    FrameGeo g;           // g.B: the frames of this launch
    FaceList f;
    int mode, shape, m;
    float scale;
    uint32_t fill;        // SOLID: the three bytes in PLANE order (BGR; Y, first chroma channel in memory order, second)
    uint32_t* cells; int gw, gh;
    int group;            // lanes that share one cell in the means launch: 4, 16 or 64
};

// MOSAIC, first launch: the means of the cells a face's clipped box touches.  A group of a.group lanes shares one cell (its lanes stride
// over the cell's samples, a shuffle reduction adds them up, the group's first lane stores the dword); the cells of a face are spread
// over the groups of its gridDim.y slices.  Reads the frame, writes a.cells only.
__global__ void __launch_bounds__(256) redact_means_kernel(RedactArgs a, RedactPtrs t) {
    Clip c;
    if (!face_clip(a.g, a.f, a.scale, c)) return;
    const int m = a.m, G = a.group, w = a.g.w, h = a.g.h, pitch0 = a.g.pitch0, pitch1 = a.g.pitch1;
    const int gx0 = c.cx1 / m, gy0 = c.cy1 / m, ncx = (c.cx2 - 1) / m - gx0 + 1, ncells = ncx * ((c.cy2 - 1) / m - gy0 + 1);
    const int tid = (int)threadIdx.x, sub = tid & (G - 1);
    const int grp = ((int)blockIdx.y * 256 + tid) / G, ngrp = (int)gridDim.y * 256 / G;
    const bool bgr = a.g.format == CF_FRAME_BGR, il = frame_is_il(a.g.format);
    const uint8_t* p0 = t.p0[c.b];
    const uint8_t* p1 = t.p1[c.b];
    const uint8_t* p2 = t.p2[c.b];
    for (int base = 0; base < ncells; base += ngrp) {           // uniform trip count: every lane reaches the shuffles
        const int cell = base + grp;
        const bool valid = cell < ncells;
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        int n0 = 1, n1 = 1, gx = 0, gy = 0;
        if (valid) {
            gy = gy0 + cell / ncx; gx = gx0 + (cell - (cell / ncx) * ncx);
            const int xa = gx * m, ya = gy * m, cw = min(xa + m, w) - xa, ch = min(ya + m, h) - ya;
            n0 = cw * ch;
            if (bgr) {
                for (int k = sub; k < n0; k += G) {
                    const int y = k / cw, x = k - y * cw;
                    const uint8_t* q = p0 + (size_t)(ya + y) * pitch0 + (size_t)(xa + x) * 3;
                    s0 += q[0]; s1 += q[1]; s2 += q[2];
                }
                n1 = n0;
            } else {
                for (int k = sub; k < n0; k += G) {
                    const int y = k / cw, x = k - y * cw;
                    s0 += p0[(size_t)(ya + y) * pitch0 + (xa + x)];
                }
                const int mc = m >> 1, xc = gx * mc, yc = gy * mc, cwc = min(xc + mc, w >> 1) - xc, chc = min(yc + mc, h >> 1) - yc;
                n1 = cwc * chc;
                for (int k = sub; k < n1; k += G) {
                    const int j = k / cwc, i = k - j * cwc;
                    if (il) {
                        const uint8_t* q = p1 + (size_t)(yc + j) * pitch1 + (size_t)(xc + i) * 2;
                        s1 += q[0]; s2 += q[1];
                    } else {
                        const size_t o = (size_t)(yc + j) * pitch1 + (xc + i);
                        s1 += p1[o]; s2 += p2[o];
                    }
                }
            }
        }
        for (int o = G >> 1; o > 0; o >>= 1) {
            s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o);
        }
        if (valid && sub == 0) {
            const uint32_t un0 = (uint32_t)n0, un1 = (uint32_t)n1;
            a.cells[((size_t)c.b * a.gh + gy) * a.gw + gx] = ((s0 + un0 / 2) / un0) | (((s1 + un1 / 2) / un1) << 8) | (((s2 + un1 / 2) / un1) << 16);
        }
    }
}

// Second launch (the only one of SOLID): writes the covered samples of one face, plane after plane (PlanePass; the plane-order channel
// of a pass's first byte is its number).  Item = one aligned dword of a plane row inside the clipped box.  Reads a.cells, never the frame.
__global__ void __launch_bounds__(256) redact_write_kernel(RedactArgs a, RedactPtrs t) {
    Clip c;
    if (!face_clip(a.g, a.f, a.scale, c)) return;
    // the point test is written out, not face_covers: RECT is the clipped sample range itself, and face_covers' four bounds cost 6 SGPRs
    const long long A = c.X2 - c.X1, Bv = c.Y2 - c.Y1, R2 = (A * Bv) * (A * Bv);
    const int sumx = c.X1 + c.X2, sumy = c.Y1 + c.Y2;
    const bool ellipse = a.shape == CF_REDACT_ELLIPSE, mosaic = a.mode == CF_REDACT_MOSAIC;
    const int first = (int)blockIdx.y * 256 + (int)threadIdx.x, stride = (int)gridDim.y * 256;
    for (int ps = 0; ps < frame_planes(a.g.format); ++ps) {
        uint8_t* base = ps == 0 ? t.p0[c.b] : ps == 1 ? t.p1[c.b] : t.p2[c.b];
        const PlanePass pp = plane_pass(a.g, ps, c);
        const int bps = pp.bps, cs = pp.chroma ? a.m >> 1 : a.m, items = pp.nd * (pp.sy1 - pp.sy0);
        for (int item = first; item < items; item += stride) {
            const int r = pp.sy0 + item / pp.nd, d = pp.d0 + (item - (item / pp.nd) * pp.nd);
            const long long dv = pp.point(r) - sumy, tv = dv * A, tv2 = tv * tv;
            const uint32_t* cellrow = mosaic ? a.cells + ((size_t)c.b * a.gh + r / cs) * a.gw : nullptr;
            uint32_t val = 0;
            int mask = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int byte = 4 * d + k;
                const int s = bps == 3 ? byte / 3 : bps == 2 ? byte >> 1 : byte, ch = ps + (byte - s * bps);
                if (s < pp.sx0 || s >= pp.sx1) continue;
                if (ellipse) {
                    const long long tu = (long long)(pp.point(s) - sumx) * Bv;
                    if (tu * tu + tv2 > R2) continue;
                }
                const uint32_t src = mosaic ? cellrow[s / cs] : a.fill;
                val |= ((src >> (8 * ch)) & 255u) << (8 * k);
                mask |= 1 << k;
            }
            store_masked_dword(base + (size_t)r * pp.pitch + (size_t)d * 4, val, mask);
        }
    }
}

}  // namespace

const char* redact_check(int format, int mode, int shape, int cell, float scale, int B, int h, int w, int pitch0, int pitch1) {
    const char* geo = frame_geometry_check(FrameGeo{format, B, h, w, pitch0, pitch1}, 1, false);
    if (format < CF_YUV_NV12 || format > CF_FRAME_BGR) return geo;             // the format is refused first, then the options
    if (mode != CF_REDACT_SOLID && mode != CF_REDACT_MOSAIC) return "unknown mode (0 = CF_REDACT_SOLID, 1 = CF_REDACT_MOSAIC)";
    if (shape != CF_REDACT_RECT && shape != CF_REDACT_ELLIPSE) return "unknown shape (0 = CF_REDACT_RECT, 1 = CF_REDACT_ELLIPSE)";
    if (mode == CF_REDACT_MOSAIC && (cell < 2 || cell > 256 || (cell & 1))) return "cell must be even and in [2, 256]";
    if (!(scale >= 0.25f && scale <= 4.0f)) return "scale must be in [0.25, 4]";
    return geo;
}

const char* redact_check_planes(int format, const void* const* planes, int B, int on_device, int pitch0, int pitch1) {
    if (!planes) return "null frame table";
    const int need = frame_planes(format);
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < need; ++k) {
            if (!planes[3 * b + k]) return "a frame has a null plane";
            if (on_device && (reinterpret_cast<uintptr_t>(planes[3 * b + k]) & 3)) return "device planes must be 4-byte aligned";
        }
    if (on_device && ((pitch0 & 3) || (need > 1 && (pitch1 & 3)))) return "device pitches must be multiples of 4";
    return nullptr;
}

size_t redact_cells(int B, int h, int w, int cell) {
    return (size_t)B * ((h + cell - 1) / cell) * ((w + cell - 1) / cell);
}

hipError_t launch_redact_faces(hipStream_t s, const RedactParams& p) {
    const FrameGeo& g = p.g;
    if (redact_check(g.format, p.mode, p.shape, p.cell, p.scale, g.B, g.h, g.w, g.pitch0, g.pitch1) ||
        redact_check_planes(g.format, p.planes, g.B, 1, g.pitch0, g.pitch1) || p.f.H < 1 || p.f.W < 1 || !p.f.boxes || !p.f.counts ||
        p.f.box_stride < 1 || p.f.rows_cap < 1 || p.f.faces_cap < 1 || (p.mode == CF_REDACT_MOSAIC && !p.cells))
        return hipErrorInvalidValue;
    const bool swap = frame_swaps_chroma(g.format);
    RedactArgs a{};
    a.g = g; a.f = p.f; a.mode = p.mode; a.shape = p.shape; a.m = p.mode == CF_REDACT_MOSAIC ? p.cell : 2; a.scale = p.scale;
    a.fill = (uint32_t)p.fill[0] | ((uint32_t)p.fill[swap ? 2 : 1] << 8) | ((uint32_t)p.fill[swap ? 1 : 2] << 16);
    a.gw = (g.w + a.m - 1) / a.m; a.gh = (g.h + a.m - 1) / a.m;
    a.group = a.m <= 4 ? 4 : a.m <= 16 ? 16 : 64;
    for (int f0 = 0; f0 < g.B; f0 += kRedactFrames) {
        const int nb = std::min(g.B - f0, kRedactFrames);
        const RedactPtrs tab = frame_ptrs<kRedactFrames>(p.planes, g.format, f0, nb, false);
        a.g.B = nb;
        a.f.boxes = p.f.boxes + (size_t)f0 * p.f.box_stride * 4;
        a.f.counts = p.f.counts + f0;
        a.cells = p.cells ? p.cells + (size_t)f0 * a.gh * a.gw : nullptr;
        const long long faces = (long long)nb * p.f.faces_cap;
        if (faces > INT_MAX) return hipErrorInvalidValue;
        // slices per face: enough that one thread of a frame-sized face handles at most ~32 dwords, as long as the launch stays
        // near kRedactGridTarget workgroups (most of which belong to faces that do not exist and leave at once)
        const long long dwords = (long long)g.h * (g.pitch0 / 4 + 1);
        long long slices = (dwords + 256 * 32 - 1) / (256 * 32);
        slices = std::min<long long>(slices, std::max<long long>(kRedactGridTarget / faces, 1));
        slices = std::min<long long>(std::max<long long>(slices, 1), kRedactMaxSlices);
        const dim3 grid((unsigned)faces, (unsigned)slices);
        if (p.mode == CF_REDACT_MOSAIC) {
            hipLaunchKernelGGL(redact_means_kernel, grid, dim3(256), 0, s, a, tab);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(redact_write_kernel, grid, dim3(256), 0, s, a, tab);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace cf
