// Blur redaction in the source frame (cf_blur_faces, cf_op_blur): every sample that the scaled box of a kept face (RECT) or the ellipse
// inscribed in it (ELLIPSE) covers is overwritten with a Gaussian-like blur of the frame as it was before the call -- in a BGR or 4:2:0
// frame that stays on the device.
//
// The arithmetic is this project's own statement, restated in numpy in tests/test_blur.py; kernel and restatement are equal bit for
// bit.  Everything is integer arithmetic except the box mapping, which is cf_redact.hip's (cf_redactmath.h: float64 in the order
// written, no FMA contraction; this file is compiled with -ffp-contract=off).
//
// 1. Faces, boxes, coverage: steps 1 and 2 of cf_redact.hip -- the box grown by `scale`, mapped with floor / ceil, clamped, X1, Y1
//    snapped down and X2, Y2 up to even; a BGR pixel / luma sample (x, y) is the point (2x+1, 2y+1), a chroma sample (i, j) the point
//    (4i+2, 4j+2), tested against the RECT or the int64 ELLIPSE.
// 2. Filter of strength r, 1 <= r <= 24: b = 2r+1, the 1-D taps t are the integer sequence box_b * box_b * box_b (three discrete
//    convolutions of b ones): 6r+1 taps, radius R = 3r, sum b^3, variance r(r+1), so sigma is about r; r = 1: 1 3 6 7 6 3 1.  The taps
//    come from integer convolution (here: by the compiler, in a constexpr table), never from exp.  For a sample (x, y) of a plane of
//    cw x ch samples, per channel:
//      S = sum_j sum_i t[j] * t[i] * src[clamp(y+j-R, 0, ch-1)][clamp(x+i-R, 0, cw-1)]
//      value = (S + D/2) / D,  D = b^6, in 64-bit integers  (S <= 255 * 49^6 ~ 3.5e12; the row sums <= 255 * 49^3 fit int32)
//    One rounding only, so the separable evaluation below equals the 2-D one.  src is the plane as it was before the call; border
//    samples replicate; the three bytes of BGR and the two interleaved channels of NV12 / NV21 are filtered separately; chroma planes
//    use r_c = (r+1)/2 on their w/2 x h/2 grid.
// 3. Which r: opts.radius in 1..24 is the r of every face.  opts.radius == 0: per face, with A = X2-X1, Bv = Y2-Y1 of the snapped,
//    unclipped box, r_f = clamp(min(A, Bv) / 8, 1, 24); a covered sample takes the value computed with r* = max r_f over the faces of
//    its image that cover that sample (the sample's own point test; (r+1)/2 is monotonic, so the chroma radius is that of r*).  The
//    value depends only on (plane, x, y, r*) and the untouched frame: neither face order nor overlap matters.
// 4. Writes: only covered samples inside the frame, never by read-modify-write: a whole dword when all four bytes are covered, single
//    bytes otherwise.  Pitch padding, the corners of an ELLIPSE box and uncovered bytes are not touched.
//
// Two launches in stream order, for the reason the mosaic takes two: blur_compute_kernel only READS the frame and writes the value of
// every covered sample into a scratch that mirrors the planes (redact_stage_layout); blur_write_kernel only WRITES the frame, copying
// covered samples from the scratch.  So the call runs in place, and no workgroup reads a byte another one has overwritten.
//
// blur_compute_kernel: one workgroup of 256 lanes per (face, tile of the face's clipped box); the grid is B x faces_cap faces x slices,
// a workgroup walks its face's tiles with the slice stride and leaves at once (uniformly) when its face does not exist.  The tile is
// 32 x 32 samples of one plane.  Per channel the workgroup stages the tile plus its R-halo in LDS as bytes (coordinates clamped while
// loading: at most 176 x 176 = 30976 B at R = 72), runs the horizontal pass into an int32 array of (32 + 2R) rows x 32 (22528 B), then
// the vertical pass from that array and the 64-bit divide.  With the taps and the face list that is 54 KiB, so two workgroups fit the
// 160 KiB of a CU at r = 24 (64 x 32 tiles would need 82 KiB and leave one).  LDS banks: in the horizontal pass the 32 lanes of a half
// wave read consecutive bytes and write consecutive dwords; in the vertical pass they read 32 consecutive dwords of one row: no
// conflicts in either (ds_read_b32 banks over 32 dwords per 32-lane half).
// radius == 0: a lane must know whether a face of larger r covers its sample, because then that face's workgroup writes it.  The faces
// of the image whose r_f exceeds this face's and whose clipped box meets the tile are preloaded into LDS, 64 at a time, and every lane
// clears the samples they cover from its mask.  Faces of equal r that cover one sample both store the same value.
#include <limits.h>
#include <algorithm>

#include "centerface_hip.h"
#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_redactmath.h"

namespace cf {
namespace {

constexpr int kTile = 32;                              // tile side in samples (a power of two: lane -> (row, column) by shifts)
constexpr int kMaxR = 3 * kBlurMaxRadius;              // 72
constexpr int kSrcW = kTile + 2 * kMaxR;               // 176: pitch and rows of the staged bytes
constexpr int kFaceChunk = 64;                         // faces preloaded per round of the skip rule
constexpr int kBlurMaxSlices = 256;
constexpr int kTapsTotal = (kBlurMaxRadius) * (3 * kBlurMaxRadius + 4);       // sum over r of 6r+1 = 3 * 24 * 25 + 24 = 1824

// taps of r at t[(r-1) * (3r+1)], 6r+1 of them: ones convolved with b ones twice, each convolution as a running sum
struct BlurTaps { int t[kTapsTotal]; };
constexpr BlurTaps make_taps() {
    BlurTaps T{};
    for (int r = 1; r <= kBlurMaxRadius; ++r) {
        const int b = 2 * r + 1, n = 6 * r + 1;
        int a[6 * kBlurMaxRadius + 1] = {}, c[6 * kBlurMaxRadius + 1] = {};
        for (int i = 0; i < b; ++i) a[i] = 1;
        for (int pass = 0; pass < 2; ++pass) {
            int run = 0;
            for (int i = 0; i < n; ++i) {
                run += a[i];
                if (i >= b) run -= a[i - b];
                c[i] = run;
            }
            for (int i = 0; i < n; ++i) a[i] = c[i];
        }
        for (int i = 0; i < n; ++i) T.t[(r - 1) * (3 * r + 1) + i] = a[i];
    }
    return T;
}
constexpr BlurTaps kHostTaps = make_taps();
static_assert(kHostTaps.t[0] == 1 && kHostTaps.t[1] == 3 && kHostTaps.t[2] == 6 && kHostTaps.t[3] == 7 && kHostTaps.t[6] == 1, "r = 1: 1 3 6 7 6 3 1");
static_assert(kHostTaps.t[7] == 1 && kHostTaps.t[7 + 6] == 19 && kHostTaps.t[kTapsTotal - 1] == 1, "r = 2 peaks at 19; the table ends with r = 24's last 1");
__constant__ BlurTaps g_taps = make_taps();

struct BlurArgs {
    int shape, radius;
    float scale;
    FrameGeo g;                                        // g.B: the frames of this launch
    FaceList f;
    uint8_t* scratch;                                  // first frame of this launch
    unsigned long long sone, soff1, soff2;             // bytes per frame, offsets of the chroma planes
    int spitch0, spitch1;
};

__device__ __forceinline__ int face_r(const FaceBox& f, int radius) {
    return radius ? radius : min(max(min(f.X2 - f.X1, f.Y2 - f.Y1) / 8, 1), kBlurMaxRadius);
}

// First launch: reads the frame, writes a.scratch only.
__global__ void __launch_bounds__(256) blur_compute_kernel(BlurArgs a, RedactPtrs t) {
    __shared__ uint8_t s_src[kSrcW * kSrcW];
    __shared__ int s_hs[kSrcW * kTile];
    __shared__ int s_taps[2 * kMaxR + 1];
    __shared__ int s_face[kFaceChunk][4];
    __shared__ int s_face_on[kFaceChunk];
    Clip c;
    if (!face_clip(a.g, a.f, a.scale, c)) return;
    const bool ellipse = a.shape == CF_REDACT_ELLIPSE;
    const int tid = (int)threadIdx.x;
    FaceBox me; me.X1 = c.X1; me.Y1 = c.Y1; me.X2 = c.X2; me.Y2 = c.Y2; me.ok = true;
    const int r_me = face_r(me, a.radius);
    const int nfaces = a.radius ? 0 : min(a.f.counts[c.b], a.f.rows_cap);       // the skip rule only matters when r varies
    for (int ps = 0; ps < frame_planes(a.g.format); ++ps) {
        const uint8_t* base = ps == 0 ? t.p0[c.b] : ps == 1 ? t.p1[c.b] : t.p2[c.b];
        uint8_t* sbase = a.scratch + (size_t)c.b * a.sone + (ps == 0 ? 0 : ps == 1 ? a.soff1 : a.soff2);
        const PlanePass pp = plane_pass(a.g, ps, c);
        const bool chroma = pp.chroma;
        const int bps = pp.bps, pitch = pp.pitch, spitch = chroma ? a.spitch1 : a.spitch0;
        const int cw = chroma ? a.g.w >> 1 : a.g.w, ch = chroma ? a.g.h >> 1 : a.g.h;
        const int sx0 = pp.sx0, sx1 = pp.sx1, sy0 = pp.sy0, sy1 = pp.sy1;
        const int r = chroma ? (r_me + 1) >> 1 : r_me, R = 3 * r, ntaps = 2 * R + 1, bb = 2 * r + 1;
        const unsigned long long D = (unsigned long long)(bb * bb * bb) * (unsigned long long)(bb * bb * bb);
        const int ntx = (sx1 - sx0 + kTile - 1) / kTile, ntiles = ntx * ((sy1 - sy0 + kTile - 1) / kTile);
        __syncthreads();                                                       // the previous pass's taps are no longer read
        if (tid < ntaps) s_taps[tid] = g_taps.t[(r - 1) * (3 * r + 1) + tid];
        for (int tile = (int)blockIdx.y; tile < ntiles; tile += (int)gridDim.y) {
            const int ty = tile / ntx, tx0 = sx0 + (tile - ty * ntx) * kTile, ty0 = sy0 + ty * kTile;
            const int tw = min(kTile, sx1 - tx0), th = min(kTile, sy1 - ty0);
            // lane -> samples k = tid + 256 q, q < 4: row k / 32, column k % 32; mask = those this face covers
            int mask = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = tid + 256 * q, ly = k >> 5, lx = k & (kTile - 1);
                if (lx < tw && ly < th) {
                    const int x = tx0 + lx, y = ty0 + ly;
                    if (face_covers(c.X1, c.Y1, c.X2, c.Y2, ellipse, pp.point(x), pp.point(y))) mask |= 1 << q;
                }
            }
            // the skip rule: samples that a face of larger r covers belong to that face's workgroup
            const int lx0 = chroma ? 2 * tx0 : tx0, ly0 = chroma ? 2 * ty0 : ty0;             // the tile in frame pixels
            const int lx1 = chroma ? 2 * (tx0 + tw) : tx0 + tw, ly1 = chroma ? 2 * (ty0 + th) : ty0 + th;
            for (int f0 = 0; f0 < nfaces; f0 += kFaceChunk) {
                const int nf = min(kFaceChunk, nfaces - f0);
                __syncthreads();                                               // the previous round's list is no longer read
                if (tid < nf) {
                    const FaceBox f = face_box(a.f.boxes + ((size_t)c.b * a.f.box_stride + f0 + tid) * 4, a.scale, a.g.h, a.g.w, a.f.H, a.f.W);
                    const bool on = f.ok && face_r(f, 0) > r_me && max(f.X1, lx0) < min(f.X2, lx1) && max(f.Y1, ly0) < min(f.Y2, ly1);
                    s_face[tid][0] = f.X1; s_face[tid][1] = f.Y1; s_face[tid][2] = f.X2; s_face[tid][3] = f.Y2;
                    s_face_on[tid] = on ? 1 : 0;
                }
                __syncthreads();
                for (int j = 0; j < nf; ++j) {
                    if (!s_face_on[j]) continue;
                    const int X1 = s_face[j][0], Y1 = s_face[j][1], X2 = s_face[j][2], Y2 = s_face[j][3];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (!(mask & (1 << q))) continue;
                        const int k = tid + 256 * q, x = tx0 + (k & (kTile - 1)), y = ty0 + (k >> 5);
                        if (face_covers(X1, Y1, X2, Y2, ellipse, pp.point(x), pp.point(y))) mask &= ~(1 << q);
                    }
                }
            }
            if (!__syncthreads_or(mask)) continue;                             // uniform: nothing of this tile is this face's
            const int SW = tw + 2 * R, SH = th + 2 * R;                         // <= kSrcW each
            for (int cc = 0; cc < bps; ++cc) {
                __syncthreads();                                               // the previous channel's arrays are no longer read
                for (int idx = tid; idx < SW * SH; idx += 256) {
                    const int yy = idx / SW, xx = idx - yy * SW;
                    const int gx = min(max(tx0 + xx - R, 0), cw - 1), gy = min(max(ty0 + yy - R, 0), ch - 1);
                    s_src[yy * kSrcW + xx] = base[(size_t)gy * pitch + (size_t)gx * bps + cc];
                }
                __syncthreads();
                for (int idx = tid; idx < SH * kTile; idx += 256) {
                    const int row = idx >> 5, x = idx & (kTile - 1);
                    if (x < tw) {
                        const uint8_t* q = s_src + row * kSrcW + x;
                        int sum = 0;
                        for (int i = 0; i < ntaps; ++i) sum += s_taps[i] * (int)q[i];
                        s_hs[idx] = sum;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (!(mask & (1 << q))) continue;
                    const int k = tid + 256 * q, ly = k >> 5, lx = k & (kTile - 1);
                    const int* col = s_hs + ly * kTile + lx;
                    unsigned long long S = 0;
                    for (int j = 0; j < ntaps; ++j) S += (unsigned long long)(unsigned)s_taps[j] * (unsigned)col[j * kTile];
                    sbase[(size_t)(ty0 + ly) * spitch + (size_t)(tx0 + lx) * bps + cc] = (uint8_t)((S + D / 2) / D);
                }
            }
        }
    }
}

// Second launch: writes the covered samples of one face, plane after plane, from the scratch; never reads the frame.  Item = one aligned
// dword of a plane row inside the clipped box (the scratch rows hold the same bytes at the same offsets, in whole dwords).
__global__ void __launch_bounds__(256) blur_write_kernel(BlurArgs a, RedactPtrs t) {
    Clip c;
    if (!face_clip(a.g, a.f, a.scale, c)) return;
    const bool ellipse = a.shape == CF_REDACT_ELLIPSE;
    const int first = (int)blockIdx.y * 256 + (int)threadIdx.x, stride = (int)gridDim.y * 256;
    for (int ps = 0; ps < frame_planes(a.g.format); ++ps) {
        uint8_t* base = ps == 0 ? t.p0[c.b] : ps == 1 ? t.p1[c.b] : t.p2[c.b];
        const uint8_t* sbase = a.scratch + (size_t)c.b * a.sone + (ps == 0 ? 0 : ps == 1 ? a.soff1 : a.soff2);
        const PlanePass pp = plane_pass(a.g, ps, c);
        const int bps = pp.bps, spitch = pp.chroma ? a.spitch1 : a.spitch0, items = pp.nd * (pp.sy1 - pp.sy0);
        for (int item = first; item < items; item += stride) {
            const int row = pp.sy0 + item / pp.nd, d = pp.d0 + (item - (item / pp.nd) * pp.nd);
            int mask = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int byte = 4 * d + k;
                const int s = bps == 3 ? byte / 3 : bps == 2 ? byte >> 1 : byte;
                if (s < pp.sx0 || s >= pp.sx1) continue;
                if (face_covers(c.X1, c.Y1, c.X2, c.Y2, ellipse, pp.point(s), pp.point(row))) mask |= 1 << k;
            }
            if (mask) store_masked_dword(base + (size_t)row * pp.pitch + (size_t)d * 4,
                                         *reinterpret_cast<const uint32_t*>(sbase + (size_t)row * spitch + (size_t)d * 4), mask);
        }
    }
}

}  // namespace

const char* blur_check(int format, int shape, int radius, float scale, int B, int h, int w, int pitch0, int pitch1) {
    if (const char* why = redact_check(format, CF_REDACT_SOLID, shape, 2, scale, B, h, w, pitch0, pitch1)) return why;
    if (radius < 0 || radius > kBlurMaxRadius) return "radius must be in [0, 24] (0 = per face, from the box size)";
    return nullptr;
}

size_t blur_scratch_bytes(int format, int B, int h, int w) { return redact_stage_layout(format, h, w).one * (size_t)B; }

hipError_t launch_blur_faces(hipStream_t s, const BlurParams& p) {
    const FrameGeo& g = p.g;
    if (blur_check(g.format, p.shape, p.radius, p.scale, g.B, g.h, g.w, g.pitch0, g.pitch1) ||
        redact_check_planes(g.format, p.planes, g.B, 1, g.pitch0, g.pitch1) || p.f.H < 1 || p.f.W < 1 || !p.f.boxes || !p.f.counts ||
        p.f.box_stride < 1 || p.f.rows_cap < 1 || p.f.faces_cap < 1 || !p.scratch)
        return hipErrorInvalidValue;
    const RedactStage st = redact_stage_layout(g.format, g.h, g.w);
    BlurArgs a{};
    a.g = g; a.f = p.f; a.shape = p.shape; a.radius = p.radius; a.scale = p.scale;
    a.sone = st.one; a.soff1 = st.off1; a.soff2 = st.off2; a.spitch0 = st.pitch0; a.spitch1 = st.pitch1;
    for (int f0 = 0; f0 < g.B; f0 += kRedactFrames) {
        const int nb = std::min(g.B - f0, kRedactFrames);
        const RedactPtrs tab = frame_ptrs<kRedactFrames>(p.planes, g.format, f0, nb, false);
        a.g.B = nb;
        a.f.boxes = p.f.boxes + (size_t)f0 * p.f.box_stride * 4;
        a.f.counts = p.f.counts + f0;
        a.scratch = p.scratch + (size_t)f0 * st.one;
        const long long faces = (long long)nb * p.f.faces_cap;
        if (faces > INT_MAX) return hipErrorInvalidValue;
        // slices per face: one per tile of a frame-sized face, as long as the launch stays near kRedactGridTarget workgroups (most of
        // which belong to faces that do not exist and leave at once); a workgroup walks the tiles beyond its slice
        const long long room = std::max<long long>(kRedactGridTarget / faces, 1);
        const long long tiles = (long long)((g.w + kTile - 1) / kTile) * ((g.h + kTile - 1) / kTile);
        const long long cs = std::min<long long>(std::min(tiles, room), kBlurMaxSlices);
        hipLaunchKernelGGL(blur_compute_kernel, dim3((unsigned)faces, (unsigned)cs), dim3(256), 0, s, a, tab);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const long long dwords = (long long)g.h * (g.pitch0 / 4 + 1);
        const long long ws = std::min<long long>(std::min<long long>((dwords + 256 * 32 - 1) / (256 * 32), room), 64);
        hipLaunchKernelGGL(blur_write_kernel, dim3((unsigned)faces, (unsigned)std::max<long long>(ws, 1)), dim3(256), 0, s, a, tab);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace cf
