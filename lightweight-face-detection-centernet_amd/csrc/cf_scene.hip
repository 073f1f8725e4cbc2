// Scene cuts (cf_scene_check / cf_op_scene): does the frame of a stream continue the frame before it, measured in the luma of the two,
// and -- where it does not -- the reset of the stream's face tracks, decided and done on the device.  THE STATEMENT is in
// include/centerface_hip.h ("scene cuts"); tests/scene_cases.py restates it in numpy and the two agree bit for bit.  Integers throughout.
//
// THE KERNELS
// scene_sums_kernel: workgroups of 256 threads (four waves) over (chunk of rows, cell row, frame).  A workgroup reads at most kSceneRows
//   rows, all of ONE cell row j, over the whole width: the eight cell sums of a row segment are then all it can add to.  The row is cut
//   into runs of 16 pixels; lane l of every wave owns the runs l, l + 64, ..., the four waves take the rows in turn.  A run is read by
//   16-byte loads (one of a Y row, three of a BGR row) when the plane's address and pitch are multiples of 16, else by dwords (every
//   plane is 4-byte aligned, so no load starts past the row's bytes or ends past its pitch); the luma is computed in registers.  The bins
//   are counted with LDS integer adds in a histogram per wave, merged once; a lane adds a whole stretch of pixels of one bin at a time (one
//   add per thread for a flat frame, where every lane of a wave would otherwise queue on one counter).  A run that touches one or two cells -- every run of a frame
//   at least 128 wide -- keeps two sums in registers over all rows of the lane and adds them to LDS once; a run of a narrower frame adds
//   per pixel.  The workgroup leaves 72 int32 partials (64 bins, 8 cell sums) in a slot of its own: no atomics in device memory, and a
//   workgroup without rows leaves zeros.
// scene_decide_kernel: one wave per stream.  Lane k sums the partials of bin k and of cell k, divides the cell sum, takes the two absolute
//   differences against the stream's last signature; two xor butterflies leave A and grid in every lane, so every lane knows the code.
//   Lane 0 writes out and the state's words; on CUT with a tracker the wave zeroes the stream's max_tracks * 4 meta words; every lane
//   stores its two words of the new signature.  Integer sums in a fixed order: the result does not depend on the launch geometry.
#include <algorithm>

#include "cf_common.h"
#include "cf_kernels.h"

namespace cf {

namespace {

constexpr int kSceneFrames = 16;                   // frames (= streams) of one launch: their plane-0 addresses go by value
constexpr int kSceneRun = 16;                      // pixels of one run
struct ScenePlanes { const uint8_t* p0[kSceneFrames]; };

__device__ inline int scene_luma_bgr(int b, int g, int r) { return (29 * b + 150 * g + 77 * r + 128) >> 8; }
__host__ __device__ inline int scene_chunks(int h) { return ((h + 7) / 8 + kSceneRows - 1) / kSceneRows; }      // of the tallest cell row

__global__ __launch_bounds__(256) void scene_sums_kernel(SceneParams p, ScenePlanes fr) {
    __shared__ int s_hist[4][64];
    __shared__ int s_cell[8];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int chunk = blockIdx.x, j = blockIdx.y, b = blockIdx.z;
    const int h = p.g.h, w = p.g.w, pitch = p.g.pitch0;
    const bool bgr = p.g.format == CF_FRAME_BGR;
    s_hist[wv][lane] = 0;
    if (t < 8) s_cell[t] = 0;
    __syncthreads();
    const int ya = (j * h) / 8 + chunk * kSceneRows, yb = min(((j + 1) * h) / 8, ya + kSceneRows);
    const uint8_t* p0 = fr.p0[b];
    const bool wide = ((reinterpret_cast<uintptr_t>(p0) | (uintptr_t)pitch) & 15) == 0;
    const int rowbytes = bgr ? 3 * w : w, nd = bgr ? 12 : 4;      // dwords of a run
    int* hist = s_hist[wv];
    int cb = 0, cn = 0;                                                       // cn pixels in a row fell into bin cb: one add when the bin changes
    for (int run = lane; run * kSceneRun < w; run += 64) {
        const int x0 = run * kSceneRun, n = min(kSceneRun, w - x0);
        // the cell of the run's first pixel and the pixels of the run that lie in it: the largest ci with (ci * w) / 8 <= x0
        int ci = (int)(((long long)x0 * 8 + 7) / w);
        if (ci > 7) ci = 7;
        while (ci > 0 && (ci * w) / 8 > x0) --ci;
        while (ci < 7 && ((ci + 1) * w) / 8 <= x0) ++ci;
        const int k1 = min(((ci + 1) * w) / 8 - x0, n);                       // pixels i < k1: cell ci
        const bool two = ci == 7 || ((ci + 2) * w) / 8 - x0 >= n;            // the others: all in cell ci + 1
        int lo = 0, hi = 0;
        for (int y = ya + wv; y < yb; y += 4) {
            const uint8_t* row = p0 + (size_t)y * pitch;
            const int o = bgr ? 3 * x0 : x0;                                   // a multiple of 16
            uint32_t d[12];
#pragma unroll
            for (int q = 0; q < 12; ++q) d[q] = 0;
            if (wide) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if (q * 4 < nd && o + 16 * q < rowbytes) {
                        const uint4 v = *reinterpret_cast<const uint4*>(row + o + 16 * q);
                        d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
                    }
            } else {
#pragma unroll
                for (int q = 0; q < 12; ++q)
                    if (q < nd && o + 4 * q < rowbytes) d[q] = *reinterpret_cast<const uint32_t*>(row + o + 4 * q);
            }
            int cc = ci, next = k1;
#pragma unroll
            for (int i = 0; i < kSceneRun; ++i) {
                int l;
                if (bgr) {
                    const int k = 3 * i;
                    const int c0 = (int)((d[k >> 2] >> (8 * (k & 3))) & 255u), c1 = (int)((d[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 255u);
                    const int c2 = (int)((d[(k + 2) >> 2] >> (8 * ((k + 2) & 3))) & 255u);
                    l = scene_luma_bgr(c0, c1, c2);
                } else {
                    l = (int)((d[i >> 2] >> (8 * (i & 3))) & 255u);
                }
                if (i < n) {
                    const int k = l >> 2;
                    if (k == cb) ++cn;
                    else { if (cn) atomicAdd(&hist[cb], cn); cb = k; cn = 1; }
                    if (two) {
                        if (i < k1) lo += l; else hi += l;
                    } else {
                        while (i >= next) { ++cc; next = ((cc + 1) * w) / 8 - x0; }
                        atomicAdd(&s_cell[cc], l);
                    }
                }
            }
        }
        if (two) {
            if (lo) atomicAdd(&s_cell[ci], lo);
            if (hi) atomicAdd(&s_cell[ci + 1], hi);                          // hi != 0 only with pixels at i >= k1, and then ci < 7
        }
    }
    if (cn) atomicAdd(&hist[cb], cn);
    __syncthreads();
    int* out = p.part + (((size_t)b * 8 + j) * gridDim.x + chunk) * kScenePart;
    if (t < 64) out[t] = s_hist[0][t] + s_hist[1][t] + s_hist[2][t] + s_hist[3][t];
    else if (t < 72) out[t] = s_cell[t - 64];
}

__device__ inline int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(64) void scene_decide_kernel(SceneParams p, int chunks) {
    const int b = blockIdx.x, k = threadIdx.x, s = p.stream0 + b;
    const int h = p.g.h, w = p.g.w;
    int* sig = p.sig + (size_t)s * kSceneSig;
    int* st = p.st + (size_t)s * 4;                                           // h, w, valid, run
    // everything the check reads of the state, before any lane writes it
    const int ph = st[0], pw = st[1], valid = st[2], prun = st[3];
    const int pbin = sig[k], pmean = sig[64 + k];
    const int* part = p.part + (size_t)b * 8 * chunks * kScenePart;
    int bin = 0, sum = 0;
    for (int q = 0; q < 8 * chunks; ++q) bin += part[(size_t)q * kScenePart + k];
    const int i = k & 7, j = k >> 3;
    for (int q = 0; q < chunks; ++q) sum += part[((size_t)j * chunks + q) * kScenePart + 64 + i];
    const int n = (((i + 1) * w) / 8 - (i * w) / 8) * (((j + 1) * h) / 8 - (j * h) / 8);      // >= 1: h, w >= 8
    const int mean = (sum + n / 2) / n;
    const bool first = !valid || ph != h || pw != w;
    const int da = bin > pbin ? bin - pbin : pbin - bin, dg = mean > pmean ? mean - pmean : pmean - mean;
    const long long A = wave_sum(da);                                         // <= 2 * h * w <= 2^27
    const int grid = first ? 0 : wave_sum(dg);
    const int hist = first ? 0 : (int)((A * 1000) / (2ll * h * w));
    const bool cut = !first && hist >= p.hist_thresh && grid >= p.grid_thresh;
    const int run = first || cut ? 0 : (prun < (1 << 30) ? prun + 1 : (1 << 30));
    __syncthreads();
    if (k == 0) {
        int* o = p.out + (size_t)b * 4;
        o[0] = first ? CF_SCENE_FIRST : cut ? CF_SCENE_CUT : CF_SCENE_SAME; o[1] = hist; o[2] = grid; o[3] = run;
        st[0] = h; st[1] = w; st[2] = 1; st[3] = run;
    }
    sig[k] = bin; sig[64 + k] = mean;
    if (p.sig_out) { p.sig_out[(size_t)b * kSceneSig + k] = bin; p.sig_out[(size_t)b * kSceneSig + 64 + k] = mean; }
    if (cut && p.meta) {                                                      // cf_track_reset of stream s: the slots' meta words
        int* meta = p.meta + (size_t)s * p.max_tracks * 4;
        for (int q = k; q < p.max_tracks * 4; q += 64) meta[q] = 0;
    }
}

}  // namespace

const char* scene_check(const cf_scene_opts* o, int format, int B, int h, int w, int pitch0, int pitch1) {
    if (!o) return "null options";
    const FrameGeo g{format, B, h, w, pitch0, pitch1};
    if (format < CF_YUV_NV12 || format > CF_FRAME_BGR) return frame_geometry_check(g, 2, true);      // the format is refused first, then the options
    if (o->hist_thresh < 0 || o->hist_thresh > 1000) return "hist_thresh must be in 0..1000";
    if (o->grid_thresh < 0 || o->grid_thresh > 16320) return "grid_thresh must be in 0..16320";
    if (B < 1) return "B must be at least 1";
    if (((h | w) & 1) || h < 8 || w < 8 || h > kRedactMaxSide || w > kRedactMaxSide) return "h and w must be even and in [8, 8192]";
    return frame_geometry_check(g, 2, true);
}

size_t scene_part_bytes(int B, int h) { return (size_t)std::min(B, kSceneFrames) * 8 * scene_chunks(h) * kScenePart * sizeof(int); }

hipError_t launch_scene_check(hipStream_t s, const SceneParams& p) {
    const FrameGeo& g = p.g;
    cf_scene_opts o{p.hist_thresh, p.grid_thresh};
    if (scene_check(&o, g.format, g.B, g.h, g.w, g.pitch0, g.pitch1) || redact_check_planes(g.format, p.planes, g.B, 1, g.pitch0, g.pitch1) ||
        p.stream0 < 0 || !p.sig || !p.st || !p.part || !p.out || (p.meta && (p.max_tracks < 1 || p.max_tracks > kTrackMaxSlots)))
        return hipErrorInvalidValue;
    const int chunks = scene_chunks(g.h);
    for (int f0 = 0; f0 < g.B; f0 += kSceneFrames) {
        const int nb = std::min(g.B - f0, kSceneFrames);
        ScenePlanes fr{};
        for (int k = 0; k < nb; ++k) fr.p0[k] = (const uint8_t*)p.planes[3 * (f0 + k)];
        SceneParams q = p;
        q.g.B = nb; q.stream0 = p.stream0 + f0; q.out = p.out + (size_t)f0 * 4;
        if (p.sig_out) q.sig_out = p.sig_out + (size_t)f0 * kSceneSig;
        hipLaunchKernelGGL(scene_sums_kernel, dim3(chunks, 8, nb), dim3(256), 0, s, q, fr);
        if (const hipError_t e = hipGetLastError()) return e;
        hipLaunchKernelGGL(scene_decide_kernel, dim3(nb), dim3(64), 0, s, q, chunks);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace cf
