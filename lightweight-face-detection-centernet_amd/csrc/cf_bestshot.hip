// Best-shot selection (cf_bestshot_offer / cf_bestshot_collect, cf_op_chip_quality, cf_op_bestshot): the consumer of the tracker's ids and of
// the aligned chips.  A table on the device keeps, per track id, the chip with the highest quality; an id that disappears from the tracked
// rows finishes its entry, and a collect hands the finished entries out in finishing order.  The statement -- the quality of one chip, one
// offer, one collect -- is in include/centerface_hip.h and restated in numpy in tests/bestshot_cases.py; the two agree bit for bit.
// Integers throughout, except the three weights: float64 in the order written (this file is compiled with -ffp-contract=off).
//
// THE KERNELS.  An offer is three launches with no host read between them:
//   score   one workgroup of 256 per chip n < cap_faces.  It finds its row by walking the offsets (as the align kernels find their face) and
//           leaves at once, before any barrier, writing -1, when the row does not count or is not eligible.  Luma of the central half plus its
//           one-pixel apron is staged in LDS, four pixels (three aligned dwords of the chip row) per item, in bands of at most 64 + 2 rows of
//           at most 66 dwords (17 424 bytes).  Per-thread int32 partial sums of the Laplacian and its square (at most 256 pixels per thread:
//           256 * 1020^2 < 2^31), widened to int64, reduced with __shfl_xor and across the four waves through LDS; thread 0 does the float64
//           weights and writes Q, the parts and the image that owns the chip to a scratch.
//   decide  one workgroup of 256 per stream: which rows count (ids compared in LDS), presence of every LIVE entry (entries x rows compares),
//           the finishing with consecutive seqs by a prefix sum over the entries (ballot per wave, wave totals in LDS, a running base), the
//           match by id, and the k-th new eligible row takes the k-th FREE entry -- both ranks are prefix sums, which is "the lowest free
//           entry in row order" without a serial loop.  It writes the entry records and a job list (chip n -> entry e).  No atomics.
//   copy    one workgroup per (job slot, chunk of 16 KB): 16-byte loads and stores; a slot without a job leaves at once.
// A collect is one workgroup per stream -- flush, rank of every DONE entry by done_seq, the output rows, the jobs -- and the same copy kernel.
// Every store is a plain vector store from C++.
#include <climits>
#include <cmath>

#include "centerface_hip.h"
#include "cf_common.h"
#include "cf_kernels.h"

namespace cf {

namespace {

constexpr int ST_FREE = 0, ST_LIVE = 1, ST_DONE = 2;
// entry record, kBestRecInts int32: state, id, best_t, first_t, last_t, n_offered, done_seq, sharp, size_w, pose_w, score_w, -, Q (int64), -, -
constexpr int R_STATE = 0, R_ID = 1, R_BEST = 2, R_FIRST = 3, R_LAST = 4, R_NOFF = 5, R_SEQ = 6, R_PARTS = 7, R_Q = 12;
constexpr int M_T = 0, M_SEQ = 1, M_STICKY = 2;                 // stream record, kBestStreamInts int32
constexpr int kCopyUnits = 1024;                                // 16-byte units per workgroup of the copy kernel

// rank of this thread among the threads of the workgroup whose pred is set, in thread order, plus base; base grows by their number.
// Every thread of the 256 calls it.
__device__ __forceinline__ int block_rank(bool pred, int& base, int* s_w) {
    const unsigned long long bal = __ballot(pred);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();                                            // the totals of the round before have been read
    if (lane == 0) s_w[w] = __popcll(bal);
    __syncthreads();
    int r = base + __popcll(bal & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; ++k) r += s_w[k];
    base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return r;
}

__device__ __forceinline__ int luma(uint32_t b, uint32_t g, uint32_t r) { return (int)((29u * b + 150u * g + 77u * r + 128u) >> 8); }

// size_w, pose_w, score_w of one row (steps 3..5 of the statement)
__device__ void best_weights(int S, int terms, const float* box, float score, const float* lm, double fx, double fy, int* w3) {
    int size_w = 256, pose_w = 256, score_w = 256;
    if (terms & CF_BEST_SIZE) {
        const double wx = ((double)box[2] - (double)box[0]) * fx, wy = ((double)box[3] - (double)box[1]) * fy;
        if (!(wx > 0) || !(wy > 0)) size_w = 0;
        else {
            const double side = wx < wy ? wx : wy;
            const int side_i = side >= (double)S ? S : (int)floor(side);
            size_w = side_i * 256 / S;
        }
    }
    if (terms & CF_BEST_POSE) {
        bool fin = true;
        for (int j = 0; j < 10; ++j) fin = fin && isfinite(lm[j]);
        if (!fin) pose_w = 0;
        else {
            double P[10];
            for (int j = 0; j < 5; ++j) { P[2 * j] = (double)lm[2 * j] * fx; P[2 * j + 1] = (double)lm[2 * j + 1] * fy; }
            const double ex = (P[0] + P[2]) * 0.5, ey = (P[1] + P[3]) * 0.5;
            const double mx = (P[6] + P[8]) * 0.5, my = (P[7] + P[9]) * 0.5;
            const double ax = mx - ex, ay = my - ey;
            const double dx = P[4] - ex, dy = P[5] - ey;
            const double cr = ax * dy - ay * dx, len2 = ax * ax + ay * ay;
            if (!(len2 > 0)) pose_w = 0;
            else {
                const double t = fabs(cr) / len2 * 512.0;
                pose_w = !(t < 256.0) ? 0 : 256 - (int)floor(t);
            }
        }
    }
    if (terms & CF_BEST_SCORE) {
        const double t = (double)score * 256.0;
        score_w = !(t > 0) ? 0 : (t >= 256.0 ? 256 : (int)floor(t));
    }
    w3[0] = size_w; w3[1] = pose_w; w3[2] = score_w;
}

__global__ __launch_bounds__(256) void best_score_kernel(BestOffer p) {
    __shared__ uint32_t s_l[66 * 66];             // luma bytes of one band: (rows + 2) x ng dwords
    __shared__ long long s_red[8];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, S = p.t.size, rows = p.r.rows;
    // the image whose offsets name this chip (the lowest, should malformed offsets name it twice) and the row
    int b = -1, i = 0;
    for (int k = 0; k < p.B; ++k) {
        const int o0 = p.offsets[k], o1 = p.offsets[k + 1];
        if (b < 0 && o0 >= 0 && o0 <= o1 && n >= o0 && n < o1) { b = k; i = n - o0; }
    }
    bool on = b >= 0 && i < rows;
    if (tid == 0) p.sc[(size_t)n * kBestScratchInts + 4] = on ? b * rows + i : -1;
    int id = 0;
    const int32_t* info = p.r.info + (size_t)(on ? b : 0) * rows * 3;
    if (on) {
        const int cnt = p.r.counts[b];
        on = i < (cnt < rows ? cnt : rows);
    }
    if (on) {
        id = info[i * 3];
        on = id >= 1 && info[i * 3 + 2] == 0 && info[i * 3 + 1] >= p.t.min_hits;
    }
    if (on) {                                     // an earlier row of the image with the same id: this one does not count (every wave looks)
        bool dup = false;
        for (int j = lane; j < i; j += 64) dup = dup || info[j * 3] == id;
        on = !__any(dup);
    }
    if (!on) {                                    // uniform: before any barrier
        if (tid == 0) {
            p.q[n] = -1;
            for (int k = 0; k < 4; ++k) p.sc[(size_t)n * kBestScratchInts + k] = 0;
        }
        return;
    }
    const int a = S >> 2, e = 3 * a, Wd = S >> 1;                 // window [a, e) of S / 2 pixels (S is a multiple of 4)
    const int g0 = (a - 1) >> 2, ng = (e >> 2) - g0 + 1, x0 = g0 << 2;      // groups of 4 pixels that hold the columns a - 1 .. e
    const uint32_t* chip = reinterpret_cast<const uint32_t*>(p.chips + (size_t)n * 3 * S * S);
    const int row_dw = 3 * a;                                      // dwords per chip row: 3 * S / 4
    const uint8_t* lb = reinterpret_cast<const uint8_t*>(s_l);
    int s1 = 0, s2 = 0;
    for (int y0 = 0; y0 < Wd; y0 += 64) {
        const int R = Wd - y0 < 64 ? Wd - y0 : 64;
        if (y0) __syncthreads();                                   // the band before has been read
        for (int it = tid; it < (R + 2) * ng; it += 256) {
            const int r = it / ng, g = it - r * ng;
            const uint32_t* src = chip + (size_t)(a + y0 - 1 + r) * row_dw + (size_t)(g0 + g) * 3;      // rows a - 1 .. e, groups <= e / 4 < S / 4
            const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
            const int l0 = luma(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u);
            const int l1 = luma(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u);
            const int l2 = luma((w1 >> 16) & 255u, w1 >> 24, w2 & 255u);
            const int l3 = luma((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24);
            s_l[it] = (uint32_t)l0 | (uint32_t)l1 << 8 | (uint32_t)l2 << 16 | (uint32_t)l3 << 24;
        }
        __syncthreads();
        const int pitch = ng * 4;
        for (int it = tid; it < R * Wd; it += 256) {
            const int yl = it / Wd, x = it - yl * Wd;
            const uint8_t* c = lb + (yl + 1) * pitch + (a + x - x0);
            const int lap = 4 * (int)c[0] - (int)c[-pitch] - (int)c[pitch] - (int)c[-1] - (int)c[1];
            s1 += lap; s2 += lap * lap;
        }
    }
    long long t1 = s1, t2 = s2;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { t1 += __shfl_xor(t1, off); t2 += __shfl_xor(t2, off); }
    if (lane == 0) { s_red[tid >> 6] = t1; s_red[4 + (tid >> 6)] = t2; }
    __syncthreads();
    if (tid != 0) return;
    const long long S1 = s_red[0] + s_red[1] + s_red[2] + s_red[3], S2 = s_red[4] + s_red[5] + s_red[6] + s_red[7];
    const long long N = (long long)Wd * Wd, V = N * S2 - S1 * S1;
    const int sharp = (int)(V / (N * N));
    const size_t row = (size_t)b * rows + i;
    int w3[3];
    best_weights(S, p.t.terms, p.r.boxes + row * 4, p.r.scores[row * p.r.score_stride], p.r.lms + row * 10, p.fx, p.fy, w3);
    int32_t* sc = p.sc + (size_t)n * kBestScratchInts;
    sc[0] = sharp; sc[1] = w3[0]; sc[2] = w3[1]; sc[3] = w3[2];
    p.q[n] = (long long)sharp * w3[0] * w3[1] * w3[2];
}

__global__ __launch_bounds__(256) void best_decide_kernel(BestOffer p) {
    __shared__ int s_id[kBestMaxRows];            // the id of a row that counts, else 0
    __shared__ int s_match[kBestMaxRows];         // the LIVE entry that holds it, or -1
    __shared__ int s_free[kBestMaxRows];          // the first FREE entries in entry order
    __shared__ int s_w[4];
    __shared__ int s_over;
    const int b = blockIdx.x, tid = threadIdx.x, rows = p.r.rows, E = p.t.entries;
    const size_t st = (size_t)(p.stream0 + b);
    int32_t* meta = p.t.smeta + st * kBestStreamInts;
    int32_t* erec = p.t.erec + st * E * kBestRecInts;
    float* erow = p.t.erow + st * E * kBestRowFloats;
    const int32_t* info = p.r.info + (size_t)b * rows * 3;
    const int cnt = p.r.counts[b];
    const int n = cnt < 0 ? 0 : cnt < rows ? cnt : rows;
    const int t = meta[M_T], seq = meta[M_SEQ];
    if (tid == 0) s_over = 0;
    // 1. the rows that count
    for (int i = tid; i < n; i += 256) { const int id = info[i * 3]; s_id[i] = id >= 1 ? id : 0; s_match[i] = -1; }
    __syncthreads();
    bool dup[kBestMaxRows / 256];
    for (int k = 0; k < kBestMaxRows / 256; ++k) {
        const int i = k * 256 + tid;
        dup[k] = false;
        if (i < n && s_id[i]) { const int id = info[i * 3]; for (int j = 0; j < i; ++j) if (info[j * 3] == id) { dup[k] = true; break; } }
    }
    __syncthreads();
    for (int k = 0; k < kBestMaxRows / 256; ++k) if (dup[k]) s_id[k * 256 + tid] = 0;
    __syncthreads();
    // 2. presence of the LIVE entries, the finishing in entry order, the free list
    int n_fin = 0, n_free = 0;
    for (int e0 = 0; e0 < E; e0 += 256) {
        const int e = e0 + tid;
        int32_t* r = erec + (size_t)(e < E ? e : 0) * kBestRecInts;
        const int state = e < E ? r[R_STATE] : -1;
        bool present = false;
        if (state == ST_LIVE) {
            const int id = r[R_ID];
            for (int i = 0; i < n; ++i) if (s_id[i] == id) { present = true; s_match[i] = e; break; }
        }
        const bool fin = state == ST_LIVE && !present;
        const int rk = block_rank(fin, n_fin, s_w);
        if (fin) { r[R_STATE] = ST_DONE; r[R_SEQ] = seq + rk; }
        if (present) r[R_LAST] = t;
        const bool fr = state == ST_FREE;
        const int rf = block_rank(fr, n_free, s_w);
        if (fr && rf < kBestMaxRows) s_free[rf] = e;
    }
    __syncthreads();
    // 3. the eligible rows in row order
    int n_new = 0;
    const int o0 = p.offsets[b], o1 = p.offsets[b + 1];
    for (int i0 = 0; i0 < rows; i0 += 256) {
        const int i = i0 + tid;
        bool elig = false;
        int c = 0;
        if (i < n && s_id[i] && info[i * 3 + 2] == 0 && info[i * 3 + 1] >= p.t.min_hits &&
            o0 >= 0 && o0 <= o1 && i < o1 - o0 && (long long)o0 + i < p.cap_faces) {
            c = o0 + i;
            elig = p.sc[(size_t)c * kBestScratchInts + 4] == b * rows + i && p.q[c] >= 0;
        }
        const int m = elig ? s_match[i] : -1;
        const bool is_new = elig && m < 0;
        const int k = block_rank(is_new, n_new, s_w);
        int job_e = -1;
        if (elig) {
            const long long Q = p.q[c];
            int32_t* r = nullptr;
            if (m >= 0) {
                r = erec + (size_t)m * kBestRecInts;
                const int no = r[R_NOFF];
                r[R_NOFF] = no < (1 << 30) ? no + 1 : (1 << 30);
                if (Q > *reinterpret_cast<const long long*>(r + R_Q)) job_e = m;
            } else if (k < n_free) {              // (n_free may exceed the list: k < rows <= kBestMaxRows is inside it)
                job_e = s_free[k];
                r = erec + (size_t)job_e * kBestRecInts;
                r[R_STATE] = ST_LIVE; r[R_ID] = s_id[i]; r[R_FIRST] = t; r[R_LAST] = t; r[R_NOFF] = 1; r[R_SEQ] = 0;
            } else {
                s_over = 1;
            }
            if (job_e >= 0) {
                r = erec + (size_t)job_e * kBestRecInts;
                *reinterpret_cast<long long*>(r + R_Q) = Q;
                r[R_BEST] = t;
                for (int j = 0; j < 4; ++j) r[R_PARTS + j] = p.sc[(size_t)c * kBestScratchInts + j];
                float* w = erow + (size_t)job_e * kBestRowFloats;
                const size_t row = (size_t)b * rows + i;
                for (int j = 0; j < 4; ++j) w[j] = p.r.boxes[row * 4 + j];
                w[4] = p.r.scores[row * p.r.score_stride];
                for (int j = 0; j < 10; ++j) w[5 + j] = p.r.lms[row * 10 + j];
            }
        }
        if (i < rows) {
            int32_t* job = p.jobs + ((size_t)b * rows + i) * 2;
            job[0] = job_e >= 0 ? c : -1;
            job[1] = job_e >= 0 ? (int)(st * E) + job_e : -1;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int over = s_over;
        meta[M_T] = t + 1; meta[M_SEQ] = seq + n_fin;
        if (over) meta[M_STICKY] = meta[M_STICKY] | 1;
        if (p.flags) p.flags[b] = over;
    }
}

// jobs [.][2] = source chip, destination chip (in chips of `units` 16-byte units), or -1: no job
__global__ __launch_bounds__(256) void best_copy_kernel(const uint4* src, uint4* dst, const int32_t* jobs, int units) {
    const int from = jobs[(size_t)blockIdx.x * 2], to = jobs[(size_t)blockIdx.x * 2 + 1];
    if (from < 0 || to < 0) return;
    const uint4* s = src + (size_t)from * units;
    uint4* d = dst + (size_t)to * units;
    const int u0 = blockIdx.y * kCopyUnits, u1 = u0 + kCopyUnits < units ? u0 + kCopyUnits : units;
    for (int u = u0 + threadIdx.x; u < u1; u += 256) d[u] = s[u];
}

__global__ __launch_bounds__(256) void best_collect_kernel(BestCollect p) {
    __shared__ int s_seq[kBestMaxEntries];        // done_seq of a DONE entry, else -1
    __shared__ int s_w[4];
    const int b = blockIdx.x, tid = threadIdx.x, E = p.t.entries, cap = p.cap;
    const size_t st = (size_t)(p.stream0 + b);
    int32_t* meta = p.t.smeta + st * kBestStreamInts;
    int32_t* erec = p.t.erec + st * E * kBestRecInts;
    const float* erow = p.t.erow + st * E * kBestRowFloats;
    const int seq = meta[M_SEQ];
    int n_fl = 0, n_done = 0;
    for (int e0 = 0; e0 < E; e0 += 256) {
        const int e = e0 + tid;
        int32_t* r = erec + (size_t)(e < E ? e : 0) * kBestRecInts;
        int state = e < E ? r[R_STATE] : -1;
        if (p.flush) {                            // uniform
            const bool live = state == ST_LIVE;
            const int rk = block_rank(live, n_fl, s_w);
            if (live) { r[R_STATE] = state = ST_DONE; r[R_SEQ] = seq + rk; }
        }
        block_rank(state == ST_DONE, n_done, s_w);
        if (e < E) s_seq[e] = state == ST_DONE ? r[R_SEQ] : -1;
    }
    for (int k = tid; k < cap; k += 256) { p.jobs[((size_t)b * cap + k) * 2] = -1; p.jobs[((size_t)b * cap + k) * 2 + 1] = -1; }
    __syncthreads();
    for (int e = tid; e < E; e += 256) {
        const int mine = s_seq[e];
        if (mine < 0) continue;
        int k = 0;
        for (int j = 0; j < E; ++j) { const int v = s_seq[j]; k += v >= 0 && v < mine; }
        if (k >= cap) continue;
        int32_t* r = erec + (size_t)e * kBestRecInts;
        const size_t o = (size_t)b * cap + k;
        if (p.quality) p.quality[o] = *reinterpret_cast<const long long*>(r + R_Q);
        if (p.records) {
            int32_t* w = p.records + o * 8;
            w[0] = r[R_ID]; w[1] = r[R_BEST]; w[2] = r[R_FIRST]; w[3] = r[R_LAST]; w[4] = r[R_NOFF]; w[5] = r[R_PARTS];
            w[6] = r[R_PARTS + 1] | r[R_PARTS + 2] << 10 | r[R_PARTS + 3] << 20; w[7] = mine;
        }
        const float* q = erow + (size_t)e * kBestRowFloats;
        if (p.dets) for (int j = 0; j < 5; ++j) p.dets[o * 5 + j] = q[j];
        if (p.lms) for (int j = 0; j < 10; ++j) p.lms[o * 10 + j] = q[5 + j];
        p.jobs[o * 2] = (int)(st * E) + e; p.jobs[o * 2 + 1] = (int)o;
        r[R_STATE] = ST_FREE;
    }
    if (tid == 0) {
        const int out = n_done < cap ? n_done : cap;
        if (p.counts) p.counts[b] = out;
        if (p.pending) p.pending[b] = n_done - out;
        if (p.flags) p.flags[b] = meta[M_STICKY];
        meta[M_STICKY] = 0; meta[M_SEQ] = seq + n_fl;
    }
}

bool table_ok(const BestTable& t) {
    return t.size >= 16 && t.size <= 512 && !(t.size & 3) && t.entries >= 1 && t.entries <= kBestMaxEntries && t.erec && t.erow && t.chips && t.smeta &&
           !(reinterpret_cast<uintptr_t>(t.chips) & 15);
}

}  // namespace

const char* best_check(const cf_bestshot_opts* o, int n_streams) {
    if (!o) return "null options";
    if (o->size < 16 || o->size > 512 || (o->size & 3)) return "size must be a multiple of 4 in 16..512";
    if (o->entries < 1 || o->entries > kBestMaxEntries) return "entries must be in 1..2048";
    if (o->min_hits < 1 || o->min_hits > 1000) return "min_hits must be in 1..1000";
    if (o->terms < 0 || o->terms > 7) return "terms must be in 0..7";
    if (n_streams < 1 || n_streams > kTrackMaxStreams) return "n_streams must be in 1..4096";
    if ((long long)n_streams * o->entries > INT_MAX / 2) return "n_streams x entries exceeds 2^30";
    return nullptr;
}

size_t best_chip_bytes(int size) { return (size_t)3 * size * size; }

hipError_t launch_best_score(hipStream_t s, const BestOffer& p) {
    if (p.t.size < 16 || p.t.size > 512 || (p.t.size & 3) || p.B < 1 || p.r.rows < 1 ||      // (the score reads no table: cf_op_chip_quality has none) p.cap_faces < 0 || !p.offsets || !p.q || !p.sc || !p.r.info || !p.r.counts || !p.r.boxes ||
        !p.r.scores || !p.r.lms || (p.cap_faces > 0 && (!p.chips || (reinterpret_cast<uintptr_t>(p.chips) & 15))) || (long long)p.B * p.r.rows > INT_MAX / 2)
        return hipErrorInvalidValue;
    if (p.cap_faces == 0) return hipSuccess;
    hipLaunchKernelGGL(best_score_kernel, dim3(p.cap_faces), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_best_offer(hipStream_t s, const BestOffer& p) {
    if (!table_ok(p.t) || p.r.rows > kBestMaxRows || !p.jobs || p.stream0 < 0) return hipErrorInvalidValue;
    hipError_t e = launch_best_score(s, p);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(best_decide_kernel, dim3(p.B), dim3(256), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (p.cap_faces == 0) return hipSuccess;                    // no chip, no job
    const int units = (int)(best_chip_bytes(p.t.size) / 16);
    hipLaunchKernelGGL(best_copy_kernel, dim3(p.B * p.r.rows, (units + kCopyUnits - 1) / kCopyUnits), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(p.chips), reinterpret_cast<uint4*>(p.t.chips), p.jobs, units);
    return hipGetLastError();
}

hipError_t launch_best_collect(hipStream_t s, const BestCollect& p) {
    if (!table_ok(p.t) || p.B < 1 || p.cap < 0 || p.cap > kBestMaxEntries || p.stream0 < 0 || !p.jobs || (p.chips && (reinterpret_cast<uintptr_t>(p.chips) & 15)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(best_collect_kernel, dim3(p.B), dim3(256), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !p.chips || p.cap == 0) return e;
    const int units = (int)(best_chip_bytes(p.t.size) / 16);
    hipLaunchKernelGGL(best_copy_kernel, dim3(p.B * p.cap, (units + kCopyUnits - 1) / kCopyUnits), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(p.t.chips), reinterpret_cast<uint4*>(p.chips), p.jobs, units);
    return hipGetLastError();
}

}  // namespace cf
