// Lookback (cf_lookback_step / cf_op_lookback): a delay line of the last depth frames' tracked rows per stream, kept on the device, that
// covers a face in the frames BEFORE its first detection.  THE STATEMENT is in include/centerface_hip.h ("lookback");
// tests/lookback_cases.py restates it in numpy and the two agree bit for bit.  Integers and bit copies throughout, except the growth of a
// back-filled box: float64 in the order of the tracker's held rows (cf_trackemit.h), no FMA contraction.
//
// THE KERNEL
// One launch per step, one workgroup of 256 threads (four waves) per stream.  The queue of a stream is a rotating array of depth + 1
// entries in device memory the object owns -- per entry rec [rows][16] (box, score, lms[10], 0), info [rows][4] (id, hits, misses, born)
// and four meta words (seq, cut, n) --, its head, fill, max_id and seq_next four words beside it: the host reads none of them.
//   Push.  A parallel copy of the image's tracked rows into the entry behind the newest; born = id > max_id with the max_id the step
//   began with; the new max_id is a butterfly per wave and four LDS words.
//   Emit.  The oldest entry's rows are copied out as they are.  Then the later entries in entry order, up to the first one with `cut`
//   (a value every thread reads from the same word: the loop bounds around the barriers are workgroup-uniform).  An entry is walked in
//   chunks of 256 rows, thread t owning row base + t; the eligible rows of a chunk are ranked by one ballot per wave plus the four wave
//   counts in LDS, so the output order is entry order, then row order, and no atomic decides a position.  With confirm > 1 the id
//   columns of the later entries are staged in LDS one entry at a time by the whole workgroup and every candidate scans them (all
//   lanes read the same word: a broadcast); a chunk without a candidate skips the search (__syncthreads_or: uniform).
//   Thread 0 stores the count, the state words of the output and of the queue last, behind the barriers: every thread has read them by then.
//
// THE TRACE (cf_lookback_trace_enable, cf_lookback_step_frames; "lookback with a trace" in the header; tests/lookback_trace_cases.py)
// Two more launches ahead of the step kernel when an enabled object is pushed into: lookback_retain_kernel stores the frame's luma in
// the ring plane of the entry the push will fill, lookback_trace_kernel matches every row the push will call born backwards through the
// queued planes with the follower's device functions (cf_followmatch.h) and leaves PX, PY, SAD, code per distance in the entry's
// table.  The step kernel reads that table for the rows it appends (p.trace; nullptr: the untraced step, as it was).
#include <algorithm>
#include <cmath>

#include "cf_common.h"
#include "cf_followmatch.h"
#include "cf_kernels.h"

namespace cf {

namespace {

constexpr int kLbThreads = 256, kLbWaves = kLbThreads / 64;

__device__ inline bool lb_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN and the infinities

__global__ __launch_bounds__(kLbThreads) void lookback_step_kernel(LookbackParams p) {
    __shared__ int s_ids[kLookbackMaxRows];
    __shared__ int s_wave[kLbWaves];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, b = blockIdx.x, s = p.stream0 + b;
    const int cap = p.depth + 1, R = p.rows;
    int* qm = p.qmeta + (size_t)s * 4;                                       // head, fill, max_id, seq_next
    int head = qm[0], fill = qm[1], max_id = qm[2], seq_next = qm[3];
    const int pending = p.pend[s];
    int* em = p.emeta + (size_t)s * cap * 4;                                 // [cap][4]: seq, cut, n, 0
    float* rec = p.rec + (size_t)s * cap * R * 16;
    int* inf = p.info + (size_t)s * cap * R * 4;
    int* o_state = p.state + (size_t)b * 4;
    __syncthreads();                                                          // every thread holds the queue's words before thread 0 may store them

    if (p.push) {                                                             // fill <= depth here: a push that filled the queue emitted
        const int slot = (head + fill) % cap;
        const int n = min(max(p.in_counts[b], 0), min(p.in_stride, R));
        float* er = rec + (size_t)slot * R * 16;
        int* ei = inf + (size_t)slot * R * 4;
        const float* d = p.in_dets + (size_t)b * p.in_stride * 5;
        const float* l = p.in_lms + (size_t)b * p.in_stride * 10;
        const int* ii = p.in_info + (size_t)b * p.in_stride * 3;
        for (int e = t; e < n * 16; e += kLbThreads) {
            const int row = e >> 4, c = e & 15;
            er[e] = c < 5 ? d[row * 5 + c] : c < 15 ? l[row * 10 + c - 5] : 0.0f;
        }
        int mx = max_id;
        for (int i = t; i < n; i += kLbThreads) {
            const int id = ii[i * 3];
            ei[i * 4] = id; ei[i * 4 + 1] = ii[i * 3 + 1]; ei[i * 4 + 2] = ii[i * 3 + 2]; ei[i * 4 + 3] = id > max_id ? 1 : 0;
            mx = max(mx, id);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
        if (lane == 0) s_wave[wv] = mx;
        if (t == 0) {
            em[slot * 4] = seq_next;
            em[slot * 4 + 1] = (pending || (p.scene && p.scene[(size_t)b * 4] != CF_SCENE_SAME)) ? 1 : 0;
            em[slot * 4 + 2] = n; em[slot * 4 + 3] = 0;
        }
        __syncthreads();                                                      // the entry is visible to the whole workgroup
#pragma unroll
        for (int q = 0; q < kLbWaves; ++q) max_id = max(max_id, s_wave[q]);
        ++seq_next; ++fill;
        __syncthreads();                                                      // s_wave is free again
    }

    const bool emit = p.push ? fill == cap : fill > 0;
    if (!emit) {                                                              // uniform
        if (t == 0) {
            p.counts[b] = 0;
            o_state[0] = -1; o_state[1] = 0; o_state[2] = 0; o_state[3] = 0;
            qm[0] = head; qm[1] = fill; qm[2] = max_id; qm[3] = seq_next;
            if (p.push) p.pend[s] = 0;
        }
        return;
    }

    const int te = head;
    head = (head + 1) % cap; --fill;
    const int m = fill, nt = em[te * 4 + 2], seq_t = em[te * 4];
    float* od = p.dets + (size_t)b * R * 5;
    float* ol = p.lms + (size_t)b * R * 10;
    int* oi = p.out_info + (size_t)b * R * 3;
    float* oc = p.corners ? p.corners + (size_t)b * R * 4 : nullptr;
    {                                                                         // own rows, bit for bit
        const float* tr = rec + (size_t)te * R * 16;
        const int* ti = inf + (size_t)te * R * 4;
        for (int e = t; e < nt * 16; e += kLbThreads) {
            const int row = e >> 4, c = e & 15;
            const float v = tr[e];
            if (c < 5) { od[row * 5 + c] = v; if (c < 4 && oc) oc[row * 4 + c] = v; }
            else if (c < 15) ol[row * 10 + c - 5] = v;
        }
        for (int e = t; e < nt * 3; e += kLbThreads) oi[e] = ti[(e / 3) * 4 + e % 3];
        if (p.moves) for (int e = t; e < nt * 4; e += kLbThreads) p.moves[(size_t)b * R * 4 + e] = (e & 3) == 3 ? CF_FOLLOW_NONE : 0;
    }
    int stop = m + 1;                                                         // the first later entry of another scene
    for (int j = m; j >= 1; --j) if (em[((te + j) % cap) * 4 + 1]) stop = j;
    int written = nt, flags = 0;
    for (int j = 1; j < stop; ++j) {
        const int ej = (te + j) % cap, nj = em[ej * 4 + 2];
        const float* jr = rec + (size_t)ej * R * 16;
        const int* ji = inf + (size_t)ej * R * 4;
        for (int base = 0; base < nj; base += kLbThreads) {
            const int i = base + t;
            bool cand = false;
            int id = 0;
            float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
            if (i < nj && ji[i * 4 + 3]) {
                id = ji[i * 4];
                const float4 bx = *reinterpret_cast<const float4*>(jr + (size_t)i * 16);
                x1 = bx.x; y1 = bx.y; x2 = bx.z; y2 = bx.w;
                cand = lb_finite(x1) && lb_finite(y1) && lb_finite(x2) && lb_finite(y2);
            }
            int seen = 1;                                                     // e_j itself shows the id
            if (p.confirm > 1 && __syncthreads_or(cand ? 1 : 0)) {
                for (int jj = j + 1; jj < stop; ++jj) {
                    const int ejj = (te + jj) % cap, njj = em[ejj * 4 + 2];
                    const int* qi = inf + (size_t)ejj * R * 4;
                    __syncthreads();                                          // the scan of the entry before is over
                    for (int k = t; k < njj; k += kLbThreads) s_ids[k] = qi[k * 4];
                    __syncthreads();
                    if (cand) {
                        bool found = false;
                        for (int k = 0; k < njj; ++k) found |= s_ids[k] == id;
                        seen += found ? 1 : 0;
                    }
                }
            }
            const bool on = cand && seen >= p.confirm;
            const unsigned long long bal = __ballot(on);
            if (lane == 0) s_wave[wv] = __popcll(bal);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int q = 0; q < kLbWaves; ++q) { const int c = s_wave[q]; before += q < wv ? c : 0; total += c; }
            __syncthreads();                                                  // s_wave is free again
            if (on) {
                const int r = written + before + __popcll(bal & ((1ull << lane) - 1ull));
                if (r < R) {
                    const float* q = jr + (size_t)i * 16;
                    float lm[10];
                    for (int c = 0; c < 10; ++c) lm[c] = q[5 + c];
                    int mv[4] = {0, 0, 0, CF_FOLLOW_NONE};
                    if (p.trace) {                                            // an enabled object: where the walk found the face at distance j
                        const int* T = p.trace + ((((size_t)s * cap + ej) * R + i) * p.depth + (j - 1)) * 4;
                        for (int c = 0; c < 4; ++c) mv[c] = T[c];
                    }
                    if (mv[0] != 0 || mv[1] != 0) {                           // the follower's formula; then the growth
                        const double mx = (double)mv[0] / p.fx, my = (double)mv[1] / p.fy;
                        x1 = (float)((double)x1 + mx); y1 = (float)((double)y1 + my); x2 = (float)((double)x2 + mx); y2 = (float)((double)y2 + my);
                        for (int c = 0; c < 10; c += 2) { lm[c] = (float)((double)lm[c] + mx); lm[c + 1] = (float)((double)lm[c + 1] + my); }
                    }
                    if (p.moves) { int* om = p.moves + ((size_t)b * R + r) * 4; for (int c = 0; c < 4; ++c) om[c] = mv[c]; }
                    const double g = 1.0 + (double)p.grow * (double)j;
                    const double cx = ((double)x1 + (double)x2) * 0.5, hw = ((double)x2 - (double)x1) * 0.5 * g;
                    const double cy = ((double)y1 + (double)y2) * 0.5, hh = ((double)y2 - (double)y1) * 0.5 * g;
                    const float X1 = (float)(cx - hw), X2 = (float)(cx + hw), Y1 = (float)(cy - hh), Y2 = (float)(cy + hh);
                    float* d = od + (size_t)r * 5;
                    d[0] = X1; d[1] = Y1; d[2] = X2; d[3] = Y2; d[4] = q[4];
                    if (oc) { oc[r * 4] = X1; oc[r * 4 + 1] = Y1; oc[r * 4 + 2] = X2; oc[r * 4 + 3] = Y2; }
                    for (int c = 0; c < 10; ++c) ol[(size_t)r * 10 + c] = lm[c];
                    oi[r * 3] = id; oi[r * 3 + 1] = 0; oi[r * 3 + 2] = j;
                }
            }
            if (written + total > R) flags |= 1;                             // an eligible row found no place: THAT FACE IS NOT COVERED
            written = min(R, written + total);
        }
    }
    if (t == 0) {
        p.counts[b] = written;
        o_state[0] = seq_t; o_state[1] = nt; o_state[2] = written - nt; o_state[3] = flags;
        qm[0] = head; qm[1] = fill; qm[2] = max_id; qm[3] = seq_next;
        if (p.push) p.pend[s] = 0;
    }
}

// ---- the trace of an enabled object: retain, then walk the queue backwards
constexpr int kLbFrames = 16;                                      // frames (= streams) of one retain launch: their plane-0 addresses go by value
struct LbPlanes { const uint8_t* p0[kLbFrames]; };

// Retain: the luma of frame f0 + blockIdx.y goes into the ring plane of the entry the push behind this launch will fill, which the
// queue's words name.  A thread makes 16 lumas and stores them as one uint4 (the ring's rows are multiples of 16 bytes; the bytes past w
// are zero); a Y plane is a pitched copy, a BGR row gives 16 lumas per 48 bytes.  A source whose base and pitch are multiples of 16 is
// read in 16-byte loads, any other in dwords (planes are 4-byte aligned with pitches that are multiples of 4); the last chunk of a row
// whose width is no multiple of 16 is read byte by byte.
__global__ __launch_bounds__(256) void lookback_retain_kernel(LookbackTraceParams p, LbPlanes fr, int f0) {
    const int b = f0 + blockIdx.y, s = p.step.stream0 + b, cap = p.step.depth + 1;
    const int* qm = p.step.qmeta + (size_t)s * 4;
    const int slot = (qm[0] + qm[1]) % cap;                                   // head + fill: fill <= depth at a push
    const int h = p.g.h, w = p.g.w, wp = lookback_luma_pitch(w), cpr = wp / 16;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= h * cpr) return;
    const int y = idx / cpr, x = (idx - y * cpr) * 16;
    const uint8_t* base = fr.p0[blockIdx.y];
    const uint8_t* src = base + (size_t)y * p.g.pitch0;
    const bool a16 = (((uintptr_t)base | (uintptr_t)(unsigned)p.g.pitch0) & 15) == 0;
    const bool bgr = p.g.format == CF_FRAME_BGR;
    uint32_t out[4] = {0u, 0u, 0u, 0u};
    if (x + 16 <= w) {
        if (bgr) {
            uint32_t d[12];
            const uint8_t* q = src + 3 * x;                                   // 48-byte steps from the row's start
            if (a16) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint4 v = reinterpret_cast<const uint4*>(q)[k];
                    d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) d[k] = reinterpret_cast<const uint32_t*>(q)[k];
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int k = 3 * i;
                const int cb = (int)((d[k >> 2] >> (8 * (k & 3))) & 255u), cg = (int)((d[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 255u),
                          cr = (int)((d[(k + 2) >> 2] >> (8 * ((k + 2) & 3))) & 255u);
                out[i >> 2] |= (uint32_t)luma_bgr(cb, cg, cr) << (8 * (i & 3));
            }
        } else if (a16) {
            const uint4 v = *reinterpret_cast<const uint4*>(src + x);
            out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) out[k] = reinterpret_cast<const uint32_t*>(src + x)[k];
        }
    } else {
        for (int i = 0; x + i < w; ++i) {
            const int xx = x + i;
            const int v = bgr ? luma_bgr(src[3 * xx], src[3 * xx + 1], src[3 * xx + 2]) : src[xx];
            out[i >> 2] |= (uint32_t)v << (8 * (i & 3));
        }
    }
    uint8_t* dst = p.luma + (((size_t)s * cap + slot) * h + y) * wp + x;
    *reinterpret_cast<uint4*>(dst) = make_uint4(out[0], out[1], out[2], out[3]);
}

// Trace: one workgroup per (row, stream) of the rows about to be pushed; it leaves at once for a row the push will not call born (or
// whose corners are not finite: no emit reads its trace).  The template of the birth frame stays in LDS for the whole chain; the loop
// over the distances has workgroup-uniform bounds -- every thread reads the queue's and the entries' words from the same addresses, and
// the end of a chain (LOST) is decided from the key every thread reads out of LDS (match_best_key).  The phases are the follower's own
// device functions (cf_followmatch.h), on the dense retained planes.
__global__ __launch_bounds__(kMatchThreads) void lookback_trace_kernel(LookbackTraceParams p) {
    __shared__ int s_sum[kWin * kWin];
    __shared__ uint32_t s_win[kWin * kWinPitch];
    __shared__ uint32_t s_tpl[kFollowSide * kFollowSide / 4];
    __shared__ unsigned long long s_key[kMatchThreads / 64];
    const LookbackParams& q = p.step;
    const int i = blockIdx.x, b = blockIdx.y, t = threadIdx.x, s = q.stream0 + b, cap = q.depth + 1, R = q.rows;
    const int n = min(max(q.in_counts[b], 0), min(q.in_stride, R));
    if (i >= n) return;
    const int* qm = q.qmeta + (size_t)s * 4;
    const int head = qm[0], m = qm[1], max_id = qm[2];                        // m entries are queued in front of the new one
    if (!(q.in_info[((size_t)b * q.in_stride + i) * 3] > max_id)) return;    // not born
    const float* bx = q.in_dets + ((size_t)b * q.in_stride + i) * 5;
    const float x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
    if (!(lb_finite(x1) && lb_finite(y1) && lb_finite(x2) && lb_finite(y2))) return;
    const int slot = (head + m) % cap;
    int* T = p.trace + (((size_t)s * cap + slot) * R + i) * q.depth * 4;
    const double sw = ((double)x2 - (double)x1) * p.fx, sh = ((double)y2 - (double)y1) * p.fy;
    const double side = sh > sw ? sh : sw;
    if (!(side > 0.0)) {
        for (int d = t; d < m; d += kMatchThreads) { T[d * 4] = 0; T[d * 4 + 1] = 0; T[d * 4 + 2] = 0; T[d * 4 + 3] = CF_FOLLOW_NONE; }
        return;
    }
    const double cx = ((double)x1 + (double)x2) * 0.5 * p.fx, cy = ((double)y1 + (double)y2) * 0.5 * p.fy;
    const int CX = (int)floor(fmin(fmax(cx, -8192.0), 16384.0)), CY = (int)floor(fmin(fmax(cy, -8192.0), 16384.0));
    const int S = (int)ceil(fmin(fmax(side, 1.0), 8192.0));
    const int c = (S + kFollowSide - 1) / kFollowSide;
    const int h = p.g.h, w = p.g.w, wp = lookback_luma_pitch(w);
    const uint8_t* ring = p.luma + (size_t)s * cap * h * wp;
    const size_t plane = (size_t)h * wp;
    // learn: the template of the birth frame
    match_cell_means<false>(t, ring + slot * plane, wp, h, w, false, CX - (kFollowSide / 2) * c, CY - (kFollowSide / 2) * c, kFollowSide, c, s_sum, s_win);
    if (t < kFollowSide * kFollowSide / 4) s_tpl[t] = s_win[(t >> 2) * kWinPitch + (t & 3)];
    __syncthreads();
    const int* em = q.emeta + (size_t)s * cap * 4;
    const bool cut_new = q.pend[s] || (q.scene && q.scene[(size_t)b * 4] != CF_SCENE_SAME);
    const int Rs = p.search, nw = kFollowSide + 2 * Rs;
    int PX = 0, PY = 0;
    for (int d = 1; d <= m; ++d) {
        const bool cut = d == 1 ? cut_new : em[((head + m - d + 1) % cap) * 4 + 1] != 0;
        if (cut) break;                                                       // uniform: the same words for every thread
        const int sl = (head + m - d) % cap;
        match_cell_means<false>(t, ring + sl * plane, wp, h, w, false, CX + PX - (kFollowSide / 2 + Rs) * c, CY + PY - (kFollowSide / 2 + Rs) * c, nw, c,
                                s_sum, s_win);
        const unsigned long long best = match_best_key(t, Rs, s_win, s_tpl, s_key);      // the same key in every thread
        const int sad = match_key_sad(best);
        const bool lost = sad > p.max_sad;
        if (!lost) { PX += match_key_dx(best, Rs) * c; PY += match_key_dy(best, Rs) * c; }
        if (t == 0)
            for (int e = d; e <= (lost ? m : d); ++e) {                       // a lost chain: every further distance takes the same words
                int* o = T + (e - 1) * 4;
                o[0] = PX; o[1] = PY; o[2] = sad; o[3] = lost ? CF_FOLLOW_LOST : CF_FOLLOW_MOVED;
            }
        if (lost) break;                                                      // uniform
    }
}

}  // namespace

const char* lookback_check(const cf_lookback_opts* o, int n_streams) {
    if (!o) return "null options";
    if (o->depth < 1 || o->depth > kLookbackMaxDepth) return "depth must be in 1..32";
    if (o->rows < 1 || o->rows > kLookbackMaxRows) return "rows must be in 1..1024";
    if (!std::isfinite(o->grow) || o->grow < 0.0f || o->grow > 1.0f) return "grow must be finite and in 0..1";
    if (o->confirm < 1 || o->confirm > o->depth + 1) return "confirm must be in 1..depth + 1";
    if (n_streams < 1 || n_streams > kTrackMaxStreams) return "n_streams must be in 1..4096";
    return nullptr;
}

hipError_t launch_lookback_step(hipStream_t s, const LookbackParams& p) {
    const cf_lookback_opts o{p.depth, p.rows, p.grow, p.confirm};
    if (lookback_check(&o, 1) || p.B < 1 || p.stream0 < 0 || !p.qmeta || !p.pend || !p.emeta || !p.rec || !p.info || !p.dets || !p.lms || !p.out_info ||
        !p.counts || !p.state || (p.push && (!p.in_dets || !p.in_lms || !p.in_info || !p.in_counts || p.in_stride < 1)) ||
        (p.trace && (!(p.fx > 0.0) || !(p.fy > 0.0))))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(lookback_step_kernel, dim3(p.B), dim3(kLbThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_lookback_trace(hipStream_t s, const LookbackTraceParams& p) {
    const FrameGeo& g = p.g;
    const LookbackParams& q = p.step;
    const cf_lookback_opts o{q.depth, q.rows, q.grow, q.confirm};
    const cf_follow_opts fo{p.search, p.max_sad};
    if (lookback_check(&o, 1) || follow_check(&fo, g.format, g.B, g.h, g.w, g.pitch0, g.pitch1) || redact_check_planes(g.format, p.planes, g.B, 1, g.pitch0, g.pitch1) ||
        ((g.h | g.w) & 1) || g.h < 2 || g.w < 2 || (g.pitch0 & 3) || g.B != q.B || !q.push || q.stream0 < 0 || !(p.fx > 0.0) || !(p.fy > 0.0) || !p.luma || !p.trace ||
        !q.qmeta || !q.pend || !q.emeta || !q.in_dets || !q.in_info || !q.in_counts || q.in_stride < 1)
        return hipErrorInvalidValue;
    const int chunks = g.h * (lookback_luma_pitch(g.w) / 16);
    for (int f0 = 0; f0 < g.B; f0 += kLbFrames) {
        const int nb = std::min(g.B - f0, kLbFrames);
        LbPlanes fr{};
        for (int k = 0; k < nb; ++k) fr.p0[k] = (const uint8_t*)p.planes[3 * (f0 + k)];
        hipLaunchKernelGGL(lookback_retain_kernel, dim3((chunks + 255) / 256, nb), dim3(256), 0, s, p, fr, f0);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(lookback_trace_kernel, dim3(std::min(q.in_stride, q.rows), g.B), dim3(kMatchThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace cf
