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
#include <algorithm>
#include <cmath>

#include "cf_common.h"
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
                    const double g = 1.0 + (double)p.grow * (double)j;
                    const double cx = ((double)x1 + (double)x2) * 0.5, hw = ((double)x2 - (double)x1) * 0.5 * g;
                    const double cy = ((double)y1 + (double)y2) * 0.5, hh = ((double)y2 - (double)y1) * 0.5 * g;
                    const float X1 = (float)(cx - hw), X2 = (float)(cx + hw), Y1 = (float)(cy - hh), Y2 = (float)(cy + hh);
                    const float* q = jr + (size_t)i * 16;
                    float* d = od + (size_t)r * 5;
                    d[0] = X1; d[1] = Y1; d[2] = X2; d[3] = Y2; d[4] = q[4];
                    if (oc) { oc[r * 4] = X1; oc[r * 4 + 1] = Y1; oc[r * 4 + 2] = X2; oc[r * 4 + 3] = Y2; }
                    for (int c = 0; c < 10; ++c) ol[(size_t)r * 10 + c] = q[5 + c];
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
        !p.counts || !p.state || (p.push && (!p.in_dets || !p.in_lms || !p.in_info || !p.in_counts || p.in_stride < 1)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(lookback_step_kernel, dim3(p.B), dim3(kLbThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace cf
