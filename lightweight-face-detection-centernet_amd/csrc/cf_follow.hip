// The follower of the face tracks (cf_track_follow / cf_op_follow): where did every tracked face go, measured by block matching in the
// luma of the new frame, without a forward.  THE STATEMENT is in include/centerface_hip.h ("follow tracked faces between detections");
// tests/follow_cases.py restates it in numpy and the two agree bit for bit.  Integers throughout, except the box geometry and the move
// of the state, which are float64 in the order written (this file is built without FMA contraction).
//
// THE KERNELS
// follow_kernel: one workgroup of 256 threads per (slot, stream); it leaves at once when the slot is not alive.
//   1. Cell sums of the window -- 16 x 16 cells when the slot learns, (16 + 2R)^2 <= 32 x 32 when it follows.  A work item is one frame
//      row of one cell (c pixels): neighbouring lanes read neighbouring runs, so a wave reads one contiguous stretch of the row.  A run
//      inside the frame is read through aligned dwords (a Y run: the head and tail bytes singly, the dwords summed by v_sad_u8 against 0;
//      a BGR run: its 3c bytes taken out of the dwords that hold them); a run that crosses the frame border clamps pixel by pixel.
//      The partial sums are added into LDS: integer addition, so the order of the adds does not show.  Then every cell sum becomes its
//      rounded mean, one byte, in window rows of 9 dwords.
//   2. The (2R + 1)^2 <= 289 SADs, one candidate per thread: per template row four v_sad_u8 on four packed cells each, the window's
//      bytes brought to the template's alignment by v_alignbyte_b32 (__builtin_amdgcn_sad_u8, __builtin_amdgcn_alignbyte: the builtins
//      are what ships, there is no plain-loop variant).
//   3. One 64-bit key (SAD, dx^2 + dy^2, dy + R, dx + R) per thread, reduced by min: xor butterfly in the wave, four keys through LDS.
//   4. Thread 0 moves the state (or not) and writes the slot's px, py, SAD, code.
// follow_emit_kernel: a second launch, one wave per stream: step 5 of the tracker's statement (cf_trackemit.h, the very function the
// update kernel calls) from the moved state, plus the moves in the same row order.
// The cost of phase 1 grows with the face's area: c * c pixels per cell, c = ceil(side / 16).
// Phases 1 to 3 are device functions in cf_followmatch.h, which the lookback's backward trace (cf_lookback.hip) calls too.
#include <algorithm>
#include <cmath>

#include "cf_common.h"
#include "cf_followmatch.h"
#include "cf_kernels.h"
#include "cf_trackemit.h"

namespace cf {

namespace {

constexpr int kFollowFrames = 16;                                  // frames (= streams) of one launch: their plane-0 addresses go by value
struct FollowPlanes { const uint8_t* p0[kFollowFrames]; };

__global__ __launch_bounds__(256) void follow_kernel(FollowParams p, FollowPlanes fr) {
    __shared__ int s_sum[kWin * kWin];
    __shared__ uint32_t s_win[kWin * kWinPitch];
    __shared__ uint32_t s_tpl[kFollowSide * kFollowSide / 4];
    __shared__ unsigned long long s_key[4];
    const int k = blockIdx.x, b = blockIdx.y, t = threadIdx.x, M = p.max_tracks;
    const size_t slot = (size_t)(p.stream0 + b) * M + k;
    const int* meta = p.meta + slot * 4;
    if (!meta[0]) return;
    float* rec = p.rec + slot * 16;
    int* tm = p.tmeta + slot * 6;
    uint32_t* tpl = reinterpret_cast<uint32_t*>(p.tpl + slot * (kFollowSide * kFollowSide));
    int* res = p.slot_moves + ((size_t)b * M + k) * 4;
    const float x1 = rec[0], y1 = rec[1], x2 = rec[2], y2 = rec[3];
    const double sw = ((double)x2 - (double)x1) * p.fx, sh = ((double)y2 - (double)y1) * p.fy;
    const double side = sh > sw ? sh : sw;
    if (!(isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2)) || !(side > 0.0)) {
        if (t == 0) { res[0] = 0; res[1] = 0; res[2] = 0; res[3] = CF_FOLLOW_NONE; }
        return;
    }
    const double cx = ((double)x1 + (double)x2) * 0.5 * p.fx, cy = ((double)y1 + (double)y2) * 0.5 * p.fy;
    const int CX = (int)floor(fmin(fmax(cx, -8192.0), 16384.0)), CY = (int)floor(fmin(fmax(cy, -8192.0), 16384.0));
    const int S = (int)ceil(fmin(fmax(side, 1.0), 8192.0));
    const int id = meta[1];
    bool learn = tm[1] != id;
    for (int q = 0; q < 4; ++q) learn = learn || tm[2 + q] != __float_as_int(rec[q]);
    learn = learn || tm[0] < 1 || tm[0] > kRedactMaxSide / kFollowSide;      // (only a learn writes tpl_c, so never: the loops below trust c)
    // (every thread has read the state by the first barrier below; thread 0 writes it behind the last one)
    const int c = learn ? (S + kFollowSide - 1) / kFollowSide : tm[0];
    const int R = learn ? 0 : p.search, n = kFollowSide + 2 * R, X0 = CX - (kFollowSide / 2 + R) * c, Y0 = CY - (kFollowSide / 2 + R) * c;
    // 1. the cell means of the window
    match_cell_means<true>(t, fr.p0[b], p.g.pitch0, p.g.h, p.g.w, p.g.format == CF_FRAME_BGR, X0, Y0, n, c, s_sum, s_win);
    if (learn) {
        if (t < kFollowSide * kFollowSide / 4) tpl[t] = s_win[(t >> 2) * kWinPitch + (t & 3)];
        if (t == 0) {
            tm[0] = c; tm[1] = id;
            for (int q = 0; q < 4; ++q) tm[2 + q] = __float_as_int(rec[q]);
            res[0] = 0; res[1] = 0; res[2] = 0; res[3] = CF_FOLLOW_LEARNED;
        }
        return;
    }
    // 2. + 3. the SADs and the best of them
    if (t < kFollowSide * kFollowSide / 4) s_tpl[t] = tpl[t];
    __syncthreads();
    const unsigned long long best = match_best_key(t, R, s_win, s_tpl, s_key);
    // 4. the state and the slot's result
    if (t == 0) {
        const int sad = match_key_sad(best), px = match_key_dx(best, R) * c, py = match_key_dy(best, R) * c;
        const bool moved = sad <= p.max_sad;
        if (moved) {
            const double mx = (double)px / p.fx, my = (double)py / p.fy;
            for (int q = 0; q < 4; q += 2) { rec[q] = (float)((double)rec[q] + mx); rec[q + 1] = (float)((double)rec[q + 1] + my); }
            for (int q = 5; q < 15; q += 2) { rec[q] = (float)((double)rec[q] + mx); rec[q + 1] = (float)((double)rec[q + 1] + my); }
            for (int q = 0; q < 4; ++q) tm[2 + q] = __float_as_int(rec[q]);
        }
        res[0] = px; res[1] = py; res[2] = sad; res[3] = moved ? CF_FOLLOW_MOVED : CF_FOLLOW_LOST;
    }
}

__global__ __launch_bounds__(64) void follow_emit_kernel(FollowParams p) {
    const int b = blockIdx.x, lane = threadIdx.x, M = p.max_tracks;
    const size_t so = (size_t)(p.stream0 + b) * M, ro = (size_t)b * M;
    const int* meta = p.meta + so * 4;
    const TrackRows o{p.dets + ro * 5, p.lms_out + ro * 10, p.info + ro * 3, p.corners + ro * 4};
    const int* sm = p.slot_moves + ro * 4;
    int* mv = p.moves + ro * 4;
    const int n = track_emit_rows(lane, M, p.hold_grow, meta, p.rec + so * 16, o, [&](int k) { return meta[k * 4] != 0; },
                                  [&](int r, int k) { for (int q = 0; q < 4; ++q) mv[r * 4 + q] = sm[k * 4 + q]; });
    if (lane == 0) p.out_counts[b] = n;
}

}  // namespace

const char* follow_check(const cf_follow_opts* o, int format, int B, int h, int w, int pitch0, int pitch1) {
    if (!o) return "null options";
    const char* geo = frame_geometry_check(FrameGeo{format, B, h, w, pitch0, pitch1}, 1, false);
    if (format < CF_YUV_NV12 || format > CF_FRAME_BGR) return geo;             // the format is refused first, then the options
    if (o->search < 1 || o->search > kFollowMaxSearch) return "search must be in 1..8";
    if (o->max_sad < 0 || o->max_sad > kFollowMaxSad) return "max_sad must be in 0..65280";
    return geo;
}

hipError_t launch_track_follow(hipStream_t s, const FollowParams& p) {
    const FrameGeo& g = p.g;
    cf_follow_opts o{p.search, p.max_sad};
    if (follow_check(&o, g.format, g.B, g.h, g.w, g.pitch0, g.pitch1) || redact_check_planes(g.format, p.planes, g.B, 1, g.pitch0, g.pitch1) ||
        p.max_tracks < 1 || p.max_tracks > kTrackMaxSlots || p.stream0 < 0 || !(p.fx > 0.0) || !(p.fy > 0.0) || !p.meta || !p.rec || !p.tpl ||
        !p.tmeta || !p.slot_moves || !p.dets || !p.lms_out || !p.info || !p.corners || !p.out_counts || !p.moves)
        return hipErrorInvalidValue;
    for (int f0 = 0; f0 < g.B; f0 += kFollowFrames) {
        const int nb = std::min(g.B - f0, kFollowFrames);
        FollowPlanes fr{};
        for (int k = 0; k < nb; ++k) fr.p0[k] = (const uint8_t*)p.planes[3 * (f0 + k)];
        FollowParams q = p;
        q.g.B = nb; q.stream0 = p.stream0 + f0; q.slot_moves = p.slot_moves + (size_t)f0 * p.max_tracks * 4;
        hipLaunchKernelGGL(follow_kernel, dim3(p.max_tracks, nb), dim3(256), 0, s, q, fr);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(follow_emit_kernel, dim3(g.B), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace cf
