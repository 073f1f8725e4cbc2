// Face tracks across the frames of a video stream (cf_track_update / cf_op_track): the association of the current frame's detection rows
// with the tracks of the frames before, and the rows -- detections and held tracks -- that the redaction of this frame covers.
//
// THE STATEMENT (tests/track_cases.py restates it in numpy; the two agree bit for bit)
// A tracker holds n_streams independent streams; stream s has max_tracks slots.  A slot holds: alive, id, hits, misses, box[4] f32,
// score f32, lms[10] f32.  The stream holds next_id (starts at 1, never reused).  One update of stream s with the rows
// i < n = min(count, rows written per image), in row order (the decode's / the merge's keep order):
//   1. A row with a non-finite corner is skipped: it neither matches nor is born.
//   2. Match.  For each remaining row in row order, over the slots that were alive WHEN THE UPDATE BEGAN and are not yet matched in this
//      update, the measure is the decode's float32 "+1" IoU of the slot's box t and the row's box d:
//        at = (t.x2 - t.x1 + 1) * (t.y2 - t.y1 + 1), ad likewise; w = max(0, min(t.x2, d.x2) - max(t.x1, d.x1) + 1), h likewise;
//        inter = w * h; iou = inter / (at + ad - inter)            (float32 throughout, every operation rounded, no FMA contraction)
//      The largest measure wins, ties go to the lowest slot; a slot whose measure is NaN (or -inf) never wins.  A winner with
//      iou >= iou_thresh takes the row's box, score and landmarks as they are, hits = min(hits + 1, 1 << 30), misses = 0.  Otherwise
//      (or without a winner) the row is NEW.
//   3. Age.  Every slot that was alive at the start and is unmatched: hits < min_hits -> freed at once (a tentative track is never
//      held); otherwise misses += 1, and it is freed when misses > max_age.
//   4. Birth.  New rows, in row order, take the lowest free slot (free after step 3) with id = next_id++, hits = 1, misses = 0.  With no
//      free slot the row is DROPPED -- that face is not covered -- and bit 0 of flags[s] is set.
//   5. Output.  The alive slots in ascending slot order become rows k < counts[s] <= max_tracks: dets[k] = box, score; lms[k];
//      info[k] = id, hits, misses.  misses == 0: the box bit for bit.  misses > 0 (a held track): the box grown about its centre in
//      float64, cx = ((double)x1 + (double)x2) * 0.5, hw = ((double)x2 - (double)x1) * 0.5 * (1.0 + (double)hold_grow * (double)misses),
//      x1' = (float)(cx - hw), x2' = (float)(cx + hw), y likewise; its landmarks are the last ones seen.
//
// TWO THRESHOLDS (cf_track_create_weak / cf_op_track_weak; tests/weak_cases.py restates it).  A tracker created with birth_score and
// weak_iou, both float32, finite, in (0, 1], calls a row STRONG when score > birth_score (strict, float32: the threshold decodes keep
// hm > score_thresh, so the strong rows of a decode at a lower threshold are the rows of a decode at birth_score) and WEAK otherwise -- a
// NaN score and score == birth_score are weak.  Step 1 holds for both kinds.  Step 2 becomes
//   2a. Strong pass: step 2 over the strong rows only, in row order; a strong row without a winner >= iou_thresh is NEW.
//   2b. Weak pass, after every strong row: over the weak rows in row order, among the slots that were alive when the update began, are
//       matched by neither pass so far, and had hits >= min_hits when the update began (confirmed tracks, live or held; a tentative
//       track is never matched by a weak row).  Measure, arg-max, tie rule and NaN rule are step 2's.  A winner with iou >= weak_iou takes
//       the row exactly as a strong match does (box, score, landmarks as they are, hits = min(hits + 1, 1 << 30), misses = 0).  Otherwise
//       the row is DISCARDED: not new, never born, never the cause of flag bit 0.
// Steps 3 to 5 are unchanged, so a weak match stops the ageing and its row comes out ungrown.  Bit 1 (value 2) of flags[s] is set when at
// least one weak row matched in this update of stream s.  Without the two numbers the update is the one above, bit for bit.
//
// THE KERNEL
// One launch per update, one workgroup of ONE wave per stream.  The loop over the rows is sequential by definition; per row only an
// arg-max over the slots is needed.  Lane l owns the slots j * 64 + l (j < ceil(max_tracks / 64) <= 16): it keeps their start-of-update
// boxes and a flag in LDS words that no other lane touches, takes the best of its own slots in ascending order, and a six-step
// xor butterfly over (measure, slot) leaves the winner in every lane.  No workgroup barrier in the loop.  The owner of the winning slot
// writes the slot.  Free-slot ranks (birth) and alive-slot ranks (compaction) are prefix sums: one ballot per 64 slots plus a running
// base, in slot order because slot = j * 64 + lane.  The state lives in device memory the tracker owns; nothing is read on the host.
// A weak tracker is the same launch with the row loop run twice (a template parameter: the plain instance has no second loop, reads no
// score in the loop and knows no fourth flag bit); the prologue that reads `alive` also reads `hits` once for the "confirmed at the
// start" bit of the lane-owned flag word.
#include <climits>
#include <cmath>

#include "cf_common.h"
#include "cf_kernels.h"
#include "cf_trackemit.h"

namespace cf {

namespace {

// s_flag: alive when the update began | matched in this update | alive after it | (weak trackers) hits >= min_hits when it began
constexpr int F_START = 1, F_MATCHED = 2, F_ALIVE = 4, F_CONF = 8;

// The winner of row box d among the slots whose flag word, under MASK, equals WANT: each lane over its own slots in ascending order,
// then the butterfly; every lane of the wave calls it and every lane returns the same (bv, bk), bk == INT_MAX without a winner.
template <int MASK, int WANT>
__device__ __forceinline__ void track_best(const float4 d, int lane, int M, int per, const int* s_flag, const float4* s_box, float& bv, int& bk) {
    const float ad = (d.z - d.x + 1.0f) * (d.w - d.y + 1.0f);
    bv = -INFINITY;
    bk = INT_MAX;
    for (int j = 0; j < per; ++j) {
        const int k = j * 64 + lane;
        if (k >= M || (s_flag[k] & MASK) != WANT) continue;
        const float4 t = s_box[k];
        const float at = (t.z - t.x + 1.0f) * (t.w - t.y + 1.0f);
        const float w = fmaxf(0.0f, fminf(t.z, d.z) - fmaxf(t.x, d.x) + 1.0f), h = fmaxf(0.0f, fminf(t.w, d.w) - fmaxf(t.y, d.y) + 1.0f);
        const float inter = w * h;
        const float v = inter / (at + ad - inter);
        if (v > bv) { bv = v; bk = k; }            // ascending k: the lowest slot among equals; a NaN never passes
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int ok = __shfl_xor(bk, off);
        if (ov > bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
    }
}

// The owner of the winning slot bk takes row i: the slot's flag word, its record and its counters (no other lane touches them).
__device__ __forceinline__ void track_take(const TrackParams& p, int lane, int bk, int i, const float4 d, const float* scores, const float* lms, int* s_flag,
                                           int* meta, float* rec) {
    if ((bk & 63) != lane) return;
    s_flag[bk] = F_START | F_MATCHED;
    float* r = rec + (size_t)bk * 16;
    r[0] = d.x; r[1] = d.y; r[2] = d.z; r[3] = d.w; r[4] = scores[(size_t)i * p.score_stride];
    for (int q = 0; q < 10; ++q) r[5 + q] = lms[(size_t)i * 10 + q];
    const int hits = meta[bk * 4 + 2];
    meta[bk * 4 + 2] = hits < (1 << 30) ? hits + 1 : (1 << 30);
    meta[bk * 4 + 3] = 0;
}

// WEAK = false is the plain tracker: one pass over every row, no score read in the loop, no F_CONF bit anywhere.  WEAK = true splits the
// rows by score > birth_score (a wave-uniform test: every lane reads the same score) and walks them twice.  A lane reads and writes only
// the flag words of its own slots in both passes, so the second pass needs no barrier either.
template <bool WEAK>
__global__ __launch_bounds__(64) void track_update_kernel(TrackParams p) {
    __shared__ float4 s_box[kTrackMaxSlots];      // start-of-update boxes (lane-owned words)
    __shared__ int s_flag[kTrackMaxSlots];
    __shared__ int s_new[kTrackMaxSlots];         // the first max_tracks new rows: no more can be born
    const int b = blockIdx.x, lane = threadIdx.x, M = p.max_tracks, per = (M + 63) >> 6;
    const size_t so = (size_t)(p.stream0 + b) * M;
    int* meta = p.meta + so * 4;
    float* rec = p.rec + so * 16;
    for (int j = 0; j < per; ++j) {
        const int k = j * 64 + lane;
        if (k >= M) continue;
        const int alive = meta[k * 4];
        int f = alive ? F_START : 0;
        if constexpr (WEAK) { if (alive && meta[k * 4 + 2] >= p.min_hits) f |= F_CONF; }
        s_flag[k] = f;
        if (alive) s_box[k] = *reinterpret_cast<const float4*>(rec + (size_t)k * 16);
    }
    const int cnt = p.counts[b];
    const int n = cnt < 0 ? 0 : cnt < p.rows ? cnt : p.rows;
    const float* boxes = p.boxes + (size_t)b * p.rows * 4;
    const float* scores = p.scores + (size_t)b * p.rows * p.score_stride;
    const float* lms = p.lms + (size_t)b * p.rows * 10;
    int n_new = 0, n_weak = 0;
    float bv;
    int bk;
    for (int i = 0; i < n; ++i) {
        const float4 d = *reinterpret_cast<const float4*>(boxes + (size_t)i * 4);
        if (!(isfinite(d.x) && isfinite(d.y) && isfinite(d.z) && isfinite(d.w))) continue;
        if constexpr (WEAK) { if (!(scores[(size_t)i * p.score_stride] > p.birth_score)) continue; }      // weak (a NaN too): the second pass
        track_best<WEAK ? ~F_CONF : ~0, F_START>(d, lane, M, per, s_flag, s_box, bv, bk);      // alive at the start, not yet matched
        if (bk != INT_MAX && bv >= p.iou_thresh) {
            track_take(p, lane, bk, i, d, scores, lms, s_flag, meta, rec);
        } else {
            if (lane == 0 && n_new < M) s_new[n_new] = i;
            ++n_new;
        }
    }
    if constexpr (WEAK) {
        for (int i = 0; i < n; ++i) {
            const float4 d = *reinterpret_cast<const float4*>(boxes + (size_t)i * 4);
            if (!(isfinite(d.x) && isfinite(d.y) && isfinite(d.z) && isfinite(d.w))) continue;
            if (scores[(size_t)i * p.score_stride] > p.birth_score) continue;
            track_best<~0, F_START | F_CONF>(d, lane, M, per, s_flag, s_box, bv, bk);      // confirmed at the start, matched by neither pass
            if (bk != INT_MAX && bv >= p.weak_iou) {
                track_take(p, lane, bk, i, d, scores, lms, s_flag, meta, rec);
                ++n_weak;
            }                                          // otherwise DISCARDED: never new, never born
        }
    }
    __syncthreads();                                   // s_new: written by lane 0, read by the owners of the free slots
    // age the unmatched, then give the free slots to the new rows in slot order
    const int next = p.next_id[p.stream0 + b];
    int base = 0;
    for (int j = 0; j < per; ++j) {
        const int k = j * 64 + lane;
        bool is_free = false;
        if (k < M) {
            const int f = WEAK ? s_flag[k] & ~F_CONF : s_flag[k];
            bool alive = (f & F_MATCHED) != 0;
            if (f == F_START) {
                const int hits = meta[k * 4 + 2], misses = meta[k * 4 + 3] + 1;
                alive = hits >= p.min_hits && misses <= p.max_age;
                if (alive) meta[k * 4 + 3] = misses; else meta[k * 4] = 0;
            }
            s_flag[k] = alive ? F_ALIVE : 0;
            is_free = !alive;
        }
        const unsigned long long bal = __ballot(is_free);
        const int r = base + __popcll(bal & ((1ull << lane) - 1ull));
        if (is_free && r < n_new) {
            const int i = s_new[r];                    // r < the free slots <= max_tracks: written
            float* q = rec + (size_t)k * 16;
            for (int c = 0; c < 4; ++c) q[c] = boxes[(size_t)i * 4 + c];
            q[4] = scores[(size_t)i * p.score_stride];
            for (int c = 0; c < 10; ++c) q[5 + c] = lms[(size_t)i * 10 + c];
            meta[k * 4] = 1; meta[k * 4 + 1] = next + r; meta[k * 4 + 2] = 1; meta[k * 4 + 3] = 0;
            s_flag[k] = F_ALIVE;
        }
        base += __popcll(bal);
    }
    if (lane == 0) {
        p.next_id[p.stream0 + b] = next + (n_new < base ? n_new : base);
        p.flags[b] = (n_new > base ? 1 : 0) | (WEAK && n_weak > 0 ? 2 : 0);
    }
    // the alive slots, compacted in slot order (every lane reads back only what it wrote itself): step 5, cf_trackemit.h
    const TrackRows o{p.dets + (size_t)b * M * 5, p.lms_out + (size_t)b * M * 10, p.info + (size_t)b * M * 3, p.corners + (size_t)b * M * 4};
    base = track_emit_rows(lane, M, p.hold_grow, meta, rec, o, [&](int k) { return s_flag[k] == F_ALIVE; }, [](int, int) {});
    if (lane == 0) p.out_counts[b] = base;
}

}  // namespace

const char* track_check(const cf_track_opts* o, int n_streams) {
    if (!o) return "null options";
    if (!std::isfinite(o->iou_thresh) || !(o->iou_thresh > 0.f) || !(o->iou_thresh <= 1.f)) return "iou_thresh must be finite and in (0, 1]";
    if (o->max_age < 0 || o->max_age > 1000) return "max_age must be in 0..1000";
    if (o->min_hits < 1 || o->min_hits > 1000) return "min_hits must be in 1..1000";
    if (o->max_tracks < 1 || o->max_tracks > kTrackMaxSlots) return "max_tracks must be in 1..1024";
    if (!std::isfinite(o->hold_grow) || !(o->hold_grow >= 0.f) || !(o->hold_grow <= 1.f)) return "hold_grow must be finite and in 0..1";
    if (n_streams < 1 || n_streams > kTrackMaxStreams) return "n_streams must be in 1..4096";
    return nullptr;
}

const char* track_weak_check(const cf_track_weak_opts* w) {
    if (!w) return nullptr;                            // no weak options: the plain tracker
    if (!std::isfinite(w->birth_score) || !(w->birth_score > 0.f) || !(w->birth_score <= 1.f)) return "birth_score must be finite and in (0, 1]";
    if (!std::isfinite(w->weak_iou) || !(w->weak_iou > 0.f) || !(w->weak_iou <= 1.f)) return "weak_iou must be finite and in (0, 1]";
    return nullptr;
}

hipError_t launch_track_update(hipStream_t s, const TrackParams& p) {
    if (p.B < 1 || p.rows < 1 || p.max_tracks < 1 || p.max_tracks > kTrackMaxSlots || p.stream0 < 0) return hipErrorInvalidValue;
    if (p.weak) hipLaunchKernelGGL(track_update_kernel<true>, dim3(p.B), dim3(64), 0, s, p);
    else hipLaunchKernelGGL(track_update_kernel<false>, dim3(p.B), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace cf
