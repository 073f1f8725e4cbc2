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
// CONSTANT VELOCITY (cf_track_create_ex / cf_op_track_ex; tests/motion_cases.py restates it).  A tracker created with gain, finite, in
// (0, 1], and damp, finite, in [0, 1], holds per slot vel = (vx, vy) in float32 beside the record.  All new arithmetic is float32, every
// operation rounded, no FMA contraction (this file is built with -ffp-contract=off).  One update of a stream becomes
//   1'. Skip.  Step 1 as it is; in addition a row with a corner of magnitude above 16777216 (2^24) is skipped too.  This keeps every later
//       quantity finite.
//   P.  Predict.  For every slot alive when the update began, with stored box o and velocity v: P = (o.x1 + vx, o.y1 + vy, o.x2 + vx,
//       o.y2 + vy).
//   2'. Match.  Steps 2, 2a and 2b measure the IoU of P and the row, not of the stored box and the row; the measure, the arg-max, the tie
//       rule, the NaN rule, the thresholds and the eligibility (including "confirmed when the update began") are unchanged.  A winner takes
//       the row's box d, score and landmarks as they are.  Its velocity is updated from the values BEFORE the take -- the stored box o,
//       g = misses, hb = hits:
//         cdx = (d.x1 + d.x2) * 0.5f;  cox = (o.x1 + o.x2) * 0.5f;  rx = (cdx - cox) - vx;
//         a = hb == 1 ? 1.0f : gain;   vx' = vx + a * (rx / (float)(g + 1));        y likewise
//       hb == 1 is the track's second sighting: its velocity is still the 0 of birth, so the first measured displacement is taken whole.
//   3'. Age.  Freeing tentative tracks and counting misses are unchanged.  A slot that stays alive unmatched (a held track) COASTS: every x
//       of its box and of its ten landmarks becomes x + vx, every y becomes y + vy; then vel = (vx * damp, vy * damp).  If a coasted
//       corner's magnitude exceeds 2^24 the slot is freed instead.
//       Follower records: if the tracker has follower records, and the slot's tpl_id == id, and tpl_box equals the box before the coast bit
//       for bit, then tpl_box takes the coasted box: the next cf_track_follow FOLLOWS from the coasted place with the template of the
//       last detection (without this write it would LEARN whatever stands there).
//   4'. Birth.  As it is, with vel = (0, 0): a reused slot never inherits a velocity.
//   5.  Output.  Unchanged: the held row is the coasted box, grown by hold_grow, with its landmarks coasted with it.
// Consequences: cf_track_follow leaves vel alone; it still LEARNS behind any match, because the box changed, and behind a coast it now follows
// about the predicted centre.  With the follower running between updates, v is the motion per update that the follower has not already
// put into the box.  Lookback, best shots, redact, blur, draw and chips take the rows unchanged.  cf_track_reset and a scene cut need no
// word about velocities, because birth zeroes them.  Device state per slot becomes 88 bytes for a motion tracker.
// Limits: the model cannot bootstrap -- a face so fast that its SECOND sighting misses iou_thresh against the unpredicted box is reborn
// every frame, as before.  Only the centre moves; size is not predicted.  A wrong match yields a wrong velocity for a few frames.  Coasting
// at damp = 1 carries a held box max_age * v away.  gain = 0.5 and damp = 1.0 (SORT's coast) are this project's choices: there is no
// labelled video here, nobody has measured them, and no accuracy claim is made.
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
// A motion tracker is a second template parameter, four instances in all; the two without it are what they were (no velocity pointer read,
// no new branch).  In the motion instances s_box holds P.  The owner lane of a winning slot reads o, g and hb from the global state before
// it overwrites them (a slot is matched at most once per update, so they are still the start-of-update values); the coast runs in the
// ageing loop on lane-owned slots; the velocities of the output rows go out through step 5's per-row hook.  No new barrier, no atomics,
// no new LDS.
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

// (motion trackers) a corner beyond 2^24 in magnitude: such a row is skipped, such a coasted slot is freed
constexpr float kTrackFar = 16777216.0f;
__device__ __forceinline__ bool track_far(const float4 d) {
    return fabsf(d.x) > kTrackFar || fabsf(d.y) > kTrackFar || fabsf(d.z) > kTrackFar || fabsf(d.w) > kTrackFar;
}

// (motion trackers) The owner of the winning slot bk, BEFORE track_take: the slot's velocity from the row's box d and the stored box, misses
// and hits as the update found them.
__device__ __forceinline__ void track_learn(const TrackParams& p, int lane, int bk, const float4 d, const int* meta, const float* rec, float* vel) {
    if ((bk & 63) != lane) return;
    const float* o = rec + (size_t)bk * 16;
    const float a = meta[bk * 4 + 2] == 1 ? 1.0f : p.gain, n = (float)(meta[bk * 4 + 3] + 1);
    const float vx = vel[bk * 2], vy = vel[bk * 2 + 1];
    const float cdx = (d.x + d.z) * 0.5f, cox = (o[0] + o[2]) * 0.5f, rx = (cdx - cox) - vx;
    const float cdy = (d.y + d.w) * 0.5f, coy = (o[1] + o[3]) * 0.5f, ry = (cdy - coy) - vy;
    vel[bk * 2] = vx + a * (rx / n);
    vel[bk * 2 + 1] = vy + a * (ry / n);
}

// (motion trackers) The owner of the held slot k coasts it: box and landmarks by vel, vel by damp, and the follower's tpl_box (tm: the
// stream's follower records or nullptr) along with the box it described.  false, and nothing written: a corner went beyond 2^24.
__device__ __forceinline__ bool track_coast(const TrackParams& p, int k, const int* meta, float* rec, float* vel, int* tm) {
    float* q = rec + (size_t)k * 16;
    const float vx = vel[k * 2], vy = vel[k * 2 + 1];
    const float4 o = make_float4(q[0], q[1], q[2], q[3]);
    const float4 c = make_float4(o.x + vx, o.y + vy, o.z + vx, o.w + vy);
    if (track_far(c)) return false;
    q[0] = c.x; q[1] = c.y; q[2] = c.z; q[3] = c.w;
    for (int i = 0; i < 10; ++i) q[5 + i] = q[5 + i] + ((i & 1) ? vy : vx);
    vel[k * 2] = vx * p.damp;
    vel[k * 2 + 1] = vy * p.damp;
    if (tm) {
        int* t = tm + (size_t)k * 6;
        if (t[1] == meta[k * 4 + 1] && t[2] == __float_as_int(o.x) && t[3] == __float_as_int(o.y) && t[4] == __float_as_int(o.z) && t[5] == __float_as_int(o.w)) {
            t[2] = __float_as_int(c.x); t[3] = __float_as_int(c.y); t[4] = __float_as_int(c.z); t[5] = __float_as_int(c.w);
        }
    }
    return true;
}

// WEAK = false is the plain tracker: one pass over every row, no score read in the loop, no F_CONF bit anywhere.  WEAK = true splits the
// rows by score > birth_score (a wave-uniform test: every lane reads the same score) and walks them twice.  A lane reads and writes only
// the flag words of its own slots in both passes, so the second pass needs no barrier either.  MOTION = true is "constant velocity" above;
// every line of it stands under an `if constexpr (MOTION)`.
template <bool WEAK, bool MOTION>
__global__ __launch_bounds__(64) void track_update_kernel(TrackParams p) {
    __shared__ float4 s_box[kTrackMaxSlots];      // start-of-update boxes (lane-owned words)
    __shared__ int s_flag[kTrackMaxSlots];
    __shared__ int s_new[kTrackMaxSlots];         // the first max_tracks new rows: no more can be born
    const int b = blockIdx.x, lane = threadIdx.x, M = p.max_tracks, per = (M + 63) >> 6;
    const size_t so = (size_t)(p.stream0 + b) * M;
    int* meta = p.meta + so * 4;
    float* rec = p.rec + so * 16;
    float* vel = nullptr;
    if constexpr (MOTION) vel = p.vel + so * 2;
    for (int j = 0; j < per; ++j) {
        const int k = j * 64 + lane;
        if (k >= M) continue;
        const int alive = meta[k * 4];
        int f = alive ? F_START : 0;
        if constexpr (WEAK) { if (alive && meta[k * 4 + 2] >= p.min_hits) f |= F_CONF; }
        s_flag[k] = f;
        if (alive) s_box[k] = *reinterpret_cast<const float4*>(rec + (size_t)k * 16);
        if constexpr (MOTION) {
            if (alive) {                               // P: the box where the face is expected
                const float4 o = s_box[k];
                const float vx = vel[k * 2], vy = vel[k * 2 + 1];
                s_box[k] = make_float4(o.x + vx, o.y + vy, o.z + vx, o.w + vy);
            }
        }
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
        if constexpr (MOTION) { if (track_far(d)) continue; }
        if constexpr (WEAK) { if (!(scores[(size_t)i * p.score_stride] > p.birth_score)) continue; }      // weak (a NaN too): the second pass
        track_best<WEAK ? ~F_CONF : ~0, F_START>(d, lane, M, per, s_flag, s_box, bv, bk);      // alive at the start, not yet matched
        if (bk != INT_MAX && bv >= p.iou_thresh) {
            if constexpr (MOTION) track_learn(p, lane, bk, d, meta, rec, vel);
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
            if constexpr (MOTION) { if (track_far(d)) continue; }
            if (scores[(size_t)i * p.score_stride] > p.birth_score) continue;
            track_best<~0, F_START | F_CONF>(d, lane, M, per, s_flag, s_box, bv, bk);      // confirmed at the start, matched by neither pass
            if (bk != INT_MAX && bv >= p.weak_iou) {
                if constexpr (MOTION) track_learn(p, lane, bk, d, meta, rec, vel);
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
                if constexpr (MOTION) { if (alive) alive = track_coast(p, k, meta, rec, vel, p.tmeta ? p.tmeta + so * 6 : nullptr); }
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
            if constexpr (MOTION) { vel[k * 2] = 0.0f; vel[k * 2 + 1] = 0.0f; }
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
    if constexpr (MOTION) {
        float* vo = p.vel_out ? p.vel_out + (size_t)b * M * 2 : nullptr;
        base = track_emit_rows(lane, M, p.hold_grow, meta, rec, o, [&](int k) { return s_flag[k] == F_ALIVE; }, [&](int r, int k) {
            if (vo) { vo[(size_t)r * 2] = vel[k * 2]; vo[(size_t)r * 2 + 1] = vel[k * 2 + 1]; }
        });
    } else
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

const char* track_motion_check(const cf_track_motion_opts* m) {
    if (!m) return nullptr;                            // no motion options: the tracker without velocities
    if (!std::isfinite(m->gain) || !(m->gain > 0.f) || !(m->gain <= 1.f)) return "gain must be finite and in (0, 1]";
    if (!std::isfinite(m->damp) || !(m->damp >= 0.f) || !(m->damp <= 1.f)) return "damp must be finite and in [0, 1]";
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
    if (p.motion && !p.vel) return hipErrorInvalidValue;
    if (p.motion && p.weak) hipLaunchKernelGGL((track_update_kernel<true, true>), dim3(p.B), dim3(64), 0, s, p);
    else if (p.motion) hipLaunchKernelGGL((track_update_kernel<false, true>), dim3(p.B), dim3(64), 0, s, p);
    else if (p.weak) hipLaunchKernelGGL((track_update_kernel<true, false>), dim3(p.B), dim3(64), 0, s, p);
    else hipLaunchKernelGGL((track_update_kernel<false, false>), dim3(p.B), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace cf
