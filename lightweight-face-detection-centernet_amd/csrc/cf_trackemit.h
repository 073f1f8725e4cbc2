// Step 5 of the tracker's statement (cf_track.hip), shared by the update kernel and the follower's emit launch (cf_follow.hip): the alive
// slots of one stream become its output rows, compacted in ascending slot order by ONE wave.  Lane l owns the slots j * 64 + l; the rank
// of a slot is a prefix sum, one ballot per 64 slots plus a running base, in slot order because slot = j * 64 + lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace cf {

// the output rows of one stream (device): dets [max_tracks][5], lms [.][10], info [.][3] = id, hits, misses, corners [.][4]
struct TrackRows { float* dets; float* lms; int* info; float* corners; };

// meta [max_tracks][4] = alive, id, hits, misses and rec [max_tracks][16] = box, score, lms[10], 0 of the stream; alive(k) says whether slot
// k < M is an output row, also(r, k) runs for every row r = the rank of slot k (more columns in the same row order).  A held box
// (misses > 0) is grown about its centre in float64 in the stated order.  Returns the number of rows, in every lane.
template <class Alive, class Also>
__device__ inline int track_emit_rows(int lane, int M, float hold_grow, const int* meta, const float* rec, const TrackRows& o, Alive alive, Also also) {
    const int per = (M + 63) >> 6;
    int base = 0;
    for (int j = 0; j < per; ++j) {
        const int k = j * 64 + lane;
        const bool on = k < M && alive(k);
        const unsigned long long bal = __ballot(on);
        if (on) {
            const int r = base + __popcll(bal & ((1ull << lane) - 1ull));
            const float* q = rec + (size_t)k * 16;
            const int misses = meta[k * 4 + 3];
            float x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
            if (misses > 0) {
                const double g = 1.0 + (double)hold_grow * (double)misses;
                const double cx = ((double)x1 + (double)x2) * 0.5, hw = ((double)x2 - (double)x1) * 0.5 * g;
                const double cy = ((double)y1 + (double)y2) * 0.5, hh = ((double)y2 - (double)y1) * 0.5 * g;
                x1 = (float)(cx - hw); x2 = (float)(cx + hw); y1 = (float)(cy - hh); y2 = (float)(cy + hh);
            }
            float* od = o.dets + (size_t)r * 5;
            od[0] = x1; od[1] = y1; od[2] = x2; od[3] = y2; od[4] = q[4];
            float* oc = o.corners + (size_t)r * 4;
            oc[0] = x1; oc[1] = y1; oc[2] = x2; oc[3] = y2;
            for (int c = 0; c < 10; ++c) o.lms[(size_t)r * 10 + c] = q[5 + c];
            o.info[r * 3] = meta[k * 4 + 1]; o.info[r * 3 + 1] = meta[k * 4 + 2]; o.info[r * 3 + 2] = misses;
            also(r, k);
        }
        base += __popcll(bal);
    }
    return base;
}

}  // namespace cf
