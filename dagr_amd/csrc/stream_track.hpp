// stream_track.hpp -- what the stream tracker's kernels share and what has no bearing on their instruction streams: the
// caller-owned state and how it is carved, the box and wave helpers of stream_box.hpp, and the outputs only the motion
// model has.  stream_track.hip (the greedy entries) and stream_track_optimal.hip
// (dagr_stream_track_optimal) include it; include/dagr_hip.h documents the layouts.
#pragma once
#include "stream_box.hpp"

namespace dagr {

// The caller-owned state, as include/dagr_hip.h documents it: five arrays over [B, max_tracks] -- six with the motion
// model, whose layout has `vel` behind `box` -- and next_id[B].
struct Tracks {
    int64_t *id;        // 0: the slot is free
    int64_t *t_last;
    float4 *box;
    int32_t *label, *hits;
    int64_t *next_id;
    float4 *vel;        // the motion layout only; last, with what else only the motion model has: see k_stream_track
};

inline size_t carve_tracks(bool motion, int B, int M, char *base, Tracks *out) {
    const size_t n = (size_t)B * M;
    const size_t after_box = (motion ? 48 : 32) * n;
    Tracks t;
    t.id = (int64_t *)base;
    t.t_last = (int64_t *)(base + 8 * n);
    t.box = (float4 *)(base + 16 * n);
    t.vel = motion ? (float4 *)(base + 32 * n) : nullptr;
    t.label = (int32_t *)(base + after_box);
    t.hits = (int32_t *)(base + after_box + 4 * n);
    t.next_id = (int64_t *)(base + after_box + 8 * n);
    if (out) *out = t;
    return after_box + 8 * n + 8 * (size_t)B;
}

// what a step with the motion model leaves besides ids and hits: the filtered box and the velocity of every row, and the
// lane's coast list.  Without the model all of it is NULL and nothing reads it.
struct MotionOut {
    float4 *track_box, *track_vel;      // [B, A]
    int64_t *coast_id;                  // [B, max_tracks]; NULL with the four below: no coast list
    float4 *coast_box;
    int32_t *coast_label;
    int64_t *coast_age;
    int32_t *n_coast;                   // [B]
};

}  // namespace dagr
