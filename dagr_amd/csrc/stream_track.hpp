// stream_track.hpp -- what the stream tracker's kernels share and what has no bearing on their instruction streams: the
// caller-owned state and how it is carved, numpy's minimum / maximum, the IoU of the definition, the rank of a thread in a
// ballot, and the outputs only the motion model has.  stream_track.hip (the greedy entries) and stream_track_optimal.hip
// (dagr_stream_track_optimal) include it; include/dagr_hip.h documents the layouts.
#pragma once
#include "common.hpp"

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

// numpy.minimum / numpy.maximum: a NaN operand comes back
__device__ __forceinline__ float np_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float np_max(float a, float b) { return (a > b || a != a) ? a : b; }

// TrackDefinition.iou, operation by operation: a is the row, b the track
__device__ __forceinline__ float iou_xyxy(const float4 &a, const float4 &b) {
    const float iw = np_min(a.z, b.z) - np_max(a.x, b.x);
    const float ih = np_min(a.w, b.w) - np_max(a.y, b.y);
    const float inter = (iw > 0.0f && ih > 0.0f) ? iw * ih : 0.0f;
    const float uni = ((a.z - a.x) * (a.w - a.y) + (b.z - b.x) * (b.w - b.y)) - inter;
    return inter / uni;
}

__device__ __forceinline__ int lanes_below(uint64_t mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

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
