// stream_box.hpp -- the box and wave helpers of the stream's one-wave-per-lane kernels, once: numpy's minimum / maximum,
// the IoU of the definition, the 2^-20 unit IoUs are counted in, the rank of a thread in a ballot and a ballot's first
// thread.  stream_track.hpp (the tracker) and stream_eval.hpp (the scorer, the identity step, HOTA) include it.
#pragma once
#include "common.hpp"

namespace dagr {

constexpr float kIouOne = 1048576.0f;               // an IoU in units of 2^-20

// numpy.minimum / numpy.maximum: a NaN operand comes back
__device__ __forceinline__ float np_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float np_max(float a, float b) { return (a > b || a != a) ? a : b; }

// TrackDefinition.iou, operation by operation: a is the row (the tracker) or the ground-truth box (the labelled step), b
// the track or the hypothesis
__device__ __forceinline__ float iou_xyxy(const float4 &a, const float4 &b) {
    const float iw = np_min(a.z, b.z) - np_max(a.x, b.x);
    const float ih = np_min(a.w, b.w) - np_max(a.y, b.y);
    const float inter = (iw > 0.0f && ih > 0.0f) ? iw * ih : 0.0f;
    const float uni = ((a.z - a.x) * (a.w - a.y) + (b.z - b.x) * (b.w - b.y)) - inter;
    return inter / uni;
}

__device__ __forceinline__ int lanes_below(uint64_t mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }
__device__ __forceinline__ int first_lane(uint64_t mask) { return __ffsll((unsigned long long)mask) - 1; }

}  // namespace dagr
