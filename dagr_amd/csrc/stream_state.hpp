// stream_state.hpp -- the caller-owned state of an event stream (dagr_stream_stage) and how it is carved, once:
// graph_build.hip (the staging entries, which write it) and stream_render.hip (dagr_stream_render, which reads the
// resident raw set) include it; include/dagr_hip.h documents what the entries do with it.
#pragma once
#include "common.hpp"

namespace dagr {

constexpr int kStreamLanes = 128;           // validate(): batch_size <= 127
constexpr int64_t kNever = INT64_MIN;       // t_ref / t_last of a lane that has none yet

struct StreamState {
    int32_t *hdr;       // [8]: 0 raw set holding the current window, 1 its event count, 2 events of the step being staged,
                        //      3 raw set that step reads
    int64_t *t_ref;     // [B]  reference instant of the last step
    int64_t *t_last;    // [B]  newest event ever pushed to the lane
    int32_t *seg;       // [2B] {start, count} of each lane's segment in the current set
    int32_t *plan;      // [5B] per lane {output start, count, first survivor, survivors, first new event kept}
    int64_t *t0, *t1;   // [cap] raw sets: timestamps,
    int32_t *xy0, *xy1; // [cap] pixels (x | y << 16, two int16),
    int8_t *p0, *p1;    // [cap] polarities
    size_t head_bytes;  // everything in front of the raw sets
};

inline size_t carve_stream(int B, int64_t cap, char *base, StreamState *st) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return base ? base + o : nullptr;
    };
    StreamState s;
    s.hdr = (int32_t *)take(8 * 4);
    s.t_ref = (int64_t *)take((size_t)B * 8);
    s.t_last = (int64_t *)take((size_t)B * 8);
    s.seg = (int32_t *)take((size_t)B * 2 * 4);
    s.plan = (int32_t *)take((size_t)B * 5 * 4);
    s.head_bytes = off;
    s.t0 = (int64_t *)take((size_t)cap * 8);
    s.t1 = (int64_t *)take((size_t)cap * 8);
    s.xy0 = (int32_t *)take((size_t)cap * 4);
    s.xy1 = (int32_t *)take((size_t)cap * 4);
    s.p0 = (int8_t *)take((size_t)cap);
    s.p1 = (int8_t *)take((size_t)cap);
    if (st) *st = s;
    return off;
}

}  // namespace dagr
