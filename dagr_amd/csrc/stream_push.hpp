// stream_push.hpp -- the keyed push, stated once for the stream's three push stages (downsample.hip, stream_denoise.hip,
// stream_flicker.hip).  Each stage keys the events of a push by (lane, pixel or cell), sorts (uint32 key, int32 arrival
// index) pairs with the library's stable radix sort, decides every event in a kernel of its own, scans the keep flags with
// the project's chained scan and compacts the survivors in arrival order.  What differs between the stages is their maps,
// their decision kernel and what their last launch counts; everything else is here: the carving of the scratch behind a
// stage's maps, the size and argument checks, the key of an event, the sort, the two halves of the compaction and the
// dispatch on the lane type.  The kernels themselves stay in the stages' files, under their own names.
#pragma once
#include "common.hpp"

#include <algorithm>
#include <string>
#include <rocprim/device/device_radix_sort.hpp>

namespace dagr {

// bits that hold every key up to and including `sentinel`
inline int key_bits(int64_t sentinel) {
    int bits = 1;
    while (bits < 32 && (sentinel >> bits) != 0) ++bits;
    return bits;
}

// the sort's temporary storage for a push of n events (0 if the library cannot say, e.g. without a device)
inline size_t sort_tmp_bytes(int64_t n, int bits) {
    size_t bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr,
                                  (int32_t *)nullptr, (size_t)n, 0u, (unsigned)bits, (hipStream_t)0) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return bytes;
}

// ... for every push of up to max_push events (at least 256 bytes).  The library picks its algorithm by size, so the
// largest push need not ask for the most: max_push and every power of two below it.
inline size_t sort_tmp_bytes_upto(int64_t max_push, int bits) {
    size_t bytes = 256;
    for (int64_t n = max_push; n >= 1; n = (n & (n - 1)) ? (int64_t)1 << (63 - __builtin_clzll((unsigned long long)n)) : n / 2)
        bytes = std::max(bytes, sort_tmp_bytes(n, bits));
    return bytes;
}

// ---------------------------------------------------------------------------------------------
// The state.  A stage's caller-owned state holds the stage's maps first (offset 0), then the scratch of a largest push.

// Arrays one behind the other, each at the next multiple of 256 bytes; without a base it only measures.
struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(void *base_) : base((char *)base_) {}
    template <typename T = void>
    T *take(size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return (T *)(base ? base + o : nullptr);
    }
};

// The scratch, in the order the state holds it.
struct PushScratch {
    void *scan_state;               // the chained scan's look-back state: zero before the first push
    size_t scan_bytes;
    uint32_t *key_in, *key_out;     // [max_push] keys in arrival order / sorted
    int32_t *idx_in, *idx_out;      // [max_push] arrival indices in arrival order / sorted by key, ascending inside a key
    int32_t *flag, *offs;           // [max_push] keep flags in arrival order and their exclusive prefix sum
    void *extra;                    // [extra_bytes] a stage's own per-event array (the flicker stage's outcomes)
    void *sort_tmp;
    size_t sort_tmp_bytes, tmp_offset;
    size_t end;                     // where the sort's storage ends: measuring, what dagr_stream_*_bytes returns
};

// The scratch behind the maps `c` has carved.  Measuring (no base), the sort's storage is sized for every push up to
// max_push; on a caller's state of state_bytes it is what the state has left behind tmp_offset (0: the state ends before).
inline PushScratch carve_push(Carver &c, int64_t max_push, int64_t sentinel, size_t state_bytes, size_t extra_bytes = 0) {
    PushScratch s;
    s.scan_bytes = scan_chained_state_bytes(max_push);
    s.scan_state = c.take(s.scan_bytes);
    s.key_in = c.take<uint32_t>((size_t)max_push * 4);
    s.key_out = c.take<uint32_t>((size_t)max_push * 4);
    s.idx_in = c.take<int32_t>((size_t)max_push * 4);
    s.idx_out = c.take<int32_t>((size_t)max_push * 4);
    s.flag = c.take<int32_t>((size_t)max_push * 4);
    s.offs = c.take<int32_t>((size_t)max_push * 4);
    s.extra = extra_bytes ? c.take(extra_bytes) : nullptr;
    s.tmp_offset = c.off;
    s.sort_tmp_bytes = !c.base ? sort_tmp_bytes_upto(max_push, key_bits(sentinel))
                               : state_bytes > s.tmp_offset ? state_bytes - s.tmp_offset : 0;
    s.sort_tmp = c.take(s.sort_tmp_bytes);
    s.end = c.off;
    return s;
}

// a caller's state reaches at least 256 bytes into the sort's storage (the least dagr_stream_*_bytes returns)
inline bool push_state_holds(const PushScratch &s) { return s.sort_tmp_bytes >= 256; }

// The sizes of a stage whose keys are the pixels of a sensor (the two filters; the front bounds its cells itself).
inline bool push_sizes_ok(int32_t B, int32_t sensor_w, int32_t sensor_h, int64_t max_push) {
    return B >= 1 && B < 128 && sensor_w >= 1 && sensor_h >= 1 && sensor_w <= 32767 && sensor_h <= 32767 && max_push >= 1 &&
           max_push < (1ll << 31) / 64 && (int64_t)B * sensor_w * sensor_h < (1ll << 31);
}

// What every push must satisfy, whatever the stage: the complaint, under the stage's prefix, or nothing.
inline std::string push_args_complaint(const char *prefix, const void *state, const void *n_out, const void *status,
                                       int64_t n_raw, int64_t max_push, const void *xy_raw, const void *t_raw,
                                       const void *p_raw, const void *batch_raw, const void *xy_out, const void *t_out,
                                       const void *p_out, const void *batch_out) {
    const char *what = nullptr;
    if (!(state && n_out && status)) what = "NULL pointer";
    else if (!(n_raw >= 0 && n_raw <= max_push)) what = "max_push < n_raw";
    else if (!(n_raw == 0 || (xy_raw && t_raw && p_raw && batch_raw && xy_out && t_out && p_out && batch_out)))
        what = "NULL input or output";
    else if (((uintptr_t)xy_raw & 3) != 0 || ((uintptr_t)xy_out & 3) != 0) what = "xy must be 4-byte aligned";
    return what ? std::string(prefix) + ": " + what : std::string();
}

// f(batch) with the lanes of a push under their type
template <typename F>
inline void with_batch(const void *batch, int32_t batch_is_int64, F &&f) {
    if (batch_is_int64) f((const int64_t *)batch);
    else f((const int32_t *)batch);
}

// The sort, in two steps around the stage's keys launch so that a refusal launches nothing: whether the state holds the
// storage the library asks for for n pairs (a query that fails asks for 0: the sort then reports the failure itself) ...
inline bool sort_push_fits(const PushScratch &s, int n, int bits) { return sort_tmp_bytes(n, bits) <= s.sort_tmp_bytes; }

// ... and the sort of (key_in, idx_in) into (key_out, idx_out)
inline hipError_t sort_push(const PushScratch &s, int n, int bits, hipStream_t stream) {
    size_t tmp = s.sort_tmp_bytes;
    return rocprim::radix_sort_pairs(s.sort_tmp, tmp, s.key_in, s.key_out, s.idx_in, s.idx_out, (size_t)n, 0u, (unsigned)bits,
                                     stream);
}

// ---------------------------------------------------------------------------------------------
// The device stages: each is the body of one thread of a stage's kernel.

// Launch 1, event i: its key lane * grid + gy * grid_w + gx over a grid_w x grid_h grid of fx x fy pixel cells (1 x 1: the
// pixels themselves), and its arrival index.  An event outside the sensor (status bit 4), beyond the grid (the strip right
// of / below the last whole cell) or with a lane outside [0, B) gets the sentinel key B * grid: it sorts behind every key
// and meets no state.  flag_lane_less: an outside event raises the status bit whatever its lane; else only with a lane of
// the stream's (the flicker stage, whose lane-less rows are the stage in front's).
template <typename BatchT>
__device__ __forceinline__ void push_key(const int32_t *__restrict__ xy, const BatchT *__restrict__ batch, int i, int B,
                                         int sensor_w, int sensor_h, int fx, int fy, int grid_w, int grid_h,
                                         bool flag_lane_less, uint32_t *__restrict__ key, int32_t *__restrict__ idx,
                                         int32_t *__restrict__ status) {
    const int32_t v = xy[i];
    const int x = (int16_t)(v & 0xffff), y = (int16_t)(v >> 16);
    const int64_t b = (int64_t)batch[i];
    const bool lane_ok = b >= 0 && b < B;
    const bool outside = x < 0 || x >= sensor_w || y < 0 || y >= sensor_h;
    if (outside && (flag_lane_less || lane_ok)) atomicOr(status, 16);
    const int gx = outside ? 0 : x / fx, gy = outside ? 0 : y / fy;
    const uint32_t grid = (uint32_t)grid_w * (uint32_t)grid_h;
    const bool none = outside || gx >= grid_w || gy >= grid_h || !lane_ok;
    key[i] = none ? (uint32_t)B * grid : (uint32_t)b * grid + (uint32_t)(gy * grid_w + gx);
    idx[i] = i;
}

// Launch 5 (after the scan), first half, event i: a survivor goes to row offs[i], at its cell's coordinates (fx = fy = 1:
// its own).
template <typename BatchT>
__device__ __forceinline__ void push_survivor(int i, const int32_t *__restrict__ flag, const int32_t *__restrict__ offs,
                                              const int32_t *__restrict__ xy, const int64_t *__restrict__ t,
                                              const int8_t *__restrict__ p, const BatchT *__restrict__ batch, int fx, int fy,
                                              int32_t *__restrict__ xy_out, int64_t *__restrict__ t_out,
                                              int8_t *__restrict__ p_out, int32_t *__restrict__ batch_out) {
    const int keep = flag[i], j = offs[i];
    if (!keep || j < 0 || j > i) return;
    const int32_t v = xy[i];
    const int x = (int16_t)(v & 0xffff) / fx, y = (int16_t)(v >> 16) / fy;
    xy_out[j] = (x & 0xffff) | (y << 16);
    t_out[j] = t[i];
    p_out[j] = p[i];
    batch_out[j] = (int32_t)batch[i];
}

// the survivors of a push of n events, from the scan's last entry
__device__ __forceinline__ int push_total(const int32_t *__restrict__ flag, const int32_t *__restrict__ offs, int n) {
    return min(max(offs[n - 1] + flag[n - 1], 0), n);
}

// Launch 5, second half, row i < n (the two filters; the front's consumer takes the count from the device): the rows from the
// count up get lane -1 at pixel (0, 0), which a consumer without a device-side count drops silently; the last writes n_out.
__device__ __forceinline__ void push_tail(int i, int n, int total, int32_t *__restrict__ xy_out,
                                          int32_t *__restrict__ batch_out, int32_t *__restrict__ n_out) {
    if (i == n - 1) *n_out = total;
    if (i >= total) {
        xy_out[i] = 0;
        batch_out[i] = -1;
    }
}

}  // namespace dagr
