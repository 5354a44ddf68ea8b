// stream_denoise.hip -- the event stream's noise filter (dagr_stream_denoise): a background-activity filter and a
// refractory filter on a raw push, in front of dagr_stream_downsample / dagr_stream_stage_dev.
//
// Every lane owns a stamp map int64 [sensor_h, sensor_w]: the timestamp of the last event on every pixel, kept or not
// ("never" = INT64_MIN).  An event is supported if one of its 8 neighbours has a stamp at most denoise_us old, refractory if
// its own pixel has a stamp less than refractory_us old, and kept iff supported and not refractory; then it stamps its
// pixel.  Every event stamps, so a decision depends on the timestamps of earlier events only, never on earlier decisions:
// one thread per event.  The events are sorted by pixel key (lane, y, x) with the arrival index as payload (a stable radix
// sort: the arrival index ascends inside a run); the latest earlier event of a pixel is then a binary search away, and
// where the push has none the carried stamp applies.  The stamps are written in a later launch than the one that reads
// them.  Keep flags, the project's chained scan, an order-preserving compaction: a keyed push (stream_push.hpp).
#include "common.hpp"
#include "stream_push.hpp"

namespace dagr {
namespace {

constexpr int64_t kNever = INT64_MIN;

// Caller-owned state: the lanes' stamp maps first (offset 0, int64 [B, sensor_h, sensor_w]), then the push's scratch.
struct Denoise {
    int64_t *stamps;
    PushScratch s;
};

Denoise carve_denoise(int B, int64_t pixels, int64_t max_push, void *base, size_t state_bytes) {
    Carver c(base);
    Denoise f;
    f.stamps = c.take<int64_t>((size_t)B * pixels * 8);
    f.s = carve_push(c, max_push, (int64_t)B * pixels, state_bytes);
    return f;
}

__global__ __launch_bounds__(kBlock) void k_denoise_never(int64_t *__restrict__ stamps, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) stamps[i] = kNever;
}

// Launch 1: the key of every event over the sensor's pixels, lane * pixels + y * sensor_w + x (push_key).  An event with
// the sentinel key is never kept and never stamps; dagr_stream_stage_dev flags a lane outside [0, B).
template <typename BatchT>
__global__ __launch_bounds__(kBlock) void k_denoise_keys(const int32_t *__restrict__ xy, const BatchT *__restrict__ batch, int n,
                                                        int B, int sensor_w, int sensor_h, uint32_t *__restrict__ key,
                                                        int32_t *__restrict__ idx, int32_t *__restrict__ status) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    push_key(xy, batch, i, B, sensor_w, sensor_h, 1, 1, sensor_w, sensor_h, true, key, idx, status);
}

// The stamp pixel `want` shows to the event with arrival index `me`: the t of the last sorted position whose
// (key, arrival index) is below (want, me) if that position holds `want`, else the carried stamp.
__device__ __forceinline__ int64_t stamp_before(const uint32_t *__restrict__ key, const int32_t *__restrict__ idx, int n,
                                                uint32_t want, int me, const int64_t *__restrict__ t, int64_t carried) {
    int lo = 0, hi = n;                 // first position with (key, idx) >= (want, me)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t k = key[mid];
        if (k < want || (k == want && idx[mid] < me)) lo = mid + 1;
        else hi = mid;
    }
    if (lo > 0 && key[lo - 1] == want) {
        const int e = idx[lo - 1];
        if (e >= 0 && e < n) return t[e];
    }
    return carried;
}

// Launch 3 (after the sort): one thread per sorted position decides its event.  Reads the stamp maps, writes none.
__global__ __launch_bounds__(kBlock) void k_denoise_decide(const uint32_t *__restrict__ key, const int32_t *__restrict__ idx,
                                                          int n, uint32_t sentinel, int sensor_w, int sensor_h,
                                                          const int64_t *__restrict__ t, int64_t denoise_us,
                                                          int64_t refractory_us, const int64_t *__restrict__ stamps,
                                                          int32_t *__restrict__ flag) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const uint32_t mine = key[k];
    const int me = min(max(idx[k], 0), n - 1);
    if (mine >= sentinel) {
        flag[me] = 0;
        return;
    }
    const int64_t now = t[me];
    bool keep = true;
    if (refractory_us > 0) {            // the predecessor on the event's own pixel: the previous sorted position, or the map
        int64_t s = stamps[mine];
        if (k > 0 && key[k - 1] == mine) s = t[min(max(idx[k - 1], 0), n - 1)];
        keep = !(s != kNever && now - s < refractory_us);
    }
    if (keep && denoise_us > 0) {
        const uint32_t pixels = (uint32_t)sensor_w * (uint32_t)sensor_h;
        const int pix = (int)(mine % pixels);
        const int x = pix % sensor_w, y = pix / sensor_w;
        bool supported = false;
        // a carried stamp that supports is enough: an event of the push on that pixel could only be newer
        for (int d = 0; d < 9 && !supported; ++d) {
            const int nx = x + d % 3 - 1, ny = y + d / 3 - 1;
            if (d == 4 || nx < 0 || nx >= sensor_w || ny < 0 || ny >= sensor_h) continue;
            const int64_t s = stamps[(int64_t)mine + (ny - y) * sensor_w + (nx - x)];
            supported = s != kNever && now - s <= denoise_us;
        }
        for (int d = 0; d < 9 && !supported; ++d) {
            const int nx = x + d % 3 - 1, ny = y + d / 3 - 1;
            if (d == 4 || nx < 0 || nx >= sensor_w || ny < 0 || ny >= sensor_h) continue;
            const uint32_t want = (uint32_t)((int64_t)mine + (ny - y) * sensor_w + (nx - x));
            const int64_t s = stamp_before(key, idx, n, want, me, t, kNever);
            supported = s != kNever && now - s <= denoise_us;
        }
        keep = supported;
    }
    flag[me] = keep ? 1 : 0;
}

// Launch 5 (after the scan), three jobs over one index:
//   arrival index i: the survivors in arrival order and their count; the rows from the count up to n get lane -1 at pixel
//     (0, 0), which a consumer without a device-side count (dagr_stream_downsample) drops silently;
//   sorted position i: the last event of a run stamps its pixel -- every decision has been read by now;
//   lane i: the events of the lane that were inside the sensor and not kept are added to lane_filtered[i], by this thread
//     alone.  The lane's arrival range comes from the sorted batch, its in-sensor events from the sorted keys.
template <typename BatchT>
__global__ __launch_bounds__(kBlock) void k_denoise_finish(const int32_t *__restrict__ flag, const int32_t *__restrict__ offs,
                                                          int n, const uint32_t *__restrict__ key,
                                                          const int32_t *__restrict__ idx, uint32_t sentinel, int B,
                                                          uint32_t pixels, const int32_t *__restrict__ xy,
                                                          const int64_t *__restrict__ t, const int8_t *__restrict__ p,
                                                          const BatchT *__restrict__ batch, int64_t *__restrict__ stamps,
                                                          int32_t *__restrict__ xy_out, int64_t *__restrict__ t_out,
                                                          int8_t *__restrict__ p_out, int32_t *__restrict__ batch_out,
                                                          int32_t *__restrict__ n_out, int64_t *__restrict__ lane_filtered) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int total = push_total(flag, offs, n);
    if (i < n) {
        push_survivor(i, flag, offs, xy, t, p, batch, 1, 1, xy_out, t_out, p_out, batch_out);
        push_tail(i, n, total, xy_out, batch_out, n_out);
        const uint32_t mine = key[i];
        if (mine < sentinel && (i == n - 1 || key[i + 1] != mine)) stamps[mine] = t[min(max(idx[i], 0), n - 1)];
    }
    if (i < B && lane_filtered) {
        auto first_lane = [&](int64_t lane) {          // first arrival index whose lane is >= `lane`
            int lo = 0, hi = n;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((uint64_t)(int64_t)batch[mid] < (uint64_t)lane) lo = mid + 1;   // (a lane-less row, -1, sorts last)
                else hi = mid;
            }
            return lo;
        };
        auto first_key = [&](uint32_t want) {           // first sorted position whose key is >= `want`
            int lo = 0, hi = n;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (key[mid] < want) lo = mid + 1;
                else hi = mid;
            }
            return lo;
        };
        auto kept_before = [&](int a) { return a >= n ? total : offs[a]; };
        const int a0 = first_lane(i), a1 = first_lane((int64_t)i + 1);
        const int kept = kept_before(a1) - kept_before(a0);
        const int inside = first_key((uint32_t)(i + 1) * pixels) - first_key((uint32_t)i * pixels);
        const int removed = inside - kept;
        if (removed > 0) lane_filtered[i] += removed;
    }
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" size_t dagr_stream_denoise_bytes(int32_t B, int32_t sensor_w, int32_t sensor_h, int64_t max_push) {
    if (!push_sizes_ok(B, sensor_w, sensor_h, max_push)) return 0;
    return carve_denoise(B, (int64_t)sensor_w * sensor_h, max_push, nullptr, 0).s.end;
}

extern "C" int dagr_stream_denoise_reset(void *state, size_t state_bytes, int32_t B, int32_t sensor_w, int32_t sensor_h,
                                         int64_t max_push, void *stream) {
    DAGR_CHECK_ARG(state != nullptr, "stream denoise: state is NULL");
    DAGR_CHECK_ARG(push_sizes_ok(B, sensor_w, sensor_h, max_push), "stream denoise: sizes out of range");
    const int64_t pixels = (int64_t)sensor_w * sensor_h;
    const Denoise f = carve_denoise(B, pixels, max_push, state, state_bytes);
    DAGR_CHECK_ARG(push_state_holds(f.s), "stream denoise: state smaller than dagr_stream_denoise_bytes");
    const int64_t n = (int64_t)B * pixels;
    k_denoise_never<<<(unsigned)ceil_div(n, kBlock), kBlock, 0, (hipStream_t)stream>>>(f.stamps, n);
    DAGR_CHECK_LAUNCH();
    DAGR_CHECK_HIP(hipMemsetAsync(f.s.scan_state, 0, f.s.scan_bytes, (hipStream_t)stream));
    return DAGR_OK;
}

extern "C" int dagr_stream_denoise(void *state, size_t state_bytes, int32_t B, int64_t max_push, int32_t sensor_w,
                                   int32_t sensor_h, int64_t denoise_us, int64_t refractory_us, const int16_t *xy_raw,
                                   const int64_t *t_raw, const int8_t *p_raw, const void *batch_raw, int32_t batch_is_int64,
                                   int64_t n_raw, int16_t *xy_out, int64_t *t_out, int8_t *p_out, int32_t *batch_out,
                                   int32_t *n_out, int64_t *lane_filtered, int32_t *status, void *stream_) {
    DAGR_CHECK_ARG(push_sizes_ok(B, sensor_w, sensor_h, max_push), "stream denoise: sizes out of range");
    DAGR_CHECK_ARG(denoise_us >= 0 && refractory_us >= 0 && (denoise_us > 0 || refractory_us > 0),
                   "stream denoise: denoise_us and refractory_us are positive, or 0 for off, and not both off");
    const std::string complaint = push_args_complaint("stream denoise", state, n_out, status, n_raw, max_push, xy_raw, t_raw,
                                                      p_raw, batch_raw, xy_out, t_out, p_out, batch_out);
    DAGR_CHECK_ARG(complaint.empty(), complaint);
    hipStream_t stream = (hipStream_t)stream_;
    if (n_raw == 0) {
        DAGR_CHECK_HIP(hipMemsetAsync(n_out, 0, 4, stream));
        return DAGR_OK;
    }
    const int64_t pixels = (int64_t)sensor_w * sensor_h;
    const Denoise f = carve_denoise(B, pixels, max_push, state, state_bytes);
    DAGR_CHECK_ARG(push_state_holds(f.s), "stream denoise: state smaller than dagr_stream_denoise_bytes");
    const int n = (int)n_raw, bits = key_bits((int64_t)B * pixels);
    const unsigned grid = (unsigned)ceil_div(n_raw, kBlock);
    const uint32_t sentinel = (uint32_t)((int64_t)B * pixels);
    const int32_t *xy = (const int32_t *)xy_raw;
    DAGR_CHECK_ARG(sort_push_fits(f.s, n, bits), "stream denoise: the sort asks for more temporary storage than the state holds");
    with_batch(batch_raw, batch_is_int64, [&](auto *batch) {
        k_denoise_keys<<<grid, kBlock, 0, stream>>>(xy, batch, n, B, sensor_w, sensor_h, f.s.key_in, f.s.idx_in, status);
    });
    DAGR_CHECK_LAUNCH();
    DAGR_CHECK_HIP(sort_push(f.s, n, bits, stream));
    k_denoise_decide<<<grid, kBlock, 0, stream>>>(f.s.key_out, f.s.idx_out, n, sentinel, sensor_w, sensor_h, t_raw, denoise_us,
                                                  refractory_us, f.stamps, f.s.flag);
    DAGR_CHECK_LAUNCH();
    DAGR_CHECK_HIP(exclusive_scan_i32_chained(f.s.flag, f.s.offs, n_raw, f.s.scan_state, false, stream));
    const unsigned grid_f = (unsigned)ceil_div(std::max<int64_t>(n_raw, B), kBlock);
    with_batch(batch_raw, batch_is_int64, [&](auto *batch) {
        k_denoise_finish<<<grid_f, kBlock, 0, stream>>>(f.s.flag, f.s.offs, n, f.s.key_out, f.s.idx_out, sentinel, B,
                                                        (uint32_t)pixels, xy, t_raw, p_raw, batch, f.stamps, (int32_t *)xy_out,
                                                        t_out, p_out, batch_out, n_out, lane_filtered);
    });
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

