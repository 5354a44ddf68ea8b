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
// them.  Keep flags, the project's chained scan, an order-preserving compaction: as the stream front (downsample.hip).
#include "common.hpp"
#include "stream_sort.hpp"

namespace dagr {
namespace {

constexpr int64_t kNever = INT64_MIN;

// Caller-owned state: the lanes' stamp maps first (offset 0, int64 [B, sensor_h, sensor_w]), then the scan's look-back
// state, then keys / sorted order / flags / offsets for a largest push and the sort's temporary storage.
struct Denoise {
    int64_t *stamps;
    void *scan_state;
    size_t scan_bytes;
    uint32_t *key_in, *key_out;     // [max_push] pixel keys in arrival order / sorted
    int32_t *idx_in, *idx_out;      // [max_push] arrival indices in arrival order / sorted by key, ascending inside a key
    int32_t *flag, *offs;           // [max_push] keep flags in arrival order and their exclusive prefix sum
    void *sort_tmp;
    size_t sort_tmp_bytes, tmp_offset;
};

// sort_storage: also size the sort's temporary storage (dagr_stream_denoise_bytes); the other callers take what is left of
// the caller's buffer behind `sort_tmp`.
size_t carve_denoise(int B, int64_t pixels, int64_t max_push, char *base, Denoise *out, bool sort_storage) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return base ? base + o : nullptr;
    };
    Denoise f;
    f.stamps = (int64_t *)take((size_t)B * pixels * 8);
    f.scan_bytes = scan_chained_state_bytes(max_push);
    f.scan_state = take(f.scan_bytes);
    f.key_in = (uint32_t *)take((size_t)max_push * 4);
    f.key_out = (uint32_t *)take((size_t)max_push * 4);
    f.idx_in = (int32_t *)take((size_t)max_push * 4);
    f.idx_out = (int32_t *)take((size_t)max_push * 4);
    f.flag = (int32_t *)take((size_t)max_push * 4);
    f.offs = (int32_t *)take((size_t)max_push * 4);
    f.sort_tmp_bytes = sort_storage ? sort_tmp_bytes_upto(max_push, key_bits((int64_t)B * pixels)) : 256;
    f.tmp_offset = off;
    f.sort_tmp = take(f.sort_tmp_bytes);
    if (out) *out = f;
    return off;
}

bool denoise_sizes_ok(int32_t B, int32_t sensor_w, int32_t sensor_h, int64_t max_push) {
    return B >= 1 && B < 128 && sensor_w >= 1 && sensor_h >= 1 && sensor_w <= 32767 && sensor_h <= 32767 && max_push >= 1 &&
           max_push < (1ll << 31) / 64 && (int64_t)B * sensor_w * sensor_h < (1ll << 31);
}

__global__ __launch_bounds__(kBlock) void k_denoise_never(int64_t *__restrict__ stamps, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) stamps[i] = kNever;
}

// Launch 1: the key of every event, lane * pixels + y * sensor_w + x, and its arrival index.  An event outside the sensor
// (status bit 4) or with a lane outside [0, B) (dagr_stream_stage_dev flags that one) gets the sentinel key B * pixels: it
// sorts behind every pixel, is never kept and never stamps.
template <typename BatchT>
__global__ __launch_bounds__(kBlock) void k_denoise_keys(const int32_t *__restrict__ xy, const BatchT *__restrict__ batch, int n,
                                                        int B, int sensor_w, int sensor_h, uint32_t *__restrict__ key,
                                                        int32_t *__restrict__ idx, int32_t *__restrict__ status) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t v = xy[i];
    const int x = (int16_t)(v & 0xffff), y = (int16_t)(v >> 16);
    const int64_t b = (int64_t)batch[i];
    const bool outside = x < 0 || x >= sensor_w || y < 0 || y >= sensor_h;
    if (outside) atomicOr(status, 16);
    const uint32_t pixels = (uint32_t)sensor_w * (uint32_t)sensor_h;
    const bool none = outside || b < 0 || b >= B;
    key[i] = none ? (uint32_t)B * pixels : (uint32_t)b * pixels + (uint32_t)(y * sensor_w + x);
    idx[i] = i;
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
    const int total = min(max(offs[n - 1] + flag[n - 1], 0), n);
    if (i < n) {
        const int keep = flag[i], j = offs[i];
        if (i == n - 1) *n_out = total;
        if (keep && j >= 0 && j <= i) {
            xy_out[j] = xy[i];
            t_out[j] = t[i];
            p_out[j] = p[i];
            batch_out[j] = (int32_t)batch[i];
        }
        if (i >= total) {
            xy_out[i] = 0;
            batch_out[i] = -1;
        }
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
    if (!denoise_sizes_ok(B, sensor_w, sensor_h, max_push)) return 0;
    return carve_denoise(B, (int64_t)sensor_w * sensor_h, max_push, nullptr, nullptr, true);
}

extern "C" int dagr_stream_denoise_reset(void *state, size_t state_bytes, int32_t B, int32_t sensor_w, int32_t sensor_h,
                                         int64_t max_push, void *stream) {
    DAGR_CHECK_ARG(state != nullptr, "stream denoise: state is NULL");
    DAGR_CHECK_ARG(denoise_sizes_ok(B, sensor_w, sensor_h, max_push), "stream denoise: sizes out of range");
    Denoise f;
    const int64_t pixels = (int64_t)sensor_w * sensor_h;
    carve_denoise(B, pixels, max_push, (char *)state, &f, false);
    DAGR_CHECK_ARG(state_bytes >= f.tmp_offset + 256, "stream denoise: state smaller than dagr_stream_denoise_bytes");
    const int64_t n = (int64_t)B * pixels;
    k_denoise_never<<<(unsigned)ceil_div(n, kBlock), kBlock, 0, (hipStream_t)stream>>>(f.stamps, n);
    DAGR_CHECK_LAUNCH();
    DAGR_CHECK_HIP(hipMemsetAsync(f.scan_state, 0, f.scan_bytes, (hipStream_t)stream));
    return DAGR_OK;
}

extern "C" int dagr_stream_denoise(void *state, size_t state_bytes, int32_t B, int64_t max_push, int32_t sensor_w,
                                   int32_t sensor_h, int64_t denoise_us, int64_t refractory_us, const int16_t *xy_raw,
                                   const int64_t *t_raw, const int8_t *p_raw, const void *batch_raw, int32_t batch_is_int64,
                                   int64_t n_raw, int16_t *xy_out, int64_t *t_out, int8_t *p_out, int32_t *batch_out,
                                   int32_t *n_out, int64_t *lane_filtered, int32_t *status, void *stream_) {
    DAGR_CHECK_ARG(denoise_sizes_ok(B, sensor_w, sensor_h, max_push), "stream denoise: sizes out of range");
    DAGR_CHECK_ARG(denoise_us >= 0 && refractory_us >= 0 && (denoise_us > 0 || refractory_us > 0),
                   "stream denoise: denoise_us and refractory_us are positive, or 0 for off, and not both off");
    DAGR_CHECK_ARG(state && n_out && status, "stream denoise: NULL pointer");
    DAGR_CHECK_ARG(n_raw >= 0 && n_raw <= max_push, "stream denoise: max_push < n_raw");
    DAGR_CHECK_ARG(n_raw == 0 || (xy_raw && t_raw && p_raw && batch_raw && xy_out && t_out && p_out && batch_out),
                   "stream denoise: NULL input or output");
    DAGR_CHECK_ARG(((uintptr_t)xy_raw & 3) == 0 && ((uintptr_t)xy_out & 3) == 0, "stream denoise: xy must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    if (n_raw == 0) {
        DAGR_CHECK_HIP(hipMemsetAsync(n_out, 0, 4, stream));
        return DAGR_OK;
    }
    Denoise f;
    const int64_t pixels = (int64_t)sensor_w * sensor_h;
    carve_denoise(B, pixels, max_push, (char *)state, &f, false);
    DAGR_CHECK_ARG(state_bytes >= f.tmp_offset + 256, "stream denoise: state smaller than dagr_stream_denoise_bytes");
    f.sort_tmp_bytes = state_bytes - f.tmp_offset;
    const int n = (int)n_raw, bits = key_bits((int64_t)B * pixels);
    const unsigned grid = (unsigned)ceil_div(n_raw, kBlock);
    const uint32_t sentinel = (uint32_t)((int64_t)B * pixels);
    size_t tmp = 0;
    DAGR_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, tmp, f.key_in, f.key_out, f.idx_in, f.idx_out, (size_t)n, 0u,
                                             (unsigned)bits, stream));
    DAGR_CHECK_ARG(tmp <= f.sort_tmp_bytes, "stream denoise: the sort asks for more temporary storage than the state holds");
    tmp = f.sort_tmp_bytes;
    if (batch_is_int64)
        k_denoise_keys<int64_t><<<grid, kBlock, 0, stream>>>((const int32_t *)xy_raw, (const int64_t *)batch_raw, n, B,
                                                            sensor_w, sensor_h, f.key_in, f.idx_in, status);
    else
        k_denoise_keys<int32_t><<<grid, kBlock, 0, stream>>>((const int32_t *)xy_raw, (const int32_t *)batch_raw, n, B,
                                                            sensor_w, sensor_h, f.key_in, f.idx_in, status);
    DAGR_CHECK_LAUNCH();
    DAGR_CHECK_HIP(rocprim::radix_sort_pairs(f.sort_tmp, tmp, f.key_in, f.key_out, f.idx_in, f.idx_out, (size_t)n, 0u,
                                             (unsigned)bits, stream));
    k_denoise_decide<<<grid, kBlock, 0, stream>>>(f.key_out, f.idx_out, n, sentinel, sensor_w, sensor_h, t_raw, denoise_us,
                                                  refractory_us, f.stamps, f.flag);
    DAGR_CHECK_LAUNCH();
    DAGR_CHECK_HIP(exclusive_scan_i32_chained(f.flag, f.offs, n_raw, f.scan_state, false, stream));
    const unsigned grid_f = (unsigned)ceil_div(std::max<int64_t>(n_raw, B), kBlock);
    if (batch_is_int64)
        k_denoise_finish<int64_t><<<grid_f, kBlock, 0, stream>>>(f.flag, f.offs, n, f.key_out, f.idx_out, sentinel, B,
                                                                (uint32_t)pixels, (const int32_t *)xy_raw, t_raw, p_raw,
                                                                (const int64_t *)batch_raw, f.stamps, (int32_t *)xy_out,
                                                                t_out, p_out, batch_out, n_out, lane_filtered);
    else
        k_denoise_finish<int32_t><<<grid_f, kBlock, 0, stream>>>(f.flag, f.offs, n, f.key_out, f.idx_out, sentinel, B,
                                                                (uint32_t)pixels, (const int32_t *)xy_raw, t_raw, p_raw,
                                                                (const int32_t *)batch_raw, f.stamps, (int32_t *)xy_out,
                                                                t_out, p_out, batch_out, n_out, lane_filtered);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
