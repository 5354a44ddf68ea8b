// stream_flicker.hip -- the event stream's anti-flicker and trail filters (dagr_stream_flicker): two per-pixel state
// machines on a raw push, in front of dagr_stream_denoise / dagr_stream_downsample / dagr_stream_stage_dev.
//
// Every pixel of every lane carries t_edge, last_p, count, blocking (the flicker stage: it counts OFF -> ON edges whose
// period lies in [min_period, max_period] and blocks the pixel between two hysteresis thresholds) and t_pass, p_pass (the
// trail stage: an event of the polarity of the last event that reached the stage, less than trail_us after it, is
// dropped).  The trail stage sees only what the flicker stage let through, so a decision depends on earlier decisions:
// the one-thread-per-event shape of stream_denoise.hip does not carry over.  Instead, as the stream front (downsample.hip):
// pixel keys (lane, y, x), a stable radix sort with the arrival index as payload, then the head of every run takes its
// pixel's events in arrival order through both stages, from the carried state, and stores the state once.  A pixel's
// state is read and written by its run's walker alone.  Keep flags, the project's chained scan, an order-preserving
// compaction: a keyed push (stream_push.hpp), as the other two fronts.  No floating point anywhere.
//
// The walk.  Real pushes hold a few events per pixel, and one thread per run is then the right shape: 64 runs per wave,
// one dependent load chain (arrival index -> t, p) per event.  A stuck pixel puts hundreds or thousands of events into one
// run, and a single lane would pay that chain once per event while its wave waits.  So a run of kLongRun events or more
// -- the head sees that from key[head + kLongRun - 1], the keys being sorted -- is left to the whole wave: 64 events are
// loaded per round by 64 lanes, one load latency for all of them, and walked from registers (v_readlane with a uniform
// index, so the state machine itself runs once per wave, not per lane).
#include "common.hpp"
#include "stream_push.hpp"

namespace dagr {
namespace {

constexpr int64_t kNever = INT64_MIN;
// Runs from this length on are walked by their wave.  Not a measured optimum: below it a wave's 64 lanes walk up to 64 runs
// side by side and a cooperative round would serialise them; from it on the longest lane would hold its wave for
// 16 dependent load chains or more.
constexpr int kLongRun = 16;

// The options of a call, as the kernels take them.
struct FlickerRule {
    int64_t min_period, max_period;     // max_period == 0: the flicker stage is off
    int64_t trail_us;                   // 0: the trail stage is off
    int start, stop, max_count;
};

// A pixel's state, unpacked.  The packed word: bits 0..7 count, bit 8 blocking, bits 9..10 last_p, bits 11..12 p_pass
// (a polarity field is 0: none yet, 1: +1, 2: -1); 0 is the initial state.
struct Pixel {
    int64_t t_edge, t_pass;
    int count, last_p, p_pass;          // polarities as -1 / 0 / +1
    bool blocking;
};

__device__ __forceinline__ int pol_of(int field) { return field == 1 ? 1 : field == 2 ? -1 : 0; }
__device__ __forceinline__ int field_of(int pol) { return pol > 0 ? 1 : pol < 0 ? 2 : 0; }

__device__ __forceinline__ Pixel unpack_pixel(int64_t t_edge, int64_t t_pass, int32_t word) {
    Pixel s;
    s.t_edge = t_edge;
    s.t_pass = t_pass;
    s.count = word & 0xff;
    s.blocking = (word >> 8) & 1;
    s.last_p = pol_of((word >> 9) & 3);
    s.p_pass = pol_of((word >> 11) & 3);
    return s;
}

__device__ __forceinline__ int32_t pack_word(const Pixel &s) {
    return (s.count & 0xff) | ((s.blocking ? 1 : 0) << 8) | (field_of(s.last_p) << 9) | (field_of(s.p_pass) << 11);
}

// One event through both stages: 0 kept, 1 removed by the flicker stage, 2 removed by the trail stage.  Every walker
// calls this, so the rule is stated once on the device.
__device__ __forceinline__ int pixel_event(Pixel &s, int64_t t, int p, const FlickerRule &r) {
    const int pol = p > 0 ? 1 : -1;
    if (r.max_period > 0) {
        if (s.t_edge != kNever && t - s.t_edge > r.max_period) s.count = 0;                 // stale
        if (pol > 0 && s.last_p < 0) {                                                      // an OFF -> ON edge
            if (s.t_edge != kNever) {
                const int64_t d = t - s.t_edge;
                if (d >= r.min_period && d <= r.max_period) s.count = min(s.count + 1, r.max_count);
                else if (d < r.min_period) s.count = max(s.count - 1, 0);
            }
            s.t_edge = t;
        }
        if (s.count >= r.start) s.blocking = true;
        else if (s.count <= r.stop) s.blocking = false;
        s.last_p = pol;
        if (s.blocking) return 1;
    }
    if (r.trail_us > 0) {
        const bool trail = s.p_pass == pol && s.t_pass != kNever && t - s.t_pass < r.trail_us;
        s.t_pass = t;
        s.p_pass = pol;
        if (trail) return 2;
    }
    return 0;
}

// Caller-owned state: the per-pixel maps first -- t_edge int64 [B, sensor_h, sensor_w] at offset 0, t_pass int64 at
// map_stride, the packed words int32 at 2 * map_stride, with map_stride = 8 * B * pixels rounded up to 256 --, then the
// push's scratch (stream_push.hpp) with the outcomes as its extra array.
struct Flicker {
    int64_t *t_edge, *t_pass;
    int32_t *word;
    PushScratch s;
    int8_t *outcome;                // [max_push] 0 / 1 / 2 in arrival order (0 for an event that is none of the sensor's)
};

Flicker carve_flicker(int B, int64_t pixels, int64_t max_push, void *base, size_t state_bytes) {
    Carver c(base);
    Flicker f;
    f.t_edge = c.take<int64_t>((size_t)B * pixels * 8);
    f.t_pass = c.take<int64_t>((size_t)B * pixels * 8);
    f.word = c.take<int32_t>((size_t)B * pixels * 4);
    f.s = carve_push(c, max_push, (int64_t)B * pixels, state_bytes, (size_t)max_push);
    f.outcome = (int8_t *)f.s.extra;
    return f;
}

__global__ __launch_bounds__(kBlock) void k_flicker_initial(int64_t *__restrict__ t_edge, int64_t *__restrict__ t_pass,
                                                           int32_t *__restrict__ word, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    t_edge[i] = kNever;
    t_pass[i] = kNever;
    word[i] = 0;
}

// Launch 1: the key of every event over the sensor's pixels, lane * pixels + y * sensor_w + x (push_key).  An event with
// the sentinel key meets no state and is not counted.  A row with a lane outside [0, B) is a lane-less row of the stage in
// front (dagr_stream_stage_dev flags any other on the clock): it raises no status bit, wherever it lies.
template <typename BatchT>
__global__ __launch_bounds__(kBlock) void k_flicker_keys(const int32_t *__restrict__ xy, const BatchT *__restrict__ batch, int n,
                                                        int B, int sensor_w, int sensor_h, uint32_t *__restrict__ key,
                                                        int32_t *__restrict__ idx, int32_t *__restrict__ status) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    push_key(xy, batch, i, B, sensor_w, sensor_h, 1, 1, sensor_w, sensor_h, false, key, idx, status);
}

// Launch 3 (after the sort): one thread per sorted position.  A position whose key differs from its predecessor's is a run
// head.  A head of a run shorter than kLongRun walks it alone; then the wave takes its longer runs one after the other, 64
// events a round.  Every event gets its outcome and its keep flag at its arrival index; the pixel's state is stored once.
// No early return: every lane of a wave reaches the cooperative part.
__global__ __launch_bounds__(kBlock) void k_flicker_walk(const uint32_t *__restrict__ key, const int32_t *__restrict__ idx,
                                                        int n, uint32_t sentinel, const int64_t *__restrict__ t,
                                                        const int8_t *__restrict__ p, FlickerRule rule,
                                                        int64_t *__restrict__ t_edge, int64_t *__restrict__ t_pass,
                                                        int32_t *__restrict__ word, int32_t *__restrict__ flag,
                                                        int8_t *__restrict__ outcome) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const bool live = k < n;
    const uint32_t mine = live ? key[k] : sentinel;
    const bool pixel = live && mine < sentinel;
    if (live && !pixel) {
        const int e = min(max(idx[k], 0), n - 1);
        flag[e] = 0;
        outcome[e] = 0;
    }
    const bool head = pixel && (k == 0 || key[k - 1] != mine);
    const bool long_run = head && k + kLongRun - 1 < n && key[k + kLongRun - 1] == mine;
    if (head && !long_run) {
        Pixel s = unpack_pixel(t_edge[mine], t_pass[mine], word[mine]);
        for (int j = k; j < n && j < k + kLongRun && key[j] == mine; ++j) {
            const int e = min(max(idx[j], 0), n - 1);
            const int out = pixel_event(s, t[e], p[e], rule);
            flag[e] = out == 0 ? 1 : 0;
            outcome[e] = (int8_t)out;
        }
        t_edge[mine] = s.t_edge;
        t_pass[mine] = s.t_pass;
        word[mine] = pack_word(s);
    }
    unsigned long long todo = __ballot(long_run);
    while (todo != 0) {                                     // (wave-uniform: a ballot's result)
        const int owner = __ffsll(todo) - 1;
        todo &= todo - 1;
        const int k0 = __shfl(k, owner);
        const uint32_t pix = (uint32_t)__shfl((int)mine, owner);
        Pixel s = unpack_pixel(t_edge[pix], t_pass[pix], word[pix]);      // every lane reads the same three words
        for (int base = k0; base < n; base += kWave) {
            const int j = base + lane;
            const bool in_run = j < n && key[j] == pix;     // a prefix of the round's lanes: the keys are sorted
            int e = 0, pe = 0, out = 0;
            int64_t te = 0;
            if (in_run) {
                e = min(max(idx[j], 0), n - 1);
                te = t[e];
                pe = p[e];
            }
            const int count = __popcll(__ballot(in_run));
            const int t_lo = (int)(uint32_t)te, t_hi = (int)(te >> 32);
            for (int i = 0; i < count; ++i) {
                const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane(t_lo, i);
                const int64_t ti = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane(t_hi, i) << 32) | lo);
                const int o = pixel_event(s, ti, __builtin_amdgcn_readlane(pe, i), rule);
                if (lane == i) out = o;
            }
            if (in_run) {
                flag[e] = out == 0 ? 1 : 0;
                outcome[e] = (int8_t)out;
            }
            if (count < kWave) break;
        }
        if (lane == owner) {
            t_edge[pix] = s.t_edge;
            t_pass[pix] = s.t_pass;
            word[pix] = pack_word(s);
        }
    }
}

// One wave adds its events of outcome `which` to their lanes' counters: one vector atomic per lane id present in the wave
// (the push is in lane order, so that is nearly always one).  Every lane of the wave calls this.
__device__ __forceinline__ void count_outcome(bool is, int b, int lane, int64_t *__restrict__ counter) {
    unsigned long long left = __ballot(is);
    while (left != 0) {
        const int first = __ffsll(left) - 1;
        const int bb = __shfl(b, first);
        const unsigned long long same = __ballot(is && b == bb);
        if (lane == first) atomicAdd((unsigned long long *)&counter[bb], (unsigned long long)__popcll(same));
        left &= ~same;
    }
}

// Launch 5 (after the scan), over the arrival index: the survivors in arrival order and their count; the rows from the
// count up to n get lane -1 at pixel (0, 0), as dagr_stream_denoise leaves them; the two per-lane counters.
template <typename BatchT>
__global__ __launch_bounds__(kBlock) void k_flicker_finish(const int32_t *__restrict__ flag, const int32_t *__restrict__ offs,
                                                          const int8_t *__restrict__ outcome, int n, int B,
                                                          const int32_t *__restrict__ xy, const int64_t *__restrict__ t,
                                                          const int8_t *__restrict__ p, const BatchT *__restrict__ batch,
                                                          int32_t *__restrict__ xy_out, int64_t *__restrict__ t_out,
                                                          int8_t *__restrict__ p_out, int32_t *__restrict__ batch_out,
                                                          int32_t *__restrict__ n_out, int64_t *__restrict__ lane_flicker,
                                                          int64_t *__restrict__ lane_trail) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const int total = push_total(flag, offs, n);
    int out = 0, b = 0;
    if (i < n) {
        const int64_t b64 = (int64_t)batch[i];
        out = outcome[i];
        if (b64 < 0 || b64 >= B) out = 0;                  // (its outcome is 0 already: it met no state)
        b = (int)min(max(b64, (int64_t)0), (int64_t)B - 1);
        push_survivor(i, flag, offs, xy, t, p, batch, 1, 1, xy_out, t_out, p_out, batch_out);
        push_tail(i, n, total, xy_out, batch_out, n_out);
    }
    if (lane_flicker) count_outcome(out == 1, b, lane, lane_flicker);
    if (lane_trail) count_outcome(out == 2, b, lane, lane_trail);
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" size_t dagr_stream_flicker_bytes(int32_t B, int32_t sensor_w, int32_t sensor_h, int64_t max_push) {
    if (!push_sizes_ok(B, sensor_w, sensor_h, max_push)) return 0;
    return carve_flicker(B, (int64_t)sensor_w * sensor_h, max_push, nullptr, 0).s.end;
}

extern "C" int dagr_stream_flicker_reset(void *state, size_t state_bytes, int32_t B, int32_t sensor_w, int32_t sensor_h,
                                         int64_t max_push, void *stream) {
    DAGR_CHECK_ARG(state != nullptr, "stream flicker: state is NULL");
    DAGR_CHECK_ARG(push_sizes_ok(B, sensor_w, sensor_h, max_push), "stream flicker: sizes out of range");
    const int64_t pixels = (int64_t)sensor_w * sensor_h;
    const Flicker f = carve_flicker(B, pixels, max_push, state, state_bytes);
    DAGR_CHECK_ARG(push_state_holds(f.s), "stream flicker: state smaller than dagr_stream_flicker_bytes");
    const int64_t n = (int64_t)B * pixels;
    k_flicker_initial<<<(unsigned)ceil_div(n, kBlock), kBlock, 0, (hipStream_t)stream>>>(f.t_edge, f.t_pass, f.word, n);
    DAGR_CHECK_LAUNCH();
    DAGR_CHECK_HIP(hipMemsetAsync(f.s.scan_state, 0, f.s.scan_bytes, (hipStream_t)stream));
    return DAGR_OK;
}

extern "C" int dagr_stream_flicker(void *state, size_t state_bytes, int32_t B, int64_t max_push, int32_t sensor_w,
                                   int32_t sensor_h, int64_t min_period_us, int64_t max_period_us, int32_t start, int32_t stop,
                                   int32_t max_count, int64_t trail_us, const int16_t *xy_raw, const int64_t *t_raw,
                                   const int8_t *p_raw, const void *batch_raw, int32_t batch_is_int64, int64_t n_raw,
                                   int16_t *xy_out, int64_t *t_out, int8_t *p_out, int32_t *batch_out, int32_t *n_out,
                                   int64_t *lane_flicker, int64_t *lane_trail, int32_t *status, void *stream_) {
    DAGR_CHECK_ARG(push_sizes_ok(B, sensor_w, sensor_h, max_push), "stream flicker: sizes out of range");
    DAGR_CHECK_ARG(max_period_us >= 0 && trail_us >= 0 && (max_period_us > 0 || trail_us > 0),
                   "stream flicker: max_period_us and trail_us are positive, or 0 for off, and not both off");
    DAGR_CHECK_ARG(max_period_us == 0 || (min_period_us >= 1 && min_period_us <= max_period_us && max_period_us <= 1000000),
                   "stream flicker: the periods must satisfy 1 <= min_period_us <= max_period_us <= 1000000");
    DAGR_CHECK_ARG(max_period_us == 0 || (0 <= stop && stop < start && start <= max_count && max_count <= 255),
                   "stream flicker: the thresholds must satisfy 0 <= stop < start <= max_count <= 255");
    const std::string complaint = push_args_complaint("stream flicker", state, n_out, status, n_raw, max_push, xy_raw, t_raw,
                                                      p_raw, batch_raw, xy_out, t_out, p_out, batch_out);
    DAGR_CHECK_ARG(complaint.empty(), complaint);
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t pixels = (int64_t)sensor_w * sensor_h;
    const Flicker f = carve_flicker(B, pixels, max_push, state, state_bytes);
    DAGR_CHECK_ARG(push_state_holds(f.s), "stream flicker: state smaller than dagr_stream_flicker_bytes");
    if (n_raw == 0) {
        DAGR_CHECK_HIP(hipMemsetAsync(n_out, 0, 4, stream));
        return DAGR_OK;
    }
    const int n = (int)n_raw, bits = key_bits((int64_t)B * pixels);
    const unsigned grid = (unsigned)ceil_div(n_raw, kBlock);
    const uint32_t sentinel = (uint32_t)((int64_t)B * pixels);
    const FlickerRule rule{min_period_us, max_period_us, trail_us, start, stop, max_count};
    const int32_t *xy = (const int32_t *)xy_raw;
    DAGR_CHECK_ARG(sort_push_fits(f.s, n, bits), "stream flicker: the sort asks for more temporary storage than the state holds");
    with_batch(batch_raw, batch_is_int64, [&](auto *batch) {
        k_flicker_keys<<<grid, kBlock, 0, stream>>>(xy, batch, n, B, sensor_w, sensor_h, f.s.key_in, f.s.idx_in, status);
    });
    DAGR_CHECK_LAUNCH();
    DAGR_CHECK_HIP(sort_push(f.s, n, bits, stream));
    k_flicker_walk<<<grid, kBlock, 0, stream>>>(f.s.key_out, f.s.idx_out, n, sentinel, t_raw, p_raw, rule, f.t_edge, f.t_pass,
                                                f.word, f.s.flag, f.outcome);
    DAGR_CHECK_LAUNCH();
    DAGR_CHECK_HIP(exclusive_scan_i32_chained(f.s.flag, f.s.offs, n_raw, f.s.scan_state, false, stream));
    with_batch(batch_raw, batch_is_int64, [&](auto *batch) {
        k_flicker_finish<<<grid, kBlock, 0, stream>>>(f.s.flag, f.s.offs, f.outcome, n, B, xy, t_raw, p_raw, batch,
                                                      (int32_t *)xy_out, t_out, p_out, batch_out, n_out, lane_flicker,
                                                      lane_trail);
    });
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

