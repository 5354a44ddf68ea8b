// downsample.hip -- event-stream downsampling on the device (f5: the on-GPU half of the event I/O).
// Reference: scripts/downsample_events.py:91-124 (`downsample_events` / `_filter_events_resize`, a numba loop over all
// events): every output cell of fx x fy input pixels integrates polarity / (fx*fy); when |state| reaches 1 the event
// passes (at the cell's coordinates) and its polarity is subtracted.  The loop is sequential in time but independent
// between cells, so: events grouped by output cell in time order (stable sort by cell, done by the caller with one
// torch.sort -- the same preparation the reference's graph builder asks for, graph/utils.py:9-13), then one thread per
// occupied cell walks its run.  `change_map` carries the integrator state from chunk to chunk as in the reference.
//
// The stream front (dagr_stream_downsample) runs the same integrator in front of dagr_stream_stage_dev on raw sensor events
// of several lanes: cell keys, a stable radix sort by key, one thread per run head, a chained scan over the keep flags and
// an order-preserving compaction that leaves the survivors and their count in device memory.
#include "common.hpp"
#include "stream_push.hpp"

namespace dagr {
namespace {

// One event through a cell's integrator; both kernels below call it.
// downsample_events.py:118: change_map[y_l, x_l] += p[i] * 1.0 / (fx * fy) -- the float64 quotient +-1 / (fx * fy), added
// to the fp32 cell in float64 and rounded into it; :120 passes when |state| >= 1; :122 subtracts the polarity of an event
// that passed.  `inc` is the float64 1.0 / (fx * fy), formed on the host and never rounded to fp32 (at an area that is no
// power of two an fp32 increment keeps other events).  Contract: pol in {-1, 0, +1}; then pol * inc is exact and equals the
// reference's (p * 1.0) / area bit for bit, division being correctly rounded and symmetric in sign.
__device__ __forceinline__ bool integrate_event(float &state, float pol, double inc) {
    state = (float)((double)state + (double)pol * inc);
    const bool pass = fabsf(state) >= 1.0f;
    if (pass) state -= pol;
    return pass;
}

__global__ __launch_bounds__(kBlock) void k_downsample_cells(const int32_t *__restrict__ order,       // event ids by (cell, time)
                                                            const int32_t *__restrict__ cell_of,     // [n_runs] cell id
                                                            const int32_t *__restrict__ run_end,     // [n_runs] cumulative
                                                            int n_runs, const int8_t *__restrict__ p, double inc,
                                                            float *__restrict__ change_map, uint8_t *__restrict__ keep) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_runs) return;
    const int a = r == 0 ? 0 : run_end[r - 1], b = run_end[r];
    const int cell = cell_of[r];
    float state = change_map[cell];
    for (int k = a; k < b; k++) {
        const int e = order[k];
        keep[e] = integrate_event(state, (float)p[e], inc) ? 1 : 0;
    }
    change_map[cell] = state;
}

// ---------------------------------------------------------------------------------------------
// Stream front, a keyed push (stream_push.hpp).  Caller-owned state: the lanes' change maps first (offset 0, fp32
// [B, cells_h, cells_w]), then the push's scratch.
struct StreamFront {
    float *maps;
    PushScratch s;
    size_t head_bytes;              // maps + scan state: what a reset zeroes
};

StreamFront carve_front(int B, int64_t cells, int64_t max_push, void *base, size_t state_bytes) {
    Carver c(base);
    StreamFront f;
    f.maps = c.take<float>((size_t)B * cells * 4);
    f.s = carve_push(c, max_push, (int64_t)B * cells, state_bytes);
    f.head_bytes = align_up((size_t)B * cells * 4, 256) + align_up(f.s.scan_bytes, 256);
    return f;
}

bool front_sizes_ok(int32_t B, int32_t cells_w, int32_t cells_h, int64_t max_push) {
    return B >= 1 && B < 128 && cells_w >= 1 && cells_h >= 1 && max_push >= 1 && max_push < (1ll << 31) / 64 &&
           (int64_t)B * cells_w * cells_h < (1ll << 31) - 1;
}

// Launch 1: the key of every raw event over the cell grid (push_key): an event in the strip right of / below the last whole
// cell is never kept either; dagr_stream_stage_dev flags a lane outside [0, B).
template <typename BatchT>
__global__ __launch_bounds__(kBlock) void k_front_keys(const int32_t *__restrict__ xy, const BatchT *__restrict__ batch, int n,
                                                      int B, int fx, int fy, int sensor_w, int sensor_h, int cells_w,
                                                      int cells_h, uint32_t *__restrict__ key, int32_t *__restrict__ idx,
                                                      int32_t *__restrict__ status) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    push_key(xy, batch, i, B, sensor_w, sensor_h, fx, fy, cells_w, cells_h, true, key, idx, status);
}

// Launch 3 (after the sort): one thread per grouped position.  A position whose key differs from its predecessor's is a run
// head and walks its run in arrival order through the cell's integrator; a cell outside the model's width x height
// integrates as every other (the reference downsamples the whole sensor and crops afterwards) but keeps nothing.
__global__ __launch_bounds__(kBlock) void k_front_integrate(const uint32_t *__restrict__ key, const int32_t *__restrict__ idx,
                                                           int n, uint32_t sentinel, int cells_w, int cells_h, int width,
                                                           int height, const int8_t *__restrict__ p, double inc,
                                                           float *__restrict__ maps, int32_t *__restrict__ flag) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const uint32_t mine = key[k];
    if (mine >= sentinel) {
        flag[idx[k]] = 0;
        return;
    }
    if (k > 0 && key[k - 1] == mine) return;
    const int cell = (int)(mine % ((uint32_t)cells_w * (uint32_t)cells_h));
    const bool inside = cell % cells_w < width && cell / cells_w < height;
    float state = maps[mine];
    for (int j = k; j < n && key[j] == mine; ++j) {
        const int e = idx[j];
        const bool pass = integrate_event(state, (float)p[e], inc);
        flag[e] = pass && inside ? 1 : 0;
    }
    maps[mine] = state;
}

// Launch 5 (after the scan): the survivors, in arrival order, at the cells' coordinates, and their count -- as the scan
// leaves it, and no lane-less tail: dagr_stream_stage_dev takes the count from the device.
template <typename BatchT>
__global__ __launch_bounds__(kBlock) void k_front_compact(const int32_t *__restrict__ flag, const int32_t *__restrict__ offs,
                                                         int n, const int32_t *__restrict__ xy, const int64_t *__restrict__ t,
                                                         const int8_t *__restrict__ p, const BatchT *__restrict__ batch,
                                                         int fx, int fy, int32_t *__restrict__ xy_out,
                                                         int64_t *__restrict__ t_out, int8_t *__restrict__ p_out,
                                                         int32_t *__restrict__ batch_out, int32_t *__restrict__ n_out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1) *n_out = offs[i] + flag[i];
    push_survivor(i, flag, offs, xy, t, p, batch, fx, fy, xy_out, t_out, p_out, batch_out);
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" int dagr_downsample_events(const int32_t *order, const int32_t *run_cell, const int32_t *run_end,
                                      int32_t n_runs, const int8_t *polarity, int32_t fx, int32_t fy, float *change_map,
                                      uint8_t *keep, void *stream) {
    DAGR_CHECK_ARG(n_runs >= 0 && fx >= 1 && fy >= 1, "bad sizes");
    if (n_runs == 0) return DAGR_OK;
    DAGR_CHECK_ARG(order && run_cell && run_end && polarity && change_map && keep, "NULL pointer");
    const double inc = 1.0 / (double)(fx * fy);
    k_downsample_cells<<<(unsigned)ceil_div(n_runs, kBlock), kBlock, 0, (hipStream_t)stream>>>(
        order, run_cell, run_end, n_runs, polarity, inc, change_map, keep);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

extern "C" size_t dagr_stream_front_bytes(int32_t B, int32_t cells_w, int32_t cells_h, int64_t max_push) {
    if (!front_sizes_ok(B, cells_w, cells_h, max_push)) return 0;
    return carve_front(B, (int64_t)cells_w * cells_h, max_push, nullptr, 0).s.end;
}

extern "C" int dagr_stream_front_reset(void *front, size_t front_bytes, int32_t B, int32_t cells_w, int32_t cells_h,
                                       int64_t max_push, void *stream) {
    DAGR_CHECK_ARG(front != nullptr, "stream front: state is NULL");
    DAGR_CHECK_ARG(front_sizes_ok(B, cells_w, cells_h, max_push), "stream front: sizes out of range");
    const StreamFront f = carve_front(B, (int64_t)cells_w * cells_h, max_push, front, front_bytes);
    DAGR_CHECK_ARG(push_state_holds(f.s), "stream front: state smaller than dagr_stream_front_bytes");
    DAGR_CHECK_HIP(hipMemsetAsync(front, 0, f.head_bytes, (hipStream_t)stream));
    return DAGR_OK;
}

extern "C" int dagr_stream_downsample(void *front, size_t front_bytes, int32_t B, int64_t max_push, int32_t fx, int32_t fy, int32_t sensor_w,
                                      int32_t sensor_h, int32_t width, int32_t height, const int16_t *xy_raw,
                                      const int64_t *t_raw, const int8_t *p_raw, const void *batch_raw,
                                      int32_t batch_is_int64, int64_t n_raw, int16_t *xy_out, int64_t *t_out, int8_t *p_out,
                                      int32_t *batch_out, int32_t *n_out, int32_t *status, void *stream_) {
    DAGR_CHECK_ARG(fx >= 1 && fy >= 1 && sensor_w >= fx && sensor_h >= fy && sensor_w <= 32767 && sensor_h <= 32767,
                   "stream front: bad factors or sensor size");
    const int32_t cells_w = sensor_w / fx, cells_h = sensor_h / fy;
    DAGR_CHECK_ARG(front_sizes_ok(B, cells_w, cells_h, max_push), "stream front: sizes out of range");
    DAGR_CHECK_ARG(width >= 1 && height >= 1 && width <= cells_w && height <= cells_h,
                   "stream front: the cell grid does not cover width x height");
    const std::string complaint = push_args_complaint("stream front", front, n_out, status, n_raw, max_push, xy_raw, t_raw,
                                                      p_raw, batch_raw, xy_out, t_out, p_out, batch_out);
    DAGR_CHECK_ARG(complaint.empty(), complaint);
    hipStream_t stream = (hipStream_t)stream_;
    if (n_raw == 0) {
        DAGR_CHECK_HIP(hipMemsetAsync(n_out, 0, 4, stream));
        return DAGR_OK;
    }
    const int64_t cells = (int64_t)cells_w * cells_h;
    const StreamFront f = carve_front(B, cells, max_push, front, front_bytes);
    DAGR_CHECK_ARG(push_state_holds(f.s), "stream front: state smaller than dagr_stream_front_bytes");
    const int n = (int)n_raw, bits = key_bits((int64_t)B * cells);
    const unsigned grid = (unsigned)ceil_div(n_raw, kBlock);
    const uint32_t sentinel = (uint32_t)((int64_t)B * cells);
    const double inc = 1.0 / (double)(fx * fy);
    const int32_t *xy = (const int32_t *)xy_raw;
    DAGR_CHECK_ARG(sort_push_fits(f.s, n, bits), "stream front: the sort asks for more temporary storage than the state holds");
    with_batch(batch_raw, batch_is_int64, [&](auto *batch) {
        k_front_keys<<<grid, kBlock, 0, stream>>>(xy, batch, n, B, fx, fy, sensor_w, sensor_h, cells_w, cells_h, f.s.key_in,
                                                  f.s.idx_in, status);
    });
    DAGR_CHECK_LAUNCH();
    DAGR_CHECK_HIP(sort_push(f.s, n, bits, stream));
    k_front_integrate<<<grid, kBlock, 0, stream>>>(f.s.key_out, f.s.idx_out, n, sentinel, cells_w, cells_h, width, height, p_raw,
                                                   inc, f.maps, f.s.flag);
    DAGR_CHECK_LAUNCH();
    DAGR_CHECK_HIP(exclusive_scan_i32_chained(f.s.flag, f.s.offs, n_raw, f.s.scan_state, false, stream));
    with_batch(batch_raw, batch_is_int64, [&](auto *batch) {
        k_front_compact<<<grid, kBlock, 0, stream>>>(f.s.flag, f.s.offs, n, xy, t_raw, p_raw, batch, fx, fy, (int32_t *)xy_out,
                                                     t_out, p_out, batch_out, n_out);
    });
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
