/*
 * dagr_hip.h -- C ABI of libdagr_hip.so, the MI355X (gfx950) engine for DAGR's
 * event-graph hot path.
 *
 * Conventions (all entry points)
 *   - plain C: pointers + sizes, no torch / HIP types.  `stream` is a
 *     hipStream_t passed as void* (NULL = the null stream).
 *   - every pointer is a DEVICE pointer owned by the caller unless marked
 *     "host".  The library never allocates device memory: callers query
 *     *_workspace_bytes() and hand in a workspace.
 *   - returns 0 on success, a negative dagr_status otherwise;
 *     dagr_last_error() returns a thread-local message (the Python binding
 *     turns it into RuntimeError, mirroring the reference's AT_ASSERTM ->
 *     RuntimeError convention, ev_graph.cu:9-12).
 *   - kernels are enqueued asynchronously on `stream`; nothing synchronises
 *     unless the entry point says so.
 *
 * Reference interfaces replaced (paths relative to uzh-rpg/dagr @ 2025-02-02):
 *   src/dagr/graph/ev_graph.cu:279-283   pybind module `ev_graph_cuda`
 *   src/dagr/graph/utils.py:6-23         host prep around it (sort/unique/cumsum, mask compaction)
 *   src/dagr/graph/ev_graph.py:18-166    AsyncGraph / SlidingWindowGraph state
 *   src/dagr/model/layers/ev_tgn.py:11-16 denormalize_pos
 *   src/dagr/utils/buffers.py:33-44      format_data
 *   third-party ops named at each section below.
 */
#ifndef DAGR_HIP_H
#define DAGR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    DAGR_OK = 0,
    DAGR_ERR_INVALID_ARG = -1,
    DAGR_ERR_HIP = -2,
    DAGR_ERR_WORKSPACE = -3,
    DAGR_ERR_UNSUPPORTED = -4
} dagr_status;

const char *dagr_last_error(void);
/* library / ABI version: major*10000 + minor*100 + patch */
int dagr_version(void);
/* number of visible HIP devices (<0 on error) -- lets bindings fail loudly early */
int dagr_device_count(void);

/* ------------------------------------------------------------------------ *
 * (a1) format_data  -- src/dagr/utils/buffers.py:33-44
 *   pos_out[n] = { x/W, y/H, t/T } as fp32 true division of fp32-converted ints,
 *   feat_out[n] = (float)p.
 * ------------------------------------------------------------------------ */
int dagr_format_events(const int16_t *xy /*[N,2]*/, const int32_t *t /*[N]*/, const int8_t *p /*[N]*/,
                       int64_t N, int32_t width, int32_t height, int32_t time_window,
                       float *pos_out /*[N,3]*/, float *feat_out /*[N]*/, void *stream);

/* ------------------------------------------------------------------------ *
 * 1:1 replacements of the reference's native module `ev_graph_cuda` (src/dagr/graph/ev_graph.cu:279-283),
 * same arguments in the same order, on the caller's own state (FIFO volume int32[B,Q,H,W] with -1 =
 * empty and q = 0 newest, timestamp log, -1-filled int64 edge buffer), so the Python classes of
 * src/dagr/graph/ev_graph.py work unchanged on top of them -- including reset=False / min_index > 0.
 *   dagr_fill_edges             <- fill_edges_cuda(batch, pos, all_timestamps, event_queue, indices,
 *                                  max_num_neighbors, radius, delta_t_us, edges, min_index)   ev_graph.cu:82-128
 *   dagr_insert_in_queue        <- insert_in_queue_cuda(indices, unique_coords, cumsum_counts, queue)   :241-276
 *   dagr_insert_in_queue_single <- insert_in_queue_single_cuda(indices, events, queue)                  :215-238
 * Shapes ride along as integers (N = len(batch), edges_cols = edges.size(1), queue dims).
 * ------------------------------------------------------------------------ */
int dagr_fill_edges(const int32_t *batch /*[N]*/, const int32_t *pos /*[N,3] x,y,t_us*/,
                    const int32_t *all_timestamps, const int32_t *event_queue /*[B,Q,H,W]*/,
                    const int32_t *indices /*[N]*/, int32_t max_num_neighbors, float radius, float delta_t_us,
                    int64_t *edges /*[2,edges_cols], in/out*/, int64_t edges_cols, int32_t min_index,
                    int64_t N, int32_t B, int32_t Q, int32_t H, int32_t W, void *stream);
int dagr_insert_in_queue(const int32_t *indices /*[N] pixel-sorted*/, const int32_t *unique_coords /*[num_pixels]*/,
                         const int32_t *cumsum_counts /*[num_pixels]*/, int64_t num_pixels, int32_t *queue,
                         int32_t B, int32_t Q, int32_t H, int32_t W, void *stream);
int dagr_insert_in_queue_single(const int32_t *indices /*[1]*/, const int32_t *event_xy /*>= [2]: x, y*/,
                                int32_t *queue, int32_t B, int32_t Q, int32_t H, int32_t W, void *stream);

/* ------------------------------------------------------------------------ *
 * Window graph builder (reset=True semantics)
 *   replaces, for one self-contained window, the sequence
 *     SlidingWindowGraph.reset()                       ev_graph.py:52-60
 *     denormalize_pos                                  ev_tgn.py:11-16
 *     _insert_events_into_queue + insert_in_queue_*    graph/utils.py:6-18, ev_graph.cu:130-212
 *     _search_for_edges + fill_edges_cuda_kernel       graph/utils.py:20-23, ev_graph.cu:15-80
 *   Output is the reference's edge set in the reference's order (self loop
 *   first, then spiral discovery order, <= max_neighbors per destination),
 *   stored as fixed-stride neighbour lists instead of a -1-padded int64 buffer.
 * ------------------------------------------------------------------------ */
typedef struct {
    int32_t width;          /* W, pixels                                  */
    int32_t height;         /* H, pixels                                  */
    int32_t batch_size;     /* B, samples per window batch                */
    int32_t max_neighbors;  /* K, incl. the self loop (reference: 16)     */
    int32_t queue_size;     /* Q, per-pixel FIFO depth (reference: 128)   */
    int32_t radius;         /* r, pixels: int(radius*W+1), ev_tgn.py:29   */
    int32_t delta_t_us;     /* int(radius*time_window),  ev_tgn.py:28     */
    int32_t time_window;    /* T, us (normaliser of pos[:,2])             */
    int64_t max_events;     /* capacity N_max of the workspace            */
} dagr_graph_desc;

size_t dagr_graph_workspace_bytes(const dagr_graph_desc *desc);
/* must be called once on a fresh workspace (zeroes the per-key counters) */
int dagr_graph_workspace_init(const dagr_graph_desc *desc, void *workspace, size_t workspace_bytes, void *stream);

/* Node numbering: the graph comes out in *slot space* -- node n is the n-th event in (sample, y, x,
 * time) order (the builder's CSR-by-pixel order), so that spatial neighbours are memory
 * neighbours in every level-0 array and the events of a range of pixel rows are one run of nodes.  nbr_src holds node numbers.  dagr_graph_node_order exports the permutation,
 * dagr_graph_gather_inputs brings the per-event inputs into node order, dagr_graph_edge_index emits the
 * reference-shaped, event-ordered int64 edge_index.
 *
 * pos: pos_is_int32 == 0: normalised fp32 [N,3] exactly as format_data produces it (denormalised
 *      on the fly, ev_tgn.py:11-16); pos_is_int32 == 1: int32 [N,3] = (x, y, t_us), the input
 *      contract of SlidingWindowGraph.forward (ev_graph.py:139).
 * batch: int32[N] or int64[N] (sample index, non-decreasing not required).
 * nbr_src[N,K] int32 : source node of slot j of destination node n (slot 0 = n itself)
 * nbr_code[N,K] int16: (dx+r)*(2r+1) + (dy+r) with (dx,dy) = pixel offset source - destination
 * deg[N] int32       : number of valid slots (1..K)
 * Slots >= deg[n] are left untouched. */
int dagr_graph_build_window(const dagr_graph_desc *desc, void *workspace,
                            const void *pos, int32_t pos_is_int32,
                            const void *batch, int32_t batch_is_int64, int64_t N,
                            int32_t *nbr_src, int16_t *nbr_code, int32_t *deg, void *stream);

/* dagr_graph_build_window with the event count in DEVICE memory: every launch is sized for `n_cap` events and bounded by
 * *n_dev (<= n_cap) on the device, so the call can be captured in a HIP graph once and replayed for windows of any size.
 * pos / batch: the static buffers dagr_stage_window filled -- that launch has already run the build's first step
 * (denormalise + per-key count) on them and cleared the status words; this call continues from there. */
int dagr_graph_build_window_dev(const dagr_graph_desc *desc, void *workspace, const void *pos, int32_t pos_is_int32,
                                const void *batch, int32_t batch_is_int64, int64_t n_cap, const int32_t *n_dev,
                                int32_t *nbr_src, int16_t *nbr_code, int32_t *deg, void *stream);
/* device address of the number of nodes (indexed events) of the last build on this workspace: the `n_ptr` of the kernels
 * that follow it in a captured window */
const int32_t *dagr_graph_node_count_ptr(const dagr_graph_desc *desc, void *workspace);
/* One launch that copies a caller's window (format_data output: pos fp32[N,3], feat fp32[N], batch int32/int64[N]) into
 * static buffers (batch as int32), writes N to *n_dev, clears the builder's status words and runs the build's first step
 * (denormalise_pos + the per-key count, ev_tgn.py:11-16): the only per-window launch in front of a captured window graph
 * (dagr_graph_build_window_dev continues from its results). */
int dagr_stage_window(const dagr_graph_desc *desc, void *workspace, const float *pos, const float *feat, const void *batch,
                      int32_t batch_is_int64, int64_t N, float *pos_out, float *feat_out, int32_t *batch_out,
                      int32_t *n_dev, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream: a sliding window kept on the device
 *   The raw events of the running window stay in caller-owned device memory (`state`); a step takes the NEW raw events,
 *   retires what has left the window and writes the next window straight into the static input buffers of a captured
 *   window -- what dagr_stage_window does for a caller's window -- with the event count left in device memory.
 *
 * What a step computes.  Lanes b = 0..B-1 are the samples of desc.batch_size; each lane is an endless event sequence of
 * (x, y) int16 pixels, t int64 absolute microseconds, p int8 in {-1, +1}; inside a lane t is non-decreasing, within a
 * push and across pushes.  After a push
 *   t_ref[b] = t_now[b] when t_now is given, else the t of the lane's newest event; it must not be older than the lane's
 *              newest event nor than the lane's previous t_ref;
 *   the lane's window is every event ever pushed to it with 0 <= t_ref[b] - t < window_us, in arrival order (a suffix of
 *              the lane: what has left never comes back);
 *   t_rel    = time_window - (t_ref[b] - t) as int32 (without t_now the newest event sits at time_window, where
 *              DSEC.preprocess_events puts it, data/dsec_data.py:157-163);
 *   the batch window is the lanes' windows concatenated in lane order, and the outputs are dagr_format_events of
 *              (x, y, t_rel, p) under (width, height, time_window): pos_out fp32[n,3], feat_out fp32[n], batch_out
 *              int32[n] = the lane, *n_dev = n, lane_count[b] = events of lane b.
 * The stage also clears the builder's status words and runs the build's first step on the formatted rows, exactly as
 * dagr_stage_window does: dagr_graph_build_window_dev continues from either.  Two launches, no host synchronisation.
 *
 * state: dagr_stream_state_bytes(B, capacity) bytes, dagr_stream_reset before the first step (and to empty the stream).
 *        It holds two raw sets of `capacity` events written alternately (13 bytes per event each), the lanes' segment
 *        bounds and t_ref[B].  capacity <= desc.max_events, which sizes the outputs.
 * xy_new int16[n_new,2] (4-byte aligned), t_new int64[n_new], p_new int8[n_new], batch_new int32/int64[n_new] sorted, in
 * [0, B); t_now int64[B] or NULL; all in device memory.
 * status: one int32 in device memory, bits are OR-ed in and never acted on by faulting (every index is clamped to the
 * buffers; a flagged step's outputs are unspecified):
 *   bit 0: a timestamp goes backwards inside a lane, within a push or against the lane's newest event;
 *   bit 1: t_ref is behind the lane's newest event or behind its previous t_ref;
 *   bit 2: survivors plus new events exceed `capacity`;
 *   bit 3: batch_new is not sorted or is outside [0, B);
 *   bit 4: (dagr_stream_downsample) a raw event outside the sensor;
 *   bit 5: (dagr_stream_frame) a frame's lane is outside [0, B);
 *   bit 6: (dagr_stream_decode) a push decodes more events than max_out.
 * Events outside the sensor raise the builder's own flag (dagr_graph_status).
 * DAGR_ERR_INVALID_ARG before any launch: window_us <= 0, window_us > desc.time_window, capacity < n_new,
 * capacity > desc.max_events, B != desc.batch_size, NULL pointers.
 * dagr_stream_grow copies a state into a larger one (capacity_new >= capacity) on the device.
 *
 * dagr_stream_stage_capped: the same step with a cap on every lane's event count, max_lane_events = N >= 1.  The lane's
 * window is what the rule above leaves, cut to its LAST N events in arrival order when there are more (equal timestamps
 * are cut by arrival order): the newest events stay.  The cut takes the oldest events away, the lane's survivors first,
 * then the front of its push, and adds their number -- max(0, survivors + new events after the time cut - N) -- to
 * lane_dropped[b] (int64[B] in device memory, accumulated by plain stores of the lane's thread; the caller zeroes it; may
 * be NULL).  t_ref, t_rel, the clock, the status bits and the lane order are unchanged.  The capped window equals the time
 * rule applied to everything ever pushed to the lane, then the last N, whatever the chunking of the pushes.
 * Capacity: capacity >= B * max_lane_events replaces capacity >= n_new; a push may be larger than the capacity (only its
 * newest N per lane can stay; n_new < 2^30), no window can exceed it, and bit 2 is never raised.  A state can change
 * between the capped and the uncapped entry from step to step.
 * ------------------------------------------------------------------------ */
size_t dagr_stream_state_bytes(int32_t B, int64_t capacity);
int dagr_stream_reset(void *state, int32_t B, int64_t capacity, void *stream);
int dagr_stream_grow(const void *state, int64_t capacity, void *state_new, int64_t capacity_new, int32_t B, void *stream);
int dagr_stream_stage(const dagr_graph_desc *desc, void *workspace, void *state, int32_t B, int64_t capacity,
                      const int16_t *xy_new, const int64_t *t_new, const int8_t *p_new, const void *batch_new,
                      int32_t batch_is_int64, int64_t n_new, const int64_t *t_now /* [B] or NULL */, int64_t window_us,
                      float *pos_out, float *feat_out, int32_t *batch_out, int32_t *n_dev, int32_t *lane_count /* [B] */,
                      int32_t *status, void *stream);
int dagr_stream_stage_capped(const dagr_graph_desc *desc, void *workspace, void *state, int32_t B, int64_t capacity,
                             const int16_t *xy_new, const int64_t *t_new, const int8_t *p_new, const void *batch_new,
                             int32_t batch_is_int64, int64_t n_new, const int64_t *t_now /* [B] or NULL */,
                             int64_t window_us, int64_t max_lane_events,
                             int64_t *lane_dropped /* [B], device, accumulated; may be NULL */, float *pos_out,
                             float *feat_out, int32_t *batch_out, int32_t *n_dev, int32_t *lane_count /* [B] */,
                             int32_t *status, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream front: raw sensor events, downsampled on the device
 *   The models read events_2x streams: the sensor's events through the integrate-and-fire loop of
 *   scripts/downsample_events.py:91-124 (every cell of fx x fy sensor pixels adds p / (fx * fy) to its fp32 state; an event
 *   that brings |state| to 1 survives at (x / fx, y / fy) and its polarity is subtracted), then cut to the model's rows
 *   (DSEC.preprocess_events).  dagr_stream_downsample does this to a push of raw events of B lanes and leaves the survivors
 *   and their count in device memory; dagr_stream_stage_dev is dagr_stream_stage reading that count from the device.
 *   Five launches and a library radix sort, no host synchronisation.
 *
 * The cell grid is cells_w x cells_h = (sensor_w / fx) x (sensor_h / fy) and must cover the model's width x height.  Every
 * lane owns a change map fp32[cells_h, cells_w], carried from push to push.  A lane's raw events pass through their cells'
 * integrators in arrival order -- the arithmetic of dagr_downsample_events, one device function --; a survivor whose cell is
 * outside width x height is dropped silently (its cell integrates all the same), and so is an event in the strip right of /
 * below the last whole cell.  A raw event outside [0, sensor_w) x [0, sensor_h) is dropped and raises bit 4 (value 16) of
 * `status`, the stream's status word.  The survivors keep the order of the push.
 *
 * front: dagr_stream_front_bytes(B, cells_w, cells_h, max_push) bytes (0: sizes out of range), dagr_stream_front_reset
 *        before the first push, after a change of max_push and to zero the maps.  The change maps are its first
 *        B * cells_h * cells_w floats (a caller that needs a larger max_push copies them into the new state after its
 *        reset); keys, run order, keep flags, their prefix sums and the sort's storage for max_push events follow.
 * xy_raw int16[n_raw,2] (4-byte aligned) sensor pixels, t_raw int64[n_raw], p_raw int8[n_raw] in {-1, +1}, batch_raw
 * int32/int64[n_raw]; outputs for n_raw events: xy_out int16[.,2] (4-byte aligned), t_out int64, p_out int8, batch_out
 * int32, *n_out = the number of survivors.  All in device memory.
 *
 * dagr_stream_stage_dev: the new events are the first *n_new_dev (clamped to 0..n_new_max) of xy_new / t_new / p_new /
 * batch_new (int32); the clock is t_clock / batch_clock (int32/int64, n_clock events) -- the raw push --, which the order
 * checks (bits 0 and 3) run on and the lanes' newest timestamps (t_last, and t_ref without t_now) come from.  Everything
 * else as dagr_stream_stage, which is this entry with the new events as their own clock.  n_new_max, n_clock <= capacity.
 * dagr_stream_stage_dev_capped is to it what dagr_stream_stage_capped is to dagr_stream_stage: the cap counts the new
 * events it is given (behind dagr_stream_downsample: the survivors), capacity >= B * max_lane_events replaces the bounds on
 * n_new_max and n_clock (both < 2^30).
 * ------------------------------------------------------------------------ */
size_t dagr_stream_front_bytes(int32_t B, int32_t cells_w, int32_t cells_h, int64_t max_push);
int dagr_stream_front_reset(void *front, size_t front_bytes, int32_t B, int32_t cells_w, int32_t cells_h, int64_t max_push,
                            void *stream);
int dagr_stream_downsample(void *front, size_t front_bytes, int32_t B, int64_t max_push, int32_t fx, int32_t fy,
                           int32_t sensor_w, int32_t sensor_h, int32_t width, int32_t height, const int16_t *xy_raw,
                           const int64_t *t_raw, const int8_t *p_raw, const void *batch_raw, int32_t batch_is_int64,
                           int64_t n_raw, int16_t *xy_out, int64_t *t_out, int8_t *p_out, int32_t *batch_out,
                           int32_t *n_out, int32_t *status, void *stream);
int dagr_stream_stage_dev(const dagr_graph_desc *desc, void *workspace, void *state, int32_t B, int64_t capacity,
                          const int16_t *xy_new, const int64_t *t_new, const int8_t *p_new, const int32_t *batch_new,
                          const int32_t *n_new_dev, int64_t n_new_max, const int64_t *t_clock, const void *batch_clock,
                          int32_t clock_is_int64, int64_t n_clock, const int64_t *t_now /* [B] or NULL */,
                          int64_t window_us, float *pos_out, float *feat_out, int32_t *batch_out, int32_t *n_dev,
                          int32_t *lane_count /* [B] */, int32_t *status, void *stream);
int dagr_stream_stage_dev_capped(const dagr_graph_desc *desc, void *workspace, void *state, int32_t B, int64_t capacity,
                                 const int16_t *xy_new, const int64_t *t_new, const int8_t *p_new, const int32_t *batch_new,
                                 const int32_t *n_new_dev, int64_t n_new_max, const int64_t *t_clock,
                                 const void *batch_clock, int32_t clock_is_int64, int64_t n_clock,
                                 const int64_t *t_now /* [B] or NULL */, int64_t window_us, int64_t max_lane_events,
                                 int64_t *lane_dropped /* [B], device, accumulated; may be NULL */, float *pos_out,
                                 float *feat_out, int32_t *batch_out, int32_t *n_dev, int32_t *lane_count /* [B] */,
                                 int32_t *status, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream noise filter: background activity and hot pixels, removed on the device
 *   A raw sensor stream carries isolated background-activity events and hot pixels.  dagr_stream_denoise filters a push of
 *   raw events of B lanes in front of dagr_stream_downsample / dagr_stream_stage_dev and leaves the survivors and their count
 *   in device memory.  Three launches of its own, the project's one-launch scan and a library radix sort, no host
 *   synchronisation.
 *
 * Every lane owns a stamp map int64[sensor_h, sensor_w], carried from push to push: the t of the last event on the pixel,
 * or "never" = INT64_MIN.  A lane's events are taken in arrival order.  An event (x, y, t) inside the sensor is
 *   supported  (denoise_us = D > 0) if a pixel of its 8-neighbourhood -- the centre excluded, pixels outside the sensor do
 *              not exist, nothing wraps into the next row or lane -- has a stamp s != never with t - s <= D; with D = 0
 *              (off) every event is supported;
 *   refractory (refractory_us = R > 0) if its own pixel has a stamp s != never with t - s < R; with R = 0 (off) none is;
 *   kept       iff supported and not refractory; then stamp[y, x] = t, kept or not.
 * Every event stamps, so a decision depends on the timestamps of earlier events only: the same sequence in any chunking
 * leaves the same survivors and the same maps.  "Earlier" is arrival order: of two events with one timestamp the second sees
 * the first.  All time arithmetic is int64.  An event outside [0, sensor_w) x [0, sensor_h) is dropped, does not stamp and
 * raises bit 4 (value 16) of `status`, the stream's status word; an event whose lane is outside [0, B) is dropped and does
 * not stamp (dagr_stream_stage_dev flags it on the clock).  The survivors keep the order of the push.
 *
 * state: dagr_stream_denoise_bytes(B, sensor_w, sensor_h, max_push) bytes (0: sizes out of range -- B in 1..127,
 *        B * sensor_w * sensor_h < 2^31, max_push in 1..2^25 - 1), dagr_stream_denoise_reset before the first push, after a
 *        change of max_push and to empty the maps.  The stamps are its first B * sensor_h * sensor_w int64 (a caller that
 *        needs a larger max_push copies them into the new state after its reset); keys, sorted order, keep flags, their
 *        prefix sums and the sort's storage for max_push events follow.
 * xy_raw int16[n_raw,2] (4-byte aligned) sensor pixels, t_raw int64[n_raw] non-decreasing inside a lane, p_raw int8[n_raw],
 * batch_raw int32/int64[n_raw] sorted; outputs for n_raw events, none of them an input: xy_out int16[.,2] (4-byte aligned),
 * t_out int64, p_out int8, batch_out int32, *n_out = the number of survivors.  Rows *n_out .. n_raw - 1 of xy_out are (0, 0)
 * and of batch_out -1: dagr_stream_downsample, which takes its count from the host, can be given all n_raw rows and drops
 * those silently.  lane_filtered int64[B] (may be NULL): the lane's events inside the sensor that were not kept are added
 * to it by plain stores of the lane's thread; the caller zeroes it.  All in device memory.
 * DAGR_ERR_INVALID_ARG before any launch: sizes out of range, negative denoise_us / refractory_us or both 0,
 * n_raw > max_push, a state smaller than dagr_stream_denoise_bytes, NULL pointers.
 * ------------------------------------------------------------------------ */
size_t dagr_stream_denoise_bytes(int32_t B, int32_t sensor_w, int32_t sensor_h, int64_t max_push);
int dagr_stream_denoise_reset(void *state, size_t state_bytes, int32_t B, int32_t sensor_w, int32_t sensor_h,
                              int64_t max_push, void *stream);
int dagr_stream_denoise(void *state, size_t state_bytes, int32_t B, int64_t max_push, int32_t sensor_w, int32_t sensor_h,
                        int64_t denoise_us /* 0: off */, int64_t refractory_us /* 0: off */, const int16_t *xy_raw,
                        const int64_t *t_raw, const int8_t *p_raw, const void *batch_raw, int32_t batch_is_int64,
                        int64_t n_raw, int16_t *xy_out, int64_t *t_out, int8_t *p_out, int32_t *batch_out, int32_t *n_out,
                        int64_t *lane_filtered /* [B], device, accumulated; may be NULL */, int32_t *status, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream anti-flicker and trail filters: two per-pixel state machines, run on the device
 *   Mains- and PWM-driven lights make their pixels emit ON / OFF bursts at a steady rate, and an edge crossing a pixel fires
 *   a burst of same-polarity events of which the first carries the information.  dagr_stream_flicker removes both from a
 *   push of raw events of B lanes, in front of dagr_stream_denoise / dagr_stream_downsample / dagr_stream_stage_dev, and
 *   leaves the survivors and their count in device memory.  Three launches of its own, the project's one-launch scan and a
 *   library radix sort, no host synchronisation, no floating point.  The rule below is this project's statement of two
 *   well-known filters; agreement with any vendor's filter is not claimed.
 *
 * Every pixel of every lane carries, from push to push: t_edge int64 (never = INT64_MIN), last_p (0, +1, -1), count
 * (0..255), blocking; t_pass int64 (never), p_pass (0, +1, -1) -- initially never / 0 / 0 / false / never / 0.  A lane's
 * events are taken in arrival order; of two events with one timestamp the second sees the first.  An event (t, p) inside the
 * sensor on a lane in [0, B), with s = +1 if p > 0 else -1:
 *   flicker stage (max_period_us > 0):
 *     1. stale: if t_edge != never and t - t_edge > max_period_us, count = 0;
 *     2. edge iff s > 0 and last_p < 0.  On an edge with t_edge != never and d = t - t_edge: count = min(count + 1,
 *        max_count) if min_period_us <= d <= max_period_us, count = max(count - 1, 0) if d < min_period_us.  On every
 *        edge t_edge = t;
 *     3. if count >= start, blocking = true; else if count <= stop, blocking = false;
 *     4. last_p = s;
 *     5. a blocking pixel's event is removed (outcome 1) and does not reach the trail stage;
 *   trail stage (trail_us > 0), for what passed the flicker stage, or for every event when that stage is off:
 *     trail = p_pass == s and t - t_pass < trail_us (a never t_pass is not subtracted); then t_pass = t and p_pass = s,
 *     trailed or not; a trailing event is removed (outcome 2).
 * Everything else is kept.  All arithmetic is int64.  The same sequence in any chunking into pushes leaves the same
 * survivors and the same state.  An event outside [0, sensor_w) x [0, sensor_h) or with a lane outside [0, B) -- the
 * lane-less rows a stage in front leaves behind its count among them -- is dropped, meets no state and is not counted; an
 * event outside the sensor on a lane in [0, B) raises bit 4 (value 16) of `status`, the stream's status word.  The survivors
 * keep the order of the push.
 *
 * state: dagr_stream_flicker_bytes(B, sensor_w, sensor_h, max_push) bytes (0: sizes out of range -- B in 1..127,
 *        B * sensor_w * sensor_h < 2^31, max_push in 1..2^25 - 1), dagr_stream_flicker_reset before the first push, after a
 *        change of max_push and to return every pixel to its initial state.  The per-pixel maps come first, each over
 *        [B, sensor_h, sensor_w]: with S = 8 * B * sensor_h * sensor_w rounded up to a multiple of 256, t_edge int64 at
 *        offset 0, t_pass int64 at offset S, and at offset 2 * S one int32 word per pixel: bits 0..7 count, bit 8
 *        blocking, bits 9..10 last_p, bits 11..12 p_pass (a polarity field is 0: none yet, 1: +1, 2: -1).  A caller that
 *        needs a larger max_push copies these 2 * S + 4 * B * sensor_h * sensor_w bytes into the new state after its
 *        reset; keys, sorted order, keep flags, their prefix sums, outcomes and the sort's storage for max_push events
 *        follow.
 * min_period_us / max_period_us: the edge periods that count, 1 <= min <= max <= 1000000; max_period_us = 0 turns the
 * flicker stage off (min_period_us, start, stop and max_count are then ignored).  0 <= stop < start <= max_count <= 255.
 * trail_us > 0, or 0 for off; both stages off is an error.
 * xy_raw int16[n_raw,2] (4-byte aligned) sensor pixels, t_raw int64[n_raw] non-decreasing inside a lane, p_raw int8[n_raw],
 * batch_raw int32/int64[n_raw] sorted; outputs for n_raw events, none of them an input: xy_out int16[.,2] (4-byte aligned),
 * t_out int64, p_out int8, batch_out int32, *n_out = the number of survivors, written on the device.  Rows *n_out ..
 * n_raw - 1 of xy_out are (0, 0) and of batch_out -1, as dagr_stream_denoise leaves them; nothing is written past n_raw;
 * n_raw = 0 only zeroes *n_out.  lane_flicker / lane_trail int64[B] (each may be NULL): the lane's events removed by the
 * flicker / the trail stage are added to them with vector atomics; the caller zeroes them.  All in device memory.
 * DAGR_ERR_INVALID_ARG before any launch: sizes out of range, periods, thresholds or trail_us out of range or both stages
 * off, n_raw > max_push, a state smaller than dagr_stream_flicker_bytes, NULL pointers.
 * ------------------------------------------------------------------------ */
size_t dagr_stream_flicker_bytes(int32_t B, int32_t sensor_w, int32_t sensor_h, int64_t max_push);
int dagr_stream_flicker_reset(void *state, size_t state_bytes, int32_t B, int32_t sensor_w, int32_t sensor_h,
                              int64_t max_push, void *stream);
int dagr_stream_flicker(void *state, size_t state_bytes, int32_t B, int64_t max_push, int32_t sensor_w, int32_t sensor_h,
                        int64_t min_period_us, int64_t max_period_us /* 0: off */, int32_t start, int32_t stop,
                        int32_t max_count, int64_t trail_us /* 0: off */, const int16_t *xy_raw, const int64_t *t_raw,
                        const int8_t *p_raw, const void *batch_raw, int32_t batch_is_int64, int64_t n_raw, int16_t *xy_out,
                        int64_t *t_out, int8_t *p_out, int32_t *batch_out, int32_t *n_out,
                        int64_t *lane_flicker /* [B], device, accumulated; may be NULL */,
                        int64_t *lane_trail /* [B], device, accumulated; may be NULL */, int32_t *status, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream decoder: the camera's EVT 3.0 / EVT 2.0 words, decoded on the device
 *   An event camera delivers words, not (x, y, t, p) arrays: EVT 2.0 is one 32-bit word per event plus time words, EVT 3.0
 *   a stateful stream of 16-bit words with run-length vectors.  dagr_stream_decode turns a push of words of B lanes into
 *   the rows dagr_stream_denoise / dagr_stream_downsample / dagr_stream_stage_dev_clock take and leaves them and their count
 *   in device memory.  Three launches, no host synchronisation, integer arithmetic only.  The formats are stated in
 *   dagr_amd/streaming.py (module docstring) from the vendor's public descriptions as recalled; DecodeDefinition there is the
 *   yardstick, and agreement with a real camera file has not been demonstrated.
 *
 * Every lane owns a decoder state, carried from push to push: int64[8] = high, low, loops, y, base_x (uint32 arithmetic),
 * pol, synced, 0.  A lane's words are taken in order (type = w >> 12 for EVT 3.0, w >> 28 for EVT 2.0):
 *   EVT 3.0  0x0 ADDR_Y y = w & 0x7FF; 0x2 ADDR_X one event at x = w & 0x7FF with the word's bit 11 as polarity; 0x3
 *            VECT_BASE_X base_x = w & 0x7FF, pol = bit 11; 0x4 VECT_12 / 0x5 VECT_8 an event at base_x + i for every set bit
 *            i < 12 / 8 in ascending order with the state's pol, then base_x += 12 / 8; 0x6 TIME_LOW low = w & 0xFFF; 0x8
 *            TIME_HIGH v = w & 0xFFF, loops += 1 if synced and high - v >= 2048, then high = v, synced = 1; every other
 *            type is skipped.  t = t_base[b] + (loops << 24) + (high << 12) + low.
 *   EVT 2.0  0x0 / 0x1 CD_OFF / CD_ON one event at x = (w >> 11) & 0x7FF, y = w & 0x7FF, polarity = type, low6 =
 *            (w >> 22) & 0x3F; 0x8 TIME_HIGH v = w & 0x0FFFFFFF, loops += 1 if synced and high - v >= 2^27, then high = v,
 *            synced = 1; every other type is skipped.  t = t_base[b] + (loops << 34) + (high << 6) + low6.
 * An emitted event is dropped and counted as unsynced if synced == 0; else dropped, counted as outside and flagged (bit 4,
 * value 16) unless x < sensor_w and y < sensor_h; else it is a decoded row (x, y, t, p = pol ? +1 : -1, lane b).  Dropped
 * events take no output row.  The rows keep word order, bit order inside a vector word, and lane order.  The result depends
 * on the word sequence only: any chunking of a lane's words into pushes gives the same rows, counters and final state.
 *
 * state: dagr_stream_decode_bytes(B, max_words) bytes (0: out of range -- B in 1..127, max_words in 1..2^25 - 1),
 *        dagr_stream_decode_reset before the first push and to zero the lanes' states.  The states are its first
 *        B * 8 int64 (a caller that needs a larger max_words copies them into the new state after its reset); a copy of
 *        them and one summary, one carried summary and one count per tile of DAGR_DECODE_TILE words follow.
 * words uint16 (EVT 3.0) / uint32 (EVT 2.0), little-endian, aligned to the word size, the lanes' runs concatenated;
 * word_end int64[B] the cumulative end of each lane's run, non-decreasing, last == n_words; t_base int64[B] or NULL (0).
 * Outputs for max_out rows: xy_out int16[.,2] (4-byte aligned), t_out int64, p_out int8, batch_out int32, *n_out =
 * min(decoded events, max_out).  If the push decodes more than max_out events the first max_out are written, the states
 * and counters advance as if all had been, and bit 6 (value 64) of `status` is raised.  Rows *n_out .. max_out - 1 of
 * xy_out are (0, 0) and of batch_out -1, as dagr_stream_denoise leaves them.  lane_counts int64[B, 4] (may be NULL):
 * decoded, unsynced, outside, skipped are added to it; the caller zeroes it.  All in device memory.
 * A word_end that is not non-decreasing, exceeds n_words or does not end at n_words is clamped on the device and raises
 * bit 3 (value 8); words behind the last lane's end are ignored.  No index leaves the buffers.
 * DAGR_ERR_INVALID_ARG before any launch: unknown format, sizes out of range (sensor_w, sensor_h in 1..32767),
 * n_words > max_words, max_out < 1 or >= 2^30, a state smaller than dagr_stream_decode_bytes, NULL pointers, words not
 * aligned to its word size.
 *
 * dagr_stream_stage_dev_clock / dagr_stream_stage_dev_clock_capped: dagr_stream_stage_dev / _capped with the clock's
 * length on the device too: the clock has clamp(*n_clock_dev, 0, n_clock) events.  A decoded push is its own clock and only
 * the device knows its length.
 * ------------------------------------------------------------------------ */
#define DAGR_DECODE_EVT2 2
#define DAGR_DECODE_EVT3 3
#define DAGR_DECODE_TILE 1024
size_t dagr_stream_decode_bytes(int32_t B, int64_t max_words);
int dagr_stream_decode_reset(void *state, size_t state_bytes, int32_t B, int64_t max_words, void *stream);
int dagr_stream_decode(void *state, size_t state_bytes, int32_t B, int64_t max_words, int32_t format, int32_t sensor_w,
                       int32_t sensor_h, const void *words, const int64_t *word_end /* [B], device */, int64_t n_words,
                       const int64_t *t_base /* [B], device, or NULL */, int64_t max_out, int16_t *xy_out, int64_t *t_out,
                       int8_t *p_out, int32_t *batch_out, int32_t *n_out,
                       int64_t *lane_counts /* [B, 4], device, accumulated; may be NULL */, int32_t *status, void *stream);
int dagr_stream_stage_dev_clock(const dagr_graph_desc *desc, void *workspace, void *state, int32_t B, int64_t capacity,
                                const int16_t *xy_new, const int64_t *t_new, const int8_t *p_new, const int32_t *batch_new,
                                const int32_t *n_new_dev, int64_t n_new_max, const int64_t *t_clock, const void *batch_clock,
                                int32_t clock_is_int64, const int32_t *n_clock_dev, int64_t n_clock,
                                const int64_t *t_now /* [B] or NULL */, int64_t window_us, float *pos_out, float *feat_out,
                                int32_t *batch_out, int32_t *n_dev, int32_t *lane_count /* [B] */, int32_t *status,
                                void *stream);
int dagr_stream_stage_dev_clock_capped(const dagr_graph_desc *desc, void *workspace, void *state, int32_t B,
                                       int64_t capacity, const int16_t *xy_new, const int64_t *t_new, const int8_t *p_new,
                                       const int32_t *batch_new, const int32_t *n_new_dev, int64_t n_new_max,
                                       const int64_t *t_clock, const void *batch_clock, int32_t clock_is_int64,
                                       const int32_t *n_clock_dev, int64_t n_clock, const int64_t *t_now /* [B] or NULL */,
                                       int64_t window_us, int64_t max_lane_events,
                                       int64_t *lane_dropped /* [B], device, accumulated; may be NULL */, float *pos_out,
                                       float *feat_out, int32_t *batch_out, int32_t *n_dev, int32_t *lane_count /* [B] */,
                                       int32_t *status, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream frames: raw sensor frames, prepared on the device
 *   DSEC.preprocess_image (crop, bicubic shrink by a whole factor, back to uint8) and format_data's `/ 255` in one launch,
 *   for n frames at once: rows [0, fy * height) and columns [0, fx * width) of every uint8 [frame_h, frame_w, 3] frame are
 *   shrunk to width x height, the channels reversed if `bgr`, and written as fp32 in [0, 1] into lane lanes[k] of `out`.
 *
 * Per axis with factor f, output pixel d reads the four taps base - 1 .. base + 2, base = f * d + (f - 1) / 2, clamped to the
 * CROP (not to the frame), with the weights (-3, 19, 19, -3) / 32 for even f and (0, 1, 0, 0) for odd f: torch's bicubic
 * interpolation (A = -0.75, align_corners off) at these factors.  The 16-tap sum is an exact integer over 1024; it is
 * rounded half to even, clamped to [0, 255] and divided by 255.0f (a correctly rounded division).
 *
 * frames: frame k starts at frames + k * frame_stride, its rows are row_stride >= 3 * frame_w bytes apart, a pixel is three
 * consecutive bytes.  lanes int32[n] in device memory.  out: element (b, c, y, x) at b * stride_b + c * stride_c +
 * y * stride_y + x * stride_x floats, b in [0, B).  A lane outside [0, B) writes nothing and raises bit 5 (value 32) of
 * `status`, the stream's status word.  One thread per output pixel; n <= 65535, height <= 65535, fx * width and
 * fy * height <= 32767.  DAGR_ERR_INVALID_ARG before the launch: a frame smaller than the crop, strides smaller than the
 * frame, sizes out of range, NULL pointers.
 * ------------------------------------------------------------------------ */
int dagr_stream_frame(const uint8_t *frames, int64_t frame_stride, int64_t row_stride, int32_t n, const int32_t *lanes,
                      int32_t frame_w, int32_t frame_h, int32_t fx, int32_t fy, int32_t width, int32_t height, int32_t bgr,
                      float *out, int32_t B, int64_t stride_b, int64_t stride_c, int64_t stride_y, int64_t stride_x,
                      int32_t *status, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream tracker: the detections of a step get track ids, on the device
 *   A step's detection list says nothing about the step before.  dagr_stream_track associates the rows of every lane with
 *   the tracks the lane carries from step to step -- greedy IoU matching inside a label -- and writes a track id and a hit
 *   count per row.  One launch (one wave per lane), no host synchronisation.  dagr_amd/streaming.py: TrackDefinition is the
 *   same in numpy.
 *
 * A lane owns max_tracks slots, each free or holding a track: box fp32[4] (x1, y1, x2, y2), label int32, id int64 >= 1,
 * t_last int64, hits int32; and next_id int64, 1 after a reset (id 0 means "no track").  One call is one step of every
 * lane b on the rows det[b, 0 .. n_keep[b]) -- (x1, y1, x2, y2, score, label) fp32 as dagr_postprocess leaves them,
 * n_keep[b] clamped to 0..A -- at the instant t_ref[b]:
 *   never:    t_ref[b] = INT64_MIN (the lane has no reference instant yet): every row gets id 0 and hits 0, nothing else
 *             changes;
 *   retire:   a track with t_ref[b] - t_last > max_age_us is freed (an age equal to max_age_us stays; int64 arithmetic);
 *   eligible: rows with score >= min_score (a NaN score is not).  The first DAGR_TRACK_MAX_DETS eligible rows in row order
 *             take part; every further eligible row gets id 0 and adds 1 to untracked[b]; a row that is not eligible gets
 *             id 0 and is not counted;
 *   match:    the participating rows in row order, greedily: among the live tracks with the row's label ((int32_t)label)
 *             that no earlier row of this step has matched, the one with the largest IoU, the LOWEST id on a tie; if that
 *             IoU is >= iou the track takes the row's box, t_last = t_ref[b], hits += 1, and the row gets the track's id and
 *             hits.  A NaN IoU (0 / 0 of two empty boxes) never matches.  Labels are finite class indices, as
 *             dagr_postprocess writes them: the conversion of a NaN or out-of-int32-range label is not specified (the device
 *             gives 0 or a saturated value, numpy's astype INT32_MIN), and equality with the definition holds for finite ones;
 *   spawn:    after all rows have been matched, the participating rows that did not match take, in row order, the free slots
 *             in ascending slot order (slots freed by this step's retirement included): id = next_id++, hits = 1,
 *             t_last = t_ref[b].  Without a free slot the row gets id 0 and adds 1 to untracked[b].
 * The IoU of row a and track b, in fp32 and in this order, without contraction:
 *   iw = min(ax2, bx2) - max(ax1, bx1);  ih = min(ay2, by2) - max(ay1, by1);  (min / max hand a NaN operand on)
 *   inter = iw > 0 && ih > 0 ? iw * ih : 0;  uni = ((ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1)) - inter;
 *   iou = inter / uni  (a correctly rounded division).
 *
 * tracks: dagr_stream_track_bytes(B, max_tracks) bytes (0: B outside 1..65535 or max_tracks outside
 *         1..DAGR_TRACK_MAX_TRACKS), 16-byte aligned, dagr_stream_track_reset before the first step and to empty it.  With
 *         n = B * max_tracks it holds, back to back, slot s of lane b at index b * max_tracks + s:
 *           id     int64 [n]    at byte 0        (0: the slot is free, and its other fields mean nothing)
 *           t_last int64 [n]    at byte  8 * n
 *           box    fp32  [n, 4] at byte 16 * n
 *           label  int32 [n]    at byte 32 * n
 *           hits   int32 [n]    at byte 36 * n
 *           next_id int64 [B]   at byte 40 * n
 * track_id int64[B, A] and track_hits int32[B, A]: rows < n_keep[b] are written, the rest are left as they are.
 * untracked int64[B] (may be NULL): accumulated by plain stores of one thread per lane; the caller zeroes it.
 * det fp32[B, A, 6], n_keep int32[B], t_ref int64[B]; all in device memory.
 * DAGR_ERR_INVALID_ARG before any launch: B or max_tracks out of range, iou outside (0, 1], max_age_us < 0, A < 0, a state
 * smaller than dagr_stream_track_bytes, NULL or misaligned pointers.
 *
 * dagr_stream_t_ref: where t_ref[B] lives inside a dagr_stream_stage state (device memory; pointer arithmetic on the host,
 * nothing is launched or read), or NULL when B / capacity are out of range: the instants the last step left, which is what
 * a stream hands to dagr_stream_track after its step.
 * ------------------------------------------------------------------------ */
#define DAGR_TRACK_MAX_TRACKS 256
#define DAGR_TRACK_MAX_DETS 256
size_t dagr_stream_track_bytes(int32_t B, int32_t max_tracks);
int dagr_stream_track_reset(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, void *stream);
int dagr_stream_track(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, float iou, int64_t max_age_us,
                      float min_score, const float *det, const int32_t *n_keep, int32_t A, const int64_t *t_ref,
                      int64_t *track_id, int32_t *track_hits, int64_t *untracked /* [B], accumulated; may be NULL */,
                      void *stream);
const int64_t *dagr_stream_t_ref(const void *state, int32_t B, int64_t capacity);

/* ------------------------------------------------------------------------ *
 * Event stream tracker with a constant-velocity motion model: tracks survive a gap, and coast
 *   dagr_stream_track_cv is dagr_stream_track with a velocity per track: the rows are matched against the boxes the
 *   tracks are PREDICTED to have at t_ref[b], a match filters box and velocity, every row also gets the filtered box and the
 *   velocity of its track, and the live tracks a step did not see leave their prediction in the lane's coast list.  One
 *   launch (one wave per lane) in place of dagr_stream_track's, no host synchronisation.  dagr_amd/streaming.py:
 *   TrackDefinition(motion=) is the same in numpy, bit for bit.
 *
 * A slot additionally holds vel fp32[4], pixels per microsecond per corner (x1, y1, x2, y2); zero in a free and in a
 * freshly spawned slot.  never / retire / eligible / spawn and the IoU are dagr_stream_track's (a retired slot's vel is
 * zeroed; a spawned track's is 0).  Added or replaced, all fp32 arithmetic in this order and without contraction:
 *   predict:  after the retirement and before any row, for every live track: dt = (float)(t_ref[b] - t_last) -- the int64
 *             difference converted to the nearest fp32, ties to even; exact for a live track, whose age is at most
 *             max_age_us <= DAGR_TRACK_CV_MAX_AGE_US, unless the clock went backwards -- and pred[k] = box[k] + vel[k] * dt
 *             for the four corners (one multiply, then one add).  Predictions depend on the state from before the step
 *             only; they are computed once per slot.
 *   match:    dagr_stream_track's, with iou(row, pred) in place of iou(row, box).  On a match, with z the row's box and
 *             r[k] = z[k] - pred[k]:  if dt > 0: q[k] = r[k] / dt (correctly rounded), and vel[k] = q[k] when the track's
 *             hits was 1 (its first continuation), else vel[k] = vel[k] + beta * q[k];  if dt <= 0 vel stays.
 *             box = z when alpha == 1, else box[k] = pred[k] + alpha * r[k].  t_last = t_ref[b], hits += 1.  The row gets
 *             the track's id and hits, track_box = box and track_vel = vel, both after the update.
 *   rows without a track (id 0) and rows that spawn one: track_box is the row's own box, track_vel is 0 -- also in a lane
 *             whose t_ref is INT64_MIN, where additionally n_coast[b] = 0.
 *   coast:    last.  The live tracks that no row matched in this step and that were not spawned in it, in ascending slot
 *             order: coast_id[b, j], coast_box[b, j] = pred, coast_label[b, j], coast_age_us[b, j] = t_ref[b] - t_last
 *             (int64), and n_coast[b] their number.  Entries at and behind n_coast[b] are left as they are.  Coasting changes
 *             no state.
 *
 * tracks: dagr_stream_track_cv_bytes(B, max_tracks) bytes (0 out of range, as dagr_stream_track_bytes), 16-byte aligned,
 *         dagr_stream_track_cv_reset before the first step and to empty it.  A layout of its own; with n = B * max_tracks,
 *         slot s of lane b at index b * max_tracks + s:
 *           id     int64 [n]    at byte 0        (0: the slot is free)
 *           t_last int64 [n]    at byte  8 * n
 *           box    fp32  [n, 4] at byte 16 * n
 *           vel    fp32  [n, 4] at byte 32 * n
 *           label  int32 [n]    at byte 48 * n
 *           hits   int32 [n]    at byte 52 * n
 *           next_id int64 [B]   at byte 56 * n      -- 56 * n + 8 * B bytes in all
 * alpha: position gain in (0, 1]; beta: velocity gain in [0, 1].
 * track_box, track_vel fp32[B, A, 4], 16-byte aligned: rows < n_keep[b] are written, the rest are left as they are (so are
 * track_id and track_hits).  coast_id int64[B, max_tracks], coast_box fp32[B, max_tracks, 4] (16-byte aligned), coast_label
 * int32[B, max_tracks], coast_age_us int64[B, max_tracks], n_coast int32[B]: all five NULL together (no coast list is
 * written) or none.  Everything else as dagr_stream_track takes it.
 * DAGR_ERR_INVALID_ARG before any launch: whatever dagr_stream_track refuses, alpha outside (0, 1], beta outside [0, 1]
 * (NaN included), max_age_us > DAGR_TRACK_CV_MAX_AGE_US, a state smaller than dagr_stream_track_cv_bytes, NULL track_box /
 * track_vel with A > 0, partly NULL coast arrays, misaligned arrays.
 * ------------------------------------------------------------------------ */
#define DAGR_TRACK_CV_MAX_AGE_US 16777215
size_t dagr_stream_track_cv_bytes(int32_t B, int32_t max_tracks);
int dagr_stream_track_cv_reset(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, void *stream);
int dagr_stream_track_cv(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, float iou, int64_t max_age_us,
                         float min_score, float alpha, float beta, const float *det, const int32_t *n_keep, int32_t A,
                         const int64_t *t_ref, int64_t *track_id, int32_t *track_hits, float *track_box, float *track_vel,
                         int64_t *coast_id, float *coast_box, int32_t *coast_label, int64_t *coast_age_us, int32_t *n_coast,
                         int64_t *untracked /* [B], accumulated; may be NULL */, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream tracker, second association round: rows under min_score may continue a track
 *   dagr_stream_track_rescue is dagr_stream_track, and dagr_stream_track_cv_rescue is dagr_stream_track_cv, with a second
 *   round of matching for the rows whose score has dipped under min_score (two-round association, as ByteTrack has it).
 *   Confident rows are matched first and only they start tracks; the low rows may then continue the tracks that are still
 *   unmatched.  One launch (one wave per lane) in place of the base entry's, no host synchronisation.
 *   dagr_amd/streaming.py: TrackDefinition(rescue=) is the same in numpy, bit for bit.
 *
 * Each entry works on the SAME state as its base entry: dagr_stream_track[_cv]_bytes and _reset serve it, the layout is
 * unchanged.  The order of a step: never, retire, (predict), round one, round two, spawn, (coast).  never / retire /
 * eligible / match / spawn, and with _cv predict / filter / coast, are the base entry's over the rows with
 * score >= min_score (the HIGH rows); added:
 *   low rows: score >= low_score && !(score >= min_score); a NaN score is in neither band, score == low_score is low,
 *             score == min_score is high.  The first DAGR_TRACK_MAX_DETS low rows in row order take part.  Every other low
 *             row, and every low row that does not match, gets what a row that is not eligible gets: id 0 and hits 0, with
 *             _cv track_box = its own box and track_vel = 0; it is NOT counted in untracked[b];
 *   round two: after every high row has been matched and before any spawn, the participating low rows in row order,
 *             greedily, by the rule of `match`: among the live tracks with the row's label that no row of this step, of
 *             either round, has matched, the one with the largest IoU (against box; with _cv against pred), the LOWEST id on
 *             a tie; a match if that IoU is >= low_iou; a NaN IoU never matches.  A match does exactly what a match of
 *             round one does (box, t_last, hits += 1, the row's outputs; with _cv the same velocity and alpha filter, and
 *             the track does not coast), and adds 1 to rescued[b];
 *   spawn:    takes the unmatched HIGH rows only: a low row never matches a track spawned in its own step and never
 *             occupies a slot.  Where a row stands in det does not decide its round.
 * Unlike ByteTrack, round two considers every live unmatched track, not only those seen in the step before.
 *
 * low_score: the lower edge of the band, below min_score.  low_iou: round two's own threshold in (0, 1] (pass iou for the
 * tracker's).  rescued int64[B] (8-byte aligned; may be NULL): accumulated by plain stores of one thread per lane; the
 * caller zeroes it.  Everything else as the base entry takes it.
 * DAGR_ERR_INVALID_ARG before any launch: whatever the base entry refuses, a NaN low_score, low_score >= min_score (the
 * band would be empty), low_iou outside (0, 1] (NaN included), a misaligned rescued.
 * ------------------------------------------------------------------------ */
int dagr_stream_track_rescue(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, float iou, int64_t max_age_us,
                             float min_score, const float *det, const int32_t *n_keep, int32_t A, const int64_t *t_ref,
                             int64_t *track_id, int32_t *track_hits, int64_t *untracked /* [B], accumulated; may be NULL */,
                             float low_score, float low_iou, int64_t *rescued /* [B], accumulated; may be NULL */,
                             void *stream);
int dagr_stream_track_cv_rescue(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, float iou, int64_t max_age_us,
                                float min_score, float alpha, float beta, const float *det, const int32_t *n_keep, int32_t A,
                                const int64_t *t_ref, int64_t *track_id, int32_t *track_hits, float *track_box,
                                float *track_vel, int64_t *coast_id, float *coast_box, int32_t *coast_label,
                                int64_t *coast_age_us, int32_t *n_coast,
                                int64_t *untracked /* [B], accumulated; may be NULL */, float low_score, float low_iou,
                                int64_t *rescued /* [B], accumulated; may be NULL */, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream tracker, optimal assignment: the match of a round as a one-to-one assignment, not greedily
 *   dagr_stream_track_optimal is any of the four entries above -- flags says which -- with the MATCH of a round replaced:
 *   the rows of the round and the lane's slots are paired by dagr_assign_max_weight's method, so that the round has the most
 *   matches possible and, among those, the largest sum of IoUs.  Greedy matching in row order gives a track to the first
 *   row that wants it and may leave a later row, which overlaps that track alone, without one.  One launch (one wave per
 *   lane) in place of the greedy entry's, no host synchronisation, no atomics.  dagr_amd/streaming.py:
 *   TrackDefinition(assign="optimal") is the same in numpy, bit for bit.
 *
 * It works on the SAME states as the greedy entries: dagr_stream_track[_cv]_bytes and _reset serve it.  never / retire /
 * eligible / the DAGR_TRACK_MAX_DETS cut / predict / filter / low rows / spawn / coast / rescued are stated above and
 * unchanged.  For a round (round one: the participating high rows at the threshold iou; with DAGR_TRACK_OPTIMAL_RESCUE
 * round two: the participating low rows at low_iou):
 *   weights:  w int32[rows of the round in row order, max_tracks slots in slot order].  w[r, s] = (1 << 29) + q if slot s is
 *             live (after the retirement), no earlier round of this step took it, its label is the row's and
 *             v = iou(row, box[s]) -- with DAGR_TRACK_OPTIMAL_MOTION iou(row, pred[s]) -- satisfies v >= the round's
 *             threshold (a NaN never does); q = (int32_t)(v * 1048576.0f), one fp32 multiply and a truncating conversion:
 *             the IoU is quantised to 2^-20.  Every other entry is 0.  256 * 2^20 < 2^29: one more match outweighs every
 *             IoU; every weight is below 2^31.
 *   pairing:  row_col of dagr_assign_max_weight's method on w (n_rows = the round's rows, n_cols = max_tracks; more rows
 *             than slots: the transposed matrix).  The pairing is the definition's: the device routine makes
 *             assign_max_weight_definition's comparisons one for one -- the same relaxation, the lowest column on a tie, the
 *             same transposition -- and tests/test_assign_pairing_gpu.py holds row_col equal entry for entry on matrices
 *             full of ties.  Track ids depend on it.
 *   apply:    every pair (row, slot) does exactly what a match of the greedy entry does (box or filter, t_last, hits += 1,
 *             the row's outputs; in round two rescued[b] += 1).  Pairs do not interact: any order leaves the same state.
 *             Round one's rows without a pair spawn in row order, round two's get no id.
 * Most-matches-first is this project's choice.  It is not SORT's rule, which solves on all pairs and then drops the pairs
 * under the threshold.
 *
 * flags: DAGR_TRACK_OPTIMAL_MOTION (bit 0) selects dagr_stream_track_cv's state layout and motion model,
 *        DAGR_TRACK_OPTIMAL_RESCUE (bit 1) the second round.  Without bit 0 alpha, beta, track_box, track_vel and the five
 *        coast arrays are not looked at and may be 0 / NULL; without bit 1 low_score, low_iou and rescued are not looked at.
 *        With a bit set its arguments are what dagr_stream_track_cv / the _rescue entries take, refused as there.
 * ws:    dagr_stream_track_optimal_bytes(B, max_tracks) bytes (0: B outside 1..65535 or max_tracks outside
 *        1..DAGR_TRACK_MAX_TRACKS), 16-byte aligned, caller-owned, means nothing between calls.  Lane b owns
 *        2 * DAGR_TRACK_MAX_DETS * max_tracks int32 words at word b * 2 * DAGR_TRACK_MAX_DETS * max_tracks: first the weight
 *        matrix of the round being matched, w[r, s] at word r * max_tracks + s, then, DAGR_TRACK_MAX_DETS * max_tracks words
 *        on, the transposed copy the method wants when the round has more rows than the lane has slots.
 * Everything else as dagr_stream_track_cv_rescue takes it.
 * DAGR_ERR_INVALID_ARG before any launch: unknown bits in flags; whatever dagr_stream_track refuses; with bit 0 whatever
 * dagr_stream_track_cv adds (partly NULL coast arrays among it), with bit 1 whatever the _rescue entries add; a NULL,
 * misaligned or too small workspace.
 * ------------------------------------------------------------------------ */
#define DAGR_TRACK_OPTIMAL_MOTION 1
#define DAGR_TRACK_OPTIMAL_RESCUE 2
size_t dagr_stream_track_optimal_bytes(int32_t B, int32_t max_tracks);
int dagr_stream_track_optimal(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, float iou, int64_t max_age_us,
                              float min_score, float alpha, float beta, const float *det, const int32_t *n_keep, int32_t A,
                              const int64_t *t_ref, int64_t *track_id, int32_t *track_hits, float *track_box,
                              float *track_vel, int64_t *coast_id, float *coast_box, int32_t *coast_label,
                              int64_t *coast_age_us, int32_t *n_coast,
                              int64_t *untracked /* [B], accumulated; may be NULL */, float low_score, float low_iou,
                              int64_t *rescued /* [B], accumulated; may be NULL */, int32_t flags, void *ws,
                              size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream scorer: the track ids of a step against labelled boxes, on the device
 *   dagr_stream_score scores what a dagr_stream_track* entry left for a step -- det, n_keep, track_id and, optionally, the
 *   motion model's track_box -- against ground-truth boxes that carry an identity, and accumulates the CLEAR-MOT counts
 *   (Bernardin & Stiefelhagen): misses, false positives, identity switches, fragmentations.  The matcher is greedy in
 *   ground-truth row order inside a label, not a minimum-cost assignment; agreement with another MOT tool is not claimed.
 *   One launch (one wave per lane), no host synchronisation, no global atomics: the lane's wave owns the lane's state.
 *   dagr_amd/streaming.py: ScoreDefinition is the same in numpy, integer for integer.
 *
 * One call is one scored step of every lane b with n_gt[b] >= 0 (n_gt[b] < 0: the lane has no labels at this instant and
 * not one byte of its state or of its outputs changes; n_gt[b] > G is clamped):
 *   hypotheses: the rows i < clamp(n_keep[b], 0, A) with track_id[b, i] != 0, in row order; the first DAGR_TRACK_MAX_DETS
 *             take part, each further one adds 1 to unscored_hyp.  A row without an id is neither a match nor a false
 *             positive.  The box is det's, or track_box[b, i] when track_box is given; the label is (int32_t)det[b, i, 5];
 *   slots:    the ground-truth rows in row order.  Unscored (outcome -1, unscored_gt += 1, takes part in nothing): gt_id <= 0,
 *             an earlier row of this step with the same gt_id, or a new identity and a full table.  Otherwise the row finds
 *             its slot by id, or takes slot n_objects++;
 *   keep:     the scored rows in row order whose object has seen_step == steps - 1 and prev_hyp != 0: the FIRST hypothesis
 *             row with that id is kept if it is still free, has the row's label and iou(gt, hyp) >= iou; kept += 1;
 *   match:    the remaining scored rows in row order: among the free hypotheses of the row's label the largest
 *             iou(gt, hyp) >= iou, the LOWEST row on a tie; a NaN IoU matches nothing.  The IoU is dagr_stream_track's,
 *             with a the ground-truth box and b the hypothesis;
 *   count:    per scored row gt += 1, present += 1, seen_step = steps.  Matched to track h: match += 1,
 *             iou_q += (int64)rintf(iou * 1048576.0f); switch iff last_hyp != 0 && last_hyp != h (switch += 1,
 *             switches += 1); fragmentation iff tracked > 0 && prev_hyp == 0 (frag += 1, frags += 1); then tracked += 1,
 *             last_hyp = prev_hyp = h.  Unmatched: miss += 1, prev_hyp = 0.  An absent object's slot is untouched.  Then
 *             hyp += participating hypotheses, false_pos += those left free, steps += 1.
 *
 * state: dagr_stream_score_bytes(B, max_objects) bytes (0: B outside 1..65535 or max_objects outside
 *        1..DAGR_SCORE_MAX_OBJECTS), 16-byte aligned, dagr_stream_score_reset before the first step and to empty it.  With
 *        n = B * max_objects it holds, back to back, slot s of lane b at index b * max_objects + s, all int64:
 *          id        [n] at byte  0        (the ground-truth identity, > 0; slots at and behind n_objects[b] mean nothing)
 *          last_hyp  [n] at byte  8 * n    (the track id of the object's last match ever; 0: none)
 *          prev_hyp  [n] at byte 16 * n    (the track id of its match at its last scored step; 0: a miss)
 *          seen_step [n] at byte 24 * n    (the lane's `steps` at its last scored step; -1: never)
 *          present   [n] at byte 32 * n
 *          tracked   [n] at byte 40 * n
 *          switches  [n] at byte 48 * n
 *          frags     [n] at byte 56 * n
 *          lane      [B, 16] at byte 64 * n: n_objects, steps, gt, hyp, match, miss, false_pos, switch, frag, kept, iou_q,
 *                    unscored_gt, unscored_hyp, and three words that stay 0 -- 64 * n + 128 * B bytes in all
 * det fp32[B, A, 6], n_keep int32[B], track_id int64[B, A]; track_box fp32[B, A, 4], 16-byte aligned, or NULL: det's boxes.
 * gt_box fp32[B, G, 4] (x1, y1, x2, y2; 16-byte aligned), gt_label int32[B, G], gt_id int64[B, G], n_gt int32[B],
 * 0 <= G <= DAGR_SCORE_MAX_GT.  gt_match int64[B, G] (the track id, 0: a miss, -1: unscored) and gt_flags int32[B, G] (bit
 * 0 switch, bit 1 fragmentation, bit 2 kept): both NULL or both given; rows at and behind n_gt[b] are left as they are.
 * All in device memory.
 * DAGR_ERR_INVALID_ARG before any launch: B, max_objects, G or A out of range, iou outside (0, 1] (NaN included), a state
 * smaller than dagr_stream_score_bytes, NULL or misaligned arrays, only one of gt_match / gt_flags.
 * ------------------------------------------------------------------------ */
#define DAGR_SCORE_MAX_OBJECTS 1024
#define DAGR_SCORE_MAX_GT 256
size_t dagr_stream_score_bytes(int32_t B, int32_t max_objects);
int dagr_stream_score_reset(void *state, size_t bytes, int32_t B, int32_t max_objects, void *stream);
int dagr_stream_score(void *state, size_t bytes, int32_t B, int32_t max_objects, float iou,
                      const float *det, const int32_t *n_keep, int32_t A, const int64_t *track_id,
                      const float *track_box /* [B, A, 4] or NULL: det's boxes */,
                      const float *gt_box, const int32_t *gt_label, const int64_t *gt_id, const int32_t *n_gt, int32_t G,
                      int64_t *gt_match, int32_t *gt_flags, void *stream);

/* ------------------------------------------------------------------------ *
 * Maximum-weight bipartite assignment, on the device
 *   dagr_assign_max_weight pairs rows with columns one to one so that the sum of w over the pairs is the largest possible,
 *   for B independent matrices in one launch (one wave per matrix), no host synchronisation, no global atomics.
 *   dagr_amd/streaming.py: assign_max_weight_definition is the same method in numpy.
 *
 * Matrix b is w[b, :n_rows[b], :n_cols[b]] of w int32[B, ld_rows, ld] (row r of matrix b starts at (b * ld_rows + r) * ld),
 * every weight >= 0 (a negative weight is the caller's error and is not detected), 0 <= n_rows[b] <= max_rows <= ld_rows,
 * 0 <= n_cols[b] <= max_cols <= ld, max_rows and max_cols in 1..DAGR_ASSIGN_MAX; a count outside its range is clamped.
 * The method is the Hungarian method by shortest augmenting paths in integers on the cost -w, with the smaller side as
 * rows: a matrix with n_rows > n_cols is first transposed into the workspace.  Potentials are int64.  One row enters at a
 * time; a path step marks column j0 used, relaxes minv[j] = min(minv[j], cost[p[j0], j] - u[p[j0]] - v[j]) over the unused
 * columns, takes delta = the smallest minv, the LOWEST column on a tie, moves the potentials by delta and goes on from that
 * column until it is free; then the path is flipped.
 * total int64[B]: the largest sum, which is unique.  row_col int32[B, max_rows]: for r < n_rows[b] the column paired with
 * row r in ONE pairing that reaches it, or -1 (no pair, or a pair of weight 0); -1 for the rows behind n_rows[b].  The
 * pairing is not unique: it is one-to-one, lists only pairs with w > 0 and sums to total.  WHICH pairing comes back is
 * fixed, though: the pairing is the definition's, assign_max_weight_definition's row_col entry for entry (the same walk,
 * comparison for comparison; tests/test_assign_pairing_gpu.py).  dagr_stream_track_optimal relies on that.
 * workspace: dagr_assign_workspace_bytes(B, max_rows, max_cols) bytes (0: a size out of range), 16-byte aligned; it holds
 * the transposed matrices, int32[B, max_cols, max_rows], and means nothing between calls.  All in device memory.
 * DAGR_ERR_INVALID_ARG before any launch: B outside 1..65535, max_rows / max_cols outside 1..DAGR_ASSIGN_MAX, ld_rows <
 * max_rows, ld < max_cols, a workspace smaller than dagr_assign_workspace_bytes, NULL or misaligned arrays.
 * ------------------------------------------------------------------------ */
#define DAGR_ASSIGN_MAX 1024
size_t dagr_assign_workspace_bytes(int32_t B, int32_t max_rows, int32_t max_cols);
int dagr_assign_max_weight(const int32_t *w, int32_t B, int32_t ld_rows, int32_t ld, const int32_t *n_rows,
                           const int32_t *n_cols, int32_t max_rows, int32_t max_cols, int32_t *row_col, int64_t *total,
                           void *workspace, size_t bytes, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream identity state: IDF1 (Ristani et al., 2016) behind the scorer, on the device
 *   dagr_stream_identity runs after dagr_stream_score on the same step's arrays and counts, per lane, how many steps every
 *   (object identity, track id) pair overlapped; dagr_stream_identity_solve runs dagr_assign_max_weight's method on those
 *   counts: idtp is the largest number of frames a one-to-one pairing of identities with track ids can share.
 *   idf1 = 2 idtp / (gt_frames + hyp_frames), idp = idtp / hyp_frames, idr = idtp / gt_frames are the caller's divisions.
 *   One launch each (one wave per lane), no host synchronisation, no global atomics.  dagr_amd/streaming.py:
 *   IdentityDefinition is the same in numpy, integer for integer.  Agreement with another MOT tool is not claimed.
 *
 * One dagr_stream_identity call is one step of every lane b with n_gt[b] >= 0 (n_gt[b] < 0: not one byte of the lane
 * changes):
 *   hypotheses: dagr_stream_score's rule -- the rows i < clamp(n_keep[b], 0, A) with track_id[b, i] != 0, the first
 *             DAGR_TRACK_MAX_DETS in row order, box and label as there.  A row whose id an earlier participating row of this
 *             step carries takes no part, dup_hyp += 1; every other row counts hyp_frames += 1;
 *   columns:  in row order a hypothesis finds its column by id, or takes column n_tracks++; with a full table it gets no
 *             column and unlisted_hyp += 1.  With a column track_len[col] += 1;
 *   rows:     the rows g < min(n_gt[b], G) with gt_match[b, g] != -1 and gt_id[b, g] > 0 whose gt_id is in the first n_objects
 *             slots of the scorer's id table; slot = that index.  gt_frames += 1, obj_len[slot] += 1,
 *             n_objects = max(n_objects, slot + 1);
 *   pairs:    for every such row and every hypothesis with a column, when the labels are equal and iou(gt, hyp) >= iou
 *             (dagr_stream_score's IoU; a NaN IoU overlaps nothing): overlap[slot, col] += 1, pairs += 1.  Every overlapping
 *             pair counts, not a one-to-one match.  Then steps += 1.
 *
 * state: dagr_stream_identity_bytes(B, max_objects, max_tracks) bytes (0: B outside 1..65535, max_objects outside
 *        1..DAGR_SCORE_MAX_OBJECTS or max_tracks outside 1..DAGR_ASSIGN_MAX), 16-byte aligned, dagr_stream_identity_reset
 *        before the first step and to empty it (all zero).  With M = max_objects and T = max_tracks it holds, back to back:
 *          track_id  int64 [B, T]    at byte 0                (the track id of a column, != 0; columns at and behind n_tracks: 0)
 *          track_len int64 [B, T]    at byte  8 * B * T       (the steps at which the column's track was a hypothesis)
 *          obj_len   int64 [B, M]    at byte 16 * B * T       (the steps at which the object of a slot was a row)
 *          lane      int64 [B, 8]    at byte 16 * B * T + 8 * B * M: n_tracks, n_objects, gt_frames, hyp_frames, dup_hyp,
 *                                    unlisted_hyp, pairs, steps
 *          overlap   int32 [B, M, T] at byte 16 * B * T + 8 * B * M + 64 * B
 *          obj_col   int32 [B, M]    behind it (the last solve's pairing as columns, -1: none; 0 after a reset)
 *        -- 16 * B * T + 8 * B * M + 64 * B + 4 * B * M * T + 4 * B * M bytes, rounded up to a multiple of 16.
 * score_state: dagr_stream_score's state of the same B and max_objects AFTER its step (read only: the id table and n_objects).
 * det, n_keep, A, track_id, track_box, gt_box, gt_label, gt_id, n_gt, G: as dagr_stream_score takes them; gt_match
 * int64[B, G] is what it wrote (read only here).
 * dagr_stream_identity_solve: obj_track int64[B, max_objects] (the track id paired with the object of a slot, 0: none) and
 * result int64[B, DAGR_IDENTITY_RESULT_WORDS]: idtp, idfn = gt_frames - idtp, idfp = hyp_frames - idtp, gt_frames,
 * hyp_frames, n_objects, n_tracks, dup_hyp, unlisted_hyp.  workspace: dagr_assign_workspace_bytes(B, max_objects,
 * max_tracks).  The state's counts are not changed: a solve can be asked for at any step.
 * DAGR_ERR_INVALID_ARG before any launch: sizes out of range, iou outside (0, 1] (NaN included), a state or workspace too
 * small, NULL or misaligned arrays.
 * ------------------------------------------------------------------------ */
#define DAGR_IDENTITY_RESULT_WORDS 9
size_t dagr_stream_identity_bytes(int32_t B, int32_t max_objects, int32_t max_tracks);
int dagr_stream_identity_reset(void *state, size_t bytes, int32_t B, int32_t max_objects, int32_t max_tracks, void *stream);
int dagr_stream_identity(void *state, size_t bytes, int32_t B, int32_t max_objects, int32_t max_tracks, float iou,
                         const void *score_state, size_t score_bytes,
                         const float *det, const int32_t *n_keep, int32_t A, const int64_t *track_id,
                         const float *track_box /* [B, A, 4] or NULL: det's boxes */,
                         const float *gt_box, const int32_t *gt_label, const int64_t *gt_id, const int32_t *n_gt, int32_t G,
                         const int64_t *gt_match, void *stream);
int dagr_stream_identity_solve(void *state, size_t bytes, int32_t B, int32_t max_objects, int32_t max_tracks,
                               int64_t *obj_track, int64_t *result, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream HOTA state (Luiten et al., "HOTA: a higher order metric for evaluating multi-object tracking", IJCV 2021)
 * behind the identity step, on the device
 *   HOTA needs two passes: the matching of an instant is weighted by an alignment score of (object, track) pairs that is
 *   known only when the whole sequence has been seen.  dagr_stream_hota runs after dagr_stream_identity on the same step's
 *   arrays: pass 1 and the append of the instant to the lane's log.  dagr_stream_hota_solve replays the log with the final
 *   tables: one maximum-weight assignment (dagr_assign_max_weight's method, entry for entry) per logged instant, the counts
 *   at the 19 thresholds alpha = k / 20, and the fp64 sums behind AssA, AssRe and AssPr.  DetA, AssA, LocA and
 *   HOTA = sqrt(DetA * AssA) are the caller's divisions.  dagr_amd/streaming.py: HotaDefinition is the same in numpy,
 *   integer for integer.  No host synchronisation.
 *   THIS PROJECT'S statement of HOTA departs from the usual tool: the similarities are quantised to 2^-20, the alignment
 *   score is floored to 2^-20 and the weight to 2^-30, a pair of weight 0 is never matched, there is no epsilon at the
 *   thresholds, the labels gate the similarity, and the instants behind max_instants are left out.  Agreement with
 *   TrackEval is not claimed.
 *
 * One dagr_stream_hota call is one instant of every lane b with n_gt[b] >= 0 (n_gt[b] < 0: not one byte of the lane changes):
 *   participants: what dagr_stream_identity used at this step.  Rows: the rows g < min(n_gt[b], G) with gt_match[b, g] != -1
 *             and gt_id[b, g] > 0 whose gt_id is in the first n_objects slots of the scorer's id table, in row order; slot s
 *             = that index.  Columns: the first DAGR_TRACK_MAX_DETS rows i < clamp(n_keep[b], 0, A) with track_id != 0,
 *             without those whose id an earlier one carries, whose id is in the first n_tracks columns of the identity
 *             state's track table (as dagr_stream_identity left it at this step), in row order; c = that column.  Box and
 *             label as dagr_stream_score takes them;
 *   full log: with instants == max_instants the step only adds 1 to dropped_instants;
 *   similarity: q[g, i] = (int) rintf(iou(gt, hyp) * 1048576.0f), dagr_stream_score's IoU, and 0 when the labels differ or the
 *             IoU is NaN (or outside (0, 1], which only a box with a negative side gives);
 *   pass 1:   rs[g] and cs[i] the row and column sums of q; for q > 0: pmc[s, c] += (q << 20) / (rs[g] + cs[i] - q) (int64);
 *             gc[s] += 1 and tc[c] += 1 for every participant;
 *   append:   the participants' slot or column, box and label go to entry `instants` of the lane's log; instants += 1,
 *             rows += the rows, columns += the columns.
 * dagr_stream_hota_solve, per logged instant with the tables as they are:
 *   gq[s, c] = (pmc[s, c] << 20) / (((gc[s] + tc[c]) << 20) - pmc[s, c]), 0 where pmc is 0; w[g, i] = (gq * q[g, i]) >> 10,
 *   in 0 .. 2^30, compacted to the instant's rows and columns in log order; the pairing is dagr_assign_max_weight's.  For
 *   k = 1 .. 19 a matched pair is a TP when 20 * q >= k << 20: tp[k] += TPs, fn[k] += rows - TPs, fp[k] += columns - TPs,
 *   loc_q[k] += the TPs' q, mc[k][s, c] += 1 per TP.  Then per lane and k in fp64, over the pairs with mc > 0, one division
 *   then one multiplication a term: ass[k] = sum mc * (mc / (gc[s] + tc[c] - mc)), re[k] = sum mc * (mc / gc[s]),
 *   pr[k] = sum mc * (mc / tc[c]).  It first zeroes mc, the counters and the sums; the log, pmc, gc, tc and the words are not
 *   changed, so a solve can be asked for at any step and repeated.  The solve is one launch of at most
 *   DAGR_HOTA_SOLVE_WAVES one-wave workgroups that walk the instants of all lanes (integer atomics on mc and the
 *   counters: sums of integers do not depend on the order), and one launch of 19 * B workgroups for the fp64 sums: a
 *   thread adds its entries in index order and the workgroup's 256 partial sums are added in a fixed tree, so there is no
 *   fp64 atomic and no sum depends on how anything was scheduled.
 *
 * state: dagr_stream_hota_bytes(B, max_objects, max_tracks, max_instants) bytes (0: B outside 1..65535, max_objects outside
 *        1..DAGR_SCORE_MAX_OBJECTS, max_tracks outside 1..DAGR_ASSIGN_MAX or max_instants outside
 *        1..DAGR_HOTA_MAX_INSTANTS), 16-byte aligned, dagr_stream_hota_reset before the first step and to empty it (all
 *        zero).  With M = max_objects, T = max_tracks, I = max_instants and E = DAGR_HOTA_LOG_ENTRIES it holds, in this
 *        order, EACH ARRAY STARTING AT THE NEXT MULTIPLE OF 16 BYTES behind the one before it (the first at byte 0):
 *          pmc       int64 [B, M, T]      8 * B * M * T bytes
 *          gc        int64 [B, M]         8 * B * M      (the logged instants at which the object of a slot was a row)
 *          tc        int64 [B, T]         8 * B * T      (the logged instants at which the track of a column was a column)
 *          lane      int64 [B, 4]         32 * B         instants, dropped_instants, rows, columns
 *          count     int64 [B, 19, 4]     608 * B        tp, fn, fp, loc_q of threshold k at [b, k - 1] (the last solve's)
 *          sums      fp64  [B, 19, 3]     456 * B        ass, re, pr of threshold k at [b, k - 1] (the last solve's)
 *          log_box   fp32  [B, I, E, 4]   16 * B * I * E an instant's rows at entries 0 .., its columns at entries
 *                                                        DAGR_SCORE_MAX_GT ..
 *          log_n     int32 [B, I, 2]      8 * B * I      the instant's rows and columns
 *          log_index int32 [B, I, E]      4 * B * I * E  the slot of a row, the column of a column
 *          log_label int32 [B, I, E]      4 * B * I * E
 *          mc        int32 [B, 19, M, T]  76 * B * M * T (the last solve's)
 *        -- the sum of these, each rounded up to a multiple of 16.  dagr_amd/streaming.py refuses a stream whose state
 *        would exceed DAGR_HOTA_MAX_STATE_BYTES.
 * identity_state / score_state: the states of dagr_stream_identity and dagr_stream_score of the same B, max_objects and
 * max_tracks AFTER their steps (read only: the tables of track ids and object ids, n_tracks and n_objects).  det, n_keep,
 * A, track_id, track_box, gt_box, gt_label, gt_id, n_gt, G, gt_match: as dagr_stream_identity takes them.
 * workspace (the solve's): dagr_stream_hota_workspace_bytes(B, max_objects, max_tracks, max_instants) bytes (0: a size out
 * of range), 16-byte aligned: per wave of min(B * I, DAGR_HOTA_SOLVE_WAVES) the instant's weight matrix and the
 * assignment's transposed copy, 2 * min(M, DAGR_SCORE_MAX_GT) * min(T, DAGR_TRACK_MAX_DETS) int32; it means nothing
 * between calls.  All in device memory.
 * DAGR_ERR_INVALID_ARG before any launch: sizes out of range, a state or workspace too small, NULL or misaligned arrays.
 * ------------------------------------------------------------------------ */
#define DAGR_HOTA_THRESHOLDS 19
#define DAGR_HOTA_MAX_INSTANTS 65535
#define DAGR_HOTA_LOG_ENTRIES 512
#define DAGR_HOTA_SOLVE_WAVES 256
#define DAGR_HOTA_MAX_STATE_BYTES 1073741824
size_t dagr_stream_hota_bytes(int32_t B, int32_t max_objects, int32_t max_tracks, int32_t max_instants);
size_t dagr_stream_hota_workspace_bytes(int32_t B, int32_t max_objects, int32_t max_tracks, int32_t max_instants);
int dagr_stream_hota_reset(void *state, size_t bytes, int32_t B, int32_t max_objects, int32_t max_tracks,
                           int32_t max_instants, void *stream);
int dagr_stream_hota(void *state, size_t bytes, int32_t B, int32_t max_objects, int32_t max_tracks, int32_t max_instants,
                     const void *identity_state, size_t identity_bytes, const void *score_state, size_t score_bytes,
                     const float *det, const int32_t *n_keep, int32_t A, const int64_t *track_id,
                     const float *track_box /* [B, A, 4] or NULL: det's boxes */,
                     const float *gt_box, const int32_t *gt_label, const int64_t *gt_id, const int32_t *n_gt, int32_t G,
                     const int64_t *gt_match, void *stream);
int dagr_stream_hota_solve(void *state, size_t bytes, int32_t B, int32_t max_objects, int32_t max_tracks,
                           int32_t max_instants, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream label store: the ground truth of every step, interpolated between labelled keyframes on the device
 *   Labels arrive far more rarely than steps (DSEC: 20 Hz against a 1 kHz stream).  dagr_stream_labels_push keeps the
 *   labelled keyframes of every lane in a ring, and dagr_stream_labels_at writes, for every lane, the ground truth at the
 *   lane's own reference instant -- t_ref[b], a device array: dagr_stream_t_ref's -- into the arrays dagr_stream_score,
 *   dagr_stream_identity and dagr_stream_hota read.  The rule is the reference's inter-frame evaluation (interpolate_tracks:
 *   the boxes of the identities both frames hold, linear in x, y, w, h, in ascending identity; then filter_small_bboxes).
 *   Linear between keyframes, so wrong wherever the object's motion is not.  One launch each, no host synchronisation, no
 *   atomics.  dagr_amd/streaming.py: LabelDefinition is the same in numpy, bit for bit.
 *
 * A keyframe is an instant t (int64 microseconds, the stream's clock) and n <= max_rows rows of xywh fp64[4] (top-left plus
 * size), label int32 and id int64.  With K = max_keyframes and R = max_rows:
 *   push:  lane b takes the keyframes f = 0 .. F - 1 of the call in order: t[b, f], n[b, f], xywh[b, f, :, :], label[b, f, :],
 *          id[b, f, :], the arrays R rows wide.  n[b, f] < 0: none.  A keyframe whose t is not greater than the lane's newest
 *          keyframe instant is refused (refused += 1, nothing else).  Rows at and behind R are cut (cut_rows += n - R).  On a
 *          full ring the oldest keyframe is overwritten (overwritten += 1).
 *   at:    n_gt[b] = -1, nothing else written, and outside += 1 when t_ref[b] is INT64_MIN, the lane has no keyframe, or
 *          t_ref[b] is before the oldest resident keyframe or after the newest; likewise and gap += 1 when max_gap_us > 0
 *          and the bracketing keyframes are more than max_gap_us apart.  Otherwise labelled += 1 and, with t_k <= t_ref <
 *          t_k+1 the bracketing pair, the rows are the identities both keyframes hold -- only id > 0, an identity counts at
 *          its first row inside a keyframe -- in ascending identity: r = (double)(t_ref - t_k) / (double)(t_k+1 - t_k), every
 *          one of x, y, w, h is a * (1 - r) + b * r (two multiplies, one add, fp64, no contraction), the label is the
 *          earlier keyframe's.  t_ref == the newest keyframe's instant: that keyframe's rows with id > 0, first rows only,
 *          in ascending identity, as they are.  Then the small-box filter on the fp64 values: a row survives iff
 *          sqrt(h * h + w * w) > min_diag && w > min_height && h > min_height; a NaN min_diag / min_height switches that
 *          half off.  gt_box[b, i] = (float)x, (float)y, (float)(x + w), (float)(y + h), the sums in fp64; gt_label, gt_id;
 *          n_gt[b] = the rows written (0: labelled, but no row).  Rows at and behind n_gt[b] are left as they are.
 *
 * state: dagr_stream_labels_bytes(B, max_keyframes, max_rows) bytes (0: B or max_keyframes outside 1..65535, max_rows
 *        outside 1..DAGR_SCORE_MAX_GT), 16-byte aligned, dagr_stream_labels_reset before the first push and to empty it (it
 *        zeroes the words; what lies behind them means nothing until a push has written it).  It holds, each at the next
 *        multiple of 16 bytes behind the one before:
 *          lane  int64 [B, DAGR_LABELS_WORDS]: keyframes (resident), head (the ring index of the oldest), refused, cut_rows,
 *                overwritten, labelled, outside, gap
 *          t     int64 [B, K]          (resident keyframe i of lane b is ring index (head + i) % K, instants ascending)
 *          n     int32 [B, K]
 *          xywh  fp64  [B, K, R, 4]
 *          label int32 [B, K, R]
 *          id    int64 [B, K, R]
 * push: t int64[B, F], n int32[B, F], xywh fp64[B, F, R, 4] (16-byte aligned), label int32[B, F, R], id int64[B, F, R],
 * 1 <= F <= 65535.  at: t_ref int64[B]; gt_box fp32[B, R, 4] (16-byte aligned), gt_label int32[B, R], gt_id int64[B, R], n_gt
 * int32[B] -- G = max_rows for the scorer.  All in device memory.  Instants are expected to differ by less than 2^63.
 * DAGR_ERR_INVALID_ARG before any launch: sizes out of range, max_gap_us < 0, a state smaller than
 * dagr_stream_labels_bytes, NULL or misaligned arrays.
 * ------------------------------------------------------------------------ */
#define DAGR_LABELS_WORDS 8
size_t dagr_stream_labels_bytes(int32_t B, int32_t max_keyframes, int32_t max_rows);
int dagr_stream_labels_reset(void *state, size_t bytes, int32_t B, int32_t max_keyframes, int32_t max_rows, void *stream);
int dagr_stream_labels_push(void *state, size_t bytes, int32_t B, int32_t max_keyframes, int32_t max_rows, int32_t F,
                            const int64_t *t, const int32_t *n, const double *xywh, const int32_t *label, const int64_t *id,
                            void *stream);
int dagr_stream_labels_at(void *state, size_t bytes, int32_t B, int32_t max_keyframes, int32_t max_rows,
                          const int64_t *t_ref, int64_t max_gap_us, double min_height, double min_diag,
                          float *gt_box, int32_t *gt_label, int64_t *gt_id, int32_t *n_gt, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream mAP: the evaluated images logged on the device, and the COCO protocol's job list built from the log
 *   dagr_stream_map_log appends, for every lane, the step's detections and ground truth to a log of fixed capacity in a
 *   caller-owned state -- one launch of one wave per lane, no atomics, no host synchronisation -- and dagr_stream_map_plan
 *   turns the log, where it lies, into everything dagr_coco_match and dagr_coco_accumulate (below) take, in the order of
 *   utils/coco_eval.py:build_jobs.  dagr_amd/streaming.py: MapDefinition is the log's rule in numpy, bit for bit; the
 *   metric's definition is utils/coco_eval.py:evaluate_detection on its images.
 *
 * An image is one (lane, instant).  With I = max_images, D = max_dets, and the step's det fp32[B, A, 6] (x1, y1, x2, y2,
 * score, label) / n_keep int32[B], gt_box fp32[B, G, 4] (x1, y1, x2, y2) / gt_label int32[B, G] / n_gt int32[B] (as
 * dagr_stream_labels_at writes them) and t_ref int64[B]:
 *   log:   lane b is logged only if n_gt[b] > 0 (metrics only where there is a box: evaluated_images' rule); n_gt[b] < 0:
 *          unlabelled += 1, n_gt[b] == 0: empty += 1, nothing else.  A lane that holds I images already: dropped_images += 1,
 *          nothing else.  Otherwise the image takes the lane's next slot: its t_ref[b], its first min(n_gt[b], G)
 *          ground-truth rows and labels, and its first min(n_keep[b], D) detection rows in det order (n_keep clamped to
 *          0 .. A); cut_dets += the rows cut.  Rows are kept as the 32-bit words they are.
 *   order: the images of the protocol are lane-major -- all of lane 0's in log order, then lane 1's, ... -- which matters
 *          only for ties in score.
 *   plan:  a detection row counts for class c iff its label == (float)c, a ground-truth row iff its label == c; labels
 *          outside [0, n_classes) belong to no job.  A job is one (class, area range, image) with at least one row of the
 *          class, ordered by class, then area range, then image.  (x, y, w, h) = x1, y1, x2 - x1, y2 - y1 with the
 *          subtraction in fp32 and then widened, as utils/coco_eval.py:_xywh does.
 *
 * state: dagr_stream_map_bytes(B, I, G, D) bytes (0: B outside 1..65535, I outside 1..DAGR_MAP_MAX_IMAGES, G outside
 *        1..DAGR_COCO_MAX_GT, D outside 1..DAGR_COCO_MAX_DT, or B * I * (G + 2 D + 256) >= 2^31 - 1: every offset of the plan is
 *        an int32), 16-byte aligned, dagr_stream_map_reset before the first log and to empty it (it zeroes the words; what lies
 *        behind them means nothing until a log has written it).  It holds, each at the next multiple of 16 bytes behind the
 *        one before:
 *          lane     int64 [B, DAGR_MAP_WORDS]: images (logged), dropped_images, cut_dets, unlabelled, empty
 *          t        int64 [B, I]
 *          n_gt     int32 [B, I]
 *          n_dt     int32 [B, I]
 *          gt_box   fp32  [B, I, G, 4]
 *          gt_label int32 [B, I, G]
 *          det      fp32  [B, I, D, 6]
 * log: A in 1..DAGR_COCO_MAX_DT; gt_box 16-byte aligned.  Because G and D are bounded here, no job of the plan ever exceeds
 * dagr_coco_match's per-job bounds.
 *
 * plan: n_classes in 1..DAGR_MAP_MAX_CLASSES with B * I * n_classes < 2^28; area_rngs fp64[n_areas, 2] (the host's
 * AREA_RNG, never recomputed here), n_areas in 1..DAGR_MAP_MAX_AREAS; max_dets_per_job the protocol's cut (MAX_DETS),
 * 1..DAGR_COCO_MAX_DETS; workspace of dagr_stream_map_plan_workspace_bytes(B, I, n_classes) bytes (0: out of range), 16-byte
 * aligned, contents irrelevant.  Outputs, every one sized from the capacities (N = B * I, P = N * min(n_classes, G + D)
 * pairs at most, K = N * min(D, max_dets_per_job * n_classes) columns an area range at most):
 *   gt_xywh fp64[N * G, 4], dt_xywh fp64[N * D, 4], dt_score fp64[N * D]: the rows of an (image, class) once, shared by its
 *                           area ranges, class after class and inside a class image after image, in row order
 *   jobs int64[n_areas * P, 6], area_rng fp64[n_areas * P, 2]: dagr_coco_match's, the columns and g_ign entries of ALL jobs
 *                           laid out in job order (column_layout)
 *   job_info int64[n_areas * P, DAGR_MAP_JOB_WORDS]: group = class * n_areas + area range, kept = min(D of the job,
 *                           max_dets_per_job), first column, first g_ign entry
 *   col_group int64[n_areas * K], entry_group int64[n_areas * N * G]: the group of every column / g_ign entry
 *   group_ptr int64[n_classes * n_areas + 1]: dagr_coco_accumulate's (accumulate_groups)
 *   totals int64[DAGR_MAP_TOTALS]: n_jobs, n_gt, n_dt, n_out, n_gign, the largest G and the largest D of a job, and the
 *                           detection rows the log holds (in a class or not)
 * Entries behind the totals' counts are left as they are.  Count, scan (csrc/scan.hip), scatter: five launches and a
 * memset, grids bounded by the capacity, the rows touched bounded by the lanes' words on the device (the count arrays, four
 * ints per (slot, class), are scanned whole); every position is a prefix sum, so no atomic decides an order.  No host
 * synchronisation.  All arrays are device memory.  The totals come from ONE workgroup of 1024 threads that walks all
 * B * I * n_classes pairs and all B * I slots, whatever the log holds: its length grows with the capacity, not with the
 * lanes' words -- measured up to 76800 pairs (B = 8, I = 1200, two classes, the whole plan 16 ms with match and
 * accumulate), NOT measured near the 2^28 limit, where it would take about 2^18 iterations a thread.
 * The class rule for detections (label == (float)c) deliberately differs from DetectionBuffer's truncation for labels that
 * are no whole number: 0.5 counts for no class here and for class 0 there.  The engine writes whole labels.
 * DAGR_ERR_INVALID_ARG before any launch: sizes out of range, a state or workspace that is too small, NULL or misaligned
 * arrays.
 * ------------------------------------------------------------------------ */
#define DAGR_MAP_WORDS 5
#define DAGR_MAP_MAX_IMAGES 65535
#define DAGR_MAP_MAX_CLASSES 256
#define DAGR_MAP_MAX_AREAS 8
#define DAGR_MAP_JOB_WORDS 4
#define DAGR_MAP_TOTALS 8
size_t dagr_stream_map_bytes(int32_t B, int32_t max_images, int32_t G, int32_t max_dets);
int dagr_stream_map_reset(void *state, size_t bytes, int32_t B, int32_t max_images, int32_t G, int32_t max_dets, void *stream);
int dagr_stream_map_log(void *state, size_t bytes, int32_t B, int32_t max_images, int32_t G, int32_t max_dets,
                        const float *det, const int32_t *n_keep, int32_t A, const float *gt_box, const int32_t *gt_label,
                        const int32_t *n_gt, const int64_t *t_ref, void *stream);
size_t dagr_stream_map_plan_workspace_bytes(int32_t B, int32_t max_images, int32_t n_classes);
int dagr_stream_map_plan(const void *state, size_t bytes, int32_t B, int32_t max_images, int32_t G, int32_t max_dets,
                         int32_t n_classes, const double *area_rngs, int32_t n_areas, int32_t max_dets_per_job,
                         void *workspace, size_t workspace_bytes, double *gt_xywh, double *dt_xywh, double *dt_score,
                         int64_t *jobs, double *area_rng, int64_t *job_info, int64_t *col_group, int64_t *entry_group,
                         int64_t *group_ptr, int64_t *totals, void *stream);

/* ------------------------------------------------------------------------ *
 * Event stream picture: events, boxes, track ids and trails of a step, drawn on the device
 *   dagr_stream_render paints one uint8 BGR frame [H, W, 3] per lane from what a stream keeps on the device -- the
 *   resident raw events of a dagr_stream_stage state, the step's det / n_keep, the tracker's track_id, and the trail rings
 *   dagr_stream_trail keeps from the tracker's slots.  Three launches at most, no host synchronisation, and no result that
 *   depends on the order of execution: every pixel is decided independently.  The look is this project's own;
 *   dagr_amd/streaming.py: RenderDefinition is the same in numpy, byte for byte.
 *
 * Layers of lane b, in this order:
 *   1 base:    base[b] (base + b * base_stride bytes; base_stride 0: one image for every lane), or 0 when base is NULL.
 *   2 events:  (state != NULL) the lane's resident events -- the segment seg[b] of the current raw set, in arrival order --
 *              with t <= t_ref[b] and t_ref[b] - t < event_window_us (int64; event_window_us < 0: every resident event).  A
 *              lane with t_ref[b] = INT64_MIN draws none.  An event whose p - 1 lies outside [-3, 2] is dropped (status bit
 *              0); one outside [0, W) x [0, H) is skipped.  A pixel hit by at least one of them becomes, as dagr_viz_render
 *              states it, trunc(alpha * v) on its three channels, then channel p - 1 (wrapped like a Python index) of the
 *              LAST such event gets trunc(that + 255 * (1 - alpha)); float64.
 *   3 trails:  (rings != NULL) ring (b, s) with at least two points draws the segments between consecutive points, oldest
 *              first.  Segment P0 -> P1 with dx = x1 - x0, dy = y1 - y0, n = max(|dx|, |dy|): the pixels k = 0 .. n along
 *              the major axis (x when |dx| >= |dy|), major = major0 + sign(dmajor) * k, minor = minor0 + sign(dminor) *
 *              ((2 * k * |dminor| + n) / (2 * n)) (integer division; n = 0: the point itself), clipped to the image.  A
 *              segment with n > W + H is not drawn (status bit 2).  A pixel on several trails takes the one of the HIGHEST
 *              slot, in the colour of the ring's id (below).
 *   4 boxes:   the rows r < min(n_keep[b], A) of det[b] (x1, y1, x2, y2, score, label), in row order, a later row on top.
 *              A row with a non-finite coordinate is skipped.  Corners: (int32_t)floorf(clamp(v, -2^20, 2^20)); the
 *              rectangle is [min(x1, x2), max(x1, x2)] x [min(y1, y2), max(y1, y2)] = [xa, xb] x [ya, yb], and a pixel
 *              belongs to the outline by dagr_viz_render's rule: Chebyshev distance to the rectangle's border <=
 *              linewidth / 2.  Colour: with track_id, colors[0] for id 0, else colors[1 + (id - 1) % (n_colors - 1)] (the
 *              id as an unsigned 64-bit number); without, colors[(int32_t)label], and a label outside [0, n_colors) skips
 *              the row (status bit 1).
 *   5 plates:  (ids != 0, track_id != NULL) the same rows with id != 0, in row order, a later row on top, above every
 *              outline.  Text: the decimal digits of id % 1000000 (unsigned), nd of them, no leading zeros.  With s =
 *              id_scale the plate is (4 * nd + 1) * s wide and 7 * s high, its left edge at xa, its rows ya - 7 * s ..
 *              ya - 1, or, when ya - 7 * s < 0, ya + 1 .. ya + 7 * s; filled with the row's colour.  Digit d (0: the most
 *              significant) is the 3 x 5 glyph below scaled by s with its top-left at (xa + (1 + 4 * d) * s, top + s), in
 *              black.  Clipped to the image per pixel.
 * DAGR_RENDER_GLYPH_<d>: 15 bits, row major, bit 14 the top-left pixel and bit 0 the bottom-right one.
 *
 * rings: dagr_stream_trail_bytes(B, max_tracks, trail) bytes (0: B outside 1..65535, max_tracks outside
 *        1..DAGR_TRACK_MAX_TRACKS or trail outside 1..DAGR_RENDER_MAX_TRAIL), 8-byte aligned, dagr_stream_trail_reset before
 *        the first step and to empty them.  With n = B * max_tracks, ring (b, s) at index i = b * max_tracks + s:
 *          id    int64 [n]           at byte 0       (0: the ring is empty)
 *          count int32 [n]           at byte  8 * n  (points appended so far; the point appended at count c sits at
 *                                                     c % trail, so the ring's points are, oldest first, 0 .. count - 1
 *                                                     while count <= trail and then (count + j) % trail, j = 0 .. trail - 1;
 *                                                     a count that reaches 2^30 goes on from trail + 2^30 % trail)
 *          pt    int32 [n, trail, 2] at byte 12 * n  (x, y)
 * dagr_stream_trail, one launch behind the tracker's on the slots it left (tracks / tracks_bytes: a dagr_stream_track or
 * a dagr_stream_track_cv state, told apart by tracks_bytes, which must be the one's or the other's _bytes), per slot:
 * a free slot (id 0) empties its ring; a slot whose id differs from the ring's restarts the ring under the slot's id;
 * then, if t_ref[b] != INT64_MIN and the slot's t_last == t_ref[b] (the step saw the track; a coasting track appends
 * nothing), the centre cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f of the slot's box (fp32, no contraction) is appended
 * as (int32_t)clamp(floorf(c), -2^20, 2^20), unless cx or cy is not finite.
 *
 * dagr_stream_render: state / capacity a dagr_stream_stage state (NULL: no events); det fp32 [B, A, 6] and n_keep int32
 * [B] (A = 0: no rows, both may then be NULL); track_id int64 [B, A] or NULL; rings or NULL (then max_tracks and trail are
 * not read); alpha in [0, 1]; linewidth 1..DAGR_RENDER_MAX_LINEWIDTH; id_scale 1..DAGR_RENDER_MAX_ID_SCALE; colors uint8
 * [n_colors, 3] BGR, 2 <= n_colors <= 256; out uint8 [B, H, W, 3], which may be base when base_stride != 0 or B = 1 (a thread
 * reads its pixel before it writes it); status one int32, OR-ed into (the caller zeroes it).  workspace:
 * dagr_stream_render_workspace_bytes(B, H, W) bytes (0: B outside 1..65535, H or W < 1 or H * W > 2^29), 256-byte aligned,
 * ALL ZERO before the first call; every call leaves it zero again, so no call clears it.  It holds two int32 maps over
 * [B, H, W]: the arrival index + 1 of the last drawn event on the pixel and the highest trail slot + 1 (integer
 * atomicMax, so the order of execution does not matter).  A flagged frame is unspecified; nothing faults.
 * DAGR_ERR_INVALID_ARG before any launch: sizes or options out of range, a workspace or rings smaller than their _bytes,
 * NULL or misaligned pointers.
 * ------------------------------------------------------------------------ */
#define DAGR_RENDER_MAX_TRAIL 64
#define DAGR_RENDER_MAX_LINEWIDTH 7
#define DAGR_RENDER_MAX_ID_SCALE 4
#define DAGR_RENDER_BAD_POLARITY 1
#define DAGR_RENDER_BAD_CLASS 2
#define DAGR_RENDER_LONG_SEGMENT 4
enum {
    DAGR_RENDER_GLYPH_0 = 0x7b6f, DAGR_RENDER_GLYPH_1 = 0x2c97, DAGR_RENDER_GLYPH_2 = 0x73e7, DAGR_RENDER_GLYPH_3 = 0x73cf,
    DAGR_RENDER_GLYPH_4 = 0x5bc9, DAGR_RENDER_GLYPH_5 = 0x79cf, DAGR_RENDER_GLYPH_6 = 0x79ef, DAGR_RENDER_GLYPH_7 = 0x7249,
    DAGR_RENDER_GLYPH_8 = 0x7bef, DAGR_RENDER_GLYPH_9 = 0x7bcf
};
size_t dagr_stream_trail_bytes(int32_t B, int32_t max_tracks, int32_t trail);
int dagr_stream_trail_reset(void *rings, size_t bytes, int32_t B, int32_t max_tracks, int32_t trail, void *stream);
int dagr_stream_trail(void *rings, size_t bytes, int32_t B, int32_t max_tracks, int32_t trail, const void *tracks,
                      size_t tracks_bytes, const int64_t *t_ref, void *stream);
size_t dagr_stream_render_workspace_bytes(int32_t B, int32_t H, int32_t W);
int dagr_stream_render(const void *state, int32_t B, int64_t capacity, int64_t event_window_us, double alpha,
                       const float *det, const int32_t *n_keep, int32_t A, const int64_t *track_id, const void *rings,
                       int32_t max_tracks, int32_t trail, int32_t linewidth, int32_t ids, int32_t id_scale,
                       const uint8_t *colors, int32_t n_colors, const uint8_t *base, int64_t base_stride, uint8_t *out,
                       int32_t H, int32_t W, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* The neighbour search alone, again, on the pixel index the last dagr_graph_build_window left in `workspace` (same N):
 * rewrites nbr_src / nbr_code / deg and the edge count.  For measurement (bench.py times the search kernels on their own
 * stream with HIP events); a product caller has no use for it. */
int dagr_graph_search_window(const dagr_graph_desc *desc, void *workspace, int64_t N,
                             int32_t *nbr_src, int16_t *nbr_code, int32_t *deg, void *stream);

/* Device-side status words written by the last build on this workspace.
 * Synchronises `stream`.  flags bit0: event outside [0,W)x[0,H)x[0,B); bit1: internal list overflow.
 * num_edges = sum(deg). */
int dagr_graph_status(const dagr_graph_desc *desc, void *workspace, int64_t *num_edges /*host*/,
                      int32_t *flags /*host*/, void *stream);
/* All eight status words of the last build (synchronises `stream`): [0] pixels with more than min(64, Q) events, [1] flags,
 * [2..3] num_edges (uint64), [4] pixels beyond the FIFO depth, [5] destinations the row kernel deferred to the
 * position-centric walk (neighbourhoods of more than 320 candidates), [6] 1 when timestamps were not non-decreasing inside
 * a sample (every destination then takes the generic search), [7] destinations the row kernel answered from the inner rings
 * of their neighbourhood.  Tests use it to show which paths a window took. */
int dagr_graph_counters(const dagr_graph_desc *desc, void *workspace, int32_t *out8_host, void *stream);

/* Reference-shaped output: edge_index int64[2,E] in the order of
 * `edges[:, edges[1] >= 0]` (graph/utils.py:22), i.e. event ids, destinations ascending.
 * `row_stride` = allocated columns (>= E).  rowptr int32[N+1] receives the exclusive scan of the
 * per-event in-degree.
 * Asynchronous; E = rowptr[N]. scratch: int32[dagr_scan_scratch_elems(N+1)]. */
size_t dagr_scan_scratch_elems(int64_t n);
/* The int32 exclusive prefix sum behind the row pointers, per-pixel offsets and voxel relabelling, on its own:
 * out[i] = in[0] + ... + in[i-1] over n entries (16-byte aligned buffers).  in may be out unless zero_input, which
 * clears in[] once it is consumed.  chained == 0: one workgroup up to 65 536 entries, three launches beyond; scratch =
 * int32[dagr_scan_scratch_elems(n)], no initial state.  chained != 0: one launch (decoupled look-back; tiles of 2048
 * entries up to 320 of them, then tiles of 1024 x 8 / 16 / 32 / 48); scratch = dagr_scan_chained_state_bytes(n) bytes,
 * ALL ZERO before the first call and then left to the calls (any n the state is large enough for, one stream).
 * scratch_bytes: what the caller allocated.  Asynchronous. */
size_t dagr_scan_chained_state_bytes(int64_t n);
int dagr_exclusive_scan_i32(int32_t *in, int32_t *out, int64_t n, void *scratch, size_t scratch_bytes, int32_t chained,
                            int32_t zero_input, void *stream);
int dagr_graph_edge_index(const dagr_graph_desc *desc, void *workspace, const int32_t *nbr_src, const int32_t *deg,
                          int64_t N, int32_t *rowptr, int32_t *scan_scratch,
                          int64_t *edge_index, int64_t row_stride, void *stream);
/* The same edges as dagr_graph_edge_index, in the form the convolutions consume, without a host round trip for E:
 * rowptr int32[N+1] by destination EVENT, col int32[e_cap] source event ids, code int32[e_cap] = (dx + code_bias) |
 * (dy + code_bias) << 16 with (dx, dy) = source pixel - destination pixel (what T.Cartesian's attribute of the edge
 * encodes, transforms/cartesian in ev_tgn.py:39-58 + net.py:118-121); row e holds deg(e) entries, self loop first.
 * e_cap >= N * max_neighbors always suffices.  Asynchronous. */
int dagr_graph_csr_codes(const dagr_graph_desc *desc, void *workspace, const int32_t *nbr_src, const int16_t *nbr_code,
                         const int32_t *deg, int64_t N, int32_t code_bias, int32_t *rowptr, int32_t *scan_scratch,
                         int32_t *col, int32_t *code, int64_t e_cap, void *stream);
/* slot_event[n] = event id of node n, event_slot[e] = node of event e (either may be NULL) */
int dagr_graph_node_order(const dagr_graph_desc *desc, void *workspace, int64_t N, int32_t *slot_event,
                          int32_t *event_slot, void *stream);
/* node-ordered level-0 inputs: pos_nodes[N,3], batch_nodes[N] (int32), and per node the feature row
 * x0[n, col_feat] = feat[e], x0[n, col_pos..col_pos+1] = pos_xy[e]  (Net.forward's cat(x, pos[:, :2]), net.py:124-125;
 * the other columns are left for the sampled image features -- the column order of x0 is the caller's choice as long
 * as the packed weights follow it) */
int dagr_graph_gather_inputs(const dagr_graph_desc *desc, void *workspace, const float *pos, const float *feat,
                             int64_t N, float *pos_nodes, int32_t *batch_nodes, float *x0, int32_t ldx0,
                             int32_t col_feat, int32_t col_pos, void *stream);

/* dagr_graph_build_window (n_dev NULL) / dagr_graph_build_window_dev (n_dev given) on normalised fp32 positions that ALSO
 * writes the node-ordered level-0 inputs of dagr_graph_gather_inputs, from its last launch: one launch less per window. */
typedef struct dagr_l0_inputs {
    const float *feat;          /* fp32[N] per event (polarity)                       */
    float *pos_nodes;           /* fp32[N,3]                                          */
    int32_t *batch_nodes;       /* int32[N]                                           */
    float *x0;                  /* level-0 feature rows, row stride ldx0              */
    int32_t ldx0, col_feat, col_pos;
} dagr_l0_inputs;
int dagr_graph_build_window_inputs(const dagr_graph_desc *desc, void *workspace, const float *pos, const void *batch,
                                   int32_t batch_is_int64, int64_t N, const int32_t *n_dev, int32_t *nbr_src,
                                   int16_t *nbr_code, int32_t *deg, const dagr_l0_inputs *inputs, void *stream);

/* ------------------------------------------------------------------------ *
 * SplineConv (degree-1 open B-spline, 5x5 kernel, sum aggregation)
 *   replaces MySplineConv.forward/_forward/message_lut          model/layers/spline_conv.py:39-78
 *   over  torch_geometric SplineConv + ToSparseTensor, torch_spline_conv spline_basis /
 *   spline_weighting, torch_scatter segment_csr  (third-party, un-vendored: SURVEY.md 2.3),
 *   fused with BatchNorm(eval)+ReLU (model/layers/conv.py:23-28) and the skip branch (:47-56).
 *
 *   Edge offsets are integer LUT coordinates (ix, iy) in [0,2rx] x [0,2ry], exactly the index the
 *   reference's message_lut derives (spline_conv.py:41-42); den_x = fp32(2*Mx*width),
 *   den_y = fp32(2*My*height) as in init_lut (spline_conv.py:29-30).
 *   Weight packing (host side, BN folded: W*scale[o], shift[o]):
 *     level 0  : wpack[(tx*ty*cin taps | cin root | cskip skip)][16], taps = tx x ty window starting
 *                at (win_x, win_y) of the 5x5 kernel, tap row = (a + tx*b)*cin + i
 *     generic  : Wm[(25*cin taps | cin root | cskip skip)][cout], tap row = (kx + 5*ky)*cin + i
 * ------------------------------------------------------------------------ */
/* first kernel tap (0..4) and number of taps touched by offsets -r..r on one axis (host) */
int dagr_spline_tap_window(int32_t r, float den, int32_t *first_tap_host, int32_t *num_taps_host);
/* tab[(2rx+1)*(2ry+1)][ntp], ntp = round_up(tx*ty, 4): per offset code = ix*(2ry+1)+iy the window
 * products bx[a]*by[b] at [a + tx*b]; window = taps [win_x, win_x+tx) x [win_y, win_y+ty);
 * bad_flag (device int32) is set if an offset needs a tap outside the window */
int dagr_spline_l0_table(int32_t rx, int32_t ry, float den_x, float den_y, int32_t win_x, int32_t tx,
                         int32_t win_y, int32_t ty, float *tab, int32_t *bad_flag, void *stream);
/* fused level-0 conv on the builder's neighbour lists; cout is 16 (Net: int(base_width*32)).
 * out[n,0:16] = act(sum_j x[src_j] . What(code_j) + x[n] . root + xskip[n] . skip + shift) */
int dagr_spline_conv_l0(int32_t cin, int32_t cskip, int32_t ntaps /* tx*ty: 9, 15 or 25 */,
                        int64_t N, int32_t K, int32_t ncodes,
                        const int32_t *nbr_src, const int16_t *nbr_code, const int32_t *deg,
                        const float *x, int32_t ldx, const float *xskip, int32_t ldskip,
                        const float *tab, const float *wpack, const float *shift, int32_t relu,
                        float *out, int32_t ldo, void *stream);
/* level-0 conv as 16-node wave tiles (csrc/conv_l0_tiles.hip): same function as dagr_spline_conv_l0, but the basis is
 * evaluated from the offset domain (rx, ry, den_x, den_y; tap window [win_x, win_x+tx) x [win_y, win_y+ty)) instead of
 * a code table, and the input row is [cmain (0 or 16) channels | cextra (<= 4) channels], 16-byte aligned when cmain = 16.
 * wpack rows: [(a + tx*b)*cin + i | cin root | cskip skip] x 16 with i in the column order of x, cin = cmain + cextra.
 * K (neighbour-list stride) must be 16; (tx, ty) in {(3,3), (3,5), (5,3)}. */
int dagr_spline_conv_l0_tiles(int32_t cmain, int32_t cextra, int32_t cskip, int32_t win_x, int32_t tx, int32_t win_y,
                              int32_t ty, int32_t rx, int32_t ry, float den_x, float den_y, int64_t N, int32_t K,
                              const int32_t *nbr_src, const int16_t *nbr_code, const int32_t *deg, const float *x,
                              int32_t ldx, const float *xskip, int32_t ldskip, const float *wpack, const float *shift,
                              int32_t relu, float *out, int32_t ldo, const int32_t *n_ptr, void *stream);
/* n_ptr (device, may be NULL): the level's node count; the rows processed are min(N, *n_ptr - first_node) -- a launch
 * sized for a capacity N then serves windows of any size (captured HIP graphs).
 * the same on the nodes [first_node, first_node + N) only (all arrays are the full level's: an asynchronous update
 * computes the rows it appended; a node's result does not depend on which nodes share its tile) */
int dagr_spline_conv_l0_tiles_rows(int32_t cmain, int32_t cextra, int32_t cskip, int32_t win_x, int32_t tx, int32_t win_y,
                                   int32_t ty, int32_t rx, int32_t ry, float den_x, float den_y, int64_t first_node,
                                   int64_t N, int32_t K, const int32_t *nbr_src, const int16_t *nbr_code,
                                   const int32_t *deg, const float *x, int32_t ldx, const float *xskip, int32_t ldskip,
                                   const float *wpack, const float *shift, int32_t relu, float *out, int32_t ldo,
                                   const int32_t *n_ptr, void *stream);
/* The same two entry points for the other level-0 widths: cout = int(base_width * 32) in {8, 16, 32}; anything else returns
 * DAGR_ERR_UNSUPPORTED.  cout = 16 IS dagr_spline_conv_l0_tiles[_rows].  wpack rows are cout wide, out[n, 0:cout] is
 * written (ldo >= cout).  The input row is [cmain | cextra (<= 4)] with cmain in {0, cout} -- 8-byte pieces per lane when
 * cmain = 8, two 16-channel passes when cmain = 32 -- and cskip = (0 or cout) + (<= 4).  Instantiated: (cmain, cextra,
 * cskip) in {(0,3,0), (cout,0,3), (cout,3,0), (cout,0,cout+3)}: the events-only and --use_image conv pairs of Net.
 * The kernel's LDS (packed weights + per-offset tap rows, all dynamic) is checked here against 64 KB (cout 8, 16) or the
 * CU's 160 KB (cout 32): DAGR_ERR_INVALID_ARG instead of a launch past it. */
int dagr_spline_conv_l0_tiles_w(int32_t cout, int32_t cmain, int32_t cextra, int32_t cskip, int32_t win_x, int32_t tx,
                                int32_t win_y, int32_t ty, int32_t rx, int32_t ry, float den_x, float den_y, int64_t N,
                                int32_t K, const int32_t *nbr_src, const int16_t *nbr_code, const int32_t *deg,
                                const float *x, int32_t ldx, const float *xskip, int32_t ldskip, const float *wpack,
                                const float *shift, int32_t relu, float *out, int32_t ldo, const int32_t *n_ptr,
                                void *stream);
int dagr_spline_conv_l0_tiles_rows_w(int32_t cout, int32_t cmain, int32_t cextra, int32_t cskip, int32_t win_x, int32_t tx,
                                     int32_t win_y, int32_t ty, int32_t rx, int32_t ry, float den_x, float den_y,
                                     int64_t first_node, int64_t N, int32_t K, const int32_t *nbr_src,
                                     const int16_t *nbr_code, const int32_t *deg, const float *x, int32_t ldx,
                                     const float *xskip, int32_t ldskip, const float *wpack, const float *shift,
                                     int32_t relu, float *out, int32_t ldo, const int32_t *n_ptr, void *stream);
/* generic step 1: A[n] = [sum_j basis*x_j per tap (25*cin) | x[n] (cin) | xskip[n] (cskip)] over a
 * CSR-by-destination graph; code[e] = ix | iy<<16.  n_nodes_ptr (device, may be NULL) bounds the
 * rows actually processed (<= n_nodes_max) without a host sync. */
int dagr_spline_tap_aggregate(const int32_t *n_nodes_ptr, int32_t n_nodes_max, const int32_t *rowptr,
                              const int32_t *col, const int32_t *code, const float *x, int32_t ldx,
                              int32_t cin, const float *xskip, int32_t ldskip, int32_t cskip,
                              int32_t rx, int32_t ry, float den_x, float den_y,
                              float *A, int32_t lda, void *stream);
/* backward of step 1 w.r.t. x (training path): grad_x[src] = sum over its out-edges of basis * grad_A[dst][tap], plus
 * grad_A[n][25 cin ..] (root copy).  Deterministic: the scatter adds 64-bit fixed-point integers (unit *grad_A_absmax *
 * (E + 1) / 2^62 with E = rowptr[n_nodes] -- no sum can wrap, whatever a node's out-degree; *grad_A_absmax is a device
 * scalar >= max |grad_A|; acc int64[n_nodes_max * cin], zeroed by the caller), so the result does not depend on the
 * order in which the atomics land; grad_x is overwritten.  The weight gradient of the
 * contraction is a plain GEMM (A^T . grad_out) on the A matrix of dagr_spline_tap_aggregate. */
int dagr_spline_tap_scatter_grad(const int32_t *n_nodes_ptr, int32_t n_nodes_max, const int32_t *rowptr,
                                 const int32_t *col, const int32_t *code, const float *grad_A, int32_t lda, int32_t cin,
                                 int32_t rx, int32_t ry, float den_x, float den_y, const float *grad_A_absmax,
                                 int64_t *acc, float *grad_x, int32_t ldg, void *stream);
/* The same gradient for narrow convs (cin, cout <= 16: the event level, 400 k rows per training step) straight from
 * grad_out[n, cout] and the weight matrix Wm[26 cin, cout] (rows: 25 taps x cin, then the root rows): grad_A's row of a
 * node is rebuilt in LDS instead of being written by a GEMM (0.67 GB for the 16 -> 16 conv), reduced for its maximum and
 * read back.  *grad_A_bound: a device scalar >= max |grad_out . Wm^T|, e.g. max|grad_out| * max_k sum_co |Wm[k, co]|. */
int dagr_spline_tap_scatter_grad_w(const int32_t *n_nodes_ptr, int32_t n_nodes_max, const int32_t *rowptr,
                                   const int32_t *col, const int32_t *code, const float *grad_out, int32_t ldg, int32_t cout,
                                   const float *Wm, int32_t ldw, int32_t cin, int32_t rx, int32_t ry, float den_x,
                                   float den_y, const float *grad_A_bound, int64_t *acc, float *grad_x, int32_t ldgx,
                                   void *stream);
/* fused steps 1+2: 16 aggregated rows live in LDS, no A matrix in HBM, one launch.  K = 26*cin + cskip beyond the tile
 * (~2270 floats) is cut at tap boundaries into passes over the same edges, the accumulators staying in registers;
 * dagr_spline_conv_fused_lds_bytes(cin, cskip) = the tile of the scheme chosen, > 160 KiB when a single tap
 * (cin floats, + cin + cskip in the last pass) does not fit.
 * Wq = the [K, N] matrix of dagr_gemm_bias_act re-packed on the host into MFMA operand order:
 *   Wq[c][g][l][j] = W[16 g + 4 j + (l >> 4)][16 c + (l & 15)],  c < ceil(N/16), g < ceil(K/16), l < 64, j < 4,
 * zero outside [K, N]; 16-byte aligned. */
size_t dagr_spline_conv_fused_lds_bytes(int32_t cin, int32_t cskip);
/* passes of the scheme (1 = the whole row in the tile; 0 = unsupported).  Every pass walks the edges again: measured on
 * MI355X the multi-pass form beats tap_aggregate + gemm up to ~1.5 k node slots (one launch instead of two, no A
 * matrix) and loses beyond (tools/microbench/head_ab.hip). */
int32_t dagr_spline_conv_fused_passes(int32_t cin, int32_t cskip);
int dagr_spline_conv_fused(const int32_t *n_nodes_ptr, int32_t n_nodes_max, const int32_t *rowptr,
                           const int32_t *col, const int32_t *code, const float *x, int32_t ldx, int32_t cin,
                           const float *xskip, int32_t ldskip, int32_t cskip, int32_t rx, int32_t ry,
                           float den_x, float den_y, const float *Wq, const float *bias, float *C, int32_t ldc,
                           int32_t N, int32_t relu, void *stream);
/* Two fused convs over the SAME graph in one launch (gridDim.z = 2): same row shape (cin channels, no skip input, row
 * stride ldx), each with its own input pointer, packed weights, bias, output pointer (row stride ldc) and width.  The
 * detection head's predictors: cls_pred on the cls_conv half of the fused row and reg_pred | obj_pred on the reg_conv half
 * (model/networks/dagr.py:183-189) -- on <= 1 260-row levels a launch is what a conv costs. */
int dagr_spline_conv_fused_pair(const int32_t *n_nodes_ptr, int32_t n_nodes_max, const int32_t *rowptr,
                                const int32_t *col, const int32_t *code, int32_t ldx, int32_t cin, int32_t rx, int32_t ry,
                                float den_x, float den_y, int32_t ldc, int32_t relu, const float *x_a, const float *Wq_a,
                                const float *bias_a, float *C_a, int32_t N_a, const float *x_b, const float *Wq_b,
                                const float *bias_b, float *C_b, int32_t N_b, void *stream);
/* 1 .. 4 INDEPENDENT fused convs in one launch (gridDim.z = job): each job is a full dagr_spline_conv_fused argument set
 * (its own graph, row shape, weights, output).  What a window offers at one point of its dependency graph -- head scale 1's
 * stem beside the first conv of layer5, its cls_conv | reg_conv beside the second, its predictors beside head scale 2's
 * stem (model/networks/net.py:166-186, dagr.py:213-236) -- costs one launch instead of a stream fork + join.  All jobs must
 * take the same form (dagr_spline_conv_fused_passes == 1 for all, or > 1 for all); DAGR_ERR_UNSUPPORTED otherwise. */
typedef struct dagr_conv_job {
    const int32_t *n_nodes_ptr;
    int32_t n_nodes_max;
    const int32_t *rowptr, *col, *code;
    const float *x;
    int32_t ldx, cin;
    const float *xskip;
    int32_t ldskip, cskip, rx, ry;
    float den_x, den_y;
    const float *Wq, *bias;
    float *C;
    int32_t ldc, N, relu;
} dagr_conv_job;
int dagr_spline_conv_fused_multi(const dagr_conv_job *jobs, int32_t count, void *stream);
/* generic step 2: C[M,N] = act(A[M,K] . Wm[K,N] + bias[N]); M = min(*m_ptr, m_max) */
int dagr_gemm_bias_act(const int32_t *m_ptr, int32_t m_max, const float *A, int32_t lda,
                       const float *Wm, int32_t ldw, const float *bias, float *C, int32_t ldc,
                       int32_t K, int32_t N, int32_t relu, void *stream);

/* ------------------------------------------------------------------------ *
 * Voxel-grid pooling
 *   replaces Pooling.forward / consecutive_cluster / round_to_pixel   model/layers/pooling.py:12-97
 *   over torch_cluster.grid_cluster, torch_scatter.scatter_max, PyG pool_pos / _avg_pool_x,
 *   T.Cartesian (third-party, un-vendored), plus the LUT index of the consuming SplineConvs
 *   (spline_conv.py:41-42).  Output graph: CSR by destination cluster, sources ascending,
 *   code[e] = ix | iy<<16.  All counts stay on the device (n_out, e_out; rowptr_out[n_out] = e_out).
 * ------------------------------------------------------------------------ */
typedef struct {
    int32_t batch_size;   /* B                                                          */
    int32_t channels;     /* C: feature channels pooled                                 */
    int32_t gx, gy;       /* voxels per axis = trunc(0.9999999/size)+1 (grid_cluster)   */
    float vx, vy;         /* voxel_size[0], voxel_size[1]  (pooling.py:24)              */
    float inv_w, inv_h;   /* wh_inv = 1/W, 1/H in fp32      (pooling.py:32)             */
    float two_max;        /* fp32(2*max_value) of this pooling's Cartesian transform    */
    float r00, r02, r11, r12; /* attr_remapping_matrix of the consuming convs (spline_conv.py:23-24) */
    int32_t rx, ry;       /* their LUT offset domain                                    */
    int32_t aggr;         /* 0 = max, 1 = mean.  max: any non-NaN fp32, -0.0 ranks below +0.0.  mean: every term is
                           * rounded to a multiple of 2^-32 and summed in 64-bit fixed point (exact, order-free), so a
                           * cluster's features must satisfy |v| * members < 2^31 (|v| < 2^20 with up to 2048 members)
                           * and values below 2^-33 count as 0; the result is within 2^-33 + one fp32 rounding of the
                           * exact mean                                                    */
    int32_t append_pos;   /* also write pos[:, :2] into columns C, C+1 of each output row (net.py:137-138) */
    int32_t keep_order;   /* --keep_temporal_ordering (pooling.py:69-72).  0: every coarse edge.  1: a coarse edge
                           * src -> dst is emitted only if t_max[dst] > t_max[src] (strict: equal t_max drops it both
                           * ways), t_max = largest pos[:, 2] over the cluster's INPUT nodes (level 0: the events' t,
                           * t == 1.0 nodes included; pooled levels: the mean t the previous pooling emitted).  One
                           * extra launch per pooling step (none on the generic level-0 path), none with 0.  A larger
                           * workspace only when set.  C callers must zero this field.                            */
} dagr_pool_desc;

size_t dagr_pool_workspace_bytes(const dagr_pool_desc *desc);
int dagr_pool_workspace_init(const dagr_pool_desc *desc, void *workspace, size_t workspace_bytes, void *stream);
/* level 0: pools the events of the window whose graph was just built on (gdesc, graph_ws).
 * xlo[gx+1] / ylo[gy+1]: first pixel column/row of each voxel (device int32; from the same fp32
 * division as grid_cluster).  x_out rows start at column xoff; outputs sized for
 * T = gx*gy*(B+1) clusters; rowptr_out has T+2 entries; e_cap = capacity of col_out/code_out.
 * nbr_code (the offset codes dagr_graph_build_window wrote next to nbr_src) enables the coarse-edge fast
 * path: with radius <= 2 voxels the source voxels of a voxel's in-edges are a 5x5 bitmap collected while it
 * is pooled; windows containing t == 1.0 events (whose cluster ids leave the pixel grid) and NULL fall back
 * to the generic per-edge set insertion.  Same result either way. */
int dagr_pool_l0(const dagr_pool_desc *desc, void *pool_ws, const dagr_graph_desc *gdesc, void *graph_ws,
                 const int32_t *xlo, const int32_t *ylo, const float *x, int32_t ldx,
                 const float *pos_nodes, const int32_t *batch_nodes /* node order */,
                 const void *batch, int32_t batch_is_int64 /* event order */, int64_t N,
                 const int32_t *nbr_src, const int16_t *nbr_code /* may be NULL */, const int32_t *deg,
                 int32_t *cluster_scratch /*[N]*/, float *x_out, int32_t ldo, int32_t xoff, float *pos_out,
                 int32_t *batch_out, int32_t *n_out, int32_t *rowptr_out, int32_t *col_out, int32_t *code_out,
                 int32_t *e_out, int32_t e_cap, void *stream);
/* ------------------------------------------------------------------------ *
 * Asynchronous operation (reset=False): a micro-batch of events joins the resident window
 *   replaces, for the events-to-level-1 part, the reference's incremental update
 *     EV_TGN.forward(reset=False) -> AsyncGraph.forward            model/layers/ev_tgn.py:45-56, graph/ev_graph.py:63-103
 *     insert_in_queue_cuda_kernel / fill_edges_cuda_kernel (min_index > 0)   graph/ev_graph.cu:15-80,169-212
 *     asynchronous conv on the new nodes (graph_new_nodes branch)  asynchronous/conv.py:107-125,196-207
 *     asynchronous pooling, new-node branch (cluster caches)       asynchronous/max_pool.py:126-158
 *   Edges point from older to newer events: the rows of the window's events never change, an update appends rows.
 *   State owned by the caller (device): app_head int32[B*H*W] (-1 = empty), app_next int32[capacity],
 *   app_xytb int32[capacity][4]; event ids continue the window's (first_id = n_static + number appended so far); an
 *   appended event's node row is its id.  status int32[>=1]: bit 0 = event outside the sensor (self loop only).
 * ------------------------------------------------------------------------ */
int dagr_async_graph_append(const dagr_graph_desc *desc, void *graph_ws, int64_t n_static, int64_t first_id,
                            int32_t *app_head, int32_t *app_next, int32_t *app_xytb, int64_t capacity,
                            const void *pos /* fp32 normalised or int32 [n,3] */, int32_t pos_is_int32,
                            const void *batch, int32_t batch_is_int64, int64_t n_new,
                            int32_t *nbr_src, int16_t *nbr_code, int32_t *deg /* the level's full arrays */,
                            int32_t *status,
                            /* optional (x0 != NULL, fp32 pos): the node-ordered level-0 inputs of the new rows, as
                             * dagr_graph_gather_inputs writes them for a window, and the sample index by event id */
                            const float *feat, float *pos_nodes, int32_t *batch_nodes, int32_t *batch_events, float *x0,
                            int32_t ldx0, int32_t col_feat, int32_t col_pos, void *stream);
/* One asynchronous update as ONE call: dagr_async_graph_append (with the node-ordered inputs), conv_block1 on the n new rows
 * (dagr_spline_conv_l0_tiles_rows twice) and dagr_pool_l0_stream, issued back to back from native code.  Same kernels, same
 * arguments as the four calls; what it removes is the host time between their launches (an update of a few events is
 * ~8 launches of a few microseconds each: issued one by one from the caller's language the GPU waits for the host).
 * Events-only rows (polarity | pos_xy: cin1 = 3). */
typedef struct dagr_async_update_args {
    const dagr_graph_desc *gdesc; void *graph_ws; int64_t n_static, first_id;
    int32_t *app_head, *app_next, *app_xytb; int64_t capacity;
    const float *pos; const void *batch; int32_t batch_is_int64; int64_t n_new;
    int32_t *nbr_src; int16_t *nbr_code; int32_t *deg; int32_t *status;
    const float *feat; float *pos_nodes; int32_t *batch_nodes, *batch_events; float *x0; int32_t ldx0, col_feat, col_pos;
    int32_t win_x, tx, win_y, ty, rx, ry; float den_x, den_y;
    int32_t cin1; const float *w1, *s1; float *h1; int32_t ldh1;
    const float *w2, *s2; float *hp0; int32_t ldhp0;
    const dagr_pool_desc *pdesc; void *pool_ws; const int32_t *xlo, *ylo;
    float *x_out; int32_t ldo; float *pos_out; int32_t *batch_out, *n_out, *rowptr_out, *col_out, *code_out, *e_out;
    int32_t e_cap;
} dagr_async_update_args;
int dagr_async_update(const dagr_async_update_args *args, void *stream);
/* the same at a level-0 width cout0 in {8, 16, 32} (h1 rows are cout0 wide, hp0's first cout0 columns are written);
 * dagr_async_update is cout0 = 16 */
int dagr_async_update_w(const dagr_async_update_args *args, int32_t cout0, void *stream);
/* Launch (A) of dagr_pool_l0 alone: the level-0 accumulation kernel over the window last built on `graph_ws`, into the
 * accumulators of `pool_ws` (max / fixed-point sums: repeating it leaves max accumulators unchanged and scales the sums;
 * the next dagr_pool_l0 call re-arms everything).  For measurement (bench.py times the kernel on its own with HIP
 * events); a product caller has no use for it. */
int dagr_pool_l0_accumulate(const dagr_pool_desc *desc, void *pool_ws, const dagr_graph_desc *gdesc, void *graph_ws,
                            const int32_t *xlo, const int32_t *ylo, const float *x, int32_t ldx, const float *pos,
                            int64_t N, const int32_t *nbr_src, const int16_t *nbr_code, const int32_t *deg, void *stream);
/* pool1 with RESIDENT accumulators (its own workspace, dagr_pool_workspace_bytes): rebuild != 0 recomputes them from the
 * window (nodes [0, n_window) through the builder's pixel index); rows [first_row, first_row + n_rows) -- appended
 * nodes, first_row >= n_window -- are added; then level 1 is emitted exactly as dagr_pool_l0 emits it, and the
 * accumulators stay.  batch_events: sample index by EVENT id (window events in event order, then the appended ones).
 * Needs the cell-bitmap form of the coarse edges (search radius <= two cells). */
int dagr_pool_l0_stream(const dagr_pool_desc *desc, void *pool_ws, int32_t rebuild, const dagr_graph_desc *gdesc,
                        void *graph_ws, const int32_t *xlo, const int32_t *ylo, const float *x, int32_t ldx, const float *pos,
                        const int32_t *batch_events, int64_t n_window, int64_t first_row, int64_t n_rows,
                        const int32_t *nbr_src, const int16_t *nbr_code, const int32_t *deg, float *x_out, int32_t ldo,
                        int32_t xoff, float *pos_out, int32_t *batch_out, int32_t *n_out, int32_t *rowptr_out,
                        int32_t *col_out, int32_t *code_out, int32_t *e_out, int32_t e_cap, void *stream);

/* dagr_spline_conv_fused + launch (A) of the pooling step that consumes its output (dagr_pool_csr's accumulation) in one
 * launch: the epilogue merges every output element into its cluster's accumulator (the values it holds in registers),
 * wave w does the bookkeeping and the in-edges of node w.  Single-pass form only (dagr_spline_conv_fused_passes == 1);
 * pdesc->channels must equal N.  Follow with dagr_pool_csr(..., n_max = 0, ...): scan + emit only.  pos / batch: the
 * level's node positions and samples; cluster_scratch int32[n_nodes_max]. */
int dagr_spline_conv_fused_pool(const int32_t *n_nodes_ptr, int32_t n_nodes_max, const int32_t *rowptr,
                                const int32_t *col, const int32_t *code, const float *x, int32_t ldx, int32_t cin,
                                const float *xskip, int32_t ldskip, int32_t cskip, int32_t rx, int32_t ry,
                                float den_x, float den_y, const float *Wq, const float *bias, float *C,
                                int32_t ldc, int32_t N, int32_t relu, const dagr_pool_desc *pdesc, void *pool_ws,
                                const float *pos, const int32_t *batch, int32_t *cluster_scratch, void *stream);
/* coarser levels: input graph in CSR; n_ptr (device) = number of valid input nodes (<= n_max) */
int dagr_pool_csr(const dagr_pool_desc *desc, void *pool_ws, const int32_t *n_ptr, int32_t n_max, const float *x,
                  int32_t ldx, const float *pos, const int32_t *batch, const int32_t *rowptr, const int32_t *col,
                  int32_t *cluster_scratch /*[n_max]*/, float *x_out, int32_t ldo, int32_t xoff, float *pos_out,
                  int32_t *batch_out, int32_t *n_out, int32_t *rowptr_out, int32_t *col_out, int32_t *code_out,
                  int32_t *e_out, int32_t e_cap, void *stream);
/* LUT coordinates of an existing pooled level (CSR + pos as written by dagr_pool_*) for a consumer whose table
 * covers ANOTHER domain: DAGR.cache_luts (dagr.py:52-62) gives head "1" the pool3 table even when num_scales = 1
 * makes it consume out4.  code_out[e] = ix | iy<<16 with ix = trunc(attr_x*r00 + r02 + 1e-3) (message_lut,
 * spline_conv.py:41-42), attr = (pos[src]-pos[dst])/two_max + 0.5 of THIS level's Cartesian transform.
 * status (device int32): bit3 set when a coordinate leaves [0,2rx] x [0,2ry]. */
int dagr_pool_recode(const int32_t *n_ptr, int32_t n_max, const int32_t *rowptr, const int32_t *col, const float *pos,
                     float two_max, float r00, float r02, float r11, float r12, int32_t rx, int32_t ry,
                     int32_t *code_out, int32_t e_cap, int32_t *status, void *stream);
/* flags bit0: node outside the voxel grid; bit1: > 64 distinct sources for one cluster;
 * bit2: edge capacity exceeded; bit3: LUT coordinate out of range.  Synchronises `stream`. */
int dagr_pool_status(const dagr_pool_desc *desc, void *pool_ws, int32_t *flags_host, void *stream);
/* device address of that status word (inside pool_ws): a caller that reads other results back anyway (the training path
 * reads the two output counts of dagr_pool_csr) fetches it in the same transfer instead of a synchronisation of its own */
const int32_t *dagr_pool_status_ptr(const dagr_pool_desc *desc, void *pool_ws);
/* All eight status words (synchronises `stream`): [0] the flags above, [4] accumulator epoch, [5] level-0 nodes merged
 * through the global path so far (outside the streaming kernel's LDS window, or t == 1.0 nodes; cumulative). */
int dagr_pool_counters(const dagr_pool_desc *desc, void *pool_ws, int32_t *out8_host, void *stream);

/* ------------------------------------------------------------------------ *
 * to_dense  -- model/layers/spline_conv.py:80-107 (SplineConvToDense tail)
 *   dense[B,C,Hc,Wc] (fully written, zeros where no node); cell = trunc(pos_xy / voxel_xy);
 *   winner_scratch int32[B*Hc*Wc]; status (device int32) bit0 = node outside the map.
 * ------------------------------------------------------------------------ */
int dagr_to_dense(const int32_t *n_ptr, int32_t n_max, const float *x, int32_t ldx, int32_t channels,
                  const float *pos, const int32_t *batch, float vx, float vy, int32_t batch_size,
                  int32_t Hc, int32_t Wc, int32_t *winner_scratch, float *dense, int32_t *status, void *stream);

/* ------------------------------------------------------------------------ *
 * training path (scripts/train_ncaltech101.py:41-74): backward halves the reference gets from
 * torch_scatter's / torch's autograd.  The forward entry points above are reused unchanged.
 * ------------------------------------------------------------------------ */
/* Pooling's feature aggregation, max (pooling.py:74-75, torch_scatter.scatter_max): arg[c, ch] = lowest node index
 * among cluster c's members whose x equals x_pooled[c, ch] (the CPU reducer's first maximum).  cluster int32[n] =
 * consecutive cluster id of each node (-1: outside the grid); arg int32[n_clusters, channels]. */
int dagr_pool_argmax(const int32_t *cluster, int32_t n, const float *x, int32_t ldx, int32_t channels,
                     const float *x_pooled, int32_t ldp, int32_t n_clusters, int32_t *arg, void *stream);
/* grad_x[n, ch] = grad_pooled[cluster[n], ch] where arg[cluster[n], ch] == n, else 0 (aggr 0, max), or
 * grad_pooled[cluster[n], ch] / count[cluster[n]] (aggr 1, mean: _avg_pool_x, pooling.py:77).  Fully written. */
int dagr_pool_grad(const int32_t *cluster, int32_t n, int32_t channels, int32_t aggr, const int32_t *arg,
                   const int32_t *count, const float *grad_pooled, int32_t ldg, float *grad_x, int32_t ldgx,
                   void *stream);
/* to_dense (spline_conv.py:80-107) backward: grad_x[n, :] = grad_dense[batch[n], :, cy, cx] for every node inside the
 * map (0 outside) -- INCLUDING nodes whose row a later node of the same cell overwrote in the forward: torch's
 * index_put backward gathers grad[indices] for all written rows, which is what the reference back-propagates. */
int dagr_to_dense_grad(int32_t n, int32_t channels, const float *pos, const int32_t *batch, float vx, float vy,
                       int32_t batch_size, int32_t Hc, int32_t Wc, const float *grad_dense,
                       float *grad_x, int32_t ldgx, void *stream);

/* y = relu(y + z) in place over n floats (16-byte aligned buffers of identical layout): the residual join of the
 * image branch's ResNet blocks (reference: torchvision Bottleneck/BasicBlock.forward, used by
 * src/dagr/model/networks/net_img.py:42-86) in one pass instead of add + clamp. */
int dagr_add_relu(float *y, const float *z, int64_t n, void *stream);
/* y = relu(y + bias[c]) in place over a channels-last map of n floats, C channels (C % 4 == 0): bias + ReLU after a
 * bias-free convolution in one pass (torchvision block forward: bnX folded into convX, then relu). */
int dagr_bias_relu(float *y_nhwc, const float *bias, int64_t n, int32_t C, void *stream);
/* same with SiLU (v / (1 + exp(-v))): yolox BaseConv (conv -> BN -> SiLU) of the CNN head (dagr.py:106-122). */
int dagr_bias_silu(float *y_nhwc, const float *bias, int64_t n, int32_t C, void *stream);
/* ResNet stem tail in one pass over channels-last maps: y[B, OH, OW, C] = maxpool 3x3 / stride 2 / pad 1 of
 * relu(x[B, H, W, C] * scale[c] + shift[c]), OH = (H-1)/2 + 1 (torchvision ResNet.forward bn1 -> relu -> maxpool,
 * net_img.py:80-84; eval-mode BatchNorm as an affine pair).  C % 4 == 0, 16-byte aligned buffers. */
int dagr_bn_relu_maxpool(const float *x_nhwc, int32_t B, int32_t H, int32_t W, int32_t C, const float *scale,
                         const float *shift, float *y_nhwc, void *stream);

/* ------------------------------------------------------------------------ *
 * sample_features (--use_image) -- model/networks/net.py:15-17,193-221
 *   out[n, coff:coff+C] = trilinear grid_sample (align_corners=True) of feat at node n's position;
 *   feat is channels-last fp32 [B,h,w,C]; width/height = sensor size used for normalisation.
 * ------------------------------------------------------------------------ */
int dagr_sample_features(const int32_t *n_ptr, int32_t n_max, const float *pos, const void *batch,
                         int32_t batch_is_int64, const float *feat_nhwc, int32_t B, int32_t h, int32_t w, int32_t C,
                         int32_t width, int32_t height, float *out, int32_t ldo, int32_t coff, void *stream);

/* ------------------------------------------------------------------------ *
 * Detection post-processing -- model/utils.py:25-33,61-110 (batched_nms_coordinate_trick over
 * torchvision.ops.nms, called per image from a Python loop)
 *   boxes[B,A,4] (x1,y1,x2,y2), scores[B,A], cls[B,A] (class id; boxes are shifted by cls*class_offset
 *   before the IoU test), valid[B,A] (uint8).  order_out[B,A]: anchor indices by descending score
 *   (invalid last), keep_out[B,A]: 1 where order_out[i] survives greedy NMS (IoU > thr suppressed),
 *   n_keep[B].  A <= 1024.
 * ------------------------------------------------------------------------ */
int dagr_nms_batched(const float *boxes, const float *scores, const int32_t *cls, const uint8_t *valid,
                     int32_t B, int32_t A, float iou_threshold, float class_offset,
                     int32_t *order_out, int32_t *keep_out, int32_t *n_keep, void *stream);

/* to_dense of the head scales (model/layers/spline_conv.py:80-107: cell = trunc(pos_xy / voxel_xy), highest node index
 * wins a shared cell) + the image branch's logits (model/networks/dagr.py:219-222,230-234) + collect_outputs /
 * decode_outputs (dagr.py:283-312) in ONE launch.  Per scale: the predictor rows pred[n, ld] (reg 4 | obj 1 | cls C),
 * node positions / samples, the map geometry, optionally the CNN head's reg / obj / cls maps (element strides for
 * [b, c, y, x]; NULL = events only) and optionally a dense[B, 5 + C, Hc, Wc] buffer that receives the fused logit maps.
 * out[B, A, 5 + C] as dagr_decode_heads.  scale1 may be NULL (num_scales = 1).  status bit0: node outside the map. */
typedef struct dagr_head_scale {
    const int32_t *n_ptr; int32_t n_max;
    const float *pred; int32_t ld;
    const float *pos; const int32_t *batch;
    float vx, vy, stride; int32_t Hc, Wc;
    const float *cnn[3]; int32_t cnn_stride[3][4];
    float *dense;
} dagr_head_scale;
int dagr_heads_finish(const dagr_head_scale *scale0, const dagr_head_scale *scale1, int32_t batch_size, int32_t channels,
                      float *out, int32_t *status, void *stream);
/* The same launch followed, inside it, by dagr_postprocess of every image (model/utils.py:61-110; dagr.py:94-95: the eval
 * forward post-processes its decoded outputs at once): one workgroup per image decodes the image's rows and runs its
 * confidence mask + class-offset NMS on them.  det[B, A, 6] / n_keep[B] as dagr_postprocess; `out` is still written. */
int dagr_heads_finish_detect(const dagr_head_scale *scale0, const dagr_head_scale *scale1, int32_t batch_size,
                             int32_t channels, float *out, int32_t *status, float conf_threshold, float iou_threshold,
                             float class_offset, float *det, int32_t *n_keep, void *stream);
/* collect_outputs + decode_outputs of the eval head (model/networks/dagr.py:283-312; grid/stride cache of
 * model/utils.py:119-134) for one or two scales in one launch: dense logit maps [B, channels = 5+C, Hs, Ws] (reg | obj |
 * cls) -> out[B, A, channels], A = H0*W0 (+ H1*W1), xy = (logit + cell) * stride, wh = exp(logit) * stride, the rest
 * sigmoid.  dense1 may be NULL (num_scales = 1). */
int dagr_decode_heads(const float *dense0, int32_t H0, int32_t W0, float stride0, const float *dense1, int32_t H1,
                      int32_t W1, float stride1, int32_t B, int32_t channels, float *out, void *stream);

/* The whole of postprocess_network_output (model/utils.py:61-110, filtering=True) for a window batch in ONE launch:
 * pred[B,A,5+C] = decoded head outputs (cx, cy, w, h, obj, cls...) -> cxcywh->xyxy in the reference's op order,
 * class max / argmax, score = obj*class_conf, mask (score*class_conf >= conf_threshold), class-offset greedy NMS.
 * det[B,A,6]: the survivors of image b are rows 0..n_keep[b]-1 = (x1, y1, x2, y2, score, label) in descending score
 * (ties: ascending anchor); rows beyond are unspecified.  A <= 1024. */
int dagr_postprocess(const float *pred, int32_t B, int32_t A, int32_t num_classes, float conf_threshold,
                     float iou_threshold, float class_offset, float *det, int32_t *n_keep, void *stream);

/* ------------------------------------------------------------------------ *
 * 1:1 replacements of the reference's native module `asy_tools` (src/dagr/asynchronous/asy_tools/main.cu:239-244): the
 * masked row operators of the asynchronous per-event network update.  indices int64[K] = rows (nodes) that changed;
 * feature matrices are [num_nodes, C] fp32 row-major; only the selected rows are read / written, in place.
 *   dagr_masked_lin          <- masked_lin(indices, x_in, x_out, weight[Cout,Cin], bias[Cout], add)      main.cu:220-236
 *   dagr_masked_lin_no_bias  <- masked_lin_no_bias(indices, x_in, x_out, weight, add)                    main.cu:198-216
 *   dagr_masked_isdiff       <- masked_isdiff(indices, x_old, x_new, atol, rtol): marks unchanged rows with -1 in
 *                               `indices`; the caller compacts (`indices[indices > -1]`, main.cu:138)     main.cu:112-139
 *   dagr_masked_inplace_BN   <- masked_inplace_BN(indices, x, x_out, mean, var, weight, bias, eps)       main.cu:69-96
 * Same argument order as the reference, then the shapes (K, Cin, Cout / C) and the stream.  add != 0: accumulate onto
 * x_out instead of overwriting it.
 * ------------------------------------------------------------------------ */
int dagr_masked_lin(const int64_t *indices, const float *x_in, float *x_out, const float *weight, const float *bias,
                    int32_t add, int64_t K, int32_t Cin, int32_t Cout, void *stream);
int dagr_masked_lin_no_bias(const int64_t *indices, const float *x_in, float *x_out, const float *weight, int32_t add,
                            int64_t K, int32_t Cin, int32_t Cout, void *stream);
int dagr_masked_isdiff(int64_t *indices, const float *x_old, const float *x_new, float atol, float rtol, int64_t K,
                       int32_t C, void *stream);
int dagr_masked_inplace_BN(const int64_t *indices, const float *x, float *x_out, const float *running_mean,
                           const float *running_var, const float *weight, const float *bias, float eps, int64_t K,
                           int32_t C, void *stream);

/* ------------------------------------------------------------------------ *
 * Event-stream downsampling -- scripts/downsample_events.py:91-124 (downsample_events / _filter_events_resize)
 *   Events grouped by output cell (x / fx, y / fy) in time order: order[N] = event ids sorted (stably) by cell,
 *   run_cell[n_runs] / run_end[n_runs] = the cells that occur and the cumulative end of their runs in `order`
 *   (torch.sort + unique_consecutive + cumsum, as graph/utils.py:9-13 prepares pixels).  polarity int8[N] in {-1,+1};
 *   change_map fp32[Ho*Wo] = the integrator state, carried from chunk to chunk; keep[N] (uint8) = 1 where the event
 *   passes.  The surviving events keep their order; their coordinates are x / fx, y / fy.
 * ------------------------------------------------------------------------ */
int dagr_downsample_events(const int32_t *order, const int32_t *run_cell, const int32_t *run_end, int32_t n_runs,
                           const int8_t *polarity, int32_t fx, int32_t fy, float *change_map, uint8_t *keep,
                           void *stream);

/* The 1x1 convolutions of the channels-last image branch (src/dagr/model/networks/net_img.py:42-48, BatchNorm folded) as
 * library GEMMs (hipBLASLt, fp32 in / fp32 accumulate) with the whole epilogue in the kernel:
 *   D[M, N] = act(A[M, K] . Wt[K, N] + bias[N] (+ R[M, N])),  row-major, row strides lda / ldr / ldd; act 0 = none, 1 = ReLU;
 * bias and R may be NULL; D may alias neither A nor R (DAGR_ERR_INVALID_ARG).  The residual join + ReLU of a bottleneck
 * (relu(bn3(conv3(x)) + identity)) is one launch.
 * workspace: device scratch of at least dagr_gemm_epilogue_workspace_bytes() bytes (caller-owned, no hidden allocation). */
size_t dagr_gemm_epilogue_workspace_bytes(void);
int dagr_gemm_epilogue(const float *A, int64_t M, int32_t K, int64_t lda, const float *Wt, int32_t N, const float *bias,
                       const float *R, int64_t ldr, int32_t act, float *D, int64_t ldd, void *workspace,
                       size_t workspace_bytes, void *stream);

/* The same GEMM on the bf16 matrix pipe at fp32 accuracy (gemm_split_bf16.hip): every operand is split into three bf16
 * pieces and six of the nine piece products are accumulated in fp32 (the three dropped ones are <= 2^-24 relative each).
 * fp32 in memory on both sides, no split-K and no atomics (same operands, same bits), nothing allocated, synchronised or
 * initialised at launch (capturable).
 *   dagr_gemm_split_bf16_packed_bytes(K, N): size of the packed weights; 0 for a shape the kernel does not take.
 *   dagr_gemm_split_bf16_pack: Wt[K, N] (row-major, dense) -> packed (three bf16 planes in the kernel's own LDS image, K-slice
 *     major, N padded to 128 columns; opaque -- only the kernel reads it).  Once per layer: the kernel never reads Wt.
 *   dagr_gemm_split_bf16: D[M, N] = act(A . W + bias[N] (+ R[M, N])), arguments as dagr_gemm_epilogue.  stride == 1: A
 *     is M rows of K floats at pitch lda (B, H, W unused).  stride > 1: a 1x1 convolution with that spatial stride on a
 *     channels-last map A[B, H, W, K] (pixel pitch lda), read in place; M must be B * ceil(H/stride) * ceil(W/stride).
 *   dagr_conv3x3_split_bf16: D[B*H*W, N] = act(conv3x3(X) + bias (+ R)), stride 1, pad 1, X[B, H, W, C] channels-last with
 *     pixel pitch ldx; packed from Wt[9 C, N] with row (3 ky + kx) C + c.
 *   tile (rows x columns): 0 = chosen from the shape (among the variants below), 1 = 64 x 128, 2 = 32 x 128, 3 = 64 x 64,
 *     4 = 32 x 64 (the same result bits whichever runs: K is never split, the 32-wide K-slices are added in ascending order).
 * DAGR_ERR_UNSUPPORTED: K (C for the 3x3) not a multiple of 32, N not a multiple of 16.  DAGR_ERR_INVALID_ARG: row
 * strides not multiples of 4 floats, pointers not 16-byte aligned, D aliasing A or R, a packed buffer too small. */
size_t dagr_gemm_split_bf16_packed_bytes(int32_t K, int32_t N);
int dagr_gemm_split_bf16_pack(const float *Wt, int32_t K, int32_t N, void *packed, size_t packed_bytes, void *stream);
int dagr_gemm_split_bf16(const float *A, int64_t M, int32_t K, int64_t lda, const void *packed, int32_t N,
                         const float *bias, const float *R, int64_t ldr, int32_t act, float *D, int64_t ldd, int32_t B,
                         int32_t H, int32_t W, int32_t stride, int32_t tile, void *stream);
int dagr_conv3x3_split_bf16(const float *X, int32_t B, int32_t H, int32_t W, int32_t C, int64_t ldx, const void *packed,
                            int32_t N, const float *bias, const float *R, int64_t ldr, int32_t act, float *D, int64_t ldd,
                            int32_t tile, void *stream);

/* The same two calls with every form of the kernel selectable: `variant` (tile x waves) in place of `tile`.  Variants 1 - 4
 * are the tiles above, on four waves; W8 is the 64 x 128 tile on eight waves (2 x 4, each 32 x 32 of the output), which tile 0
 * chooses for the 1x1 shapes with K <= 512 and enough rows to fill the chip.  0 = chosen from the shape, as tile 0.  Every
 * variant gives the same result bits.  A variant past DAGR_SPLIT_VARIANT_LAST is DAGR_ERR_INVALID_ARG and nothing is
 * written. */
#define DAGR_SPLIT_64X128 1
#define DAGR_SPLIT_32X128 2
#define DAGR_SPLIT_64X64 3
#define DAGR_SPLIT_32X64 4
#define DAGR_SPLIT_64X128_W8 5
#define DAGR_SPLIT_VARIANT_LAST 5
int dagr_gemm_split_bf16_variant(const float *A, int64_t M, int32_t K, int64_t lda, const void *packed, int32_t N,
                                 const float *bias, const float *R, int64_t ldr, int32_t act, float *D, int64_t ldd,
                                 int32_t B, int32_t H, int32_t W, int32_t stride, int32_t variant, void *stream);
int dagr_conv3x3_split_bf16_variant(const float *X, int32_t B, int32_t H, int32_t W, int32_t C, int64_t ldx,
                                    const void *packed, int32_t N, const float *bias, const float *R, int64_t ldr,
                                    int32_t act, float *D, int64_t ldd, int32_t variant, void *stream);

/* ------------------------------------------------------------------------ *
 * FLOP accounting in the reference's scheme (src/dagr/asynchronous/flops/conv.py and the per-module logs of
 * asynchronous/conv.py, max_pool.py, linear.py, cartesian.py, batch_norm.py): the counts of the init pass (log index 0,
 * evaluate_flops(..., dense=True)) of one window, one int64 per logged module.
 *   deg[n_events]      level-0 in-degrees of the window's events (level-0 edges = their sum)
 *   counts1..counts4   [n_nodes, n_edges] of pooled levels 1..4 (device)
 *   mods[n_mods]       the modules (device): kind, graph level (0..4; a pooling's INPUT level), cin / cout, whether
 *                      the conv has a root weight / a bias
 *   out[n_mods]        int64 counts (device)
 * ------------------------------------------------------------------------ */
enum { DAGR_FLOPS_ZERO = 0, DAGR_FLOPS_CONV = 1, DAGR_FLOPS_LINEAR = 2, DAGR_FLOPS_POOL = 3, DAGR_FLOPS_CARTESIAN = 4 };
typedef struct dagr_flops_module {
    int32_t kind, level, cin, cout, root, bias;
} dagr_flops_module;
int dagr_async_flops(const int32_t *deg, int32_t n_events, const int32_t *counts1, const int32_t *counts2,
                     const int32_t *counts3, const int32_t *counts4, const dagr_flops_module *mods, int32_t n_mods,
                     int64_t *out, void *stream);

/* ------------------------------------------------------------------------ *
 * Visualisation frames -- visualization/event_viz.py:3-10, the outlines of visualization/bbox_viz.py:11-53,
 * scripts/visualize_detections.py:58-78.  F independent frames in one call; frame f is:
 *   images[frame_image[f]]  its base image, uint8 BGR [H, W, 3], one of n_images stacked images
 *   events [ev_ptr[f], ev_ptr[f+1])  of the concatenated ev_x / ev_y (int32) and ev_p (int8); ev_ptr[F + 1] (device),
 *                           n_events = ev_ptr[F]
 *   alpha[f]                float64 in [0, 1] (device)
 *   boxes [box_ptr[f], box_ptr[f+1])  of boxes[n_boxes, 5] int32 (x0, y0, x1, y1, class id); box_ptr NULL = no boxes
 * out[F, H, W, 3] uint8.  Events, exactly as the reference's loop: a pixel hit by at least one event of the frame becomes
 * trunc(alpha * base) on every channel, then channel p - 1 (wrapped like a Python index: p = 0 -> 2, p = 1 -> 0,
 * p = -1 -> 1) of the LAST such event, in array order, becomes trunc(that + 255 * (1 - alpha)); float64 arithmetic.
 * Events with y >= H are skipped as in the reference; so are x >= W (unchecked there) and negative coordinates.
 * Outlines, this project's own rule (OpenCV's thick-line rasteriser is not reproduced): pixel q lies on a box's outline
 * when its Chebyshev distance to the border of the rectangle [min(x0, x1), max(x0, x1)] x [min(y0, y1), max(y0, y1)] is
 * <= linewidth / 2 (integer division): linewidth 1 = the one-pixel border, 2 and 3 = a three-pixel band centred on it.
 * Clipped to the image; painted in colors[3 * class id ..] after the events; a later box of the frame wins.
 * workspace: dagr_viz_workspace_bytes(F, H, W) (per-pixel last event index).  status (device int32, zeroed here):
 * bit0 an event's p - 1 outside [-3, 2] (the event is dropped), bit1 a drawn class id outside [0, n_colors), bit2 a
 * frame_image entry outside [0, n_images) (the frame is not written), bit3 an alpha outside [0, 1] (events not drawn).
 * `out` may alias `images` only when frame_image[f] == f for every f (each thread reads its pixel before writing it).
 * ------------------------------------------------------------------------ */
size_t dagr_viz_workspace_bytes(int32_t F, int32_t H, int32_t W);
int dagr_viz_render(const uint8_t *images, int32_t n_images, int32_t H, int32_t W, const int32_t *frame_image, int32_t F,
                    const int32_t *ev_x, const int32_t *ev_y, const int8_t *ev_p, const int32_t *ev_ptr, int32_t n_events,
                    const double *alpha, const int32_t *boxes, const int32_t *box_ptr, int32_t n_boxes, int32_t linewidth,
                    const uint8_t *colors, int32_t n_colors, uint8_t *out, int32_t *status, void *workspace,
                    size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------ *
 * Training augmentations on a collated batch on the device -- src/dagr/data/augment.py: RandomHFlip :90-112,
 * RandomZoom :148-198, RandomCrop(p = 0.2) :201-243, RandomTranslate :246-279, Crop([0, 0], [1, 1]) :115-145, chained as
 * Augmentations.__init__ :287-294 chains them.  The random draws are made on the host; the kernels read one record per
 * sample from DEVICE memory:
 *   flip            != 0: x = W - 1 - x
 *   crop_on         != 0: only events with crop_lo <= (x, y) <= crop_hi (both ends inclusive) stay; not shifted
 *   zoom            fp32 factor about (W / 2, H / 2): (float(x) - cx) * zoom + cx, two roundings, truncated to int16.
 *                   zoom < 1 shrinks without the reference's integrate-and-fire subsampling (subsample = False).
 *   move            whole-pixel shift added after the zoom; then only 0 <= x < W, 0 <= y < H stays.
 *
 * dagr_augment_events: pos[N, 2] (int16: pos_width 2, int32: pos_width 4), t[N] (t_width bytes per entry, 4 or 8) and
 * p[N] (p_width bytes, 1 / 2 / 4 / 8); t and p are copied as they are and carry no range check; sample b owns [sample_ptr[b], sample_ptr[b + 1]),
 * sample_ptr[B + 1] int32 on the device.  Survivors are written densely in their input order: out_pos[., 2] int16, out_t,
 * out_p (the input widths), out_batch (int64 sample index, may be NULL), out_ptr[B + 1] their segment bounds.  All
 * outputs hold N entries; out_ptr[B] tells how many are used.  Two launches up to 4 M events (beyond: a scan of the
 * per-tile counts between them), no host synchronisation.  workspace: dagr_augment_workspace_bytes(N) bytes, no initial
 * state.  status (device int32, zeroed here): bit0 sample_ptr does not run from 0 to N without decreasing (nothing is
 * written but zeros to out_ptr), bit1 an int32 coordinate outside int16 (that event is dropped).
 * dagr_augment_status reads it (synchronises the stream) and returns DAGR_ERR_INVALID_ARG with a message if a bit is set.
 *
 * dagr_augment_frames: out[B, C, H, W] from in[B, C, H, W] (elem_bytes 1: uint8, 4: fp32; in != out), one thread per output
 * pixel walking the chain backwards: undo the shift (black outside), undo the zoom (torch's `nearest` source index of a
 * resize to (ceil(H zoom), ceil(W zoom)), centre-cropped or centre-padded to the sensor), blank by the crop window, undo
 * the flip.  reference_crop != 0 blanks as augment.py:51-58 does (the window indexes the batch and channel dimensions
 * of the sample's [1, C, H, W] frame: crop_lo[1] > 0 blanks the frame, crop_lo[0] = c blanks channels < c, crop_hi[0]
 * bounds them above); 0 blanks rows outside [crop_lo[1], crop_hi[1]) and columns outside [crop_lo[0], crop_hi[0]).
 *
 * dagr_augment_boxes: rows of `ld` >= 4 fp32 columns (x, y, w, h first; the others are copied), box_batch[M] int64 their
 * samples: mirrored, clamped to the window, scaled, shifted and clamped to the sensor as the boxes of the chain are.
 * ------------------------------------------------------------------------ */
typedef struct dagr_aug_params {
    int32_t flip, crop_on;
    int32_t crop_lo[2], crop_hi[2];
    float zoom;
    int32_t move[2];
} dagr_aug_params;
size_t dagr_augment_workspace_bytes(int64_t N);
int dagr_augment_events(const dagr_aug_params *params, int32_t B, int32_t W, int32_t H, const void *pos, int32_t pos_width,
                        const void *t, int32_t t_width, const void *p, int32_t p_width, const int32_t *sample_ptr, int64_t N,
                        int16_t *out_pos, void *out_t, void *out_p, int64_t *out_batch, int32_t *out_ptr,
                        int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
int dagr_augment_status(const int32_t *status, void *stream);
int dagr_augment_frames(const dagr_aug_params *params, int32_t B, int32_t C, int32_t H, int32_t W, int32_t elem_bytes,
                        int32_t reference_crop, const void *in, void *out, void *stream);
int dagr_augment_boxes(const dagr_aug_params *params, int32_t B, int32_t W, int32_t H, const float *boxes,
                       const int64_t *box_batch, int32_t M, int32_t ld, float *out, void *stream);

/* ---------------------------------------------------------------------------
 * COCO-protocol matching (csrc/coco_match.hip): utils/coco_eval.py:_evaluate_image for a flat list of jobs in one launch.
 * A job is one (image, class, area range) with at least one ground-truth box or one detection of that class; one
 * workgroup matches it, one wave per IoU threshold.  All arrays are DEVICE memory.
 *
 *   gt_xywh[n_gt, 4], dt_xywh[n_dt, 4]   float64 (x, y, w, h): the float32 corner boxes with w = x2 - x1, h = y2 - y1
 *                                        subtracted in float32 and then widened, as _xywh does
 *   dt_score[n_dt]                       float64
 *   jobs[n_jobs, 6]                      int64: {first ground-truth row, G, first detection row, D,
 *                                        first column of the job in order / dtm / dt_ign, first entry of the job in g_ign}
 *   area_rng[n_jobs, 2]                  float64 [lo, hi]: boxes with area < lo or > hi are ignored
 *   iou_thrs[n_thr]                      float64, 1 <= n_thr <= 16: the host's IOU_THRS, never recomputed here
 *
 * Outputs, with D' = min(D, max_dets) columns per job and n_out = sum of D', n_gign = sum of G over the jobs:
 *   order[n_out]            int32: the job's detections (index inside the job) by descending score, equal scores in
 *                           input order, NaN last (numpy's argsort(-scores, kind="mergesort")), cut to max_dets
 *   dtm[n_thr, n_out]       uint8: the detection of that column is matched at that threshold
 *   dt_ign[n_thr, n_out]    uint8: ... matched to ignored ground truth, or unmatched and outside the area range
 *   g_ign[n_gign]           uint8: the job's ground truth, evaluated boxes first (stable), 1 = ignored
 *   status                  int32, zeroed here; 1 afterwards if a job's offsets or counts did not fit the arrays or the
 *                           bounds below (that job wrote nothing)
 *
 * Per-job bounds (dagr_coco_match_bounds reports them): G <= DAGR_COCO_MAX_GT = 256 -- the sorted ground truth of a job
 * sits in an LDS tile of 32 bytes a box, under 12 KiB per workgroup with the detections, so the LDS of a CU holds a dozen
 * jobs, and each lane keeps the matched flags of its G / 64 boxes in one register; the training targets of this
 * project hold at most 100 boxes an image.  D <= DAGR_COCO_MAX_DT = 4096 before the cut (the rank of a score is counted
 * against all others).  max_dets <= DAGR_COCO_MAX_DETS = 100.  The caller states the largest G and D of its jobs
 * (max_gt_per_job, max_dt_per_job); beyond the bounds the call fails with DAGR_ERR_INVALID_ARG before any device work,
 * and such a job is to be matched on the host.  No host synchronisation.
 * ------------------------------------------------------------------------ */
#define DAGR_COCO_MAX_GT 256
#define DAGR_COCO_MAX_DT 4096
#define DAGR_COCO_MAX_DETS 100
void dagr_coco_match_bounds(int32_t *max_gt, int32_t *max_dt, int32_t *max_dets);
int dagr_coco_match(const double *gt_xywh, const double *dt_xywh, const double *dt_score, const int64_t *jobs,
                    const double *area_rng, const double *iou_thrs, int32_t n_thr, int32_t max_dets, int64_t n_jobs,
                    int64_t n_gt, int64_t n_dt, int32_t max_gt_per_job, int32_t max_dt_per_job, int64_t n_out,
                    int64_t n_gign, int32_t *order, uint8_t *dtm, uint8_t *dt_ign, uint8_t *g_ign, int32_t *status,
                    void *stream);

/* ---------------------------------------------------------------------------
 * COCO-protocol accumulation (csrc/coco_accumulate.hip): utils/coco_eval.py:_accumulate after its sort, for every
 * (class, area range) group and every IoU threshold in one call -- cumulative counts of the counted true and false
 * positives along the score order, precision, its envelope, and the envelope at the first position whose recall reaches
 * each recall point.  All arrays are DEVICE memory.
 *
 *   dtm[n_thr, n_cols], dt_ign[n_thr, n_cols]   uint8, as dagr_coco_match wrote them (non-zero = true)
 *   perm[n_cols]                                int32: the column visited k-th.  The positions of a group are contiguous, and
 *                                               inside a group they run by descending score, equal scores in the order of
 *                                               _accumulate's concatenation (image, then the matcher's order)
 *   group_ptr[n_groups + 1]                     int64: group g owns the positions group_ptr[g] .. group_ptr[g + 1] of perm
 *   group_ngt[n_groups]                         int64: the group's ground truth that is not ignored
 *   rec_thrs[n_rec]                             float64, 1 <= n_rec <= DAGR_COCO_ACC_MAX_REC = 128: the host's REC_THRS
 *   eps                                         the host's numpy.spacing(1), > 0
 *
 * Outputs:
 *   precision[n_thr, n_rec, n_groups]   float64: -1 for a group with group_ngt <= 0; otherwise, per threshold and recall
 *                           point r, max over i >= idx of tp[i] / ((fp[i] + tp[i]) + eps), idx the first position with
 *                           tp[idx] / group_ngt >= rec_thrs[r] (both float64 divisions), and 0 when no position qualifies
 *                           (a group without positions included).  The same bits as the host's.
 *   status                  int32, zeroed here; 1 afterwards if an entry of perm lies outside [0, n_cols) or group_ptr is
 *                           not non-decreasing inside [0, n_cols]: `precision` is then left untouched
 *
 * One workgroup per (group, threshold) walks its segment in tiles of DAGR_COCO_ACC_TILE positions (dagr_coco_accumulate_tile
 * reports it) with the counts carried as integers, so a segment may be of any length up to n_cols <= 2^31 - 1.  The
 * workspace (dagr_coco_accumulate_workspace_bytes; 0 and an error message for sizes out of range) holds one byte per
 * (threshold, position): the flags gathered through perm.  A workspace that is too small, n_thr > 16 or n_rec beyond its
 * bound fail with DAGR_ERR_INVALID_ARG before any device work.  No host synchronisation.
 * ------------------------------------------------------------------------ */
#define DAGR_COCO_ACC_TILE 1024
#define DAGR_COCO_ACC_MAX_REC 128
int32_t dagr_coco_accumulate_tile(void);
size_t dagr_coco_accumulate_workspace_bytes(int32_t n_thr, int64_t n_cols);
int dagr_coco_accumulate(const uint8_t *dtm, const uint8_t *dt_ign, const int32_t *perm, const int64_t *group_ptr,
                         const int64_t *group_ngt, const double *rec_thrs, int32_t n_rec, double eps, int32_t n_thr,
                         int32_t n_groups, int64_t n_cols, void *workspace, size_t workspace_bytes, double *precision,
                         int32_t *status, void *stream);

/* Host-side helper: first n offsets of the search spiral (spiral.h:1-15), the closed form the
 * search kernel uses.  dx/dy are HOST arrays.  Lets CPU-only tests pin the visiting order. */
int dagr_spiral_offsets(int32_t n, int32_t *dx_host, int32_t *dy_host);

#ifdef __cplusplus
}
#endif
#endif /* DAGR_HIP_H */
