// stream_track.hip -- the event stream's tracker (dagr_stream_track, dagr_stream_track_cv and their _rescue entries): the
// detections of a step are associated with the tracks the lane carries from step to step, by greedy IoU matching inside a
// label, and get a track id.
//
// ONE kernel, k_stream_track<MOTION, RESCUE>, instantiated four times: retirement, eligibility, the match with its tie rule
// and the spawn are written once.  Below, <false> and <true> stand for MOTION with RESCUE = false.  <false> is dagr_stream_track.  <true> is dagr_stream_track_cv, the same walk with a constant-velocity
// motion model (TrackDefinition(motion=)): a slot also holds `vel`; every live slot is predicted once, in front of the row
// loop, to pred = box + vel * fp32(t_ref - t_last), the rows are compared against pred, a match filters box and vel, and
// the live tracks that no row matched leave their prediction in the lane's coast list -- one ballot compaction per slot
// register.  Whatever exists only with the motion model stands under `if constexpr (MOTION)`; nothing of it is left in
// the code of <false>.  The two states have layouts of their own (include/dagr_hip.h).
//
// RESCUE (dagr_stream_track_rescue, dagr_stream_track_cv_rescue; TrackDefinition(rescue=)) adds a second association round
// on the same states: the rows with low_score <= score < min_score are staged in LDS rows of their own (behind the high
// rows', in the same arrays) while the high rows are, walk the tracks that round one left unmatched through the SAME match
// body at an IoU threshold of their own, and never spawn.  The body is shared by making the row loop run over both rounds,
// not by a lambda or a function: with the body in a lambda the instantiations that existed before lost their instruction
// stream (other registers, another schedule), as a loop they keep it instruction for instruction, with their registers and
// their LDS (profiles/stream_rescue.md).  A low row that does not match has no effect, so round two stops when a ballot
// shows no live untaken track.  Whatever only round two has stands under `if constexpr (RESCUE)` or folds away with it.
//
// One workgroup of ONE wave per lane.  A thread holds the slots `lane`, `lane + 64`, ... of its lane's max_tracks slots in
// registers (kMaxTracks / 64 = 4 at most).  The walk over the rows is serial, as greedy matching is; the work of a row is
// parallel over the slots, and the (largest IoU, lowest id) choice is a ballot in the usual case of one candidate and a
// shuffle reduction otherwise: the row loop has no barrier.  Spawning pairs the k-th unmatched row with the k-th free slot,
// both counted by ballot + popcount.  Every float decision repeats the numpy definition (dagr_amd/streaming.py:
// TrackDefinition) operation by operation; this library is built with -ffp-contract=off, and the fp32 division is correctly
// rounded.
#include "stream_track.hpp"

namespace dagr {
namespace {

constexpr int kMaxTracks = DAGR_TRACK_MAX_TRACKS;
constexpr int kMaxDets = DAGR_TRACK_MAX_DETS;
constexpr int kSlots = kMaxTracks / kWave;          // slots of one thread
constexpr int64_t kNever = INT64_MIN;
static_assert(kMaxTracks % kWave == 0 && kMaxDets % kWave == 0 && kMaxDets / kWave <= 32, "one flag word per thread");

bool track_sizes_ok(int32_t B, int32_t M) { return B >= 1 && B <= 65535 && M >= 1 && M <= kMaxTracks; }

__global__ __launch_bounds__(kBlock) void k_track_first_ids(int64_t *__restrict__ next_id, int B) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b < B) next_id[b] = 1;
}

// The order of the arguments is measured, not taste: what only the motion model has comes last (st.vel, alpha, beta, o), so
// that everything <false> reads lies in the first 128 bytes of the argument segment, which is all its kernel had when it
// was a kernel of its own.  With the state first and `vel` in its middle, <false> read a third 64-byte line of arguments
// and a launch took 0.3 us longer (profiles/stream_track_unified.md).  What only RESCUE has (low_score, low_iou, rescued) comes
// behind that again, for the same reason.
template <bool MOTION, bool RESCUE>
__global__ __launch_bounds__(kWave) void k_stream_track(int M, float iou_thr, int64_t max_age, float min_score,
                                                        const float *__restrict__ det, const int32_t *__restrict__ n_keep,
                                                        int A, const int64_t *__restrict__ t_ref,
                                                        int64_t *__restrict__ track_id, int32_t *__restrict__ track_hits,
                                                        int64_t *__restrict__ untracked, Tracks st, float alpha, float beta,
                                                        MotionOut o, float low_score, float low_iou,
                                                        int64_t *__restrict__ rescued) {
    constexpr int kRows = RESCUE ? 2 * kMaxDets : kMaxDets;     // RESCUE: the participating low rows at kMaxDets and behind
    __shared__ float4 s_box[kRows];             // the participating rows, in row order
    __shared__ int32_t s_label[kRows];
    __shared__ int32_t s_row[kRows];            // their row in det
    __shared__ int32_t s_spawn[kMaxDets];       // k-th unmatched participating row

    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = min(max(n_keep[b], 0), A);
    const int64_t now = t_ref[b];
    const float *rows = det + (int64_t)b * A * 6;
    int64_t *out_id = track_id + (int64_t)b * A;
    int32_t *out_hits = track_hits + (int64_t)b * A;
    float4 *out_box = nullptr, *out_vel = nullptr;
    if constexpr (MOTION) {
        out_box = o.track_box + (int64_t)b * A;
        out_vel = o.track_vel + (int64_t)b * A;
    }
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (now == kNever) {                        // no reference instant yet: nothing is tracked, nothing coasts or changes
        for (int i = lane; i < n; i += kWave) {
            out_id[i] = 0;
            out_hits[i] = 0;
            if constexpr (MOTION) {
                const float *p = rows + (int64_t)i * 6;
                out_box[i] = make_float4(p[0], p[1], p[2], p[3]);
                out_vel[i] = zero4;
            }
        }
        if constexpr (MOTION) {
            if (o.n_coast && lane == 0) o.n_coast[b] = 0;
        }
        return;
    }

    // ---- the lane's slots; retire what has not been seen for more than max_age.  MOTION: predict what lives, once
    int64_t id[kSlots], seen[kSlots];
    float4 box[kSlots];
    int32_t label[kSlots], hits[kSlots];
    float4 vel[kSlots], pred[kSlots];           // MOTION only, as is dt
    float dt[kSlots];
    const int64_t base = (int64_t)b * M;
#pragma unroll
    for (int k = 0; k < kSlots; k++) {
        const int slot = k * kWave + lane;
        id[k] = 0, seen[k] = 0, label[k] = 0, hits[k] = 0;
        box[k] = zero4;
        if constexpr (MOTION) dt[k] = 0.0f, vel[k] = zero4, pred[k] = zero4;
        if (slot < M) {
            id[k] = st.id[base + slot];
            seen[k] = st.t_last[base + slot];
            box[k] = st.box[base + slot];
            if constexpr (MOTION) vel[k] = st.vel[base + slot];
            label[k] = st.label[base + slot];
            hits[k] = st.hits[base + slot];
            if (id[k] != 0 && now - seen[k] > max_age) id[k] = 0;
            if constexpr (MOTION) {
                if (id[k] == 0) vel[k] = zero4;                        // a free slot is at rest
                if (id[k] != 0) {
                    dt[k] = (float)(now - seen[k]);                    // (exact inside the age bound; else to nearest even)
                    pred[k] = make_float4(box[k].x + vel[k].x * dt[k], box[k].y + vel[k].y * dt[k],
                                          box[k].z + vel[k].z * dt[k], box[k].w + vel[k].w * dt[k]);
                }
            }
        }
    }

    // ---- the eligible rows, 64 at a time: the first kMaxDets of them take part and go to the LDS in row order
    int n_eligible = 0;
    int n_low = 0;                              // RESCUE only
    for (int first = 0; first < n; first += kWave) {
        const int i = first + lane;
        float4 r = zero4;
        float score = 0.0f, cls = 0.0f;
        if (i < n) {
            const float *p = rows + (int64_t)i * 6;
            r = make_float4(p[0], p[1], p[2], p[3]);
            score = p[4];
            cls = p[5];
        }
        const bool eligible = i < n && score >= min_score;         // (a NaN score compares false)
        const uint64_t mask = __ballot(eligible);
        const int rank = n_eligible + lanes_below(mask, lane);
        n_eligible += __popcll(mask);
        int low_rank = kMaxDets;                                   // RESCUE: the row's place among the low rows, if it is one
        if constexpr (RESCUE) {
            const bool low = i < n && score >= low_score && !(score >= min_score);   // (a NaN score is in neither band)
            const uint64_t low_mask = __ballot(low);
            if (low) low_rank = n_low + lanes_below(low_mask, lane);
            n_low += __popcll(low_mask);
        }
        if (eligible && rank < kMaxDets) {
            s_box[rank] = r;
            s_label[rank] = (int32_t)cls;
            s_row[rank] = i;
        } else if (RESCUE && low_rank < kMaxDets) {                // waits for round two, which writes its outputs
            s_box[kMaxDets + low_rank] = r;
            s_label[kMaxDets + low_rank] = (int32_t)cls;
            s_row[kMaxDets + low_rank] = i;
        } else if (i < n) {                                        // no id.  MOTION: the row's own box, no velocity
            out_id[i] = 0;
            out_hits[i] = 0;
            if constexpr (MOTION) out_box[i] = r, out_vel[i] = zero4;
        }
    }
    const int P = min(n_eligible, kMaxDets);
    __syncthreads();

    // ---- match: the rows in order, every thread against its own slots; thread r % 64 remembers the unmatched row r.
    // MOTION compares a row with pred[k], where the track is predicted to be, and without it with box[k].  That is the
    // box from before the step in both: a matched slot is `taken` and never compared again, and spawns come after the loop.
    //
    // RESCUE: ONE loop is both rounds, so the body below is written once.  Behind the P high rows it walks the PL low rows,
    // which lie at kMaxDets and behind, at their own threshold; thread r % 64 remembers the MATCHED low row r.  A low row
    // that does not match changes nothing, so the walk ends when a ballot finds no live untaken track.
    uint32_t taken = 0, unmatched = 0;
    uint32_t low_matched = 0;                   // RESCUE only, as are PL and n_rescued
    const int PL = RESCUE ? min(n_low, kMaxDets) : 0;
    int n_rescued = 0;
    for (int r = 0; r < P + PL; r++) {
        bool second = false;
        int at = r;
        float thr = iou_thr;
        if constexpr (RESCUE) {
            if (r >= P) {
                bool open = false;
#pragma unroll
                for (int k = 0; k < kSlots; k++) open |= id[k] != 0 && !((taken >> k) & 1u);
                if (__ballot(open) == 0) break;
                second = true, at = kMaxDets + (r - P), thr = low_iou;
            }
        }
        const float4 d = s_box[at];
        const int32_t cls = s_label[at];
        float best = 0.0f;
        int64_t best_id = 0;
        int best_k = -1;
#pragma unroll
        for (int k = 0; k < kSlots; k++) {
            if (id[k] == 0 || label[k] != cls || ((taken >> k) & 1u)) continue;
            float v;
            if constexpr (MOTION) v = iou_xyxy(d, pred[k]);
            else v = iou_xyxy(d, box[k]);
            if (!(v >= thr)) continue;                                 // (a NaN IoU never matches)
            if (best_k < 0 || v > best || (v == best && id[k] < best_id)) {
                best = v;
                best_id = id[k];
                best_k = k;
            }
        }
        uint64_t cand = __ballot(best_k >= 0);
        if (cand == 0) {
            if (!second && lane == (r & 63)) unmatched |= 1u << (r >> 6);
            continue;
        }
        if constexpr (RESCUE) {
            if (second) {
                if (lane == ((r - P) & 63)) low_matched |= 1u << ((r - P) >> 6);
                n_rescued++;
            }
        }
        if (cand & (cand - 1)) {                                      // several threads have one: largest IoU, lowest id
            float top = best_k >= 0 ? best : -1.0f;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) top = fmaxf(top, __shfl_xor(top, off, kWave));
            cand = __ballot(best_k >= 0 && best == top);
            if (cand & (cand - 1)) {
                int64_t low = (best_k >= 0 && best == top) ? best_id : INT64_MAX;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const int64_t o2 = __shfl_xor(low, off, kWave);
                    low = o2 < low ? o2 : low;
                }
                cand = __ballot(best_k >= 0 && best == top && best_id == low);
            }
        }
        if (lane == __ffsll((unsigned long long)cand) - 1) {
            const int row = s_row[at];
#pragma unroll
            for (int k = 0; k < kSlots; k++) {
                if (k != best_k) continue;
                if constexpr (MOTION) {                                // filter: the row pulls box and vel off the prediction
                    const float4 p = pred[k];
                    const float4 res = make_float4(d.x - p.x, d.y - p.y, d.z - p.z, d.w - p.w);
                    if (dt[k] > 0.0f) {                                // the residual as a velocity; the first one is taken whole
                        const float4 q = make_float4(res.x / dt[k], res.y / dt[k], res.z / dt[k], res.w / dt[k]);
                        vel[k] = hits[k] == 1 ? q
                                              : make_float4(vel[k].x + beta * q.x, vel[k].y + beta * q.y,
                                                            vel[k].z + beta * q.z, vel[k].w + beta * q.w);
                    }
                    box[k] = alpha == 1.0f ? d
                                           : make_float4(p.x + alpha * res.x, p.y + alpha * res.y, p.z + alpha * res.z,
                                                         p.w + alpha * res.w);
                } else {
                    box[k] = d;
                }
                seen[k] = now;
                hits[k] += 1;
                taken |= 1u << k;
                out_id[row] = id[k];
                out_hits[row] = hits[k];
                if constexpr (MOTION) out_box[row] = box[k], out_vel[row] = vel[k];
            }
        }
    }

    if constexpr (RESCUE) {                     // the low rows no track took: no id.  MOTION: the row's own box, no velocity
#pragma unroll
        for (int q = 0; q < kMaxDets / kWave; q++) {
            const int r = q * kWave + lane;
            if (r >= PL || ((low_matched >> q) & 1u)) continue;
            const int row = s_row[kMaxDets + r];
            out_id[row] = 0;
            out_hits[row] = 0;
            if constexpr (MOTION) out_box[row] = s_box[kMaxDets + r], out_vel[row] = zero4;
        }
    }

    // ---- spawn: the k-th unmatched row takes the k-th free slot and the id next_id + k (MOTION: at rest)
    int n_unmatched = 0;
#pragma unroll
    for (int q = 0; q < kMaxDets / kWave; q++) {
        const bool mine = (unmatched >> q) & 1u;
        const uint64_t mask = __ballot(mine);
        if (mine) s_spawn[n_unmatched + lanes_below(mask, lane)] = q * kWave + lane;
        n_unmatched += __popcll(mask);
    }
    __syncthreads();
    const int64_t first_id = st.next_id[b];
    int n_free = 0;
    int free_rank[kSlots];
#pragma unroll
    for (int k = 0; k < kSlots; k++) {
        const bool is_free = k * kWave + lane < M && id[k] == 0;
        const uint64_t mask = __ballot(is_free);
        free_rank[k] = is_free ? n_free + lanes_below(mask, lane) : -1;
        n_free += __popcll(mask);
    }
    const int n_spawn = min(n_unmatched, n_free);
    uint32_t spawned = 0;                       // MOTION only: the coast list leaves them out
#pragma unroll
    for (int k = 0; k < kSlots; k++) {
        if (free_rank[k] < 0 || free_rank[k] >= n_spawn) continue;
        const int r = s_spawn[free_rank[k]];
        id[k] = first_id + free_rank[k];
        seen[k] = now;
        box[k] = s_box[r];
        label[k] = s_label[r];
        hits[k] = 1;
        if constexpr (MOTION) vel[k] = zero4, spawned |= 1u << k;
    }
    for (int k = lane; k < n_unmatched; k += kWave) {              // the rows' own outputs; past the free slots: untracked
        const int r = s_spawn[k], row = s_row[r];
        out_id[row] = k < n_spawn ? first_id + k : 0;
        out_hits[row] = k < n_spawn ? 1 : 0;
        if constexpr (MOTION) out_box[row] = s_box[r], out_vel[row] = zero4;
    }

    // ---- coast (MOTION): the live tracks this step neither matched nor spawned, in slot order, where they are predicted to be
    if constexpr (MOTION) {
        if (o.n_coast) {
            int n_coast = 0;
#pragma unroll
            for (int k = 0; k < kSlots; k++) {
                const bool coasts = id[k] != 0 && !(((taken | spawned) >> k) & 1u);
                const uint64_t mask = __ballot(coasts);
                if (coasts) {
                    const int64_t at = base + n_coast + lanes_below(mask, lane);
                    o.coast_id[at] = id[k];
                    o.coast_box[at] = pred[k];
                    o.coast_label[at] = label[k];
                    o.coast_age[at] = now - seen[k];
                }
                n_coast += __popcll(mask);
            }
            if (lane == 0) o.n_coast[b] = n_coast;
        }
    }

    // ---- the state goes back
#pragma unroll
    for (int k = 0; k < kSlots; k++) {
        const int slot = k * kWave + lane;
        if (slot < M) {
            st.id[base + slot] = id[k];
            st.t_last[base + slot] = seen[k];
            st.box[base + slot] = box[k];
            if constexpr (MOTION) st.vel[base + slot] = vel[k];
            st.label[base + slot] = label[k];
            st.hits[base + slot] = hits[k];
        }
    }
    if (lane == 0) {
        st.next_id[b] = first_id + n_spawn;
        const int lost = (n_eligible - P) + (n_unmatched - n_spawn);
        if (untracked && lost > 0) untracked[b] += lost;
        if constexpr (RESCUE) {
            if (rescued && n_rescued > 0) rescued[b] += n_rescued;
        }
    }
}

// A refusal of the helpers below, which both families of entry points share: DAGR_CHECK_ARG, headed by the name of the
// entry point that was called (`entry`) and by the family's prefix (`who`).
#define TRACK_CHECK_ARG(cond, msg)                                             \
    do {                                                                       \
        if (!(cond)) {                                                         \
            set_error(std::string(entry) + ": " + who + ": " + (msg));         \
            return DAGR_ERR_INVALID_ARG;                                       \
        }                                                                      \
    } while (0)

const char *track_prefix(bool motion) { return motion ? "stream track cv" : "stream track"; }
const char *track_bytes_name(bool motion) { return motion ? "dagr_stream_track_cv_bytes" : "dagr_stream_track_bytes"; }

size_t track_bytes(bool motion, int32_t B, int32_t M) {
    return track_sizes_ok(B, M) ? carve_tracks(motion, B, M, nullptr, nullptr) : 0;
}

int track_reset(const char *entry, bool motion, void *tracks, size_t bytes, int32_t B, int32_t M, void *stream) {
    const std::string who = track_prefix(motion);
    TRACK_CHECK_ARG(tracks != nullptr, "tracks is NULL");
    TRACK_CHECK_ARG(track_sizes_ok(B, M), "B or max_tracks out of range (1 .. DAGR_TRACK_MAX_TRACKS)");
    TRACK_CHECK_ARG(((uintptr_t)tracks & 15) == 0, "tracks must be 16-byte aligned");
    Tracks st;
    const size_t need = carve_tracks(motion, B, M, (char *)tracks, &st);
    TRACK_CHECK_ARG(bytes >= need, std::string("state smaller than ") + track_bytes_name(motion));
    DAGR_CHECK_HIP(hipMemsetAsync(tracks, 0, need, (hipStream_t)stream));
    k_track_first_ids<<<(unsigned)ceil_div(B, kBlock), kBlock, 0, (hipStream_t)stream>>>(st.next_id, B);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

// What both step entries refuse, in the order they refuse it; `st` is the carved state when nothing is refused.
int track_check_args(const char *entry, bool motion, void *tracks, size_t bytes, int32_t B, int32_t M, float iou,
                     int64_t max_age_us, const float *det, const int32_t *n_keep, int32_t A, const int64_t *t_ref,
                     const int64_t *track_id, const int32_t *track_hits, const int64_t *untracked, Tracks *st) {
    const std::string who = track_prefix(motion);
    TRACK_CHECK_ARG(track_sizes_ok(B, M), "B or max_tracks out of range (1 .. DAGR_TRACK_MAX_TRACKS)");
    TRACK_CHECK_ARG(iou > 0.0f && iou <= 1.0f, "iou must be in (0, 1]");
    TRACK_CHECK_ARG(max_age_us >= 0, "max_age_us must not be negative");
    TRACK_CHECK_ARG(A >= 0 && A <= (1 << 24), "A out of range");
    TRACK_CHECK_ARG(tracks && n_keep && t_ref, "NULL pointer");
    TRACK_CHECK_ARG(A == 0 || (det && track_id && track_hits), "NULL detections or outputs");
    TRACK_CHECK_ARG(((uintptr_t)tracks & 15) == 0 && (((uintptr_t)t_ref | (uintptr_t)track_id | (uintptr_t)untracked) & 7) == 0 &&
                        (((uintptr_t)det | (uintptr_t)n_keep | (uintptr_t)track_hits) & 3) == 0,
                    "tracks must be 16-byte aligned, int64 arrays 8-byte, fp32 / int32 arrays 4-byte");
    TRACK_CHECK_ARG(bytes >= carve_tracks(motion, B, M, (char *)tracks, st),
                    std::string("state smaller than ") + track_bytes_name(motion));
    return DAGR_OK;
}

// A refusal by name of the entry point that was called, from a helper that several entries share.
#define ENTRY_CHECK_ARG(cond, msg)                                             \
    do {                                                                       \
        if (!(cond)) {                                                         \
            set_error(std::string(entry) + ": " + (msg));                      \
            return DAGR_ERR_INVALID_ARG;                                       \
        }                                                                      \
    } while (0)

// What the _rescue entries refuse in addition, behind everything their base entry refuses.
int rescue_check_args(const char *entry, bool motion, float min_score, float low_score, float low_iou, const int64_t *rescued) {
    const std::string who = std::string(track_prefix(motion)) + " rescue";
    TRACK_CHECK_ARG(low_score == low_score, "low_score is NaN");
    TRACK_CHECK_ARG(low_score < min_score, "low_score must be below min_score (no score lies in between; raise min_score)");
    TRACK_CHECK_ARG(low_iou > 0.0f && low_iou <= 1.0f, "low_iou must be in (0, 1]");
    TRACK_CHECK_ARG(((uintptr_t)rescued & 7) == 0, "rescued must be 8-byte aligned");
    return DAGR_OK;
}

// dagr_stream_track (rescue = false: the three last arguments are not looked at) and dagr_stream_track_rescue
int step_plain(const char *entry, bool rescue, void *tracks, size_t bytes, int32_t B, int32_t max_tracks, float iou,
               int64_t max_age_us, float min_score, const float *det, const int32_t *n_keep, int32_t A, const int64_t *t_ref,
               int64_t *track_id, int32_t *track_hits, int64_t *untracked, float low_score, float low_iou, int64_t *rescued,
               void *stream) {
    Tracks st;
    if (const int rc = track_check_args(entry, false, tracks, bytes, B, max_tracks, iou, max_age_us, det, n_keep, A, t_ref,
                                        track_id, track_hits, untracked, &st))
        return rc;
    if (rescue) {
        if (const int rc = rescue_check_args(entry, false, min_score, low_score, low_iou, rescued)) return rc;
        k_stream_track<false, true><<<(unsigned)B, kWave, 0, (hipStream_t)stream>>>(
            max_tracks, iou, max_age_us, min_score, det, n_keep, A, t_ref, track_id, track_hits, untracked, st, 0.0f, 0.0f,
            MotionOut{}, low_score, low_iou, rescued);
    } else {
        k_stream_track<false, false><<<(unsigned)B, kWave, 0, (hipStream_t)stream>>>(
            max_tracks, iou, max_age_us, min_score, det, n_keep, A, t_ref, track_id, track_hits, untracked, st, 0.0f, 0.0f,
            MotionOut{}, 0.0f, 0.0f, nullptr);
    }
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

// dagr_stream_track_cv and dagr_stream_track_cv_rescue, likewise
int step_cv(const char *entry, bool rescue, void *tracks, size_t bytes, int32_t B, int32_t max_tracks, float iou,
            int64_t max_age_us, float min_score, float alpha, float beta, const float *det, const int32_t *n_keep, int32_t A,
            const int64_t *t_ref, int64_t *track_id, int32_t *track_hits, float *track_box, float *track_vel,
            int64_t *coast_id, float *coast_box, int32_t *coast_label, int64_t *coast_age_us, int32_t *n_coast,
            int64_t *untracked, float low_score, float low_iou, int64_t *rescued, void *stream) {
    // what the motion model adds; the rest is dagr_stream_track's
    ENTRY_CHECK_ARG(max_age_us <= DAGR_TRACK_CV_MAX_AGE_US,
                    "stream track cv: max_age_us must not exceed DAGR_TRACK_CV_MAX_AGE_US = 2^24 - 1 (a live track's age is exact in fp32)");
    ENTRY_CHECK_ARG(alpha > 0.0f && alpha <= 1.0f, "stream track cv: alpha must be in (0, 1]");
    ENTRY_CHECK_ARG(beta >= 0.0f && beta <= 1.0f, "stream track cv: beta must be in [0, 1]");
    ENTRY_CHECK_ARG(A == 0 || (det && track_id && track_hits && track_box && track_vel),
                    "stream track cv: NULL detections or outputs (track_id, track_hits, track_box, track_vel)");
    const bool coast = coast_id || coast_box || coast_label || coast_age_us || n_coast;
    ENTRY_CHECK_ARG(!coast || (coast_id && coast_box && coast_label && coast_age_us && n_coast),
                    "stream track cv: coast_id, coast_box, coast_label, coast_age_us and n_coast are NULL together or not at all");
    ENTRY_CHECK_ARG((((uintptr_t)track_box | (uintptr_t)track_vel | (uintptr_t)coast_box) & 15) == 0,
                    "stream track cv: track_box, track_vel and coast_box must be 16-byte aligned (one store a box)");
    ENTRY_CHECK_ARG((((uintptr_t)coast_id | (uintptr_t)coast_age_us) & 7) == 0 &&
                        (((uintptr_t)coast_label | (uintptr_t)n_coast) & 3) == 0,
                    "stream track cv: coast_id and coast_age_us must be 8-byte aligned, coast_label and n_coast 4-byte");
    Tracks st;
    if (const int rc = track_check_args(entry, true, tracks, bytes, B, max_tracks, iou, max_age_us, det, n_keep, A, t_ref,
                                        track_id, track_hits, untracked, &st))
        return rc;
    const MotionOut o = {(float4 *)track_box, (float4 *)track_vel, coast_id, (float4 *)coast_box, coast_label, coast_age_us, n_coast};
    if (rescue) {
        if (const int rc = rescue_check_args(entry, true, min_score, low_score, low_iou, rescued)) return rc;
        k_stream_track<true, true><<<(unsigned)B, kWave, 0, (hipStream_t)stream>>>(
            max_tracks, iou, max_age_us, min_score, det, n_keep, A, t_ref, track_id, track_hits, untracked, st, alpha, beta, o,
            low_score, low_iou, rescued);
    } else {
        k_stream_track<true, false><<<(unsigned)B, kWave, 0, (hipStream_t)stream>>>(
            max_tracks, iou, max_age_us, min_score, det, n_keep, A, t_ref, track_id, track_hits, untracked, st, alpha, beta, o,
            0.0f, 0.0f, nullptr);
    }
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" size_t dagr_stream_track_bytes(int32_t B, int32_t max_tracks) { return track_bytes(false, B, max_tracks); }
extern "C" size_t dagr_stream_track_cv_bytes(int32_t B, int32_t max_tracks) { return track_bytes(true, B, max_tracks); }

extern "C" int dagr_stream_track_reset(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, void *stream) {
    return track_reset(__func__, false, tracks, bytes, B, max_tracks, stream);
}

extern "C" int dagr_stream_track_cv_reset(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, void *stream) {
    return track_reset(__func__, true, tracks, bytes, B, max_tracks, stream);
}

extern "C" int dagr_stream_track(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, float iou, int64_t max_age_us,
                                 float min_score, const float *det, const int32_t *n_keep, int32_t A, const int64_t *t_ref,
                                 int64_t *track_id, int32_t *track_hits, int64_t *untracked, void *stream) {
    return step_plain(__func__, false, tracks, bytes, B, max_tracks, iou, max_age_us, min_score, det, n_keep, A, t_ref, track_id,
                      track_hits, untracked, 0.0f, 0.0f, nullptr, stream);
}

extern "C" int dagr_stream_track_rescue(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, float iou, int64_t max_age_us,
                                        float min_score, const float *det, const int32_t *n_keep, int32_t A,
                                        const int64_t *t_ref, int64_t *track_id, int32_t *track_hits, int64_t *untracked,
                                        float low_score, float low_iou, int64_t *rescued, void *stream) {
    return step_plain(__func__, true, tracks, bytes, B, max_tracks, iou, max_age_us, min_score, det, n_keep, A, t_ref, track_id,
                      track_hits, untracked, low_score, low_iou, rescued, stream);
}

extern "C" int dagr_stream_track_cv(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, float iou, int64_t max_age_us,
                                    float min_score, float alpha, float beta, const float *det, const int32_t *n_keep,
                                    int32_t A, const int64_t *t_ref, int64_t *track_id, int32_t *track_hits, float *track_box,
                                    float *track_vel, int64_t *coast_id, float *coast_box, int32_t *coast_label,
                                    int64_t *coast_age_us, int32_t *n_coast, int64_t *untracked, void *stream) {
    return step_cv(__func__, false, tracks, bytes, B, max_tracks, iou, max_age_us, min_score, alpha, beta, det, n_keep, A, t_ref,
                   track_id, track_hits, track_box, track_vel, coast_id, coast_box, coast_label, coast_age_us, n_coast, untracked,
                   0.0f, 0.0f, nullptr, stream);
}

extern "C" int dagr_stream_track_cv_rescue(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, float iou,
                                           int64_t max_age_us, float min_score, float alpha, float beta, const float *det,
                                           const int32_t *n_keep, int32_t A, const int64_t *t_ref, int64_t *track_id,
                                           int32_t *track_hits, float *track_box, float *track_vel, int64_t *coast_id,
                                           float *coast_box, int32_t *coast_label, int64_t *coast_age_us, int32_t *n_coast,
                                           int64_t *untracked, float low_score, float low_iou, int64_t *rescued, void *stream) {
    return step_cv(__func__, true, tracks, bytes, B, max_tracks, iou, max_age_us, min_score, alpha, beta, det, n_keep, A, t_ref,
                   track_id, track_hits, track_box, track_vel, coast_id, coast_box, coast_label, coast_age_us, n_coast, untracked,
                   low_score, low_iou, rescued, stream);
}
