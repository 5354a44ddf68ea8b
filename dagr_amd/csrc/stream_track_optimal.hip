// stream_track_optimal.hip -- dagr_stream_track_optimal: the stream tracker (stream_track.hip) with the match of a round
// replaced by an optimal one-to-one assignment (TrackDefinition(assign="optimal"), include/dagr_hip.h).  Never, retire,
// eligibility, the 256-row cut, predict, filter, spawn, coast and `rescued` are the greedy entries', on their states; the
// kernels there are not touched: this file has its own, and shares only stream_track.hpp.
//
// One workgroup of ONE wave per lane, as there; a thread holds the slots `lane`, `lane + 64`, ... in registers.  A round
// (round one: the participating high rows; round two: the participating low rows) is
//   fill:   every thread computes, for every row of the round, the weight of its own slots and stores its columns of the
//           lane's weight matrix w[row, slot] in the workspace: (1 << 29) + (int32)(iou * 2^20) for an admissible pair, else 0;
//   solve:  assign_wave (assign.hpp) on w, with row_col in LDS; its pairing is assign_max_weight_definition's entry for
//           entry, which is what makes the track ids the definition's;
//   apply:  row_col is inverted to slot -> row in LDS and every thread applies the matches of its own slots -- in
//           parallel, where the greedy walk is serial: pairs do not interact.
// The solve is skipped when the fill found no row and no slot with two admissible partners: the admissible pairs are then
// disjoint, every optimal pairing -- the definition's too -- consists of exactly them, and the fill has already noted them.
#include "assign.hpp"
#include "stream_track.hpp"

namespace dagr {
namespace {

constexpr int kMaxTracks = DAGR_TRACK_MAX_TRACKS;
constexpr int kMaxDets = DAGR_TRACK_MAX_DETS;
constexpr int kSlots = kMaxTracks / kWave;          // slots of one thread
constexpr int64_t kNever = INT64_MIN;
constexpr int32_t kPair = 1 << 29;                  // an admissible pair, before its IoU: above kMaxDets quantised IoUs
static_assert(kMaxTracks % kWave == 0 && kMaxDets % kWave == 0 && kMaxDets / kWave <= 32, "one flag word per thread");
static_assert(kMaxTracks <= kAssignMax && kMaxDets <= kAssignMax, "a round fits assign_wave");
static_assert((int64_t)kMaxDets * (1 << 20) < kPair, "one more match outweighs every IoU");

// the lane's part of the workspace: the weight matrix and the transposed copy, kMaxDets x M words each
__host__ __device__ inline size_t lane_words(int M) { return 2 * (size_t)kMaxDets * M; }

template <bool MOTION, bool RESCUE>
__global__ __launch_bounds__(kWave) void k_stream_track_optimal(int M, float iou_thr, int64_t max_age, float min_score,
                                                                const float *__restrict__ det,
                                                                const int32_t *__restrict__ n_keep, int A,
                                                                const int64_t *__restrict__ t_ref,
                                                                int64_t *__restrict__ track_id,
                                                                int32_t *__restrict__ track_hits,
                                                                int64_t *__restrict__ untracked, Tracks st, float alpha,
                                                                float beta, MotionOut o, float low_score, float low_iou,
                                                                int64_t *__restrict__ rescued, int32_t *__restrict__ ws) {
    constexpr int kRows = RESCUE ? 2 * kMaxDets : kMaxDets;     // RESCUE: the participating low rows at kMaxDets and behind
    __shared__ float4 s_box[kRows];             // the participating rows, in row order
    __shared__ int32_t s_label[kRows];
    __shared__ int32_t s_row[kRows];            // their row in det
    __shared__ int32_t s_spawn[kMaxDets];       // k-th unmatched participating row
    __shared__ int32_t s_row_col[kMaxDets];     // the round's pairing: the slot of a row, -1: none
    __shared__ int32_t s_slot_row[kMaxTracks];  // and inverted: the row of a slot, -1: none
    __shared__ AssignLds s_assign;

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
    const int PL = RESCUE ? min(n_low, kMaxDets) : 0;

    // ---- match: one assignment per round.  MOTION compares a row with pred[k], where the track is predicted to be, and
    // without it with box[k]; either is from before the step, since round two never looks at a slot that round one took.
    int32_t *w = ws + (int64_t)b * lane_words(M);                  // [rows of the round, M]
    int32_t *wt = w + (int64_t)kMaxDets * M;                       // assign_wave's transposed copy
    uint32_t taken = 0, unmatched = 0;
    int n_rescued = 0;
    for (int round = 0; round < (RESCUE ? 2 : 1); round++) {
        const int R = round ? PL : P, at = round ? kMaxDets : 0;
        const float thr = round ? low_iou : iou_thr;
        if (R == 0) continue;                                      // (uniform)
        for (int r = lane; r < R; r += kWave) s_row_col[r] = -1;
        for (int s = lane; s < M; s += kWave) s_slot_row[s] = -1;
        __syncthreads();                                           // the staged rows; the two tables before the fill writes them

        // fill.  A thread counts the admissible rows of each of its slots, a ballot counts the admissible slots of a row
        int mine[kSlots], partners[kSlots];                        // the last admissible row of the slot, and how many
#pragma unroll
        for (int k = 0; k < kSlots; k++) mine[k] = -1, partners[k] = 0;
        bool conflict = false;
        for (int r = 0; r < R; r++) {
            const float4 d = s_box[at + r];
            const int32_t cls = s_label[at + r];
            int row_partners = 0;
#pragma unroll
            for (int k = 0; k < kSlots; k++) {
                const int slot = k * kWave + lane;
                if (k * kWave >= M) continue;                      // (uniform)
                int32_t weight = 0;
                if (id[k] != 0 && label[k] == cls && !((taken >> k) & 1u)) {
                    float v;
                    if constexpr (MOTION) v = iou_xyxy(d, pred[k]);
                    else v = iou_xyxy(d, box[k]);
                    if (v >= thr) weight = kPair + (int32_t)(v * kIouOne);      // (a NaN IoU never is)
                }
                if (slot < M) w[r * M + slot] = weight;
                if (weight > 0) mine[k] = r, partners[k]++, s_row_col[r] = slot;    // (several writers only under a conflict)
                row_partners += __popcll(__ballot(weight > 0));
            }
            conflict |= row_partners > 1;
        }
#pragma unroll
        for (int k = 0; k < kSlots; k++) conflict |= partners[k] > 1;
        conflict = __ballot(conflict) != 0;

        if (conflict) {
            __syncthreads();                                       // w: written by this workgroup, read by all of it
            assign_wave(w, M, R, M, wt, s_row_col, s_assign);
            __syncthreads();
            for (int r = lane; r < R; r += kWave) {
                const int c = s_row_col[r];
                if (c >= 0) s_slot_row[c] = r;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kSlots; k++) {
                const int slot = k * kWave + lane;
                mine[k] = slot < M ? s_slot_row[slot] : -1;
            }
        } else {
            __syncthreads();                                       // s_row_col, which the fill wrote
        }

        // apply: every thread the matches of its own slots
#pragma unroll
        for (int k = 0; k < kSlots; k++) {
            if (mine[k] < 0) continue;
            const float4 d = s_box[at + mine[k]];
            const int row = s_row[at + mine[k]];
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

        // the rows without a pair: round one's wait for the spawn (thread r % 64 remembers row r), round two's get no id
#pragma unroll
        for (int q = 0; q < kMaxDets / kWave; q++) {
            const int r = q * kWave + lane;
            const bool paired = r < R && s_row_col[r] >= 0;
            if (round == 0) {
                if (r < R && !paired) unmatched |= 1u << q;
            } else {
                n_rescued += __popcll(__ballot(paired));
                if (r < R && !paired) {                            // MOTION: the row's own box, no velocity
                    const int row = s_row[at + r];
                    out_id[row] = 0;
                    out_hits[row] = 0;
                    if constexpr (MOTION) out_box[row] = s_box[at + r], out_vel[row] = zero4;
                }
            }
        }
        __syncthreads();                                           // the tables are read before the next round resets them
    }
    if (P == 0 && PL == 0) __syncthreads();                        // (uniform) the staged rows, which no round waited for

    // ---- spawn: the k-th unmatched row takes the k-th free slot and the id next_id + k (MOTION: at rest)
    int n_unmatched = 0;
#pragma unroll
    for (int q = 0; q < kMaxDets / kWave; q++) {
        const bool is_mine = (unmatched >> q) & 1u;
        const uint64_t mask = __ballot(is_mine);
        if (is_mine) s_spawn[n_unmatched + lanes_below(mask, lane)] = q * kWave + lane;
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
                    const int64_t to = base + n_coast + lanes_below(mask, lane);
                    o.coast_id[to] = id[k];
                    o.coast_box[to] = pred[k];
                    o.coast_label[to] = label[k];
                    o.coast_age[to] = now - seen[k];
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

bool sizes_ok(int32_t B, int32_t M) { return B >= 1 && B <= 65535 && M >= 1 && M <= kMaxTracks; }
size_t workspace_bytes(int32_t B, int32_t M) { return align_up(4 * (size_t)B * lane_words(M), 16); }

}  // namespace
}  // namespace dagr

using namespace dagr;

#define OPTIMAL_CHECK_ARG(cond, msg) DAGR_CHECK_ARG(cond, std::string("stream track optimal: ") + (msg))

extern "C" size_t dagr_stream_track_optimal_bytes(int32_t B, int32_t max_tracks) {
    return sizes_ok(B, max_tracks) ? workspace_bytes(B, max_tracks) : 0;
}

extern "C" int dagr_stream_track_optimal(void *tracks, size_t bytes, int32_t B, int32_t max_tracks, float iou,
                                         int64_t max_age_us, float min_score, float alpha, float beta, const float *det,
                                         const int32_t *n_keep, int32_t A, const int64_t *t_ref, int64_t *track_id,
                                         int32_t *track_hits, float *track_box, float *track_vel, int64_t *coast_id,
                                         float *coast_box, int32_t *coast_label, int64_t *coast_age_us, int32_t *n_coast,
                                         int64_t *untracked, float low_score, float low_iou, int64_t *rescued, int32_t flags,
                                         void *ws, size_t ws_bytes, void *stream) {
    OPTIMAL_CHECK_ARG((flags & ~(DAGR_TRACK_OPTIMAL_MOTION | DAGR_TRACK_OPTIMAL_RESCUE)) == 0,
                      "unknown bits in flags (DAGR_TRACK_OPTIMAL_MOTION | DAGR_TRACK_OPTIMAL_RESCUE)");
    const bool motion = flags & DAGR_TRACK_OPTIMAL_MOTION, rescue = flags & DAGR_TRACK_OPTIMAL_RESCUE;
    if (motion) {                               // what dagr_stream_track_cv refuses in addition; without the bit nothing of it is looked at
        const bool coast = coast_id || coast_box || coast_label || coast_age_us || n_coast;
        OPTIMAL_CHECK_ARG(max_age_us <= DAGR_TRACK_CV_MAX_AGE_US,
                          "motion: max_age_us must not exceed DAGR_TRACK_CV_MAX_AGE_US = 2^24 - 1 (a live track's age is exact in fp32)");
        OPTIMAL_CHECK_ARG(alpha > 0.0f && alpha <= 1.0f, "motion: alpha must be in (0, 1]");
        OPTIMAL_CHECK_ARG(beta >= 0.0f && beta <= 1.0f, "motion: beta must be in [0, 1]");
        OPTIMAL_CHECK_ARG(A == 0 || (det && track_id && track_hits && track_box && track_vel),
                          "motion: NULL detections or outputs (track_id, track_hits, track_box, track_vel)");
        OPTIMAL_CHECK_ARG(!coast || (coast_id && coast_box && coast_label && coast_age_us && n_coast),
                          "motion: coast_id, coast_box, coast_label, coast_age_us and n_coast are NULL together or not at all");
        OPTIMAL_CHECK_ARG((((uintptr_t)track_box | (uintptr_t)track_vel | (uintptr_t)coast_box) & 15) == 0,
                          "motion: track_box, track_vel and coast_box must be 16-byte aligned (one store a box)");
        OPTIMAL_CHECK_ARG((((uintptr_t)coast_id | (uintptr_t)coast_age_us) & 7) == 0 &&
                              (((uintptr_t)coast_label | (uintptr_t)n_coast) & 3) == 0,
                          "motion: coast_id and coast_age_us must be 8-byte aligned, coast_label and n_coast 4-byte");
    }
    OPTIMAL_CHECK_ARG(sizes_ok(B, max_tracks), "B or max_tracks out of range (1 .. DAGR_TRACK_MAX_TRACKS)");
    OPTIMAL_CHECK_ARG(iou > 0.0f && iou <= 1.0f, "iou must be in (0, 1]");
    OPTIMAL_CHECK_ARG(max_age_us >= 0, "max_age_us must not be negative");
    OPTIMAL_CHECK_ARG(A >= 0 && A <= (1 << 24), "A out of range");
    OPTIMAL_CHECK_ARG(tracks && n_keep && t_ref, "NULL pointer");
    OPTIMAL_CHECK_ARG(A == 0 || (det && track_id && track_hits), "NULL detections or outputs");
    OPTIMAL_CHECK_ARG(((uintptr_t)tracks & 15) == 0 && (((uintptr_t)t_ref | (uintptr_t)track_id | (uintptr_t)untracked) & 7) == 0 &&
                          (((uintptr_t)det | (uintptr_t)n_keep | (uintptr_t)track_hits) & 3) == 0,
                      "tracks must be 16-byte aligned, int64 arrays 8-byte, fp32 / int32 arrays 4-byte");
    Tracks st;
    OPTIMAL_CHECK_ARG(bytes >= carve_tracks(motion, B, max_tracks, (char *)tracks, &st),
                      motion ? "state smaller than dagr_stream_track_cv_bytes" : "state smaller than dagr_stream_track_bytes");
    if (rescue) {                               // what the _rescue entries refuse in addition
        OPTIMAL_CHECK_ARG(low_score == low_score, "rescue: low_score is NaN");
        OPTIMAL_CHECK_ARG(low_score < min_score, "rescue: low_score must be below min_score (no score lies in between; raise min_score)");
        OPTIMAL_CHECK_ARG(low_iou > 0.0f && low_iou <= 1.0f, "rescue: low_iou must be in (0, 1]");
        OPTIMAL_CHECK_ARG(((uintptr_t)rescued & 7) == 0, "rescue: rescued must be 8-byte aligned");
    }
    OPTIMAL_CHECK_ARG(ws != nullptr, "the workspace is NULL");
    OPTIMAL_CHECK_ARG(((uintptr_t)ws & 15) == 0, "the workspace must be 16-byte aligned");
    OPTIMAL_CHECK_ARG(ws_bytes >= workspace_bytes(B, max_tracks), "workspace smaller than dagr_stream_track_optimal_bytes");

    const MotionOut o = {(float4 *)track_box, (float4 *)track_vel, coast_id, (float4 *)coast_box, coast_label, coast_age_us, n_coast};
#define OPTIMAL_LAUNCH(MOTION, RESCUE)                                                                                      \
    k_stream_track_optimal<MOTION, RESCUE><<<(unsigned)B, kWave, 0, (hipStream_t)stream>>>(                                  \
        max_tracks, iou, max_age_us, min_score, det, n_keep, A, t_ref, track_id, track_hits, untracked, st, alpha, beta, o, \
        low_score, low_iou, rescued, (int32_t *)ws)
    if (motion && rescue) OPTIMAL_LAUNCH(true, true);
    else if (motion) OPTIMAL_LAUNCH(true, false);
    else if (rescue) OPTIMAL_LAUNCH(false, true);
    else OPTIMAL_LAUNCH(false, false);
#undef OPTIMAL_LAUNCH
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
