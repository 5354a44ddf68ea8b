// stream_identity.hip -- the event stream's identity state (dagr_stream_identity, dagr_stream_identity_solve): behind the
// scorer's step (stream_score.hip) on the same arrays, per lane the number of steps every (object identity, track id) pair
// overlapped, and on request the maximum-weight pairing of identities with track ids on those counts -- IDF1's idtp, idfn
// and idfp.  dagr_amd/streaming.py: IdentityDefinition is the same in numpy, integer for integer; include/dagr_hip.h
// states the rule and the state's layout.
//
// One workgroup of ONE wave per lane, as the scorer has it; the lane's wave owns the lane's state, so there is no atomic.
// The step: hypotheses, duplicates, the lookup of columns and slots and the rows that count are stream_eval.hpp's stages,
// as are both states' layouts.  Its own:
//   columns: new ids take the columns behind n_tracks in row order, counted by ballot + popcount; a full table lists no more;
//   pairs:   a serial walk over the counted rows (a ballot mask), the work of a row parallel over the hypotheses: a
//            hypothesis owns its column and a row its slot, so every word of `overlap` has one writer per row.
// The solve is assign.hpp's routine on the lane's `overlap`.  Every float decision repeats the numpy definition operation
// by operation; this library is built with -ffp-contract=off, and the fp32 division is correctly rounded.
#include "assign.hpp"
#include "stream_eval.hpp"

namespace dagr {
namespace {

using namespace identity_word;
static_assert(kMaxObjects <= kAssignMax, "one staging table for the track ids and the object ids");

__global__ __launch_bounds__(kWave) void k_stream_identity(int M, int T, float thr, const int64_t *__restrict__ score_id,
                                                           const int64_t *__restrict__ score_words,
                                                           const float *__restrict__ det, const int32_t *__restrict__ n_keep,
                                                           int A, const int64_t *__restrict__ track_id,
                                                           const float4 *__restrict__ track_box,
                                                           const float4 *__restrict__ gt_box, const int32_t *__restrict__ gt_label,
                                                           const int64_t *__restrict__ gt_id, const int32_t *__restrict__ n_gt,
                                                           int G, const int64_t *__restrict__ gt_match, Identity st) {
    __shared__ float4 s_hbox[kMaxHyp];          // the hypotheses, in row order (stage_hypotheses)
    __shared__ int64_t s_hid[kMaxHyp];
    __shared__ int32_t s_hlabel[kMaxHyp];
    __shared__ float4 s_gbox[kMaxGt];           // the ground-truth rows
    __shared__ int32_t s_glabel[kMaxGt];
    __shared__ int32_t s_gslot[kMaxGt];         // the slot of a counted row
    __shared__ int64_t s_table[kAssignMax];     // the lane's track ids, then the scorer's object ids

    const int b = blockIdx.x, lane = threadIdx.x;
    const int labelled = n_gt[b];
    if (labelled < 0) return;                   // no labels at this instant: not one byte of the lane changes
    const int ng = min(labelled, G);
    const int n = min(max(n_keep[b], 0), A);
    int64_t *words = st.lane + (int64_t)b * identity_word::kCount;
    const int n_tr = table_fill(words[kNTracks], T);
    const int n_obj = table_fill(score_words[(int64_t)b * score_word::kCount + score_word::kNObjects], M);

    const int P = min(stage_hypotheses(b, lane, n, A, det, track_id, track_box, s_hbox, s_hid, s_hlabel), kMaxHyp);
    int64_t gid[kGtRegs];
    bool scored[kGtRegs];
    stage_scored_rows(b, lane, ng, G, gt_box, gt_label, gt_id, gt_match, s_gbox, s_glabel, gid, scored);
    for (int k = lane; k < n_tr; k += kWave) s_table[k] = st.track_id[(int64_t)b * T + k];
    __syncthreads();

    float4 hbox[kHypRegs];
    int32_t hlabel[kHypRegs];
    int64_t hid[kHypRegs];                      // 0: no hypothesis in this register
    int col[kHypRegs];
    bool dup[kHypRegs];
    load_hypotheses(lane, P, s_hbox, s_hid, s_hlabel, hbox, hlabel, hid);
    mark_duplicates(lane, P, s_hid, hid, dup);
    find_columns(n_tr, s_table, hid, col);

    // ---- columns: by id, or the columns behind n_tracks in row order; a full table lists no more
    int n_new = 0, n_dup = 0, n_unlisted = 0;
#pragma unroll
    for (int k = 0; k < kHypRegs; k++) {
        const bool takes_part = hid[k] != 0 && !dup[k];
        const bool fresh = takes_part && col[k] < 0;
        const uint64_t mask = __ballot(fresh);
        bool unlisted = false;
        if (fresh) {
            const int c = n_tr + n_new + lanes_below(mask, lane);
            if (c < T) {
                col[k] = c;
                st.track_id[(int64_t)b * T + c] = hid[k];
            } else {
                unlisted = true;
            }
        }
        if (!takes_part) col[k] = -1;
        if (col[k] >= 0) st.track_len[(int64_t)b * T + col[k]] += 1;          // (distinct ids: one writer a column)
        n_new += __popcll(mask);
        n_dup += __popcll(__ballot(hid[k] != 0 && dup[k]));
        n_unlisted += __popcll(__ballot(unlisted));
    }
    __syncthreads();                            // (every thread is done with the track ids in s_table)

    // ---- rows: the rows the scorer scored, at the slot of their identity in the scorer's table
    for (int k = lane; k < n_obj; k += kWave) s_table[k] = score_id[(int64_t)b * M + k];
    __syncthreads();
    int slot[kGtRegs];
    find_slots(n_obj, s_table, gid, scored, slot);
    uint64_t counted[kGtRegs];
    int n_rows = 0, top = 0;
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        const int g = j * kWave + lane;
        if (slot[j] >= 0) {
            st.obj_len[(int64_t)b * M + slot[j]] += 1;                      // (scored rows have distinct identities)
            top = max(top, slot[j] + 1);
        }
        if (g < ng) s_gslot[g] = slot[j];
        counted[j] = __ballot(slot[j] >= 0);
        n_rows += __popcll(counted[j]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top = max(top, __shfl_xor(top, off, kWave));
    __syncthreads();

    // ---- pairs: every counted row against every hypothesis with a column
    int n_pairs = 0;
    int32_t *lane_overlap = st.overlap + (int64_t)b * M * T;
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        for (uint64_t m = counted[j]; m; m &= m - 1) {
            const int g = j * kWave + first_lane(m);
            const float4 d = s_gbox[g];
            const int32_t cls = s_glabel[g];
            int32_t *row = lane_overlap + (int64_t)s_gslot[g] * T;
#pragma unroll
            for (int k = 0; k < kHypRegs; k++) {
                if (col[k] < 0 || hlabel[k] != cls) continue;
                const float v = iou_xyxy(d, hbox[k]);
                if (!(v >= thr)) continue;                                  // (a NaN IoU overlaps nothing)
                row[col[k]] += 1;
                n_pairs++;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_pairs += __shfl_xor(n_pairs, off, kWave);
    if (lane == 0) {
        words[kNTracks] = min(n_tr + n_new, T);
        words[kNObjects] = max(words[kNObjects], (int64_t)top);
        words[kGtFrames] += n_rows;
        words[kHypFrames] += P - n_dup;
        words[kDupHyp] += n_dup;
        words[kUnlistedHyp] += n_unlisted;
        words[kPairs] += n_pairs;
        words[kSteps] += 1;
    }
}

__global__ __launch_bounds__(kWave) void k_stream_identity_solve(int M, int T, Identity st, int64_t *__restrict__ obj_track,
                                                                 int64_t *__restrict__ result, int32_t *__restrict__ workspace) {
    __shared__ AssignLds s;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t *words = st.lane + (int64_t)b * identity_word::kCount;
    const int n_tr = table_fill(words[kNTracks], T);
    const int n_obj = table_fill(words[kNObjects], M);
    int32_t *pairs = st.obj_col + (int64_t)b * M;
    for (int r = n_obj + lane; r < M; r += kWave) pairs[r] = -1;
    const int64_t idtp = assign_wave(st.overlap + (int64_t)b * M * T, T, n_obj, n_tr, workspace + (int64_t)b * M * T, pairs, s);
    __syncthreads();                            // (the pairing: written by this workgroup, read by it)
    for (int r = lane; r < M; r += kWave) {
        const int c = pairs[r];
        obj_track[(int64_t)b * M + r] = c >= 0 ? st.track_id[(int64_t)b * T + c] : 0;
    }
    if (lane == 0) {
        int64_t *out = result + (int64_t)b * DAGR_IDENTITY_RESULT_WORDS;
        out[0] = idtp;
        out[1] = words[kGtFrames] - idtp;
        out[2] = words[kHypFrames] - idtp;
        out[3] = words[kGtFrames];
        out[4] = words[kHypFrames];
        out[5] = n_obj;
        out[6] = n_tr;
        out[7] = words[kDupHyp];
        out[8] = words[kUnlistedHyp];
    }
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" size_t dagr_stream_identity_bytes(int32_t B, int32_t max_objects, int32_t max_tracks) {
    return identity_sizes_ok(B, max_objects, max_tracks) ? carve_identity(B, max_objects, max_tracks, nullptr, nullptr) : 0;
}

extern "C" int dagr_stream_identity_reset(void *state, size_t bytes, int32_t B, int32_t max_objects, int32_t max_tracks,
                                          void *stream) {
    DAGR_CHECK_ARG(state != nullptr, "stream identity: state is NULL");
    DAGR_CHECK_ARG(identity_sizes_ok(B, max_objects, max_tracks),
                   "stream identity: B, max_objects (1 .. DAGR_SCORE_MAX_OBJECTS) or max_tracks (1 .. DAGR_ASSIGN_MAX) out of range");
    DAGR_CHECK_ARG(((uintptr_t)state & 15) == 0, "stream identity: state must be 16-byte aligned");
    const size_t need = carve_identity(B, max_objects, max_tracks, nullptr, nullptr);
    DAGR_CHECK_ARG(bytes >= need, "stream identity: state smaller than dagr_stream_identity_bytes");
    DAGR_CHECK_HIP(hipMemsetAsync(state, 0, need, (hipStream_t)stream));
    return DAGR_OK;
}

extern "C" int dagr_stream_identity(void *state, size_t bytes, int32_t B, int32_t max_objects, int32_t max_tracks, float iou,
                                    const void *score_state, size_t score_bytes, const float *det, const int32_t *n_keep,
                                    int32_t A, const int64_t *track_id, const float *track_box, const float *gt_box,
                                    const int32_t *gt_label, const int64_t *gt_id, const int32_t *n_gt, int32_t G,
                                    const int64_t *gt_match, void *stream) {
    DAGR_CHECK_ARG(identity_sizes_ok(B, max_objects, max_tracks),
                   "stream identity: B, max_objects (1 .. DAGR_SCORE_MAX_OBJECTS) or max_tracks (1 .. DAGR_ASSIGN_MAX) out of range");
    DAGR_CHECK_ARG(iou > 0.0f && iou <= 1.0f, "stream identity: iou must be in (0, 1]");
    DAGR_CHECK_ARG(A >= 0 && A <= (1 << 24), "stream identity: A out of range");
    DAGR_CHECK_ARG(G >= 0 && G <= kMaxGt, "stream identity: G out of range (0 .. DAGR_SCORE_MAX_GT)");
    DAGR_CHECK_ARG(state && score_state && n_keep && n_gt, "stream identity: NULL pointer");
    DAGR_CHECK_ARG(A == 0 || (det && track_id), "stream identity: NULL detections or track ids");
    DAGR_CHECK_ARG(G == 0 || (gt_box && gt_label && gt_id && gt_match), "stream identity: NULL ground truth");
    DAGR_CHECK_ARG((((uintptr_t)state | (uintptr_t)score_state | (uintptr_t)track_box | (uintptr_t)gt_box) & 15) == 0 &&
                       (((uintptr_t)track_id | (uintptr_t)gt_id | (uintptr_t)gt_match) & 7) == 0 &&
                       (((uintptr_t)det | (uintptr_t)n_keep | (uintptr_t)gt_label | (uintptr_t)n_gt) & 3) == 0,
                   "stream identity: the states, track_box and gt_box must be 16-byte aligned, int64 arrays 8-byte, fp32 / int32 "
                   "arrays 4-byte");
    Identity st;
    DAGR_CHECK_ARG(bytes >= carve_identity(B, max_objects, max_tracks, (char *)state, &st),
                   "stream identity: state smaller than dagr_stream_identity_bytes");
    DAGR_CHECK_ARG(score_bytes >= dagr_stream_score_bytes(B, max_objects),
                   "stream identity: score_state smaller than dagr_stream_score_bytes");
    Score score;                                // (read only: the kernel takes its id table and its words as const)
    carve_score(B, max_objects, (char *)score_state, &score);
    k_stream_identity<<<(unsigned)B, kWave, 0, (hipStream_t)stream>>>(max_objects, max_tracks, iou, score.id, score.lane, det,
                                                                      n_keep, A, track_id, (const float4 *)track_box,
                                                                      (const float4 *)gt_box, gt_label, gt_id, n_gt, G, gt_match,
                                                                      st);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

extern "C" int dagr_stream_identity_solve(void *state, size_t bytes, int32_t B, int32_t max_objects, int32_t max_tracks,
                                          int64_t *obj_track, int64_t *result, void *workspace, size_t workspace_bytes,
                                          void *stream) {
    DAGR_CHECK_ARG(identity_sizes_ok(B, max_objects, max_tracks),
                   "stream identity: B, max_objects (1 .. DAGR_SCORE_MAX_OBJECTS) or max_tracks (1 .. DAGR_ASSIGN_MAX) out of range");
    DAGR_CHECK_ARG(state && obj_track && result && workspace, "stream identity: NULL pointer");
    DAGR_CHECK_ARG((((uintptr_t)state | (uintptr_t)workspace) & 15) == 0 && (((uintptr_t)obj_track | (uintptr_t)result) & 7) == 0,
                   "stream identity: state and workspace must be 16-byte aligned, obj_track and result 8-byte");
    Identity st;
    DAGR_CHECK_ARG(bytes >= carve_identity(B, max_objects, max_tracks, (char *)state, &st),
                   "stream identity: state smaller than dagr_stream_identity_bytes");
    DAGR_CHECK_ARG(workspace_bytes >= assign_workspace_bytes(B, max_objects, max_tracks),
                   "stream identity: workspace smaller than dagr_assign_workspace_bytes");
    k_stream_identity_solve<<<(unsigned)B, kWave, 0, (hipStream_t)stream>>>(max_objects, max_tracks, st, obj_track, result,
                                                                            (int32_t *)workspace);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
