// stream_score.hip -- the event stream's scorer (dagr_stream_score): the track ids a dagr_stream_track* entry left for a
// step are scored against ground-truth boxes that carry an identity, and the CLEAR-MOT counts (misses, false positives,
// identity switches, fragmentations) accumulate in a caller-owned state.  dagr_amd/streaming.py: ScoreDefinition is the
// same in numpy, integer for integer; include/dagr_hip.h states the rule and the state's layout.
//
// One workgroup of ONE wave per lane, as k_stream_track has it; the lane's wave owns the lane's state, so there is no
// atomic and no second launch.  The state's layout, the staging of the hypotheses and a thread's registers are
// stream_eval.hpp's; the ground-truth rows and the ids of the lane's object table are staged in LDS beside them, 24 KB.
//   slots: the scorer's own rule, for it makes the slots the identity step and HOTA look up: every thread scans the rows
//          for an earlier carrier of its identities (those rows are unscored) and the staged table for their slots (one
//          broadcast LDS read per word, four compares);
//          new identities take the slots behind n_objects in row order, counted by ballot + popcount;
//   keep:  a serial walk over the rows whose object was matched at the step before (a ballot mask, so only they cost
//          anything): the first hypothesis with the remembered id is found by ballot, the test itself is uniform;
//   match: a serial walk over the other scored rows, as greedy matching is; the work of a row is parallel over the
//          hypotheses, and the (largest IoU, lowest row) choice is a ballot in the usual case of one candidate and a shuffle
//          reduction otherwise -- the structure of k_stream_track's match.  Which hypotheses are taken is a uniform 64-bit
//          mask per hypothesis register, so the walks have no barrier; they stop when every hypothesis is taken;
//   count: parallel over the rows: a scored row owns its slot (duplicates are unscored), so every table word has one writer.
// The counters are summed by ballot + popcount (iou_q by a shuffle reduction of int64) and stored once, by thread 0.
// Every float decision repeats the numpy definition operation by operation; this library is built with -ffp-contract=off,
// and the fp32 division is correctly rounded.
#include "stream_eval.hpp"

namespace dagr {
namespace {

using namespace score_word;

__device__ __forceinline__ int32_t iou_units(float v) { return (int32_t)rintf(v * kIouOne); }      // exact: v <= 1

__global__ __launch_bounds__(kWave) void k_stream_score(int M, float thr, const float *__restrict__ det,
                                                        const int32_t *__restrict__ n_keep, int A,
                                                        const int64_t *__restrict__ track_id,
                                                        const float4 *__restrict__ track_box,
                                                        const float4 *__restrict__ gt_box, const int32_t *__restrict__ gt_label,
                                                        const int64_t *__restrict__ gt_id, const int32_t *__restrict__ n_gt,
                                                        int G, int64_t *__restrict__ gt_match, int32_t *__restrict__ gt_flags,
                                                        Score st) {
    __shared__ float4 s_hbox[kMaxHyp];          // the participating hypotheses, in row order
    __shared__ int64_t s_hid[kMaxHyp];
    __shared__ int32_t s_hlabel[kMaxHyp];
    __shared__ float4 s_gbox[kMaxGt];           // the ground-truth rows
    __shared__ int64_t s_gid[kMaxGt];
    __shared__ int64_t s_gprev[kMaxGt];         // prev_hyp of the rows that go through the keep round
    __shared__ int32_t s_glabel[kMaxGt];
    __shared__ int64_t s_obj[kMaxObjects];      // the ids of the lane's table

    const int b = blockIdx.x, lane = threadIdx.x;
    const int labelled = n_gt[b];
    if (labelled < 0) return;                   // no labels at this instant: not one byte of the lane changes
    const int ng = min(labelled, G);
    const int n = min(max(n_keep[b], 0), A);
    int64_t *words = st.lane + (int64_t)b * score_word::kCount;
    const int n_obj = table_fill(words[kNObjects], M);
    const int64_t steps = words[kSteps];
    const int64_t base = (int64_t)b * M;

    const int n_hyp = stage_hypotheses(b, lane, n, A, det, track_id, track_box, s_hbox, s_hid, s_hlabel);
    const int P = min(n_hyp, kMaxHyp);
    for (int g = lane; g < ng; g += kWave) {
        s_gbox[g] = gt_box[(int64_t)b * G + g];
        s_glabel[g] = gt_label[(int64_t)b * G + g];
        s_gid[g] = gt_id[(int64_t)b * G + g];
    }
    for (int k = lane; k < n_obj; k += kWave) s_obj[k] = st.id[base + k];
    __syncthreads();

    float4 hbox[kHypRegs];
    int32_t hlabel[kHypRegs];
    int64_t hid[kHypRegs];                      // 0: no hypothesis in this register
    load_hypotheses(lane, P, s_hbox, s_hid, s_hlabel, hbox, hlabel, hid);

    // ---- slots: a row is scored unless its id is <= 0, an earlier row has it, or it is new and the table is full
    int64_t gid[kGtRegs], prev[kGtRegs];
    int slot[kGtRegs];
    bool scored[kGtRegs];
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        const int g = j * kWave + lane;
        gid[j] = g < ng ? s_gid[g] : 0;
        scored[j] = gid[j] > 0;
        slot[j] = -1, prev[j] = 0;
    }
    for (int g2 = 0; g2 < ng; g2++) {
        const int64_t v = s_gid[g2];
#pragma unroll
        for (int j = 0; j < kGtRegs; j++)
            if (g2 < j * kWave + lane && v == gid[j]) scored[j] = false;
    }
    for (int k = 0; k < n_obj; k++) {
        const int64_t v = s_obj[k];
#pragma unroll
        for (int j = 0; j < kGtRegs; j++)
            if (v == gid[j]) slot[j] = k;
    }
    int n_new = 0;
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        const bool fresh = scored[j] && slot[j] < 0;
        const uint64_t mask = __ballot(fresh);
        if (fresh) {
            const int s = n_obj + n_new + lanes_below(mask, lane);
            if (s < M) {
                slot[j] = s;
                st.id[base + s] = gid[j];       // (its other words are what the reset left: never seen, no hypothesis)
            } else {
                scored[j] = false;
            }
        }
        n_new += __popcll(mask);
    }
    uint64_t scored_mask[kGtRegs], keep_mask[kGtRegs], kept_mask[kGtRegs];
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        bool wants = false;
        if (scored[j]) {
            prev[j] = st.prev_hyp[base + slot[j]];
            wants = prev[j] != 0 && st.seen_step[base + slot[j]] == steps - 1;
            if (wants) s_gprev[j * kWave + lane] = prev[j];
        }
        scored_mask[j] = __ballot(scored[j]);
        keep_mask[j] = __ballot(wants);
        kept_mask[j] = 0;
    }
    __syncthreads();

    // ---- keep, then match.  `taken` is uniform: bit l of taken[k] is hypothesis k * 64 + l.  The thread that owns a row
    // remembers the row's track id and IoU.
    uint64_t taken[kHypRegs];
#pragma unroll
    for (int k = 0; k < kHypRegs; k++) taken[k] = 0;
    int n_taken = 0;
    int64_t m_id[kGtRegs];
    int32_t m_q[kGtRegs];
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) m_id[j] = 0, m_q[j] = 0;

#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        for (uint64_t m = keep_mask[j]; m; m &= m - 1) {
            const int l = first_lane(m), g = j * kWave + l;
            const int64_t want = s_gprev[g];
            int p = -1;
#pragma unroll
            for (int k = 0; k < kHypRegs; k++) {                       // the FIRST hypothesis with that id
                const uint64_t has = __ballot(hid[k] == want);
                if (p < 0 && has) p = k * kWave + first_lane(has);
            }
            if (p < 0) continue;
            bool is_free = true;
#pragma unroll
            for (int k = 0; k < kHypRegs; k++)
                if (k == (p >> 6) && ((taken[k] >> (p & 63)) & 1ull)) is_free = false;
            if (!is_free || s_hlabel[p] != s_glabel[g]) continue;
            const float v = iou_xyxy(s_gbox[g], s_hbox[p]);
            if (!(v >= thr)) continue;                                 // (a NaN IoU keeps nothing)
#pragma unroll
            for (int k = 0; k < kHypRegs; k++)
                if (k == (p >> 6)) taken[k] |= 1ull << (p & 63);
            n_taken++;
            kept_mask[j] |= 1ull << l;
            if (lane == l) m_id[j] = want, m_q[j] = iou_units(v);
        }
    }

#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        for (uint64_t m = scored_mask[j] & ~kept_mask[j]; m && n_taken < P; m &= m - 1) {
            const int l = first_lane(m), g = j * kWave + l;
            const float4 d = s_gbox[g];
            const int32_t cls = s_glabel[g];
            float best = 0.0f;
            int best_k = -1;
#pragma unroll
            for (int k = 0; k < kHypRegs; k++) {
                if (hid[k] == 0 || hlabel[k] != cls || ((taken[k] >> lane) & 1ull)) continue;
                const float v = iou_xyxy(d, hbox[k]);
                if (!(v >= thr)) continue;                             // (a NaN IoU matches nothing)
                if (best_k < 0 || v > best) best = v, best_k = k;      // (ascending k: the lowest row of equals)
            }
            uint64_t cand = __ballot(best_k >= 0);
            if (cand == 0) continue;
            if (cand & (cand - 1)) {                                   // several threads have one: largest IoU, lowest row
                float top = best_k >= 0 ? best : -1.0f;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) top = fmaxf(top, __shfl_xor(top, off, kWave));
                cand = __ballot(best_k >= 0 && best == top);
                if (cand & (cand - 1)) {
                    const int mine = (best_k >= 0 && best == top) ? best_k * kWave + lane : INT32_MAX;
                    int low = mine;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) low = min(low, __shfl_xor(low, off, kWave));
                    cand = __ballot(mine == low && mine != INT32_MAX);
                }
            }
            const int w = first_lane(cand);
            const int wk = __shfl(best_k, w, kWave);
            const float wv = __shfl(best, w, kWave);
#pragma unroll
            for (int k = 0; k < kHypRegs; k++)
                if (k == wk) taken[k] |= 1ull << w;
            n_taken++;
            if (lane == l) m_id[j] = s_hid[wk * kWave + w], m_q[j] = iou_units(wv);
        }
    }

    // ---- count: a scored row owns its slot
    int n_scored = 0, n_switch = 0, n_frag = 0, n_kept = 0;
    int64_t q_sum = 0;
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        const int g = j * kWave + lane;
        const bool matched = scored[j] && m_id[j] != 0;
        bool sw = false, fr = false;
        if (scored[j]) {
            const int64_t at = base + slot[j];
            st.present[at] += 1;
            st.seen_step[at] = steps;
            if (matched) {
                const int64_t last = st.last_hyp[at], tracked = st.tracked[at];
                sw = last != 0 && last != m_id[j];
                fr = tracked > 0 && prev[j] == 0;
                st.tracked[at] = tracked + 1;
                st.last_hyp[at] = m_id[j];
                st.prev_hyp[at] = m_id[j];
                if (sw) st.switches[at] += 1;
                if (fr) st.frags[at] += 1;
                q_sum += m_q[j];
            } else {
                st.prev_hyp[at] = 0;
            }
        }
        if (gt_match && g < ng) {
            gt_match[(int64_t)b * G + g] = scored[j] ? m_id[j] : -1;
            gt_flags[(int64_t)b * G + g] = (sw ? 1 : 0) | (fr ? 2 : 0) | (int)((kept_mask[j] >> lane) & 1ull) * 4;
        }
        n_scored += __popcll(scored_mask[j]);
        n_switch += __popcll(__ballot(sw));
        n_frag += __popcll(__ballot(fr));
        n_kept += __popcll(kept_mask[j]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q_sum += __shfl_xor(q_sum, off, kWave);
    if (lane == 0) {
        words[kNObjects] = min(n_obj + n_new, M);
        words[kSteps] = steps + 1;
        words[kGt] += n_scored;
        words[kHyp] += P;
        words[kMatch] += n_taken;
        words[kMiss] += n_scored - n_taken;
        words[kFalsePos] += P - n_taken;
        words[kSwitch] += n_switch;
        words[kFrag] += n_frag;
        words[kKept] += n_kept;
        words[kIouQ] += q_sum;
        words[kUnscoredGt] += ng - n_scored;
        words[kUnscoredHyp] += n_hyp - P;
    }
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" size_t dagr_stream_score_bytes(int32_t B, int32_t max_objects) {
    return score_sizes_ok(B, max_objects) ? carve_score(B, max_objects, nullptr, nullptr) : 0;
}

extern "C" int dagr_stream_score_reset(void *state, size_t bytes, int32_t B, int32_t max_objects, void *stream) {
    DAGR_CHECK_ARG(state != nullptr, "stream score: state is NULL");
    DAGR_CHECK_ARG(score_sizes_ok(B, max_objects), "stream score: B or max_objects out of range (1 .. DAGR_SCORE_MAX_OBJECTS)");
    DAGR_CHECK_ARG(((uintptr_t)state & 15) == 0, "stream score: state must be 16-byte aligned");
    Score st;
    const size_t need = carve_score(B, max_objects, (char *)state, &st);
    DAGR_CHECK_ARG(bytes >= need, "stream score: state smaller than dagr_stream_score_bytes");
    DAGR_CHECK_HIP(hipMemsetAsync(state, 0, need, (hipStream_t)stream));
    // seen_step = -1, "never": every byte 0xff
    DAGR_CHECK_HIP(hipMemsetAsync(st.seen_step, 0xff, 8 * (size_t)B * max_objects, (hipStream_t)stream));
    return DAGR_OK;
}

extern "C" int dagr_stream_score(void *state, size_t bytes, int32_t B, int32_t max_objects, float iou, const float *det,
                                 const int32_t *n_keep, int32_t A, const int64_t *track_id, const float *track_box,
                                 const float *gt_box, const int32_t *gt_label, const int64_t *gt_id, const int32_t *n_gt,
                                 int32_t G, int64_t *gt_match, int32_t *gt_flags, void *stream) {
    DAGR_CHECK_ARG(score_sizes_ok(B, max_objects), "stream score: B or max_objects out of range (1 .. DAGR_SCORE_MAX_OBJECTS)");
    DAGR_CHECK_ARG(iou > 0.0f && iou <= 1.0f, "stream score: iou must be in (0, 1]");
    DAGR_CHECK_ARG(A >= 0 && A <= (1 << 24), "stream score: A out of range");
    DAGR_CHECK_ARG(G >= 0 && G <= kMaxGt, "stream score: G out of range (0 .. DAGR_SCORE_MAX_GT)");
    DAGR_CHECK_ARG(state && n_keep && n_gt, "stream score: NULL pointer");
    DAGR_CHECK_ARG(A == 0 || (det && track_id), "stream score: NULL detections or track ids");
    DAGR_CHECK_ARG(G == 0 || (gt_box && gt_label && gt_id), "stream score: NULL ground truth");
    DAGR_CHECK_ARG((gt_match == nullptr) == (gt_flags == nullptr),
                   "stream score: gt_match and gt_flags are NULL together or not at all");
    DAGR_CHECK_ARG((((uintptr_t)state | (uintptr_t)track_box | (uintptr_t)gt_box) & 15) == 0 &&
                       (((uintptr_t)track_id | (uintptr_t)gt_id | (uintptr_t)gt_match) & 7) == 0 &&
                       (((uintptr_t)det | (uintptr_t)n_keep | (uintptr_t)gt_label | (uintptr_t)n_gt | (uintptr_t)gt_flags) & 3) == 0,
                   "stream score: state, track_box and gt_box must be 16-byte aligned, int64 arrays 8-byte, fp32 / int32 arrays 4-byte");
    Score st;
    DAGR_CHECK_ARG(bytes >= carve_score(B, max_objects, (char *)state, &st), "stream score: state smaller than dagr_stream_score_bytes");
    k_stream_score<<<(unsigned)B, kWave, 0, (hipStream_t)stream>>>(max_objects, iou, det, n_keep, A, track_id,
                                                                   (const float4 *)track_box, (const float4 *)gt_box, gt_label,
                                                                   gt_id, n_gt, G, gt_match, gt_flags, st);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
