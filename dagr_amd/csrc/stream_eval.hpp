// stream_eval.hpp -- the labelled step, stated once for the kernels that run it behind the tracker: the scorer
// (stream_score.hip), the identity step (stream_identity.hip) and HOTA's pass 1 (stream_hota.hip).  Which rows of a step
// are hypotheses, which labelled rows count, and where the scorer's and the identity state's tables lie.
// dagr_amd/streaming.py holds the same rule in numpy (_labelled_step, _lane_hypotheses, _lane_scored_rows);
// include/dagr_hip.h documents the layouts.
//
// Every kernel here is one workgroup of ONE wave per lane.  A thread owns the hypotheses `lane`, `lane + 64`, ...
// (kHypRegs = 4) and the ground-truth rows `lane`, `lane + 64`, ... (kGtRegs = 4) in registers; the stages below take those
// registers as references to arrays and the kernel's own __shared__ arrays as pointers, so that a kernel keeps its LDS in
// the order it declares it.  Every stage is called by all 64 threads with uniform arguments.
#pragma once
#include "stream_box.hpp"

namespace dagr {

constexpr int kMaxObjects = DAGR_SCORE_MAX_OBJECTS;
constexpr int kMaxGt = DAGR_SCORE_MAX_GT;
constexpr int kMaxHyp = DAGR_TRACK_MAX_DETS;
constexpr int kGtRegs = kMaxGt / kWave;             // ground-truth rows of one thread
constexpr int kHypRegs = kMaxHyp / kWave;           // hypotheses of one thread
static_assert(kMaxGt % kWave == 0 && kMaxHyp % kWave == 0, "whole registers");

// ---- the scorer's state: eight int64 arrays over [B, max_objects] and the lanes' words
namespace score_word {      // a lane's int64 words, in the order include/dagr_hip.h documents
enum { kNObjects = 0, kSteps, kGt, kHyp, kMatch, kMiss, kFalsePos, kSwitch, kFrag, kKept, kIouQ, kUnscoredGt, kUnscoredHyp,
       kCount = 16 };
}

struct Score {
    int64_t *id, *last_hyp, *prev_hyp, *seen_step, *present, *tracked, *switches, *frags;
    int64_t *lane;      // [B, score_word::kCount]
};

inline size_t carve_score(int B, int M, char *base, Score *out) {
    const size_t n = (size_t)B * M;
    if (out) {
        int64_t *p = (int64_t *)base;
        *out = Score{p, p + n, p + 2 * n, p + 3 * n, p + 4 * n, p + 5 * n, p + 6 * n, p + 7 * n, p + 8 * n};
    }
    return 64 * n + 8 * (size_t)score_word::kCount * B;
}

inline bool score_sizes_ok(int32_t B, int32_t M) { return B >= 1 && B <= 65535 && M >= 1 && M <= kMaxObjects; }

// ---- the identity state
namespace identity_word {   // a lane's int64 words, in the order include/dagr_hip.h documents
enum { kNTracks = 0, kNObjects, kGtFrames, kHypFrames, kDupHyp, kUnlistedHyp, kPairs, kSteps, kCount };
}

struct Identity {
    int64_t *track_id, *track_len;      // [B, T]
    int64_t *obj_len;                   // [B, M]
    int64_t *lane;                      // [B, identity_word::kCount]
    int32_t *overlap;                   // [B, M, T]
    int32_t *obj_col;                   // [B, M]
};

inline size_t carve_identity(int B, int M, int T, char *base, Identity *out) {
    const size_t nt = (size_t)B * T, nm = (size_t)B * M;
    if (out) {
        int64_t *p = (int64_t *)base;
        int32_t *q = (int32_t *)(p + 2 * nt + nm + (size_t)identity_word::kCount * B);
        *out = Identity{p, p + nt, p + 2 * nt, p + 2 * nt + nm, q, q + nm * T};
    }
    return align_up(16 * nt + 8 * nm + 8 * (size_t)identity_word::kCount * B + 4 * nm * T + 4 * nm, 16);
}

inline bool identity_sizes_ok(int32_t B, int32_t M, int32_t T) {
    return B >= 1 && B <= 65535 && M >= 1 && M <= kMaxObjects && T >= 1 && T <= DAGR_ASSIGN_MAX;
}

// a table's fill as a lane's word has it (a state that was never reset stays inside)
__device__ __forceinline__ int table_fill(int64_t word, int cap) { return (int)min(max(word, (int64_t)0), (int64_t)cap); }

// ---- the hypotheses: the rows below n with an id, 64 at a time; the first kMaxHyp go to the LDS in row order, with
// track_box's box where there is one and the detection's otherwise.  Returns how many rows have an id: P = min(that,
// kMaxHyp) are staged.  A barrier stands between this and the first read of what it staged.
__device__ __forceinline__ int stage_hypotheses(int b, int lane, int n, int A, const float *__restrict__ det,
                                                const int64_t *__restrict__ track_id, const float4 *__restrict__ track_box,
                                                float4 *s_hbox, int64_t *s_hid, int32_t *s_hlabel) {
    int n_hyp = 0;
    for (int first = 0; first < n; first += kWave) {
        const int i = first + lane;
        const int64_t id = i < n ? track_id[(int64_t)b * A + i] : 0;
        const uint64_t mask = __ballot(id != 0);
        const int rank = n_hyp + lanes_below(mask, lane);
        n_hyp += __popcll(mask);
        if (id != 0 && rank < kMaxHyp) {
            const float *p = det + ((int64_t)b * A + i) * 6;
            s_hbox[rank] = track_box ? track_box[(int64_t)b * A + i] : make_float4(p[0], p[1], p[2], p[3]);
            s_hid[rank] = id;
            s_hlabel[rank] = (int32_t)p[5];
        }
    }
    return n_hyp;
}

// a thread's hypotheses, from the LDS to its registers; hid = 0: no hypothesis in this register
__device__ __forceinline__ void load_hypotheses(int lane, int P, const float4 *s_hbox, const int64_t *s_hid,
                                                const int32_t *s_hlabel, float4 (&hbox)[kHypRegs],
                                                int32_t (&hlabel)[kHypRegs], int64_t (&hid)[kHypRegs]) {
#pragma unroll
    for (int k = 0; k < kHypRegs; k++) {
        const int p = k * kWave + lane;
        hbox[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hlabel[k] = 0, hid[k] = 0;
        if (p < P) hbox[k] = s_hbox[p], hlabel[k] = s_hlabel[p], hid[k] = s_hid[p];
    }
}

// ---- duplicates: a hypothesis whose id an earlier one carries takes no part (the first carrier always does).  Every
// thread scans the staged ids once for its hypotheses: one broadcast LDS read per id, kHypRegs compares.
__device__ __forceinline__ void mark_duplicates(int lane, int P, const int64_t *s_hid, const int64_t (&hid)[kHypRegs],
                                                bool (&dup)[kHypRegs]) {
#pragma unroll
    for (int k = 0; k < kHypRegs; k++) dup[k] = false;
    for (int q = 0; q < P; q++) {
        const int64_t v = s_hid[q];
#pragma unroll
        for (int k = 0; k < kHypRegs; k++)
            if (q < k * kWave + lane && v == hid[k]) dup[k] = true;
    }
}

// ---- columns: the column of a hypothesis is where the staged track table has its id; -1: not listed (or no hypothesis)
__device__ __forceinline__ void find_columns(int n_tr, const int64_t *s_table, const int64_t (&hid)[kHypRegs],
                                             int (&col)[kHypRegs]) {
#pragma unroll
    for (int k = 0; k < kHypRegs; k++) col[k] = -1;
    for (int c = 0; c < n_tr; c++) {
        const int64_t v = s_table[c];
#pragma unroll
        for (int k = 0; k < kHypRegs; k++)
            if (v == hid[k]) col[k] = c;
    }
}

// ---- the ground-truth rows behind the scorer: box and label to the LDS, the identity to the thread's registers; a row is
// `scored` if the scorer's step left a gt_match other than -1 for it and its identity is positive
__device__ __forceinline__ void stage_scored_rows(int b, int lane, int ng, int G, const float4 *__restrict__ gt_box,
                                                  const int32_t *__restrict__ gt_label, const int64_t *__restrict__ gt_id,
                                                  const int64_t *__restrict__ gt_match, float4 *s_gbox, int32_t *s_glabel,
                                                  int64_t (&gid)[kGtRegs], bool (&scored)[kGtRegs]) {
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        const int g = j * kWave + lane;
        gid[j] = 0, scored[j] = false;
        if (g < ng) {
            s_gbox[g] = gt_box[(int64_t)b * G + g];
            s_glabel[g] = gt_label[(int64_t)b * G + g];
            gid[j] = gt_id[(int64_t)b * G + g];
            scored[j] = gt_match[(int64_t)b * G + g] != -1 && gid[j] > 0;
        }
    }
}

// ---- slots: a scored row counts at the first slot of the scorer's staged id table that has its identity; -1: it does not
__device__ __forceinline__ void find_slots(int n_obj, const int64_t *s_table, const int64_t (&gid)[kGtRegs],
                                           const bool (&scored)[kGtRegs], int (&slot)[kGtRegs]) {
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) slot[j] = -1;
    for (int k = 0; k < n_obj; k++) {
        const int64_t v = s_table[k];
#pragma unroll
        for (int j = 0; j < kGtRegs; j++)
            if (scored[j] && slot[j] < 0 && v == gid[j]) slot[j] = k;
    }
}

}  // namespace dagr
