// stream_hota.hip -- the event stream's HOTA state (dagr_stream_hota, dagr_stream_hota_solve): behind the identity step
// (stream_identity.hip) on the same arrays, pass 1 of HOTA and the append of the labelled instant to the lane's log; on
// request the replay of the log with the final tables -- one maximum-weight assignment per logged instant (assign.hpp),
// the counts at the 19 thresholds -- and the fp64 sums behind AssA, AssRe and AssPr.  dagr_amd/streaming.py: HotaDefinition
// is the same in numpy, integer for integer; include/dagr_hip.h states the rule and the state's layout.
//
// The step: one workgroup of ONE wave per lane, as the scorer and the identity step have it; the lane's wave owns the
// lane's state, so there is no atomic.  Hypotheses, duplicates, columns (against the identity state's track table) and
// slots (against the scorer's id table) are stream_eval.hpp's stages, read only here, as are the layouts of those two
// states.  Its own: the participants get their place in the log by ballot + popcount, and the similarities are computed
// twice, once for the row sums (a shuffle reduction a row, kept in LDS) and the column sums (in registers), once for pmc:
// a hypothesis owns its column and a row its slot, so every word of pmc has one writer per row.
//
// The solve: a bounded grid of one-wave workgroups walks the logged instants of all lanes.  For an instant the wave stages
// the rows in LDS, keeps the columns in registers, writes the compacted weight matrix to its own part of the workspace,
// runs assign_wave on it and counts: a thread takes the rows `lane`, `lane + 64`, ..., adds its pairs to the mc tables
// with int32 atomics, the per-threshold counts are ballots and shuffle sums, and the threads 0 .. 18 add them to the
// lane's counters with int64 atomics (integer sums: the order does not matter).  The reduce: one workgroup of 256 threads
// per (threshold, lane); a thread adds its entries in index order, the 256 partial sums go through one fixed tree in LDS.
// Every float decision repeats the numpy definition operation by operation; this library is built with -ffp-contract=off,
// and the fp32 and fp64 divisions are correctly rounded.
#include <algorithm>

#include "assign.hpp"
#include "stream_eval.hpp"

namespace dagr {
namespace {

constexpr int kK = DAGR_HOTA_THRESHOLDS;
constexpr int kEntries = DAGR_HOTA_LOG_ENTRIES;     // of an instant: the rows at 0 .., the columns at kMaxGt ..
constexpr int kSolveWaves = DAGR_HOTA_SOLVE_WAVES;
constexpr int kLaneWords = 4;                       // int64 words of a lane
constexpr int kReduceBlock = 256;
static_assert(kMaxObjects <= kAssignMax, "one staging table for the track ids and the object ids");
static_assert(kEntries == kMaxGt + kMaxHyp, "an instant's rows and columns");
static_assert(kMaxGt <= kAssignMax && kMaxHyp <= kAssignMax, "an instant fits assign_wave");
static_assert(kK <= kWave, "one thread a threshold");

// the lane's words, in the order include/dagr_hip.h documents
enum { kInstants = 0, kDropped, kRows, kColumns };

struct Hota {
    int64_t *pmc;                       // [B, M, T]
    int64_t *gc, *tc;                   // [B, M], [B, T]
    int64_t *lane;                      // [B, kLaneWords]
    int64_t *count;                     // [B, kK, 4]: tp, fn, fp, loc_q
    double *sums;                       // [B, kK, 3]: ass, re, pr
    float4 *log_box;                    // [B, I, kEntries]
    int32_t *log_n;                     // [B, I, 2]
    int32_t *log_index, *log_label;     // [B, I, kEntries]
    int32_t *mc;                        // [B, kK, M, T]
};

size_t carve_hota(int B, int M, int T, int I, char *base, Hota *out) {
    const size_t nb = (size_t)B, mt = nb * M * T, log = nb * I * kEntries;
    const size_t sizes[11] = {8 * mt, 8 * nb * M, 8 * nb * T, 8 * nb * kLaneWords, 8 * nb * kK * 4, 8 * nb * kK * 3,
                              16 * log,  8 * nb * I, 4 * log, 4 * log, 4 * kK * mt};
    size_t at[12];
    at[0] = 0;
    for (int k = 0; k < 11; k++) at[k + 1] = at[k] + align_up(sizes[k], 16);
    if (out)
        *out = Hota{(int64_t *)(base + at[0]), (int64_t *)(base + at[1]), (int64_t *)(base + at[2]), (int64_t *)(base + at[3]),
                    (int64_t *)(base + at[4]), (double *)(base + at[5]), (float4 *)(base + at[6]), (int32_t *)(base + at[7]),
                    (int32_t *)(base + at[8]), (int32_t *)(base + at[9]), (int32_t *)(base + at[10])};
    return at[11];
}

bool hota_sizes_ok(int32_t B, int32_t M, int32_t T, int32_t I) {
    return B >= 1 && B <= 65535 && M >= 1 && M <= kMaxObjects && T >= 1 && T <= kAssignMax && I >= 1 &&
           I <= DAGR_HOTA_MAX_INSTANTS;
}

int solve_waves(int B, int I) { return (int)std::min((int64_t)B * I, (int64_t)kSolveWaves); }
// a wave's part of the workspace: the weight matrix and the transposed copy
size_t wave_words(int M, int T) { return 2 * (size_t)std::min(M, kMaxGt) * std::min(T, kMaxHyp); }
size_t hota_workspace_bytes(int B, int M, int T, int I) { return align_up(4 * (size_t)solve_waves(B, I) * wave_words(M, T), 16); }

// the similarity in units of 2^-20: 0 for a NaN IoU and for one outside (0, 1]
__device__ __forceinline__ int32_t similarity(const float4 &a, const float4 &b) {
    const float v = iou_xyxy(a, b);
    return (v > 0.0f && v <= 1.0f) ? (int32_t)rintf(v * kIouOne) : 0;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(kWave) void k_stream_hota(int M, int T, int I, const int64_t *__restrict__ score_id,
                                                       const int64_t *__restrict__ score_words,
                                                       const int64_t *__restrict__ ident_track,
                                                       const int64_t *__restrict__ ident_words,
                                                       const float *__restrict__ det, const int32_t *__restrict__ n_keep,
                                                       int A, const int64_t *__restrict__ track_id,
                                                       const float4 *__restrict__ track_box,
                                                       const float4 *__restrict__ gt_box, const int32_t *__restrict__ gt_label,
                                                       const int64_t *__restrict__ gt_id, const int32_t *__restrict__ n_gt,
                                                       int G, const int64_t *__restrict__ gt_match, Hota st) {
    __shared__ float4 s_hbox[kMaxHyp];          // the hypotheses, in row order (stage_hypotheses)
    __shared__ int64_t s_hid[kMaxHyp];
    __shared__ int32_t s_hlabel[kMaxHyp];
    __shared__ float4 s_gbox[kMaxGt];           // the ground-truth rows
    __shared__ int32_t s_glabel[kMaxGt];
    __shared__ int32_t s_gslot[kMaxGt];         // the slot of a participating row
    __shared__ int32_t s_rs[kMaxGt];            // its row sum (at most 256 * 2^20)
    __shared__ int64_t s_table[kAssignMax];     // the identity state's track ids, then the scorer's object ids

    const int b = blockIdx.x, lane = threadIdx.x;
    const int labelled = n_gt[b];
    if (labelled < 0) return;                   // no labels at this instant: not one byte of the lane changes
    int64_t *words = st.lane + (int64_t)b * kLaneWords;
    const int64_t at = words[kInstants];
    if (at < 0 || at >= I) {                    // a full log (or a state that was never reset): only the count of what is left out
        if (lane == 0) words[kDropped] += 1;
        return;
    }
    const int ng = min(labelled, G);
    const int n = min(max(n_keep[b], 0), A);
    const int n_tr = table_fill(ident_words[(int64_t)b * identity_word::kCount + identity_word::kNTracks], T);
    const int n_obj = table_fill(score_words[(int64_t)b * score_word::kCount + score_word::kNObjects], M);

    const int P = min(stage_hypotheses(b, lane, n, A, det, track_id, track_box, s_hbox, s_hid, s_hlabel), kMaxHyp);
    int64_t gid[kGtRegs];
    bool scored[kGtRegs];
    stage_scored_rows(b, lane, ng, G, gt_box, gt_label, gt_id, gt_match, s_gbox, s_glabel, gid, scored);
    for (int k = lane; k < n_tr; k += kWave) s_table[k] = ident_track[(int64_t)b * T + k];
    __syncthreads();

    float4 hbox[kHypRegs];
    int32_t hlabel[kHypRegs];
    int64_t hid[kHypRegs];                      // 0: no hypothesis in this register
    int col[kHypRegs];
    bool dup[kHypRegs];
    load_hypotheses(lane, P, s_hbox, s_hid, s_hlabel, hbox, hlabel, hid);
    mark_duplicates(lane, P, s_hid, hid, dup);
    // ---- columns: by id in the identity state's table, which its step has just brought up to date; without one: no part
    find_columns(n_tr, s_table, hid, col);
    int64_t *lane_tc = st.tc + (int64_t)b * T;
    const int64_t entry = ((int64_t)b * I + at) * kEntries;
    int n_cols = 0;
#pragma unroll
    for (int k = 0; k < kHypRegs; k++) {
        if (hid[k] == 0 || dup[k]) col[k] = -1;
        const uint64_t mask = __ballot(col[k] >= 0);
        if (col[k] >= 0) {
            const int64_t to = entry + kMaxGt + n_cols + lanes_below(mask, lane);
            st.log_box[to] = hbox[k];
            st.log_index[to] = col[k];
            st.log_label[to] = hlabel[k];
            lane_tc[col[k]] += 1;                                              // (distinct ids: one writer a column)
        }
        n_cols += __popcll(mask);
    }
    __syncthreads();                            // (every thread is done with the track ids in s_table)

    // ---- rows: the rows the scorer scored, at the slot of their identity in the scorer's table
    for (int k = lane; k < n_obj; k += kWave) s_table[k] = score_id[(int64_t)b * M + k];
    __syncthreads();
    int slot[kGtRegs];
    find_slots(n_obj, s_table, gid, scored, slot);
    uint64_t counted[kGtRegs];
    int n_rows = 0;
    int64_t *lane_gc = st.gc + (int64_t)b * M;
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        const int g = j * kWave + lane;
        counted[j] = __ballot(slot[j] >= 0);
        if (slot[j] >= 0) {
            const int64_t to = entry + n_rows + lanes_below(counted[j], lane);
            st.log_box[to] = s_gbox[g];
            st.log_index[to] = slot[j];
            st.log_label[to] = s_glabel[g];
            lane_gc[slot[j]] += 1;                                             // (scored rows have distinct identities)
        }
        if (g < ng) s_gslot[g] = slot[j];
        n_rows += __popcll(counted[j]);
    }
    __syncthreads();

    // ---- pass 1: the row sums and the column sums of the similarities, then the normalised similarities into pmc
    int32_t cs[kHypRegs];
#pragma unroll
    for (int k = 0; k < kHypRegs; k++) cs[k] = 0;
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        for (uint64_t m = counted[j]; m; m &= m - 1) {
            const int g = j * kWave + first_lane(m);
            const float4 d = s_gbox[g];
            const int32_t cls = s_glabel[g];
            int32_t sum = 0;
#pragma unroll
            for (int k = 0; k < kHypRegs; k++) {
                if (col[k] < 0 || hlabel[k] != cls) continue;
                const int32_t q = similarity(d, hbox[k]);
                cs[k] += q;
                sum += q;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, kWave);
            if (lane == 0) s_rs[g] = sum;
        }
    }
    __syncthreads();
    int64_t *lane_pmc = st.pmc + (int64_t)b * M * T;
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        for (uint64_t m = counted[j]; m; m &= m - 1) {
            const int g = j * kWave + first_lane(m);
            const float4 d = s_gbox[g];
            const int32_t cls = s_glabel[g];
            const int64_t rs = s_rs[g];
            int64_t *row = lane_pmc + (int64_t)s_gslot[g] * T;
#pragma unroll
            for (int k = 0; k < kHypRegs; k++) {
                if (col[k] < 0 || hlabel[k] != cls) continue;
                const int64_t q = similarity(d, hbox[k]);
                if (q > 0) row[col[k]] += (q << 20) / (rs + cs[k] - q);       // (rs, cs >= q > 0: the divisor is positive)
            }
        }
    }
    if (lane == 0) {
        st.log_n[((int64_t)b * I + at) * 2] = n_rows;
        st.log_n[((int64_t)b * I + at) * 2 + 1] = n_cols;
        words[kInstants] = at + 1;
        words[kRows] += n_rows;
        words[kColumns] += n_cols;
    }
}

__global__ __launch_bounds__(kWave) void k_stream_hota_solve(int B, int M, int T, int I, Hota st, int32_t *__restrict__ ws,
                                                             int ws_rows, int ws_cols) {
    __shared__ AssignLds s_assign;
    __shared__ float4 s_gbox[kMaxGt];           // the instant's rows
    __shared__ int32_t s_glabel[kMaxGt];
    __shared__ int32_t s_gslot[kMaxGt];
    __shared__ int64_t s_ggc[kMaxGt];           // gc of the row's slot
    __shared__ int32_t s_row_col[kMaxGt];       // the instant's pairing

    const int lane = threadIdx.x;
    int32_t *w = ws + (int64_t)blockIdx.x * 2 * ws_rows * ws_cols;             // [rows, columns], compacted
    int32_t *wt = w + (int64_t)ws_rows * ws_cols;                              // assign_wave's transposed copy
    for (int64_t idx = blockIdx.x; idx < (int64_t)B * I; idx += gridDim.x) {   // (every test below is uniform)
        const int b = (int)(idx / I), t = (int)(idx % I);
        if (t >= st.lane[(int64_t)b * kLaneWords + kInstants]) continue;
        // (the counts of a state that was never reset stay inside the workspace)
        const int n_r = clampi(st.log_n[idx * 2], 0, ws_rows), n_c = clampi(st.log_n[idx * 2 + 1], 0, ws_cols);
        const int64_t entry = idx * kEntries;
        const int64_t *lane_pmc = st.pmc + (int64_t)b * M * T;
        for (int r = lane; r < n_r; r += kWave) {
            const int s = clampi(st.log_index[entry + r], 0, M - 1);
            s_gbox[r] = st.log_box[entry + r];
            s_glabel[r] = st.log_label[entry + r];
            s_gslot[r] = s;
            s_ggc[r] = st.gc[(int64_t)b * M + s];
        }
        float4 hbox[kHypRegs];
        int32_t hlabel[kHypRegs];
        int hcol[kHypRegs];
        int64_t htc[kHypRegs];
#pragma unroll
        for (int k = 0; k < kHypRegs; k++) {
            const int i = k * kWave + lane;
            hbox[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hlabel[k] = 0, hcol[k] = 0, htc[k] = 0;
            if (i < n_c) {
                hbox[k] = st.log_box[entry + kMaxGt + i];
                hlabel[k] = st.log_label[entry + kMaxGt + i];
                hcol[k] = clampi(st.log_index[entry + kMaxGt + i], 0, T - 1);
                htc[k] = st.tc[(int64_t)b * T + hcol[k]];
            }
        }
        __syncthreads();

        // fill: w[g, i] = (gq[s, c] * q[g, i]) >> 10, in 0 .. 2^30
        for (int r = 0; r < n_r; r++) {
            const float4 d = s_gbox[r];
            const int32_t cls = s_glabel[r];
            const int64_t ggc = s_ggc[r];
            const int64_t *row = lane_pmc + (int64_t)s_gslot[r] * T;
#pragma unroll
            for (int k = 0; k < kHypRegs; k++) {
                const int i = k * kWave + lane;
                if (i >= n_c) continue;
                int64_t weight = 0;
                if (hlabel[k] == cls) {
                    const int64_t q = similarity(d, hbox[k]);
                    const int64_t pmc = q > 0 ? row[hcol[k]] : 0;
                    if (pmc > 0) {
                        const int64_t gq = (pmc << 20) / (((ggc + htc[k]) << 20) - pmc);
                        weight = (gq * q) >> 10;
                    }
                }
                w[r * n_c + i] = (int32_t)min(max(weight, (int64_t)0), (int64_t)1 << 30);
            }
        }
        __syncthreads();                        // w: written by this workgroup, read by all of it
        assign_wave(w, n_c, n_r, n_c, wt, s_row_col, s_assign);
        __syncthreads();

        // count: a thread the rows lane, lane + 64, ...; a pair is a TP at the thresholds k <= (20 * q) >> 20
        int kmax[kGtRegs];
        int32_t pq[kGtRegs];
#pragma unroll
        for (int j = 0; j < kGtRegs; j++) {
            const int r = j * kWave + lane;
            kmax[j] = 0, pq[j] = 0;
            const int i = r < n_r ? s_row_col[r] : -1;
            if (i < 0) continue;
            pq[j] = st.log_label[entry + kMaxGt + i] == s_glabel[r] ? similarity(s_gbox[r], st.log_box[entry + kMaxGt + i]) : 0;
            kmax[j] = min(kK, (int)((20 * (int64_t)pq[j]) >> 20));
            const int c = clampi(st.log_index[entry + kMaxGt + i], 0, T - 1);
            int32_t *pair = st.mc + ((int64_t)b * kK * M + s_gslot[r]) * T + c;
            for (int k = 0; k < kmax[j]; k++) atomicAdd(pair + (int64_t)k * M * T, 1);
        }
        int64_t my_tp = 0, my_loc = 0;          // of threshold lane + 1, in the threads 0 .. 18
        for (int k = 1; k <= kK; k++) {
            int tps = 0;
            int32_t loc = 0;                    // at most 256 * 2^20
#pragma unroll
            for (int j = 0; j < kGtRegs; j++) {
                tps += __popcll(__ballot(kmax[j] >= k));
                loc += kmax[j] >= k ? pq[j] : 0;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) loc += __shfl_xor(loc, off, kWave);
            if (lane == k - 1) my_tp = tps, my_loc = loc;
        }
        if (lane < kK) {
            unsigned long long *c = (unsigned long long *)(st.count + ((int64_t)b * kK + lane) * 4);
            atomicAdd(c + 0, (unsigned long long)my_tp);
            atomicAdd(c + 1, (unsigned long long)(n_r - my_tp));
            atomicAdd(c + 2, (unsigned long long)(n_c - my_tp));
            atomicAdd(c + 3, (unsigned long long)my_loc);
        }
        __syncthreads();                        // the staged rows and the pairing are read before the next instant overwrites them
    }
}

// ass, re and pr of one (threshold, lane): a thread's entries in index order, then one fixed tree over the 256 partial sums
__global__ __launch_bounds__(kReduceBlock) void k_stream_hota_reduce(int M, int T, Hota st) {
    __shared__ double s_sum[3][kReduceBlock];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int32_t *mc = st.mc + ((int64_t)b * kK + k) * M * T;
    const int64_t *gc = st.gc + (int64_t)b * M, *tc = st.tc + (int64_t)b * T;
    double ass = 0.0, re = 0.0, pr = 0.0;
    for (int64_t e = tid; e < (int64_t)M * T; e += kReduceBlock) {
        const int32_t m = mc[e];
        if (m <= 0) continue;
        const double dm = (double)m, g = (double)gc[e / T], t = (double)tc[e % T];
        ass += dm * (dm / (g + t - dm));
        re += dm * (dm / g);
        pr += dm * (dm / t);
    }
    s_sum[0][tid] = ass, s_sum[1][tid] = re, s_sum[2][tid] = pr;
    __syncthreads();
    for (int half = kReduceBlock / 2; half > 0; half >>= 1) {
        if (tid < half)
            for (int v = 0; v < 3; v++) s_sum[v][tid] += s_sum[v][tid + half];
        __syncthreads();
    }
    if (tid < 3) st.sums[((int64_t)b * kK + k) * 3 + tid] = s_sum[tid][0];
}

}  // namespace
}  // namespace dagr

using namespace dagr;

#define HOTA_SIZES_MSG                                                                                                     \
    "stream hota: B, max_objects (1 .. DAGR_SCORE_MAX_OBJECTS), max_tracks (1 .. DAGR_ASSIGN_MAX) or max_instants (1 .. " \
    "DAGR_HOTA_MAX_INSTANTS) out of range"

extern "C" size_t dagr_stream_hota_bytes(int32_t B, int32_t max_objects, int32_t max_tracks, int32_t max_instants) {
    return hota_sizes_ok(B, max_objects, max_tracks, max_instants)
               ? carve_hota(B, max_objects, max_tracks, max_instants, nullptr, nullptr)
               : 0;
}

extern "C" size_t dagr_stream_hota_workspace_bytes(int32_t B, int32_t max_objects, int32_t max_tracks, int32_t max_instants) {
    return hota_sizes_ok(B, max_objects, max_tracks, max_instants)
               ? hota_workspace_bytes(B, max_objects, max_tracks, max_instants)
               : 0;
}

extern "C" int dagr_stream_hota_reset(void *state, size_t bytes, int32_t B, int32_t max_objects, int32_t max_tracks,
                                      int32_t max_instants, void *stream) {
    DAGR_CHECK_ARG(state != nullptr, "stream hota: state is NULL");
    DAGR_CHECK_ARG(hota_sizes_ok(B, max_objects, max_tracks, max_instants), HOTA_SIZES_MSG);
    DAGR_CHECK_ARG(((uintptr_t)state & 15) == 0, "stream hota: state must be 16-byte aligned");
    const size_t need = carve_hota(B, max_objects, max_tracks, max_instants, nullptr, nullptr);
    DAGR_CHECK_ARG(bytes >= need, "stream hota: state smaller than dagr_stream_hota_bytes");
    DAGR_CHECK_HIP(hipMemsetAsync(state, 0, need, (hipStream_t)stream));
    return DAGR_OK;
}

extern "C" int dagr_stream_hota(void *state, size_t bytes, int32_t B, int32_t max_objects, int32_t max_tracks,
                                int32_t max_instants, const void *identity_state, size_t identity_bytes,
                                const void *score_state, size_t score_bytes, const float *det, const int32_t *n_keep, int32_t A,
                                const int64_t *track_id, const float *track_box, const float *gt_box, const int32_t *gt_label,
                                const int64_t *gt_id, const int32_t *n_gt, int32_t G, const int64_t *gt_match, void *stream) {
    DAGR_CHECK_ARG(hota_sizes_ok(B, max_objects, max_tracks, max_instants), HOTA_SIZES_MSG);
    DAGR_CHECK_ARG(A >= 0 && A <= (1 << 24), "stream hota: A out of range");
    DAGR_CHECK_ARG(G >= 0 && G <= kMaxGt, "stream hota: G out of range (0 .. DAGR_SCORE_MAX_GT)");
    DAGR_CHECK_ARG(state && identity_state && score_state && n_keep && n_gt, "stream hota: NULL pointer");
    DAGR_CHECK_ARG(A == 0 || (det && track_id), "stream hota: NULL detections or track ids");
    DAGR_CHECK_ARG(G == 0 || (gt_box && gt_label && gt_id && gt_match), "stream hota: NULL ground truth");
    DAGR_CHECK_ARG((((uintptr_t)state | (uintptr_t)identity_state | (uintptr_t)score_state | (uintptr_t)track_box |
                     (uintptr_t)gt_box) & 15) == 0 &&
                       (((uintptr_t)track_id | (uintptr_t)gt_id | (uintptr_t)gt_match) & 7) == 0 &&
                       (((uintptr_t)det | (uintptr_t)n_keep | (uintptr_t)gt_label | (uintptr_t)n_gt) & 3) == 0,
                   "stream hota: the states, track_box and gt_box must be 16-byte aligned, int64 arrays 8-byte, fp32 / int32 "
                   "arrays 4-byte");
    Hota st;
    DAGR_CHECK_ARG(bytes >= carve_hota(B, max_objects, max_tracks, max_instants, (char *)state, &st),
                   "stream hota: state smaller than dagr_stream_hota_bytes");
    DAGR_CHECK_ARG(identity_bytes >= dagr_stream_identity_bytes(B, max_objects, max_tracks),
                   "stream hota: identity_state smaller than dagr_stream_identity_bytes");
    DAGR_CHECK_ARG(score_bytes >= dagr_stream_score_bytes(B, max_objects),
                   "stream hota: score_state smaller than dagr_stream_score_bytes");
    Score score;                                // (both read only: the kernel takes their tables and words as const)
    Identity ident;
    carve_score(B, max_objects, (char *)score_state, &score);
    carve_identity(B, max_objects, max_tracks, (char *)identity_state, &ident);
    k_stream_hota<<<(unsigned)B, kWave, 0, (hipStream_t)stream>>>(max_objects, max_tracks, max_instants, score.id, score.lane,
                                                                  ident.track_id, ident.lane, det, n_keep, A, track_id,
                                                                  (const float4 *)track_box, (const float4 *)gt_box, gt_label,
                                                                  gt_id, n_gt, G, gt_match, st);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

extern "C" int dagr_stream_hota_solve(void *state, size_t bytes, int32_t B, int32_t max_objects, int32_t max_tracks,
                                      int32_t max_instants, void *workspace, size_t workspace_bytes, void *stream) {
    DAGR_CHECK_ARG(hota_sizes_ok(B, max_objects, max_tracks, max_instants), HOTA_SIZES_MSG);
    DAGR_CHECK_ARG(state && workspace, "stream hota: NULL pointer");
    DAGR_CHECK_ARG((((uintptr_t)state | (uintptr_t)workspace) & 15) == 0, "stream hota: state and workspace must be 16-byte aligned");
    Hota st;
    DAGR_CHECK_ARG(bytes >= carve_hota(B, max_objects, max_tracks, max_instants, (char *)state, &st),
                   "stream hota: state smaller than dagr_stream_hota_bytes");
    DAGR_CHECK_ARG(workspace_bytes >= hota_workspace_bytes(B, max_objects, max_tracks, max_instants),
                   "stream hota: workspace smaller than dagr_stream_hota_workspace_bytes");
    // what the solve fills: the counters and the sums (back to back in the state) and the mc tables
    DAGR_CHECK_HIP(hipMemsetAsync(st.count, 0, (char *)st.log_box - (char *)st.count, (hipStream_t)stream));
    DAGR_CHECK_HIP(hipMemsetAsync(st.mc, 0, 4 * (size_t)kK * B * max_objects * max_tracks, (hipStream_t)stream));
    k_stream_hota_solve<<<(unsigned)solve_waves(B, max_instants), kWave, 0, (hipStream_t)stream>>>(
        B, max_objects, max_tracks, max_instants, st, (int32_t *)workspace, std::min(max_objects, kMaxGt),
        std::min(max_tracks, kMaxHyp));
    DAGR_CHECK_LAUNCH();
    k_stream_hota_reduce<<<dim3(kK, (unsigned)B), kReduceBlock, 0, (hipStream_t)stream>>>(max_objects, max_tracks, st);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
