// stream_labels.hip -- the event stream's label store (dagr_stream_labels_push, dagr_stream_labels_at): the labelled
// keyframes of every lane live in a ring in a caller-owned state, and the ground truth of a step is interpolated between the
// two keyframes that bracket the step's own reference instant, on the device, into the arrays dagr_stream_score reads.
// dagr_amd/streaming.py: LabelDefinition is the same in numpy, bit for bit; include/dagr_hip.h states the rule and the
// state's layout.
//
// push: one workgroup per lane walks the call's keyframes in order; what is refused, cut or overwritten is decided from
//       the lane's words, which every thread holds in registers (uniform), so there is no atomic; row r of a keyframe is
//       always copied by thread r % 256, so two keyframes of one call that land in the same ring slot are written in order.
// at:   one workgroup of ONE wave per lane, as k_stream_score has it.  The bracketing pair is found by a uniform binary
//       search over the lane's resident instants.  A thread owns the rows `lane`, `lane + 64`, ... of the earlier keyframe
//       in registers (kGtRegs = 4); the ids of both keyframes and the later one's xywh are staged in LDS, 12 KB.
//   first:   every thread scans the earlier keyframe's ids for an earlier carrier of its identities (stream_eval.hpp's
//            mark_duplicates: one broadcast LDS read per id, four compares);
//   partner: the FIRST row of the later keyframe with the identity (find_columns' scan, first match instead of last);
//   value:   fp64, operation by operation what the definition does: r = double(t - t0) / double(t1 - t0), then
//            a * (1 - r) + b * r per coordinate -- this library is built with -ffp-contract=off, so no fma --, the small-box
//            filter with fp64 sqrt, and the box as fp32(x), fp32(y), fp32(x + w), fp32(y + h);
//   order:   the surviving rows' ids go back to the LDS (0: not surviving) and a row's output position is the number of
//            surviving ids below its own, from one more scan -- identities are unique among the survivors, so the
//            positions are 0 .. n_gt - 1 in ascending identity: no sort, no atomic, no second launch.
// Thread 0 writes n_gt and the lane's counter.
#include "stream_eval.hpp"

namespace dagr {
namespace {

namespace labels_word {     // a lane's int64 words, in the order include/dagr_hip.h documents
enum { kKeyframes = 0, kHead, kRefused, kCutRows, kOverwritten, kLabelled, kOutside, kGap, kCount };
}
static_assert(labels_word::kCount == DAGR_LABELS_WORDS, "the header's count of words");
using namespace labels_word;

constexpr int kPushBlock = 256;

struct Labels {
    int64_t *lane;      // [B, labels_word::kCount]
    int64_t *t;         // [B, K]
    int32_t *n;         // [B, K]
    double *xywh;       // [B, K, R, 4]
    int32_t *label;     // [B, K, R]
    int64_t *id;        // [B, K, R]
};

inline size_t carve_labels(int B, int K, int R, char *base, Labels *out) {
    const size_t bk = (size_t)B * K, rows = bk * R;
    size_t at = 0;
    const size_t o_lane = at;   at = align_up(at + 8 * (size_t)labels_word::kCount * B, 16);
    const size_t o_t = at;      at = align_up(at + 8 * bk, 16);
    const size_t o_n = at;      at = align_up(at + 4 * bk, 16);
    const size_t o_xywh = at;   at = align_up(at + 32 * rows, 16);
    const size_t o_label = at;  at = align_up(at + 4 * rows, 16);
    const size_t o_id = at;     at = align_up(at + 8 * rows, 16);
    if (out)
        *out = Labels{(int64_t *)(base + o_lane), (int64_t *)(base + o_t),         (int32_t *)(base + o_n),
                      (double *)(base + o_xywh),  (int32_t *)(base + o_label),     (int64_t *)(base + o_id)};
    return at;
}

inline bool labels_sizes_ok(int32_t B, int32_t K, int32_t R) {
    return B >= 1 && B <= 65535 && K >= 1 && K <= 65535 && R >= 1 && R <= kMaxGt;
}

__device__ __forceinline__ int ring_slot(int head, int i, int K) {
    const int s = head + i;
    return s >= K ? s - K : s;
}

// ---- push: the lane's keyframes of this call, in order
__global__ __launch_bounds__(kPushBlock) void k_stream_labels_push(Labels st, int K, int R, int F,
                                                                    const int64_t *__restrict__ t, const int32_t *__restrict__ n,
                                                                    const double *__restrict__ xywh,
                                                                    const int32_t *__restrict__ label,
                                                                    const int64_t *__restrict__ id) {
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t *words = st.lane + (int64_t)b * labels_word::kCount;
    int count = table_fill(words[kKeyframes], K);
    int head = table_fill(words[kHead], K - 1);
    int64_t refused = 0, cut = 0, over = 0;
    int64_t newest = count > 0 ? st.t[(int64_t)b * K + ring_slot(head, count - 1, K)] : 0;
    __syncthreads();            // every thread has read the words and the newest instant before thread 0 writes either
    for (int f = 0; f < F; f++) {
        const int64_t at = (int64_t)b * F + f;
        const int rows = n[at];
        if (rows < 0) continue;                                 // none for this lane
        const int64_t tf = t[at];
        if (count > 0 && tf <= newest) {
            refused++;
            continue;
        }
        const int kept = min(rows, R);
        cut += rows - kept;
        int slot;
        if (count == K) {                                       // a full ring: the oldest keyframe goes
            slot = head;
            head = head + 1 == K ? 0 : head + 1;
            over++;
        } else {
            slot = ring_slot(head, count, K);
            count++;
        }
        newest = tf;
        const int64_t dst = ((int64_t)b * K + slot) * R, src = at * R;
        for (int r = tid; r < kept; r += kPushBlock) {
            const double2 lo = *(const double2 *)(xywh + (src + r) * 4), hi = *(const double2 *)(xywh + (src + r) * 4 + 2);
            *(double2 *)(st.xywh + (dst + r) * 4) = lo;
            *(double2 *)(st.xywh + (dst + r) * 4 + 2) = hi;
            st.label[dst + r] = label[src + r];
            st.id[dst + r] = id[src + r];
        }
        if (tid == 0) {
            st.t[(int64_t)b * K + slot] = tf;
            st.n[(int64_t)b * K + slot] = kept;
        }
    }
    if (tid == 0) {
        words[kKeyframes] = count;
        words[kHead] = head;
        words[kRefused] += refused;
        words[kCutRows] += cut;
        words[kOverwritten] += over;
    }
}

// ---- at: the ground truth of every lane at its own t_ref
__global__ __launch_bounds__(kWave) void k_stream_labels_at(Labels st, int K, int R, const int64_t *__restrict__ t_ref,
                                                            int64_t max_gap, bool use_height, double min_height,
                                                            bool use_diag, double min_diag, float4 *__restrict__ gt_box,
                                                            int32_t *__restrict__ gt_label, int64_t *__restrict__ gt_id,
                                                            int32_t *__restrict__ n_gt) {
    __shared__ int64_t s_aid[kMaxGt];           // the earlier keyframe's ids; later the survivors' (0: not surviving)
    __shared__ int64_t s_bid[kMaxGt];           // the later keyframe's ids
    __shared__ __attribute__((aligned(16))) double s_bxywh[kMaxGt * 4];     // and its boxes

    const int b = blockIdx.x, lane = threadIdx.x;
    int64_t *words = st.lane + (int64_t)b * labels_word::kCount;
    const int64_t t = t_ref[b];
    const int count = table_fill(words[kKeyframes], K);
    const int head = table_fill(words[kHead], K - 1);
    const int64_t *lt = st.t + (int64_t)b * K;

    // ---- the bracketing pair, uniform: i0 is the last resident keyframe at or before t
    int why = kLabelled, i0 = 0;
    if (t == INT64_MIN || count == 0 || t < lt[ring_slot(head, 0, K)] || t > lt[ring_slot(head, count - 1, K)]) {
        why = kOutside;
    } else {
        int lo = 0, hi = count - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (lt[ring_slot(head, mid, K)] <= t) lo = mid; else hi = mid - 1;
        }
        i0 = lo;
    }
    const bool pair = why == kLabelled && i0 < count - 1;       // otherwise t is the newest keyframe's instant
    const int slot_a = ring_slot(head, i0, K), slot_b = ring_slot(head, pair ? i0 + 1 : i0, K);
    int64_t t0 = 0, t1 = 0;
    if (pair) {
        t0 = lt[slot_a], t1 = lt[slot_b];
        if (max_gap > 0 && t1 - t0 > max_gap) why = kGap;
    }
    if (why != kLabelled) {                     // no labels at this instant: the scorer skips the lane
        if (lane == 0) {
            n_gt[b] = -1;
            words[why] += 1;
        }
        return;
    }

    const int na = min(max(st.n[(int64_t)b * K + slot_a], 0), R);
    const int nb = pair ? min(max(st.n[(int64_t)b * K + slot_b], 0), R) : 0;
    const int64_t base_a = ((int64_t)b * K + slot_a) * R, base_b = ((int64_t)b * K + slot_b) * R;
    for (int g = lane; g < na; g += kWave) s_aid[g] = st.id[base_a + g];
    for (int g = lane; g < nb; g += kWave) {
        s_bid[g] = st.id[base_b + g];
        *(double2 *)(s_bxywh + 4 * g) = *(const double2 *)(st.xywh + (base_b + g) * 4);
        *(double2 *)(s_bxywh + 4 * g + 2) = *(const double2 *)(st.xywh + (base_b + g) * 4 + 2);
    }
    __syncthreads();

    // ---- a thread's rows of the earlier keyframe
    int64_t id[kGtRegs];
    double v[kGtRegs][4];
    int32_t lab[kGtRegs];
    bool ok[kGtRegs];
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        const int g = j * kWave + lane;
        id[j] = 0, lab[j] = 0;
        v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0.0;
        if (g < na) {
            const double2 lo = *(const double2 *)(st.xywh + (base_a + g) * 4), hi = *(const double2 *)(st.xywh + (base_a + g) * 4 + 2);
            id[j] = s_aid[g], lab[j] = st.label[base_a + g];
            v[j][0] = lo.x, v[j][1] = lo.y, v[j][2] = hi.x, v[j][3] = hi.y;
        }
        ok[j] = id[j] > 0;                      // only a positive identity takes part
    }
    // first: an identity counts at its first row
    for (int q = 0; q < na; q++) {
        const int64_t w = s_aid[q];
#pragma unroll
        for (int j = 0; j < kGtRegs; j++)
            if (q < j * kWave + lane && w == id[j]) ok[j] = false;
    }
    if (pair) {
        // partner: the first row of the later keyframe with the identity
        int col[kGtRegs];
#pragma unroll
        for (int j = 0; j < kGtRegs; j++) col[j] = -1;
        for (int c = 0; c < nb; c++) {
            const int64_t w = s_bid[c];
#pragma unroll
            for (int j = 0; j < kGtRegs; j++)
                if (col[j] < 0 && w == id[j]) col[j] = c;
        }
        // value: a * (1 - r) + b * r, two multiplies and one add
        const double r = (double)(t - t0) / (double)(t1 - t0);
        const double s = 1.0 - r;
#pragma unroll
        for (int j = 0; j < kGtRegs; j++) {
            ok[j] = ok[j] && col[j] >= 0;
            if (!ok[j]) continue;
#pragma unroll
            for (int k = 0; k < 4; k++) v[j][k] = v[j][k] * s + s_bxywh[4 * col[j] + k] * r;
        }
    }
    if (use_height || use_diag) {
#pragma unroll
        for (int j = 0; j < kGtRegs; j++) {
            const double w = v[j][2], h = v[j][3];
            if (use_diag && !(sqrt(h * h + w * w) > min_diag)) ok[j] = false;
            if (use_height && !(w > min_height && h > min_height)) ok[j] = false;
        }
    }

    // ---- order: the position of a surviving row is the number of surviving identities below its own
    __syncthreads();                            // (every scan of the earlier keyframe's ids is over)
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        const int g = j * kWave + lane;
        if (g < na) s_aid[g] = ok[j] ? id[j] : 0;
    }
    __syncthreads();
    int pos[kGtRegs];
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) pos[j] = 0;
    for (int q = 0; q < na; q++) {
        const int64_t w = s_aid[q];
#pragma unroll
        for (int j = 0; j < kGtRegs; j++)
            if (w > 0 && w < id[j]) pos[j]++;
    }
    int total = 0;
#pragma unroll
    for (int j = 0; j < kGtRegs; j++) {
        total += __popcll(__ballot(ok[j]));
        if (!ok[j]) continue;
        const int64_t at = (int64_t)b * R + pos[j];             // pos < the survivors <= na <= R
        gt_box[at] = make_float4((float)v[j][0], (float)v[j][1], (float)(v[j][0] + v[j][2]), (float)(v[j][1] + v[j][3]));
        gt_label[at] = lab[j];
        gt_id[at] = id[j];
    }
    if (lane == 0) {
        n_gt[b] = total;
        words[kLabelled] += 1;
    }
}

}  // namespace
}  // namespace dagr

using namespace dagr;

#define DAGR_LABELS_SIZES "stream labels: B (1 .. 65535), max_keyframes (1 .. 65535) or max_rows (1 .. DAGR_SCORE_MAX_GT) out of range"

extern "C" size_t dagr_stream_labels_bytes(int32_t B, int32_t max_keyframes, int32_t max_rows) {
    return labels_sizes_ok(B, max_keyframes, max_rows) ? carve_labels(B, max_keyframes, max_rows, nullptr, nullptr) : 0;
}

extern "C" int dagr_stream_labels_reset(void *state, size_t bytes, int32_t B, int32_t max_keyframes, int32_t max_rows,
                                        void *stream) {
    DAGR_CHECK_ARG(state != nullptr, "stream labels: state is NULL");
    DAGR_CHECK_ARG(labels_sizes_ok(B, max_keyframes, max_rows), DAGR_LABELS_SIZES);
    DAGR_CHECK_ARG(((uintptr_t)state & 15) == 0, "stream labels: state must be 16-byte aligned");
    DAGR_CHECK_ARG(bytes >= carve_labels(B, max_keyframes, max_rows, nullptr, nullptr),
                   "stream labels: state smaller than dagr_stream_labels_bytes");
    // the words alone: no keyframe is resident, so nothing behind them is ever read
    DAGR_CHECK_HIP(hipMemsetAsync(state, 0, 8 * (size_t)labels_word::kCount * B, (hipStream_t)stream));
    return DAGR_OK;
}

extern "C" int dagr_stream_labels_push(void *state, size_t bytes, int32_t B, int32_t max_keyframes, int32_t max_rows,
                                       int32_t F, const int64_t *t, const int32_t *n, const double *xywh,
                                       const int32_t *label, const int64_t *id, void *stream) {
    DAGR_CHECK_ARG(labels_sizes_ok(B, max_keyframes, max_rows), DAGR_LABELS_SIZES);
    DAGR_CHECK_ARG(F >= 1 && F <= 65535, "stream labels: F out of range (1 .. 65535 keyframes a lane and call)");
    DAGR_CHECK_ARG(state && t && n && xywh && label && id, "stream labels: NULL pointer");
    DAGR_CHECK_ARG((((uintptr_t)state | (uintptr_t)xywh) & 15) == 0 && (((uintptr_t)t | (uintptr_t)id) & 7) == 0 &&
                       (((uintptr_t)n | (uintptr_t)label) & 3) == 0,
                   "stream labels: state and xywh must be 16-byte aligned, int64 arrays 8-byte, int32 arrays 4-byte");
    Labels st;
    DAGR_CHECK_ARG(bytes >= carve_labels(B, max_keyframes, max_rows, (char *)state, &st),
                   "stream labels: state smaller than dagr_stream_labels_bytes");
    k_stream_labels_push<<<(unsigned)B, kPushBlock, 0, (hipStream_t)stream>>>(st, max_keyframes, max_rows, F, t, n, xywh, label,
                                                                             id);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

extern "C" int dagr_stream_labels_at(void *state, size_t bytes, int32_t B, int32_t max_keyframes, int32_t max_rows,
                                     const int64_t *t_ref, int64_t max_gap_us, double min_height, double min_diag,
                                     float *gt_box, int32_t *gt_label, int64_t *gt_id, int32_t *n_gt, void *stream) {
    DAGR_CHECK_ARG(labels_sizes_ok(B, max_keyframes, max_rows), DAGR_LABELS_SIZES);
    DAGR_CHECK_ARG(max_gap_us >= 0, "stream labels: max_gap_us must be >= 0 (0: no limit)");
    DAGR_CHECK_ARG(state && t_ref && gt_box && gt_label && gt_id && n_gt, "stream labels: NULL pointer");
    DAGR_CHECK_ARG((((uintptr_t)state | (uintptr_t)gt_box) & 15) == 0 && (((uintptr_t)t_ref | (uintptr_t)gt_id) & 7) == 0 &&
                       (((uintptr_t)gt_label | (uintptr_t)n_gt) & 3) == 0,
                   "stream labels: state and gt_box must be 16-byte aligned, int64 arrays 8-byte, int32 arrays 4-byte");
    Labels st;
    DAGR_CHECK_ARG(bytes >= carve_labels(B, max_keyframes, max_rows, (char *)state, &st),
                   "stream labels: state smaller than dagr_stream_labels_bytes");
    // a NaN bound: that half of the small-box filter is off
    k_stream_labels_at<<<(unsigned)B, kWave, 0, (hipStream_t)stream>>>(st, max_keyframes, max_rows, t_ref, max_gap_us,
                                                                       min_height == min_height, min_height,
                                                                       min_diag == min_diag, min_diag, (float4 *)gt_box,
                                                                       gt_label, gt_id, n_gt);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
