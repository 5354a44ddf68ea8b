// coco_match.hip -- the greedy matcher of the COCO-protocol evaluation (utils/coco_eval.py:_evaluate_image) for a flat
// list of (image, class, area range) jobs: one workgroup per job, one wave per IoU threshold.
//
// Every comparison of the host matcher is made on the same float64 values: the IoU is evaluated with the operations of
// _iou_xywh in their order (this library is built with -ffp-contract=off, so no FMA replaces a rounded product), the
// thresholds come from the host, and the serial "walk the ground truth, keep the last best" rule is restated as a wave
// reduction that picks the same index (largest IoU, the later index on a tie; a NaN IoU -- 0 / 0 of two empty boxes --
// makes the host loop take every later candidate, so the last unmatched box of the part wins).
#include "common.hpp"

namespace dagr {
namespace {

constexpr int kCocoMaxGt = DAGR_COCO_MAX_GT;        // ground-truth boxes of one job: kCocoMaxGt / 64 per lane
constexpr int kCocoMaxDt = DAGR_COCO_MAX_DT;        // detections of one job before the cut to max_dets
constexpr int kCocoMaxDets = DAGR_COCO_MAX_DETS;    // detections of one job that are matched
constexpr int kCocoMaxThr = 16;                     // waves of a workgroup
constexpr int kGtPerLane = kCocoMaxGt / kWave;
static_assert(kCocoMaxGt % kWave == 0 && kGtPerLane <= 32, "the matched flags of a lane's boxes are one 32-bit word");

struct Box {
    double x, y, w, h;
};

// numpy.minimum / numpy.maximum: a NaN operand comes back
__device__ __forceinline__ double np_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double np_max(double a, double b) { return (a > b || a != a) ? a : b; }

// _iou_xywh (maskApi bbIou, iscrowd = 0), operation by operation
__device__ __forceinline__ double iou_xywh(const Box &d, const Box &g) {
    const double w = np_min(d.x + d.w, g.x + g.w) - np_max(d.x, g.x);
    const double h = np_min(d.y + d.h, g.y + g.h) - np_max(d.y, g.y);
    const double inter = (w > 0.0 && h > 0.0) ? w * h : 0.0;
    const double uni = (d.w * d.h + g.w * g.h) - inter;
    return inter / uni;
}

__device__ __forceinline__ Box load_box(const double *p) { return Box{p[0], p[1], p[2], p[3]}; }

// whether detection k stands before detection i in argsort(-scores, kind="mergesort"): descending, NaN last, stable
__device__ __forceinline__ bool sorts_before(double sk, int k, double si, int i) {
    const bool nan_k = sk != sk, nan_i = si != si;
    if (nan_i) return !nan_k || k < i;
    return !nan_k && (sk > si || (sk == si && k < i));
}

// jobs[j] = {gt offset, gt count, dt offset, dt count, offset of the job's columns in order / dtm / dt_ign, offset of its
// entries in g_ign}.  A job whose numbers do not fit the arrays or the bounds writes nothing and raises *status.
__global__ __launch_bounds__(kCocoMaxThr * kWave) void k_coco_match(
    const double *__restrict__ gt, const double *__restrict__ dt, const double *__restrict__ score,
    const int64_t *__restrict__ jobs, const double *__restrict__ area_rng, const double *__restrict__ iou_thrs, int max_dets,
    int64_t n_gt, int64_t n_dt, int64_t n_out, int64_t n_gign, int32_t *__restrict__ order, uint8_t *__restrict__ dtm,
    uint8_t *__restrict__ dt_ign, uint8_t *__restrict__ g_ign, int32_t *__restrict__ status) {
    __shared__ Box s_gt[kCocoMaxGt];              // ground truth, evaluated boxes first
    __shared__ Box s_dt[kCocoMaxDets];            // detections by descending score
    __shared__ uint8_t s_ign_in[kCocoMaxGt];      // ignored flag by input index
    __shared__ uint8_t s_ign[kCocoMaxGt];         // ... in the order of s_gt
    __shared__ int s_n_eval;

    const int64_t *job = jobs + (int64_t)blockIdx.x * 6;
    const int64_t g_off = job[0], g_cnt = job[1], d_off = job[2], d_cnt = job[3], o_off = job[4], gi_off = job[5];
    const int64_t d_kept = d_cnt < max_dets ? d_cnt : max_dets;
    const bool fits = g_off >= 0 && g_cnt >= 0 && g_cnt <= kCocoMaxGt && g_off <= n_gt - g_cnt && d_off >= 0 && d_cnt >= 0 &&
                      d_cnt <= kCocoMaxDt && d_off <= n_dt - d_cnt && o_off >= 0 && o_off <= n_out - d_kept && gi_off >= 0 &&
                      gi_off <= n_gign - g_cnt;
    if (!fits) {                                  // the same for every thread of the workgroup
        if (threadIdx.x == 0) *status = 1;
        return;
    }
    const int G = (int)g_cnt, D = (int)d_cnt, Dk = (int)d_kept;
    const int tid = threadIdx.x, n_threads = blockDim.x;
    const double lo = area_rng[2 * (int64_t)blockIdx.x], hi = area_rng[2 * (int64_t)blockIdx.x + 1];

    // ---- ground truth: ignored outside the area range; argsort(g_ign, kind="mergesort") puts the evaluated boxes first
    for (int gi = tid; gi < G; gi += n_threads) {
        const Box b = load_box(gt + 4 * (g_off + gi));
        const double area = b.w * b.h;
        s_ign_in[gi] = (area < lo) | (area > hi);
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int k = 0; k < G; k++) n += !s_ign_in[k];
        s_n_eval = n;
    }
    for (int gi = tid; gi < G; gi += n_threads) {
        const int ign = s_ign_in[gi];
        int same_before = 0, n_eval = 0;
        for (int k = 0; k < G; k++) {
            n_eval += !s_ign_in[k];
            same_before += (k < gi) & (s_ign_in[k] == ign);
        }
        const int pos = ign ? n_eval + same_before : same_before;
        s_gt[pos] = load_box(gt + 4 * (g_off + gi));
        s_ign[pos] = (uint8_t)ign;
        g_ign[gi_off + pos] = (uint8_t)ign;
    }
    // ---- detections: rank of every score in the stable descending order; the first max_dets are matched
    for (int i = tid; i < D; i += n_threads) {
        const double si = score[d_off + i];
        int rank = 0;
        for (int k = 0; k < D; k++) rank += sorts_before(score[d_off + k], k, si, i);
        if (rank < Dk) {
            order[o_off + rank] = i;
            s_dt[rank] = load_box(dt + 4 * (d_off + i));
        }
    }
    __syncthreads();

    // ---- one wave per threshold walks the detections; lane l owns the boxes l, l + 64, ... of s_gt and their matched flags
    const int t = tid >> 6, lane = tid & 63;
    const double thr = iou_thrs[t];
    const double thr_eff = (1.0 - 1e-10) < thr ? (1.0 - 1e-10) : thr;          // min(thr, 1 - 1e-10)
    const int n_eval = s_n_eval;
    uint32_t matched = 0;
    for (int di = 0; di < Dk; di++) {
        const Box d = s_dt[di];
        int m = -1;
        // evaluated ground truth first; the ignored part only when nothing matched there (the loop's `break`)
        for (int part = 0; part < 2 && m < 0; part++) {
            const int first = part ? n_eval : 0, end = part ? G : n_eval;
            double best = thr_eff;
            int best_i = -1, last_open = -1, saw_nan = 0;
#pragma unroll
            for (int k = 0; k < kGtPerLane; k++) {
                const int gi = lane + k * kWave;
                if (gi < first || gi >= end || ((matched >> k) & 1u)) continue;
                const double v = iou_xywh(d, s_gt[gi]);
                last_open = gi;
                if (v != v) {
                    saw_nan = 1;
                } else if (!(v < best)) {            // `<` skips, so an equal IoU at a later index overwrites
                    best = v;
                    best_i = gi;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ov = __shfl_xor(best, off, kWave);
                const int oi = __shfl_xor(best_i, off, kWave);
                const int ol = __shfl_xor(last_open, off, kWave);
                if (oi >= 0 && (best_i < 0 || ov > best || (ov == best && oi > best_i))) {
                    best = ov;
                    best_i = oi;
                }
                last_open = ol > last_open ? ol : last_open;
            }
            m = __any(saw_nan) ? last_open : best_i;
        }
        if (m >= 0 && (m & 63) == lane) matched |= 1u << (m >> 6);
        if (lane == 0) {
            const double area = d.w * d.h;
            const int64_t at = (int64_t)t * n_out + o_off + di;
            dtm[at] = (uint8_t)(m >= 0);
            // matched: the ground truth's flag; unmatched: ignored when the detection lies outside the area range
            dt_ign[at] = m >= 0 ? s_ign[m] : (uint8_t)((area < lo) | (area > hi));
        }
    }
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" void dagr_coco_match_bounds(int32_t *max_gt, int32_t *max_dt, int32_t *max_dets) {
    if (max_gt) *max_gt = kCocoMaxGt;
    if (max_dt) *max_dt = kCocoMaxDt;
    if (max_dets) *max_dets = kCocoMaxDets;
}

extern "C" int dagr_coco_match(const double *gt_xywh, const double *dt_xywh, const double *dt_score, const int64_t *jobs,
                               const double *area_rng, const double *iou_thrs, int32_t n_thr, int32_t max_dets,
                               int64_t n_jobs, int64_t n_gt, int64_t n_dt, int32_t max_gt_per_job, int32_t max_dt_per_job,
                               int64_t n_out, int64_t n_gign, int32_t *order, uint8_t *dtm, uint8_t *dt_ign, uint8_t *g_ign,
                               int32_t *status, void *stream) {
    DAGR_CHECK_ARG(n_jobs >= 0 && n_jobs <= 0x7fffffff && n_gt >= 0 && n_dt >= 0 && n_out >= 0 && n_gign >= 0, "bad sizes");
    DAGR_CHECK_ARG(n_thr >= 1 && n_thr <= kCocoMaxThr, "1 to 16 IoU thresholds (one wave each)");
    DAGR_CHECK_ARG(max_dets >= 1 && max_dets <= kCocoMaxDets, "max_dets must be 1 .. DAGR_COCO_MAX_DETS");
    DAGR_CHECK_ARG(max_gt_per_job >= 0 && max_gt_per_job <= kCocoMaxGt,
                   "a job's ground truth does not fit the LDS tile (DAGR_COCO_MAX_GT boxes): match it on the host");
    DAGR_CHECK_ARG(max_dt_per_job >= 0 && max_dt_per_job <= kCocoMaxDt,
                   "a job has more than DAGR_COCO_MAX_DT detections: match it on the host");
    DAGR_CHECK_ARG(status != nullptr, "NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    DAGR_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_jobs == 0) return DAGR_OK;
    DAGR_CHECK_ARG(jobs && area_rng && iou_thrs, "NULL pointer");
    DAGR_CHECK_ARG((n_gt == 0 || gt_xywh) && (n_dt == 0 || (dt_xywh && dt_score)), "NULL pointer");
    DAGR_CHECK_ARG((n_out == 0 || (order && dtm && dt_ign)) && (n_gign == 0 || g_ign), "NULL pointer");
    DAGR_CHECK_ARG((((uintptr_t)gt_xywh | (uintptr_t)dt_xywh | (uintptr_t)dt_score | (uintptr_t)jobs | (uintptr_t)area_rng |
                     (uintptr_t)iou_thrs) & 7) == 0 && ((uintptr_t)order & 3) == 0 && ((uintptr_t)status & 3) == 0,
                   "float64 / int64 arrays must be 8-byte aligned, int32 arrays 4-byte aligned");
    k_coco_match<<<(unsigned)n_jobs, n_thr * kWave, 0, s>>>(gt_xywh, dt_xywh, dt_score, jobs, area_rng, iou_thrs, max_dets,
                                                            n_gt, n_dt, n_out, n_gign, order, dtm, dt_ign, g_ign, status);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
