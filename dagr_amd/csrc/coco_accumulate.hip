// coco_accumulate.hip -- the precision accumulation of the COCO-protocol evaluation (utils/coco_eval.py:_accumulate,
// the part after the sort) for every (class, area range) group and every IoU threshold in one call.
//
// Two launches.  k_coco_acc_gather reads the matcher's dtm / dt_ign through `perm` -- the random gather, one thread per
// visited column, all thresholds -- and leaves one byte per (threshold, visited position) in the workspace: bit 0 = counted
// true positive (dtm & ~dt_ign), bit 1 = counted false positive (~dtm & ~dt_ign).  It also checks `perm` and `group_ptr`
// and raises *status; k_coco_accumulate does nothing once the status is raised, so a bad argument leaves `precision` as
// it was.  k_coco_accumulate: one workgroup per (group, threshold) walks the group's segment of those bytes in tiles of
// DAGR_COCO_ACC_TILE with the cumulative (tp, fp) carried from tile to tile as exact integers.
//
// The host walks the precision backwards (the envelope = suffix maximum) and then looks the recall points up.  Only the
// envelope AT the crossing index of a recall point is ever read, and a maximum does not depend on the order it is taken
// in, so one forward walk is enough: a recall point that crosses in this tile starts from the tile's own suffix maximum
// at its index, one that crossed earlier takes the maximum with the whole tile.  Every float64 value is made by the
// host's operations on the host's operands -- tp / n_gt, tp / ((fp + tp) + eps), both IEEE divisions of exactly
// converted integers (this library is built with -ffp-contract=off) -- so the output is the host's, bit for bit.
#include "common.hpp"

namespace dagr {
namespace {

constexpr int kAccBlock = 256;
constexpr int kAccItems = 4;                        // consecutive positions of a thread
constexpr int kAccTile = DAGR_COCO_ACC_TILE;
constexpr int kAccWaves = kAccBlock / kWave;
constexpr int kAccMaxRec = DAGR_COCO_ACC_MAX_REC;   // one thread per recall point
constexpr int kAccMaxThr = 16;
static_assert(kAccTile == kAccBlock * kAccItems && kAccMaxRec <= kAccBlock, "tile = block x items; a thread per recall point");

__device__ __forceinline__ double max_f64(double a, double b) { return a > b ? a : b; }

__global__ __launch_bounds__(kAccBlock) void k_coco_acc_gather(
    const uint8_t *__restrict__ dtm, const uint8_t *__restrict__ dt_ign, const int32_t *__restrict__ perm,
    const int64_t *__restrict__ group_ptr, int n_thr, int n_groups, int64_t n_cols, uint8_t *__restrict__ codes,
    int32_t *__restrict__ status) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t g = first; g < n_groups; g += stride) {
        const int64_t lo = group_ptr[g], hi = group_ptr[g + 1];
        // monotone with both ends inside [0, n_cols]: every segment lies inside the arrays
        if (lo > hi || (g == 0 && lo < 0) || (g == n_groups - 1 && hi > n_cols)) *status = 1;
    }
    for (int64_t k = first; k < n_cols; k += stride) {
        const int64_t c = perm[k];
        const bool ok = c >= 0 && c < n_cols;
        if (!ok) *status = 1;
        for (int t = 0; t < n_thr; t++) {
            uint8_t code = 0;
            if (ok) {
                const bool m = dtm[(int64_t)t * n_cols + c] != 0, ign = dt_ign[(int64_t)t * n_cols + c] != 0;
                code = ign ? 0 : (m ? 1 : 2);
            }
            codes[(int64_t)t * n_cols + k] = code;
        }
    }
}

// grid = n_groups * n_thr workgroups: block b is group b % n_groups at threshold b / n_groups
__global__ __launch_bounds__(kAccBlock) void k_coco_accumulate(
    const uint8_t *__restrict__ codes, const int64_t *__restrict__ group_ptr, const int64_t *__restrict__ group_ngt,
    const double *__restrict__ rec_thrs, int n_rec, int n_groups, int64_t n_cols, double eps, double *__restrict__ precision,
    const int32_t *__restrict__ status) {
    __shared__ uint32_t s_tp[kAccTile];           // cumulative true positives at every position of the tile
    __shared__ double s_env[kAccTile];            // max of the precision from that position to the end of the tile
    __shared__ uint64_t s_wave_sum[kAccWaves];
    __shared__ double s_wave_max[kAccWaves];

    if (*status != 0) return;                     // the same for every thread of the grid: raised by the launch before
    const int g = blockIdx.x % n_groups, t = blockIdx.x / n_groups;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t begin = group_ptr[g], end = group_ptr[g + 1], ngt = group_ngt[g];
    double *out = precision + (int64_t)t * n_rec * n_groups + g;       // [n_thr, n_rec, n_groups]
    if (ngt <= 0) {
        if (tid < n_rec) out[(int64_t)tid * n_groups] = -1.0;
        return;
    }
    const double n_gt = (double)ngt;
    const double thr = tid < n_rec ? rec_thrs[tid] : 0.0;
    const uint8_t *row = codes + (int64_t)t * n_cols;
    bool crossed = false;                         // tp / n_gt has reached this thread's recall point
    double best = 0.0;                            // ... and the largest precision from there on
    uint64_t carry = 0;                           // tp | fp << 32 before the tile; each < 2^31 (perm is int32)

    for (int64_t base = begin; base < end; base += kAccTile) {
        const int n = (int)(end - base < kAccTile ? end - base : kAccTile);
        uint64_t local[kAccItems], run = 0;
#pragma unroll
        for (int i = 0; i < kAccItems; i++) {
            const int k = tid * kAccItems + i;
            const uint32_t code = k < n ? row[base + k] : 0u;
            run += (uint64_t)(code & 1u) | ((uint64_t)((code >> 1) & 1u) << 32);
            local[i] = run;
        }
        uint64_t incl = run;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint64_t o = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += o;
        }
        if (lane == kWave - 1) s_wave_sum[wave] = incl;
        __syncthreads();
        uint64_t before = carry + incl - run, total = 0;
#pragma unroll
        for (int w = 0; w < kAccWaves; w++) {
            if (w < wave) before += s_wave_sum[w];
            total += s_wave_sum[w];
        }
        // precision at the thread's positions, then its maximum from each of them to the thread's last one
        double p[kAccItems];
#pragma unroll
        for (int i = 0; i < kAccItems; i++) {
            const int k = tid * kAccItems + i;
            const uint64_t c = before + local[i];
            const uint32_t tp = (uint32_t)c, fp = (uint32_t)(c >> 32);
            const double tpd = (double)tp;
            p[i] = k < n ? tpd / (((double)fp + tpd) + eps) : -1.0;         // past the end: below every precision
            if (k < n) s_tp[k] = tp;
        }
#pragma unroll
        for (int i = kAccItems - 2; i >= 0; i--) p[i] = max_f64(p[i], p[i + 1]);
        double sfx = p[0];                                                  // max over this and the later lanes
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const double o = __shfl_down(sfx, d, kWave);
            if (lane + d < kWave) sfx = max_f64(sfx, o);
        }
        if (lane == 0) s_wave_max[wave] = sfx;
        double later = __shfl_down(sfx, 1, kWave);                          // max over the later lanes of the wave
        if (lane == kWave - 1) later = -1.0;
        __syncthreads();
#pragma unroll
        for (int w = 1; w < kAccWaves; w++)
            if (w > wave) later = max_f64(later, s_wave_max[w]);
#pragma unroll
        for (int i = 0; i < kAccItems; i++) {
            const int k = tid * kAccItems + i;
            if (k < n) s_env[k] = max_f64(p[i], later);
        }
        __syncthreads();
        if (tid < n_rec) {
            if (crossed) {
                best = max_f64(best, s_env[0]);
            } else if ((double)s_tp[n - 1] / n_gt >= thr) {
                // searchsorted(rc, thr, side="left") on the non-decreasing rc = tp / n_gt: the first position with rc >= thr
                int lo = 0, hi = n - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if ((double)s_tp[mid] / n_gt >= thr) hi = mid; else lo = mid + 1;
                }
                best = s_env[lo];
                crossed = true;
            }
        }
        carry += total;
        __syncthreads();                          // the next tile rewrites s_tp / s_env / s_wave_*
    }
    if (tid < n_rec) out[(int64_t)tid * n_groups] = crossed ? best : 0.0;
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" int32_t dagr_coco_accumulate_tile(void) { return kAccTile; }

extern "C" size_t dagr_coco_accumulate_workspace_bytes(int32_t n_thr, int64_t n_cols) {
    if (n_thr < 1 || n_thr > kAccMaxThr || n_cols < 0 || n_cols > 0x7fffffff) {
        set_error("dagr_coco_accumulate_workspace_bytes: bad size");
        return 0;
    }
    return align_up((size_t)n_thr * (size_t)n_cols, 256) + 256;
}

extern "C" int dagr_coco_accumulate(const uint8_t *dtm, const uint8_t *dt_ign, const int32_t *perm, const int64_t *group_ptr,
                                    const int64_t *group_ngt, const double *rec_thrs, int32_t n_rec, double eps, int32_t n_thr,
                                    int32_t n_groups, int64_t n_cols, void *workspace, size_t workspace_bytes,
                                    double *precision, int32_t *status, void *stream) {
    DAGR_CHECK_ARG(n_cols >= 0 && n_cols <= 0x7fffffff && n_groups >= 0 && n_groups <= (1 << 20), "bad sizes");
    DAGR_CHECK_ARG(n_thr >= 1 && n_thr <= kAccMaxThr, "1 to 16 IoU thresholds");
    DAGR_CHECK_ARG(n_rec >= 1 && n_rec <= kAccMaxRec, "1 to DAGR_COCO_ACC_MAX_REC recall points (one thread each)");
    DAGR_CHECK_ARG(eps > 0.0, "eps must be positive: it keeps 0 / 0 out of the precision");
    DAGR_CHECK_ARG(status != nullptr, "NULL pointer");
    DAGR_CHECK_ARG(workspace_bytes >= dagr_coco_accumulate_workspace_bytes(n_thr, n_cols),
                   "workspace smaller than dagr_coco_accumulate_workspace_bytes");
    DAGR_CHECK_ARG(n_groups == 0 || (group_ptr && group_ngt && rec_thrs && precision && workspace), "NULL pointer");
    DAGR_CHECK_ARG(n_cols == 0 || (dtm && dt_ign && perm), "NULL pointer");
    DAGR_CHECK_ARG((((uintptr_t)group_ptr | (uintptr_t)group_ngt | (uintptr_t)rec_thrs | (uintptr_t)precision) & 7) == 0 &&
                       (((uintptr_t)perm | (uintptr_t)status) & 3) == 0,
                   "float64 / int64 arrays must be 8-byte aligned, int32 arrays 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    DAGR_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_groups == 0) return DAGR_OK;
    const int64_t items = n_cols > n_groups ? n_cols : n_groups;
    int64_t blocks = ceil_div(items, kAccBlock);
    if (blocks > 8 * (int64_t)device_cu_count()) blocks = 8 * (int64_t)device_cu_count();
    k_coco_acc_gather<<<(unsigned)blocks, kAccBlock, 0, s>>>(dtm, dt_ign, perm, group_ptr, n_thr, n_groups, n_cols,
                                                              (uint8_t *)workspace, status);
    DAGR_CHECK_LAUNCH();
    k_coco_accumulate<<<(unsigned)((int64_t)n_groups * n_thr), kAccBlock, 0, s>>>(
        (const uint8_t *)workspace, group_ptr, group_ngt, rec_thrs, n_rec, n_groups, n_cols, eps, precision, status);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
