// stream_map.hip -- detection mAP over every step of an event stream (dagr_stream_map_log, dagr_stream_map_plan): a
// fixed-capacity log of the evaluated images in a caller-owned state, and the COCO protocol's job list built from that log
// where it lies -- everything dagr_coco_match and dagr_coco_accumulate take, in utils/coco_eval.py:build_jobs' order.
// dagr_amd/streaming.py: MapDefinition is the log's rule in numpy, bit for bit; include/dagr_hip.h states the rule and the
// layouts.
//
// log:  one workgroup of ONE wave per lane.  What is logged, dropped or cut is decided from the lane's words and the
//       step's n_gt / n_keep, which every thread reads (uniform); the rows are copied as the 32-bit words they are; lane
//       0 of the wave writes the image's instant and counts and the lane's words last.  No atomic, one launch.
// plan: count, scan, scatter over the pairs p = class * (B * max_images) + lane * max_images + image -- the order of
//       build_jobs' (class, image) groups with the images lane-major, the slots that hold no image counting nothing:
//   count:   one wave per (slot, class) counts the class's ground-truth rows G and detections D: four ints a pair
//            (G, D, the pair exists, min(D, max_dets)), each in a segment of its own of ONE array;
//   scan:    ONE exclusive scan over the four segments on end (scan.hip); a segment's own prefix is the difference to its
//            first entry, a class's share the difference between the entries of its first pair and the next class's;
//   totals:  one workgroup: the seven totals and the largest G and D of a job;
//   scatter: one wave per (slot, class) compacts the class's rows in row order (ballot + popcount) behind the pair's
//            offsets and writes the pair's jobs, one an area range: job = areas * pairs before the class + range * pairs
//            of the class + rank inside the class, and likewise its first column and first g_ign entry.
// Every position is a prefix sum, so nothing depends on the order of execution.
#include "stream_eval.hpp"

namespace dagr {
namespace {

namespace map_word {        // a lane's int64 words, in the order include/dagr_hip.h documents
enum { kImages = 0, kDroppedImages, kCutDets, kUnlabelled, kEmpty, kCount };
}
static_assert(map_word::kCount == DAGR_MAP_WORDS, "the header's count of words");
using namespace map_word;

constexpr int kTotalsBlock = 1024;

struct MapLog {
    int64_t *lane;      // [B, map_word::kCount]
    int64_t *t;         // [B, I]
    int32_t *n_gt;      // [B, I]
    int32_t *n_dt;      // [B, I]
    float4 *gt_box;     // [B, I, G]
    int32_t *gt_label;  // [B, I, G]
    uint32_t *det;      // [B, I, D, 6]: fp32 rows as 32-bit words
};

inline size_t carve_map(int B, int I, int G, int D, char *base, MapLog *out) {
    const size_t bi = (size_t)B * I;
    size_t at = 0;
    const size_t o_lane = at;   at = align_up(at + 8 * (size_t)map_word::kCount * B, 16);
    const size_t o_t = at;      at = align_up(at + 8 * bi, 16);
    const size_t o_ngt = at;    at = align_up(at + 4 * bi, 16);
    const size_t o_ndt = at;    at = align_up(at + 4 * bi, 16);
    const size_t o_box = at;    at = align_up(at + 16 * bi * G, 16);
    const size_t o_label = at;  at = align_up(at + 4 * bi * G, 16);
    const size_t o_det = at;    at = align_up(at + 24 * bi * D, 16);
    if (out)
        *out = MapLog{(int64_t *)(base + o_lane), (int64_t *)(base + o_t),      (int32_t *)(base + o_ngt),
                      (int32_t *)(base + o_ndt),  (float4 *)(base + o_box),     (int32_t *)(base + o_label),
                      (uint32_t *)(base + o_det)};
    return at;
}

// every prefix sum of the plan is an int32: B * I * (G + 2 D + 256) stays below 2^31
inline bool map_sizes_ok(int32_t B, int32_t I, int32_t G, int32_t D) {
    if (!(B >= 1 && B <= 65535 && I >= 1 && I <= DAGR_MAP_MAX_IMAGES && G >= 1 && G <= DAGR_COCO_MAX_GT && D >= 1 &&
          D <= DAGR_COCO_MAX_DT))
        return false;
    return (int64_t)B * I * ((int64_t)G + 2 * (int64_t)D + DAGR_MAP_MAX_CLASSES) < 0x7fffffffll;
}

// ---- log: the lane's image of this step, if it has one
__global__ __launch_bounds__(kWave) void k_stream_map_log(MapLog st, int I, int G, int D, const uint32_t *__restrict__ det,
                                                          const int32_t *__restrict__ n_keep, int A,
                                                          const float4 *__restrict__ gt_box,
                                                          const int32_t *__restrict__ gt_label,
                                                          const int32_t *__restrict__ n_gt, const int64_t *__restrict__ t_ref) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int64_t *words = st.lane + (int64_t)b * map_word::kCount;
    const int rows = n_gt[b];
    if (rows <= 0) {                            // metrics only where there is a box
        if (lane == 0) words[rows < 0 ? kUnlabelled : kEmpty] += 1;
        return;
    }
    const int images = table_fill(words[kImages], I);
    if (images == I) {                          // a full log: the image is counted and nothing else is written
        if (lane == 0) words[kDroppedImages] += 1;
        return;
    }
    const int ng = min(rows, G);
    const int nk = min(max(n_keep[b], 0), A), kept = min(nk, D);
    const int64_t slot = (int64_t)b * I + images;
    for (int g = lane; g < ng; g += kWave) {
        st.gt_box[slot * G + g] = gt_box[(int64_t)b * G + g];
        st.gt_label[slot * G + g] = gt_label[(int64_t)b * G + g];
    }
    const uint32_t *src = det + (int64_t)b * A * 6;
    uint32_t *dst = st.det + slot * D * 6;
    for (int e = lane; e < kept * 6; e += kWave) dst[e] = src[e];
    if (lane == 0) {
        st.t[slot] = t_ref[b];
        st.n_gt[slot] = ng;
        st.n_dt[slot] = kept;
        words[kImages] = images + 1;
        words[kCutDets] += nk - kept;
    }
}

// ---- plan
struct MapPlan {
    int64_t NI, L;              // B * I slots; a segment's entries: classes * NI pairs and one behind them
    int32_t *cnt, *off;         // [4 L]: G, D, exists, min(D, max_dets) of every pair; their exclusive scan on end
};

// the class a detection row counts for is the one its label IS: c iff label == (float)c
__device__ __forceinline__ bool det_in_class(const uint32_t *row, int c) { return __uint_as_float(row[5]) == (float)c; }

__global__ __launch_bounds__(kWave) void k_stream_map_count(MapLog st, MapPlan pl, int I, int G, int D, int cut) {
    const int64_t s = blockIdx.x;
    const int c = blockIdx.y, lane = threadIdx.x;
    const int b = (int)(s / I), k = (int)(s % I);
    if (k >= table_fill(st.lane[(int64_t)b * map_word::kCount + kImages], I)) return;
    const int ng = min(max(st.n_gt[s], 0), G), nd = min(max(st.n_dt[s], 0), D);
    int g = 0, d = 0;
    for (int r0 = 0; r0 < ng; r0 += kWave) {
        const int r = r0 + lane;
        g += __popcll(__ballot(r < ng && st.gt_label[s * G + r] == c));
    }
    for (int r0 = 0; r0 < nd; r0 += kWave) {
        const int r = r0 + lane;
        d += __popcll(__ballot(r < nd && det_in_class(st.det + (s * D + r) * 6, c)));
    }
    if (lane == 0) {
        const int64_t p = (int64_t)c * pl.NI + s;
        pl.cnt[p] = g;
        pl.cnt[pl.L + p] = d;
        pl.cnt[2 * pl.L + p] = (g | d) ? 1 : 0;
        pl.cnt[3 * pl.L + p] = min(d, cut);
    }
}

__device__ __forceinline__ int64_t block_reduce(int64_t v, bool take_max, int64_t *smem) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t w = __shfl_xor(v, o, 64);
        v = take_max ? max(v, w) : v + w;
    }
    __syncthreads();            // (the round before has been read)
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
    __syncthreads();
    int64_t r = smem[0];
    for (int w = 1; w < kTotalsBlock / kWave; w++) r = take_max ? max(r, smem[w]) : r + smem[w];
    return r;
}

__global__ __launch_bounds__(kTotalsBlock) void k_stream_map_totals(MapLog st, MapPlan pl, int I, int n_areas,
                                                                    int64_t *__restrict__ totals) {
    __shared__ int64_t smem[kTotalsBlock / kWave];
    const int64_t pairs = pl.L - 1;
    int64_t mg = 0, md = 0, rows = 0;
    for (int64_t p = threadIdx.x; p < pairs; p += kTotalsBlock) {
        mg = max(mg, (int64_t)pl.cnt[p]);
        md = max(md, (int64_t)pl.cnt[pl.L + p]);
    }
    for (int64_t s = threadIdx.x; s < pl.NI; s += kTotalsBlock) {   // the detection rows the log holds, in a class or not
        const int b = (int)(s / I), k = (int)(s % I);
        if (k < table_fill(st.lane[(int64_t)b * map_word::kCount + kImages], I)) rows += max(st.n_dt[s], 0);
    }
    mg = block_reduce(mg, true, smem);
    md = block_reduce(md, true, smem);
    rows = block_reduce(rows, false, smem);
    if (threadIdx.x == 0) {
        const int64_t L = pl.L;
        const int64_t n_gt = pl.off[L], n_dt = pl.off[2 * L] - pl.off[L], n_pairs = pl.off[3 * L] - pl.off[2 * L];
        const int64_t n_kept = (int64_t)pl.off[3 * L + pairs] - pl.off[3 * L];
        totals[0] = n_areas * n_pairs;          // n_jobs
        totals[1] = n_gt;
        totals[2] = n_dt;
        totals[3] = n_areas * n_kept;           // n_out
        totals[4] = n_areas * n_gt;             // n_gign
        totals[5] = mg;
        totals[6] = md;
        totals[7] = rows;
    }
}

__global__ __launch_bounds__(kWave) void k_stream_map_scatter(MapLog st, MapPlan pl, int I, int G, int D, int n_classes,
                                                              const double *__restrict__ area_rngs, int n_areas,
                                                              double *__restrict__ gt_xywh, double *__restrict__ dt_xywh,
                                                              double *__restrict__ dt_score, int64_t *__restrict__ jobs,
                                                              double *__restrict__ area_rng, int64_t *__restrict__ job_info,
                                                              int64_t *__restrict__ col_group, int64_t *__restrict__ entry_group,
                                                              int64_t *__restrict__ group_ptr) {
    const int64_t s = blockIdx.x, L = pl.L;
    const int c = blockIdx.y, lane = threadIdx.x;
    const int64_t first = (int64_t)c * pl.NI, next = first + pl.NI, p = first + s;      // next <= L - 1
    const int32_t *oG = pl.off, *oD = pl.off + L, *oP = pl.off + 2 * L, *oK = pl.off + 3 * L;
    // the class's share of the pairs, columns and g_ign entries: what lies before it, and its own
    const int64_t p_before = oP[first] - oP[0], p_class = oP[next] - oP[first];
    const int64_t k_before = oK[first] - oK[0], k_class = oK[next] - oK[first];
    const int64_t g_before = oG[first], g_class = oG[next] - oG[first];
    if (s == 0) {                               // every class has this wave: the class's groups, with or without a job
        if (lane < n_areas) group_ptr[c * n_areas + lane] = n_areas * k_before + lane * k_class;
        if (lane == 0 && c == n_classes - 1) group_ptr[n_classes * n_areas] = n_areas * ((int64_t)oK[L - 1] - oK[0]);
    }
    if (pl.cnt[2 * L + p] == 0) return;         // no image in the slot, or none of its rows in the class
    const int gn = pl.cnt[p], dn = pl.cnt[L + p], kept = pl.cnt[3 * L + p];
    const int64_t g0 = oG[p], d0 = oD[p] - oD[0];
    const int ng = min(max(st.n_gt[s], 0), G), nd = min(max(st.n_dt[s], 0), D);
    const unsigned long long below = (1ull << lane) - 1ull;
    int at = 0;
    for (int r0 = 0; r0 < ng; r0 += kWave) {
        const int r = r0 + lane;
        const bool mine = r < ng && st.gt_label[s * G + r] == c;
        const unsigned long long m = __ballot(mine);
        if (mine) {                             // w = x2 - x1, h = y2 - y1 in fp32, then widened
            const float4 v = st.gt_box[s * G + r];
            double *o = gt_xywh + (g0 + at + __popcll(m & below)) * 4;
            o[0] = (double)v.x, o[1] = (double)v.y, o[2] = (double)(v.z - v.x), o[3] = (double)(v.w - v.y);
        }
        at += __popcll(m);
    }
    at = 0;
    for (int r0 = 0; r0 < nd; r0 += kWave) {
        const int r = r0 + lane;
        const uint32_t *row = st.det + (s * D + min(r, nd - 1)) * 6;
        const bool mine = r < nd && det_in_class(row, c);
        const unsigned long long m = __ballot(mine);
        if (mine) {
            const float x1 = __uint_as_float(row[0]), y1 = __uint_as_float(row[1]);
            const float x2 = __uint_as_float(row[2]), y2 = __uint_as_float(row[3]);
            const int64_t q = d0 + at + __popcll(m & below);
            double *o = dt_xywh + q * 4;
            o[0] = (double)x1, o[1] = (double)y1, o[2] = (double)(x2 - x1), o[3] = (double)(y2 - y1);
            dt_score[q] = (double)__uint_as_float(row[4]);
        }
        at += __popcll(m);
    }
    const int64_t rank = oP[p] - oP[first], k_rank = oK[p] - oK[first], g_rank = g0 - oG[first];
    for (int a = 0; a < n_areas; a++) {
        const int64_t j = n_areas * p_before + a * p_class + rank, group = (int64_t)c * n_areas + a;
        const int64_t col = n_areas * k_before + a * k_class + k_rank, entry = n_areas * g_before + a * g_class + g_rank;
        if (lane == 0) {
            int64_t *job = jobs + j * 6, *info = job_info + j * DAGR_MAP_JOB_WORDS;
            job[0] = g0, job[1] = gn, job[2] = d0, job[3] = dn, job[4] = col, job[5] = entry;
            info[0] = group, info[1] = kept, info[2] = col, info[3] = entry;
            area_rng[j * 2] = area_rngs[a * 2], area_rng[j * 2 + 1] = area_rngs[a * 2 + 1];
        }
        for (int i = lane; i < kept; i += kWave) col_group[col + i] = group;
        for (int i = lane; i < gn; i += kWave) entry_group[entry + i] = group;
    }
}

struct PlanCarve {
    size_t cnt, off, scratch, bytes;
    int64_t NI, L;
};

inline PlanCarve carve_plan(int B, int I, int n_classes) {
    PlanCarve c;
    c.NI = (int64_t)B * I;
    c.L = c.NI * n_classes + 1;
    size_t at = 0;
    c.cnt = at;      at = align_up(at + 16 * (size_t)c.L, 16);
    c.off = at;      at = align_up(at + 16 * (size_t)c.L, 16);
    c.scratch = at;  at = align_up(at + 4 * scan_scratch_elems(4 * c.L), 16);
    c.bytes = at;
    return c;
}

inline bool plan_sizes_ok(int32_t B, int32_t I, int32_t n_classes) {
    return B >= 1 && B <= 65535 && I >= 1 && I <= DAGR_MAP_MAX_IMAGES && n_classes >= 1 && n_classes <= DAGR_MAP_MAX_CLASSES &&
           (int64_t)B * I * n_classes < (1ll << 28);
}

}  // namespace
}  // namespace dagr

using namespace dagr;

#define DAGR_MAP_SIZES                                                                                                     \
    "stream map: B (1 .. 65535), max_images (1 .. DAGR_MAP_MAX_IMAGES), G (1 .. DAGR_COCO_MAX_GT) or max_dets (1 .. "       \
    "DAGR_COCO_MAX_DT) out of range, or B * max_images * (G + 2 * max_dets + 256) beyond 2^31"

extern "C" size_t dagr_stream_map_bytes(int32_t B, int32_t max_images, int32_t G, int32_t max_dets) {
    return map_sizes_ok(B, max_images, G, max_dets) ? carve_map(B, max_images, G, max_dets, nullptr, nullptr) : 0;
}

extern "C" int dagr_stream_map_reset(void *state, size_t bytes, int32_t B, int32_t max_images, int32_t G, int32_t max_dets,
                                     void *stream) {
    DAGR_CHECK_ARG(state != nullptr, "stream map: state is NULL");
    DAGR_CHECK_ARG(map_sizes_ok(B, max_images, G, max_dets), DAGR_MAP_SIZES);
    DAGR_CHECK_ARG(((uintptr_t)state & 15) == 0, "stream map: state must be 16-byte aligned");
    DAGR_CHECK_ARG(bytes >= carve_map(B, max_images, G, max_dets, nullptr, nullptr),
                   "stream map: state smaller than dagr_stream_map_bytes");
    // the words alone: no image is logged, so nothing behind them is ever read
    DAGR_CHECK_HIP(hipMemsetAsync(state, 0, 8 * (size_t)map_word::kCount * B, (hipStream_t)stream));
    return DAGR_OK;
}

extern "C" int dagr_stream_map_log(void *state, size_t bytes, int32_t B, int32_t max_images, int32_t G, int32_t max_dets,
                                   const float *det, const int32_t *n_keep, int32_t A, const float *gt_box,
                                   const int32_t *gt_label, const int32_t *n_gt, const int64_t *t_ref, void *stream) {
    DAGR_CHECK_ARG(map_sizes_ok(B, max_images, G, max_dets), DAGR_MAP_SIZES);
    DAGR_CHECK_ARG(A >= 1 && A <= DAGR_COCO_MAX_DT, "stream map: A out of range (1 .. DAGR_COCO_MAX_DT rows a lane)");
    DAGR_CHECK_ARG(state && det && n_keep && gt_box && gt_label && n_gt && t_ref, "stream map: NULL pointer");
    DAGR_CHECK_ARG((((uintptr_t)state | (uintptr_t)gt_box) & 15) == 0 && ((uintptr_t)t_ref & 7) == 0 &&
                       (((uintptr_t)det | (uintptr_t)n_keep | (uintptr_t)gt_label | (uintptr_t)n_gt) & 3) == 0,
                   "stream map: state and gt_box must be 16-byte aligned, t_ref 8-byte, fp32 and int32 arrays 4-byte");
    MapLog st;
    DAGR_CHECK_ARG(bytes >= carve_map(B, max_images, G, max_dets, (char *)state, &st),
                   "stream map: state smaller than dagr_stream_map_bytes");
    k_stream_map_log<<<(unsigned)B, kWave, 0, (hipStream_t)stream>>>(st, max_images, G, max_dets, (const uint32_t *)det, n_keep,
                                                                     A, (const float4 *)gt_box, gt_label, n_gt, t_ref);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

extern "C" size_t dagr_stream_map_plan_workspace_bytes(int32_t B, int32_t max_images, int32_t n_classes) {
    return plan_sizes_ok(B, max_images, n_classes) ? carve_plan(B, max_images, n_classes).bytes : 0;
}

extern "C" int dagr_stream_map_plan(const void *state, size_t bytes, int32_t B, int32_t max_images, int32_t G,
                                    int32_t max_dets, int32_t n_classes, const double *area_rngs, int32_t n_areas,
                                    int32_t max_dets_per_job, void *workspace, size_t workspace_bytes, double *gt_xywh,
                                    double *dt_xywh, double *dt_score, int64_t *jobs, double *area_rng, int64_t *job_info,
                                    int64_t *col_group, int64_t *entry_group, int64_t *group_ptr, int64_t *totals,
                                    void *stream) {
    DAGR_CHECK_ARG(map_sizes_ok(B, max_images, G, max_dets), DAGR_MAP_SIZES);
    DAGR_CHECK_ARG(plan_sizes_ok(B, max_images, n_classes),
                   "stream map: n_classes out of range (1 .. DAGR_MAP_MAX_CLASSES), or B * max_images * n_classes beyond 2^28");
    DAGR_CHECK_ARG(n_areas >= 1 && n_areas <= DAGR_MAP_MAX_AREAS, "stream map: n_areas out of range (1 .. DAGR_MAP_MAX_AREAS)");
    DAGR_CHECK_ARG(max_dets_per_job >= 1 && max_dets_per_job <= DAGR_COCO_MAX_DETS,
                   "stream map: max_dets_per_job must be 1 .. DAGR_COCO_MAX_DETS");
    DAGR_CHECK_ARG(state && area_rngs && workspace && gt_xywh && dt_xywh && dt_score && jobs && area_rng && job_info &&
                       col_group && entry_group && group_ptr && totals,
                   "stream map: NULL pointer");
    DAGR_CHECK_ARG((((uintptr_t)state | (uintptr_t)workspace) & 15) == 0 &&
                       (((uintptr_t)area_rngs | (uintptr_t)gt_xywh | (uintptr_t)dt_xywh | (uintptr_t)dt_score | (uintptr_t)jobs |
                         (uintptr_t)area_rng | (uintptr_t)job_info | (uintptr_t)col_group | (uintptr_t)entry_group |
                         (uintptr_t)group_ptr | (uintptr_t)totals) & 7) == 0,
                   "stream map: state and workspace must be 16-byte aligned, fp64 and int64 arrays 8-byte");
    MapLog st;
    DAGR_CHECK_ARG(bytes >= carve_map(B, max_images, G, max_dets, (char *)state, &st),
                   "stream map: state smaller than dagr_stream_map_bytes");
    const PlanCarve pc = carve_plan(B, max_images, n_classes);
    DAGR_CHECK_ARG(workspace_bytes >= pc.bytes, "stream map: workspace smaller than dagr_stream_map_plan_workspace_bytes");
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    MapPlan pl{pc.NI, pc.L, (int32_t *)(ws + pc.cnt), (int32_t *)(ws + pc.off)};
    const dim3 grid((unsigned)pc.NI, (unsigned)n_classes);
    DAGR_CHECK_HIP(hipMemsetAsync(pl.cnt, 0, 16 * (size_t)pc.L, s));
    k_stream_map_count<<<grid, kWave, 0, s>>>(st, pl, max_images, G, max_dets, max_dets_per_job);
    DAGR_CHECK_LAUNCH();
    DAGR_CHECK_HIP(exclusive_scan_i32(pl.cnt, pl.off, 4 * pc.L, (int32_t *)(ws + pc.scratch), false, s));
    k_stream_map_totals<<<1, kTotalsBlock, 0, s>>>(st, pl, max_images, n_areas, totals);
    DAGR_CHECK_LAUNCH();
    k_stream_map_scatter<<<grid, kWave, 0, s>>>(st, pl, max_images, G, max_dets, n_classes, area_rngs, n_areas, gt_xywh, dt_xywh,
                                                dt_score, jobs, area_rng, job_info, col_group, entry_group, group_ptr);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
