// augment.hip -- the training augmentations on a collated batch that is already on the device.
// Reference: src/dagr/data/augment.py -- RandomHFlip (:90-112), RandomCrop(p = 0.2) (:201-243), RandomZoom (:148-198),
// RandomTranslate (:246-279) and the final Crop([0, 0], [1, 1]) (:115-145), the chain of Augmentations.__init__ (:287-294).
// The random numbers are drawn on the host (dagr_amd/data/augment.py, DeviceAugmentations.draw: torch's global RNG, call for
// call as the host chain draws them); one dagr_aug_params record per sample reaches the kernels through device memory.
//
// Events: the chain is a per-event map (flip, window test, zoom, shift, sensor test) followed by a stable compaction.
//   1. k_aug_count: one workgroup per tile of kAugTile events evaluates the map and writes the tile's number of survivors.
//   2. k_aug_scatter: the same tile sums the counts of the tiles before it (a few hundred words for B = 8 x 50 k events:
//      a strided read and one block reduction, no third launch for a scan of so few values), re-evaluates the map, ranks
//      the survivors with the block scan of common.hpp round by round, and writes them -- event order is array order,
//      nothing is ordered by an atomic.  out_ptr[b] is the rank at position sample_ptr[b].
//   Those sums read tiles^2 / 2 words over the grid: beyond kAugSumTiles tiles (4 M events) the counts go through
//   exclusive_scan_i32 (scan.hip) between the two launches instead and the scatter reads its base from the result.
// Frames: one thread per output pixel walks the chain backwards to the one input pixel it shows (or black).
// The fp32 zoom is multiply-then-add in two roundings as torch computes it: this file relies on -ffp-contract=off.
#include "common.hpp"

namespace dagr {
namespace {

constexpr int kAugRounds = 8;
constexpr int kAugTile = kBlock * kAugRounds;      // events per workgroup
constexpr int kAugSumTiles = 2048;                 // up to here a scatter workgroup sums the earlier tiles' counts itself

enum : int32_t { kAugBadPtr = 1, kAugBadCoord = 2 };

// (x, y) of an event through the chain; false: the event is dropped.  Every step wraps to int16 as the host chain's
// int16 `pos` tensor does, so that coordinates far outside the sensor take the host chain's values too.
__device__ __forceinline__ bool aug_event(const dagr_aug_params &a, int W, int H, int &x, int &y) {
    if (a.flip) x = (int16_t)(W - 1 - x);
    if (a.crop_on && (x < a.crop_lo[0] || x > a.crop_hi[0] || y < a.crop_lo[1] || y > a.crop_hi[1])) return false;
    const float cx = (float)(W / 2), cy = (float)(H / 2);
    const float zx = ((float)x - cx) * a.zoom + cx;
    const float zy = ((float)y - cy) * a.zoom + cy;
    x = (int16_t)((int16_t)(int)zx + (int16_t)a.move[0]);
    y = (int16_t)((int16_t)(int)zy + (int16_t)a.move[1]);
    return x >= 0 && x < W && y >= 0 && y < H;
}

// sample_ptr must start at 0, end at N and never decrease; every thread of the block gets the verdict
__device__ __forceinline__ bool aug_ptr_ok(const int32_t *__restrict__ sample_ptr, int B, int N) {
    int bad = 0;
    for (int b = threadIdx.x; b <= B; b += kBlock) {
        const int s = sample_ptr[b];
        if (s < 0 || s > N || (b == 0 && s != 0) || (b == B && s != N) || (b > 0 && sample_ptr[b - 1] > s)) bad = 1;
    }
    return __syncthreads_or(bad) == 0;
}

// sample of event i: the largest b with sample_ptr[b] <= i (empty samples share their start with the next one)
__device__ __forceinline__ int aug_sample_of(const int32_t *__restrict__ sample_ptr, int B, int i) {
    int lo = 0, hi = B;                                   // invariant: sample_ptr[lo] <= i < sample_ptr[hi]
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (sample_ptr[m] <= i) lo = m; else hi = m;
    }
    return lo;
}

template <typename PosT>
__device__ __forceinline__ bool aug_load(const PosT *__restrict__ pos, int i, int &x, int &y, int32_t *status) {
    x = pos[2 * (int64_t)i];
    y = pos[2 * (int64_t)i + 1];
    if (sizeof(PosT) > 2 && (x < -32768 || x > 32767 || y < -32768 || y > 32767)) {
        if (status != nullptr) atomicOr(status, kAugBadCoord);
        return false;
    }
    return true;
}
template <>
__device__ __forceinline__ bool aug_load<int16_t>(const int16_t *__restrict__ pos, int i, int &x, int &y, int32_t *) {
    const int32_t w = reinterpret_cast<const int32_t *>(pos)[i];            // one 4-byte load per event
    x = (int16_t)(w & 0xffff);
    y = (int16_t)(w >> 16);
    return true;
}

template <typename PosT>
__global__ __launch_bounds__(kBlock) void k_aug_count(const dagr_aug_params *__restrict__ params, int B, int W, int H,
                                                     const PosT *__restrict__ pos, const int32_t *__restrict__ sample_ptr,
                                                     int N, int32_t *__restrict__ tile_count, int32_t *__restrict__ status) {
    __shared__ int smem[4];
    if (!aug_ptr_ok(sample_ptr, B, N)) {
        if (threadIdx.x == 0) {
            tile_count[blockIdx.x] = 0;
            if (blockIdx.x == 0) atomicOr(status, kAugBadPtr);
        }
        return;
    }
    const int base = blockIdx.x * kAugTile + threadIdx.x;
    int kept = 0;
#pragma unroll
    for (int r = 0; r < kAugRounds; r++) {
        const int i = base + r * kBlock;
        int x, y;
        if (i < N && aug_load(pos, i, x, y, status) && aug_event(params[aug_sample_of(sample_ptr, B, i)], W, H, x, y)) kept++;
    }
    int total;
    block_exclusive_scan(kept, smem, total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

__device__ __forceinline__ void aug_copy(void *dst, int64_t o, const void *src, int64_t i, int width) {
    switch (width) {
        case 1: ((uint8_t *)dst)[o] = ((const uint8_t *)src)[i]; break;
        case 2: ((uint16_t *)dst)[o] = ((const uint16_t *)src)[i]; break;
        case 4: ((uint32_t *)dst)[o] = ((const uint32_t *)src)[i]; break;
        default: ((uint64_t *)dst)[o] = ((const uint64_t *)src)[i]; break;
    }
}

template <typename PosT>
__global__ __launch_bounds__(kBlock) void k_aug_scatter(const dagr_aug_params *__restrict__ params, int B, int W, int H,
                                                       const PosT *__restrict__ pos, const void *__restrict__ t, int t_width,
                                                       const void *__restrict__ p, int p_width,
                                                       const int32_t *__restrict__ sample_ptr, int N,
                                                       const int32_t *__restrict__ tile_count, int scanned,
                                                       int16_t *__restrict__ out_pos, void *__restrict__ out_t,
                                                       void *__restrict__ out_p, int64_t *__restrict__ out_batch,
                                                       int32_t *__restrict__ out_ptr, const int32_t *__restrict__ status) {
    __shared__ int smem[4];
    __shared__ int rank_s[kAugTile];                      // rank, inside the tile, of every position of the tile
    const int tile = blockIdx.x, ntiles = gridDim.x;
    if (*status & kAugBadPtr) {                           // (written by k_aug_count, earlier on the stream)
        if (tile == 0)
            for (int b = threadIdx.x; b <= B; b += kBlock) out_ptr[b] = 0;
        return;
    }
    int tile_base;                                        // survivors in the tiles before this one
    if (scanned) {
        tile_base = tile_count[tile];                     // (tile_count already holds its exclusive prefix sums)
    } else {
        int before = 0;
        for (int k = threadIdx.x; k < tile; k += kBlock) before += tile_count[k];
        block_exclusive_scan(before, smem, tile_base);
    }
    const int first = tile * kAugTile;
    int carry = 0;
    int xy[kAugRounds], sample[kAugRounds], rank[kAugRounds];
#pragma unroll
    for (int r = 0; r < kAugRounds; r++) {
        const int i = first + r * kBlock + threadIdx.x;
        int x = 0, y = 0, flag = 0;
        sample[r] = 0;
        if (i < N && aug_load(pos, i, x, y, nullptr)) {   // (bad coordinates were reported by k_aug_count)
            sample[r] = aug_sample_of(sample_ptr, B, i);
            flag = aug_event(params[sample[r]], W, H, x, y) ? 1 : 0;
        }
        xy[r] = (x & 0xffff) | (y << 16);
        int total;
        const int ex = block_exclusive_scan(flag, smem, total) + carry;
        rank_s[r * kBlock + threadIdx.x] = ex;
        rank[r] = flag ? ex : -1;
        carry += total;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kAugRounds; r++) {
        const int i = first + r * kBlock + threadIdx.x;
        if (rank[r] < 0) continue;
        const int64_t o = (int64_t)tile_base + rank[r];   // < N: a rank counts surviving events before this one
        reinterpret_cast<int32_t *>(out_pos)[o] = xy[r];
        aug_copy(out_t, o, t, i, t_width);
        aug_copy(out_p, o, p, i, p_width);
        if (out_batch != nullptr) out_batch[o] = sample[r];
    }
    // segment bounds: position s of the array belongs to the tile that holds event s; s = N to the last tile
    const int end = min(first + kAugTile, N);
    for (int b = threadIdx.x; b <= B; b += kBlock) {
        const int s = sample_ptr[b];
        if (s >= first && s < end) out_ptr[b] = tile_base + rank_s[s - first];
        else if (s == N && tile == ntiles - 1) out_ptr[b] = tile_base + carry;
    }
}

// torch's `nearest` source index of a resize from n_in to n_out entries (UpSampleKernel.cpp, HelperInterpNearest)
__device__ __forceinline__ int aug_nearest(int dst, int n_in, int n_out) {
    const float scale = (float)n_in / (float)n_out;
    return min((int)floorf((float)dst * scale), n_in - 1);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_aug_frames(const dagr_aug_params *__restrict__ params, int C, int H, int W,
                                                      int reference_crop, const T *__restrict__ in, T *__restrict__ out) {
    const int64_t HW = (int64_t)H * W;
    const int64_t pix = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= HW) return;
    const int c = blockIdx.y, b = blockIdx.z;
    const dagr_aug_params a = params[b];
    const int64_t plane = ((int64_t)b * C + c) * HW;
    T v = (T)0;
    // RandomTranslate backwards: the pixel that was shifted here (black where the shift brought nothing)
    int x = (int)(pix % W) - a.move[0], y = (int)(pix / W) - a.move[1];
    if (x >= 0 && x < W && y >= 0 && y < H) {
        // RandomZoom backwards: position in the resized (ceil(H z), ceil(W z)) frame under the centre crop / centre pad
        // (augment.py:185-196: float64 products of the float32 factor), then the `nearest` source pixel
        const int w2 = (int)ceil((double)W * (double)a.zoom), h2 = (int)ceil((double)H * (double)a.zoom);
        const int dx = w2 - W, dy = h2 - H;
        x += dx >= 0 ? dx / 2 : -((1 - dx) / 2);          // (Python's floor division)
        y += dy >= 0 ? dy / 2 : -((1 - dy) / 2);
        if (x >= 0 && x < w2 && y >= 0 && y < h2) {
            x = aug_nearest(x, W, w2);
            y = aug_nearest(y, H, h2);
            bool blank = false;
            if (a.crop_on) {
                const int x0 = a.crop_lo[0], y0 = a.crop_lo[1], x1 = a.crop_hi[0], y1 = a.crop_hi[1];
                // reference (augment.py:51-58): the four slices index the batch (size 1) and channel dimensions of the
                // sample's [1, C, H, W] frame, not rows and columns
                blank = reference_crop ? (y0 > 0 || y1 <= 0 || c < x0 || c >= x1)
                                       : (y < y0 || y >= y1 || x < x0 || x >= x1);
            }
            if (!blank) v = in[plane + (int64_t)y * W + (a.flip ? W - 1 - x : x)];
        }
    }
    out[plane + pix] = v;
}

// Boxes (x, y, w, h in columns 0..3 of fp32 rows of `ld` columns; other columns untouched) through the same chain:
// augment.py:105-110 (flip), :59-66 (window clamp), :190-194 (zoom), :272-274 (shift), :133-143 (sensor clamp).
__global__ __launch_bounds__(kBlock) void k_aug_boxes(const dagr_aug_params *__restrict__ params, int B, int W, int H,
                                                     const float *__restrict__ in, const int64_t *__restrict__ box_batch,
                                                     int M, int ld, float *__restrict__ out) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= M) return;
    const float *src = in + (int64_t)j * ld;
    float *dst = out + (int64_t)j * ld;
    for (int k = 4; k < ld; k++) dst[k] = src[k];
    float x = src[0], y = src[1], w = src[2], h = src[3];
    const int64_t b = box_batch[j];
    if (b >= 0 && b < B) {
        const dagr_aug_params a = params[b];
        if (a.flip) x = (float)(W - 1) - (x + w);
        if (a.crop_on) {
            const float lx = (float)a.crop_lo[0], ly = (float)a.crop_lo[1], hx = (float)a.crop_hi[0], hy = (float)a.crop_hi[1];
            const float fx = fminf(fmaxf(x + w, lx), hx), fy = fminf(fmaxf(y + h, ly), hy);
            x = fminf(fmaxf(x, lx), hx);
            y = fminf(fmaxf(y, ly), hy);
            w = fx - x;
            h = fy - y;
        }
        const float cx = (float)(W / 2), cy = (float)(H / 2);
        w *= a.zoom;
        h *= a.zoom;
        x = (x - cx) * a.zoom + cx;
        y = (y - cy) * a.zoom + cy;
        x += (float)a.move[0];
        y += (float)a.move[1];
        const float xm = (float)(W - 1), ym = (float)(H - 1);
        const float fx = fminf(fmaxf(x + w, 0.0f), xm), fy = fminf(fmaxf(y + h, 0.0f), ym);
        x = fminf(fmaxf(x, 0.0f), xm);
        y = fminf(fmaxf(y, 0.0f), ym);
        w = fx - x;
        h = fy - y;
    }
    dst[0] = x; dst[1] = y; dst[2] = w; dst[3] = h;
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" size_t dagr_augment_workspace_bytes(int64_t N) {
    const int64_t tiles = ceil_div(N < 0 ? 0 : N, kAugTile);
    return align_up((size_t)(tiles + 1 + (tiles > kAugSumTiles ? (int64_t)scan_scratch_elems(tiles) : 0)) * sizeof(int32_t), 256);
}

namespace {
template <typename PosT>
int aug_events_launch(const dagr_aug_params *params, int B, int W, int H, const PosT *pos, const void *t, int t_width,
                      const void *p, int p_width, const int32_t *sample_ptr, int N, int16_t *out_pos, void *out_t,
                      void *out_p, int64_t *out_batch, int32_t *out_ptr, int32_t *status, int32_t *tile_count,
                      hipStream_t s) {
    const int64_t tiles = ceil_div(N, kAugTile);
    k_aug_count<PosT><<<(unsigned)tiles, kBlock, 0, s>>>(params, B, W, H, pos, sample_ptr, N, tile_count, status);
    DAGR_CHECK_LAUNCH();
    const bool scanned = tiles > kAugSumTiles;
    if (scanned) DAGR_CHECK_HIP(exclusive_scan_i32(tile_count, tile_count, tiles, tile_count + tiles + 1, false, s));
    k_aug_scatter<PosT><<<(unsigned)tiles, kBlock, 0, s>>>(params, B, W, H, pos, t, t_width, p, p_width, sample_ptr, N,
                                                           tile_count, scanned ? 1 : 0, out_pos, out_t, out_p, out_batch,
                                                           out_ptr, status);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
}  // namespace

extern "C" int dagr_augment_events(const dagr_aug_params *params, int32_t B, int32_t W, int32_t H, const void *pos,
                                   int32_t pos_width, const void *t, int32_t t_width, const void *p, int32_t p_width,
                                   const int32_t *sample_ptr, int64_t N, int16_t *out_pos, void *out_t, void *out_p,
                                   int64_t *out_batch, int32_t *out_ptr, int32_t *status, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    DAGR_CHECK_ARG(B >= 1 && W >= 1 && H >= 1 && W <= 32767 && H <= 32767, "B, W, H must be positive, W and H int16");
    DAGR_CHECK_ARG(N >= 0 && N < ((int64_t)1 << 31) - kAugTile, "N out of range");
    DAGR_CHECK_ARG(pos_width == 2 || pos_width == 4, "pos_width must be 2 (int16) or 4 (int32)");
    DAGR_CHECK_ARG(t_width == 4 || t_width == 8, "t_width must be 4 or 8");
    DAGR_CHECK_ARG(p_width == 1 || p_width == 2 || p_width == 4 || p_width == 8, "p_width must be 1, 2, 4 or 8");
    DAGR_CHECK_ARG(params && sample_ptr && out_ptr && status, "NULL pointer");
    DAGR_CHECK_ARG(N == 0 || (pos && t && p && out_pos && out_t && out_p && workspace), "NULL pointer");
    DAGR_CHECK_ARG(((uintptr_t)pos & 3) == 0 && ((uintptr_t)out_pos & 3) == 0, "pos and out_pos must be 4-byte aligned");
    DAGR_CHECK_ARG(workspace_bytes >= dagr_augment_workspace_bytes(N), "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    DAGR_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (N == 0) {       // no event, nothing to validate sample_ptr against: every segment is empty
        DAGR_CHECK_HIP(hipMemsetAsync(out_ptr, 0, (size_t)(B + 1) * sizeof(int32_t), s));
        return DAGR_OK;
    }
    if (pos_width == 2)
        return aug_events_launch<int16_t>(params, B, W, H, (const int16_t *)pos, t, t_width, p, p_width, sample_ptr, (int)N,
                                          out_pos, out_t, out_p, out_batch, out_ptr, status, (int32_t *)workspace, s);
    return aug_events_launch<int32_t>(params, B, W, H, (const int32_t *)pos, t, t_width, p, p_width, sample_ptr, (int)N,
                                      out_pos, out_t, out_p, out_batch, out_ptr, status, (int32_t *)workspace, s);
}

extern "C" int dagr_augment_status(const int32_t *status, void *stream) {
    DAGR_CHECK_ARG(status != nullptr, "NULL pointer");
    int32_t st = 0;
    DAGR_CHECK_HIP(hipMemcpyAsync(&st, status, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    DAGR_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    DAGR_CHECK_ARG(!(st & kAugBadPtr), "sample_ptr must run from 0 to N without decreasing (no event was written)");
    DAGR_CHECK_ARG(!(st & kAugBadCoord), "an event coordinate lies outside int16 (the event was dropped)");
    return DAGR_OK;
}

extern "C" int dagr_augment_frames(const dagr_aug_params *params, int32_t B, int32_t C, int32_t H, int32_t W,
                                   int32_t elem_bytes, int32_t reference_crop, const void *in, void *out, void *stream) {
    DAGR_CHECK_ARG(B >= 0 && C >= 1 && H >= 1 && W >= 1 && W <= 32767 && H <= 32767, "bad sizes");
    DAGR_CHECK_ARG(B <= 65535 && C <= 65535, "at most 65535 frames and channels per call");
    DAGR_CHECK_ARG(elem_bytes == 1 || elem_bytes == 4, "elem_bytes must be 1 (uint8) or 4 (fp32)");
    if (B == 0) return DAGR_OK;
    DAGR_CHECK_ARG(params && in && out, "NULL pointer");
    DAGR_CHECK_ARG(in != out, "in and out must not alias");
    const dim3 grid((unsigned)ceil_div((int64_t)H * W, kBlock), (unsigned)C, (unsigned)B);
    if (elem_bytes == 1)
        k_aug_frames<uint8_t><<<grid, kBlock, 0, (hipStream_t)stream>>>(params, C, H, W, reference_crop, (const uint8_t *)in,
                                                                        (uint8_t *)out);
    else
        k_aug_frames<float><<<grid, kBlock, 0, (hipStream_t)stream>>>(params, C, H, W, reference_crop, (const float *)in,
                                                                      (float *)out);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

extern "C" int dagr_augment_boxes(const dagr_aug_params *params, int32_t B, int32_t W, int32_t H, const float *boxes,
                                  const int64_t *box_batch, int32_t M, int32_t ld, float *out, void *stream) {
    DAGR_CHECK_ARG(B >= 1 && W >= 1 && H >= 1 && M >= 0 && ld >= 4, "bad sizes");
    if (M == 0) return DAGR_OK;
    DAGR_CHECK_ARG(params && boxes && box_batch && out, "NULL pointer");
    k_aug_boxes<<<(unsigned)ceil_div(M, kBlock), kBlock, 0, (hipStream_t)stream>>>(params, B, W, H, boxes, box_batch, M, ld,
                                                                                  out);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
