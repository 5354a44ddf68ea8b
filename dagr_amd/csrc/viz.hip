// viz.hip -- detection visualisation frames on the device (scripts/visualize_detections.py).
// Reference: src/dagr/visualization/event_viz.py:3-10 (a numba loop over the events of one image) and the box outlines of
// bbox_viz.py:11-53 (cv2.rectangle).  F independent frames per call:
//   1. `last` (F*H*W int32, cleared to -1) receives, per pixel, the largest index of an event of that frame on it
//      (atomicMax).  The reference's loop blends from an untouched copy of the image, so the pixel's final value depends
//      only on that last event: no ordering of the events is needed.
//   2. one thread per output pixel composites: alpha * base on all channels (float64, truncated to uint8), plus
//      255 * (1 - alpha) on channel p - 1 (Python's negative-index wrap) of the last event, then the box outlines of the
//      frame in list order (a later box wins).
#include "common.hpp"

#include <algorithm>

namespace dagr {
namespace {

enum : int32_t { kVizBadPolarity = 1, kVizBadClass = 2, kVizBadImage = 4, kVizBadAlpha = 8 };

__global__ __launch_bounds__(kBlock) void k_viz_scatter(const int32_t *__restrict__ ev_x, const int32_t *__restrict__ ev_y,
                                                       const int8_t *__restrict__ ev_p, const int32_t *__restrict__ ev_ptr,
                                                       int F, int n_events, int H, int W, int32_t *__restrict__ last,
                                                       int32_t *__restrict__ status) {
    const int stride = (int)(gridDim.x * blockDim.x);
    const int lo = ev_ptr[0], hi = ev_ptr[F];
    for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < n_events; k += stride) {
        if (k < lo || k >= hi) continue;                      // in no frame's segment
        // frame of event k: the largest f with ev_ptr[f] <= k (empty segments share their start with the next one)
        int a = 0, b = F;                                     // invariant: ev_ptr[a] <= k < ev_ptr[b]
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if (ev_ptr[m] <= k) a = m; else b = m;
        }
        const int ch = (int)ev_p[k] - 1;
        if (ch < -3 || ch > 2) {                              // outside Python's index range of a 3-channel pixel
            atomicOr(status, kVizBadPolarity);
            continue;
        }
        const int x = ev_x[k], y = ev_y[k];
        if (x < 0 || x >= W || y < 0 || y >= H) continue;
        atomicMax(&last[((int64_t)a * H + y) * W + x], k);
    }
}

// Chebyshev distance of pixel (px, py) to the border of the rectangle [xa, xb] x [ya, yb] (xa <= xb, ya <= yb).
__device__ __forceinline__ int64_t border_distance(int64_t px, int64_t py, int64_t xa, int64_t ya, int64_t xb, int64_t yb) {
    if (px >= xa && px <= xb && py >= ya && py <= yb)
        return min(min(px - xa, xb - px), min(py - ya, yb - py));
    const int64_t dx = max(max(xa - px, px - xb), (int64_t)0);
    const int64_t dy = max(max(ya - py, py - yb), (int64_t)0);
    return max(dx, dy);
}

__global__ __launch_bounds__(kBlock) void k_viz_composite(const uint8_t *images, int n_images, int H, int W,
                                                         const int32_t *__restrict__ frame_image,
                                                         const int8_t *__restrict__ ev_p, const double *__restrict__ alpha,
                                                         const int32_t *__restrict__ last,
                                                         const int32_t *__restrict__ boxes, const int32_t *__restrict__ box_ptr,
                                                         int n_boxes, int half_width, const uint8_t *__restrict__ colors,
                                                         int n_colors, uint8_t *out, int32_t *__restrict__ status) {
    const int64_t HW = (int64_t)H * W;
    const int64_t pix = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int f = (int)blockIdx.y;
    if (pix >= HW) return;
    const int img = frame_image[f];
    if (img < 0 || img >= n_images) {
        if (pix == 0) atomicOr(status, kVizBadImage);
        return;
    }
    const uint8_t *src = images + ((int64_t)img * HW + pix) * 3;
    uint8_t v[3] = {src[0], src[1], src[2]};
    const int k = last[(int64_t)f * HW + pix];
    if (k >= 0) {
        const double a = alpha[f];
        if (a >= 0.0 && a <= 1.0) {
            // event_viz.py:8-9: img[y, x, :] = alpha * img_copy[y, x, :]; img[y, x, p - 1] += 255 * (1 - alpha)
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = (uint8_t)(int)(a * (double)v[c]);
            int ch = (int)ev_p[k] - 1;                        // in [-3, 2]: checked by the scatter
            if (ch < 0) ch += 3;
            v[ch] = (uint8_t)(int)((double)v[ch] + 255.0 * (1.0 - a));
        } else if (pix == 0) {
            atomicOr(status, kVizBadAlpha);
        }
    }
    if (box_ptr != nullptr) {
        const int64_t px = pix % W, py = pix / W;
        const int j0 = max(box_ptr[f], 0), j1 = min(box_ptr[f + 1], n_boxes);
        int hit = -1;
        for (int j = j0; j < j1; j++) {
            const int32_t *bx = boxes + (int64_t)j * 5;
            const int64_t x0 = bx[0], y0 = bx[1], x1 = bx[2], y1 = bx[3];
            if (border_distance(px, py, min(x0, x1), min(y0, y1), max(x0, x1), max(y0, y1)) <= half_width) hit = j;
        }
        if (hit >= 0) {
            const int cls = boxes[(int64_t)hit * 5 + 4];
            if (cls >= 0 && cls < n_colors) {
#pragma unroll
                for (int c = 0; c < 3; c++) v[c] = colors[cls * 3 + c];
            } else {
                atomicOr(status, kVizBadClass);
            }
        }
    }
    uint8_t *dst = out + ((int64_t)f * HW + pix) * 3;
    dst[0] = v[0];
    dst[1] = v[1];
    dst[2] = v[2];
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" size_t dagr_viz_workspace_bytes(int32_t F, int32_t H, int32_t W) {
    if (F < 1 || H < 1 || W < 1) {
        set_error("dagr_viz_workspace_bytes: F, H and W must be positive");
        return 0;
    }
    return align_up((size_t)F * (size_t)H * (size_t)W * sizeof(int32_t), 256);
}

extern "C" int dagr_viz_render(const uint8_t *images, int32_t n_images, int32_t H, int32_t W, const int32_t *frame_image,
                               int32_t F, const int32_t *ev_x, const int32_t *ev_y, const int8_t *ev_p,
                               const int32_t *ev_ptr, int32_t n_events, const double *alpha, const int32_t *boxes,
                               const int32_t *box_ptr, int32_t n_boxes, int32_t linewidth, const uint8_t *colors,
                               int32_t n_colors, uint8_t *out, int32_t *status, void *workspace, size_t workspace_bytes,
                               void *stream) {
    DAGR_CHECK_ARG(F >= 1 && F <= 65535, "F must be in [1, 65535]");
    DAGR_CHECK_ARG(H >= 1 && W >= 1 && (int64_t)H * W <= ((int64_t)1 << 31) / 4, "bad image size");
    DAGR_CHECK_ARG(n_images >= 1 && n_events >= 0 && n_boxes >= 0 && n_colors >= 0, "bad sizes");
    DAGR_CHECK_ARG(images && frame_image && ev_ptr && alpha && out && status && workspace, "NULL pointer");
    DAGR_CHECK_ARG(n_events == 0 || (ev_x && ev_y && ev_p), "NULL event pointer");
    DAGR_CHECK_ARG(box_ptr == nullptr || (linewidth >= 1 && (n_boxes == 0 || boxes) && (n_colors == 0 || colors)),
                   "boxes need linewidth >= 1, boxes and colors");
    const size_t need = dagr_viz_workspace_bytes(F, H, W);
    DAGR_CHECK_ARG(workspace_bytes >= need, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    int32_t *last = (int32_t *)workspace;
    DAGR_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    DAGR_CHECK_HIP(hipMemsetAsync(last, 0xff, (size_t)F * H * W * sizeof(int32_t), s));   // -1: no event
    if (n_events > 0) {
        const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n_events, kBlock), 8192);
        k_viz_scatter<<<grid, kBlock, 0, s>>>(ev_x, ev_y, ev_p, ev_ptr, F, n_events, H, W, last, status);
        DAGR_CHECK_LAUNCH();
    }
    const dim3 grid((unsigned)ceil_div((int64_t)H * W, kBlock), (unsigned)F);
    k_viz_composite<<<grid, kBlock, 0, s>>>(images, n_images, H, W, frame_image, ev_p, alpha, last, boxes, box_ptr,
                                            n_boxes, linewidth / 2, colors, n_colors, out, status);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
