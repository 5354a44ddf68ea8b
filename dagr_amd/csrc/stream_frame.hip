// stream_frame.hip -- raw sensor frames for the event stream, prepared on the device (dagr_stream_frame).
// Reference: DSEC.preprocess_image (data/dsec_data.py: crop to the model's rows, bicubic shrink, back to uint8) followed by
// format_data's `/ 255` (utils/buffers.py) -- `frame_definition` in dagr_amd/streaming.py states it once.
//
// The shrink is torch's bicubic interpolation (A = -0.75, align_corners off, antialias off) by a whole factor f: the source
// coordinate of output pixel d is (d + 0.5) f - 0.5, whose fraction is 0.5 for even f and 0 for odd f.  So every axis has
// four taps at base - 1 .. base + 2, base = f d + (f - 1) / 2, with the weights (-3, 19, 19, -3) / 32 for even f and
// (0, 1, 0, 0) for odd f; taps are clamped to the CROP (the interpolation never saw the rest of the frame).  The 16-tap sum
// of uint8 pixels is an exact integer over 1024: it is rounded half to even, clamped to [0, 255] and divided by 255.
#include "common.hpp"

namespace dagr {
namespace {

struct FrameTaps {
    int w[4];       // weights over 32
};

__device__ __forceinline__ FrameTaps frame_taps(int f) {
    FrameTaps t;
    const bool even = (f & 1) == 0;
    t.w[0] = even ? -3 : 0;
    t.w[1] = even ? 19 : 32;
    t.w[2] = even ? 19 : 0;
    t.w[3] = even ? -3 : 0;
    return t;
}

// One thread per output pixel (all three channels); blockIdx.y is the output row, blockIdx.z the frame.  Neighbouring
// threads read neighbouring pixel groups of the same four frame rows.
__global__ __launch_bounds__(kBlock) void k_stream_frame(const uint8_t *__restrict__ frames, int64_t frame_stride,
                                                        int64_t row_stride, const int32_t *__restrict__ lanes, int fx, int fy,
                                                        int width, int height, int bgr, float *__restrict__ out, int B,
                                                        int64_t stride_b, int64_t stride_c, int64_t stride_y,
                                                        int64_t stride_x, int32_t *__restrict__ status) {
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y, k = blockIdx.z;
    const int lane = lanes[k];
    if (lane < 0 || lane >= B) {
        if (x == 0 && y == 0) atomicOr(status, 32);
        return;
    }
    if (x >= width) return;
    const FrameTaps tx = frame_taps(fx), ty = frame_taps(fy);
    const int bx = fx * x + (fx - 1) / 2, by = fy * y + (fy - 1) / 2;
    const int crop_w = fx * width, crop_h = fy * height;
    const uint8_t *frame = frames + (int64_t)k * frame_stride;
    int sum[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (ty.w[j] == 0) continue;
        const int sy = min(max(by - 1 + j, 0), crop_h - 1);
        const uint8_t *row = frame + (int64_t)sy * row_stride;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (tx.w[i] == 0) continue;
            const int sx = min(max(bx - 1 + i, 0), crop_w - 1);
            const int w = ty.w[j] * tx.w[i];
            const uint8_t *px = row + 3 * (int64_t)sx;
            sum[0] += w * (int)px[0];
            sum[1] += w * (int)px[1];
            sum[2] += w * (int)px[2];
        }
    }
    float *o = out + (int64_t)lane * stride_b + (int64_t)y * stride_y + (int64_t)x * stride_x;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int s = sum[bgr ? 2 - c : c];
        int q = s >> 10;                                // floor(s / 1024), also below zero
        const int r = s & 1023;
        if (r > 512 || (r == 512 && (q & 1))) q++;      // half to even (torch.round)
        q = min(max(q, 0), 255);
        o[(int64_t)c * stride_c] = __fdiv_rn((float)q, 255.0f);
    }
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" int dagr_stream_frame(const uint8_t *frames, int64_t frame_stride, int64_t row_stride, int32_t n,
                                 const int32_t *lanes, int32_t frame_w, int32_t frame_h, int32_t fx, int32_t fy,
                                 int32_t width, int32_t height, int32_t bgr, float *out, int32_t B, int64_t stride_b,
                                 int64_t stride_c, int64_t stride_y, int64_t stride_x, int32_t *status, void *stream) {
    DAGR_CHECK_ARG(n >= 0 && n <= 65535 && B >= 1, "stream frame: bad frame or lane count");
    DAGR_CHECK_ARG(fx >= 1 && fy >= 1 && width >= 1 && height >= 1 && height <= 65535 && fx <= 32767 / width &&
                   fy <= 32767 / height, "stream frame: bad factors or size");
    DAGR_CHECK_ARG(frame_w >= fx * width && frame_h >= fy * height, "stream frame: the frame is smaller than the crop");
    DAGR_CHECK_ARG(row_stride >= 3 * (int64_t)frame_w && (n <= 1 || frame_stride >= row_stride * frame_h),
                   "stream frame: strides smaller than the frame");
    DAGR_CHECK_ARG(stride_b >= 0 && stride_c >= 1 && stride_y >= 1 && stride_x >= 1, "stream frame: bad output strides");
    if (n == 0) return DAGR_OK;
    DAGR_CHECK_ARG(frames && lanes && out && status, "stream frame: NULL pointer");
    const dim3 grid((unsigned)ceil_div(width, kBlock), (unsigned)height, (unsigned)n);
    k_stream_frame<<<grid, kBlock, 0, (hipStream_t)stream>>>(frames, frame_stride, row_stride, lanes, fx, fy, width, height,
                                                             bgr ? 1 : 0, out, B, stride_b, stride_c, stride_y, stride_x,
                                                             status);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
