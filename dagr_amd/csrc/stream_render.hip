// stream_render.hip -- the picture of a stream's step, on the device: dagr_stream_trail keeps a ring of the last centres of
// every track slot, dagr_stream_render paints the lanes' frames (base, resident events, trails, box outlines, id plates).
// include/dagr_hip.h states the rule, dagr_amd/streaming.py: RenderDefinition is the same in numpy; nothing is restated here.
//   k_render_mark_events  one thread per slot of a lane's resident segment: atomicMax of the arrival index + 1 into last
//   k_render_mark_trails  one wave per ring, its lanes striding over the steps of a segment: atomicMax of slot + 1 into owner
//   k_render_compose      one thread per pixel, a 32 x 8 tile per workgroup: the lane's rows are prepared 256 at a time into
//                         LDS, culled against the tile and compacted in row order; the pixel walks what is left (every
//                         thread reads the same entry: an LDS broadcast), writes its three bytes once and puts its two map
//                         entries back to 0, so that no launch clears the maps.
// The two maps take integer maxima only: no result depends on the order of execution.
#include "stream_state.hpp"
#include "stream_track.hpp"

#include <algorithm>

namespace dagr {
namespace {

constexpr int kTileW = 32, kTileH = 8;      // kTileW * kTileH == kBlock
constexpr int kRowChunk = kBlock;           // rows prepared per pass, one per thread
constexpr int kCoordMax = 1 << 20;
constexpr int kCountFold = 1 << 30;

__constant__ int32_t c_glyph[10] = {DAGR_RENDER_GLYPH_0, DAGR_RENDER_GLYPH_1, DAGR_RENDER_GLYPH_2, DAGR_RENDER_GLYPH_3,
                                    DAGR_RENDER_GLYPH_4, DAGR_RENDER_GLYPH_5, DAGR_RENDER_GLYPH_6, DAGR_RENDER_GLYPH_7,
                                    DAGR_RENDER_GLYPH_8, DAGR_RENDER_GLYPH_9};

struct Rings {
    int64_t *id;
    int32_t *count;
    int32_t *pt;        // [n, trail, 2]
};

size_t carve_rings(int B, int M, int T, char *base, Rings *out) {
    const size_t n = (size_t)B * M;
    Rings r;
    r.id = (int64_t *)base;
    r.count = (int32_t *)(base + 8 * n);
    r.pt = (int32_t *)(base + 12 * n);
    if (out) *out = r;
    return 12 * n + 8 * n * (size_t)T;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN
// (int32_t)floorf(clamp(v, -2^20, 2^20)) of a finite v
__device__ __forceinline__ int coord(float v) { return (int)floorf(fminf(fmaxf(v, -(float)kCoordMax), (float)kCoordMax)); }
__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return min(max(v, lo), hi); }
// the palette entry of a track id
__device__ __forceinline__ int id_color(int64_t id, int n_colors) {
    return id == 0 ? 0 : 1 + (int)((uint64_t)(id - 1) % (uint64_t)(n_colors - 1));
}

__global__ __launch_bounds__(kBlock) void k_trail_reset(Rings r, int n) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        r.id[i] = 0;
        r.count[i] = 0;
    }
}

// one thread per (lane, slot), behind the tracker's launch
__global__ __launch_bounds__(kBlock) void k_trail(Rings r, Tracks tr, const int64_t *__restrict__ t_ref, int B, int M, int T) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= B * M) return;
    const int64_t id = tr.id[i];
    if (id == 0) {                      // a free slot
        r.id[i] = 0;
        r.count[i] = 0;
        return;
    }
    int cnt = r.count[i];
    if (r.id[i] != id) {                // the slot has been taken by another track
        r.id[i] = id;
        cnt = 0;
    }
    const int64_t ref = t_ref[i / M];
    if (ref != kNever && tr.t_last[i] == ref) {
        const float4 bx = tr.box[i];
        const float cx = (bx.x + bx.z) * 0.5f, cy = (bx.y + bx.w) * 0.5f;
        if (finite_f(cx) && finite_f(cy)) {
            cnt = max(cnt, 0);
            int32_t *pt = r.pt + ((int64_t)i * T + cnt % T) * 2;
            pt[0] = coord(cx);
            pt[1] = coord(cy);
            cnt += 1;
            if (cnt >= kCountFold) cnt = T + kCountFold % T;
        }
    }
    r.count[i] = cnt;
}

// blockIdx.y: the lane; blockIdx.x: 256 slots of its segment (the grid comes from the capacity, the segment's count bounds it)
__global__ __launch_bounds__(kBlock) void k_render_mark_events(StreamState st, int cap, int64_t window_us, int H, int W,
                                                              int32_t *__restrict__ last, int32_t *__restrict__ status) {
    const int b = blockIdx.y;
    const int start = clamp_i(st.seg[2 * b], 0, cap);
    const int cnt = clamp_i(st.seg[2 * b + 1], 0, cap - start);
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    const int64_t ref = st.t_ref[b];
    if (ref == kNever) return;
    const bool cur = st.hdr[0] & 1;
    const int64_t t = (cur ? st.t1 : st.t0)[start + j];
    if (window_us >= 0 && (t > ref || (uint64_t)ref - (uint64_t)t >= (uint64_t)window_us)) return;
    const int ch = (int)(cur ? st.p1 : st.p0)[start + j] - 1;
    if (ch < -3 || ch > 2) {
        atomicOr(status, DAGR_RENDER_BAD_POLARITY);
        return;
    }
    const int32_t xy = (cur ? st.xy1 : st.xy0)[start + j];
    const int x = (int16_t)(xy & 0xffff), y = (int16_t)(xy >> 16);
    if (x < 0 || x >= W || y < 0 || y >= H) return;
    atomicMax(&last[((int64_t)b * H + y) * W + x], j + 1);
}

// one wave per ring
__global__ __launch_bounds__(kBlock) void k_render_mark_trails(Rings r, int B, int M, int T, int H, int W,
                                                              int32_t *__restrict__ owner, int32_t *__restrict__ status) {
    const int i = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= B * M) return;
    const int cnt = max(r.count[i], 0);
    const int npts = min(cnt, T);
    if (r.id[i] == 0 || npts < 2) return;
    const int b = i / M, slot = i - b * M;
    const int first = cnt <= T ? 0 : cnt % T;
    const int32_t *pt = r.pt + (int64_t)i * T * 2;
    int32_t *own = owner + (int64_t)b * H * W;
    for (int s = 0; s + 1 < npts; ++s) {
        const int a0 = (first + s) % T, a1 = (first + s + 1) % T;
        const int x0 = clamp_i(pt[2 * a0], -kCoordMax, kCoordMax), y0 = clamp_i(pt[2 * a0 + 1], -kCoordMax, kCoordMax);
        const int x1 = clamp_i(pt[2 * a1], -kCoordMax, kCoordMax), y1 = clamp_i(pt[2 * a1 + 1], -kCoordMax, kCoordMax);
        const int dx = x1 - x0, dy = y1 - y0;
        const int adx = abs(dx), ady = abs(dy), n = max(adx, ady);
        if (n > W + H) {
            if (lane == 0) atomicOr(status, DAGR_RENDER_LONG_SEGMENT);
            continue;
        }
        const bool x_major = adx >= ady;
        const int sx = dx > 0 ? 1 : (dx < 0 ? -1 : 0), sy = dy > 0 ? 1 : (dy < 0 ? -1 : 0);
        const int64_t dminor = x_major ? ady : adx;
        for (int k = lane; k <= n; k += kWave) {
            const int off = n == 0 ? 0 : (int)((2 * (int64_t)k * dminor + n) / (2 * (int64_t)n));
            const int x = x_major ? x0 + sx * k : x0 + sx * off;
            const int y = x_major ? y0 + sy * off : y0 + sy * k;
            if (x >= 0 && x < W && y >= 0 && y < H) atomicMax(&own[(int64_t)y * W + x], slot + 1);
        }
    }
}

// Chebyshev distance of pixel (px, py) to the border of the rectangle [xa, xb] x [ya, yb] (dagr_viz_render's outline rule)
__device__ __forceinline__ int border_distance(int px, int py, int xa, int ya, int xb, int yb) {
    if (px >= xa && px <= xb && py >= ya && py <= yb) return min(min(px - xa, xb - px), min(py - ya, yb - py));
    const int dx = max(max(xa - px, px - xb), 0);
    const int dy = max(max(ya - py, py - yb), 0);
    return max(dx, dy);
}

struct RenderRow {
    int xa, ya, xb, yb;     // the rectangle
    int color;              // its palette entry
    int nd, digits, top;    // the plate: digits (0: none), digit d at bits 4 * d, the plate's first row
};

struct ComposeArgs {
    StreamState st;         // st.hdr == nullptr: no events
    int cap;
    double alpha;
    const float *det;
    const int32_t *n_keep;
    int A;
    const int64_t *track_id;
    const int64_t *ring_id; // nullptr: no trails
    int M;
    int half_width, ids, scale;
    const uint8_t *colors;
    int n_colors;
    const uint8_t *base;
    int64_t base_stride;
    uint8_t *out;
    int H, W;
    int32_t *last, *owner, *status;
};

__global__ __launch_bounds__(kBlock) void k_render_compose(ComposeArgs a) {
    __shared__ RenderRow s_row[kRowChunk];
    __shared__ int s_wave[kBlock / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
    const int px = tx0 + (tid & (kTileW - 1)), py = ty0 + tid / kTileW;
    const bool inside = px < a.W && py < a.H;
    const bool flagger = blockIdx.x == 0 && blockIdx.y == 0;       // one workgroup per lane reports the rows' flags
    const int rows = a.A > 0 ? clamp_i(a.n_keep[b], 0, a.A) : 0;
    const int hw = a.half_width, s = a.scale;
    int box_color = -1, plate_color = -1;
    bool glyph = false;
    for (int r0 = 0; r0 < rows; r0 += kRowChunk) {
        const int r = r0 + tid;
        RenderRow row;
        bool keep = false;
        if (r < rows) {
            const float *d = a.det + ((int64_t)b * a.A + r) * 6;
            const float x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3];
            if (finite_f(x1) && finite_f(y1) && finite_f(x2) && finite_f(y2)) {
                const int cx1 = coord(x1), cy1 = coord(y1), cx2 = coord(x2), cy2 = coord(y2);
                row.xa = min(cx1, cx2); row.xb = max(cx1, cx2);
                row.ya = min(cy1, cy2); row.yb = max(cy1, cy2);
                row.nd = row.digits = row.top = 0;
                keep = true;
                if (a.track_id) {
                    const int64_t id = a.track_id[(int64_t)b * a.A + r];
                    row.color = id_color(id, a.n_colors);
                    if (a.ids && id != 0) {
                        uint32_t v = (uint32_t)((uint64_t)id % 1000000ull);
                        int nd = 1;
                        for (uint32_t q = v; q >= 10; q /= 10) nd++;
                        for (int k = nd - 1; k >= 0; --k, v /= 10) row.digits |= (int)(v % 10) << (4 * k);
                        row.nd = nd;
                        row.top = row.ya - 7 * s >= 0 ? row.ya - 7 * s : row.ya + 1;
                    }
                } else {
                    const float l = d[5];
                    if (l >= 0.0f && l < (float)a.n_colors) {
                        row.color = (int)l;
                    } else {
                        keep = false;
                        if (flagger) atomicOr(a.status, DAGR_RENDER_BAD_CLASS);
                    }
                }
            }
            if (keep) {                 // the cull: the outline's band or the plate meets the tile
                const int tx1 = tx0 + kTileW - 1, ty1 = ty0 + kTileH - 1;
                const bool band = row.xa - hw <= tx1 && row.xb + hw >= tx0 && row.ya - hw <= ty1 && row.yb + hw >= ty0 &&
                                  !(tx0 > row.xa + hw && tx1 < row.xb - hw && ty0 > row.ya + hw && ty1 < row.yb - hw);
                const bool plate = row.nd > 0 && row.xa <= tx1 && row.xa + (4 * row.nd + 1) * s - 1 >= tx0 &&
                                   row.top <= ty1 && row.top + 7 * s - 1 >= ty0;
                keep = band || plate;
            }
        }
        const uint64_t m = __ballot(keep);
        if (lane == 0) s_wave[wid] = __popcll(m);
        __syncthreads();
        int at = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) {
            at += w < wid ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (keep) s_row[at + lanes_below(m, lane)] = row;
        __syncthreads();
        if (inside) {
            for (int e = 0; e < total; ++e) {
                const RenderRow w = s_row[e];
                if (border_distance(px, py, w.xa, w.ya, w.xb, w.yb) <= hw) box_color = w.color;
                const int rx = px - w.xa, ry = py - w.top;
                if (w.nd > 0 && rx >= 0 && rx < (4 * w.nd + 1) * s && ry >= 0 && ry < 7 * s) {
                    plate_color = w.color;
                    const int gx = rx / s - 1, gy = ry / s - 1;
                    glyph = false;
                    if (gx >= 0 && gy >= 0 && gy < 5 && (gx & 3) < 3) {
                        const int digit = min((w.digits >> (4 * (gx >> 2))) & 15, 9);
                        glyph = (c_glyph[digit] >> (14 - (gy * 3 + (gx & 3)))) & 1;
                    }
                }
            }
        }
        __syncthreads();            // the next pass rewrites s_row and s_wave
    }
    if (!inside) return;
    const int64_t pix = (int64_t)py * a.W + px, HW = (int64_t)a.H * a.W;
    uint8_t v[3] = {0, 0, 0};
    if (a.base) {
        const uint8_t *src = a.base + (int64_t)b * a.base_stride + pix * 3;
        v[0] = src[0]; v[1] = src[1]; v[2] = src[2];
    }
    if (a.st.hdr) {
        int32_t *lp = a.last + (int64_t)b * HW + pix;
        const int j = *lp;
        if (j != 0) {
            *lp = 0;
            const int start = clamp_i(a.st.seg[2 * b], 0, a.cap);
            const int at = clamp_i(start + j - 1, 0, a.cap - 1);
            int ch = (int)((a.st.hdr[0] & 1) ? a.st.p1 : a.st.p0)[at] - 1;
            ch = clamp_i(ch < 0 ? ch + 3 : ch, 0, 2);
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = (uint8_t)(int)(a.alpha * (double)v[c]);
            const uint8_t add = (uint8_t)(int)((double)v[ch] + 255.0 * (1.0 - a.alpha));
            v[0] = ch == 0 ? add : v[0];
            v[1] = ch == 1 ? add : v[1];
            v[2] = ch == 2 ? add : v[2];
        }
    }
    int color = -1;
    if (a.ring_id) {
        int32_t *op = a.owner + (int64_t)b * HW + pix;
        const int o = *op;
        if (o != 0) {
            *op = 0;
            color = id_color(a.ring_id[(int64_t)b * a.M + clamp_i(o - 1, 0, a.M - 1)], a.n_colors);
        }
    }
    if (box_color >= 0) color = box_color;
    if (plate_color >= 0) color = plate_color;
    if (color >= 0) {
        const uint8_t *c = a.colors + 3 * clamp_i(color, 0, a.n_colors - 1);
        const bool black = plate_color >= 0 && glyph;
        v[0] = black ? 0 : c[0];
        v[1] = black ? 0 : c[1];
        v[2] = black ? 0 : c[2];
    }
    uint8_t *dst = a.out + ((int64_t)b * HW + pix) * 3;
    dst[0] = v[0];
    dst[1] = v[1];
    dst[2] = v[2];
}

bool trail_sizes_ok(int32_t B, int32_t M, int32_t T) {
    return B >= 1 && B <= 65535 && M >= 1 && M <= DAGR_TRACK_MAX_TRACKS && T >= 1 && T <= DAGR_RENDER_MAX_TRAIL;
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" size_t dagr_stream_trail_bytes(int32_t B, int32_t max_tracks, int32_t trail) {
    return trail_sizes_ok(B, max_tracks, trail) ? carve_rings(B, max_tracks, trail, nullptr, nullptr) : 0;
}

extern "C" int dagr_stream_trail_reset(void *rings, size_t bytes, int32_t B, int32_t max_tracks, int32_t trail, void *stream) {
    DAGR_CHECK_ARG(trail_sizes_ok(B, max_tracks, trail), "B, max_tracks or trail out of range");
    DAGR_CHECK_ARG(rings && (uintptr_t)rings % 8 == 0, "rings is NULL or not 8-byte aligned");
    DAGR_CHECK_ARG(bytes >= dagr_stream_trail_bytes(B, max_tracks, trail), "rings smaller than dagr_stream_trail_bytes");
    Rings r;
    carve_rings(B, max_tracks, trail, (char *)rings, &r);
    const int n = B * max_tracks;
    k_trail_reset<<<(unsigned)ceil_div(n, kBlock), kBlock, 0, (hipStream_t)stream>>>(r, n);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

extern "C" int dagr_stream_trail(void *rings, size_t bytes, int32_t B, int32_t max_tracks, int32_t trail, const void *tracks,
                                 size_t tracks_bytes, const int64_t *t_ref, void *stream) {
    DAGR_CHECK_ARG(trail_sizes_ok(B, max_tracks, trail), "B, max_tracks or trail out of range");
    DAGR_CHECK_ARG(rings && (uintptr_t)rings % 8 == 0, "rings is NULL or not 8-byte aligned");
    DAGR_CHECK_ARG(bytes >= dagr_stream_trail_bytes(B, max_tracks, trail), "rings smaller than dagr_stream_trail_bytes");
    DAGR_CHECK_ARG(tracks && (uintptr_t)tracks % 16 == 0 && t_ref, "tracks is NULL or not 16-byte aligned, or t_ref is NULL");
    const bool plain = tracks_bytes == dagr_stream_track_bytes(B, max_tracks);
    DAGR_CHECK_ARG(plain || tracks_bytes == dagr_stream_track_cv_bytes(B, max_tracks),
                   "tracks_bytes is neither dagr_stream_track_bytes nor dagr_stream_track_cv_bytes");
    Rings r;
    carve_rings(B, max_tracks, trail, (char *)rings, &r);
    Tracks tr;
    carve_tracks(!plain, B, max_tracks, (char *)const_cast<void *>(tracks), &tr);
    k_trail<<<(unsigned)ceil_div((int64_t)B * max_tracks, kBlock), kBlock, 0, (hipStream_t)stream>>>(r, tr, t_ref, B, max_tracks,
                                                                                                    trail);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

extern "C" size_t dagr_stream_render_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (int64_t)H * W > ((int64_t)1 << 29)) return 0;
    return 2 * align_up((size_t)B * (size_t)H * (size_t)W * sizeof(int32_t), 256);
}

extern "C" int dagr_stream_render(const void *state, int32_t B, int64_t capacity, int64_t event_window_us, double alpha,
                                  const float *det, const int32_t *n_keep, int32_t A, const int64_t *track_id,
                                  const void *rings, int32_t max_tracks, int32_t trail, int32_t linewidth, int32_t ids,
                                  int32_t id_scale, const uint8_t *colors, int32_t n_colors, const uint8_t *base,
                                  int64_t base_stride, uint8_t *out, int32_t H, int32_t W, int32_t *status, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    const size_t need = dagr_stream_render_workspace_bytes(B, H, W);
    DAGR_CHECK_ARG(need != 0, "B, H or W out of range");
    DAGR_CHECK_ARG((int64_t)B * H * W <= ((int64_t)1 << 31) / 4 && ceil_div(H, kTileH) <= 65535, "B * H * W or H out of range");
    DAGR_CHECK_ARG(alpha >= 0.0 && alpha <= 1.0, "alpha must lie in [0, 1]");
    DAGR_CHECK_ARG(linewidth >= 1 && linewidth <= DAGR_RENDER_MAX_LINEWIDTH, "linewidth out of range");
    DAGR_CHECK_ARG(id_scale >= 1 && id_scale <= DAGR_RENDER_MAX_ID_SCALE, "id_scale out of range");
    DAGR_CHECK_ARG(colors && n_colors >= 2 && n_colors <= 256, "colors is NULL or n_colors outside 2..256");
    DAGR_CHECK_ARG(A >= 0 && (A == 0 || (det && n_keep)), "A < 0, or det / n_keep is NULL");
    DAGR_CHECK_ARG((uintptr_t)det % 4 == 0 && (uintptr_t)n_keep % 4 == 0 && (uintptr_t)track_id % 8 == 0,
                   "det, n_keep or track_id is misaligned");
    DAGR_CHECK_ARG(out && status && (uintptr_t)status % 4 == 0, "out or status is NULL or misaligned");
    DAGR_CHECK_ARG(base_stride == 0 || base_stride >= (int64_t)H * W * 3, "base_stride is smaller than an image");
    DAGR_CHECK_ARG(workspace && (uintptr_t)workspace % 256 == 0 && workspace_bytes >= need,
                   "workspace is NULL, not 256-byte aligned or smaller than dagr_stream_render_workspace_bytes");
    ComposeArgs a = {};
    if (state) {
        DAGR_CHECK_ARG(B < kStreamLanes && capacity >= 1 && capacity < (1ll << 31) / 64 && (uintptr_t)state % 8 == 0,
                       "state: B, capacity or alignment out of range");
        carve_stream(B, capacity, (char *)const_cast<void *>(state), &a.st);
    }
    Rings r = {};
    if (rings) {
        DAGR_CHECK_ARG(trail_sizes_ok(B, max_tracks, trail) && (uintptr_t)rings % 8 == 0,
                       "rings: B, max_tracks, trail or alignment out of range");
        carve_rings(B, max_tracks, trail, (char *)const_cast<void *>(rings), &r);
    }
    hipStream_t s = (hipStream_t)stream;
    a.cap = (int)capacity;
    a.alpha = alpha;
    a.det = det; a.n_keep = n_keep; a.A = A; a.track_id = track_id;
    a.ring_id = r.id; a.M = max_tracks;
    a.half_width = linewidth / 2; a.ids = ids; a.scale = id_scale;
    a.colors = colors; a.n_colors = n_colors;
    a.base = base; a.base_stride = base_stride; a.out = out;
    a.H = H; a.W = W;
    a.last = (int32_t *)workspace;
    a.owner = (int32_t *)((char *)workspace + need / 2);
    a.status = status;
    if (state) {
        const dim3 grid((unsigned)ceil_div(capacity, kBlock), (unsigned)B);
        k_render_mark_events<<<grid, kBlock, 0, s>>>(a.st, a.cap, event_window_us, H, W, a.last, status);
        DAGR_CHECK_LAUNCH();
    }
    if (rings) {
        const unsigned grid = (unsigned)ceil_div((int64_t)B * max_tracks, kBlock / kWave);
        k_render_mark_trails<<<grid, kBlock, 0, s>>>(r, B, max_tracks, trail, H, W, a.owner, status);
        DAGR_CHECK_LAUNCH();
    }
    const dim3 grid((unsigned)ceil_div(W, kTileW), (unsigned)ceil_div(H, kTileH), (unsigned)B);
    k_render_compose<<<grid, kBlock, 0, s>>>(a);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
