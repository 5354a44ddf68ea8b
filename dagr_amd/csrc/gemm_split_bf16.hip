// gemm_split_bf16.hip -- fp32-accurate GEMM / implicit-GEMM 3x3 convolution on the bf16 matrix pipe.
//
// The image branch's trunk (net_img.py:42-48, BatchNorm folded) is fp32 GEMM work, and the fp32-input MFMA runs at 1/16 of
// the bf16 MFMA rate on gfx950.  An fp32 product is rebuilt from bf16 pieces instead: every operand is written as the sum of
// three bf16 values (3 x 8 mantissa bits, fp32's exponent range),
//     a = a1 + a2 + a3,   a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2)      (both subtractions are exact)
// and the six products of order up to 2^-16 are kept: a1w1, a1w2, a2w1, a2w2, a1w3, a3w1.  Each of the three dropped ones
// is at most 2^-24 relative.  Per K-tile of 32 the six products are summed by a chain of six MFMAs that starts from zero
// (corrections first, a1w1 last), and the vector ALU adds the tile's sum to the running fp32 sum.
//
//   D[M, N] = act(A . W + bias (+ R)),  fp32 in memory on both sides, no split-K, no atomics: same operands, same bits.
//
// Weights are packed once (dagr_gemm_split_bf16_pack) into three bf16 planes, K-tile major: [K/32][3][Npad][32] with Npad =
// N rounded up to the 128-column tile (zero filled), so that the W tile of a block is three contiguous 8 KB pieces.
// Activations stay fp32: the A tile is loaded to registers, split there, and written to LDS as three planes.
//
// Tile: (32*MI) x 128 x 32, MI = 2 or 1 (a 128-row tile lost to the 64-row one on every shape of the image branch); 4 waves as 2 x 2, each (16*MI) x 64 of the output; mfma_f32_16x16x32_bf16 with the
// operands swapped (W as the MFMA's A operand), so a lane ends up with four consecutive output CHANNELS of one row and the
// epilogue reads bias / residual and writes D as float4.  One LDS buffer, register staging with the global loads of tile
// t+1 issued before the MFMAs of tile t and written after them.  LDS rows are 32 bf16 padded to 40 (80 B): the sixteen rows
// of a fragment read then fall on sixteen distinct 16-byte slots of the 256-byte bank row.
//
// A-row addressing (Geo): plain rows with a pitch; a 1x1 convolution with spatial stride (reads every s-th pixel in place);
// a 3x3 / stride 1 / pad 1 convolution on an NHWC map, K = (tap, channel) -- a K-tile lies inside one tap because C is a
// multiple of 32, taps outside the image (which also closes the seam between two images of the batch) read as zero.
#include <algorithm>

#include "common.hpp"

namespace dagr {
namespace {

constexpr int kKT = 32;        // K-tile
constexpr int kBN = 128;       // N-tile
constexpr int kPitch = 40;     // LDS row pitch in bf16 (32 + 8 of padding)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct Geo {
    int mode;                  // 0: rows, 1: 1x1 with spatial stride, 2: 3x3 stride 1 pad 1
    int H, W, C, s, Ho, Wo;
};

struct Args {
    const float *A;
    const unsigned short *Wp;
    const float *bias, *R;
    float *D;
    int64_t M, lda, ldr, ldd;
    int K, N, Npad, act, n_tiles_n, n_blocks;
    Geo g;
};

__device__ __forceinline__ unsigned short bf16_bits(__bf16 v) { return __builtin_bit_cast(unsigned short, v); }

// a = p1 + p2 + p3 (+ at most 2^-24 |a|), round-to-nearest-even at every step
__device__ __forceinline__ void split3(float a, unsigned short &p1, unsigned short &p2, unsigned short &p3) {
    const __bf16 b1 = (__bf16)a;
    const float r1 = a - (float)b1;
    const __bf16 b2 = (__bf16)r1;
    const float r2 = r1 - (float)b2;
    const __bf16 b3 = (__bf16)r2;
    p1 = bf16_bits(b1);
    p2 = bf16_bits(b2);
    p3 = bf16_bits(b3);
}

__global__ __launch_bounds__(256) void k_split_pack(const float *__restrict__ Wt, int K, int N, int Npad,
                                                    unsigned short *__restrict__ out) {
    const int64_t total = (int64_t)K * Npad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i / Npad), n = (int)(i - (int64_t)k * Npad);
        unsigned short p[3] = {0, 0, 0};
        if (n < N) split3(Wt[(int64_t)k * N + n], p[0], p[1], p[2]);
        const int kt = k / kKT, kk = k - kt * kKT;
#pragma unroll
        for (int q = 0; q < 3; q++) out[(((int64_t)kt * 3 + q) * Npad + n) * kKT + kk] = p[q];
    }
}

template <int MI, int MODE>
__global__ __launch_bounds__(256, 3) void k_gemm_split(const Args a) {
    constexpr int BM = 32 * MI;
    __shared__ __attribute__((aligned(16))) unsigned short lds[3 * (BM + kBN) * kPitch];
    unsigned short *const ldsA = lds;
    unsigned short *const ldsW = lds + 3 * BM * kPitch;

    // blocks that follow each other on one XCD share the A row tile (its L2 holds it); bijective for any block count
    const int orig = blockIdx.x, xcd = orig & 7, q8 = a.n_blocks >> 3, r8 = a.n_blocks & 7;
    const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
    const int nt = lid % a.n_tiles_n, mt = lid / a.n_tiles_n;
    const int64_t m0 = (int64_t)mt * BM;
    const int n0 = nt * kBN;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // ---- staging geometry of this thread: rows r0 + 32 i, 4 consecutive k at 4 c4
    const int r0 = t >> 3, c4 = t & 7;
    // MODE 1 keeps an offset per row; the other two derive it from the first row's (rows 32 apart, a uniform step)
    int64_t rowoff[MODE == 1 ? MI : 1];
    int ryx[MODE == 2 ? MI : 1];          // MODE 2: y << 16 | x of the row's pixel
    const int64_t mrow0 = m0 + r0;
    rowoff[0] = (mrow0 < a.M ? mrow0 : 0) * a.lda;
    ryx[0] = 0;
#pragma unroll
    for (int i = 0; i < MI; i++) {
        const int64_t m = mrow0 + 32 * i;
        const int64_t mm = m < a.M ? m : 0;
        if (MODE == 1) {
            const int64_t b = mm / ((int64_t)a.g.Ho * a.g.Wo);
            const int rem = (int)(mm - b * (int64_t)a.g.Ho * a.g.Wo);
            const int yo = rem / a.g.Wo, xo = rem - yo * a.g.Wo;
            rowoff[MODE == 1 ? i : 0] = ((b * a.g.H + (int64_t)yo * a.g.s) * a.g.W + (int64_t)xo * a.g.s) * a.lda;
        } else if (MODE == 2) {
            ryx[MODE == 2 ? i : 0] = (int)((mm / a.g.W) % a.g.H) << 16 | (int)(mm % a.g.W);
        }
    }

    f32x4 ra[MI];
    u32x4 rw[6];
    unsigned okmask = 0;
    const u32x4 *const wbase = reinterpret_cast<const u32x4 *>(a.Wp) + (int64_t)n0 * 4 + t;

    auto gload = [&](int kt) {
        const int k0 = kt * kKT;
        int c0 = k0, dy = 0, dx = 0;
        int64_t toff = 0;
        if (MODE == 2) {
            const int tap = k0 / a.g.C;
            c0 = k0 - tap * a.g.C;
            dy = tap / 3 - 1;
            dx = tap - (tap / 3) * 3 - 1;
            toff = (int64_t)(dy * a.g.W + dx) * a.lda;
        }
        okmask = 0;
#pragma unroll
        for (int i = 0; i < MI; i++) {
            bool ok = mrow0 + 32 * i < a.M;
            if (MODE == 2) {
                const int yx = ryx[MODE == 2 ? i : 0];
                ok = ok && (unsigned)((yx >> 16) + dy) < (unsigned)a.g.H && (unsigned)((yx & 0xffff) + dx) < (unsigned)a.g.W;
            }
            const int64_t off = MODE == 1 ? rowoff[MODE == 1 ? i : 0] : rowoff[0] + (int64_t)(32 * i) * a.lda;
            // a masked row reads the first 16 bytes of A (always there) and is zeroed when it is written to LDS: a select
            // on the address, not a branch around the load
            const float *p = ok ? a.A + off + toff + c0 + c4 * 4 : a.A;
            ra[i] = *reinterpret_cast<const f32x4 *>(p);
            okmask |= (ok ? 1u : 0u) << i;
        }
        const u32x4 *wp = wbase + (int64_t)kt * 3 * a.Npad * 4;
#pragma unroll
        for (int p = 0; p < 3; p++) {
            rw[2 * p] = wp[(int64_t)p * a.Npad * 4];
            rw[2 * p + 1] = wp[(int64_t)p * a.Npad * 4 + 256];
        }
    };

    auto lwrite = [&]() {
#pragma unroll
        for (int i = 0; i < MI; i++) {
            const bool ok = (okmask >> i) & 1u;
            const f32x4 v = ok ? ra[i] : f32x4{0.f, 0.f, 0.f, 0.f};
            unsigned short p[3][4];
#pragma unroll
            for (int e = 0; e < 4; e++) split3(v[e], p[0][e], p[1][e], p[2][e]);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const u32x2 u = {(unsigned)p[q][0] | ((unsigned)p[q][1] << 16), (unsigned)p[q][2] | ((unsigned)p[q][3] << 16)};
                *reinterpret_cast<u32x2 *>(ldsA + (q * BM + r0 + 32 * i) * kPitch + c4 * 4) = u;
            }
        }
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int c = t + 256 * j;      // 16-byte chunk of the plane's tile: row c >> 2, 8 bf16 at 8 (c & 3)
                *reinterpret_cast<u32x4 *>(ldsW + (p * kBN + (c >> 2)) * kPitch + (c & 3) * 8) = rw[2 * p + j];
            }
    };

    // The running sum is kept by the vector ALU, not by the MFMA: the matrix pipe truncates when it adds into a large
    // accumulator (measured: the error of an MFMA-accumulated sum grew linearly with K, 1.3e-6 of max |D| at K = 2048
    // against 3e-7 for the fp32 library), so every K-tile's products are summed from zero and added here, rounded to nearest.
    f32x4 acc[MI][4];
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
        for (int ni = 0; ni < 4; ni++) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int frag = (lane & 15) * kPitch + (lane >> 4) * 8;
    const unsigned short *const fragA = ldsA + (wm * 16 * MI) * kPitch + frag;
    const unsigned short *const fragW = ldsW + (wn * 64) * kPitch + frag;

    const int n_kt = a.K / kKT;
    gload(0);
    lwrite();
    __syncthreads();
    for (int kt = 0; kt < n_kt; kt++) {
        const bool more = kt + 1 < n_kt;
        if (more) gload(kt + 1);
        bf16x8 bw[3][4];
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int ni = 0; ni < 4; ni++)
                bw[p][ni] = *reinterpret_cast<const bf16x8 *>(fragW + (p * kBN + ni * 16) * kPitch);
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mi = 0; mi < MI; mi++) {
            bf16x8 av[3];
#pragma unroll
            for (int p = 0; p < 3; p++) av[p] = *reinterpret_cast<const bf16x8 *>(fragA + (p * BM + mi * 16) * kPitch);
            // the MFMA's A operand is the W fragment (rows = output channels).  The sum of a K-tile starts from zero: the
            // five corrections, smallest first, then a1 w1 on top of them.
            f32x4 ts[4];
#pragma unroll
            for (int ni = 0; ni < 4; ni++) ts[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[2][ni], av[0], zero, 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < 4; ni++) ts[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[0][ni], av[2], ts[ni], 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < 4; ni++) ts[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[1][ni], av[1], ts[ni], 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < 4; ni++) ts[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[1][ni], av[0], ts[ni], 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < 4; ni++) ts[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[0][ni], av[1], ts[ni], 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < 4; ni++) ts[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[0][ni], av[0], ts[ni], 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < 4; ni++) acc[mi][ni] += ts[ni];
            __builtin_amdgcn_sched_barrier(0);      // one row fragment at a time: the temporaries of all of them do not fit
        }
        __syncthreads();            // every wave has read tile kt
        if (more) {
            lwrite();
            __syncthreads();
        }
    }

    // ---- epilogue: lane holds D[m][n .. n+3], m = tile row (lane & 15), n = 4 (lane >> 4) inside a 16 x 16 fragment
#pragma unroll
    for (int mi = 0; mi < MI; mi++) {
        const int64_t m = m0 + wm * 16 * MI + mi * 16 + (lane & 15);
        if (m >= a.M) continue;
#pragma unroll
        for (int ni = 0; ni < 4; ni++) {
            const int n = n0 + wn * 64 + ni * 16 + (lane >> 4) * 4;
            if (n >= a.N) continue;              // N is a multiple of 16 and n of 4: a whole float4 or nothing
            f32x4 v = acc[mi][ni];
            if (a.bias) {
                const float4 b = *reinterpret_cast<const float4 *>(a.bias + n);
                v += f32x4{b.x, b.y, b.z, b.w};
            }
            if (a.R) {
                const float4 r = *reinterpret_cast<const float4 *>(a.R + m * a.ldr + n);
                v += f32x4{r.x, r.y, r.z, r.w};
            }
            if (a.act) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
            *reinterpret_cast<float4 *>(a.D + m * a.ldd + n) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

template <int MODE>
int launch(Args &a, int tile, hipStream_t stream) {
    // tile 1: 64 x 128, 2: 32 x 128.  0: the wide one where its blocks fill the device's CUs twice over (a block is four
    // waves, one per SIMD); with fewer blocks the narrow tile's extra W traffic is the smaller loss (measured:
    // profiles/split_bf16_shapes.md -- 600 blocks of 64 rows win, 300 lose to 600 of 32)
    if (tile == 0) tile = ceil_div(a.M, 64) * a.n_tiles_n >= 2 * (int64_t)device_cu_count() ? 1 : 2;
    const int bm = tile == 1 ? 64 : 32;
    const int64_t blocks = ceil_div(a.M, bm) * a.n_tiles_n;
    DAGR_CHECK_ARG(blocks < ((int64_t)1 << 31), "too many tiles");
    a.n_blocks = (int)blocks;
    if (tile == 1)
        k_gemm_split<2, MODE><<<(unsigned)blocks, 256, 0, stream>>>(a);
    else
        k_gemm_split<1, MODE><<<(unsigned)blocks, 256, 0, stream>>>(a);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

inline int unsupported(const char *fn, const char *what) {
    set_error(std::string(fn) + ": " + what);
    return DAGR_ERR_UNSUPPORTED;
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" size_t dagr_gemm_split_bf16_packed_bytes(int32_t K, int32_t N) {
    if (K < kKT || K % kKT != 0 || N < 16 || N % 16 != 0) return 0;
    return (size_t)K * 3 * align_up((size_t)N, kBN) * sizeof(unsigned short);
}

extern "C" int dagr_gemm_split_bf16_pack(const float *Wt, int32_t K, int32_t N, void *packed, size_t packed_bytes,
                                         void *stream) {
    DAGR_CHECK_ARG(K >= 1 && N >= 1, "bad sizes");
    if (K % kKT != 0) return unsupported(__func__, "K is not a multiple of the K-tile (32)");
    if (N % 16 != 0) return unsupported(__func__, "N is not a multiple of 16");
    DAGR_CHECK_ARG(Wt && packed, "NULL pointer");
    DAGR_CHECK_ARG(aligned16(packed), "packed is not 16-byte aligned");
    DAGR_CHECK_ARG(packed_bytes >= dagr_gemm_split_bf16_packed_bytes(K, N), "packed buffer too small");
    const int Npad = (int)align_up((size_t)N, kBN);
    const int64_t blocks = std::min<int64_t>(ceil_div((int64_t)K * Npad, 256), 256 * 16);
    k_split_pack<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(Wt, K, N, Npad, (unsigned short *)packed);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

namespace {
int check_common(const char *fn, const float *A, int64_t M, int32_t K, int64_t lda, const void *packed, int32_t N,
                 const float *bias, const float *R, int64_t ldr, int32_t act, float *D, int64_t ldd, int32_t tile, bool &done) {
    done = true;
#define SPLIT_CHECK(cond, msg)                                     \
    do {                                                           \
        if (!(cond)) {                                             \
            set_error(std::string(fn) + ": " + (msg));             \
            return DAGR_ERR_INVALID_ARG;                           \
        }                                                          \
    } while (0)
    SPLIT_CHECK(M >= 0 && K >= 1 && N >= 1 && ldd >= N && (!R || ldr >= N) && (act == 0 || act == 1) && tile >= 0 && tile <= 2,
                "bad sizes");
    if (K % kKT != 0) return unsupported(fn, "K (C of a 3x3) is not a multiple of the K-tile (32)");
    if (N % 16 != 0) return unsupported(fn, "N is not a multiple of 16");
    if (M == 0) return DAGR_OK;
    SPLIT_CHECK(A && packed && D, "NULL pointer");
    SPLIT_CHECK((const float *)D != A, "D aliases A");
    SPLIT_CHECK((const float *)D != R, "D aliases R");
    SPLIT_CHECK(lda % 4 == 0 && ldd % 4 == 0 && (!R || ldr % 4 == 0), "row strides must be multiples of 4 floats");
    SPLIT_CHECK(aligned16(A) && aligned16(packed) && aligned16(D) && aligned16(bias) && aligned16(R),
                "pointers must be 16-byte aligned");
#undef SPLIT_CHECK
    done = false;
    return DAGR_OK;
}
}  // namespace

extern "C" int dagr_gemm_split_bf16(const float *A, int64_t M, int32_t K, int64_t lda, const void *packed, int32_t N,
                                    const float *bias, const float *R, int64_t ldr, int32_t act, float *D, int64_t ldd,
                                    int32_t B, int32_t H, int32_t W, int32_t stride, int32_t tile, void *stream) {
    bool done;
    const int rc = check_common(__func__, A, M, K, lda, packed, N, bias, R, ldr, act, D, ldd, tile, done);
    if (done) return rc;
    DAGR_CHECK_ARG(lda >= K && stride >= 1, "bad sizes");
    Args a{A, (const unsigned short *)packed, bias, R, D, M, lda, R ? ldr : 0, ldd, K, N, (int)align_up((size_t)N, kBN), act,
           (int)ceil_div(N, kBN), 0, Geo{0, 0, 0, K, 1, 0, 0}};
    if (stride == 1) return launch<0>(a, tile, (hipStream_t)stream);
    DAGR_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "bad image sizes");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    DAGR_CHECK_ARG(M == (int64_t)B * Ho * Wo, "M is not B * ceil(H / stride) * ceil(W / stride)");
    a.g = Geo{1, H, W, K, stride, Ho, Wo};
    return launch<1>(a, tile, (hipStream_t)stream);
}

extern "C" int dagr_conv3x3_split_bf16(const float *X, int32_t B, int32_t H, int32_t W, int32_t C, int64_t ldx,
                                       const void *packed, int32_t N, const float *bias, const float *R, int64_t ldr,
                                       int32_t act, float *D, int64_t ldd, int32_t tile, void *stream) {
    DAGR_CHECK_ARG(B >= 0 && H >= 1 && W >= 1 && C >= 1 && ldx >= C, "bad sizes");
    const int64_t M = (int64_t)B * H * W;
    bool done;
    const int rc = check_common(__func__, X, M, C, ldx, packed, N, bias, R, ldr, act, D, ldd, tile, done);
    if (done) return rc;
    DAGR_CHECK_ARG((int64_t)C * 9 < ((int64_t)1 << 31), "C too large");
    Args a{X, (const unsigned short *)packed, bias, R, D, M, ldx, R ? ldr : 0, ldd, 9 * C, N, (int)align_up((size_t)N, kBN), act,
           (int)ceil_div(N, kBN), 0, Geo{2, H, W, C, 1, H, W}};
    return launch<2>(a, tile, (hipStream_t)stream);
}
