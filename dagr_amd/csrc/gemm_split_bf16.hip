// gemm_split_bf16.hip -- fp32-accurate GEMM / implicit-GEMM 3x3 convolution on the bf16 matrix pipe.
//
// The image branch's trunk (net_img.py:42-48, BatchNorm folded) is fp32 GEMM work, and the fp32-input MFMA runs at 1/16 of
// the bf16 MFMA rate on gfx950.  An fp32 product is rebuilt from bf16 pieces instead: every operand is written as the sum of
// three bf16 values (3 x 8 mantissa bits, fp32's exponent range),
//     a = a1 + a2 + a3,   a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2)      (both subtractions are exact)
// and the six products of order up to 2^-16 are kept: a1w1, a1w2, a2w1, a2w2, a1w3, a3w1.  Each of the three dropped ones
// is at most 2^-24 relative.  Per K-slice of 32 the six products are summed by a chain of six MFMAs that starts from zero
// (corrections first, a1w1 last), and the vector ALU adds the slice's sum to the running fp32 sum.
//
//   D[M, N] = act(A . W + bias (+ R)),  fp32 in memory on both sides, no split-K, no atomics: same operands, same bits.
// K is not split in any form (neither across workgroups nor inside one): the shapes with few rows and a long K get more
// workgroups from the narrower tiles below, and the K-slices are added in ascending order whatever the tile.
//
// Weights are packed once (dagr_gemm_split_bf16_pack) into three bf16 planes, K-slice major: [K/32][3][Npad][32] with Npad =
// N rounded up to 128 columns (zero filled).  The packed planes ARE the LDS image of a W tile: a row is 64 bytes, its four
// 16-byte k-chunks stored in the swizzled order of swz() below, so a tile of BN columns of one plane is BN * 64 contiguous
// bytes and goes global -> LDS by the LDS-direct load (1 KB per wave instruction, no register in between, no ds_write).
// The layout is opaque to callers: dagr_gemm_split_bf16_packed_bytes sizes the buffer and nothing else reads it.
// Activations stay fp32: the A tile is loaded to registers, split there, and written to LDS as three planes with the same
// swizzle.
//
// Tile: (32*MI) x BN x 32, MI = 2 or 1, BN = 128 or 64 (N = 64 on a 128-column tile multiplies zero padding in half of every
// MFMA; a 128-row tile lost to the 64-row one on every shape of the image branch); 4 waves as 2 x 2, each (16*MI) x (BN/2)
// of the output; mfma_f32_16x16x32_bf16 with the operands swapped (W as the MFMA's A operand), so a lane ends up with four
// consecutive output CHANNELS of one row and the epilogue reads bias / residual and writes D as float4.
// The 64 x 128 tile also runs on 8 waves as 2 x 4, each 32 x 32 of the output (WN = 4): a thread then splits one float4 of A
// per slice instead of two and a wave brings in three W pieces instead of six, for the same 24 MFMAs a wave issues on the
// 64 x 64 tile.  That is the split per MFMA of the 128-column tile (a block splits its A rows once per 128 columns, not
// once per 64) inside the register budget of the 64-column one: 128 VGPRs, so two blocks, sixteen waves, per CU.  It is
// what tile 0 picks for the 1x1 shapes with K <= 512 that fill the chip with such blocks (launch() below).
// A three-stage loop (W image sent for two slices ahead, counted vmcnt, the A loads hidden from the compiler's wait counting)
// was built and measured beside it (profiles/split_bf16_loop.md): a wave waited less, but three stages cost a block per CU
// (73 728 B at 64 x 64) and every shape of the trunk ran 3 - 21 % slower; it is not kept.
//
// K loop: two LDS stages and one workgroup barrier per slice.  While slice kt is multiplied out of one stage, the W image of
// slice kt + 1 arrives in the other by the LDS-direct load, the A rows of slice kt + 1 (in registers since slice kt - 1) are
// split between the MFMAs and written there too, and the A rows of slice kt + 2 are on their way to a second register set.
// The barrier is a raw s_barrier behind one s_waitcnt: everything a slice sends for was issued at its top.
//
// A-row addressing (Geo): plain rows with a pitch; a 1x1 convolution with spatial stride (reads every s-th pixel in place);
// a 3x3 / stride 1 / pad 1 convolution on an NHWC map, K = (tap, channel) -- a K-slice lies inside one tap because C is a
// multiple of 32, taps outside the image (which also closes the seam between two images of the batch) read as zero.
//
// Nothing of the addressing is vector work inside the K loop (profiles/split_bf16_addressing.md).  The A view and the packed
// planes each sit behind one buffer descriptor.  A lane's byte offset of each of its rows is computed once in front of the
// loop; what a slice adds to it is the same for every lane and travels as the load's scalar offset: k0 for the 1x1 forms, the
// tap's pixel offset and the channel for the 3x3, kept as counters that step by 32 channels (no division by C).  A row that
// must read as zero -- beyond M, or for the 3x3 a tap outside the image -- has an offset of 2^31 (or that bit set), past the
// descriptor's extent, and the range check of the load returns zeros: there is no select on the address and none on the
// values.  The 3x3 keeps nine validity bits per row, computed once, and spends two vector instructions per row and slice to
// move the current tap's bit to bit 31 of the offset; its descriptor starts W + 1 pixels in front of the map, so every tap's
// scalar offset is non-negative (nothing is read in front of the map: those taps are masked).  The W pieces take the fixed
// 16 lane as their offset and the piece's place as a scalar offset there and M0 here; the wave index comes through
// readfirstlane so that the compiler knows it uniform.  That is why the entry points refuse an A view (or packed planes) of
// 2^31 bytes or more: offsets are 32 bits, and a masked offset plus any slice's scalar offset must stay below 2^32.
// Steady-state loop, vector instructions other than MFMA per two slices: 96 on 64 x 64 (142 before), 61 on the eight-wave
// tile (92), 98 on the 64 x 64 3x3 (188); the MFMA / VALU interleave is fitted to those counts (interleave<>()).
#include <algorithm>
#include <type_traits>

#include "common.hpp"

namespace dagr {
namespace {

constexpr int kKT = 32;        // K-slice
constexpr int kNPad = 128;     // the packed planes pad N to this many columns (the widest tile)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct Geo {
    int mode;                  // 0: rows, 1: 1x1 with spatial stride, 2: 3x3 stride 1 pad 1
    int H, W, C, s, Ho, Wo;
};

struct Args {
    const float *A;            // base of the A descriptor: the first element of the view (MODE 2: W + 1 pixels in front of it)
    const unsigned short *Wp;
    const float *bias, *R;
    float *D;
    int64_t M, lda, ldr, ldd;
    int K, N, Npad, act, n_tiles_n, n_blocks;
    unsigned a_bytes, w_bytes; // extents of the two descriptors (num_records)
    Geo g;
};

// A lane's byte offset of a row that must read as zero: past every descriptor extent (those are below 2^31, view_bytes()
// below), and still below 2^32 with any scalar offset of a slice added to it, so the sum does not wrap back into range.
constexpr unsigned kMasked = 0x80000000u;
// descriptor word 3 of a raw (unstructured, 32-bit data) buffer on gfx9
constexpr int kRsrcFlags = 0x00020000;

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

// The same split of two values at once, each piece as the pair's two bf16 in one dword (element 0 low): one packed
// conversion per piece, and the dword is what the LDS planes hold.  Same roundings, same bits as split3.
__device__ __forceinline__ void split3x2(float a0, float a1, unsigned &p1, unsigned &p2, unsigned &p3) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    auto widen = [](unsigned u) {
        return f32x2{__builtin_bit_cast(float, u << 16), __builtin_bit_cast(float, u & 0xffff0000u)};
    };
    const f32x2 v = {a0, a1};
    p1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    const f32x2 r1 = v - widen(p1);
    p2 = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2));
    const f32x2 r2 = r1 - widen(p2);
    p3 = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
}

// Position (in bf16) of the 8-element k-chunk `c` (0..3) of row `r` in a plane of 64-byte rows.  A fragment read takes row
// lane & 15, chunk lane >> 4 with ds_read_b128, whose four lane groups are {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and
// the same + 32: a group holds all sixteen rows, rows 4..11 at one chunk and rows 0..3, 12..15 at another.  Four rows share
// a 256-byte bank row, so rows r, r + 4, r + 8, r + 12 of a group must sit at four different chunk positions: chunks of rows
// 8..15 are stored at c ^ 3 (group 0: rows 0, 4, 8, 12 at 0, 1, 1 ^ 3, 0 ^ 3 -- all four; the other groups are this one
// XOR a constant).
__device__ __forceinline__ int swz(int r, int c) { return r * kKT + ((c ^ (((r >> 3) & 1) * 3)) << 3); }

__global__ __launch_bounds__(256) void k_split_pack(const float *__restrict__ Wt, int K, int N, int Npad,
                                                    unsigned short *__restrict__ out) {
    const int64_t total = (int64_t)K * Npad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i / Npad), n = (int)(i - (int64_t)k * Npad);
        unsigned short p[3] = {0, 0, 0};
        if (n < N) split3(Wt[(int64_t)k * N + n], p[0], p[1], p[2]);
        const int kt = k / kKT, kk = k - kt * kKT;
#pragma unroll
        for (int q = 0; q < 3; q++) out[((int64_t)kt * 3 + q) * Npad * kKT + swz(n, kk >> 3) + (kk & 7)] = p[q];
    }
}

// Waits for everything this wave has in flight (the A rows on their way to registers, its pieces of the W image on their
// way to LDS, its LDS stores), then the workgroup barrier.  The A registers pass through the statement, so the compiler
// sees them as ready from here on and puts no wait of its own in the middle of the next slice.
template <int N>
__device__ __forceinline__ void wait_all_barrier(f32x4 (&ra)[2][N]) {
    if constexpr (N == 1)
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(ra[0][0]), "+v"(ra[1][0])::"memory");
    else
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(ra[0][0]), "+v"(ra[0][1]), "+v"(ra[1][0]), "+v"(ra[1][1])::"memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// One MFMA, then its share of the slice's V vector instructions, N times: V / N of them on average, placed as evenly as whole
// numbers allow (the sizes of sched_group_barrier are compile-time constants).
template <int I, int N, int V>
__device__ __forceinline__ void interleave() {
    if constexpr (I < N) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        constexpr int n = (I + 1) * V / N - I * V / N;
        if constexpr (n > 0) __builtin_amdgcn_sched_group_barrier(0x002, n, 0);
        interleave<I + 1, N, V>();
    }
}

// Waves per SIMD that the registers are budgeted for (the second argument of __launch_bounds__).  Four waves: 2 with 128
// columns, 3 with 64.  Eight waves on 64 x 128: two blocks of 73 728 B of LDS fit in a CU, sixteen waves, 4 per SIMD, so
// 128 registers.
constexpr int waves_per_simd(int BN, int WN) { return WN == 4 ? 4 : BN == 128 ? 2 : 3; }

// WN: waves along N (2 x WN waves per block, 128 WN threads).
template <int MI, int BN, int MODE, int WN = 2>
__global__ __launch_bounds__(128 * WN, waves_per_simd(BN, WN)) void k_gemm_split(const Args a) {
    constexpr int BM = 32 * MI;
    constexpr int NT = 128 * WN;                     // threads
    constexpr int NI = BN / (16 * WN);               // 16-column fragments of a wave
    constexpr int AI = BM * 8 / NT;                  // float4 of the A tile that a thread stages per slice
    constexpr int kStage = 3 * (BM + BN) * kKT;      // one stage: three A planes, then three W planes (bf16)
    constexpr int kPieces = 3 * BN / 16 / (2 * WN);  // 1 KB pieces of a stage's W image that each wave brings in
    static_assert(AI >= 1 && AI * NT == BM * 8 && kPieces * 2 * WN * 16 == 3 * BN && NI >= 1, "tile does not divide among the waves");
    __shared__ __attribute__((aligned(1024))) unsigned short lds[2 * kStage];

    // blocks that follow each other on one XCD share the A row tile (its L2 holds it); bijective for any block count
    const int orig = blockIdx.x, xcd = orig & 7, q8 = a.n_blocks >> 3, r8 = a.n_blocks & 7;
    const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
    const int nt = lid % a.n_tiles_n, mt = lid / a.n_tiles_n;
    const int64_t m0 = (int64_t)mt * BM;
    const int n0 = nt * BN;

    // the wave index through readfirstlane: uniform to the compiler as well, so what hangs on it (the W pieces' source
    // and LDS addresses, M0) is scalar arithmetic
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // ---- staging geometry of this thread: rows r0 + kRS i, 4 consecutive k at 4 c4
    // Every A row comes through one buffer descriptor over the whole view.  A lane's byte offset of row i (voff) is
    // computed here, once; what a K-slice adds (its k0, for MODE 2 its tap and channel) is the same for all lanes and
    // goes into the load's scalar offset.  A row beyond M has the offset kMasked, which the descriptor's range check
    // answers with zeros: no select on the address, none on the values.
    constexpr int kRS = NT / 8;           // rows that the block's threads cover at once
    const int r0 = t >> 3, c4 = t & 7;
    unsigned voff[AI];
    unsigned tapout[MODE == 2 ? AI : 1];  // MODE 2: bit `tap` set where that tap of the row's pixel is outside the image
    tapout[0] = 0;
    const int64_t mrow0 = m0 + r0;
#pragma unroll
    for (int i = 0; i < AI; i++) {
        const int64_t m = mrow0 + kRS * i;
        const bool ok = m < a.M;
        const int64_t mm = ok ? m : 0;
        int64_t pix = mm;
        if (MODE == 1) {
            const int64_t b = mm / ((int64_t)a.g.Ho * a.g.Wo);
            const int rem = (int)(mm - b * (int64_t)a.g.Ho * a.g.Wo);
            const int yo = rem / a.g.Wo, xo = rem - yo * a.g.Wo;
            pix = (b * a.g.H + (int64_t)yo * a.g.s) * a.g.W + (int64_t)xo * a.g.s;
        } else if (MODE == 2) {
            const int y = (int)((mm / a.g.W) % a.g.H), x = (int)(mm % a.g.W);
            unsigned out = 0;
#pragma unroll
            for (int tap = 0; tap < 9; tap++) {
                const int dy = tap / 3 - 1, dx = tap % 3 - 1;
                const bool in = ok && (unsigned)(y + dy) < (unsigned)a.g.H && (unsigned)(x + dx) < (unsigned)a.g.W;
                out |= (in ? 0u : 1u) << tap;
            }
            tapout[MODE == 2 ? i : 0] = out;
        }
        voff[i] = ok ? (unsigned)(pix * a.lda * 4 + c4 * 16) : MODE == 2 ? 0u : kMasked;
    }
    const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.A), 0, (int)a.a_bytes, kRsrcFlags);

    static_assert(AI == 1 || AI == 2, "wait_all_barrier names the register sets");
    f32x4 ra[2][AI];                   // two register sets: slice kt + 1 is split out of one while kt + 2 arrives in the other

    // MODE 2: where the next slice to send for lies, kept as counters (a slice lies inside one tap: C is a multiple of 32).
    // The descriptor's base is W + 1 pixels in front of the map, so the tap (ty, tx) = (dy + 1, dx + 1) adds the
    // non-negative (ty W + tx) pixels; nothing is read in front of the map, because those taps are masked.
    const int n_kt = a.K / kKT;
    int nx_kt = 0, nx_c0 = 0, nx_tx = 0;
    unsigned nx_tapoff = 0, nx_shift = 31;            // byte offset of the tap; 31 - tap
    const unsigned pix_bytes = (unsigned)a.lda * 4u;

    // the A rows of the next K-slice (MODE 0 / 1: of slice kt), fp32, into register set `set`
    auto gload = [&](auto set, int kt) {
        constexpr int S = decltype(set)::value;
        unsigned soff = (unsigned)kt * (kKT * 4);
        if (MODE == 2) soff = nx_tapoff + (unsigned)nx_c0 * 4u;
#pragma unroll
        for (int i = 0; i < AI; i++) {
            unsigned v = voff[i];
            // the tap's bit to bit 31: a pixel whose tap is outside the image reads at kMasked | offset
            if (MODE == 2) v |= (tapout[MODE == 2 ? i : 0] << nx_shift) & kMasked;
            ra[S][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(arsrc, (int)v, (int)soff, 0));
        }
        if (MODE == 2) {
            // step to the slice behind it, all in scalar selects; the last slice stays (it is sent for again past the end
            // and never used)
            const bool more = nx_kt + 1 < n_kt;
            const bool tapstep = more && nx_c0 + kKT == a.g.C;
            const bool rowstep = tapstep && nx_tx == 2;
            nx_kt += more ? 1 : 0;
            nx_c0 = tapstep ? 0 : more ? nx_c0 + kKT : nx_c0;
            nx_shift -= tapstep ? 1u : 0u;
            nx_tapoff += rowstep ? (unsigned)(a.g.W - 2) * pix_bytes : tapstep ? pix_bytes : 0u;
            nx_tx = rowstep ? 0 : tapstep ? nx_tx + 1 : nx_tx;
        }
    };

    // register set `set`, split into three planes, into stage s
    auto lwrite = [&](auto set, int s) {
        constexpr int S = decltype(set)::value;
        unsigned short *const ldsA = lds + s * kStage;
#pragma unroll
        for (int i = 0; i < AI; i++) {
            const f32x4 v = ra[S][i];
            unsigned lo[3], hi[3];
            split3x2(v[0], v[1], lo[0], lo[1], lo[2]);
            split3x2(v[2], v[3], hi[0], hi[1], hi[2]);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const u32x2 u = {lo[q], hi[q]};
                *reinterpret_cast<u32x2 *>(ldsA + q * BM * kKT + swz(r0 + kRS * i, c4 >> 1) + (c4 & 1) * 4) = u;
            }
        }
    };

    // The W image of K-slice kt, global -> LDS with no register in between.  The packed planes already are the LDS image,
    // so every piece is 1 KB contiguous on both sides: through a descriptor over the packed planes the lane's part is the
    // fixed 16 lane on both sides, and the piece's place is a scalar offset there and M0 here.
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(a.Wp), 0, (int)a.w_bytes, kRsrcFlags);
    const int wlane = lane * 16;
    auto wload = [&](int kt, int s) {
#pragma unroll
        for (int j = 0; j < kPieces; j++) {
            const int piece = wave * kPieces + j, p = piece / (BN / 16), sub = piece - p * (BN / 16);
            const unsigned soff = (unsigned)(((kt * 3 + p) * a.Npad + n0 + sub * 16) * (kKT * 2));
            unsigned short *dst = lds + s * kStage + (3 * BM + p * BN + sub * 16) * kKT;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc, (__attribute__((address_space(3))) void *)dst, 16, wlane, (int)soff, 0, 0);
        }
    };

    // The running sum is kept by the vector ALU, not by the MFMA: the matrix pipe truncates when it adds into a large
    // accumulator (measured: the error of an MFMA-accumulated sum grew linearly with K, 1.3e-6 of max |D| at K = 2048
    // against 3e-7 for the fp32 library), so every K-slice's products are summed from zero and added here, rounded to nearest.
    f32x4 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
        for (int ni = 0; ni < NI; ni++) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int frag = swz(lane & 15, lane >> 4);
    const int fragA = (wm * 16 * MI) * kKT + frag;
    const int fragW = (3 * BM + wn * (BN / WN)) * kKT + frag;

    // Two LDS stages, one barrier per slice.  Slice kt is multiplied out of stage kt & 1.  At the top of that slice the
    // A rows of slice kt + 2 are sent for (into the register set slice kt was split from) and so is the W image of slice
    // kt + 1 (LDS-direct, into the other stage); between the MFMAs the vector ALU splits slice kt + 1, which arrived during
    // slice kt - 1, and writes it to the other stage.  Everything a slice sends for has the whole slice to arrive, and the
    // one wait in front of the barrier retires it.
    const std::integral_constant<int, 0> set0;
    const std::integral_constant<int, 1> set1;

    // the six-MFMA chains of one slice out of `st`, added to the running sums
    auto multiply = [&](const unsigned short *st) {
        bf16x8 bw[3][NI], av[MI][3];
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int ni = 0; ni < NI; ni++)
                bw[p][ni] = *reinterpret_cast<const bf16x8 *>(st + fragW + (p * BN + ni * 16) * kKT);
#pragma unroll
        for (int mi = 0; mi < MI; mi++)
#pragma unroll
            for (int p = 0; p < 3; p++) av[mi][p] = *reinterpret_cast<const bf16x8 *>(st + fragA + (p * BM + mi * 16) * kKT);
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mi = 0; mi < MI; mi++) {
            // the MFMA's A operand is the W fragment (rows = output channels).  The sum of a K-slice starts from zero: the
            // five corrections, smallest first, then a1 w1 on top of them.
            f32x4 ts[NI];
#pragma unroll
            for (int ni = 0; ni < NI; ni++) ts[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[2][ni], av[mi][0], zero, 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < NI; ni++) ts[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[0][ni], av[mi][2], ts[ni], 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < NI; ni++) ts[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[1][ni], av[mi][1], ts[ni], 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < NI; ni++) ts[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[1][ni], av[mi][0], ts[ni], 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < NI; ni++) ts[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[0][ni], av[mi][1], ts[ni], 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < NI; ni++) ts[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[0][ni], av[mi][0], ts[ni], 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < NI; ni++) acc[mi][ni] += ts[ni];
        }
    };

    // slice kt with a slice behind it (one basic block: no branch between the loads, the MFMAs and the split)
    auto slice = [&](auto cur, auto nxt, int kt) {
        constexpr int S = decltype(cur)::value;
        gload(cur, kt + 2 < n_kt ? kt + 2 : n_kt - 1);      // past the end: the last slice again, never used
        wload(kt + 1, S ^ 1);
        __builtin_amdgcn_sched_barrier(0);                  // both kinds of load go out before anything else of the slice
        multiply(lds + S * kStage);
        lwrite(nxt, S ^ 1);
        // spread the slice's vector instructions evenly between its MFMAs (an MFMA occupies the matrix pipe for four issue
        // slots).  Per slice: 20 for the split of a float4, 2 for a fragment's add to the running sum, and in MODE 2 two per
        // row for the tap's mask and one select of the tap counters -- what the cross-compiled loop holds
        // (profiles/split_bf16_addressing.md).
        interleave<0, 6 * MI * NI, 20 * AI + 2 * MI * NI + (MODE == 2 ? 2 * AI + 1 : 0)>();
        wait_all_barrier(ra);
    };

    gload(set0, 0);
    gload(set1, n_kt > 1 ? 1 : 0);
    wload(0, 0);
    lwrite(set0, 0);
    wait_all_barrier(ra);
    int kt = 0;
    for (; kt + 2 < n_kt; kt += 2) {
        slice(set0, set1, kt);
        slice(set1, set0, kt + 1);
    }
    if (kt + 1 < n_kt) {
        slice(set0, set1, kt);
        kt++;
    }
    multiply(lds + (kt & 1) * kStage);           // the last slice: nothing left to bring in

    // ---- epilogue: lane holds D[m][n .. n+3], m = tile row (lane & 15), n = 4 (lane >> 4) inside a 16 x 16 fragment
#pragma unroll
    for (int mi = 0; mi < MI; mi++) {
        const int64_t m = m0 + wm * 16 * MI + mi * 16 + (lane & 15);
        if (m >= a.M) continue;
#pragma unroll
        for (int ni = 0; ni < NI; ni++) {
            const int n = n0 + wn * (BN / WN) + ni * 16 + (lane >> 4) * 4;
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

template <int MI, int BN, int MODE, int WN = 2>
int launch_tile(Args &a, hipStream_t stream) {
    a.n_tiles_n = (int)ceil_div(a.N, BN);
    const int64_t blocks = ceil_div(a.M, 32 * MI) * a.n_tiles_n;
    DAGR_CHECK_ARG(blocks < ((int64_t)1 << 31), "too many tiles");
    a.n_blocks = (int)blocks;
    k_gemm_split<MI, BN, MODE, WN><<<(unsigned)blocks, 128 * WN, 0, stream>>>(a);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

template <int MODE>
int launch(Args &a, int variant, hipStream_t stream) {
    // Variants 1 - 4 are the tile codes of the first two entry points, on four waves: 1: 64 x 128, 2: 32 x 128, 3: 64 x 64,
    // 4: 32 x 64 (rows x columns); 5: 64 x 128 on eight waves.  0 picks from the shape, by what
    // profiles/split_bf16_shapes.md and profiles/split_bf16_loop.md measured.
    // Four waves, columns: always 64 -- three blocks per CU instead of two and no zero padding
    // at N = 64; it won or tied (within the spread) on every shape the rule selects, and the step as a whole was faster with
    // it than with 128 columns on the three shapes where those were 0.5 - 0.9 us ahead.  Rows: 64 where that still leaves
    // two blocks per CU, 32 below.  The 64 x 128 tile on eight waves beat the 64 x 64 tile by more than both spreads on
    // every 1x1 shape measured with K <= 512, whole 128-column tiles and at least four of its blocks per CU (1 200 -
    // 4 800 blocks; 7 - 13 % faster, plain and strided), and lost or tied on every shape with fewer blocks (608 and
    // below), with K >= 1024, with N = 64, and on the 3x3 convolutions.
    if (variant == 0) {
        const int64_t cus = device_cu_count();
        if (MODE != 2 && a.K <= 512 && a.N % 128 == 0 && ceil_div(a.M, 64) * (a.N / 128) >= 4 * cus)
            variant = DAGR_SPLIT_64X128_W8;
        else
            variant = ceil_div(a.M, 64) * ceil_div(a.N, 64) >= 2 * cus ? DAGR_SPLIT_64X64 : DAGR_SPLIT_32X64;
    }
    switch (variant) {
        case DAGR_SPLIT_64X128: return launch_tile<2, 128, MODE>(a, stream);
        case DAGR_SPLIT_32X128: return launch_tile<1, 128, MODE>(a, stream);
        case DAGR_SPLIT_64X64: return launch_tile<2, 64, MODE>(a, stream);
        case DAGR_SPLIT_32X64: return launch_tile<1, 64, MODE>(a, stream);
        case DAGR_SPLIT_64X128_W8: return launch_tile<2, 128, MODE, 4>(a, stream);
    }
    set_error("split-bf16 GEMM: unknown variant");   // (the entry points check the range first)
    return DAGR_ERR_INVALID_ARG;
}

inline int unsupported(const char *fn, const char *what) {
    set_error(std::string(fn) + ": " + what);
    return DAGR_ERR_UNSUPPORTED;
}

// Bytes from the first element of an A view of `rows` rows of K floats, `ld` floats apart, to the end of its last row, with
// `front` more rows in front of it; -1 where that is 2^31 or more.  The kernel addresses the view through one buffer
// descriptor with 32-bit offsets, and a masked row is the offset 2^31 (kMasked).
inline int64_t view_bytes(int64_t rows, int64_t ld, int64_t K, int64_t front) {
    const int64_t lim = (int64_t)1 << 31;
    if (rows - 1 + front >= lim || ld >= lim) return -1;
    const int64_t bytes = ((rows - 1 + front) * ld + K) * 4;       // below 2^64 / 4: no overflow
    return bytes < lim ? bytes : -1;
}
constexpr const char *kViewTooLarge = "the A view spans 2^31 bytes or more (the kernel addresses it with 32-bit offsets)";

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" size_t dagr_gemm_split_bf16_packed_bytes(int32_t K, int32_t N) {
    if (K < kKT || K % kKT != 0 || N < 16 || N % 16 != 0) return 0;
    return (size_t)K * 3 * align_up((size_t)N, kNPad) * sizeof(unsigned short);
}

extern "C" int dagr_gemm_split_bf16_pack(const float *Wt, int32_t K, int32_t N, void *packed, size_t packed_bytes,
                                         void *stream) {
    DAGR_CHECK_ARG(K >= 1 && N >= 1, "bad sizes");
    if (K % kKT != 0) return unsupported(__func__, "K is not a multiple of the K-tile (32)");
    if (N % 16 != 0) return unsupported(__func__, "N is not a multiple of 16");
    DAGR_CHECK_ARG(Wt && packed, "NULL pointer");
    DAGR_CHECK_ARG(aligned16(packed), "packed is not 16-byte aligned");
    DAGR_CHECK_ARG(packed_bytes >= dagr_gemm_split_bf16_packed_bytes(K, N), "packed buffer too small");
    const int Npad = (int)align_up((size_t)N, kNPad);
    const int64_t blocks = std::min<int64_t>(ceil_div((int64_t)K * Npad, 256), 256 * 16);
    k_split_pack<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(Wt, K, N, Npad, (unsigned short *)packed);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

namespace {
#define SPLIT_CHECK(cond, msg)                                     \
    do {                                                           \
        if (!(cond)) {                                             \
            set_error(std::string(fn) + ": " + (msg));             \
            return DAGR_ERR_INVALID_ARG;                           \
        }                                                          \
    } while (0)

// `code`: the tile of the first two entry points (max_code 4) or the variant of the other two (DAGR_SPLIT_VARIANT_LAST)
int check_common(const char *fn, const float *A, int64_t M, int32_t K, int64_t lda, const void *packed, int32_t N,
                 const float *bias, const float *R, int64_t ldr, int32_t act, float *D, int64_t ldd, int32_t code,
                 int32_t max_code, bool &done) {
    done = true;
    SPLIT_CHECK(M >= 0 && K >= 1 && N >= 1 && ldd >= N && (!R || ldr >= N) && (act == 0 || act == 1) && code >= 0 &&
                    code <= max_code,
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
    done = false;
    return DAGR_OK;
}

int gemm_entry(const char *fn, const float *A, int64_t M, int32_t K, int64_t lda, const void *packed, int32_t N,
               const float *bias, const float *R, int64_t ldr, int32_t act, float *D, int64_t ldd, int32_t B, int32_t H,
               int32_t W, int32_t stride, int32_t code, int32_t max_code, void *stream) {
    bool done;
    const int rc = check_common(fn, A, M, K, lda, packed, N, bias, R, ldr, act, D, ldd, code, max_code, done);
    if (done) return rc;
    SPLIT_CHECK(lda >= K && stride >= 1, "bad sizes");
    const size_t wbytes = dagr_gemm_split_bf16_packed_bytes(K, N);
    if (wbytes >= ((size_t)1 << 31)) return unsupported(fn, "the packed weights span 2^31 bytes or more");
    Args a{A, (const unsigned short *)packed, bias, R, D, M, lda, R ? ldr : 0, ldd, K, N, (int)align_up((size_t)N, kNPad), act,
           0, 0, 0, (unsigned)wbytes, Geo{0, 0, 0, K, 1, 0, 0}};
    int64_t rows = M;                                  // rows of the view that is read
    if (stride != 1) {
        SPLIT_CHECK(B >= 1 && H >= 1 && W >= 1, "bad image sizes");
        const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
        SPLIT_CHECK(M == (int64_t)B * Ho * Wo, "M is not B * ceil(H / stride) * ceil(W / stride)");
        a.g = Geo{1, H, W, K, stride, Ho, Wo};
        rows = (int64_t)B * H * W;
    }
    const int64_t abytes = view_bytes(rows, lda, K, 0);
    if (abytes < 0) return unsupported(fn, kViewTooLarge);
    a.a_bytes = (unsigned)abytes;
    return stride == 1 ? launch<0>(a, code, (hipStream_t)stream) : launch<1>(a, code, (hipStream_t)stream);
}

int conv3x3_entry(const char *fn, const float *X, int32_t B, int32_t H, int32_t W, int32_t C, int64_t ldx, const void *packed,
                  int32_t N, const float *bias, const float *R, int64_t ldr, int32_t act, float *D, int64_t ldd, int32_t code,
                  int32_t max_code, void *stream) {
    SPLIT_CHECK(B >= 0 && H >= 1 && W >= 1 && C >= 1 && ldx >= C, "bad sizes");
    const int64_t M = (int64_t)B * H * W;
    bool done;
    const int rc = check_common(fn, X, M, C, ldx, packed, N, bias, R, ldr, act, D, ldd, code, max_code, done);
    if (done) return rc;
    SPLIT_CHECK((int64_t)C * 9 < ((int64_t)1 << 31), "C too large");
    const size_t wbytes = dagr_gemm_split_bf16_packed_bytes(9 * C, N);
    if (wbytes >= ((size_t)1 << 31)) return unsupported(fn, "the packed weights span 2^31 bytes or more");
    // the descriptor starts W + 1 pixels in front of the map (the tap (-1, -1) of its first pixel), so its extent has them too
    const int64_t abytes = view_bytes(M, ldx, C, (int64_t)W + 1);
    if (abytes < 0) return unsupported(fn, kViewTooLarge);
    Args a{X - ((int64_t)W + 1) * ldx, (const unsigned short *)packed, bias, R, D, M, ldx, R ? ldr : 0, ldd, 9 * C, N,
           (int)align_up((size_t)N, kNPad), act, 0, 0, (unsigned)abytes, (unsigned)wbytes, Geo{2, H, W, C, 1, H, W}};
    return launch<2>(a, code, (hipStream_t)stream);
}
#undef SPLIT_CHECK
}  // namespace

extern "C" int dagr_gemm_split_bf16(const float *A, int64_t M, int32_t K, int64_t lda, const void *packed, int32_t N,
                                    const float *bias, const float *R, int64_t ldr, int32_t act, float *D, int64_t ldd,
                                    int32_t B, int32_t H, int32_t W, int32_t stride, int32_t tile, void *stream) {
    return gemm_entry(__func__, A, M, K, lda, packed, N, bias, R, ldr, act, D, ldd, B, H, W, stride, tile, 4, stream);
}

extern "C" int dagr_conv3x3_split_bf16(const float *X, int32_t B, int32_t H, int32_t W, int32_t C, int64_t ldx,
                                       const void *packed, int32_t N, const float *bias, const float *R, int64_t ldr,
                                       int32_t act, float *D, int64_t ldd, int32_t tile, void *stream) {
    return conv3x3_entry(__func__, X, B, H, W, C, ldx, packed, N, bias, R, ldr, act, D, ldd, tile, 4, stream);
}

extern "C" int dagr_gemm_split_bf16_variant(const float *A, int64_t M, int32_t K, int64_t lda, const void *packed, int32_t N,
                                            const float *bias, const float *R, int64_t ldr, int32_t act, float *D,
                                            int64_t ldd, int32_t B, int32_t H, int32_t W, int32_t stride, int32_t variant,
                                            void *stream) {
    return gemm_entry(__func__, A, M, K, lda, packed, N, bias, R, ldr, act, D, ldd, B, H, W, stride, variant,
                      DAGR_SPLIT_VARIANT_LAST, stream);
}

extern "C" int dagr_conv3x3_split_bf16_variant(const float *X, int32_t B, int32_t H, int32_t W, int32_t C, int64_t ldx,
                                               const void *packed, int32_t N, const float *bias, const float *R,
                                               int64_t ldr, int32_t act, float *D, int64_t ldd, int32_t variant,
                                               void *stream) {
    return conv3x3_entry(__func__, X, B, H, W, C, ldx, packed, N, bias, R, ldr, act, D, ldd, variant,
                         DAGR_SPLIT_VARIANT_LAST, stream);
}
