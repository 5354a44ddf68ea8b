// stream_decode.hip -- the event stream's decoder (dagr_stream_decode): EVT 3.0 (16-bit) and EVT 2.0 (32-bit) camera words
// into (x, y) / t / p / lane rows on the device, in front of dagr_stream_denoise / dagr_stream_downsample / the stage.
// dagr_amd/streaming.py states the formats and DecodeDefinition is the sequential loop; this file repeats it bit for bit.
//
// The loop is a scan.  What a run of words does to a lane's state is an Elem: the time-high part (first and last TIME_HIGH
// of the run and the wraps between them), last-writer-wins for `low` and `y`, and for base_x / pol either "set to" (the run
// holds a VECT_BASE_X) or "add" (the increments of its vector words).  combine(a, b) is associative; a word that starts a
// lane carries the lane's state from the push before in front of it and the SEG flag, which makes the scan segmented.
//
// Whether an emitted event is dropped (no TIME_HIGH yet; outside the sensor) depends on the state in front of its word, so
// the output offsets can only be summed once the states are known.  Three launches, one workgroup per tile of
// DAGR_DECODE_TILE words, none waiting on another:
//   1. reduce: the tile's Elem -- a thread folds its four consecutive words, one block scan joins the threads' folds;
//   2. count:  the tile composes the Elems of the tiles before it (one workgroup reads n_tiles * 32 bytes at the most; a
//              push of 100 k words has 98 tiles), rescans its words and counts decoded / unsynced / outside / skipped; the
//              thread on a lane's last word writes the lane's new state;
//   3. emit:   the tile sums the decoded counts of the tiles before it, rescans, expands its vector words through LDS and
//              writes its rows as contiguous stores.
// The carried states are copied aside by launch 1, so that launch 2 can write the new ones while its other tiles still read.
#include "common.hpp"

namespace dagr {
namespace {

constexpr int kTile = DAGR_DECODE_TILE;
constexpr int kPer = kTile / kBlock;     // consecutive words per thread
static_assert(kTile % kBlock == 0 && kTile <= 1024, "a thread takes kPer consecutive words; a row's word index has 10 bits");
constexpr int kStateInts = 8;           // int64 per lane: high, low, loops, y, base_x, pol, synced, 0

enum : int32_t { HH = 1, HL = 2, HY = 4, HB = 8, POL = 16, SEG = 32 };

struct Elem {
    int64_t wr;         // wraps between the run's TIME_HIGHs (a lane's first word adds the lane's loops)
    int32_t flags;
    int32_t fh, lh;     // first / last TIME_HIGH value (HH)
    int32_t low, y;     // (HL) / (HY)
    uint32_t base;      // HB: base_x behind the run; else what the run adds to it
};

template <int FMT> struct Fmt;
template <> struct Fmt<DAGR_DECODE_EVT3> {
    using Word = uint16_t;
    static constexpr int64_t kWrap = 2048;
    static constexpr int kHighShift = 12, kLoopShift = 24;
};
template <> struct Fmt<DAGR_DECODE_EVT2> {
    using Word = uint32_t;
    static constexpr int64_t kWrap = 1ll << 27;
    static constexpr int kHighShift = 6, kLoopShift = 34;
};

__device__ __forceinline__ Elem identity() { return Elem{0, 0, 0, 0, 0, 0, 0u}; }

// a, then b
template <int FMT>
__device__ __forceinline__ Elem combine(const Elem &a, const Elem &b) {
    if (b.flags & SEG) return b;
    Elem r;
    r.flags = (a.flags | b.flags) & ~POL;
    r.wr = a.wr + b.wr;
    if (b.flags & HH) {
        r.lh = b.lh;
        r.fh = (a.flags & HH) ? a.fh : b.fh;
        if ((a.flags & HH) && (int64_t)a.lh - (int64_t)b.fh >= Fmt<FMT>::kWrap) r.wr += 1;
    } else {
        r.fh = a.fh;
        r.lh = a.lh;
    }
    r.low = (b.flags & HL) ? b.low : a.low;
    r.y = (b.flags & HY) ? b.y : a.y;
    if (b.flags & HB) {
        r.base = b.base;
        r.flags |= b.flags & POL;
    } else {
        r.base = a.base + b.base;       // (modulo 2^32)
        r.flags |= a.flags & POL;
    }
    return r;
}

template <int FMT>
__device__ __forceinline__ Elem word_elem(uint32_t w) {
    Elem e = identity();
    if (FMT == DAGR_DECODE_EVT3) {
        const uint32_t v = w & 0xFFFu;
        switch (w >> 12) {
        case 0x0: e.flags = HY; e.y = (int32_t)(w & 0x7FFu); break;
        case 0x3: e.flags = HB | ((w >> 11) & 1u ? POL : 0); e.base = w & 0x7FFu; break;
        case 0x4: e.base = 12u; break;
        case 0x5: e.base = 8u; break;
        case 0x6: e.flags = HL; e.low = (int32_t)v; break;
        case 0x8: e.flags = HH; e.fh = e.lh = (int32_t)v; break;
        default: break;
        }
    } else if ((w >> 28) == 0x8u) {
        e.flags = HH;
        e.fh = e.lh = (int32_t)(w & 0x0FFFFFFFu);
    }
    return e;
}

// the state a lane carries, as the Elem that sets it
__device__ __forceinline__ Elem seed_elem(const int64_t *__restrict__ s) {
    Elem e;
    e.wr = s[2];
    e.flags = HL | HY | HB | (s[6] ? HH : 0) | (s[5] ? POL : 0);
    e.fh = e.lh = (int32_t)s[0];
    e.low = (int32_t)s[1];
    e.y = (int32_t)s[3];
    e.base = (uint32_t)s[4];
    return e;
}

__device__ __forceinline__ Elem shfl_up_elem(const Elem &v, int d) {
    Elem n;
    n.wr = __shfl_up((long long)v.wr, d, 64);
    n.flags = __shfl_up(v.flags, d, 64);
    n.fh = __shfl_up(v.fh, d, 64);
    n.lh = __shfl_up(v.lh, d, 64);
    n.low = __shfl_up(v.low, d, 64);
    n.y = __shfl_up(v.y, d, 64);
    n.base = (uint32_t)__shfl_up((int)v.base, d, 64);
    return n;
}

struct ScanLds {
    Elem wave[kBlock / kWave];
    Elem carry;
};

// Inclusive scan of one Elem per thread over the block, `s.carry` (everything in front of the chunk) composed in front;
// `excl` is what stands in front of the thread's own Elem.  Afterwards s.carry is the last thread's result.  Thread 0
// sets s.carry before the first chunk; a barrier separates.
template <int FMT>
__device__ __forceinline__ Elem chunk_scan(Elem v, ScanLds &s, Elem &excl) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const Elem n = shfl_up_elem(v, d);
        if (lane >= d) v = combine<FMT>(n, v);
    }
    if (lane == 63) s.wave[wid] = v;
    excl = shfl_up_elem(v, 1);
    if (lane == 0) excl = identity();
    __syncthreads();
    Elem front = s.carry;
    for (int k = 0; k < wid; ++k) front = combine<FMT>(front, s.wave[k]);
    excl = combine<FMT>(front, excl);
    v = combine<FMT>(front, v);
    __syncthreads();
    if (threadIdx.x == kBlock - 1) s.carry = v;
    __syncthreads();
    return v;
}

// The tile's words, kPer consecutive ones per thread: loaded, folded inside the thread, then ONE block scan over the
// threads' folds; state(j) is the state behind the thread's j-th word.  s.carry must hold what stands in front of the tile.
template <int FMT>
struct TileScan {
    Elem el[kPer], front;
    uint32_t w[kPer];
    int lane[kPer];
    __device__ __forceinline__ int index(int j) const { return (int)blockIdx.x * kTile + (int)threadIdx.x * kPer + j; }
    __device__ __forceinline__ TileScan(const typename Fmt<FMT>::Word *__restrict__ words, int n_words, const int *s_end, int B,
                                        const int64_t *__restrict__ seeds, ScanLds &s);
    __device__ __forceinline__ Elem state(int j) const { return combine<FMT>(front, el[j]); }
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// The lanes' cumulative ends, clamped to a non-decreasing sequence inside [0, n_words]; `bad` if that changed one.
__device__ __forceinline__ bool load_ends(const int64_t *__restrict__ word_end, int B, int n_words, int *s_end) {
    bool bad = false;
    if (threadIdx.x == 0) {
        int prev = 0;
        for (int b = 0; b < B; ++b) {
            const int64_t e = word_end[b];
            const int c = (int)min(max(e, (int64_t)prev), (int64_t)n_words);
            bad |= (int64_t)c != e;
            s_end[b] = prev = c;
        }
        bad |= prev != n_words;
    }
    return bad;
}

// the lane of word i: the first b with s_end[b] > i (B: behind every lane)
__device__ __forceinline__ int lane_of(const int *s_end, int B, int i) {
    int lo = 0, hi = B;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_end[mid] <= i) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Word i as the scan takes it: its Elem, with the lane's carried state in front of a lane's first word.
template <int FMT>
__device__ __forceinline__ Elem load_elem(const typename Fmt<FMT>::Word *__restrict__ words, int i, int n_words,
                                          const int *s_end, int B, const int64_t *__restrict__ seeds, uint32_t &w,
                                          int &lane) {
    w = 0;
    lane = B;
    if (i >= n_words) return identity();
    lane = lane_of(s_end, B, i);
    if (lane >= B) return identity();
    w = words[i];
    Elem e = word_elem<FMT>(w);
    if (i == (lane > 0 ? s_end[lane - 1] : 0)) {
        e = combine<FMT>(seed_elem(seeds + kStateInts * lane), e);
        e.flags |= SEG;
    }
    return e;
}

template <int FMT>
__device__ __forceinline__ TileScan<FMT>::TileScan(const typename Fmt<FMT>::Word *__restrict__ words, int n_words,
                                                   const int *s_end, int B, const int64_t *__restrict__ seeds, ScanLds &s) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        el[j] = load_elem<FMT>(words, index(j), n_words, s_end, B, seeds, w[j], lane[j]);
        if (j > 0) el[j] = combine<FMT>(el[j - 1], el[j]);       // (inclusive inside the thread)
    }
    chunk_scan<FMT>(el[kPer - 1], s, front);
}

// What word w emits behind the state `e` (inclusive of w): the bits of its events that are decoded, and the counts.
// x of bit i is x0 + i.
struct Emit {
    uint32_t mask, x0;
    int unsynced, outside, skipped;
};
template <int FMT>
__device__ __forceinline__ Emit emit_of(uint32_t w, const Elem &e, int sensor_w, int sensor_h, int &y, int &pol) {
    Emit m{0u, 0u, 0, 0, 0};
    uint32_t raw = 0;
    y = e.y;
    pol = (e.flags & POL) ? 1 : 0;
    if (FMT == DAGR_DECODE_EVT3) {
        switch (w >> 12) {
        case 0x2: raw = 1u; m.x0 = w & 0x7FFu; pol = (int)((w >> 11) & 1u); break;
        case 0x4: raw = w & 0xFFFu; m.x0 = e.base - 12u; break;
        case 0x5: raw = w & 0xFFu; m.x0 = e.base - 8u; break;
        case 0x0: case 0x3: case 0x6: case 0x8: break;
        default: m.skipped = 1; break;
        }
    } else {
        const uint32_t type = w >> 28;
        if (type <= 1u) {
            raw = 1u;
            m.x0 = (w >> 11) & 0x7FFu;
            y = (int)(w & 0x7FFu);
            pol = (int)type;
        } else if (type != 0x8u) {
            m.skipped = 1;
        }
    }
    if (!raw) return m;
    const int n = __popc(raw);
    if (!(e.flags & HH)) {
        m.unsynced = n;
        return m;
    }
    uint32_t in = 0;
    if (y < sensor_h)
        for (int i = 0; i < 12; ++i)
            if ((uint32_t)(m.x0 + (uint32_t)i) < (uint32_t)sensor_w) in |= 1u << i;
    m.mask = raw & in;
    m.outside = n - __popc(m.mask);
    return m;
}

template <int FMT>
__device__ __forceinline__ int64_t time_of(uint32_t w, const Elem &e, int64_t t_base) {
    const int64_t low = FMT == DAGR_DECODE_EVT3 ? (int64_t)e.low : (int64_t)((w >> 22) & 0x3Fu);
    return t_base + (e.wr << Fmt<FMT>::kLoopShift) + ((int64_t)e.lh << Fmt<FMT>::kHighShift) + low;
}

// Launch 1: the tile's Elem.  Block 0 also copies the carried states aside and checks word_end.
template <int FMT>
__global__ __launch_bounds__(kBlock) void k_decode_reduce(const typename Fmt<FMT>::Word *__restrict__ words, int n_words,
                                                         const int64_t *__restrict__ word_end, int B,
                                                         const int64_t *__restrict__ state, int64_t *__restrict__ seeds,
                                                         Elem *__restrict__ tile_sum, int32_t *__restrict__ status) {
    __shared__ ScanLds s;
    __shared__ int s_end[128];
    const bool bad = load_ends(word_end, B, n_words, s_end);
    if (threadIdx.x == 0) s.carry = identity();
    if (blockIdx.x == 0) {
        if (bad) atomicOr(status, 8);
        for (int k = threadIdx.x; k < kStateInts * B; k += kBlock) seeds[k] = state[k];
    }
    __syncthreads();
    TileScan<FMT> ts(words, n_words, s_end, B, state, s);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = s.carry;
}

// Everything in front of tile `tile`: the Elems of the tiles before it, composed (back to the last lane start: SEG).
template <int FMT>
__device__ __forceinline__ void compose_front(const Elem *__restrict__ tile_sum, int tile, ScanLds &s) {
    if (threadIdx.x == 0) s.carry = identity();
    __syncthreads();
    for (int j0 = 0; j0 < tile; j0 += kBlock) {
        const int j = j0 + (int)threadIdx.x;
        Elem unused;
        chunk_scan<FMT>(j < tile ? tile_sum[j] : identity(), s, unused);
    }
}

// Launch 2: the tile's counts, the lanes' counters and the new states of the lanes that end in the tile.
template <int FMT>
__global__ __launch_bounds__(kBlock) void k_decode_count(const typename Fmt<FMT>::Word *__restrict__ words, int n_words,
                                                        const int64_t *__restrict__ word_end, int B, int sensor_w,
                                                        int sensor_h, const int64_t *__restrict__ seeds,
                                                        int64_t *__restrict__ state, const Elem *__restrict__ tile_sum,
                                                        Elem *__restrict__ tile_in, int32_t *__restrict__ tile_cnt,
                                                        int64_t *__restrict__ lane_counts, int32_t *__restrict__ status) {
    __shared__ ScanLds s;
    __shared__ int s_end[128];
    __shared__ int s_cnt[128 * 4];
    __shared__ int s_total;
    load_ends(word_end, B, n_words, s_end);
    for (int k = threadIdx.x; k < 4 * B; k += kBlock) s_cnt[k] = 0;
    if (threadIdx.x == 0) s_total = 0;
    compose_front<FMT>(tile_sum, (int)blockIdx.x, s);
    if (threadIdx.x == 0) tile_in[blockIdx.x] = s.carry;
    int decoded_all = 0, outside_any = 0, mine[4] = {0, 0, 0, 0};
    // the common case, one lane from the tile's first word to its last: the counters are summed in registers
    const int tile_begin = (int)blockIdx.x * kTile, tile_end = min(n_words, tile_begin + kTile);
    const int first_lane = min(lane_of(s_end, B, tile_begin), B - 1);
    const bool one_lane = s_end[first_lane] >= tile_end;
    TileScan<FMT> ts(words, n_words, s_end, B, seeds, s);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = ts.index(j), lane = ts.lane[j];
        const uint32_t w = ts.w[j];
        if (lane >= B) continue;
        const Elem e = ts.state(j);
        int y, pol;
        const Emit m = emit_of<FMT>(w, e, sensor_w, sensor_h, y, pol);
        const int decoded = __popc(m.mask);
        decoded_all += decoded;
        outside_any |= m.outside;
        if (one_lane) {                     // summed over the wave below: one LDS atomic per wave and counter
            mine[0] += decoded; mine[1] += m.unsynced; mine[2] += m.outside; mine[3] += m.skipped;
        } else {
            if (decoded) atomicAdd(&s_cnt[4 * lane + 0], decoded);
            if (m.unsynced) atomicAdd(&s_cnt[4 * lane + 1], m.unsynced);
            if (m.outside) atomicAdd(&s_cnt[4 * lane + 2], m.outside);
            if (m.skipped) atomicAdd(&s_cnt[4 * lane + 3], m.skipped);
        }
        if (i + 1 == s_end[lane]) {         // the lane's last word: the state it leaves
            int64_t *st = state + kStateInts * lane;
            st[0] = e.lh;
            st[1] = e.low;
            st[2] = e.wr;
            st[3] = e.y;
            st[4] = (int64_t)e.base;
            st[5] = (e.flags & POL) ? 1 : 0;
            st[6] = (e.flags & HH) ? 1 : 0;
            st[7] = 0;
        }
    }
    decoded_all = wave_sum(decoded_all);
    outside_any = wave_sum(outside_any);
    if (one_lane)
        for (int k = 0; k < 4; ++k) mine[k] = wave_sum(mine[k]);
    if ((threadIdx.x & 63) == 0) {
        if (decoded_all) atomicAdd(&s_total, decoded_all);
        if (outside_any) atomicOr(status, 16);
        if (one_lane)
            for (int k = 0; k < 4; ++k)
                if (mine[k]) atomicAdd(&s_cnt[4 * first_lane + k], mine[k]);
    }
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_total;
    if (lane_counts)
        for (int k = threadIdx.x; k < 4 * B; k += kBlock)
            if (s_cnt[k]) atomicAdd((unsigned long long *)&lane_counts[k], (unsigned long long)s_cnt[k]);
}

// Launch 3: the rows.  The tile's decoded events get their places by a block scan; every word leaves what its rows share in
// LDS and one (word, bit) entry per row, and the block then writes the tile's rows in order, one row per thread.
template <int FMT>
__global__ __launch_bounds__(kBlock) void k_decode_emit(const typename Fmt<FMT>::Word *__restrict__ words, int n_words,
                                                       const int64_t *__restrict__ word_end, int B, int sensor_w,
                                                       int sensor_h, const int64_t *__restrict__ seeds,
                                                       const Elem *__restrict__ tile_in,
                                                       const int32_t *__restrict__ tile_cnt, int n_tiles,
                                                       const int64_t *__restrict__ t_base, int max_out,
                                                       int32_t *__restrict__ xy_out, int64_t *__restrict__ t_out,
                                                       int8_t *__restrict__ p_out, int32_t *__restrict__ batch_out,
                                                       int32_t *__restrict__ n_out, int32_t *__restrict__ status) {
    __shared__ ScanLds s;
    __shared__ int s_end[128];
    __shared__ int s_scan[4];
    __shared__ unsigned long long s_sum[2];
    __shared__ uint32_t s_x0[kTile];        // per word of the tile: x of bit 0,
    __shared__ int32_t s_ypb[kTile];        // y | pol << 12 | lane << 16,
    __shared__ int64_t s_t[kTile];          // and t
    __shared__ uint16_t s_row[kTile * 12];  // per row of the tile: word << 4 | bit
    load_ends(word_end, B, n_words, s_end);
    if (threadIdx.x == 0) {
        s.carry = tile_in[blockIdx.x];
        s_sum[0] = s_sum[1] = 0;
    }
    __syncthreads();
    {
        unsigned long long before = 0, all = 0;
        for (int j = threadIdx.x; j < n_tiles; j += kBlock) {
            const unsigned long long v = (unsigned long long)max(tile_cnt[j], 0);
            all += v;
            if (j < (int)blockIdx.x) before += v;
        }
        if (before) atomicAdd(&s_sum[0], before);
        if (all) atomicAdd(&s_sum[1], all);
    }
    __syncthreads();
    const int64_t at = (int64_t)s_sum[0];
    const int64_t total = (int64_t)s_sum[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *n_out = (int32_t)min(total, (int64_t)max_out);
        if (total > max_out) atomicOr(status, 64);
    }
    // the rows behind the count: lane-less, as dagr_stream_denoise leaves them
    for (int64_t r = total + (int64_t)blockIdx.x * kBlock + threadIdx.x; r < max_out; r += (int64_t)gridDim.x * kBlock) {
        xy_out[r] = 0;
        batch_out[r] = -1;
    }
    TileScan<FMT> ts(words, n_words, s_end, B, seeds, s);
    uint32_t mask[kPer];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        mask[j] = 0;
        if (ts.lane[j] >= B) continue;
        const Elem e = ts.state(j);
        int y, pol;
        const Emit m = emit_of<FMT>(ts.w[j], e, sensor_w, sensor_h, y, pol);
        mask[j] = m.mask;
        mine += __popc(m.mask);
        if (m.mask) {
            const int k = (int)threadIdx.x * kPer + j;
            s_x0[k] = m.x0;
            s_ypb[k] = y | pol << 12 | ts.lane[j] << 16;
            s_t[k] = time_of<FMT>(ts.w[j], e, t_base ? t_base[ts.lane[j]] : 0);
        }
    }
    int tile_total;
    int pos = block_exclusive_scan(mine, s_scan, tile_total);
#pragma unroll
    for (int j = 0; j < kPer; ++j)
        for (uint32_t bits = mask[j]; bits; bits &= bits - 1)
            s_row[pos++] = (uint16_t)(((int)threadIdx.x * kPer + j) << 4 | (__ffs(bits) - 1));
    __syncthreads();
    for (int r = threadIdx.x; r < tile_total; r += kBlock) {
        const int64_t g = at + r;
        if (g >= max_out) break;
        const int src = s_row[r] >> 4, bit = s_row[r] & 15;
        const int32_t ypb = s_ypb[src];
        xy_out[g] = (int32_t)((s_x0[src] + (uint32_t)bit) & 0xFFFFu) | (ypb & 0xFFF) << 16;
        t_out[g] = s_t[src];
        p_out[g] = (ypb >> 12 & 1) ? 1 : -1;
        batch_out[g] = ypb >> 16;
    }
}

struct Decode {
    int64_t *state, *seeds;
    Elem *tile_sum, *tile_in;
    int32_t *tile_cnt;
};

size_t carve_decode(int B, int64_t max_words, char *base, Decode *out) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return base ? base + o : nullptr;
    };
    const size_t tiles = (size_t)ceil_div(max_words, kTile);
    Decode d;
    d.state = (int64_t *)take((size_t)B * kStateInts * 8);
    d.seeds = (int64_t *)take((size_t)B * kStateInts * 8);
    d.tile_sum = (Elem *)take(tiles * sizeof(Elem));
    d.tile_in = (Elem *)take(tiles * sizeof(Elem));
    d.tile_cnt = (int32_t *)take(tiles * 4);
    if (out) *out = d;
    return off;
}

bool decode_sizes_ok(int32_t B, int64_t max_words) { return B >= 1 && B < 128 && max_words >= 1 && max_words < (1ll << 25); }

template <int FMT>
void launch_decode(const Decode &d, int B, int sensor_w, int sensor_h, const void *words_, const int64_t *word_end, int n,
                   const int64_t *t_base, int max_out, int32_t *xy_out, int64_t *t_out, int8_t *p_out, int32_t *batch_out,
                   int32_t *n_out, int64_t *lane_counts, int32_t *status, hipStream_t stream) {
    const auto *words = (const typename Fmt<FMT>::Word *)words_;
    const int tiles = (int)std::max<int64_t>(ceil_div(n, kTile), 1);
    k_decode_reduce<FMT><<<tiles, kBlock, 0, stream>>>(words, n, word_end, B, d.state, d.seeds, d.tile_sum, status);
    k_decode_count<FMT><<<tiles, kBlock, 0, stream>>>(words, n, word_end, B, sensor_w, sensor_h, d.seeds, d.state, d.tile_sum,
                                                      d.tile_in, d.tile_cnt, lane_counts, status);
    k_decode_emit<FMT><<<tiles, kBlock, 0, stream>>>(words, n, word_end, B, sensor_w, sensor_h, d.seeds, d.tile_in, d.tile_cnt,
                                                     tiles, t_base, max_out, xy_out, t_out, p_out, batch_out, n_out, status);
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" size_t dagr_stream_decode_bytes(int32_t B, int64_t max_words) {
    if (!decode_sizes_ok(B, max_words)) return 0;
    return carve_decode(B, max_words, nullptr, nullptr);
}

extern "C" int dagr_stream_decode_reset(void *state, size_t state_bytes, int32_t B, int64_t max_words, void *stream) {
    DAGR_CHECK_ARG(state != nullptr, "stream decode: state is NULL");
    DAGR_CHECK_ARG(decode_sizes_ok(B, max_words), "stream decode: sizes out of range");
    DAGR_CHECK_ARG(state_bytes >= carve_decode(B, max_words, nullptr, nullptr),
                   "stream decode: state smaller than dagr_stream_decode_bytes");
    DAGR_CHECK_HIP(hipMemsetAsync(state, 0, (size_t)B * kStateInts * 8, (hipStream_t)stream));
    return DAGR_OK;
}

extern "C" int dagr_stream_decode(void *state, size_t state_bytes, int32_t B, int64_t max_words, int32_t format,
                                  int32_t sensor_w, int32_t sensor_h, const void *words, const int64_t *word_end,
                                  int64_t n_words, const int64_t *t_base, int64_t max_out, int16_t *xy_out, int64_t *t_out,
                                  int8_t *p_out, int32_t *batch_out, int32_t *n_out, int64_t *lane_counts, int32_t *status,
                                  void *stream) {
    DAGR_CHECK_ARG(format == DAGR_DECODE_EVT2 || format == DAGR_DECODE_EVT3,
                   "stream decode: format is DAGR_DECODE_EVT2 or DAGR_DECODE_EVT3");
    DAGR_CHECK_ARG(decode_sizes_ok(B, max_words), "stream decode: sizes out of range");
    DAGR_CHECK_ARG(sensor_w >= 1 && sensor_h >= 1 && sensor_w <= 32767 && sensor_h <= 32767,
                   "stream decode: sensor size out of range");
    DAGR_CHECK_ARG(n_words >= 0 && n_words <= max_words, "stream decode: max_words < n_words");
    DAGR_CHECK_ARG(max_out >= 1 && max_out < (1ll << 30), "stream decode: max_out out of range");
    DAGR_CHECK_ARG(state && word_end && xy_out && t_out && p_out && batch_out && n_out && status,
                   "stream decode: NULL pointer");
    DAGR_CHECK_ARG(n_words == 0 || words, "stream decode: words is NULL");
    DAGR_CHECK_ARG(((uintptr_t)words & (format == DAGR_DECODE_EVT3 ? 1 : 3)) == 0,
                   "stream decode: words must be aligned to the word size");
    DAGR_CHECK_ARG(((uintptr_t)xy_out & 3) == 0, "stream decode: xy_out must be 4-byte aligned");
    Decode d;
    DAGR_CHECK_ARG(state_bytes >= carve_decode(B, max_words, (char *)state, &d),
                   "stream decode: state smaller than dagr_stream_decode_bytes");
    if (format == DAGR_DECODE_EVT3)
        launch_decode<DAGR_DECODE_EVT3>(d, B, sensor_w, sensor_h, words, word_end, (int)n_words, t_base, (int)max_out,
                                        (int32_t *)xy_out, t_out, p_out, batch_out, n_out, lane_counts, status,
                                        (hipStream_t)stream);
    else
        launch_decode<DAGR_DECODE_EVT2>(d, B, sensor_w, sensor_h, words, word_end, (int)n_words, t_base, (int)max_out,
                                        (int32_t *)xy_out, t_out, p_out, batch_out, n_out, lane_counts, status,
                                        (hipStream_t)stream);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
