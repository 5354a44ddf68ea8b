// assign.hpp -- the maximum-weight assignment of one matrix by ONE wave, as a device routine: dagr_assign_max_weight
// (assign.hip) and dagr_stream_identity_solve (stream_identity.hip) both run it.  include/dagr_hip.h states the method;
// dagr_amd/streaming.py: assign_max_weight_definition is the same in numpy.
//
// The Hungarian method by shortest augmenting paths on the cost -w, the smaller side as rows.  The columns are striped over
// the wave's 64 threads, column j in register j / 64 of thread j % 64 (16 registers at the cap of 1024): the column
// potentials v, the path's minv, its back pointers and the used bits live in registers.  What is read at a position that
// another thread decided lives in LDS, 16 KB: the row potentials u, the matching p and, for the flip, the back pointers.
// A path step is: one read of the step's cost row from global memory (coalesced, at most 4 KB), the relaxation in
// registers and one int64 shuffle reduction that carries the column in its low bits -- so the lowest column wins a tie.
// It writes nothing to LDS and has no barrier: the potentials move once per row, behind the search (see there).
#pragma once
#include "common.hpp"

namespace dagr {

constexpr int kAssignMax = DAGR_ASSIGN_MAX;
constexpr int kAssignRegs = kAssignMax / kWave;     // columns of one thread
constexpr int kAssignColBits = 11;                  // a column (< 1024) in the low bits of the reduction's key
static_assert(kAssignMax % kWave == 0 && kAssignMax <= (1 << kAssignColBits), "whole registers; a column fits its bits");

struct AssignLds {
    int64_t u[kAssignMax];      // the potential of row r
    int32_t p[kAssignMax];      // 1 + the row of column j; 0: the column is free
    int32_t way[kAssignMax];    // 1 + the column before column j on the path; 0: the path's root
};

// w: n_rows x n_cols weights >= 0, row r at w + r * ld.  t: room for n_rows * n_cols words (the transposed matrix; read
// and written only when n_rows > n_cols).  row_col[r], r < n_rows: the column of row r, or -1.  Returns the total, the
// same in every thread.  Called by all 64 threads of a one-wave workgroup with uniform arguments.
__device__ inline int64_t assign_wave(const int32_t *__restrict__ w, int ld, int n_rows, int n_cols, int32_t *__restrict__ t,
                                      int32_t *__restrict__ row_col, AssignLds &s) {
    const int lane = threadIdx.x;
    for (int r = lane; r < n_rows; r += kWave) row_col[r] = -1;
    if (n_rows == 0 || n_cols == 0) return 0;
    const bool transposed = n_rows > n_cols;
    const int32_t *a = w;
    int R = n_rows, C = n_cols, lda = ld;
    if (transposed) {
        for (int r = 0; r < n_rows; r++)
            for (int c = lane; c < n_cols; c += kWave) t[(int64_t)c * n_rows + r] = w[(int64_t)r * ld + c];
        a = t, R = n_cols, C = n_rows, lda = n_rows;
    }
    for (int j = lane; j < C; j += kWave) s.p[j] = 0;
    for (int r = lane; r < R; r += kWave) s.u[r] = 0;
    __syncthreads();                            // (the transposed matrix, too: written by this workgroup, read by it)

    const int nk = (C + kWave - 1) / kWave;
    int64_t v[kAssignRegs];
#pragma unroll
    for (int k = 0; k < kAssignRegs; k++) v[k] = 0;
    for (int i = 0; i < R; i++) {               // row i enters
        // Inside a search nothing is written to LDS.  The definition takes delta from every unused minv and moves the
        // potentials of every used column and its row at every step; here minv is kept PLUS the sum D of the search's
        // deltas so far (the reduced cost of a step gets D added, so every comparison is the definition's), a column
        // remembers D from when it became used, and the potentials move once, behind the search, by D - mark.  A row's u is
        // read when its column becomes used, which is before it has moved.
        int64_t minv[kAssignRegs], mark[kAssignRegs];
        int32_t way[kAssignRegs];               // 1 + the column before column j on the path; 0: the path's root
#pragma unroll
        for (int k = 0; k < kAssignRegs; k++) minv[k] = INT64_MAX, mark[k] = 0, way[k] = 0;
        uint32_t used = 0;                      // bit k: column k * 64 + lane is on the path's tree
        int64_t D = 0;
        int j0 = -1, i0 = i;                    // the step's column (-1: the root) and its row
        while (true) {
            const int64_t base = s.u[i0] - D;
            const int32_t *row = a + (int64_t)i0 * lda;
            const int mine = (j0 >= 0 && (j0 & (kWave - 1)) == lane) ? j0 / kWave : -1;
            // the whole row first, every load in flight at once: no load sits behind a branch (a column at or behind C reads
            // the row's last word)
            int32_t cost[kAssignRegs];
#pragma unroll
            for (int k = 0; k < kAssignRegs; k++) cost[k] = row[min(k * kWave + lane, C - 1)];
            int64_t best = INT64_MAX;
#pragma unroll
            for (int k = 0; k < kAssignRegs; k++) {
                if (k >= nk) continue;          // (uniform)
                const int j = k * kWave + lane;
                if (k == mine) used |= 1u << k, mark[k] = D;
                const bool open = j < C && !((used >> k) & 1u);
                const int64_t cur = -(int64_t)cost[k] - base - v[k];
                const bool better = open && cur < minv[k];
                minv[k] = better ? cur : minv[k];
                way[k] = better ? j0 + 1 : way[k];
                // minv + D >= 0 and below 2**43 (weights below 2**31, at most 2 * 1024 potential moves): the key is exact
                best = min(best, open ? (int64_t)(((uint64_t)minv[k] << kAssignColBits) | (uint64_t)j) : INT64_MAX);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) best = min(best, (int64_t)__shfl_xor((long long)best, off, kWave));
            if (best == INT64_MAX) return -1;   // (unreachable: row i is unpaired and R <= C, so an unused column exists)
            D = best >> kAssignColBits;         // the smallest minv, the lowest column of equals
            j0 = (int)(best & ((1 << kAssignColBits) - 1));
            const int pj = s.p[j0];
            if (pj == 0) break;                 // a free column: the path is complete
            i0 = pj - 1;
        }
#pragma unroll
        for (int k = 0; k < kAssignRegs; k++) {
            const int j = k * kWave + lane;
            if (k < nk && j < C) {
                s.way[j] = way[k];
                if ((used >> k) & 1u) s.u[s.p[j] - 1] += D - mark[k], v[k] -= D - mark[k];      // (used columns have distinct rows)
            }
        }
        if (lane == 0) s.u[i] += D;             // the root's row
        __syncthreads();
        while (j0 >= 0) {                       // flip the path (uniform walk; thread 0 writes)
            const int j1 = s.way[j0] - 1;
            const int src = j1 >= 0 ? s.p[j1] : i + 1;
            if (lane == 0) s.p[j0] = src;
            j0 = j1;
        }
        __syncthreads();
    }

    int64_t total = 0;
    for (int j = lane; j < C; j += kWave) {
        const int pj = s.p[j];
        if (pj == 0) continue;
        const int r = pj - 1;
        const int32_t wt = a[(int64_t)r * lda + j];
        if (wt <= 0) continue;                  // a pair of weight 0 is no pair
        total += wt;
        if (transposed) row_col[j] = r;
        else row_col[r] = j;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) total += (int64_t)__shfl_xor((long long)total, off, kWave);
    return total;
}

inline bool assign_sizes_ok(int32_t B, int32_t max_rows, int32_t max_cols) {
    return B >= 1 && B <= 65535 && max_rows >= 1 && max_rows <= kAssignMax && max_cols >= 1 && max_cols <= kAssignMax;
}
inline size_t assign_workspace_bytes(int32_t B, int32_t max_rows, int32_t max_cols) {
    return align_up(4 * (size_t)B * max_rows * max_cols, 16);
}

}  // namespace dagr
