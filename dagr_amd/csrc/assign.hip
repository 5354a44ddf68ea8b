// assign.hip -- dagr_assign_max_weight: the maximum-weight one-to-one pairing of rows with columns for B independent
// int32 matrices of up to 1024 x 1024, one launch, one workgroup of ONE wave per matrix (assign.hpp has the routine and says
// how the wave holds it).  include/dagr_hip.h states the method and the arguments; dagr_amd/streaming.py:
// assign_max_weight_definition is the same in numpy.
#include "assign.hpp"

namespace dagr {
namespace {

__global__ __launch_bounds__(kWave) void k_assign_max_weight(const int32_t *__restrict__ w, int ld_rows, int ld,
                                                             const int32_t *__restrict__ n_rows,
                                                             const int32_t *__restrict__ n_cols, int max_rows, int max_cols,
                                                             int32_t *__restrict__ row_col, int64_t *__restrict__ total,
                                                             int32_t *__restrict__ workspace) {
    __shared__ AssignLds s;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nr = min(max(n_rows[b], 0), max_rows), nc = min(max(n_cols[b], 0), max_cols);
    int32_t *pairs = row_col + (int64_t)b * max_rows;
    for (int r = nr + lane; r < max_rows; r += kWave) pairs[r] = -1;
    const int64_t sum = assign_wave(w + (int64_t)b * ld_rows * ld, ld, nr, nc, workspace + (int64_t)b * max_rows * max_cols,
                                    pairs, s);
    if (lane == 0) total[b] = sum;
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" size_t dagr_assign_workspace_bytes(int32_t B, int32_t max_rows, int32_t max_cols) {
    return assign_sizes_ok(B, max_rows, max_cols) ? assign_workspace_bytes(B, max_rows, max_cols) : 0;
}

extern "C" int dagr_assign_max_weight(const int32_t *w, int32_t B, int32_t ld_rows, int32_t ld, const int32_t *n_rows,
                                      const int32_t *n_cols, int32_t max_rows, int32_t max_cols, int32_t *row_col,
                                      int64_t *total, void *workspace, size_t bytes, void *stream) {
    DAGR_CHECK_ARG(assign_sizes_ok(B, max_rows, max_cols),
                   "assign: B (1 .. 65535), max_rows or max_cols (1 .. DAGR_ASSIGN_MAX) out of range");
    DAGR_CHECK_ARG(ld_rows >= max_rows && ld >= max_cols, "assign: ld_rows < max_rows or ld < max_cols");
    DAGR_CHECK_ARG(w && n_rows && n_cols && row_col && total && workspace, "assign: NULL pointer");
    DAGR_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)total & 7) == 0 &&
                       (((uintptr_t)w | (uintptr_t)n_rows | (uintptr_t)n_cols | (uintptr_t)row_col) & 3) == 0,
                   "assign: workspace must be 16-byte aligned, total 8-byte, int32 arrays 4-byte");
    DAGR_CHECK_ARG(bytes >= assign_workspace_bytes(B, max_rows, max_cols),
                   "assign: workspace smaller than dagr_assign_workspace_bytes");
    k_assign_max_weight<<<(unsigned)B, kWave, 0, (hipStream_t)stream>>>(w, ld_rows, ld, n_rows, n_cols, max_rows, max_cols,
                                                                        row_col, total, (int32_t *)workspace);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}
