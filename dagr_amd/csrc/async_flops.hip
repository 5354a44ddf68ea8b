// async_flops.hip -- device-side FLOP accounting of a window in the reference's scheme
// (src/dagr/asynchronous/flops/conv.py, conv.py:28-58, max_pool.py:361-386, linear.py:623-641, cartesian.py:718-728,
// batch_norm.py:787-797): the numbers `make_model_asynchronous(model, log_flops=True)` logs for the init pass
// (log index 0, what `evaluate_flops(..., dense=True)` reports).
//
// Every logged module's count is a closed form of its level's node and edge counts, which the engine already keeps on
// the device: level 0 = the window's events (n_events) and their in-degrees deg[n_events]; pooled level k = counts_k =
// [n_nodes, n_edges].  One workgroup of 1024: the level-0 edge count is a block reduction of deg, then one thread per
// module evaluates its formula in int64 and writes out[m].  The host reads `out` back once.
#include "common.hpp"

namespace dagr {
namespace {

constexpr int kFlopsBlock = 1024;
constexpr int kFlopsUnroll = 8;

__global__ __launch_bounds__(kFlopsBlock) void k_async_flops_init(const int32_t *__restrict__ deg, int32_t n_events,
                                                             const int32_t *__restrict__ c1, const int32_t *__restrict__ c2,
                                                             const int32_t *__restrict__ c3, const int32_t *__restrict__ c4,
                                                             const dagr_flops_module *__restrict__ mods, int32_t n_mods,
                                                             int64_t *__restrict__ out) {
    __shared__ int64_t part[kFlopsBlock];
    __shared__ int64_t nodes[5], edges[5];
    // kFlopsUnroll independent loads in flight per thread: one workgroup, so the sum is bound by load latency, not
    // bandwidth (a 25k-event window: 25 loads per thread in 4 rounds instead of ~100 dependent ones)
    int64_t s = 0;
    for (int base = 0; base < n_events; base += kFlopsBlock * kFlopsUnroll) {
        int32_t v[kFlopsUnroll];
#pragma unroll
        for (int u = 0; u < kFlopsUnroll; u++) {
            const int i = base + u * kFlopsBlock + threadIdx.x;
            v[u] = i < n_events ? deg[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < kFlopsUnroll; u++) s += v[u];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = kFlopsBlock / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int32_t *c[4] = {c1, c2, c3, c4};
        nodes[0] = n_events;
        edges[0] = part[0];
        for (int k = 0; k < 4; k++) {
            nodes[k + 1] = c[k][0];
            edges[k + 1] = c[k][1];
        }
    }
    __syncthreads();
    for (int m = threadIdx.x; m < n_mods; m += kFlopsBlock) {
        const dagr_flops_module d = mods[m];
        const int l = d.level < 0 ? 0 : (d.level > 4 ? 4 : d.level);
        const int64_t N = nodes[l], E = edges[l], cin = d.cin, cout = d.cout;
        int64_t f = 0;
        switch (d.kind) {
        case DAGR_FLOPS_CONV:        // flops/conv.py:1-24: edges * (2 m_in - 1) m_out, root and bias once per node
            f = E * (2 * cin - 1) * cout;
            if (d.root) f += N * cout * (2 * cin - 1);
            if (d.bias) f += N * cout;
            break;
        case DAGR_FLOPS_LINEAR:      // linear.py:637-639: prod(x[mask].size()) * out
            f = N * cin * cout;
            break;
        case DAGR_FLOPS_POOL: {      // max_pool.py:380-384, on the pooled level l + 1: 6 U + C U + edge_index.numel()
            const int l1 = l < 4 ? l + 1 : 4;
            f = 6 * nodes[l1] + cin * nodes[l1] + 2 * edges[l1];
            break;
        }
        case DAGR_FLOPS_CARTESIAN:   // cartesian.py:724-726: 2 * len(edge_attr)
            f = 2 * E;
            break;
        default:                     // batch norm (batch_norm.py:792-795): fused into the conv before it
            f = 0;
        }
        out[m] = f;
    }
}

}  // namespace
}  // namespace dagr

using namespace dagr;

extern "C" {

int dagr_async_flops(const int32_t *deg, int32_t n_events, const int32_t *counts1, const int32_t *counts2,
                     const int32_t *counts3, const int32_t *counts4, const dagr_flops_module *mods, int32_t n_mods,
                     int64_t *out, void *stream) {
    DAGR_CHECK_ARG(n_events >= 0 && n_mods >= 0, "bad sizes");
    if (n_mods == 0) return DAGR_OK;
    DAGR_CHECK_ARG((deg || n_events == 0) && counts1 && counts2 && counts3 && counts4 && mods && out, "NULL pointer");
    k_async_flops_init<<<1, kFlopsBlock, 0, (hipStream_t)stream>>>(deg, n_events, counts1, counts2, counts3, counts4, mods,
                                                              n_mods, out);
    DAGR_CHECK_LAUNCH();
    return DAGR_OK;
}

}  // extern "C"
