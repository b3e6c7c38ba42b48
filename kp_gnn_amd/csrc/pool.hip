// Graph readout: out[g,:] = sum (or mean) of the rows of graph g, and its backward (gfx950).
// Contract: include/kpgnn.h, kpgnn_segment_pool_fwd / _bwd.  Replaces PyG's global_add_pool / global_mean_pool
// (models/GraphRegression.py:46-51), which the framework runs as a zero fill + index_add_ with fp32 atomics (the order of
// the adds, hence the last bits of the loss, changed from run to run) and a gather in backward.  Collated batches keep
// the nodes of a graph contiguous, so a readout is a segmented sum on the walk of segment_rows.h: a sub-group of lanes owns one
// graph, lanes span the feature columns 16 B wide, rows are added in node order - bitwise reproducible, one launch per
// direction.  Rows at or beyond the live count are neither read nor counted, whatever graph_ptr says.
#include "segment_rows.h"

namespace kpgnn {
namespace {

struct PoolParams {
    const int32_t* n_dyn;
    int64_t N; int G, D, mean;
    const int32_t* ptr; const int64_t* batch;
    const float* x; int64_t xs;
    float* out;
    const float* gout; float* gx; int64_t gxs;
};

template <int VEC, int L>
__global__ void __launch_bounds__(kRowBlock) pool_fwd_kernel(PoolParams p) {
    p.N = live_rows(p.N, p.n_dyn);
    const int sg = threadIdx.x / L, sl = threadIdx.x % L, c0 = sl * VEC;
    const int64_t g = (int64_t)blockIdx.x * (kRowBlock / L) + sg;
    if (g >= p.G || c0 >= p.D) return;
    const GraphRows rows = graph_rows(p.ptr, g, p.N);
    float acc[VEC];
    for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
    for_graph_rows<VEC>(p.x, p.xs, c0, rows.beg, rows.end, [&](float (&v)[VEC], int) {
        for (int q = 0; q < VEC; ++q) acc[q] += v[q];
    });
    const float sc = (p.mean && rows.end > rows.beg) ? 1.0f / (float)(rows.end - rows.beg) : 1.0f;
    for (int q = 0; q < VEC; ++q) acc[q] *= sc;
    stv<VEC>(p.out + g * p.D + c0, acc);
}

template <int VEC, int L>
__global__ void __launch_bounds__(kRowBlock) pool_bwd_kernel(PoolParams p) {
    p.N = live_rows(p.N, p.n_dyn);
    const int sg = threadIdx.x / L, sl = threadIdx.x % L, c0 = sl * VEC;
    if (c0 >= p.D) return;
    for (int64_t n = (int64_t)blockIdx.x * (kRowBlock / L) + sg; n < p.N; n += (int64_t)gridDim.x * (kRowBlock / L)) {
        const int64_t g = p.batch[n];
        float sc = 1.0f;
        if (p.mean) {                           // (the divisor of the forward: the graph's LIVE rows)
            const GraphRows rows = graph_rows(p.ptr, g, p.N);
            sc = rows.end > rows.beg ? 1.0f / (float)(rows.end - rows.beg) : 1.0f;
        }
        float v[VEC];
        ldv<VEC>(p.gout + g * p.D + c0, v);
        for (int q = 0; q < VEC; ++q) v[q] *= sc;
        stv<VEC>(p.gx + n * p.gxs + c0, v);
    }
}

int check(const kpgnn_pool_desc* d, const char* who) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->N >= 0 && d->G >= 0 && d->D >= 1 && d->D <= 1024, "%s: bad N=%lld G=%d D=%d", who, (long long)d->N, d->G, d->D);
    KPGNN_REQUIRE(d->mode == 0 || d->mode == 1, "%s: mode must be 0 (sum) or 1 (mean)", who);
    KPGNN_REQUIRE(d->G == 0 || d->graph_ptr, "%s: NULL graph_ptr", who);
    return KPGNN_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_segment_pool_fwd(const kpgnn_pool_desc* d, kpgnn_stream_t stream) {
    int rc = check(d, "segment_pool_fwd");
    if (rc != KPGNN_OK) return rc;
    if (d->G == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->out && (d->N == 0 || (d->x && d->x_stride >= d->D)), "segment_pool_fwd: NULL x/out or bad stride");
    PoolParams p = {};
    p.N = d->N; p.n_dyn = d->n_dyn; p.G = d->G; p.D = d->D; p.mean = d->mode; p.ptr = d->graph_ptr; p.x = d->x; p.xs = d->x_stride; p.out = d->out;
    return launch_row_walk(d->D, {d->x, d->out}, {d->x_stride}, "segment_pool", "pool_fwd_kernel", graph_grid, d->G, p,
                           (hipStream_t)stream, [](auto V, auto L) { return pool_fwd_kernel<V.value, L.value>; });
}

extern "C" int kpgnn_segment_pool_bwd(const kpgnn_pool_desc* d, kpgnn_stream_t stream) {
    int rc = check(d, "segment_pool_bwd");
    if (rc != KPGNN_OK) return rc;
    if (d->N == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->batch && d->gout && d->gx && d->gx_stride >= d->D, "segment_pool_bwd: NULL batch/gout/gx or bad stride");
    PoolParams p = {};
    p.N = d->N; p.n_dyn = d->n_dyn; p.G = d->G; p.D = d->D; p.mean = d->mode; p.ptr = d->graph_ptr; p.batch = d->batch;
    p.gout = d->gout; p.gx = d->gx; p.gxs = d->gx_stride;
    return launch_row_walk(d->D, {d->gout, d->gx}, {d->gx_stride}, "segment_pool", "pool_bwd_kernel", row_grid, d->N, p,
                           (hipStream_t)stream, [](auto V, auto L) { return pool_bwd_kernel<V.value, L.value>; });
}
