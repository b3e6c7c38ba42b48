// Max graph readout: out[g,:] = column-wise max of the rows of graph g, the winning row per (graph, column), and the
// backward that hands each winner its column's gradient (gfx950).  Contract: include/kpgnn.h, kpgnn_segment_max_fwd / _bwd.
// Replaces PyG 2.1.0's global_max_pool = torch_scatter.scatter_max (models/GraphClassification.py:24-34), which the framework
// restates as a -inf fill + an atomic-max scatter over an expanded [N,D] int64 index and whose backward splits a tied
// column's gradient evenly.  The walk of segment_rows.h: a sub-group of lanes owns one graph, lanes span the feature columns
// 16 B wide, rows are compared in node order with a strict >, so the LOWEST row that attains the max wins - one winner per
// (graph, column), bitwise reproducible, one launch per direction, no fill and no atomics.
#include "segment_rows.h"

namespace kpgnn {
namespace {

struct MaxParams {
    const int32_t* n_dyn;
    int64_t N; int G, D;
    const int32_t* ptr; const int64_t* batch;
    const float* x; int64_t xs;
    float* out; int32_t* arg;
    const float* gout; float* gx; int64_t gxs;
};

// VEC int32 winners of a row as one access, the integer twin of ldv / stv (same alignment rule: row_vec sees `arg`)
template <int VEC> struct IT;
template <> struct IT<1> { using T = int; };
template <> struct IT<2> { using T = int2; };
template <> struct IT<4> { using T = int4; };
template <int VEC> __device__ __forceinline__ void ldi(const int32_t* p, int (&v)[VEC]) {
    typename IT<VEC>::T t = *reinterpret_cast<const typename IT<VEC>::T*>(p);
    for (int q = 0; q < VEC; ++q) v[q] = reinterpret_cast<const int*>(&t)[q];
}
template <int VEC> __device__ __forceinline__ void sti(int32_t* p, const int (&v)[VEC]) {
    typename IT<VEC>::T t;
    for (int q = 0; q < VEC; ++q) reinterpret_cast<int*>(&t)[q] = v[q];
    *reinterpret_cast<typename IT<VEC>::T*>(p) = t;
}

// Row r replaces the running winner when it is the first row, or the winner is not NaN and r is larger or NaN: ties keep the
// lower row, a NaN once taken stays (so arg is the first NaN row), a graph of -inf rows still names its first row.
template <int VEC>
__device__ __forceinline__ void take(float (&acc)[VEC], int (&arg)[VEC], const float (&v)[VEC], int r) {
    for (int q = 0; q < VEC; ++q)
        if (arg[q] < 0 || (acc[q] == acc[q] && !(v[q] <= acc[q]))) { acc[q] = v[q]; arg[q] = r; }
}

template <int VEC, int L>
__global__ void __launch_bounds__(kRowBlock) pool_max_fwd_kernel(MaxParams p) {
    p.N = live_rows(p.N, p.n_dyn);
    const int sg = threadIdx.x / L, sl = threadIdx.x % L, c0 = sl * VEC;
    const int64_t g = (int64_t)blockIdx.x * (kRowBlock / L) + sg;
    if (g >= p.G || c0 >= p.D) return;
    const GraphRows rows = graph_rows(p.ptr, g, p.N);       // rows at or beyond the live count are never read
    float acc[VEC];
    int arg[VEC];
    for (int q = 0; q < VEC; ++q) { acc[q] = -INFINITY; arg[q] = -1; }
    // The walk of for_graph_rows, written out: handed `take` as a callable (a lambda, a functor, state by reference or by
    // value), the compiler keeps its conditional stores as a branch per column and row, 47 in the kernel against 7, and the
    // launch takes 10.9 us where this form takes 5.7 (2048 graphs of 23 nodes, 104 columns).
    int r = rows.beg;
    for (; r + 3 < rows.end; r += 4) {        // four independent row loads per trip, compared in row order
        float v[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) ldv<VEC>(p.x + (int64_t)(r + u) * p.xs + c0, v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) take<VEC>(acc, arg, v[u], r + u);
    }
    for (; r < rows.end; ++r) {
        float v[VEC];
        ldv<VEC>(p.x + (int64_t)r * p.xs + c0, v);
        take<VEC>(acc, arg, v, r);
    }
    stv<VEC>(p.out + g * p.D + c0, acc);
    if (p.arg) sti<VEC>(p.arg + g * p.D + c0, arg);
}

template <int VEC, int L>
__global__ void __launch_bounds__(kRowBlock) pool_max_bwd_kernel(MaxParams p) {
    p.N = live_rows(p.N, p.n_dyn);
    const int sg = threadIdx.x / L, sl = threadIdx.x % L, c0 = sl * VEC;
    if (c0 >= p.D) return;
    for (int64_t n = (int64_t)blockIdx.x * (kRowBlock / L) + sg; n < p.N; n += (int64_t)gridDim.x * (kRowBlock / L)) {
        const int64_t g = p.batch[n];
        float v[VEC];
        int a[VEC];
        ldv<VEC>(p.gout + g * p.D + c0, v);          // [G,D] operands: they stay in L2, the gx row is the only HBM traffic
        ldi<VEC>(p.arg + g * p.D + c0, a);
        for (int q = 0; q < VEC; ++q) v[q] = (int64_t)a[q] == n ? v[q] : 0.0f;
        stv<VEC>(p.gx + n * p.gxs + c0, v);
    }
}

int check(const kpgnn_pool_max_desc* d, const char* who) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->N >= 0 && d->G >= 0 && d->D >= 1 && d->D <= 1024, "%s: bad N=%lld G=%d D=%d", who, (long long)d->N, d->G, d->D);
    return KPGNN_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_segment_max_fwd(const kpgnn_pool_max_desc* d, kpgnn_stream_t stream) {
    int rc = check(d, "segment_max_fwd");
    if (rc != KPGNN_OK) return rc;
    if (d->G == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->graph_ptr && d->out && (d->N == 0 || (d->x && d->x_stride >= d->D)),
                  "segment_max_fwd: NULL graph_ptr/x/out or bad stride");
    MaxParams p = {};
    p.N = d->N; p.n_dyn = d->n_dyn; p.G = d->G; p.D = d->D; p.ptr = d->graph_ptr; p.x = d->x; p.xs = d->x_stride;
    p.out = d->out; p.arg = d->arg;
    return launch_row_walk(d->D, {d->x, d->out, d->arg}, {d->x_stride}, "segment_max", "pool_max_fwd_kernel", graph_grid, d->G, p,
                           (hipStream_t)stream, [](auto V, auto L) { return pool_max_fwd_kernel<V.value, L.value>; });
}

extern "C" int kpgnn_segment_max_bwd(const kpgnn_pool_max_desc* d, kpgnn_stream_t stream) {
    int rc = check(d, "segment_max_bwd");
    if (rc != KPGNN_OK) return rc;
    if (d->N == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->G >= 1 && d->batch && d->arg && d->gout && d->gx && d->gx_stride >= d->D,
                  "segment_max_bwd: no graphs, NULL batch/arg/gout/gx or bad stride");
    MaxParams p = {};
    p.N = d->N; p.n_dyn = d->n_dyn; p.G = d->G; p.D = d->D; p.batch = d->batch;
    p.arg = d->arg; p.gout = d->gout; p.gx = d->gx; p.gxs = d->gx_stride;
    return launch_row_walk(d->D, {d->gout, d->arg, d->gx}, {d->gx_stride}, "segment_max", "pool_max_bwd_kernel", row_grid, d->N, p,
                           (hipStream_t)stream, [](auto V, auto L) { return pool_max_bwd_kernel<V.value, L.value>; });
}
