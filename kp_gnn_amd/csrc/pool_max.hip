// Max graph readout: out[g,:] = column-wise max of the rows of graph g, the winning row per (graph, column), and the
// backward that hands each winner its column's gradient (gfx950).  Contract: include/kpgnn.h, kpgnn_segment_max_fwd / _bwd.
// Replaces PyG 2.1.0's global_max_pool = torch_scatter.scatter_max (models/GraphClassification.py:24-34), which the framework
// restates as a -inf fill + an atomic-max scatter over an expanded [N,D] int64 index and whose backward splits a tied
// column's gradient evenly.  Same mapping as pool.hip: a sub-group of lanes owns one graph, lanes span the feature columns
// 16 B wide, rows are compared in node order with a strict >, so the LOWEST row that attains the max wins - one winner per
// (graph, column), bitwise reproducible, one launch per direction, no fill and no atomics.
#include <initializer_list>

#include "kpgnn_common.h"

namespace kpgnn {
namespace {

constexpr int kBlock = 256;

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
__global__ void __launch_bounds__(kBlock) pool_max_fwd_kernel(MaxParams p) {
    p.N = live_rows(p.N, p.n_dyn);
    const int sg = threadIdx.x / L, sl = threadIdx.x % L, c0 = sl * VEC;
    const int64_t g = (int64_t)blockIdx.x * (kBlock / L) + sg;
    if (g >= p.G || c0 >= p.D) return;
    const int beg = p.ptr[g];
    const int end = (int64_t)p.ptr[g + 1] < p.N ? p.ptr[g + 1] : (int)p.N;      // rows at or beyond the live count are never read
    float acc[VEC];
    int arg[VEC];
    for (int q = 0; q < VEC; ++q) { acc[q] = -INFINITY; arg[q] = -1; }
    int r = beg;
    for (; r + 3 < end; r += 4) {             // four independent row loads per trip, compared in row order
        float v[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) ldv<VEC>(p.x + (int64_t)(r + u) * p.xs + c0, v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) take<VEC>(acc, arg, v[u], r + u);
    }
    for (; r < end; ++r) {
        float v[VEC];
        ldv<VEC>(p.x + (int64_t)r * p.xs + c0, v);
        take<VEC>(acc, arg, v, r);
    }
    stv<VEC>(p.out + g * p.D + c0, acc);
    if (p.arg) sti<VEC>(p.arg + g * p.D + c0, arg);
}

template <int VEC, int L>
__global__ void __launch_bounds__(kBlock) pool_max_bwd_kernel(MaxParams p) {
    p.N = live_rows(p.N, p.n_dyn);
    const int sg = threadIdx.x / L, sl = threadIdx.x % L, c0 = sl * VEC;
    if (c0 >= p.D) return;
    for (int64_t n = (int64_t)blockIdx.x * (kBlock / L) + sg; n < p.N; n += (int64_t)gridDim.x * (kBlock / L)) {
        const int64_t g = p.batch[n];
        float v[VEC];
        int a[VEC];
        ldv<VEC>(p.gout + g * p.D + c0, v);          // [G,D] operands: they stay in L2, the gx row is the only HBM traffic
        ldi<VEC>(p.arg + g * p.D + c0, a);
        for (int q = 0; q < VEC; ++q) v[q] = (int64_t)a[q] == n ? v[q] : 0.0f;
        stv<VEC>(p.gx + n * p.gxs + c0, v);
    }
}

int shape(int D, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> strides, int* vec, int* lanes) {
    *vec = row_vec(D, ptrs, strides);
    if ((D + *vec - 1) / *vec > 256) return fail(KPGNN_ELIMIT, "segment_max: D=%d too wide", D);
    *lanes = row_lanes(D, *vec);
    return KPGNN_OK;
}

#define KP_MAX_LAUNCH(KERNEL, GRID)                                                                          \
    return dispatch_row_shape<256>(vec, lanes, "segment_max", [&](auto V, auto L) {                          \
        hipLaunchKernelGGL((KERNEL<V.value, L.value>), dim3(GRID), dim3(kBlock), 0, s, p);                   \
        KPGNN_LAUNCH_CHECK(#KERNEL);                                                                         \
        return KPGNN_OK;                                                                                     \
    })

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
    int vec, lanes;
    rc = shape(d->D, {d->x, d->out, d->arg}, {d->x_stride}, &vec, &lanes);
    if (rc != KPGNN_OK) return rc;
    MaxParams p = {};
    p.N = d->N; p.n_dyn = d->n_dyn; p.G = d->G; p.D = d->D; p.ptr = d->graph_ptr; p.x = d->x; p.xs = d->x_stride;
    p.out = d->out; p.arg = d->arg;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)((d->G + (kBlock / lanes) - 1) / (kBlock / lanes));
    KP_MAX_LAUNCH(pool_max_fwd_kernel, grid);
}

extern "C" int kpgnn_segment_max_bwd(const kpgnn_pool_max_desc* d, kpgnn_stream_t stream) {
    int rc = check(d, "segment_max_bwd");
    if (rc != KPGNN_OK) return rc;
    if (d->N == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->G >= 1 && d->batch && d->arg && d->gout && d->gx && d->gx_stride >= d->D,
                  "segment_max_bwd: no graphs, NULL batch/arg/gout/gx or bad stride");
    int vec, lanes;
    rc = shape(d->D, {d->gout, d->arg, d->gx}, {d->gx_stride}, &vec, &lanes);
    if (rc != KPGNN_OK) return rc;
    MaxParams p = {};
    p.N = d->N; p.n_dyn = d->n_dyn; p.G = d->G; p.D = d->D; p.batch = d->batch;
    p.arg = d->arg; p.gout = d->gout; p.gx = d->gx; p.gxs = d->gx_stride;
    hipStream_t s = (hipStream_t)stream;
    const int rows = kBlock / lanes;
    int64_t g = (d->N + rows * 4 - 1) / (rows * 4);
    const int64_t cap = (int64_t)device_facts().cu_count * 8;
    const unsigned grid = (unsigned)(g > cap ? cap : (g < 1 ? 1 : g));
    KP_MAX_LAUNCH(pool_max_bwd_kernel, grid);
}
