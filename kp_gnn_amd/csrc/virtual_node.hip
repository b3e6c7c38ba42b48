// Virtual node: out[n,:] = x[n,:] + v[g(n),:] for the nodes of graph g, and (optionally, from the same pass)
// pooled[g,:] = sum_n out[n,:] + v[g,:] (gfx950).  Contract: include/kpgnn.h, kpgnn_vn_add_pool.
// Replaces the bodies' h + vn[batch] (an index gather and an [N,H] add) and the global_add_pool(h) + vn at the top of the
// virtual-node update (models/GNNs.py:196-199,227-230): one read of x, one write of out.  Mapping as in pool.hip: a sub-group
// of lanes owns one graph, lanes span the feature columns 16 B wide, four independent row loads in flight, rows are added
// in node order - bitwise reproducible, no atomics.  The work is driven by graph_ptr: a row at or beyond graph_ptr[G] (or
// *n_dyn) is neither read nor written, so the buffers may be longer than the batch (dataset.StaticBatch).
// The backward is the same entry: gx = gout + gp[g], gv[g] = sum_n gx[n] + gp[g].
#include <initializer_list>

#include "kpgnn_common.h"

namespace kpgnn {
namespace {

constexpr int kBlock = 256;

struct VnParams {
    const int32_t* n_dyn;
    int64_t N; int G, D;
    const int32_t* ptr;
    const float* x; int64_t xs;
    const float* v; int64_t vs;
    float* out; int64_t os;
    float* pooled;
};

template <int VEC, int L>
__global__ void __launch_bounds__(kBlock) vn_add_pool_kernel(VnParams p) {
    p.N = live_rows(p.N, p.n_dyn);
    const int sg = threadIdx.x / L, sl = threadIdx.x % L, c0 = sl * VEC;
    const int64_t g = (int64_t)blockIdx.x * (kBlock / L) + sg;
    if (g >= p.G || c0 >= p.D) return;
    int64_t end = p.ptr[g + 1], beg = p.ptr[g];
    end = end < p.N ? end : p.N;                // (never past the live rows, whatever the pointer says)
    beg = beg < 0 ? 0 : beg;
    float vg[VEC], acc[VEC];
    ldv<VEC>(p.v + g * p.vs + c0, vg);
    for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
    int64_t r = beg;
    for (; r + 3 < end; r += 4) {               // four independent row loads per trip, added in row order
        float w[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) ldv<VEC>(p.x + (r + u) * p.xs + c0, w[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            for (int q = 0; q < VEC; ++q) { w[u][q] += vg[q]; acc[q] += w[u][q]; }
            stv<VEC>(p.out + (r + u) * p.os + c0, w[u]);
        }
    }
    for (; r < end; ++r) {
        float w[VEC];
        ldv<VEC>(p.x + r * p.xs + c0, w);
        for (int q = 0; q < VEC; ++q) { w[q] += vg[q]; acc[q] += w[q]; }
        stv<VEC>(p.out + r * p.os + c0, w);
    }
    if (p.pooled) {
        for (int q = 0; q < VEC; ++q) acc[q] += vg[q];
        stv<VEC>(p.pooled + g * p.D + c0, acc);
    }
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_vn_add_pool(const kpgnn_vn_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_vn_add_pool";
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->N >= 0 && d->G >= 0 && d->D >= 1, "%s: bad N=%lld G=%d D=%d", who, (long long)d->N, d->G, d->D);
    KPGNN_REQUIRE(d->G == 0 || d->graph_ptr, "%s: NULL graph_ptr", who);
    KPGNN_REQUIRE(d->G == 0 || d->v, "%s: NULL v", who);
    KPGNN_REQUIRE(d->N == 0 || (d->x && d->out), "%s: NULL x/out", who);
    KPGNN_REQUIRE(d->x_stride >= d->D && d->out_stride >= d->D, "%s: x/out row stride shorter than D=%d", who, d->D);
    KPGNN_REQUIRE(d->v_stride == 0 || d->v_stride >= d->D, "%s: v row stride must be 0 (one row for all graphs) or >= D=%d", who, d->D);
    if (d->D > 256) return fail(KPGNN_ELIMIT, "%s: D=%d too wide", who, d->D);
    if (d->G == 0) return KPGNN_OK;
    const int vec = row_vec(d->D, {d->x, d->v, d->out, d->pooled}, {d->x_stride, d->v_stride, d->out_stride});
    const int lanes = row_lanes(d->D, vec);
    VnParams p = {};
    p.n_dyn = d->n_dyn; p.N = d->N; p.G = d->G; p.D = d->D; p.ptr = d->graph_ptr;
    p.x = d->x; p.xs = d->x_stride; p.v = d->v; p.vs = d->v_stride; p.out = d->out; p.os = d->out_stride; p.pooled = d->pooled;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)((d->G + (kBlock / lanes) - 1) / (kBlock / lanes));
    return dispatch_row_shape<256>(vec, lanes, who, [&](auto V, auto L) {
        hipLaunchKernelGGL((vn_add_pool_kernel<V.value, L.value>), dim3(grid), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("vn_add_pool_kernel");
        return KPGNN_OK;
    });
}
