// Virtual node: out[n,:] = x[n,:] + v[g(n),:] for the nodes of graph g, and (optionally, from the same pass)
// pooled[g,:] = sum_n out[n,:] + v[g,:] (gfx950).  Contract: include/kpgnn.h, kpgnn_vn_add_pool.
// Replaces the bodies' h + vn[batch] (an index gather and an [N,H] add) and the global_add_pool(h) + vn at the top of the
// virtual-node update (models/GNNs.py:196-199,227-230): one read of x, one write of out.  The walk of segment_rows.h: a sub-group
// of lanes owns one graph, lanes span the feature columns 16 B wide, four independent row loads in flight, rows are added
// in node order - bitwise reproducible, no atomics.  The work is driven by graph_ptr: a row at or beyond graph_ptr[G] (or
// *n_dyn) is neither read nor written, so the buffers may be longer than the batch (dataset.StaticBatch).
// The backward is the same entry: gx = gout + gp[g], gv[g] = sum_n gx[n] + gp[g].
#include "segment_rows.h"

namespace kpgnn {
namespace {

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
__global__ void __launch_bounds__(kRowBlock) vn_add_pool_kernel(VnParams p) {
    p.N = live_rows(p.N, p.n_dyn);
    const int sg = threadIdx.x / L, sl = threadIdx.x % L, c0 = sl * VEC;
    const int64_t g = (int64_t)blockIdx.x * (kRowBlock / L) + sg;
    if (g >= p.G || c0 >= p.D) return;
    const GraphRows rows = graph_rows(p.ptr, g, p.N);       // (never past the live rows, whatever the pointer says)
    float vg[VEC], acc[VEC];
    ldv<VEC>(p.v + g * p.vs + c0, vg);
    for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
    for_graph_rows<VEC>(p.x, p.xs, c0, rows.beg, rows.end, [&](float (&w)[VEC], int r) {
        for (int q = 0; q < VEC; ++q) { w[q] += vg[q]; acc[q] += w[q]; }
        stv<VEC>(p.out + (int64_t)r * p.os + c0, w);
    });
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
    VnParams p = {};
    p.n_dyn = d->n_dyn; p.N = d->N; p.G = d->G; p.D = d->D; p.ptr = d->graph_ptr;
    p.x = d->x; p.xs = d->x_stride; p.v = d->v; p.vs = d->v_stride; p.out = d->out; p.os = d->out_stride; p.pooled = d->pooled;
    return launch_row_walk(d->D, {d->x, d->v, d->out, d->pooled}, {d->x_stride, d->v_stride, d->out_stride}, who,
                           "vn_add_pool_kernel", graph_grid, d->G, p, (hipStream_t)stream,
                           [](auto V, auto L) { return vn_add_pool_kernel<V.value, L.value>; });
}
