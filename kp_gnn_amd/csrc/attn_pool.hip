// Attention readout: out[g,:] = sum_n softmax_g(x[n] . w + b) x[n,:] over the nodes of graph g, and its backward (gfx950).
// Contract: include/kpgnn.h, kpgnn_attn_pool_fwd / _bwd.  Replaces PyG's AttentionalAggregation(gate_nn = nn.Linear(H, 1))
// (models/GraphClassification.py:31-32,51; train_graph_property.py:149 makes it the default readout), which the framework
// runs as a [N,H] x [H,1] library GEMM, a scatter-max, a gather, an exp, a scatter-add with fp32 atomics, a divide, a
// multiply and a second atomic scatter-add, and as many again in backward.  Collated batches keep the nodes of a graph
// contiguous, so, as in segment_rows.h, a sub-group of lanes owns one graph and its lanes span the feature columns.  Forward:
// ONE pass over the graph's rows with a running maximum (gate, online max / sum of exponentials and the weighted row sum
// all come from the one load of x[n,:]); the gates are parked in alpha[] and turned into weights by a second pass over
// those N floats only.  Backward: the same walk gives gx and per-graph sums of dgate[n] x[n,:]; the sub-groups of a block meet
// in LDS in a fixed order and leave one partial row per block, which a slab_reduce launch adds in block order.  No atomics:
// bitwise reproducible.
// The lane-group-per-graph shape is tuned for collated molecule-size graphs (tens of nodes, hundreds of graphs); the
// result is correct for any graph size, but one graph of many thousand nodes is walked by a single sub-group.
#include "segment_rows.h"

namespace kpgnn {
namespace {

constexpr int kBlock = kRowBlock;
constexpr int kMaxD = 256;

struct AttnPoolParams {
    const int32_t* n_dyn;
    int64_t N; int G, D;
    const int32_t* ptr;
    const float* x; int64_t xs;
    const float* w; const float* bias;
    float* alpha; float* out;
    const float* gout; float* gx; int64_t gxs;
    float* dwp; float* dbp; int64_t part_stride;     // block b leaves its partial dw at dwp + b * part_stride (db likewise)
};

// Chunks of L * VEC columns a lane walks: sub-groups stay inside a wave (L <= 64), so rows wider than 64 * VEC take several.
template <int VEC, int L> constexpr int chunks() { return L < 64 ? 1 : (VEC == 4 ? 1 : (VEC == 2 ? 2 : 4)); }

template <int VEC, int L>
__global__ void __launch_bounds__(kBlock) attn_pool_fwd_kernel(AttnPoolParams p) {
    constexpr int NCH = chunks<VEC, L>();
    const int64_t N = live_rows(p.N, p.n_dyn);
    const int sg = threadIdx.x / L, sl = threadIdx.x % L;
    const int64_t g = (int64_t)blockIdx.x * (kBlock / L) + sg;
    if (g >= p.G) return;                                     // (whole sub-groups leave: the shuffles below stay inside one)
    const GraphRows rows = graph_rows(p.ptr, g, N);
    const int beg = rows.beg, end = rows.end;
    const float b0 = p.bias ? p.bias[0] : 0.f;
    float w[NCH][VEC], acc[NCH][VEC];
    bool on[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = (j * L + sl) * VEC;
        on[j] = c < p.D;
        for (int q = 0; q < VEC; ++q) { w[j][q] = 0.f; acc[j][q] = 0.f; }
        if (on[j]) ldv<VEC>(p.w + c, w[j]);
    }
    float mx = -INFINITY, se = 0.f;
    for (int r0 = beg; r0 < end; r0 += 2) {                  // two independent rows in flight, folded in row order
        const int nr = end - r0 < 2 ? end - r0 : 2;
        float v[2][NCH][VEC], gate[2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                for (int q = 0; q < VEC; ++q) v[u][j][q] = 0.f;
                if (u < nr && on[j]) ldv<VEC>(p.x + (int64_t)(r0 + u) * p.xs + (j * L + sl) * VEC, v[u][j]);
            }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                for (int q = 0; q < VEC; ++q) d = fmaf(v[u][j][q], w[j][q], d);
            gate[u] = group_sum<L>(d) + b0;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u >= nr) continue;
            const int r = r0 + u;
            if (sl == ((r - beg) & (L - 1))) p.alpha[r] = gate[u];      // (the lane that rewrites it below)
            const float nm = fmaxf(mx, gate[u]);
            const float keep = expf(mx - nm), pr = expf(gate[u] - nm);   // (first row: exp(-inf) = 0)
            se = fmaf(se, keep, pr);
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                for (int q = 0; q < VEC; ++q) acc[j][q] = fmaf(acc[j][q], keep, pr * v[u][j][q]);
            mx = nm;
        }
    }
    const float inv = 1.0f / (se + 1e-16f);                   // (an empty graph: acc = 0, a zero row)
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        for (int q = 0; q < VEC; ++q) acc[j][q] *= inv;
        if (on[j]) stv<VEC>(p.out + g * p.D + (j * L + sl) * VEC, acc[j]);
    }
    for (int r = beg + sl; r < end; r += L) p.alpha[r] = expf(p.alpha[r] - mx) * inv;
}

template <int VEC, int L>
__global__ void __launch_bounds__(kBlock) attn_pool_bwd_kernel(AttnPoolParams p) {
    constexpr int NCH = chunks<VEC, L>();
    constexpr int S = kBlock / L, W = L * VEC * NCH;           // sub-groups of a block, columns they span
    __shared__ float red[S][W + 1];
    __shared__ float redb[S];
    const int64_t N = live_rows(p.N, p.n_dyn);
    const int sg = threadIdx.x / L, sl = threadIdx.x % L;
    const int64_t g = (int64_t)blockIdx.x * S + sg;
    float dwa[NCH][VEC];
    float dba = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
        for (int q = 0; q < VEC; ++q) dwa[j][q] = 0.f;
    if (g < p.G) {
        const GraphRows rows = graph_rows(p.ptr, g, N);
        const int beg = rows.beg, end = rows.end;
        float w[NCH][VEC], go[NCH][VEC];
        bool on[NCH];
        float sdot = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c = (j * L + sl) * VEC;
            on[j] = c < p.D;
            float o[VEC];
            for (int q = 0; q < VEC; ++q) { w[j][q] = 0.f; go[j][q] = 0.f; o[q] = 0.f; }
            if (on[j] && end > beg) {
                ldv<VEC>(p.w + c, w[j]);
                ldv<VEC>(p.gout + g * p.D + c, go[j]);
                ldv<VEC>(p.out + g * p.D + c, o);
            }
            for (int q = 0; q < VEC; ++q) sdot = fmaf(go[j][q], o[q], sdot);
        }
        sdot = group_sum<L>(sdot);                            // s_g = gout[g] . out[g]
        for (int r0 = beg; r0 < end; r0 += 2) {
            const int nr = end - r0 < 2 ? end - r0 : 2;
            float v[2][NCH][VEC], a[2], dg[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                a[u] = u < nr ? p.alpha[r0 + u] : 0.f;
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    for (int q = 0; q < VEC; ++q) v[u][j][q] = 0.f;
                    if (u < nr && on[j]) ldv<VEC>(p.x + (int64_t)(r0 + u) * p.xs + (j * L + sl) * VEC, v[u][j]);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float d = 0.f;
#pragma unroll
                for (int j = 0; j < NCH; ++j)
                    for (int q = 0; q < VEC; ++q) d = fmaf(v[u][j][q], go[j][q], d);
                dg[u] = a[u] * (group_sum<L>(d) - sdot);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (u >= nr) continue;
                dba += dg[u];
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    float o[VEC];
                    for (int q = 0; q < VEC; ++q) {
                        dwa[j][q] = fmaf(dg[u], v[u][j][q], dwa[j][q]);
                        o[q] = fmaf(dg[u], w[j][q], a[u] * go[j][q]);
                    }
                    if (p.gx && on[j]) stv<VEC>(p.gx + (int64_t)(r0 + u) * p.gxs + (j * L + sl) * VEC, o);
                }
            }
        }
    }
    // the block's partial: its sub-groups (graphs) in order
#pragma unroll
    for (int j = 0; j < NCH; ++j)
        for (int q = 0; q < VEC; ++q) red[sg][(j * L + sl) * VEC + q] = dwa[j][q];
    if (sl == 0) redb[sg] = dba;
    __syncthreads();
    for (int c = threadIdx.x; c < p.D; c += kBlock) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < S; ++k) s += red[k][c];
        p.dwp[blockIdx.x * p.part_stride + c] = s;
    }
    if (p.dbp && threadIdx.x == 0) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < S; ++k) s += redb[k];
        p.dbp[blockIdx.x * p.part_stride] = s;
    }
}

int shape(int D, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> strides, int* vec, int* lanes) {
    if (D > kMaxD) return fail(KPGNN_ELIMIT, "attn_pool: D=%d exceeds %d columns", D, kMaxD);
    *vec = row_vec(D, ptrs, strides);
    *lanes = row_lanes(D, *vec);
    if (*lanes > kWave) *lanes = kWave;                       // (wider rows: chunks<VEC, 64>() passes of the same lanes)
    return KPGNN_OK;
}

int check(const kpgnn_attn_pool_desc* d, const char* who) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->N >= 0 && d->G >= 0 && d->D >= 1, "%s: bad N=%lld G=%d D=%d", who, (long long)d->N, d->G, d->D);
    KPGNN_REQUIRE(d->G == 0 || d->graph_ptr, "%s: NULL graph_ptr", who);
    KPGNN_REQUIRE(d->w && d->out && (d->N == 0 || (d->x && d->alpha)), "%s: NULL x/w/alpha/out", who);
    KPGNN_REQUIRE(d->N == 0 || d->x_stride >= d->D, "%s: x_stride=%lld below D=%d", who, (long long)d->x_stride, d->D);
    return KPGNN_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" size_t kpgnn_attn_pool_workspace_bytes(int32_t G, int32_t D) {
    if (G < 1 || D < 1 || D > kMaxD) return 0;
    int lanes = row_lanes(D, 1);                              // the fewest graphs per block any row shape gives
    if (lanes > kWave) lanes = kWave;
    return (size_t)graph_grid(G, lanes) * (size_t)(D + 1) * sizeof(float);
}

extern "C" int kpgnn_attn_pool_fwd(const kpgnn_attn_pool_desc* d, kpgnn_stream_t stream) {
    int rc = check(d, "attn_pool_fwd");
    if (rc != KPGNN_OK) return rc;
    int vec, lanes;
    rc = shape(d->D, {d->x, d->w, d->out}, {d->x_stride}, &vec, &lanes);
    if (rc != KPGNN_OK) return rc;
    if (d->G == 0) return KPGNN_OK;
    AttnPoolParams p = {};
    p.n_dyn = d->n_dyn; p.N = d->N; p.G = d->G; p.D = d->D; p.ptr = d->graph_ptr; p.x = d->x; p.xs = d->x_stride;
    p.w = d->w; p.bias = d->bias; p.alpha = d->alpha; p.out = d->out;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = graph_grid(d->G, lanes);
    return dispatch_row_shape<64>(vec, lanes, "attn_pool_fwd", [&](auto V, auto L) {
        hipLaunchKernelGGL((attn_pool_fwd_kernel<V.value, L.value>), dim3(grid), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("attn_pool_fwd_kernel");
        return KPGNN_OK;
    });
}

extern "C" int kpgnn_attn_pool_bwd(const kpgnn_attn_pool_desc* d, kpgnn_stream_t stream) {
    int rc = check(d, "attn_pool_bwd");
    if (rc != KPGNN_OK) return rc;
    KPGNN_REQUIRE(d->dw && (d->G == 0 || d->gout) && (!d->gx || d->gx_stride >= d->D), "attn_pool_bwd: NULL gout/dw or bad gx stride");
    int vec, lanes;
    rc = shape(d->D, {d->x, d->w, d->out, d->gout, d->gx}, {d->x_stride, d->gx ? d->gx_stride : 0}, &vec, &lanes);
    if (rc != KPGNN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int grid = (int)graph_grid(d->G, lanes);
    if (grid == 0) {                                          // no graph: the parameter gradients are zero
        KPGNN_HIP_TRY(hipMemsetAsync(d->dw, 0, sizeof(float) * d->D, s));
        if (d->db) KPGNN_HIP_TRY(hipMemsetAsync(d->db, 0, sizeof(float), s));
        return KPGNN_OK;
    }
    AttnPoolParams p = {};
    p.n_dyn = d->n_dyn; p.N = d->N; p.G = d->G; p.D = d->D; p.ptr = d->graph_ptr; p.x = d->x; p.xs = d->x_stride;
    p.w = d->w; p.alpha = d->alpha; p.out = d->out; p.gout = d->gout; p.gx = d->gx; p.gxs = d->gx_stride;
    float* slab = (float*)d->workspace;
    if (grid == 1) {                                          // one block holds every graph: its partial IS the gradient
        p.dwp = d->dw; p.dbp = d->db; p.part_stride = 0;
    } else {
        KPGNN_REQUIRE(slab && d->workspace_bytes >= (size_t)grid * (d->D + 1) * sizeof(float),
                      "attn_pool_bwd: workspace of %zu bytes, %zu needed", d->workspace_bytes, (size_t)grid * (d->D + 1) * sizeof(float));
        p.part_stride = d->D + (d->db ? 1 : 0);
        p.dwp = slab; p.dbp = d->db ? slab + d->D : nullptr;
    }
    rc = dispatch_row_shape<64>(vec, lanes, "attn_pool_bwd", [&](auto V, auto L) {
        hipLaunchKernelGGL((attn_pool_bwd_kernel<V.value, L.value>), dim3((unsigned)grid), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("attn_pool_bwd_kernel");
        return KPGNN_OK;
    });
    if (rc != KPGNN_OK || grid == 1) return rc;
    return slab_reduce(slab, grid, p.part_stride, d->dw, d->D, d->db, d->db ? 1 : 0, nullptr, s);
}
