// The bodies' resistance-distance projection out = x + rd w^T + b and the gradients of w and b (gfx950).  Contract:
// include/kpgnn.h, kpgnn_rd_proj_fwd / _bwd.
//
// models/GNNs.py adds `self.rd_projection(data.rd)`, an nn.Linear(1, H), to the encoded node rows: as framework code a
// [N,1] x [1,H] matrix product, a bias add and the residual add forward, and backward two reductions over ALL rows of the
// tensor - the dead rows of a capacity-shaped batch included.  Here:
//   fwd  one streaming launch on the shared row shapes (a group of G lanes owns a row, VEC columns per lane, w and b in
//        registers), live rows only;
//   bwd  rd_stats_kernel: the statistics block of column_stats.h over dy and rd * dy, one partial double[2][H] per block;
//        rd_finalize_kernel: one block adds the partials in block order and writes dw, db as fp32.
// Row r belongs to block (r / R) mod kMaxStatGrid whatever the capacity, R the rows of one block pass, and blocks without a
// live row contribute +0.0: the sums depend on the live rows alone.  dx is dy itself and costs nothing.  No atomics.
#include "column_stats.h"

namespace kpgnn {
namespace {

constexpr int kBlock = kRowBlock;
constexpr int kMaxH = 256;

struct RdProjParams {
    const int32_t* n_dyn;
    int64_t N; int H;
    const float* x; int64_t xs;
    const float* rd; const float* w; const float* b;
    float* out; int64_t os;
    const float* dy; int64_t ds;
    float* dw; float* db;
    double* part; int P, R;             // [P][2][H]; rows of one block pass
};

template <int VEC, int G>
__global__ void __launch_bounds__(kBlock) rd_fwd_kernel(const RdProjParams p) {
    constexpr int R = kBlock / G;
    const int64_t n = live_rows(p.N, p.n_dyn);
    const int lane = threadIdx.x % G, rg = threadIdx.x / G, c0 = lane * VEC;
    if (c0 >= p.H) return;
    float w[VEC], b[VEC];
    ldv<VEC>(p.w + c0, w);
    ldv<VEC>(p.b + c0, b);
    for (int64_t row = (int64_t)blockIdx.x * R + rg; row < n; row += (int64_t)gridDim.x * R) {
        float v[VEC];
        ldv<VEC>(p.x + row * p.xs + c0, v);
        const float r = p.rd[row];
#pragma unroll
        for (int q = 0; q < VEC; ++q) v[q] += fmaf(r, w[q], b[q]);
        stv<VEC>(p.out + row * p.os + c0, v);
    }
}

template <int VEC, int G>
__global__ void __launch_bounds__(kBlock) rd_stats_kernel(const RdProjParams p) {
    const int c0 = (int)(threadIdx.x % G) * VEC;
    // f = dy, m = rd[row] for every column (sum dy, sum rd dy); the step is NOT gridDim.x * R: a row's block does not depend
    // on the capacity
    column_stats_block<VEC, G>(live_rows(p.N, p.n_dyn), (int64_t)kMaxStatGrid * (kBlock / G), p.H, p.part,
                               [&](int64_t row, float (&f)[VEC], float (&m)[VEC]) {
        ldv<VEC>(p.dy + row * p.ds + c0, f);
        const float r = p.rd[row];
        for (int q = 0; q < VEC; ++q) m[q] = r;
    });
}

// Slice sl adds the blocks sl, sl + nsl, ... in order, then the slices are added in order; nsl depends on H alone, and only
// the blocks that can hold a live row are read (the others wrote +0.0, which changes no sum)
__global__ void __launch_bounds__(kFinBlock) rd_finalize_kernel(const RdProjParams p) {
    __shared__ double slice[kFinBlock];
    const int ncol = 2 * p.H, t = threadIdx.x;
    const int64_t n = live_rows(p.N, p.n_dyn);
    const int64_t need = (n + p.R - 1) / p.R;
    const int P = need < p.P ? (int)need : p.P;
    int nsl = kFinBlock / ncol;
    if (nsl > kMaxSlices) nsl = kMaxSlices;
    const int sl = t / ncol, col = t - sl * ncol;
    if (sl < nsl) {
        const double* q = p.part + col;
        double s = 0.0;
        for (int b = sl; b < P; b += nsl) s += q[(int64_t)b * ncol];
        slice[sl * ncol + col] = s;
    }
    __syncthreads();
    if (t < ncol) {
        double s = 0.0;
        for (int k = 0; k < nsl; ++k) s += slice[k * ncol + t];
        if (t < p.H) p.db[t] = (float)s;
        else p.dw[t - p.H] = (float)s;
    }
}

size_t workspace_bytes(int64_t N, int H) {      // (R >= 1 whatever the row shape turns out to be)
    return ((size_t)stat_blocks(N, 1) * 2 * H * sizeof(double) + 15) & ~(size_t)15;
}

int check_desc(const kpgnn_rd_proj_desc* d, const char* who) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->N >= 0 && d->H >= 1, "%s: bad N=%lld H=%d", who, (long long)d->N, d->H);
    if (d->H > kMaxH) return fail(KPGNN_ELIMIT, "%s: H=%d is wider than the %d columns the kernels cover", who, d->H, kMaxH);
    KPGNN_REQUIRE(d->N == 0 || d->rd != nullptr, "%s: NULL rd", who);
    return KPGNN_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" size_t kpgnn_rd_proj_workspace_bytes(int64_t N, int32_t H) {
    if (N < 0 || H < 1 || H > kMaxH) return 0;
    return workspace_bytes(N, H);
}

extern "C" int kpgnn_rd_proj_fwd(const kpgnn_rd_proj_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_rd_proj_fwd";
    if (int rc = check_desc(d, who)) return rc;
    KPGNN_REQUIRE(d->w != nullptr && d->b != nullptr, "%s: NULL w/b", who);
    if (d->N == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->x != nullptr && d->out != nullptr, "%s: NULL x/out", who);
    KPGNN_REQUIRE(d->x_stride >= d->H && d->out_stride >= d->H, "%s: x/out row stride shorter than H=%d", who, d->H);
    RdProjParams p = {};
    p.n_dyn = d->n_dyn; p.N = d->N; p.H = d->H; p.x = d->x; p.xs = d->x_stride; p.rd = d->rd; p.w = d->w; p.b = d->b;
    p.out = d->out; p.os = d->out_stride;
    const int vec = row_vec(p.H, {p.x, p.out, p.w, p.b}, {p.xs, p.os});
    const int g = row_lanes(p.H, vec), rows = kBlock / g;
    const int64_t blocks = (p.N + rows - 1) / rows;
    const unsigned grid = (unsigned)(blocks > kMaxApplyGrid ? kMaxApplyGrid : blocks);
    hipStream_t s = (hipStream_t)stream;
    return dispatch_row_shape<256>(vec, g, who, [&](auto V, auto L) {
        hipLaunchKernelGGL((rd_fwd_kernel<V.value, L.value>), dim3(grid), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("rd_fwd_kernel");
        return KPGNN_OK;
    });
}

extern "C" int kpgnn_rd_proj_bwd(const kpgnn_rd_proj_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_rd_proj_bwd";
    if (int rc = check_desc(d, who)) return rc;
    KPGNN_REQUIRE(d->dw != nullptr && d->db != nullptr, "%s: NULL dw/db", who);
    KPGNN_REQUIRE(d->N == 0 || (d->dy != nullptr && d->dy_stride >= d->H), "%s: NULL dy or row stride shorter than H=%d", who, d->H);
    KPGNN_REQUIRE(d->workspace != nullptr && ((uintptr_t)d->workspace & 7) == 0, "%s: NULL or misaligned workspace", who);
    KPGNN_REQUIRE(d->workspace_bytes >= workspace_bytes(d->N, d->H), "%s: workspace of %zu bytes, %zu needed", who,
                  d->workspace_bytes, workspace_bytes(d->N, d->H));
    RdProjParams p = {};
    p.n_dyn = d->n_dyn; p.N = d->N; p.H = d->H; p.rd = d->rd; p.dy = d->dy; p.ds = d->dy_stride; p.dw = d->dw; p.db = d->db;
    p.part = reinterpret_cast<double*>(d->workspace);
    const int vec = row_vec(p.H, {p.dy}, {p.ds});
    const int g = row_lanes(p.H, vec);
    p.R = kBlock / g;
    p.P = stat_blocks(p.N, p.R);
    hipStream_t s = (hipStream_t)stream;
    return dispatch_row_shape<256>(vec, g, who, [&](auto V, auto L) {
        hipLaunchKernelGGL((rd_stats_kernel<V.value, L.value>), dim3((unsigned)p.P), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("rd_stats_kernel");
        hipLaunchKernelGGL(rd_finalize_kernel, dim3(1), dim3(kFinBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("rd_finalize_kernel");
        return KPGNN_OK;
    });
}
