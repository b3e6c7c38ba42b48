// The bodies' Layer, Instance, GraphSize and Pair norms (+ residual) and their backward passes (gfx950).  Contract:
// include/kpgnn.h, kpgnn_body_norm_fwd / _bwd.
//
// models/GNNs.py:103-112 builds one PyG norm per layer from --norm_type and calls it without a batch vector, so the whole batch
// is one graph.  All four, in both directions, are the same three steps: two column sums over the live rows (x and x^2 forward,
// gout and gout * x backward), a handful of per-column coefficients derived from them, and one streaming pass over the rows.
//   1. norm_stats_kernel: the statistics block of column_stats.h, one partial double[2][C] per block; block b owns the rows
//      b * R + group, then every gridDim.x * R rows.
//   2. norm_finalize_kernel: one block adds the partials in block order (contiguous slices of blocks, slices in order), reads the
//      live row count on the device, and leaves fp32 coefficients: `saved` forward, a [5][C] table in the workspace backward.
//   3. norm_apply_kernel: out = (x - m[c]) * s[c] * w[c] + b[c] (+ residual) forward, gx = P[c] (g - Gm[c]) + K[c] (x - m[c]) +
//      D[c] backward.  CENTRED on purpose: the folded a x + c turns a constant column, and the single row of N == 1, into
//      rounding noise scaled by 1 / sqrt(eps) = 316 where the answer is exactly 0.
// GraphSize needs no sums: one launch that reads the live count itself.  No atomics anywhere: the same inputs at the same
// capacity give the same bits.  Bound by bytes: 4 N C read per statistics pass and 8 .. 12 N C moved per apply pass.
#include "column_stats.h"

#include <cmath>

namespace kpgnn {
namespace {

constexpr int kBlock = kRowBlock;
constexpr int kMaxC = 256;           // a row fits one pass of the widest row shape, and one finalize thread per column
constexpr int kStatRows = 32;        // capacity rows per statistics block until the grid stops growing
constexpr int kCoef = 5;             // backward coefficient rows: m, P, Gm, K, D

enum { APPLY_FWD = 0, APPLY_BWD = 1, APPLY_SCALE = 2 };

struct NormParams {
    const int32_t* n_dyn;
    int64_t N; int C, kind; float eps;
    const float* x; int64_t xs;
    const float* g; int64_t gs;         // backward: gout
    const float* res; int64_t rs;
    const float* w; const float* b;
    float* out; int64_t os;             // forward: out; backward: gx
    float* saved;
    float* gw; float* gb;
    double* part; int P;                // [P][2][C]
    float* coef;                        // backward: [kCoef][C]
};

template <int BWD, int VEC, int G>
__global__ void __launch_bounds__(kBlock) norm_stats_kernel(const NormParams p) {
    const int c0 = (int)(threadIdx.x % G) * VEC;
    // f = m = x forward (sum x, sum x^2); f = gout, m = x backward (sum g, sum g x)
    column_stats_block<VEC, G>(live_rows(p.N, p.n_dyn), (int64_t)gridDim.x * (kBlock / G), p.C, p.part,
                               [&](int64_t row, float (&f)[VEC], float (&m)[VEC]) {
        ldv<VEC>(p.x + row * p.xs + c0, m);
        if (BWD) ldv<VEC>(p.g + row * p.gs + c0, f);
        else for (int j = 0; j < VEC; ++j) f[j] = m[j];
    });
}

// red[0][0], red[1][0] = the sums of red[0][0 .. 255], red[1][0 .. 255] in a fixed tree; every thread of the block calls
__device__ __forceinline__ void tree_sums(double (*red)[kMaxC]) {
    for (int s = kMaxC / 2; s > 0; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
    }
    __syncthreads();
}

template <int BWD>
__global__ void __launch_bounds__(kFinBlock) norm_finalize_kernel(const NormParams p) {
    __shared__ double slice[kFinBlock];         // [nsl][2 C]
    __shared__ double tot[2 * kMaxC];           // the two column sums
    __shared__ double red[2][kMaxC];
    const int C = p.C, ncol = 2 * C, t = threadIdx.x;
    const int64_t n = live_rows(p.N, p.n_dyn);
    const double dn = n > 0 ? (double)n : 1.0;
    int nsl = kFinBlock / ncol;
    if (nsl > kMaxSlices) nsl = kMaxSlices;
    if (nsl > p.P) nsl = p.P;
    {   // partials in block order: slice sl adds its contiguous run of blocks, then the slices are added in order
        const int sl = t / ncol, col = t - sl * ncol;
        if (sl < nsl) {
            const int per = (p.P + nsl - 1) / nsl;
            int b = sl * per, e = b + per < p.P ? b + per : p.P;
            const double* q = p.part + col;
            double s = 0.0;
            for (; b + 3 < e; b += 4) {
                const double v0 = q[(int64_t)b * ncol], v1 = q[(int64_t)(b + 1) * ncol];
                const double v2 = q[(int64_t)(b + 2) * ncol], v3 = q[(int64_t)(b + 3) * ncol];
                s += v0; s += v1; s += v2; s += v3;
            }
            for (; b < e; ++b) s += q[(int64_t)b * ncol];
            slice[sl * ncol + col] = s;
        }
        __syncthreads();
        if (t < ncol) {
            double s = 0.0;
            for (int k = 0; k < nsl; ++k) s += slice[k * ncol + t];
            tot[t] = s;
        }
        __syncthreads();
    }
    const int c = t;
    const bool col_ok = c < C;
    const double T0 = col_ok ? tot[c] : 0.0, T1 = col_ok ? tot[C + c] : 0.0;
    const double eps = (double)p.eps;
    if (!BWD) {
        // T0 = sum x, T1 = sum x^2
        if (p.kind == KPGNN_NORM_LAYER) {
            if (t < kMaxC) { red[0][t] = T0; red[1][t] = T1; }
            tree_sums(red);
            const double nc = dn * C, mu = red[0][0] / nc;
            double var = red[1][0] / nc - mu * mu;
            var = var > 0.0 ? var : 0.0;
            const double sd = sqrt(var), s = 1.0 / (sd + eps);
            if (col_ok) { p.saved[c] = (float)mu; p.saved[C + c] = (float)s; }
            if (t == 0) { p.saved[2 * C] = (float)mu; p.saved[2 * C + 1] = (float)s; p.saved[2 * C + 2] = (float)sd; p.saved[2 * C + 3] = (float)n; }
        } else if (p.kind == KPGNN_NORM_INSTANCE) {
            const double m = T0 / dn;
            double var = T1 / dn - m * m;
            var = var > 0.0 ? var : 0.0;
            if (col_ok) { p.saved[c] = (float)m; p.saved[C + c] = (float)(1.0 / sqrt(var + eps)); }
            if (t == 0) { p.saved[2 * C] = 0.f; p.saved[2 * C + 1] = 0.f; p.saved[2 * C + 2] = 0.f; p.saved[2 * C + 3] = (float)n; }
        } else {    // KPGNN_NORM_PAIR
            const double m = T0 / dn;
            double ss = T1 - dn * m * m;            // sum over the rows of (x - m)^2
            ss = ss > 0.0 ? ss : 0.0;
            if (t < kMaxC) { red[0][t] = ss; red[1][t] = 0.0; }
            tree_sums(red);
            const double r = 1.0 / sqrt(eps + red[0][0] / dn);
            if (col_ok) { p.saved[c] = (float)m; p.saved[C + c] = (float)r; }
            if (t == 0) { p.saved[2 * C] = 0.f; p.saved[2 * C + 1] = (float)r; p.saved[2 * C + 2] = 0.f; p.saved[2 * C + 3] = (float)n; }
        }
        return;
    }
    // T0 = A = sum g, T1 = B = sum g x; the forward's fp32 coefficients are the function that is differentiated
    float* cm = p.coef, *cP = p.coef + C, *cG = p.coef + 2 * C, *cK = p.coef + 3 * C, *cD = p.coef + 4 * C;
    if (p.kind == KPGNN_NORM_LAYER) {
        const double mu = (double)p.saved[2 * C], s = (double)p.saved[2 * C + 1], sd = (double)p.saved[2 * C + 2];
        const double w = col_ok ? (double)p.w[c] : 0.0, cen = T1 - mu * T0;
        if (t < kMaxC) { red[0][t] = w * T0; red[1][t] = w * cen; }
        tree_sums(red);
        const double nc = dn * C, sgh = red[0][0], sghxc = red[1][0];
        const double k = sd > 0.0 ? -s * s * sghxc / (nc * sd) : 0.0;
        if (col_ok) {
            cm[c] = (float)mu; cP[c] = (float)(s * w); cG[c] = 0.f; cK[c] = (float)k; cD[c] = (float)(-s * sgh / nc);
            if (p.gw) p.gw[c] = (float)(s * cen);
            if (p.gb) p.gb[c] = (float)T0;
        }
    } else if (p.kind == KPGNN_NORM_INSTANCE) {
        if (col_ok) {
            const double m = (double)p.saved[c], s = (double)p.saved[C + c];
            const double q = s * (T1 - m * T0) / dn;
            cm[c] = (float)m; cP[c] = (float)s; cG[c] = (float)(T0 / dn); cK[c] = (float)(-s * s * q); cD[c] = 0.f;
        }
    } else {        // KPGNN_NORM_PAIR
        const double m = col_ok ? (double)p.saved[c] : 0.0, r = (double)p.saved[2 * C + 1];
        if (t < kMaxC) { red[0][t] = T1 - m * T0; red[1][t] = 0.0; }
        tree_sums(red);
        const double k = -r * r * r * red[0][0] / dn;
        if (col_ok) { cm[c] = (float)m; cP[c] = (float)r; cG[c] = (float)(T0 / dn); cK[c] = (float)k; cD[c] = 0.f; }
    }
}

template <int MODE, int VEC, int G>
__global__ void __launch_bounds__(kBlock) norm_apply_kernel(const NormParams p) {
    constexpr int R = kBlock / G;
    const int64_t n = live_rows(p.N, p.n_dyn);
    const int C = p.C, lane = threadIdx.x % G, rg = threadIdx.x / G, c0 = lane * VEC;
    if (MODE == APPLY_SCALE && p.saved && blockIdx.x == 0) {        // (GraphSize forward: the coefficients for the record)
        const float s = n > 0 ? 1.0f / sqrtf((float)n) : 0.f;
        for (int i = threadIdx.x; i < 2 * C + 4; i += kBlock)
            p.saved[i] = i < C ? 0.f : (i < 2 * C || i == 2 * C + 1) ? s : (i == 2 * C + 3 ? (float)n : 0.f);
    }
    if (c0 >= C) return;
    // this thread's columns never change: their coefficients stay in registers over the row loop
    float m[VEC], s[VEC], w[VEC], b[VEC], k[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { m[j] = 0.f; s[j] = 1.f; w[j] = 1.f; b[j] = 0.f; k[j] = 0.f; }
    float sq = 1.f;
    if (MODE == APPLY_FWD) {
        ldv<VEC>(p.saved + c0, m);
        ldv<VEC>(p.saved + C + c0, s);
        if (p.w) ldv<VEC>(p.w + c0, w);
        if (p.b) ldv<VEC>(p.b + c0, b);
    } else if (MODE == APPLY_BWD) {
        ldv<VEC>(p.coef + c0, m);               // m
        ldv<VEC>(p.coef + C + c0, s);           // P
        ldv<VEC>(p.coef + 2 * C + c0, w);       // Gm
        ldv<VEC>(p.coef + 3 * C + c0, k);       // K
        ldv<VEC>(p.coef + 4 * C + c0, b);       // D
    } else {
        sq = sqrtf((float)n);
    }
    for (int64_t row = (int64_t)blockIdx.x * R + rg; row < n; row += (int64_t)gridDim.x * R) {
        float v[VEC], o[VEC];
        ldv<VEC>(p.x + row * p.xs + c0, v);
        if (MODE == APPLY_FWD) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] = fmaf((v[j] - m[j]) * s[j], w[j], b[j]);
        } else if (MODE == APPLY_BWD) {
            float g[VEC];
            ldv<VEC>(p.g + row * p.gs + c0, g);
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] = fmaf(k[j], v[j] - m[j], fmaf(s[j], g[j] - w[j], b[j]));
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] = v[j] / sq;
        }
        if (MODE != APPLY_BWD && p.res) {
            float r[VEC];
            ldv<VEC>(p.res + row * p.rs + c0, r);
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] += r[j];
        }
        stv<VEC>(p.out + row * p.os + c0, o);
    }
}

size_t workspace_bytes(int64_t N, int C) {
    const size_t b = (size_t)stat_blocks(N, kStatRows) * 2 * C * sizeof(double) + (size_t)kCoef * C * sizeof(float);
    return (b + 15) & ~(size_t)15;
}

int check_desc(const kpgnn_norm_desc* d, const char* who) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->N >= 0 && d->C >= 1, "%s: bad N=%lld C=%d", who, (long long)d->N, d->C);
    if (d->C > kMaxC) return fail(KPGNN_ELIMIT, "%s: C=%d is wider than the %d columns the norm kernels cover", who, d->C, kMaxC);
    KPGNN_REQUIRE(d->kind >= KPGNN_NORM_LAYER && d->kind <= KPGNN_NORM_PAIR, "%s: unknown kind %d", who, d->kind);
    KPGNN_REQUIRE(d->eps >= 0.f, "%s: bad eps=%g", who, (double)d->eps);     // (a NaN fails too)
    KPGNN_REQUIRE(d->x != nullptr && d->saved != nullptr, "%s: NULL x/saved", who);
    KPGNN_REQUIRE(d->x_stride >= d->C, "%s: x row stride shorter than C=%d", who, d->C);
    KPGNN_REQUIRE(d->kind != KPGNN_NORM_LAYER || d->weight != nullptr, "%s: NULL weight (LAYER)", who);
    KPGNN_REQUIRE(d->workspace != nullptr && ((uintptr_t)d->workspace & 7) == 0, "%s: NULL or misaligned workspace", who);
    KPGNN_REQUIRE(d->workspace_bytes >= workspace_bytes(d->N, d->C), "%s: workspace of %zu bytes, %zu needed", who,
                  d->workspace_bytes, workspace_bytes(d->N, d->C));
    return KPGNN_OK;
}

NormParams params_of(const kpgnn_norm_desc* d) {
    NormParams p = {};
    p.n_dyn = d->n_dyn; p.N = d->N; p.C = d->C; p.kind = d->kind; p.eps = d->eps;
    p.x = d->x; p.xs = d->x_stride;
    if (d->kind == KPGNN_NORM_LAYER) { p.w = d->weight; p.b = d->bias; }
    p.saved = d->saved;
    p.P = stat_blocks(d->N, kStatRows);
    p.part = reinterpret_cast<double*>(d->workspace);
    p.coef = reinterpret_cast<float*>(p.part + (size_t)p.P * 2 * d->C);
    return p;
}

// the up to three launches of one direction; `p` describes a centred pass (MODE) or the GraphSize scaling
template <int BWD>
int norm_launch(const NormParams& p, int vec, hipStream_t s) {
    const char* who = BWD ? "kpgnn_body_norm_bwd" : "kpgnn_body_norm_fwd";
    const int g = row_lanes(p.C, vec);
    const int rows = kBlock / g;
    const int64_t blocks = (p.N + rows - 1) / rows;
    const unsigned grid = (unsigned)(blocks > kMaxApplyGrid ? kMaxApplyGrid : blocks);
    if (p.kind == KPGNN_NORM_GRAPHSIZE)
        return dispatch_row_shape<256>(vec, g, who, [&](auto V, auto L) {
            hipLaunchKernelGGL((norm_apply_kernel<APPLY_SCALE, V.value, L.value>), dim3(grid), dim3(kBlock), 0, s, p);
            KPGNN_LAUNCH_CHECK("norm_apply_kernel<scale>");
            return KPGNN_OK;
        });
    return dispatch_row_shape<256>(vec, g, who, [&](auto V, auto L) {
        hipLaunchKernelGGL((norm_stats_kernel<BWD, V.value, L.value>), dim3((unsigned)p.P), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("norm_stats_kernel");
        hipLaunchKernelGGL((norm_finalize_kernel<BWD>), dim3(1), dim3(kFinBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("norm_finalize_kernel");
        hipLaunchKernelGGL((norm_apply_kernel<BWD ? APPLY_BWD : APPLY_FWD, V.value, L.value>), dim3(grid), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("norm_apply_kernel");
        return KPGNN_OK;
    });
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" size_t kpgnn_body_norm_workspace_bytes(int64_t N, int32_t C) {
    if (N < 0 || C < 1 || C > kMaxC) return 0;
    return workspace_bytes(N, C);
}

extern "C" int kpgnn_body_norm_fwd(const kpgnn_norm_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_body_norm_fwd";
    if (int rc = check_desc(d, who)) return rc;
    KPGNN_REQUIRE(d->out != nullptr, "%s: NULL out", who);
    KPGNN_REQUIRE(d->out_stride >= d->C, "%s: out row stride shorter than C=%d", who, d->C);
    KPGNN_REQUIRE(!d->residual || d->res_stride >= d->C, "%s: residual row stride shorter than C=%d", who, d->C);
    if (d->N == 0) return KPGNN_OK;
    NormParams p = params_of(d);
    p.out = d->out; p.os = d->out_stride;
    if (d->residual) { p.res = d->residual; p.rs = d->res_stride; }
    const int vec = row_vec(p.C, {p.x, p.out, p.res, p.w, p.b, p.saved}, {p.xs, p.os, p.rs});
    return norm_launch<0>(p, vec, (hipStream_t)stream);
}

extern "C" int kpgnn_body_norm_bwd(const kpgnn_norm_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_body_norm_bwd";
    if (int rc = check_desc(d, who)) return rc;
    KPGNN_REQUIRE(d->gout != nullptr && d->gx != nullptr, "%s: NULL gout/gx", who);
    KPGNN_REQUIRE(d->gout_stride >= d->C && d->gx_stride >= d->C, "%s: gout/gx row stride shorter than C=%d", who, d->C);
    if (d->N == 0) return KPGNN_OK;
    NormParams p = params_of(d);
    p.out = d->gx; p.os = d->gx_stride;
    if (d->kind == KPGNN_NORM_GRAPHSIZE) {          // gx = gout / sqrt(n): the scaling pass over gout
        p.x = d->gout; p.xs = d->gout_stride;
        p.saved = nullptr;
    } else {
        p.g = d->gout; p.gs = d->gout_stride;
        p.gw = d->gweight; p.gb = d->gbias;
    }
    const int vec = row_vec(p.C, {p.x, p.g, p.out, p.coef}, {p.xs, p.gs, p.os});
    return norm_launch<1>(p, vec, (hipStream_t)stream);
}
