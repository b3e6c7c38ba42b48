// The bodies' Layer, Instance, GraphSize and Pair norms (+ residual) PER GRAPH, and their backward passes (gfx950).  Contract:
// include/kpgnn.h, kpgnn_graph_norm_fwd / _bwd.  body_norm.hip takes the whole batch as one graph, as the reference's bodies
// do; here graph g owns the rows [graph_ptr[g], min(graph_ptr[g+1], live)) and the formulas apply to them alone.
//
// One TEAM owns one graph from its statistics to its apply pass, one launch per direction:
//   * n < kBlockRows: a wavefront, eight graphs per block (blocks 0 .. SB-1, SB = ceil(G / 8)).  The wave walks the graph's rows
//     in row order; the second walk (apply) finds a molecule's 9 .. 37 rows in the cache, so the graph is read from HBM once.
//   * n >= kBlockRows: a block (blocks SB .. SB+G-1, one per graph; a block whose graph is of the other class leaves at once,
//     which costs no host read).  Wave w walks the rows r0 + w, r0 + w + 8, ...; the per-wave column sums meet in LDS and EVERY
//     thread adds them in wave order, so every wave holds the same bits without a broadcast.
// The class depends on n alone.  A lane owns the columns lane, lane + 64, ... (4-byte accesses, 256 B per wave and
// instruction): the layout - and with it every order of summation - depends on C alone, not on the alignment of the operands.
// Sums are double: rows in row order per column, then (block team) the waves in order, then (Layer, Pair) the columns by one
// xor butterfly, which leaves the same bits in every lane.  The coefficients stay in double, the apply pass is centred and in
// double, contraction is off for the whole file, and the result is rounded to fp32 once.  So THE BITS OF A GRAPH'S ROWS OF out
// AND gx DEPEND ON THAT GRAPH'S ROWS, C, kind, eps (weight, bias, residual) AND ON NOTHING ELSE.  No atomics.
//
// The backward does not read the forward's coefficients: it sums x, x^2, gout and gout * x in ONE walk and derives everything
// in double.  A two-row graph's gradient is a difference of nearly equal terms (Instance: s e (1 - a^2), 1 - a^2 ~ eps / var);
// coefficients rounded to fp32 lose it, and the rows have to be read for gout * x anyway.
// Layer's gweight / gbias are sums over all graphs: every team leaves a double partial [2][C] (a wave-team block the sum of its
// eight waves in wave order), and graph_norm_param_kernel adds the partials that were written in slot order.
#include "segment_rows.h"

#include <cmath>

#pragma clang fp contract(off)

namespace kpgnn {
namespace {

constexpr int kTeam = 512;                      // threads of a block
constexpr int kWaves = kTeam / kWave;           // wave teams of a block; waves of a block team
constexpr int kMaxC = 256;
constexpr int kMaxCpl = kMaxC / kWave;          // columns per lane
constexpr int kBlockRows = KPGNN_GRAPH_NORM_BLOCK_ROWS;
constexpr int kParamBlock = 256;
constexpr int kRowsInFlight = 8;                // rows a wave requests before it uses the first: a molecule is 9 .. 37 rows

struct GraphNormParams {
    const int32_t* n_dyn; const int32_t* ptr;
    int64_t N; int G, C, kind; float eps;
    const float* x; int64_t xs;
    const float* g; int64_t gs;         // backward: gout
    const float* res; int64_t rs;
    const float* w; const float* b;
    float* out; int64_t os;             // forward: out; backward: gx
    float* saved;                       // forward: [G][4] or NULL
    double* part;                       // backward, Layer: [SB + G][2][C] or NULL
    float* gw; float* gb;
    int SB;                             // wave-team blocks
};

__device__ __forceinline__ double wave_sum(double v) {      // the same bits in every lane
#pragma unroll
    for (int o = kWave >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// sum over the columns of a per-column value held as v[j] = column lane + 64 j
template <int CPL>
__device__ __forceinline__ double column_sum(const double (&v)[CPL], int lane, int C) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < CPL; ++j)
        if (lane + kWave * j < C) s += v[j];
    return wave_sum(s);
}

// a, b: this wave's column sums -> the team's, added in wave order by every thread (block teams only; every thread calls)
template <int CPL>
__device__ __forceinline__ void team_sum2(double (&a)[CPL], double (&b)[CPL], double* sm, int wave, int lane, int C) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = lane + kWave * j;
        if (c < C) { sm[(wave * 2 + 0) * kMaxC + c] = a[j]; sm[(wave * 2 + 1) * kMaxC + c] = b[j]; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = lane + kWave * j;
        if (c < C) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int q = 0; q < kWaves; ++q) { s0 += sm[(q * 2 + 0) * kMaxC + c]; s1 += sm[(q * 2 + 1) * kMaxC + c]; }
            a[j] = s0; b[j] = s1;
        }
    }
    __syncthreads();
}

// One team's graph.  BIG: the team is the block (wave `wave` of kWaves), else this wave alone.  Returns through gwc / gbc the
// graph's share of Layer's gweight / gbias per column (backward).
template <int BWD, int CPL, bool BIG>
__device__ __forceinline__ void team_graph(const GraphNormParams& p, int g, int beg, int end, int wave, int lane, double* sm,
                                           double (&gwc)[CPL], double (&gbc)[CPL]) {
    const int C = p.C, kind = p.kind;
    const int first = beg + (BIG ? wave : 0), step = BIG ? kWaves : 1;
    const double dn = (double)(end - beg), eps = (double)p.eps;
    const float* xin = BWD && kind == KPGNN_NORM_GRAPHSIZE ? p.g : p.x;         // (GraphSize backward scales gout)
    const int64_t xs = BWD && kind == KPGNN_NORM_GRAPHSIZE ? p.gs : p.xs;
    double sx[CPL], sxx[CPL], sg[CPL], sgx[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) sx[j] = sxx[j] = sg[j] = sgx[j] = 0.0;
    if (kind != KPGNN_NORM_GRAPHSIZE) {
        // kRowsInFlight rows' loads in flight, added in row order; a product of two fp32 values is exact in double.  A row
        // beyond the graph's end loads nothing and adds +0.0, which changes no bit of a sum that started at +0.0.
        auto add = [&](const float (&xv)[CPL], const float (&gv)[CPL]) {
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const double xd = (double)xv[j];
                sx[j] += xd; sxx[j] += xd * xd;
                if (BWD) { const double gd = (double)gv[j]; sg[j] += gd; sgx[j] += gd * xd; }
            }
        };
        auto load = [&](int r, float (&xv)[CPL], float (&gv)[CPL]) {
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const int c = lane + kWave * j;
                const bool ok = r < end && c < C;
                xv[j] = ok ? p.x[(int64_t)r * p.xs + c] : 0.f;
                gv[j] = BWD && ok ? p.g[(int64_t)r * p.gs + c] : 0.f;
            }
        };
        for (int r = first; r < end; r += kRowsInFlight * step) {
            float xv[kRowsInFlight][CPL], gv[kRowsInFlight][CPL];
#pragma unroll
            for (int q = 0; q < kRowsInFlight; ++q) load(r + q * step, xv[q], gv[q]);
#pragma unroll
            for (int q = 0; q < kRowsInFlight; ++q) add(xv[q], gv[q]);
        }
        if (BIG) {
            team_sum2<CPL>(sx, sxx, sm, wave, lane, C);
            if (BWD) team_sum2<CPL>(sg, sgx, sm, wave, lane, C);
        }
    }
    // forward: out = (x - M[j]) * P[j] + Bv[j] (+ residual); backward: gx = P[j] * (W[j] * gout - F[j]) + K[j] * (x - M[j]).
    // The backward keeps gout's mean INSIDE the bracket: for a one-row graph (Layer: a one-element block) it is the same
    // product as the row's own term, and the difference is exactly 0.
    double M[CPL], P[CPL], W[CPL], F[CPL], K[CPL], Bv[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) { M[j] = 0.0; P[j] = 1.0; W[j] = 1.0; F[j] = 0.0; K[j] = 0.0; Bv[j] = 0.0; }
    float rec[4] = {0.f, 0.f, 0.f, (float)dn};
    if (kind == KPGNN_NORM_LAYER) {
        const double nc = dn * (double)C, mu = column_sum<CPL>(sx, lane, C) / nc;
        double var = column_sum<CPL>(sxx, lane, C) / nc - mu * mu;
        var = var > 0.0 ? var : 0.0;
        const double sd = sqrt(var), s = 1.0 / (sd + eps);
        rec[0] = (float)mu; rec[1] = (float)s; rec[2] = (float)sd;
        double wv[CPL], gh[CPL], ghx[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = lane + kWave * j;
            wv[j] = c < C ? (double)p.w[c] : 0.0;
            if (!BWD) Bv[j] = c < C && p.b ? (double)p.b[c] : 0.0;
            const double cen = sgx[j] - mu * sg[j];             // sum over the rows of gout * (x - mu)
            gh[j] = wv[j] * sg[j]; ghx[j] = wv[j] * cen;
            gwc[j] = s * cen; gbc[j] = sg[j];
            M[j] = mu; P[j] = BWD ? s : s * wv[j]; W[j] = wv[j];
        }
        if (BWD) {
            const double sgh = column_sum<CPL>(gh, lane, C), sghxc = column_sum<CPL>(ghx, lane, C);
            const double k = sd > 0.0 ? -(s * s) * sghxc / (nc * sd) : 0.0;     // a constant block: no term through sd
#pragma unroll
            for (int j = 0; j < CPL; ++j) { K[j] = k; F[j] = sgh / nc; }
        }
    } else if (kind == KPGNN_NORM_INSTANCE) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const double m = sx[j] / dn;
            double var = sxx[j] / dn - m * m;
            var = var > 0.0 ? var : 0.0;
            const double s = 1.0 / sqrt(var + eps);
            M[j] = m; P[j] = s;
            if (BWD) { F[j] = sg[j] / dn; K[j] = -(s * s * s) * (sgx[j] - m * sg[j]) / dn; }
        }
    } else if (kind == KPGNN_NORM_PAIR) {
        double ss[CPL], gxc[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const double m = sx[j] / dn;
            double q = sxx[j] - dn * m * m;                     // sum over the rows of (x - m)^2
            ss[j] = q > 0.0 ? q : 0.0;
            gxc[j] = sgx[j] - m * sg[j];
            M[j] = m;
        }
        const double r = 1.0 / sqrt(eps + column_sum<CPL>(ss, lane, C) / dn);
        rec[1] = (float)r;
        double k = 0.0;
        if (BWD) k = -(r * r * r) * column_sum<CPL>(gxc, lane, C) / dn;
#pragma unroll
        for (int j = 0; j < CPL; ++j) { P[j] = r; if (BWD) { F[j] = sg[j] / dn; K[j] = k; } }
    } else {
        rec[1] = (float)(1.0 / sqrt(dn));
    }
    if (!BWD && p.saved && lane == 0 && (!BIG || wave == 0)) {
        float* sv = p.saved + (int64_t)g * 4;
        sv[0] = rec[0]; sv[1] = rec[1]; sv[2] = rec[2]; sv[3] = rec[3];
    }
    const double sq = sqrt(dn);
    // the second operand of a row: gout backward (not GraphSize, whose first operand it is), the residual forward
    const float* yin = BWD ? (kind == KPGNN_NORM_GRAPHSIZE ? nullptr : p.g) : p.res;
    const int64_t ys = BWD ? p.gs : p.rs;
    // every load of kRowsInFlight rows is issued before the first store: out may alias nothing, but the compiler cannot know
    for (int r0 = first; r0 < end; r0 += kRowsInFlight * step) {
        float xv[kRowsInFlight][CPL], yv[kRowsInFlight][CPL];
#pragma unroll
        for (int q = 0; q < kRowsInFlight; ++q) {
            const int r = r0 + q * step;
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const int c = lane + kWave * j;
                const bool ok = r < end && c < C;
                xv[q][j] = ok ? xin[(int64_t)r * xs + c] : 0.f;
                yv[q][j] = ok && yin ? yin[(int64_t)r * ys + c] : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < kRowsInFlight; ++q) {
            const int r = r0 + q * step;
            if (r >= end) break;
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const int c = lane + kWave * j;
                if (c >= C) continue;
                const double xd = (double)xv[q][j], yd = (double)yv[q][j];
                double o;
                if (kind == KPGNN_NORM_GRAPHSIZE) {
                    o = xd / sq;
                } else if (!BWD) {
                    o = (xd - M[j]) * P[j] + Bv[j];             // (Layer: P = s w, Bv = bias; contraction is off)
                } else {
                    o = P[j] * (W[j] * yd - F[j]) + K[j] * (xd - M[j]);
                }
                if (!BWD && yin) o += yd;
                p.out[(int64_t)r * p.os + c] = (float)o;
            }
        }
    }
}

template <int BWD, int CPL>
__global__ void __launch_bounds__(kTeam) graph_norm_kernel(const GraphNormParams p) {
    __shared__ double sm[kWaves * 2 * kMaxC];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, C = p.C;
    const bool big = (int)blockIdx.x >= p.SB;
    const int g = big ? (int)blockIdx.x - p.SB : (int)blockIdx.x * kWaves + wave;
    int beg = 0, end = 0;
    if (g < p.G) {
        const GraphRows gr = graph_rows(p.ptr, g, live_rows(p.N, p.n_dyn));
        beg = gr.beg; end = gr.end;
    }
    const int n = end - beg;
    const bool layer_params = BWD && p.part != nullptr;        // (set for Layer with a gweight or gbias alone)
    double gwc[CPL], gbc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) gwc[j] = gbc[j] = 0.0;
    if (big) {
        if (n < kBlockRows) return;                             // (block-uniform) the other class, or no such graph
        team_graph<BWD, CPL, true>(p, g, beg, end, wave, lane, sm, gwc, gbc);
        if (layer_params && wave == 0) {
            double* dst = p.part + (int64_t)blockIdx.x * 2 * C;
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const int c = lane + kWave * j;
                if (c < C) { dst[c] = gwc[j]; dst[C + c] = gbc[j]; }
            }
        }
        return;
    }
    if (n > 0 && n < kBlockRows) team_graph<BWD, CPL, false>(p, g, beg, end, wave, lane, sm, gwc, gbc);    // (wave-uniform)
    if (layer_params) {     // the block's partial: its waves in wave order, zeros for a wave without a graph of this class
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = lane + kWave * j;
            if (c < C) { sm[(wave * 2 + 0) * kMaxC + c] = gwc[j]; sm[(wave * 2 + 1) * kMaxC + c] = gbc[j]; }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < 2 * C; t += kTeam) {
            const int which = t / C, c = t - which * C;
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < kWaves; ++q) s += sm[(q * 2 + which) * kMaxC + c];
            p.part[(int64_t)blockIdx.x * 2 * C + t] = s;
        }
    }
}

// gweight[c], gbias[c] = the partials of column c in slot order: thread t adds the slots t, t + 256, ..., then a fixed tree.
// A block team's slot was written only where its graph is of that class: the same test as in graph_norm_kernel.
__global__ void __launch_bounds__(kParamBlock) graph_norm_param_kernel(const GraphNormParams p) {
    __shared__ double red[2][kParamBlock];
    const int c = blockIdx.x, C = p.C, t = threadIdx.x;
    const int64_t live = live_rows(p.N, p.n_dyn);
    double s0 = 0.0, s1 = 0.0;
    for (int slot = t; slot < p.SB + p.G; slot += kParamBlock) {
        if (slot >= p.SB) {
            const GraphRows gr = graph_rows(p.ptr, slot - p.SB, live);
            if (gr.end - gr.beg < kBlockRows) continue;
        }
        const double* q = p.part + (int64_t)slot * 2 * C;
        s0 += q[c]; s1 += q[C + c];
    }
    red[0][t] = s0; red[1][t] = s1;
    for (int s = kParamBlock / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) { red[0][t] += red[0][t + s]; red[1][t] += red[1][t + s]; }
    }
    if (t == 0) {
        if (p.gw) p.gw[c] = (float)red[0][0];
        if (p.gb) p.gb[c] = (float)red[1][0];
    }
}

inline int wave_blocks(int G) { return (G + kWaves - 1) / kWaves; }

size_t workspace_bytes(int G, int C, int kind) {
    if (kind != KPGNN_NORM_LAYER) return 0;
    return ((size_t)(wave_blocks(G) + G) * 2 * C * sizeof(double) + 15) & ~(size_t)15;
}

int check_desc(const kpgnn_graph_norm_desc* d, const char* who) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->N >= 0 && d->N <= INT32_MAX && d->G >= 0 && d->C >= 1, "%s: bad N=%lld G=%d C=%d", who, (long long)d->N,
                  d->G, d->C);
    if (d->C > kMaxC) return fail(KPGNN_ELIMIT, "%s: C=%d is wider than the %d columns the norm kernels cover", who, d->C, kMaxC);
    KPGNN_REQUIRE(d->kind >= KPGNN_NORM_LAYER && d->kind <= KPGNN_NORM_PAIR, "%s: unknown kind %d", who, d->kind);
    KPGNN_REQUIRE(d->eps >= 0.f, "%s: bad eps=%g", who, (double)d->eps);     // (a NaN fails too)
    KPGNN_REQUIRE(d->x != nullptr && d->graph_ptr != nullptr, "%s: NULL x/graph_ptr", who);
    KPGNN_REQUIRE(d->x_stride >= d->C, "%s: x row stride shorter than C=%d", who, d->C);
    KPGNN_REQUIRE(d->kind != KPGNN_NORM_LAYER || d->weight != nullptr, "%s: NULL weight (LAYER)", who);
    return KPGNN_OK;
}

GraphNormParams params_of(const kpgnn_graph_norm_desc* d) {
    GraphNormParams p = {};
    p.n_dyn = d->n_dyn; p.ptr = d->graph_ptr; p.N = d->N; p.G = d->G; p.C = d->C; p.kind = d->kind; p.eps = d->eps;
    p.x = d->x; p.xs = d->x_stride;
    if (d->kind == KPGNN_NORM_LAYER) { p.w = d->weight; p.b = d->bias; }
    p.SB = wave_blocks(d->G);
    return p;
}

template <int BWD>
int graph_norm_launch(const GraphNormParams& p, hipStream_t s) {
    const unsigned grid = (unsigned)(p.SB + p.G);
    const char* name = BWD ? "graph_norm_kernel<bwd>" : "graph_norm_kernel<fwd>";
    switch ((p.C + kWave - 1) / kWave) {
        case 1: hipLaunchKernelGGL((graph_norm_kernel<BWD, 1>), dim3(grid), dim3(kTeam), 0, s, p); break;
        case 2: hipLaunchKernelGGL((graph_norm_kernel<BWD, 2>), dim3(grid), dim3(kTeam), 0, s, p); break;
        case 3: hipLaunchKernelGGL((graph_norm_kernel<BWD, 3>), dim3(grid), dim3(kTeam), 0, s, p); break;
        default: hipLaunchKernelGGL((graph_norm_kernel<BWD, kMaxCpl>), dim3(grid), dim3(kTeam), 0, s, p); break;
    }
    KPGNN_LAUNCH_CHECK(name);
    return KPGNN_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" size_t kpgnn_graph_norm_saved_floats(int32_t G, int32_t C, int32_t kind) {
    if (G < 0 || C < 1 || C > kMaxC || kind < KPGNN_NORM_LAYER || kind > KPGNN_NORM_PAIR) return 0;
    return (size_t)(G > 0 ? G : 1) * 4;
}

extern "C" size_t kpgnn_graph_norm_workspace_bytes(int64_t N, int32_t G, int32_t C, int32_t kind) {
    if (N < 0 || G < 0 || C < 1 || C > kMaxC || kind < KPGNN_NORM_LAYER || kind > KPGNN_NORM_PAIR) return 0;
    return workspace_bytes(G, C, kind);
}

extern "C" int kpgnn_graph_norm_fwd(const kpgnn_graph_norm_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_graph_norm_fwd";
    if (int rc = check_desc(d, who)) return rc;
    KPGNN_REQUIRE(d->out != nullptr, "%s: NULL out", who);
    KPGNN_REQUIRE(d->out_stride >= d->C, "%s: out row stride shorter than C=%d", who, d->C);
    KPGNN_REQUIRE(!d->residual || d->res_stride >= d->C, "%s: residual row stride shorter than C=%d", who, d->C);
    if (d->N == 0 || d->G == 0) return KPGNN_OK;
    GraphNormParams p = params_of(d);
    p.out = d->out; p.os = d->out_stride; p.saved = d->saved;
    if (d->residual) { p.res = d->residual; p.rs = d->res_stride; }
    return graph_norm_launch<0>(p, (hipStream_t)stream);
}

extern "C" int kpgnn_graph_norm_bwd(const kpgnn_graph_norm_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_graph_norm_bwd";
    if (int rc = check_desc(d, who)) return rc;
    KPGNN_REQUIRE(d->gout != nullptr && d->gx != nullptr, "%s: NULL gout/gx", who);
    KPGNN_REQUIRE(d->gout_stride >= d->C && d->gx_stride >= d->C, "%s: gout/gx row stride shorter than C=%d", who, d->C);
    const bool params = d->kind == KPGNN_NORM_LAYER && (d->gweight || d->gbias);
    if (params) {
        KPGNN_REQUIRE(d->workspace != nullptr && ((uintptr_t)d->workspace & 7) == 0, "%s: NULL or misaligned workspace", who);
        KPGNN_REQUIRE(d->workspace_bytes >= workspace_bytes(d->G, d->C, d->kind), "%s: workspace of %zu bytes, %zu needed", who,
                      d->workspace_bytes, workspace_bytes(d->G, d->C, d->kind));
    }
    if (d->N == 0 || d->G == 0) return KPGNN_OK;
    GraphNormParams p = params_of(d);
    p.out = d->gx; p.os = d->gx_stride;
    p.g = d->gout; p.gs = d->gout_stride;
    if (params) { p.part = reinterpret_cast<double*>(d->workspace); p.gw = d->gweight; p.gb = d->gbias; }
    if (int rc = graph_norm_launch<1>(p, (hipStream_t)stream)) return rc;
    if (params) {
        hipLaunchKernelGGL(graph_norm_param_kernel, dim3((unsigned)p.C), dim3(kParamBlock), 0, (hipStream_t)stream, p);
        KPGNN_LAUNCH_CHECK("graph_norm_param_kernel");
    }
    return KPGNN_OK;
}
