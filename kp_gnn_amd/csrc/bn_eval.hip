// Evaluation-mode BatchNorm1d (+ReLU, +residual) over [N, C] rows for gfx950: z = [relu]((x - running_mean) *
// rsqrt(running_var + eps) * gamma + beta) [+ residual].  Contract: include/kpgnn.h, kpgnn_bn_eval.
// With running statistics the norm is a per-column map: one HBM-bound streaming launch, no statistics slot.  A sub-group of
// G lanes spans the C columns VEC floats wide (kpgnn_common.h: row_vec / row_lanes / dispatch_row_shape), keeps its columns'
// coefficients in registers and strides over the rows; the running statistics are only read.
#include <initializer_list>

#include "kpgnn_common.h"

namespace kpgnn {
namespace {

constexpr int kBlock = 256;

struct BnEvalParams {
    const int32_t* n_dyn;
    int64_t N; int C, relu; float eps;
    const float* x; int64_t xs;
    const float* gamma; const float* beta; const float* rmean; const float* rvar;
    const float* res; int64_t rs;
    float* z; int64_t zs;
};

template <int VEC, int G>
__global__ void __launch_bounds__(kBlock) bn_eval_kernel(BnEvalParams p) {
    p.N = live_rows(p.N, p.n_dyn);
    const int rl = threadIdx.x / G, sl = threadIdx.x % G, c0 = sl * VEC;
    if (c0 >= p.C) return;                            // (VEC divides C: a lane's columns are in or out together)
    float mean[VEC], istd[VEC], g[VEC], bt[VEC];
    ldv<VEC>(p.rmean + c0, mean); ldv<VEC>(p.rvar + c0, istd); ldv<VEC>(p.gamma + c0, g); ldv<VEC>(p.beta + c0, bt);
    for (int q = 0; q < VEC; ++q) istd[q] = 1.0f / sqrtf(istd[q] + p.eps);
    auto finish = [&](int64_t r, float (&v)[VEC]) {
        for (int q = 0; q < VEC; ++q) {
            v[q] = fmaf((v[q] - mean[q]) * istd[q], g[q], bt[q]);
            if (p.relu) v[q] = fmaxf(v[q], 0.f);
        }
        if (p.res) {
            float a[VEC];
            ldv<VEC>(p.res + r * p.rs + c0, a);
            for (int q = 0; q < VEC; ++q) v[q] += a[q];
        }
        stv<VEC>(p.z + r * p.zs + c0, v);
    };
    // four rows per trip: the loads are independent, a one-row loop keeps a single request in flight per thread
    const int64_t step = (int64_t)gridDim.x * (kBlock / G);
    int64_t r = (int64_t)blockIdx.x * (kBlock / G) + rl;
    for (; r + 3 * step < p.N; r += 4 * step) {
        float v0[VEC], v1[VEC], v2[VEC], v3[VEC];
        ldv<VEC>(p.x + r * p.xs + c0, v0);
        ldv<VEC>(p.x + (r + step) * p.xs + c0, v1);
        ldv<VEC>(p.x + (r + 2 * step) * p.xs + c0, v2);
        ldv<VEC>(p.x + (r + 3 * step) * p.xs + c0, v3);
        finish(r, v0); finish(r + step, v1); finish(r + 2 * step, v2); finish(r + 3 * step, v3);
    }
    for (; r < p.N; r += step) {
        float v[VEC];
        ldv<VEC>(p.x + r * p.xs + c0, v);
        finish(r, v);
    }
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_bn_eval(const kpgnn_bn_eval_desc* d, kpgnn_stream_t stream) {
    KPGNN_REQUIRE(d != nullptr, "bn_eval: NULL descriptor");
    KPGNN_REQUIRE(d->N >= 1 && d->C >= 1, "bn_eval: bad N=%lld C=%d", (long long)d->N, d->C);
    KPGNN_REQUIRE(d->x && d->z && d->bn.gamma && d->bn.beta, "bn_eval: NULL pointer");
    KPGNN_REQUIRE(d->bn.running_mean && d->bn.running_var,
                  "bn_eval: needs running_mean and running_var (evaluation mode runs on the running statistics)");
    KPGNN_REQUIRE(d->x_stride >= d->C && d->z_stride >= d->C && (!d->residual || d->r_stride >= d->C), "bn_eval: bad strides");
    const int vec = row_vec(d->C, {d->x, d->z, d->residual, d->bn.gamma, d->bn.beta, d->bn.running_mean, d->bn.running_var},
                            {d->x_stride, d->z_stride, d->residual ? d->r_stride : 0});
    const int lanes = (d->C + vec - 1) / vec;
    if (lanes > 64) return fail(KPGNN_ELIMIT, "bn_eval: C=%d needs %d lanes > 64 (C <= 256)", d->C, lanes);
    const int g = row_lanes(d->C, vec);
    BnEvalParams p = {};
    p.N = d->N; p.n_dyn = d->n_dyn; p.C = d->C; p.relu = d->relu; p.eps = d->bn.eps;
    p.x = d->x; p.xs = d->x_stride; p.gamma = d->bn.gamma; p.beta = d->bn.beta; p.rmean = d->bn.running_mean; p.rvar = d->bn.running_var;
    p.res = d->residual; p.rs = d->r_stride; p.z = d->z; p.zs = d->z_stride;
    hipStream_t s = (hipStream_t)stream;
    // >= 4 rows per thread, at most eight blocks per CU
    const int64_t rows_per_block = kBlock / g;
    int64_t grid = (d->N + rows_per_block * 4 - 1) / (rows_per_block * 4);
    const int64_t cap = (int64_t)device_facts().cu_count * 8;
    if (grid > cap) grid = cap;
    return dispatch_row_shape<64>(vec, g, "bn_eval", [&](auto V, auto GG) {
        hipLaunchKernelGGL((bn_eval_kernel<V.value, GG.value>), dim3((unsigned)grid), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("bn_eval_kernel");
        return (int)KPGNN_OK;
    });
}
