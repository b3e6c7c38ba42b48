// nn.Linear with a narrow output, y[M,O] = x[M,I] W^T + b for 1 <= O <= 32, and its backward (gfx950).
// Contract: include/kpgnn.h, kpgnn_head_linear_fwd / _bwd.
//
// The classifiers nn.Linear(hidden, C) of models/GraphClassification.py:37,52 and NodeClassification.py:21-24,35 (C = 2, 6,
// 10, 15 in train_TU.py / train_EXP.py / train_CSL.py / train_SR.py) and the node regressor nn.Linear(hidden, 1) of
// NodeRegression.py:18,29 (train_node_property.py:46) fit none of the MFMA kernels (O % 4, I in a fixed set), so the
// framework runs them as library GEMMs: a Cijk launch per product plus a bias reduce, for a [M,I] x [I,O] product whose
// arithmetic is negligible next to reading x.  score_head_bwd_kernel walks all rows with 64 row lanes, which is sized for a
// few thousand graph rows, not for 50,000 node rows.  These are streaming kernels, no MFMA: as in pool.hip a sub-group of
// lanes owns a row and its lanes span the columns 16 B wide (rows wider than the sub-group take several chunks).
// Forward: W sits in LDS, every lane keeps O partial dot products, a fixed butterfly finishes them.  Backward: a block
// covers a tile of rows; per column chunk a lane holds its W columns and its dW partials in registers, the sub-groups of a
// wave meet by butterfly and the four waves in LDS in wave order, and the block leaves one partial [O, I] (+ [O]) slab that a
// slab_reduce launch adds in block order.  No atomics: bitwise reproducible.
// O < 1 or I < 1 is a malformed descriptor (KPGNN_EINVAL); O > 32 or I > 1024 is a shape these kernels do not instantiate
// (KPGNN_ELIMIT: the caller keeps another path).  The descriptor's I is the width of BOTH x and W: the caller checks that they agree.
#include <initializer_list>

#include "kpgnn_common.h"

namespace kpgnn {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxO = 32, kMaxI = 1024;

struct HeadParams {
    const int32_t* n_dyn;
    int64_t M; int O, I;
    const float* x; int64_t xs;
    const float* w; const float* bias;
    float* y; int64_t ys;
    const float* dy; int64_t dys;
    float* dx; int64_t dxs;
    float* dwp; float* dbp; int64_t part_stride;     // block b leaves its partial dW at dwp + b * part_stride (db likewise)
    int64_t rows_per_block;
};

template <int VEC, int L>
__global__ void __launch_bounds__(kBlock) head_linear_fwd_kernel(HeadParams p) {
    extern __shared__ __align__(16) float wl[];               // W [O][I]
    const int O = p.O, I = p.I;
    for (int e = threadIdx.x * VEC; e < O * I; e += kBlock * VEC) {      // (I % VEC == 0, so is O * I)
        float t[VEC];
        ldv<VEC>(p.w + e, t);
        stv<VEC>(wl + e, t);
    }
    __syncthreads();
    const int64_t M = live_rows(p.M, p.n_dyn);
    constexpr int S = kBlock / L;
    const int sg = threadIdx.x / L, sl = threadIdx.x % L;
    for (int64_t m = (int64_t)blockIdx.x * S + sg; m < M; m += (int64_t)gridDim.x * S) {
        float acc[kMaxO];
#pragma unroll
        for (int o = 0; o < kMaxO; ++o) acc[o] = 0.f;
        for (int c = sl * VEC; c < I; c += L * VEC) {
            float v[VEC];
            ldv<VEC>(p.x + m * p.xs + c, v);
#pragma unroll
            for (int o = 0; o < kMaxO; ++o) {
                if (o < O) {                                      // (uniform)
                    float wv[VEC];
                    ldv<VEC>(wl + o * I + c, wv);
                    for (int q = 0; q < VEC; ++q) acc[o] = fmaf(v[q], wv[q], acc[o]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < kMaxO; ++o) {
            if (o < O) {
                const float s = group_sum<L>(acc[o]);
                if ((o & (L - 1)) == sl) p.y[m * p.ys + o] = s + (p.bias ? p.bias[o] : 0.f);
            }
        }
    }
}

template <int VEC, int L, int OB>
__global__ void __launch_bounds__(kBlock) head_linear_bwd_kernel(HeadParams p) {
    constexpr int S = kBlock / L, LW = L * VEC;                  // sub-groups of a block, columns of a chunk
    __shared__ float tile[OB][LW];
    __shared__ float tileb[kBlock / kWave][OB];
    const int O = p.O, I = p.I;
    const int64_t M = live_rows(p.M, p.n_dyn);
    const int sg = threadIdx.x / L, sl = threadIdx.x % L;
    const int wave = threadIdx.x / kWave, first = (threadIdx.x % kWave) < L;    // first: the wave's first sub-group
    const int64_t lo = (int64_t)blockIdx.x * p.rows_per_block;
    int64_t hi = lo + p.rows_per_block;
    if (hi > M) hi = M;
    float* dwb = p.dwp + blockIdx.x * p.part_stride;
    for (int cb = 0; cb < I; cb += LW) {
        const int c = cb + sl * VEC;
        const bool on = c < I;
        float wr[OB][VEC], dwa[OB][VEC], dba[OB];
#pragma unroll
        for (int o = 0; o < OB; ++o) {
            dba[o] = 0.f;
            for (int q = 0; q < VEC; ++q) { wr[o][q] = 0.f; dwa[o][q] = 0.f; }
            if (o < O && on) ldv<VEC>(p.w + o * I + c, wr[o]);
        }
        for (int64_t m = lo + sg; m < hi; m += S) {
            float v[VEC], g[VEC], dyv[OB];
            for (int q = 0; q < VEC; ++q) { v[q] = 0.f; g[q] = 0.f; }
            if (on) ldv<VEC>(p.x + m * p.xs + c, v);
#pragma unroll
            for (int o = 0; o < OB; ++o) dyv[o] = o < O ? p.dy[m * p.dys + o] : 0.f;
#pragma unroll
            for (int o = 0; o < OB; ++o) {
                dba[o] += dyv[o];
                for (int q = 0; q < VEC; ++q) {
                    dwa[o][q] = fmaf(dyv[o], v[q], dwa[o][q]);
                    g[q] = fmaf(dyv[o], wr[o][q], g[q]);
                }
            }
            if (p.dx && on) stv<VEC>(p.dx + m * p.dxs + c, g);
        }
        // the sub-groups of a wave meet by butterfly, the waves in LDS in wave order
#pragma unroll
        for (int o = 0; o < OB; ++o) {
#pragma unroll
            for (int off = L; off < kWave; off <<= 1) {
                for (int q = 0; q < VEC; ++q) dwa[o][q] += __shfl_xor(dwa[o][q], off, 64);
                dba[o] += __shfl_xor(dba[o], off, 64);
            }
        }
        for (int k = 0; k < kBlock / kWave; ++k) {
            if (wave == k && first) {
#pragma unroll
                for (int o = 0; o < OB; ++o)
                    for (int q = 0; q < VEC; ++q) {
                        float* t = &tile[o][sl * VEC + q];
                        *t = k == 0 ? dwa[o][q] : *t + dwa[o][q];
                    }
            }
            __syncthreads();
        }
        for (int e = threadIdx.x; e < O * LW; e += kBlock) {
            const int o = e / LW, col = e % LW;
            if (cb + col < I) dwb[(int64_t)o * I + cb + col] = tile[o][col];
        }
        if (cb == 0 && p.dbp) {
            if (first && sl == 0) {
#pragma unroll
                for (int o = 0; o < OB; ++o) tileb[wave][o] = dba[o];
            }
            __syncthreads();
            if ((int)threadIdx.x < O) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < kBlock / kWave; ++k) s += tileb[k][threadIdx.x];
                p.dbp[blockIdx.x * p.part_stride + threadIdx.x] = s;
            }
        }
        __syncthreads();
    }
}

int check(const kpgnn_head_linear_desc* d, const char* who) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->M >= 0 && d->O >= 1 && d->I >= 1, "%s: bad M=%lld O=%d I=%d", who, (long long)d->M, d->O, d->I);
    if (d->O > kMaxO) return fail(KPGNN_ELIMIT, "%s: O=%d exceeds %d outputs", who, d->O, kMaxO);
    if (d->I > kMaxI) return fail(KPGNN_ELIMIT, "%s: I=%d exceeds %d inputs", who, d->I, kMaxI);
    KPGNN_REQUIRE(d->w && (d->M == 0 || (d->x && d->x_stride >= d->I)), "%s: NULL x/w or bad x stride", who);
    return KPGNN_OK;
}

void shape(int I, int vec_cap, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> strides, int* vec, int* lanes) {
    *vec = row_vec(I, ptrs, strides);
    if (*vec > vec_cap) *vec = vec_cap;
    *lanes = row_lanes(I, *vec);
    if (*lanes > kWave) *lanes = kWave;                       // (wider rows: several chunks of the same lanes)
}

// Rows a backward block covers: a multiple of 64 (every sub-group count divides it), at least 128, about two blocks per CU.
int64_t bwd_rows_per_block(int64_t M) {
    const int64_t slots = (int64_t)device_facts().cu_count * 2;
    int64_t r = (M + slots - 1) / slots;
    if (r < 128) r = 128;
    return (r + 63) / 64 * 64;
}

template <int OB, typename V, typename L>
int launch_bwd(V, L, const HeadParams& p, unsigned grid, hipStream_t s) {
    if constexpr (OB > 16 && V::value > 2) {
        return fail(KPGNN_EINVAL, "head_linear_bwd: no kernel for vec=%d at O=%d", V::value, p.O);
    } else {
        hipLaunchKernelGGL((head_linear_bwd_kernel<V::value, L::value, OB>), dim3(grid), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("head_linear_bwd_kernel");
        return KPGNN_OK;
    }
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" size_t kpgnn_head_linear_workspace_bytes(int64_t M, int32_t O, int32_t I) {
    if (M < 1 || O < 1 || O > kMaxO || I < 1 || I > kMaxI) return 0;
    const int64_t rpb = bwd_rows_per_block(M), grid = (M + rpb - 1) / rpb;
    return grid > 1 ? (size_t)grid * ((size_t)O * I + O) * sizeof(float) : 0;
}

extern "C" int kpgnn_head_linear_fwd(const kpgnn_head_linear_desc* d, kpgnn_stream_t stream) {
    int rc = check(d, "head_linear_fwd");
    if (rc != KPGNN_OK) return rc;
    if (d->M == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->y && d->y_stride >= d->O, "head_linear_fwd: NULL y or bad stride");
    int vec, lanes;
    shape(d->I, 4, {d->x, d->w}, {d->x_stride}, &vec, &lanes);
    HeadParams p = {};
    p.n_dyn = d->n_dyn; p.M = d->M; p.O = d->O; p.I = d->I; p.x = d->x; p.xs = d->x_stride; p.w = d->w; p.bias = d->bias;
    p.y = d->y; p.ys = d->y_stride;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)d->O * d->I * sizeof(float);
    const int rows = kBlock / lanes;
    int64_t g = (d->M + rows * 4 - 1) / (rows * 4);
    const int64_t cap = (int64_t)device_facts().cu_count * 4;
    const unsigned grid = (unsigned)(g > cap ? cap : g);
    return dispatch_row_shape<64>(vec, lanes, "head_linear_fwd", [&](auto V, auto L) {
        if (lds > 64 * 1024) KPGNN_HIP_TRY(ensure_dynamic_lds((const void*)head_linear_fwd_kernel<V.value, L.value>, lds));
        hipLaunchKernelGGL((head_linear_fwd_kernel<V.value, L.value>), dim3(grid), dim3(kBlock), lds, s, p);
        KPGNN_LAUNCH_CHECK("head_linear_fwd_kernel");
        return KPGNN_OK;
    });
}

extern "C" int kpgnn_head_linear_bwd(const kpgnn_head_linear_desc* d, kpgnn_stream_t stream) {
    int rc = check(d, "head_linear_bwd");
    if (rc != KPGNN_OK) return rc;
    KPGNN_REQUIRE(d->dw && (d->M == 0 || (d->dy && d->dy_stride >= d->O)) && (!d->dx || d->dx_stride >= d->I),
                  "head_linear_bwd: NULL dy/dw or bad stride");
    hipStream_t s = (hipStream_t)stream;
    if (d->M == 0) {                                          // no row: the parameter gradients are zero
        KPGNN_HIP_TRY(hipMemsetAsync(d->dw, 0, sizeof(float) * d->O * d->I, s));
        if (d->db) KPGNN_HIP_TRY(hipMemsetAsync(d->db, 0, sizeof(float) * d->O, s));
        return KPGNN_OK;
    }
    int vec, lanes;
    shape(d->I, d->O > 16 ? 2 : 4, {d->x, d->w, d->dx}, {d->x_stride, d->dx ? d->dx_stride : 0}, &vec, &lanes);
    HeadParams p = {};
    p.n_dyn = d->n_dyn; p.M = d->M; p.O = d->O; p.I = d->I; p.x = d->x; p.xs = d->x_stride; p.w = d->w;
    p.dy = d->dy; p.dys = d->dy_stride; p.dx = d->dx; p.dxs = d->dx_stride;
    p.rows_per_block = bwd_rows_per_block(d->M);
    const int64_t grid = (d->M + p.rows_per_block - 1) / p.rows_per_block;
    const int64_t OI = (int64_t)d->O * d->I;
    float* slab = (float*)d->workspace;
    if (grid == 1) {                                          // one block covers every row: its partial IS the gradient
        p.dwp = d->dw; p.dbp = d->db; p.part_stride = 0;
    } else {
        p.part_stride = OI + (d->db ? d->O : 0);
        KPGNN_REQUIRE(slab && d->workspace_bytes >= (size_t)grid * p.part_stride * sizeof(float),
                      "head_linear_bwd: workspace of %zu bytes, %zu needed", d->workspace_bytes, (size_t)grid * p.part_stride * sizeof(float));
        p.dwp = slab; p.dbp = d->db ? slab + OI : nullptr;
    }
    rc = dispatch_row_shape<64>(vec, lanes, "head_linear_bwd", [&](auto V, auto L) {
        if (d->O <= 4) return launch_bwd<4>(V, L, p, (unsigned)grid, s);
        if (d->O <= 16) return launch_bwd<16>(V, L, p, (unsigned)grid, s);
        return launch_bwd<32>(V, L, p, (unsigned)grid, s);
    });
    if (rc != KPGNN_OK || grid == 1) return rc;
    return slab_reduce(slab, (int)grid, p.part_stride, d->dw, OI, d->db, d->db ? d->O : 0, nullptr, s);
}
