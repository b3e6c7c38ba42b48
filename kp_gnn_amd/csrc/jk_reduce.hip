// Jumping-knowledge reduce over the S states of a body: sum, max, softmax-weighted sum (gfx950).  Contract: include/kpgnn.h,
// kpgnn_jk_reduce_fwd / _bwd.
//
// models/GNNs.py reduces the states through torch.stack: all S = num_layer + 1 states are copied into a fresh [S,N,H] (or
// [N,H,S] / [N,S,H]) tensor, reduced, and the gradient is scattered back through a tensor of that size.  Here the S state
// pointers travel BY VALUE in the kernel arguments (as in multi_copy.hip) and every state is read in place: the forward moves
// 4 N H (S + 1) bytes (+ N H for arg), the max backward 4 N H (S + 1) + N H, the softmax backward 4 N H (2 S + 1) plus the
// [N,S] terms.  Bound by bytes, not arithmetic: a group of 2^k <= 64 lanes owns a row (a row never leaves its wave), a lane
// moves 16 bytes per access where the shapes allow it, and the slot loop is unrolled by four so that four states' loads of a
// row are in flight before the first is used.  The slot index is the loop counter - the same in every lane - so the pointer
// table is read with scalar loads from the kernel-argument segment (no private copy: the resource report shows no scratch).
#include "kpgnn_common.h"

#include <cmath>

namespace kpgnn {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;      // 256 CUs x 8 blocks: grid-stride beyond
constexpr int kUnroll = 4;          // states whose loads are issued together

struct JkParams {
    const int32_t* n_dyn;
    int64_t N; int H, S;
    int64_t xs, os, gs;             // row strides of the states, out, gout
    const float* score; float* out; uint8_t* arg; float* w;
    const float* gout; float* gx; float* gscore;
    int flat;                       // SUM / MAX: every row stride equals H, the rows are one run of N * H elements
    int lanes_log2;                 // rows: 1 << lanes_log2 lanes walk a row, kBlock >> lanes_log2 rows per block
    const float* x[KPGNN_JK_MAX_STATES];
};

template <int VEC> __device__ __forceinline__ void st_arg(uint8_t* q, const int (&a)[VEC]) {
    if (VEC == 4) {
        *reinterpret_cast<uint32_t*>(q) = (uint32_t)a[0] | ((uint32_t)a[1 % VEC] << 8) | ((uint32_t)a[2 % VEC] << 16) |
                                          ((uint32_t)a[3 % VEC] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) q[j] = (uint8_t)a[j];
    }
}
template <int VEC> __device__ __forceinline__ void ld_arg(const uint8_t* q, int (&a)[VEC]) {
    if (VEC == 4) {
        const uint32_t t = *reinterpret_cast<const uint32_t*>(q);
#pragma unroll
        for (int j = 0; j < VEC; ++j) a[j] = (int)((t >> (8 * j)) & 255u);
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) a[j] = q[j];
    }
}

// slot l's contribution to VEC columns: acc / who are the running result and (MAX) its slot; wl the softmax weight
template <int MODE, int VEC>
__device__ __forceinline__ void jk_combine(float (&acc)[VEC], int (&who)[VEC], const float (&v)[VEC], int l, float wl) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        if (MODE == KPGNN_JK_SUM) {
            acc[j] += v[j];
        } else if (MODE == KPGNN_JK_MAX) {
            // `>`: the lowest slot keeps a tie; a NaN is taken and, once taken, never beaten (NaN compares false)
            const bool take = (v[j] > acc[j]) | (v[j] != v[j]);
            acc[j] = take ? v[j] : acc[j];
            who[j] = take ? l : who[j];
        } else {
            acc[j] = fmaf(wl, v[j], acc[j]);
        }
    }
}

// VEC columns of one row: states at offset xo, out at oo, arg at ao (row * H + c); SOFTMAX: the row's scores at sc, their max m
// and the sum z of exp(score - m); `lead` marks the one lane and chunk that writes the row's weights
template <int MODE, int VEC>
__device__ __forceinline__ void jk_fwd_elems(const JkParams& p, int64_t xo, int64_t oo, int64_t ao, const float* sc, float m,
                                             float z, float* wrow, bool lead) {
    float acc[VEC];
    int who[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { acc[j] = MODE == KPGNN_JK_MAX ? -INFINITY : 0.f; who[j] = 0; }
    const int S = p.S;
    int l = 0;
    for (; l + kUnroll <= S; l += kUnroll) {
        float v[kUnroll][VEC], wl[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) ldv<VEC>(p.x[l + u] + xo, v[u]);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            wl[u] = 0.f;
            if (MODE == KPGNN_JK_SOFTMAX) {
                wl[u] = expf(sc[l + u] - m) / z;
                if (lead) wrow[l + u] = wl[u];
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) jk_combine<MODE, VEC>(acc, who, v[u], l + u, wl[u]);
    }
    for (; l < S; ++l) {
        float v[VEC], wl = 0.f;
        ldv<VEC>(p.x[l] + xo, v);
        if (MODE == KPGNN_JK_SOFTMAX) {
            wl = expf(sc[l] - m) / z;
            if (lead) wrow[l] = wl;
        }
        jk_combine<MODE, VEC>(acc, who, v, l, wl);
    }
    stv<VEC>(p.out + oo, acc);
    if (MODE == KPGNN_JK_MAX && p.arg) st_arg<VEC>(p.arg + ao, who);
}

template <int MODE, int VEC>
__global__ void __launch_bounds__(kBlock) jk_reduce_fwd_kernel(const JkParams p) {
    const int64_t n = live_rows(p.N, p.n_dyn);
    if (MODE != KPGNN_JK_SOFTMAX && p.flat) {
        const int64_t total = n * (p.H / VEC), step = (int64_t)gridDim.x * kBlock;
        for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < total; g += step)
            jk_fwd_elems<MODE, VEC>(p, g * VEC, g * VEC, g * VEC, nullptr, 0.f, 1.f, nullptr, false);
        return;
    }
    const int lanes = 1 << p.lanes_log2, lane = threadIdx.x & (lanes - 1), rows = kBlock >> p.lanes_log2;
    for (int64_t row = (int64_t)blockIdx.x * rows + (threadIdx.x >> p.lanes_log2); row < n; row += (int64_t)gridDim.x * rows) {
        const float* sc = nullptr;
        float* wrow = nullptr;
        float m = 0.f, z = 1.f;
        if (MODE == KPGNN_JK_SOFTMAX) {
            // every lane of the row forms the S weights itself (S <= 32 broadcast loads): no exchange between lanes
            sc = p.score + row * p.S;
            wrow = p.w ? p.w + row * p.S : nullptr;
            m = sc[0];
            for (int l = 1; l < p.S; ++l) m = fmaxf(m, sc[l]);
            z = 0.f;
            for (int l = 0; l < p.S; ++l) z += expf(sc[l] - m);
        }
        bool lead = wrow != nullptr && lane == 0;
        for (int c = lane * VEC; c < p.H; c += lanes * VEC) {
            jk_fwd_elems<MODE, VEC>(p, row * p.xs + c, row * p.os + c, row * p.H + c, sc, m, z, wrow, lead);
            lead = false;
        }
    }
}

// MAX backward: gx[l] = gout where arg == l, else 0 - pure stores, no pointer table
template <int VEC>
__device__ __forceinline__ void jk_max_bwd_elems(const JkParams& p, int64_t go, int64_t ao, int64_t block) {
    float g[VEC], o[VEC];
    int a[VEC];
    ldv<VEC>(p.gout + go, g);
    ld_arg<VEC>(p.arg + ao, a);
    float* q = p.gx + ao;
    for (int l = 0; l < p.S; ++l, q += block) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = a[j] == l ? g[j] : 0.f;
        stv<VEC>(q, o);
    }
}

template <int VEC>
__global__ void __launch_bounds__(kBlock) jk_max_bwd_kernel(const JkParams p) {
    const int64_t n = live_rows(p.N, p.n_dyn);
    const int64_t block = p.N * p.H;          // (the capacity: block l of gx starts at l * N * H whatever the live count)
    if (p.flat) {
        const int64_t total = n * (p.H / VEC), step = (int64_t)gridDim.x * kBlock;
        for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < total; g += step)
            jk_max_bwd_elems<VEC>(p, g * VEC, g * VEC, block);
        return;
    }
    const int lanes = 1 << p.lanes_log2, lane = threadIdx.x & (lanes - 1), rows = kBlock >> p.lanes_log2;
    for (int64_t row = (int64_t)blockIdx.x * rows + (threadIdx.x >> p.lanes_log2); row < n; row += (int64_t)gridDim.x * rows)
        for (int c = lane * VEC; c < p.H; c += lanes * VEC)
            jk_max_bwd_elems<VEC>(p, row * p.gs + c, row * p.H + c, block);
}

// one slot of the SOFTMAX backward for this lane's columns of a row: stores gx[l] = wl * gout and returns the lane's share of
// d_l = <gout, x[l]>.  g0 / v0: the lane's first chunk (already loaded, have0: it exists); further chunks are loaded here
template <int VEC>
__device__ __forceinline__ float jk_softmax_bwd_slot(const JkParams& p, const float* xl, float* gxl, int64_t row, int lane,
                                                     int lanes, float wl, const float (&g0)[VEC], const float (&v0)[VEC],
                                                     bool have0) {
    float part = 0.f, o[VEC];
    const int c0 = lane * VEC;
    if (have0) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) { part = fmaf(g0[j], v0[j], part); o[j] = wl * g0[j]; }
        stv<VEC>(gxl + row * p.H + c0, o);
    }
    for (int c = c0 + lanes * VEC; c < p.H; c += lanes * VEC) {
        float g[VEC], v[VEC];
        ldv<VEC>(p.gout + row * p.gs + c, g);
        ldv<VEC>(xl + row * p.xs + c, v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) { part = fmaf(g[j], v[j], part); o[j] = wl * g[j]; }
        stv<VEC>(gxl + row * p.H + c, o);
    }
    return part;
}

template <int VEC>
__global__ void __launch_bounds__(kBlock) jk_softmax_bwd_kernel(const JkParams p) {
    const int64_t n = live_rows(p.N, p.n_dyn);
    const int64_t block = p.N * p.H;
    const int lanes = 1 << p.lanes_log2, lane = threadIdx.x & (lanes - 1), rows = kBlock >> p.lanes_log2;
    const int S = p.S;
    for (int64_t row = (int64_t)blockIdx.x * rows + (threadIdx.x >> p.lanes_log2); row < n; row += (int64_t)gridDim.x * rows) {
        const float* wrow = p.w + row * S;
        float* gsrow = p.gscore + row * S;
        const bool have0 = lane * VEC < p.H;
        const int64_t x0 = row * p.xs + lane * VEC;
        float g0[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) g0[j] = 0.f;
        if (have0) ldv<VEC>(p.gout + row * p.gs + lane * VEC, g0);
        float dot = 0.f;
        int l = 0;
        for (; l + kUnroll <= S; l += kUnroll) {
            // (the loads of four states first: the stores to gx below may alias anything as far as the compiler knows)
            float v[kUnroll][VEC], wl[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[u][j] = 0.f;
                if (have0) ldv<VEC>(p.x[l + u] + x0, v[u]);
                wl[u] = wrow[l + u];
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const float part = jk_softmax_bwd_slot<VEC>(p, p.x[l + u], p.gx + (l + u) * block, row, lane, lanes, wl[u], g0,
                                                            v[u], have0);
                const float d = group_sum(part, lanes);      // (the 1 << lanes_log2 lanes of a row never leave its wave)
                dot = fmaf(wl[u], d, dot);
                if (lane == 0) gsrow[l + u] = d;       // parked until the row's dot is known (below)
            }
        }
        for (; l < S; ++l) {
            float v[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = 0.f;
            if (have0) ldv<VEC>(p.x[l] + x0, v);
            const float wl = wrow[l];
            const float part = jk_softmax_bwd_slot<VEC>(p, p.x[l], p.gx + l * block, row, lane, lanes, wl, g0, v, have0);
            const float d = group_sum(part, lanes);
            dot = fmaf(wl, d, dot);
            if (lane == 0) gsrow[l] = d;
        }
        // gscore[l] = w_l (d_l - dot): the lane that parked the d_l reads its own stores back
        if (lane == 0)
            for (int q = 0; q < S; ++q) gsrow[q] = wrow[q] * (gsrow[q] - dot);
    }
}

int lanes_log2_of(int H, int vec) {
    const int cg = (H + vec - 1) / vec;
    int k = 0;
    while ((1 << k) < cg && k < 6) ++k;        // at most 64 lanes: a row stays inside one wave
    return k;
}

unsigned grid_of(const JkParams& p, int vec, bool flat) {
    const int cg = (p.H + vec - 1) / vec;
    const int rows = kBlock >> p.lanes_log2;
    const int64_t blocks = flat ? (p.N * cg + kBlock - 1) / kBlock : (p.N + rows - 1) / rows;
    return (unsigned)(blocks > kMaxGrid ? kMaxGrid : blocks);
}

int check_desc(const kpgnn_jk_desc* d, const char* who) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->S >= 1 && d->S <= KPGNN_JK_MAX_STATES, "%s: bad S=%d (1 .. %d states)", who, d->S, KPGNN_JK_MAX_STATES);
    KPGNN_REQUIRE(d->N >= 0 && d->H >= 1, "%s: bad N=%lld H=%d", who, (long long)d->N, d->H);
    KPGNN_REQUIRE(d->mode == KPGNN_JK_SUM || d->mode == KPGNN_JK_MAX || d->mode == KPGNN_JK_SOFTMAX, "%s: unknown mode %d", who,
                  d->mode);
    return KPGNN_OK;
}

int check_states(const kpgnn_jk_desc* d, const char* who) {
    for (int l = 0; l < d->S; ++l) KPGNN_REQUIRE(d->x[l] != nullptr, "%s: NULL x[%d]", who, l);
    KPGNN_REQUIRE(d->x_stride >= d->H, "%s: x row stride shorter than H=%d", who, d->H);
    return KPGNN_OK;
}

JkParams params_of(const kpgnn_jk_desc* d) {
    JkParams p = {};
    p.n_dyn = d->n_dyn; p.N = d->N; p.H = d->H; p.S = d->S;
    p.xs = d->x_stride; p.os = d->out_stride; p.gs = d->gout_stride;
    p.score = d->score; p.out = d->out; p.arg = d->arg; p.w = d->w;
    p.gout = d->gout; p.gx = d->gx; p.gscore = d->gscore;
    for (int l = 0; l < KPGNN_JK_MAX_STATES; ++l) p.x[l] = l < d->S ? d->x[l] : nullptr;
    return p;
}

template <int MODE>
int fwd_launch(JkParams& p, int vec, hipStream_t s) {
    const unsigned grid = grid_of(p, vec, MODE != KPGNN_JK_SOFTMAX && p.flat);
    if (vec == 4) hipLaunchKernelGGL((jk_reduce_fwd_kernel<MODE, 4>), dim3(grid), dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL((jk_reduce_fwd_kernel<MODE, 1>), dim3(grid), dim3(kBlock), 0, s, p);
    KPGNN_LAUNCH_CHECK("jk_reduce_fwd_kernel");
    return KPGNN_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_jk_reduce_fwd(const kpgnn_jk_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_jk_reduce_fwd";
    if (int rc = check_desc(d, who)) return rc;
    if (int rc = check_states(d, who)) return rc;
    KPGNN_REQUIRE(d->out != nullptr, "%s: NULL out", who);
    KPGNN_REQUIRE(d->out_stride >= d->H, "%s: out row stride shorter than H=%d", who, d->H);
    KPGNN_REQUIRE(d->mode != KPGNN_JK_SOFTMAX || d->score != nullptr, "%s: NULL score (SOFTMAX)", who);
    if (d->N == 0) return KPGNN_OK;
    JkParams p = params_of(d);
    if (d->mode != KPGNN_JK_MAX) p.arg = nullptr;
    if (d->mode != KPGNN_JK_SOFTMAX) p.w = nullptr;
    // 16 B per lane when the width, every row stride and every pointer allow it (arg: 4 B per lane); the scalar path otherwise
    int vec = row_vec(p.H, {p.out}, {p.xs, p.os}) == 4 ? 4 : 1;
    for (int l = 0; l < p.S; ++l)
        if ((uintptr_t)p.x[l] & 15) vec = 1;
    if ((uintptr_t)p.arg & 3) vec = 1;
    p.flat = p.xs == p.H && p.os == p.H;
    p.lanes_log2 = lanes_log2_of(p.H, vec);
    hipStream_t s = (hipStream_t)stream;
    if (d->mode == KPGNN_JK_SUM) return fwd_launch<KPGNN_JK_SUM>(p, vec, s);
    if (d->mode == KPGNN_JK_MAX) return fwd_launch<KPGNN_JK_MAX>(p, vec, s);
    return fwd_launch<KPGNN_JK_SOFTMAX>(p, vec, s);
}

extern "C" int kpgnn_jk_reduce_bwd(const kpgnn_jk_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_jk_reduce_bwd";
    if (int rc = check_desc(d, who)) return rc;
    KPGNN_REQUIRE(d->mode != KPGNN_JK_SUM, "%s: SUM has no backward kernel (every state's gradient is gout itself)", who);
    KPGNN_REQUIRE(d->gout != nullptr && d->gx != nullptr, "%s: NULL gout/gx", who);
    KPGNN_REQUIRE(d->gout_stride >= d->H, "%s: gout row stride shorter than H=%d", who, d->H);
    if (d->mode == KPGNN_JK_MAX) {
        KPGNN_REQUIRE(d->arg != nullptr, "%s: NULL arg (MAX)", who);
    } else {
        KPGNN_REQUIRE(d->w != nullptr && d->gscore != nullptr, "%s: NULL w/gscore (SOFTMAX)", who);
        if (int rc = check_states(d, who)) return rc;
    }
    if (d->N == 0) return KPGNN_OK;
    JkParams p = params_of(d);
    hipStream_t s = (hipStream_t)stream;
    if (d->mode == KPGNN_JK_MAX) {
        int vec = row_vec(p.H, {p.gout, p.gx}, {p.gs}) == 4 ? 4 : 1;
        if ((uintptr_t)p.arg & 3) vec = 1;
        p.flat = p.gs == p.H;
        p.lanes_log2 = lanes_log2_of(p.H, vec);
        const unsigned grid = grid_of(p, vec, p.flat);
        if (vec == 4) hipLaunchKernelGGL((jk_max_bwd_kernel<4>), dim3(grid), dim3(kBlock), 0, s, p);
        else hipLaunchKernelGGL((jk_max_bwd_kernel<1>), dim3(grid), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("jk_max_bwd_kernel");
        return KPGNN_OK;
    }
    int vec = row_vec(p.H, {p.gout, p.gx}, {p.gs, p.xs}) == 4 ? 4 : 1;
    for (int l = 0; l < p.S; ++l)
        if ((uintptr_t)p.x[l] & 15) vec = 1;
    p.lanes_log2 = lanes_log2_of(p.H, vec);
    const unsigned grid = grid_of(p, vec, false);
    if (vec == 4) hipLaunchKernelGGL((jk_softmax_bwd_kernel<4>), dim3(grid), dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL((jk_softmax_bwd_kernel<1>), dim3(grid), dim3(kBlock), 0, s, p);
    KPGNN_LAUNCH_CHECK("jk_softmax_bwd_kernel");
    return KPGNN_OK;
}
