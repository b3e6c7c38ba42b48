// Embedding collisions of the regular-graph simulation (gfx950).  Contract: include/kpgnn.h, kpgnn_collision_count.
// Replaces run_simulation.py:165-178 (compute_simulation_collisions), which builds outputs.unsqueeze(-1) - outputs.t().unsqueeze(0),
// an [N, D, N] fp32 tensor (1 TB at N = 128,000, D = 16), squares it, sums over D and counts d2 < 1e-10.  Here the N x N pair
// matrix is walked as 128 x 128 tiles of its upper triangle and never exists: a 256-thread block stages the two row panels of a
// tile in LDS transposed ([d][row], 16 columns at a time), every thread owns an 8 x 8 micro-tile of pairs in registers, and the
// only output is two exact 64-bit counts.
//
// Arithmetic.  d2(i,j) = sum_d (o[i,d] - o[j,d])^2 in the DIFFERENCE form, one fp32 subtract and one fp32 fma per column, d in
// ascending order.  The Gram form |a|^2 + |b|^2 - 2 a.b (which would put the work on the matrix cores) is not used: at
// |row| ~ 1 its three terms are O(1) and cancel to ~1e-7 absolute, three orders of magnitude above the 1e-10 threshold, so it
// cannot tell a collision from a near miss.  The compare is the plain IEEE d2 < eps: a NaN d2 (a NaN row, or Inf - Inf between
// two Inf rows) and an Inf d2 do not collide, exactly as in the framework expression; there is no fast-math in this file.
//
// Band rule.  With u = 2^-24: t_d = fl(a - b) = (a - b)(1 + e1), |e1| <= u; acc_d = fl(acc_{d-1} + t_d^2) with the square exact
// inside the fma, one rounding (1 + e2) per step.  Every term is non-negative, so the result is sum_d (a-b)^2 (1 + theta_d) with
// |theta_d| <= (1+u)^2 (1+u)^D - 1 <= (D + 2) u + O(u^2): the D roundings of the running sum and the two of the squared
// difference.  That is half of delta = (D + 2) 2^-23, the bound of the framework route (subtract, square and add rounded
// separately: 3u per term, (D-1)u for the sum, doubled for margin), so the same delta serves both: a pair whose exact d2 lies
// outside [eps (1 - delta), eps (1 + delta)] is classified as exact arithmetic classifies it.  (A term below the fp32 normal
// range loses at most 2^-149 absolutely, D of them 4e-43: nothing next to eps delta >= 4e-17 eps.)
#include "kpgnn_common.h"

#include <cmath>

namespace kpgnn {
namespace {

constexpr int kTile = 128;       // pairs tile: kTile rows i x kTile rows j
constexpr int kThreads = 256;    // 16 x 16 threads, 8 x 8 pairs each
constexpr int kChunk = 16;       // columns staged per pass: the LDS need does not grow with D
constexpr int kMaxGrid = 4096;   // partial pairs the workspace holds: the persistent grid never exceeds it
constexpr int kMaxD = 256;

struct CollParams {
    const float* x; int64_t xs; int64_t N; int D; float eps;
    int64_t tiles;               // upper-triangle tiles T (T + 1) / 2, T = ceil(N / kTile)
    unsigned long long* part;    // [grid][2]: upper, diag
};

// rows r0 .. r0 + kTile of columns d0 .. d0 + dn into p[d][row]; rows at or beyond N are not read (their slots are never counted)
__device__ __forceinline__ void stage(const CollParams& p, float (*dst)[kTile], int64_t r0, int d0, int dn) {
    const int row = threadIdx.x % kTile, half = threadIdx.x / kTile;     // consecutive lanes: consecutive rows, one LDS bank each
    const int64_t r = r0 + row;
    if (r < p.N) {
        const float* src = p.x + r * p.xs + d0;
        for (int c = half; c < dn; c += kThreads / kTile) dst[c][row] = src[c];
    } else {
        for (int c = half; c < dn; c += kThreads / kTile) dst[c][row] = 0.0f;
    }
}

__device__ __forceinline__ void ld4(const float* q, float* v) {
    const float4 t = *reinterpret_cast<const float4*>(q);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

// one column of a tile: the thread's 8 i-values and 8 j-values from the staged panels, 64 pairs as 32 packed subtracts and 32
// packed fmas (per element an IEEE subtract and an IEEE fma: the packing changes no bit)
__device__ __forceinline__ void column(const float* pa, const float* pb, int ty, int tx, float (&acc)[8][8]) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    float vi[8], vj[8];
    ld4(pa + ty * 4, vi); ld4(pa + 64 + ty * 4, vi + 4);
    ld4(pb + tx * 4, vj); ld4(pb + 64 + tx * 4, vj + 4);
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; b += 2) {
            f2 va = {vi[a], vi[a]}, vb = {vj[b], vj[b + 1]}, ac = {acc[a][b], acc[a][b + 1]};
            const f2 df = va - vb;
            ac = __builtin_elementwise_fma(df, df, ac);
            acc[a][b] = ac.x; acc[a][b + 1] = ac.y;
        }
}

__global__ void __launch_bounds__(kThreads) collision_tiles_kernel(CollParams p) {
    __shared__ __attribute__((aligned(16))) float A[kChunk][kTile];
    __shared__ __attribute__((aligned(16))) float B[kChunk][kTile];
    __shared__ unsigned long long red[2][kThreads / kWave];
    // A thread's 8 i-rows are two runs of 4, at ty * 4 and 64 + ty * 4 (its j-rows likewise with tx): each run is one 16-byte LDS
    // read, the 16 lanes of a read's lane group either share the address (i) or cover 256 contiguous bytes (j): no bank conflict.
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    unsigned long long upper = 0, diag = 0;
    for (int64_t t = blockIdx.x; t < p.tiles; t += gridDim.x) {
        // t = bj (bj + 1) / 2 + bi, bi <= bj: tiles below the diagonal have no index at all
        int64_t bj = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while (bj * (bj + 1) / 2 > t) --bj;
        while ((bj + 1) * (bj + 2) / 2 <= t) ++bj;
        const int64_t bi = t - bj * (bj + 1) / 2;
        const int64_t i0 = bi * kTile, j0 = bj * kTile;
        float acc[8][8];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[a][b] = 0.0f;
        for (int d0 = 0; d0 < p.D; d0 += kChunk) {
            const int dn = p.D - d0 < kChunk ? p.D - d0 : kChunk;
            __syncthreads();                                 // the previous chunk (or tile) is consumed
            stage(p, A, i0, d0, dn);
            stage(p, B, j0, d0, dn);
            __syncthreads();
            for (int d = 0; d < dn; ++d) column(A[d], B[d], ty, tx, acc);
        }
        unsigned up = 0, dg = 0;
        if (bi != bj && j0 + kTile <= p.N) {                 // a full tile above the diagonal: every pair has i < j < N
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) up += acc[a][b] < p.eps ? 1u : 0u;
        } else {                                             // diagonal and edge tiles: masked by index
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                const int64_t gi = i0 + (a / 4) * 64 + ty * 4 + (a % 4);
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const int64_t gj = j0 + (b / 4) * 64 + tx * 4 + (b % 4);
                    const bool hit = acc[a][b] < p.eps && gj < p.N;      // (a counted pair has gi <= gj, so gi < N as well)
                    up += hit && gi < gj ? 1u : 0u;
                    dg += hit && gi == gj ? 1u : 0u;
                }
            }
        }
        upper += up;
        diag += dg;
    }
    // block reduce in 64 bits: a butterfly inside each wave, then the four wave sums through LDS
    for (int o = kWave / 2; o > 0; o >>= 1) {
        upper += __shfl_xor(upper, o, kWave);
        diag += __shfl_xor(diag, o, kWave);
    }
    if (threadIdx.x % kWave == 0) { red[0][threadIdx.x / kWave] = upper; red[1][threadIdx.x / kWave] = diag; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long u = 0, g = 0;
        for (int w = 0; w < kThreads / kWave; ++w) { u += red[0][w]; g += red[1][w]; }
        p.part[2 * (int64_t)blockIdx.x] = u;
        p.part[2 * (int64_t)blockIdx.x + 1] = g;
    }
}

// out[0] = sum of the blocks' upper counts, out[1] = of their diag counts: one block, integer sums, any order is exact
__global__ void __launch_bounds__(kThreads) collision_finish_kernel(const unsigned long long* part, int nblocks, int64_t* out) {
    __shared__ unsigned long long red[2][kThreads / kWave];
    unsigned long long u = 0, g = 0;
    for (int b = threadIdx.x; b < nblocks; b += kThreads) { u += part[2 * b]; g += part[2 * b + 1]; }
    for (int o = kWave / 2; o > 0; o >>= 1) {
        u += __shfl_xor(u, o, kWave);
        g += __shfl_xor(g, o, kWave);
    }
    if (threadIdx.x % kWave == 0) { red[0][threadIdx.x / kWave] = u; red[1][threadIdx.x / kWave] = g; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u = g = 0;
        for (int w = 0; w < kThreads / kWave; ++w) { u += red[0][w]; g += red[1][w]; }
        out[0] = (int64_t)u;
        out[1] = (int64_t)g;
    }
}

int64_t tile_rows(int64_t N) { return (N + kTile - 1) / kTile; }

// tiles of the upper triangle, saturated at kMaxGrid (all the grid and the workspace need to know)
int64_t tiles_capped(int64_t N) {
    const int64_t T = tile_rows(N);
    return T >= 128 ? kMaxGrid : (T * (T + 1) / 2 < kMaxGrid ? T * (T + 1) / 2 : kMaxGrid);     // (128 * 129 / 2 > kMaxGrid)
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int64_t kpgnn_collision_workspace_bytes(int64_t N) {
    if (N < 0) return 0;
    const int64_t blocks = tiles_capped(N);
    return (blocks < 1 ? 1 : blocks) * 2 * (int64_t)sizeof(unsigned long long);
}

extern "C" int kpgnn_collision_count(const kpgnn_collision_desc* d, kpgnn_stream_t stream) {
    KPGNN_REQUIRE(d != nullptr, "collision_count: NULL descriptor");
    KPGNN_REQUIRE(d->N >= 0 && d->D >= 1 && d->D <= kMaxD, "collision_count: bad N=%lld D=%d (1 <= D <= %d)", (long long)d->N, d->D, kMaxD);
    KPGNN_REQUIRE(std::isfinite(d->eps) && d->eps >= 0.0f, "collision_count: eps=%g is not a finite, non-negative number", (double)d->eps);
    KPGNN_REQUIRE(d->x && d->out && d->workspace && d->x_stride >= d->D, "collision_count: NULL x/out/workspace or bad stride");
    KPGNN_REQUIRE(((uintptr_t)d->workspace % 8) == 0 && d->workspace_bytes >= kpgnn_collision_workspace_bytes(d->N),
                  "collision_count: workspace of %lld bytes, need %lld (8-byte aligned)", (long long)d->workspace_bytes,
                  (long long)kpgnn_collision_workspace_bytes(d->N));
    if (d->N == 0) return KPGNN_OK;
    CollParams p = {};
    p.x = d->x; p.xs = d->x_stride; p.N = d->N; p.D = d->D; p.eps = d->eps;
    const int64_t T = tile_rows(d->N);
    p.tiles = T * (T + 1) / 2;
    p.part = (unsigned long long*)d->workspace;
    // a persistent grid of one resident round: 64 accumulators a thread leave room for 4 blocks of 256 threads a CU at best
    int nb = resident_blocks(collision_tiles_kernel, kThreads, 0);
    nb = nb < 1 ? 1 : (nb > 4 ? 4 : nb);
    int64_t grid = (int64_t)nb * device_facts().cu_count;
    if (grid > kMaxGrid) grid = kMaxGrid;
    if (grid > p.tiles) grid = p.tiles;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(collision_tiles_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, p);
    KPGNN_LAUNCH_CHECK("collision_tiles_kernel");
    hipLaunchKernelGGL(collision_finish_kernel, dim3(1), dim3(kThreads), 0, s, p.part, (int)grid, d->out);
    KPGNN_LAUNCH_CHECK("collision_finish_kernel");
    return KPGNN_OK;
}
