// Two column sums over the live rows, sum f and sum f * m, as one partial double[2][C] per block (body_norm.hip: x and x^2
// forward, gout and gout * x backward; rd_proj.hip: dy and rd * dy).  A group of G lanes owns a row, VEC columns per lane (the
// shared row shapes); every thread sums its columns over the block's rows in DOUBLE (a product of two fp32 values is exact
// there), the block adds its row groups in group order.  EVERY block writes its partial, zeros included, so the workspace need
// not be cleared and a block without a live row contributes exactly nothing.  A finalize kernel of the caller adds the partials
// in an order of its own.
#pragma once
#include "kpgnn_common.h"

namespace kpgnn {

constexpr int kMaxStatGrid = 256;    // one block per CU: the finalize block reads P * 16 C bytes of partials alone
constexpr int kFinBlock = 1024;
constexpr int kMaxSlices = 16;
constexpr int kMaxApplyGrid = 2048;  // 256 CUs x 8 blocks: grid-stride beyond

// statistics blocks of N capacity rows at `rows` rows per block, until the grid stops growing
inline int stat_blocks(int64_t N, int rows) {
    const int64_t b = (N + rows - 1) / rows;
    return (int)(b < 1 ? 1 : (b > kMaxStatGrid ? kMaxStatGrid : b));
}

// The body of a statistics block (every thread of the block calls): rows blockIdx.x * R + group, then every `step` rows, below
// the live count n; load(row, f, m) fills the VEC columns from c0 = lane * VEC on; the partial goes to part[blockIdx.x][2][C].
template <int VEC, int G, typename Load>
__device__ __forceinline__ void column_stats_block(int64_t n, int64_t step, int C, double* part, Load&& load) {
    constexpr int R = kRowBlock / G, W = G * VEC;       // rows per pass; columns a pass spans (>= C)
    __shared__ double sm[2 * kRowBlock * VEC];          // [2][R][W]
    const int lane = threadIdx.x % G, rg = threadIdx.x / G, c0 = lane * VEC;
    double a0[VEC], a1[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) a0[j] = a1[j] = 0.0;
    if (c0 < C) {
        int64_t row = (int64_t)blockIdx.x * R + rg;
        for (; row + 3 * step < n; row += 4 * step) {      // four rows' loads in flight, added in row order
            float f[4][VEC], m[4][VEC];
#pragma unroll
            for (int q = 0; q < 4; ++q) load(row + q * step, f[q], m[q]);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    a0[j] += (double)f[q][j];
                    a1[j] = fma((double)f[q][j], (double)m[q][j], a1[j]);
                }
        }
        for (; row < n; row += step) {
            float f[VEC], m[VEC];
            load(row, f, m);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                a0[j] += (double)f[j];
                a1[j] = fma((double)f[j], (double)m[j], a1[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        sm[(0 * R + rg) * W + c0 + j] = a0[j];
        sm[(1 * R + rg) * W + c0 + j] = a1[j];
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        double t0 = 0.0, t1 = 0.0;
        for (int q = 0; q < R; ++q) { t0 += sm[(0 * R + q) * W + c]; t1 += sm[(1 * R + q) * W + c]; }
        double* dst = part + (int64_t)blockIdx.x * 2 * C;
        dst[c] = t0;
        dst[C + c] = t1;
    }
}

}  // namespace kpgnn
