// Tile helpers of the dense kernels on the fp32 matrix instruction v_mfma_f32_32x32x2_f32 (gfx950): lin_fused_kernel
// (lin_fused.h), linear_wide_kernel (linear_wide.hip), linear_group_kernel (linear_group.hip); the row pitch also serves
// table_grad_mfma.hip, hop_mlp.hip and sage_tail.hip; the last two also share the 32-node tile helpers at the end.
#pragma once
#include "bf3.h"            // f32x16
#include "kpgnn_common.h"

namespace kpgnn {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }

// Row pitch of an LDS tile of `width` floats: the next value = 4 (mod 8), i.e. 16-B aligned rows whose 16-B accesses (and the
// matrix instruction's operand reads down a column) are free of bank conflicts.
inline int mfma_pitch(int width) { return width + ((4 - width % 8) + 8) % 8; }

// Rows per tile = 32 * m with m the smallest of `ms` (ascending) that makes the launch one round over the `slots` block slots
// of the chip, else the largest; the grid is one block per tile up to the slots.  twice_at_1: at m = 1 the 32-row tiles are
// short enough that two rounds of blocks measured faster than one of 64-row tiles.
struct TilePlan { int m, rows; int64_t tiles; unsigned grid; };
inline TilePlan tile_plan(int64_t N, int64_t slots, std::initializer_list<int> ms, bool twice_at_1) {
    TilePlan t;
    const int64_t need = (N + slots * 32 - 1) / (slots * 32);
    t.m = *(ms.end() - 1);
    for (auto it = ms.end(); it != ms.begin();)
        if (*--it >= need) t.m = *it;
    t.rows = 32 * t.m;
    t.tiles = (N + t.rows - 1) / t.rows;
    const int64_t cap = (twice_at_1 && t.m == 1) ? slots * 2 : slots;
    t.grid = (unsigned)(cap < t.tiles ? cap : t.tiles);
    return t;
}

// The k-loops are fully unrolled: a kernel exists per input width.  Each kernel names the widths it instantiates;
// f(std::integral_constant<int, KS>), KS = I / 2, launches kernel<KS, ...> and returns the status.
template <int... Ws>
struct MfmaWidths {
    static bool has(int I) { return ((I == Ws) || ...); }
    template <typename F>
    static int dispatch(int I, const char* who, F&& f) {
        int rc = KPGNN_OK;
        if (((I == Ws ? (rc = f(std::integral_constant<int, Ws / 2>{}), true) : false) || ...)) return rc;
        return refuse(I, who);
    }
    static int refuse(int I, const char* who) {
        char list[64];
        int n = 0;
        for (int w : {Ws...}) n += snprintf(list + n, sizeof(list) - n, n ? ", %d" : "%d", w);
        return fail(KPGNN_ELIMIT, "%s: I=%d is not one of %s (the k-loop is fully unrolled)", who, I, list);
    }
};
using LinWidths = MfmaWidths<32, 64, 96, 104, 128>;     // lin_fused_kernel, linear_group_kernel (ops_dense._LIN_WIDTHS)
using WideWidths = MfmaWidths<32, 64, 104, 128>;        // linear_wide_kernel

// ---- 32-node LDS tiles on v_mfma_f32_16x16x4_f32 (exact fp32): shared by hop_mlp.hip and sage_tail.hip
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kTN = 32;          // nodes per tile (2 row groups of 16)
constexpr int kHmThreads = 256;
constexpr int kHmWaves = 4;
constexpr int kNPF = 4;          // float4 registers per thread of a prefetched tile (covers rows up to 128 floats)
constexpr int kMaxCols = 4;      // activation columns a thread may own in the column passes (row width <= 1024)

// One [rows, K*d] (or [rows, H]) tensor <-> the LDS tile [kTN][LD] whose hop slots are Dm wide.
struct TileIO {
    int ncol, d, Dm, LD, vec;
    int lo[kNPF];                // LDS offset of this thread's q-th float4 (vec path), -1 beyond the tile
    __device__ void init(int ncol_, int d_, int Dm_, int LD_, int vec_) {
        ncol = ncol_; d = d_; Dm = Dm_; LD = LD_; vec = vec_ && (d_ == Dm_);
#pragma unroll
        for (int q = 0; q < kNPF; ++q) {
            const int e = 4 * (threadIdx.x + q * kHmThreads);
            lo[q] = e < kTN * ncol ? (e / ncol) * LD + (e % ncol) : -1;
        }
    }
    __device__ __forceinline__ int lds_col(int c) const { return d == Dm ? c : (c / d) * Dm + (c % d); }
    // issue the loads of a tile into registers (vec path only; the scalar path loads at commit time)
    __device__ __forceinline__ void issue(float4 (&r)[kNPF], const float* __restrict__ src, int rows) const {
        if (!vec) return;
#pragma unroll
        for (int q = 0; q < kNPF; ++q) {
            const int e = 4 * (threadIdx.x + q * kHmThreads);
            r[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < rows * ncol) r[q] = *reinterpret_cast<const float4*>(src + e);
        }
    }
    // registers (+ whatever did not fit, + everything on the scalar path) -> LDS; rows beyond `rows` become zero
    __device__ __forceinline__ void commit(const float4 (&r)[kNPF], float* buf, const float* __restrict__ src, int rows) const {
        if (vec) {
#pragma unroll
            for (int q = 0; q < kNPF; ++q)
                if (lo[q] >= 0) *reinterpret_cast<float4*>(buf + lo[q]) = r[q];
            for (int e = 4 * (threadIdx.x + kNPF * kHmThreads); e < kTN * ncol; e += 4 * kHmThreads) {
                const int n = e / ncol;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (n < rows) v = *reinterpret_cast<const float4*>(src + e);
                *reinterpret_cast<float4*>(buf + n * LD + (e - n * ncol)) = v;
            }
        } else {
            for (int e = threadIdx.x; e < kTN * ncol; e += kHmThreads) {
                const int n = e / ncol;
                buf[n * LD + lds_col(e - n * ncol)] = n < rows ? src[e] : 0.f;
            }
        }
    }
    __device__ __forceinline__ void store(float* __restrict__ dst, const float* buf, int rows) const {
        if (vec) {
#pragma unroll
            for (int q = 0; q < kNPF; ++q) {
                const int e = 4 * (threadIdx.x + q * kHmThreads);
                if (e < rows * ncol) *reinterpret_cast<float4*>(dst + e) = *reinterpret_cast<const float4*>(buf + lo[q]);
            }
            for (int e = 4 * (threadIdx.x + kNPF * kHmThreads); e < rows * ncol; e += 4 * kHmThreads) {
                const int n = e / ncol;
                *reinterpret_cast<float4*>(dst + e) = *reinterpret_cast<const float4*>(buf + n * LD + (e - n * ncol));
            }
        } else {
            for (int e = threadIdx.x; e < rows * ncol; e += kHmThreads) {
                const int n = e / ncol;
                dst[e] = buf[n * LD + lds_col(e - n * ncol)];
            }
        }
    }
};

// acc[rg][t] += A_rg * B for both 16-row groups of the tile: A = rows of `bin`, columns a0 .. a0+din; B = wl, `din`
// rows (zero padded beyond) of pitch `pitch`, column tiles t.  Two independent MFMA chains per column tile.
template <int T>
__device__ __forceinline__ void tile_times_weights(f32x4 (&acc)[2][T], const float* bin, int a0, int din, const float* wl,
                                                   int pitch, int LD, int lr, int lq) {
    const float* ar0 = bin + lr * LD + a0;
    const float* ar1 = ar0 + 16 * LD;
    const int qn = (din + 3) >> 2;
#pragma unroll 2
    for (int q = 0; q < qn; ++q) {
        const int kk = 4 * q + lq;
        const int kc = kk < din ? kk : din - 1;
        float a0v = ar0[kc], a1v = ar1[kc];
        a0v = kk < din ? a0v : 0.f;
        a1v = kk < din ? a1v : 0.f;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const float b = wl[kk * pitch + t * 16 + lr];
            acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0v, b, acc[0][t], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v, b, acc[1][t], 0, 0, 0);
        }
    }
}

// Column passes: a thread owns activation column c (row lanes rl share a column when the row is narrower than the block).
struct ColMap {
    int R, rl, c0; bool on;
    __device__ void init(int ncol) {
        R = kHmThreads / ncol;
        R = R < 1 ? 1 : (R > kTN ? kTN : R);
        rl = ncol < kHmThreads ? (int)threadIdx.x / ncol : 0;
        c0 = ncol < kHmThreads ? (int)threadIdx.x - rl * ncol : (int)threadIdx.x;
        on = ncol < kHmThreads ? rl < R : true;
    }
};

}  // namespace kpgnn
