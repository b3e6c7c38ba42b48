// Tile helpers of the dense kernels on the fp32 matrix instruction v_mfma_f32_32x32x2_f32 (gfx950): lin_fused_kernel
// (lin_fused.h), linear_wide_kernel (linear_wide.hip), linear_group_kernel (linear_group.hip); the row pitch also serves
// table_grad_mfma.hip and hop_mlp.hip.
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

}  // namespace kpgnn
