// The per-graph row walk of the graph-level kernels (pool.hip, virtual_node.hip; pool_max.hip writes the walk out around its
// conditional fold and says why; attn_pool.hip has a two-row loop of its own and takes graph_rows alone).  Collated batches
// keep the nodes of a graph contiguous, so a per-graph operator is a segmented walk: a sub-group of L lanes owns graph g, its
// lanes span the feature columns VEC floats (up to 16 B) wide, and the graph's rows are folded in node order - one launch, no
// atomics, the same bits every run.
#pragma once
#include "kpgnn_common.h"

namespace kpgnn {

// The live node range of graph g: graph_ptr clamped to the live row count N (live_rows), so that no row at or beyond it is
// touched whatever the pointer says - a pointer built from a batch vector whose dead tail repeats the last graph id ends at
// the capacity.  The one place this rule is written.
struct GraphRows { int beg, end; };
__device__ __forceinline__ GraphRows graph_rows(const int32_t* ptr, int64_t g, int64_t N) {
    const int n = (int)(N < INT32_MAX ? N : INT32_MAX);     // (graph_ptr is int32: it names no row beyond; 32-bit min / max)
    return {min(max(ptr[g], 0), n), min(ptr[g + 1], n)};
}

// f(v, r) for the rows r = beg .. end - 1 of x in node order, v the VEC columns of row r from column c0 on (f may change v).
// Each trip issues four independent row loads and then folds the four rows in row order; the tail goes one row at a time.
template <int VEC, typename F>
__device__ __forceinline__ void for_graph_rows(const float* x, int64_t xs, int c0, int beg, int end, F&& f) {
    int r = beg;
    for (; r + 3 < end; r += 4) {
        float v[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) ldv<VEC>(x + (int64_t)(r + u) * xs + c0, v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) f(v[u], r + u);
    }
    for (; r < end; ++r) {
        float v[VEC];
        ldv<VEC>(x + (int64_t)r * xs + c0, v);
        f(v, r);
    }
}

// Blocks of a launch: a sub-group per graph (the forward walks), or four rows per sub-group up to 8 blocks per CU and a
// grid-stride loop beyond (the backward scatters of a [G,D] operand over the rows).
inline unsigned graph_grid(int64_t G, int lanes) { return (unsigned)((G + (kRowBlock / lanes) - 1) / (kRowBlock / lanes)); }
inline unsigned row_grid(int64_t N, int lanes) {
    const int rows = kRowBlock / lanes;
    const int64_t g = (N + rows * 4 - 1) / (rows * 4), cap = (int64_t)device_facts().cu_count * 8;
    return (unsigned)(g > cap ? cap : (g < 1 ? 1 : g));
}

// Picks the row shape of D columns under the alignment of `ptrs` and `strides` (row_vec), refuses a row that needs more than
// 256 lanes (KPGNN_ELIMIT), and launches kernel_of(V, L) = kernel<VEC, L> with grid(count, L) blocks; `who` heads the error
// texts, `name` is the kernel's in a launch failure.
template <typename Params, typename KernelOf>
int launch_row_walk(int D, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> strides, const char* who,
                    const char* name, unsigned (*grid)(int64_t, int), int64_t count, const Params& p, hipStream_t s,
                    KernelOf&& kernel_of) {
    const int vec = row_vec(D, ptrs, strides);
    if ((D + vec - 1) / vec > 256) return fail(KPGNN_ELIMIT, "%s: D=%d too wide", who, D);
    const int lanes = row_lanes(D, vec);
    return dispatch_row_shape<256>(vec, lanes, who, [&](auto V, auto L) {
        void (*kernel)(Params) = kernel_of(V, L);
        hipLaunchKernelGGL(kernel, dim3(grid(count, lanes)), dim3(kRowBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK(name);
        return KPGNN_OK;
    });
}

}  // namespace kpgnn
