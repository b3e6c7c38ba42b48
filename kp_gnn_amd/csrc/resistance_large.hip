// Resistance-distance node feature for graphs of up to 2048 nodes (gfx950).  Contract: include/kpgnn.h,
// kpgnn_resistance_distance_large.  csrc/resistance.hip is the specification: steps 1-6 of its header and the meaning of every
// status apply unchanged; what differs is where the matrix lives and how the inverse is formed.
//
// One workgroup of 1024 threads owns one graph.  Its matrix is a slab of the caller's workspace: with np = n rounded up to the
// panel width b = 32 and the ODD row stride s = np + 1, np x s doubles, then the row panel R [b, np] and the column panel C
// [np, b] of the current block step.  Rows and columns n .. np-1 are the identity: they are their own inverse, every product
// they take part in is an exact +-0, so the bits of the real entries are those of the unpadded matrix.  Everything a slab holds
// is written and read by this one workgroup and ordered by block barriers; nothing crosses workgroups.
//   1. counts: integers in the slab (the low word of each slot), global integer atomics;
//   2. symmetry by pairs of 32 x 32 tiles read row-wise and transposed through LDS, degrees by a wavefront per row: both
//      coalesced;
//   3. components by hooking over the graph's EDGE LIST (a root is hooked below the smaller label with an LDS atomicMin) and
//      full pointer jumping each round, labels and sizes in LDS.  After the jumping every label is a root, so the first hook of a
//      round lowers a label: a round changes one or ends the loop, at most n rounds of at most n jump passes, both capped;
//   4. M = D - A + sum_c (1/m_c) 1_c 1_c^T in double over the counts, slot by slot;
//   5. M^-1 in place by BLOCKED Gauss-Jordan without pivoting.  Per block step K: the b x b diagonal block P is inverted in LDS
//      by the unblocked sweep of resistance.hip (a Schur complement of an SPD matrix, hence SPD; a pivot that is not positive
//      and finite ends the graph with status 3), R = P^-1 M[K,:] and C = M[:,K] go to the side buffers, every other tile takes
//      M[I,J] -= C[I] R[J] - a 128 x 128 macro tile per pass, 4 x 4 doubles in the registers of each thread, the C / R
//      sub-panels staged in LDS, plain double FMAs over the panel index in ascending order - and M[K,:] = R,
//      M[:,K] = -C P^-1, M[K,K] = P^-1.  The unblocked form moves all n^2 doubles once per pivot; this one once per b pivots;
//   6. L+ and the feature as resistance.hip has them.
// No float atomics, a fixed order everywhere: a graph's bits depend on the graph alone, not on the batch, the chunking or the
// workspace around it.
#include "kpgnn_common.h"

#include <cmath>

namespace kpgnn {
namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kB = 32;              // panel width b; the thread grid is kB x kB
constexpr int kTile = 4 * kB;       // macro tile edge: 4 x 4 doubles per thread
constexpr int kPLd = kB + 1;        // odd row stride of the LDS blocks read by column
constexpr int kLargeCap = KPGNN_RD_LARGE_MAX_NODES;
static_assert(kThreads == kB * kB, "one thread per element of a b x b block");

struct RdLargeParams {
    int G, n_ids, cap;
    const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* ei; int64_t E;
    const int32_t* ids;
    float* out; int32_t* status;
    double* ws; int64_t slab;       // doubles per graph
};

__host__ __device__ constexpr int64_t padded(int n) { return ((int64_t)n + kB - 1) / kB * kB; }
// doubles of one slab sized for graphs of up to `cap` nodes: the matrix, the row panel, the column panel
__host__ __device__ constexpr int64_t slab_doubles(int cap) {
    return padded(cap) * (padded(cap) + 1) + 2 * (int64_t)kB * padded(cap);
}

// LDS: C sub-panel [kTile][kPLd], R sub-panel [kB][kTile], P [kB][kPLd], pivot row and column, label / size / degree, flags
constexpr size_t kLdsBytes = (size_t)(kTile * kPLd + kB * kTile + kB * kPLd + 2 * kB) * 8 + (size_t)3 * kLargeCap * 4 + 16;

__global__ void __launch_bounds__(kThreads) rd_large_kernel(const RdLargeParams p) {
    extern __shared__ __attribute__((aligned(16))) double rdl_lds[];
    const int tid = (int)threadIdx.x, tx = tid & (kB - 1), ty = tid / kB, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t slot = (int64_t)blockIdx.x;
    if (slot >= p.n_ids) return;
    const int g = p.ids[slot];
    if (g < 0 || g >= p.G) return;
    const int64_t n0 = p.node_ptr[g], n64 = p.node_ptr[g + 1] - n0;
    if (n64 <= 0) {
        if (tid == 0) p.status[g] = n64 == 0 ? KPGNN_RD_OK : KPGNN_RD_RANGE;
        return;
    }
    if (n64 > p.cap) {
        if (tid == 0) p.status[g] = KPGNN_RD_TOO_LARGE;
        return;
    }
    const int n = (int)n64, np = (int)padded(n), s = np + 1;
    int64_t e0 = p.edge_ptr[g], e1 = p.edge_ptr[g + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > p.E ? p.E : e1;

    double* M = p.ws + slot * p.slab;
    int* Mi = reinterpret_cast<int*>(M);                        // the count of slot q lives in Mi[2 q] until step 4
    double* Rbuf = M + (int64_t)np * s;                         // [kB][np]
    double* Cbuf = Rbuf + (int64_t)kB * np;                     // [np][kB]
    double* Cs = rdl_lds;
    double* Rs = Cs + kTile * kPLd;
    double* Ps = Rs + kB * kTile;
    double* rowk = Ps + kB * kPLd;
    double* colk = rowk + kB;
    int* label = reinterpret_cast<int*>(colk + kB);
    int* msize = label + kLargeCap;                             // indexed by ROOT: the size of its component
    int* deg = msize + kLargeCap;
    int* flags = deg + kLargeCap;                               // [0] bad input, [1] a hook was made, [2] a jump was made
    int* T1 = reinterpret_cast<int*>(Cs);                       // step 2's two count tiles [kB][kPLd] lie over the sub-panels
    int* T2 = reinterpret_cast<int*>(Rs);

    // 1. counts
    for (int q = tid; q < np * s; q += kThreads) reinterpret_cast<long long*>(M)[q] = 0;
    if (tid < 3) flags[tid] = 0;
    __syncthreads();
    for (int64_t e = e0 + tid; e < e1; e += kThreads) {
        const int64_t u = p.ei[e] - n0, v = p.ei[p.E + e] - n0;
        if (u < 0 || u >= n || v < 0 || v >= n) flags[0] = 1;
        else if (u != v) atomicAdd(&Mi[2 * ((int)u * s + (int)v)], 1);
    }
    __syncthreads();
    if (flags[0]) {
        if (tid == 0) p.status[g] = KPGNN_RD_RANGE;
        return;
    }
    __syncthreads();            // (everyone has read flags[0] before it is written again)

    // 2. symmetry: tile (bi, bj) against the transpose of tile (bj, bi); degrees: a wavefront per row
    const int nblk = np / kB;
    int bad = 0;
    for (int bi = 0; bi < nblk; ++bi)
        for (int bj = bi; bj < nblk; ++bj) {
            T1[ty * kPLd + tx] = Mi[2 * ((bi * kB + ty) * s + bj * kB + tx)];
            T2[ty * kPLd + tx] = Mi[2 * ((bj * kB + ty) * s + bi * kB + tx)];
            __syncthreads();
            bad |= T1[ty * kPLd + tx] != T2[tx * kPLd + ty];
            __syncthreads();
        }
    if (bad) flags[0] = 1;
    for (int i = wave; i < n; i += kWaves) {
        int d = 0;
        for (int c = lane; c < n; c += kWave) d += Mi[2 * (i * s + c)];
        for (int o = kWave >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, kWave);
        if (lane == 0) deg[i] = d;
    }
    for (int i = tid; i < n; i += kThreads) { label[i] = i; msize[i] = 0; }
    __syncthreads();
    if (flags[0]) {
        if (tid == 0) p.status[g] = KPGNN_RD_ASYMMETRIC;
        return;
    }

    // 3. components.  label[i] <= i always and label[i] is a node of i's component, so the labels are a forest whose roots are
    // the nodes with label[i] == i; labels only ever decrease.  A round ends with every label a root; the loop ends when no edge
    // joins two roots, and then the root of a component is its smallest node.
    for (int round = 0;; ++round) {
        if (round > n) {                                        // (at most n - 1 rounds can hook)
            if (tid == 0) p.status[g] = KPGNN_RD_PIVOT;
            return;
        }
        __syncthreads();
        if (tid == 0) flags[1] = 0;
        __syncthreads();
        for (int64_t e = e0 + tid; e < e1; e += kThreads) {
            const int u = (int)(p.ei[e] - n0), v = (int)(p.ei[p.E + e] - n0);
            const int lu = label[u], lv = label[v];
            if (lu != lv) {
                atomicMin(&label[lu > lv ? lu : lv], lu < lv ? lu : lv);
                flags[1] = 1;
            }
        }
        __syncthreads();
        if (!flags[1]) break;
        for (int pass = 0;; ++pass) {
            if (pass > n) {                                     // (a pass halves the depth of the forest)
                if (tid == 0) p.status[g] = KPGNN_RD_PIVOT;
                return;
            }
            __syncthreads();
            if (tid == 0) flags[2] = 0;
            __syncthreads();
            for (int i = tid; i < n; i += kThreads) {
                const int l = label[i], ll = label[l];
                if (ll < l) { label[i] = ll; flags[2] = 1; }
            }
            __syncthreads();
            if (!flags[2]) break;
        }
    }
    for (int i = tid; i < n; i += kThreads) atomicAdd(&msize[label[i]], 1);
    __syncthreads();

    // 4. M over the counts: every thread converts the slots it reads; the padding is the identity
    for (int i = wave; i < np; i += kWaves)
        for (int j = lane; j < np; j += kWave) {
            const int q = i * s + j;
            double v;
            if (i < n && j < n) {
                const int a = Mi[2 * q], li = label[i];
                const double proj = li == label[j] ? 1.0 / (double)msize[li] : 0.0;
                v = (i == j ? (double)deg[i] : -(double)a) + proj;
            } else {
                v = i == j ? 1.0 : 0.0;
            }
            M[q] = v;
        }
    __syncthreads();

    // 5. blocked Gauss-Jordan in place, no pivoting
    for (int K = 0; K < nblk; ++K) {
        const int k0 = K * kB;
        // P^-1 in LDS by the unblocked sweep
        Ps[ty * kPLd + tx] = M[(k0 + ty) * s + k0 + tx];
        __syncthreads();
        for (int k = 0; k < kB; ++k) {
            const double piv = Ps[k * kPLd + k];
            if (!(piv > 0.0) || !(piv < INFINITY)) {
                if (tid == 0) p.status[g] = KPGNN_RD_PIVOT;
                return;
            }
            if (tid < kB) {
                rowk[tid] = Ps[k * kPLd + tid] / piv;
                colk[tid] = Ps[tid * kPLd + k];
            }
            __syncthreads();
            {
                const double r = rowk[tx];
                double v;
                if (ty == k) v = tx == k ? 1.0 / piv : r;
                else if (tx == k) v = -colk[ty] / piv;
                else v = fma(-colk[ty], r, Ps[ty * kPLd + tx]);
                Ps[ty * kPLd + tx] = v;
            }
            __syncthreads();
        }
        // R = P^-1 M[K,:] (the columns of block K excepted), 128 columns of M[K,:] through LDS at a time
        for (int J0 = 0; J0 < np; J0 += kTile) {
            for (int c = tx; c < kTile && J0 + c < np; c += kB) Rs[ty * kTile + c] = M[(k0 + ty) * s + J0 + c];
            __syncthreads();
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const int j = J0 + c4 * kB + tx;
                if (J0 + c4 * kB < np && J0 / kB + c4 != K) {
                    double acc = 0.0;
#pragma unroll 8
                    for (int t = 0; t < kB; ++t) acc = fma(Ps[ty * kPLd + t], Rs[t * kTile + c4 * kB + tx], acc);
                    Rbuf[ty * np + j] = acc;
                }
            }
            __syncthreads();
        }
        // C = M[:,K]
        for (int i = ty; i < np; i += kB) Cbuf[i * kB + tx] = M[i * s + k0 + tx];
        __syncthreads();
        // every other tile: M[I,J] -= C[I] R[J]; and M[I,K] = -C[I] P^-1 while C[I] is staged
        for (int I0 = 0; I0 < np; I0 += kTile) {
            bool ra[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) ra[a] = I0 + a * kB < np && I0 / kB + a != K;
            for (int r = ty; r < kTile && I0 + r < np; r += kB) Cs[r * kPLd + tx] = Cbuf[(I0 + r) * kB + tx];
            __syncthreads();
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (ra[a]) {
                    double acc = 0.0;
#pragma unroll 8
                    for (int t = 0; t < kB; ++t) acc = fma(Cs[(a * kB + ty) * kPLd + t], Ps[t * kPLd + tx], acc);
                    M[(I0 + a * kB + ty) * s + k0 + tx] = -acc;
                }
            for (int J0 = 0; J0 < np; J0 += kTile) {
                bool ca[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) ca[c] = J0 + c * kB < np && J0 / kB + c != K;
                for (int c = tx; c < kTile && J0 + c < np; c += kB) Rs[ty * kTile + c] = Rbuf[ty * np + J0 + c];
                double acc[4][4];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        acc[a][c] = ra[a] && ca[c] ? M[(I0 + a * kB + ty) * s + J0 + c * kB + tx] : 0.0;
                __syncthreads();
#pragma unroll 4
                for (int t = 0; t < kB; ++t) {
                    double cv[4], rv[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) cv[a] = -Cs[(a * kB + ty) * kPLd + t];
#pragma unroll
                    for (int c = 0; c < 4; ++c) rv[c] = Rs[t * kTile + c * kB + tx];
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[a][c] = fma(cv[a], rv[c], acc[a][c]);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (ra[a] && ca[c]) M[(I0 + a * kB + ty) * s + J0 + c * kB + tx] = acc[a][c];
                __syncthreads();        // (the sub-panels are read to the end before the next pass stages over them)
            }
        }
        // M[K,:] = R, M[K,K] = P^-1
        for (int j = tx; j < np; j += kB) M[(k0 + ty) * s + j] = j / kB != K ? Rbuf[ty * np + j] : Ps[ty * kPLd + j - k0];
        __syncthreads();
    }

    // 6. L+ and the feature
    const int lab0 = label[0];
    const double j0 = 1.0 / (double)msize[lab0];
    const double l00 = M[0] - j0;
    for (int y = tid; y < n; y += kThreads) {
        const int ly = label[y];
        const double same = ly == lab0 ? j0 : 0.0;
        const double lyy = M[y * s + y] - 1.0 / (double)msize[ly];
        const double l0y = M[y] - same, ly0 = M[y * s] - same;
        p.out[n0 + y] = (float)(((l00 + lyy) - l0y) - ly0);
    }
    if (tid == 0) p.status[g] = KPGNN_RD_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" size_t kpgnn_rd_large_workspace_bytes(int32_t max_nodes, int32_t n_ids) {
    if (max_nodes < 1 || max_nodes > kLargeCap || n_ids < 0) return 0;
    return (size_t)n_ids * (size_t)slab_doubles(max_nodes) * 8;
}

extern "C" int kpgnn_resistance_distance_large(const kpgnn_rd_large_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_resistance_distance_large";
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->G >= 0 && d->n_ids >= 0 && d->E >= 0, "%s: bad G=%d n_ids=%d E=%lld", who, d->G, d->n_ids, (long long)d->E);
    if (d->G == 0 || d->n_ids == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->node_ptr && d->edge_ptr && d->graph_ids && d->out && d->status, "%s: NULL node_ptr/edge_ptr/graph_ids/out/status", who);
    KPGNN_REQUIRE(d->E == 0 || d->edge_index, "%s: NULL edge_index", who);
    KPGNN_REQUIRE(d->max_nodes >= 1, "%s: bad max_nodes=%d", who, d->max_nodes);
    if (d->max_nodes > kLargeCap) return fail(KPGNN_ELIMIT, "%s: max_nodes=%d is beyond the cap of %d nodes per graph", who, d->max_nodes, kLargeCap);
    const size_t need = kpgnn_rd_large_workspace_bytes(d->max_nodes, d->n_ids);
    KPGNN_REQUIRE(d->workspace != nullptr && d->workspace_bytes >= need, "%s: workspace of %zu bytes at %p, %zu needed", who,
                  d->workspace_bytes, d->workspace, need);
    KPGNN_REQUIRE(((uintptr_t)d->workspace & 7) == 0, "%s: workspace is not 8-byte aligned", who);
    RdLargeParams p = {};
    p.G = d->G; p.n_ids = d->n_ids; p.cap = d->max_nodes;
    p.node_ptr = d->node_ptr; p.edge_ptr = d->edge_ptr; p.ei = d->edge_index; p.E = d->E;
    p.ids = d->graph_ids; p.out = d->out; p.status = d->status;
    p.ws = static_cast<double*>(d->workspace); p.slab = slab_doubles(d->max_nodes);
    hipStream_t s = (hipStream_t)stream;
    KPGNN_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&rd_large_kernel), kLdsBytes));
    hipLaunchKernelGGL(rd_large_kernel, dim3((unsigned)d->n_ids), dim3(kThreads), kLdsBytes, s, p);
    KPGNN_LAUNCH_CHECK("rd_large_kernel");
    return KPGNN_OK;
}
