// Resistance-distance node feature, batched over graphs (gfx950).  Contract: include/kpgnn.h, kpgnn_resistance_distance.
//
// The reference (data_utils.py:280-303) runs scipy per graph on the host: a dense Laplacian of the summed adjacency and
// linalg.pinv, an SVD - in float32, since PyG's to_scipy_sparse_matrix fills float32 ones.  Here one workgroup owns one graph
// and never factors a singular matrix:
//   1. the integer count matrix A in LDS by LDS integer atomics (ones add to integers: no dependence on the edge order);
//      the diagonal is ignored, an endpoint outside the graph ends the graph with status 4;
//   2. A != A^T ends it with status 1; degrees are the row sums;
//   3. connected components by min-label propagation with pointer jumping, and their sizes m_c;
//   4. M = D - A + sum_c (1/m_c) 1_c 1_c^T in double, written over the counts slot by slot: symmetric positive definite,
//      block diagonal up to a permutation nobody applies (an isolated node is the block [1]);
//   5. M^-1 in place by a Gauss-Jordan sweep WITHOUT pivoting - every Schur complement of an SPD matrix is SPD, so every
//      pivot is positive; one that is not (or is not finite) ends the graph with status 3;
//   6. L+ = M^-1 - sum_c (1/m_c) 1_c 1_c^T and out[y] = ((L+[0,0] + L+[y,y]) - L+[0,y]) - L+[y,0] in double, stored as float.
// Two size classes of one kernel template: a wavefront per graph for n <= 32 (four graphs per 256-thread block, wave-level
// synchronisation only: the waves of a block run graphs of different sizes and never meet at a block barrier), and a block
// per graph up to n = 128 with dynamic LDS sized by the launch's largest graph.  The matrix has an ODD row stride (n | 1
// doubles), which keeps a column walk off one bank.  No global atomics; each graph's result comes from one workgroup in a
// fixed order.
#include "kpgnn_common.h"

#include <cmath>

namespace kpgnn {
namespace {

constexpr int kBlock = 256;
constexpr int kWaveCap = KPGNN_RD_WAVE_NODES;
constexpr int kMaxCap = KPGNN_RD_MAX_NODES;

struct RdParams {
    int G, n_ids, cap;
    const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* ei; int64_t E;
    const int32_t* ids;
    float* out; int32_t* status;
};

// LDS of one team sized for graphs of up to `cap` nodes: the matrix, the pivot row and column, three int arrays, two flags
__host__ __device__ constexpr size_t team_bytes(int cap) {
    return (size_t)cap * (cap | 1) * 8 + (size_t)cap * 2 * 8 + (size_t)cap * 3 * 4 + 16;
}

template <bool WAVE>
__global__ void __launch_bounds__(kBlock) rd_kernel(const RdParams p) {
    extern __shared__ double rd_lds[];
    constexpr int T = WAVE ? kWave : kBlock;
    const int team = WAVE ? (int)threadIdx.x / kWave : 0;
    const int tid = WAVE ? (int)threadIdx.x % kWave : (int)threadIdx.x;
    const int64_t slot = WAVE ? (int64_t)blockIdx.x * (kBlock / kWave) + team : (int64_t)blockIdx.x;
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
    const int n = (int)n64, s = n | 1;
    int64_t e0 = p.edge_ptr[g], e1 = p.edge_ptr[g + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > p.E ? p.E : e1;

    double* M = reinterpret_cast<double*>(reinterpret_cast<char*>(rd_lds) + (size_t)team * team_bytes(p.cap));
    int* Mi = reinterpret_cast<int*>(M);                      // the count of slot q lives in Mi[2 q] until step 4
    double* rowk = M + (size_t)p.cap * (p.cap | 1);
    double* colk = rowk + p.cap;
    int* deg = reinterpret_cast<int*>(colk + p.cap);
    int* label = deg + p.cap;
    int* msize = label + p.cap;
    int* flags = msize + p.cap;                                 // [0] bad input, [1] a label changed

    // the columns of a row go to CW consecutive lanes, CW the power of two >= n; the rows to the T / CW lane groups
    int cw = 8;
    while (cw < n) cw <<= 1;
    const int j = tid & (cw - 1), i0 = tid / cw, istep = T / cw;

    // 1. counts
    for (int q = tid; q < n * s; q += T) Mi[2 * q] = 0;
    if (tid < 2) flags[tid] = 0;
    team_sync<WAVE>();
    for (int64_t e = e0 + tid; e < e1; e += T) {
        const int64_t u = p.ei[e] - n0, v = p.ei[p.E + e] - n0;
        if (u < 0 || u >= n || v < 0 || v >= n) flags[0] = 1;
        else if (u != v) atomicAdd(&Mi[2 * ((int)u * s + (int)v)], 1);
    }
    team_sync<WAVE>();
    if (flags[0]) {
        if (tid == 0) p.status[g] = KPGNN_RD_RANGE;
        return;
    }
    team_sync<WAVE>();          // (everyone has read flags[0] before it is written again)

    // 2. symmetry, degrees
    for (int i = tid; i < n; i += T) {
        int d = 0, bad = 0;
        for (int c = 0; c < n; ++c) {
            const int a = Mi[2 * (i * s + c)];
            d += a;
            bad |= a != Mi[2 * (c * s + i)];
        }
        deg[i] = d;
        label[i] = i;
        if (bad) flags[0] = 1;
    }
    team_sync<WAVE>();
    if (flags[0]) {
        if (tid == 0) p.status[g] = KPGNN_RD_ASYMMETRIC;
        return;
    }

    // 3. components: labels only ever decrease towards the smallest node id of the component (a label read while its owner
    // lowers it is still a label of the same component), so the pass that changes nothing ends the loop
    for (;;) {
        team_sync<WAVE>();
        if (tid == 0) flags[1] = 0;
        team_sync<WAVE>();
        for (int i = tid; i < n; i += T) {
            const int mine = label[i];
            int l = mine;
            for (int c = 0; c < n; ++c)
                if (Mi[2 * (i * s + c)] > 0) { const int lc = label[c]; l = lc < l ? lc : l; }
            const int ll = label[l];
            l = ll < l ? ll : l;
            if (l < mine) { label[i] = l; flags[1] = 1; }
        }
        team_sync<WAVE>();
        if (!flags[1]) break;
    }
    for (int i = tid; i < n; i += T) {
        const int mine = label[i];
        int m = 0;
        for (int c = 0; c < n; ++c) m += label[c] == mine;
        msize[i] = m;
    }
    team_sync<WAVE>();

    // 4. M over the counts: every thread converts the slots it reads
    for (int i = i0; i < n; i += istep)
        if (j < n) {
            const int q = i * s + j;
            const int a = Mi[2 * q];
            const double proj = label[i] == label[j] ? 1.0 / (double)msize[i] : 0.0;
            M[q] = (i == j ? (double)deg[i] : -(double)a) + proj;
        }
    team_sync<WAVE>();

    // 5. Gauss-Jordan in place, no pivoting
    for (int k = 0; k < n; ++k) {
        const double piv = M[k * s + k];
        if (!(piv > 0.0) || !(piv < INFINITY)) {
            if (tid == 0) p.status[g] = KPGNN_RD_PIVOT;
            return;
        }
        for (int c = tid; c < n; c += T) {
            rowk[c] = M[k * s + c] / piv;
            colk[c] = M[c * s + k];
        }
        team_sync<WAVE>();
        if (j < n) {
            const double r = rowk[j];
            for (int i = i0; i < n; i += istep) {
                const int q = i * s + j;
                double v;
                if (i == k) v = j == k ? 1.0 / piv : r;
                else if (j == k) v = -colk[i] / piv;
                else v = fma(-colk[i], r, M[q]);
                M[q] = v;
            }
        }
        team_sync<WAVE>();
    }

    // 6. L+ and the feature
    const int lab0 = label[0];
    const double j0 = 1.0 / (double)msize[0];
    const double l00 = M[0] - j0;
    for (int y = tid; y < n; y += T) {
        const double same = label[y] == lab0 ? j0 : 0.0;
        const double lyy = M[y * s + y] - 1.0 / (double)msize[y];
        const double l0y = M[y] - same, ly0 = M[y * s] - same;
        p.out[n0 + y] = (float)(((l00 + lyy) - l0y) - ly0);
    }
    if (tid == 0) p.status[g] = KPGNN_RD_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_resistance_distance(const kpgnn_rd_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_resistance_distance";
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->G >= 0 && d->n_ids >= 0 && d->E >= 0, "%s: bad G=%d n_ids=%d E=%lld", who, d->G, d->n_ids, (long long)d->E);
    if (d->G == 0 || d->n_ids == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->node_ptr && d->edge_ptr && d->graph_ids && d->out && d->status, "%s: NULL node_ptr/edge_ptr/graph_ids/out/status", who);
    KPGNN_REQUIRE(d->E == 0 || d->edge_index, "%s: NULL edge_index", who);
    KPGNN_REQUIRE(d->max_nodes >= 1, "%s: bad max_nodes=%d", who, d->max_nodes);
    if (d->max_nodes > kMaxCap) return fail(KPGNN_ELIMIT, "%s: max_nodes=%d is beyond the cap of %d nodes per graph", who, d->max_nodes, kMaxCap);
    RdParams p = {};
    p.G = d->G; p.n_ids = d->n_ids; p.node_ptr = d->node_ptr; p.edge_ptr = d->edge_ptr; p.ei = d->edge_index; p.E = d->E;
    p.ids = d->graph_ids; p.out = d->out; p.status = d->status;
    hipStream_t s = (hipStream_t)stream;
    if (d->max_nodes <= kWaveCap) {
        p.cap = kWaveCap;
        constexpr int per = kBlock / kWave;
        const size_t lds = per * team_bytes(kWaveCap);
        hipLaunchKernelGGL(rd_kernel<true>, dim3((unsigned)((d->n_ids + per - 1) / per)), dim3(kBlock), lds, s, p);
        KPGNN_LAUNCH_CHECK("rd_kernel<wave>");
    } else {
        p.cap = d->max_nodes;
        const size_t lds = team_bytes(p.cap);
        KPGNN_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&rd_kernel<false>), lds));
        hipLaunchKernelGGL(rd_kernel<false>, dim3((unsigned)d->n_ids), dim3(kBlock), lds, s, p);
        KPGNN_LAUNCH_CHECK("rd_kernel<block>");
    }
    return KPGNN_OK;
}
