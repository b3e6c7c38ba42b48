// The five labels of the synthetic substructure-counting dataset, batched over graphs (gfx950).  Contract: include/kpgnn.h,
// kpgnn_count_labels.
//
// The reference (datasets/GraphCountDataset.py process) labels one graph at a time on the host with dense float64 products
// A A, A^2 A, A^3 A and a Python loop over the degrees.  Here the adjacency is a bitset of 64-bit words, (A^2)_ij is
// c_ij = popcount(row_i & row_j), and with d_i the degree and T_i = sum_{j in N(i)} c_ij = (A^3)_ii the reference's expressions
// reduce, for a symmetric graph without self loops, to
//   tri    = (sum_i T_i) / 6                     tailed = sum_i (T_i / 2) (d_i - 2)          star = sum_i d_i (d_i-1) (d_i-2) / 6
//   cyc4   = (sum_ij c_ij^2 + sum_i d_i - 2 sum_i d_i^2) / 8      (all ordered pairs, c_ii = d_i included)
//   cus    = sum_k d_k^2 exp(-s_k),  s_k = sum_{j in N(k)} d_j
// The first four are int64 sums, exact in any order (below 2^53 at 2048 nodes), converted to double once.  cus is summed by
// ONE lane in ascending k from LDS, one exp and one product per node; floating-point contraction is off in this file.  So
// the bits of a graph do not depend on the team's width, the edge order, duplicated edges, graph_ids or the other graphs.
// Three size classes:
//   n <= 32    a wavefront per graph, four graphs per 256-thread block, wave-level synchronisation only; rows are one word in
//              LDS, set by LDS atomic OR; the two halves of the wave split the targets j of row i = lane % 32
//   n <= 64    a 256-thread block per graph, the same one-word rows; the four waves split the targets j of row i = tid % 64
//   n <= 2048  a 1024-thread block per graph.  The bitset (up to 512 KiB) lives in the graph's slab of a global workspace,
//              word w of row j at slab[w * n + j] so that the lanes of a wave, which take consecutive targets j, read
//              consecutive words.  The block zeroes the slab, sets the bits with 64-bit integer atomic OR (the only global
//              atomic here) and fences before it reads them.  A wavefront owns FOUR source rows at a time, staged in LDS
//              (wave-uniform reads), so a target word is loaded once for four rows.  1024 threads: the graphs of this class
//              are few per launch and a graph costs n^2 ceil(n/64) word operations - 1.3e8 at 2048 nodes - so a graph gets a
//              whole CU's worth of lanes; the block's LDS (about 41 KiB) still lets two blocks share a CU.
// A directed list (status 1), a self loop (2), n above the launch's cap (3) are left to the host route; an endpoint outside
// [0, n) is status 4.  Every range is checked before it is used as an index.  No float atomics; all stores are plain.
#include "kpgnn_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace kpgnn {
namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int kBlock = 256;
constexpr int kLargeBlock = 1024;
constexpr int kLargeWaves = kLargeBlock / kWave;
constexpr int kWaveCap = KPGNN_CL_WAVE_NODES;
constexpr int kWordCap = KPGNN_CL_WORD_NODES;
constexpr int kMaxCap = KPGNN_CL_MAX_NODES;
constexpr int kMaxWords = kMaxCap / 64;
constexpr int kRowsPerPass = 4;           // source rows a wavefront of the large class holds at once

struct ClParams {
    int G, n_ids, cap;
    const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* ei; int64_t E;
    const int32_t* ids;
    double* out; int32_t* status;
    u64* ws; int64_t slab_words;
};

// the integer sums of a graph (or one node's, or one wavefront's, share of them)
struct Sums {
    i64 T, tail, star, sq, d, d2;
};

__device__ __forceinline__ Sums node_sums(i64 T, i64 sq, i64 d) {
    return Sums{T, (T / 2) * (d - 2), d * (d - 1) * (d - 2) / 6, sq, d, d * d};
}
__device__ __forceinline__ void add(Sums& a, const Sums& b) {
    a.T += b.T; a.tail += b.tail; a.star += b.star; a.sq += b.sq; a.d += b.d; a.d2 += b.d2;
}
__device__ __forceinline__ i64 wave_sum(i64 v) {      // integer: exact in any order
#pragma unroll
    for (int o = kWave >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ double cus_term(i64 d, i64 s) { return (double)(d * d) * exp(-(double)s); }

// one lane: the serial cus sum over term[0 .. n) and the row of graph g
__device__ __forceinline__ void finish(const ClParams& p, int g, int n, const Sums& t, const double* term) {
    double cus = 0.0;
    for (int k = 0; k < n; ++k) cus += term[k];
    double* o = p.out + (int64_t)g * 5;
    o[0] = (double)(t.T / 6);
    o[1] = (double)t.tail;
    o[2] = (double)t.star;
    o[3] = (double)((t.sq + t.d - 2 * t.d2) / 8);
    o[4] = cus;
    p.status[g] = KPGNN_CL_OK;
}

// Graph `slot` of the launch: false when there is nothing more to do for it (its status, if any, is written).
__device__ __forceinline__ bool open_graph(const ClParams& p, int64_t slot, int tid, int cap, int& g, int& n, int64_t& e0, int64_t& e1) {
    if (slot >= p.n_ids) return false;
    g = p.ids[slot];
    if (g < 0 || g >= p.G) return false;
    const int64_t n64 = p.node_ptr[g + 1] - p.node_ptr[g];
    if (n64 <= 0) {
        if (tid == 0) {
            if (n64 == 0) for (int c = 0; c < 5; ++c) p.out[(int64_t)g * 5 + c] = 0.0;
            p.status[g] = n64 == 0 ? KPGNN_CL_OK : KPGNN_CL_ENDPOINT;
        }
        return false;
    }
    if (n64 > p.cap || n64 > cap) {
        if (tid == 0) p.status[g] = KPGNN_CL_TOO_LARGE;
        return false;
    }
    n = (int)n64;
    e0 = p.edge_ptr[g];
    e1 = p.edge_ptr[g + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > p.E ? p.E : e1;
    return true;
}

__device__ __forceinline__ int status_of(const int* flags) {
    return flags[0] ? KPGNN_CL_ENDPOINT : flags[1] ? KPGNN_CL_SELF_LOOP : flags[2] ? KPGNN_CL_ASYMMETRIC : KPGNN_CL_OK;
}

// ---------------------------------------------------------------------------------------------- n <= 64: one-word rows in LDS
template <int CAP, int NQ>
struct WordTeam {
    u64 rows[CAP];
    i64 psq[NQ][CAP], pT[NQ][CAP];      // the share of target group q in row i's sum_j c_ij^2 and T_i
    double term[CAP];
    int flags[4];                       // [0] endpoint, [1] self loop, [2] asymmetric
};

template <bool WAVE>
__global__ void __launch_bounds__(kBlock) cl_word_kernel(const ClParams p) {
    constexpr int CAP = WAVE ? kWaveCap : kWordCap;
    constexpr int T = WAVE ? kWave : kBlock;
    constexpr int NQ = T / CAP;             // groups of lanes that split the targets of a row: 2 (wave), 4 (block)
    constexpr int JN = CAP / NQ;            // targets per group: 16
    __shared__ WordTeam<CAP, NQ> teams[WAVE ? kBlock / kWave : 1];
    const int team = WAVE ? (int)threadIdx.x / kWave : 0;
    const int tid = WAVE ? (int)threadIdx.x % kWave : (int)threadIdx.x;
    const int64_t slot = WAVE ? (int64_t)blockIdx.x * (kBlock / kWave) + team : (int64_t)blockIdx.x;
    int g, n;
    int64_t e0, e1;
    if (!open_graph(p, slot, tid, CAP, g, n, e0, e1)) return;       // (uniform over the team)
    WordTeam<CAP, NQ>& L = teams[team];

    // the rows, the checks
    if (tid < n) L.rows[tid] = 0ull;
    if (tid < 4) L.flags[tid] = 0;
    team_sync<WAVE>();
    for (int64_t e = e0 + tid; e < e1; e += T) {
        const int64_t u = p.ei[e], v = p.ei[p.E + e];
        if (u < 0 || u >= n || v < 0 || v >= n) L.flags[0] = 1;
        else if (u == v) L.flags[1] = 1;
        else atomicOr(&L.rows[(int)u], 1ull << (int)v);
    }
    team_sync<WAVE>();
    for (int64_t e = e0 + tid; e < e1; e += T) {
        const int64_t u = p.ei[e], v = p.ei[p.E + e];
        if (u < 0 || u >= n || v < 0 || v >= n || u == v) continue;
        if (!((L.rows[(int)v] >> (int)u) & 1ull)) L.flags[2] = 1;
    }
    team_sync<WAVE>();
    {
        const int st = status_of(L.flags);
        if (st != KPGNN_CL_OK) {
            if (tid == 0) p.status[g] = st;
            return;
        }
    }

    // lane group q takes the targets [q JN, (q + 1) JN) of row i
    const int i = tid % CAP, q = tid / CAP;
    if (i < n) {
        const u64 ri = L.rows[i];
        const int j1 = (q + 1) * JN < n ? (q + 1) * JN : n;
        i64 sq = 0, Ti = 0;
        for (int j = q * JN; j < j1; ++j) {
            const i64 c = __builtin_popcountll(ri & L.rows[j]);
            sq += c * c;
            if ((ri >> j) & 1ull) Ti += c;
        }
        L.psq[q][i] = sq;
        L.pT[q][i] = Ti;
    }
    team_sync<WAVE>();
    if (tid >= kWave) return;               // n <= 64: the team's first wavefront holds every node; no barrier below
    Sums mine = {0, 0, 0, 0, 0, 0};
    if (tid < n) {
        i64 sq = 0, Ti = 0, s = 0;
#pragma unroll
        for (int k = 0; k < NQ; ++k) { sq += L.psq[k][tid]; Ti += L.pT[k][tid]; }
        const u64 r = L.rows[tid];
        for (u64 f = r; f; f &= f - 1ull) s += __builtin_popcountll(L.rows[__builtin_ctzll(f)]);
        const i64 d = __builtin_popcountll(r);
        L.term[tid] = cus_term(d, s);
        mine = node_sums(Ti, sq, d);
    }
    const Sums tot = {wave_sum(mine.T), wave_sum(mine.tail), wave_sum(mine.star), wave_sum(mine.sq), wave_sum(mine.d), wave_sum(mine.d2)};
    team_sync<true>();                      // term[] of the other lanes
    if (tid == 0) finish(p, g, n, tot, L.term);
}

// ---------------------------------------------------------------------------------------------- 65 <= n <= 2048: rows in a slab
__global__ void __launch_bounds__(kLargeBlock) cl_large_kernel(const ClParams p) {
    __shared__ int deg[kMaxCap];
    __shared__ double term[kMaxCap];
    __shared__ u64 rowbuf[kLargeWaves][kRowsPerPass][kMaxWords];
    __shared__ Sums wpart[kLargeWaves];
    __shared__ int flags[4];
    const int tid = (int)threadIdx.x, wv = tid / kWave, lane = tid % kWave;
    int g, n;
    int64_t e0, e1;
    if (!open_graph(p, (int64_t)blockIdx.x, tid, kMaxCap, g, n, e0, e1)) return;
    const int W = (n + 63) >> 6;            // n W <= cap ceil(cap / 64) = slab_words: the host checked the workspace for that
    u64* S = p.ws + (int64_t)blockIdx.x * p.slab_words;

    for (int t = tid; t < n * W; t += kLargeBlock) S[t] = 0ull;
    if (tid < 4) flags[tid] = 0;
    __threadfence();                        // the zeroes reach L2, where the atomics work, before any OR
    __syncthreads();
    for (int64_t e = e0 + tid; e < e1; e += kLargeBlock) {
        const int64_t u = p.ei[e], v = p.ei[p.E + e];
        if (u < 0 || u >= n || v < 0 || v >= n) flags[0] = 1;
        else if (u == v) flags[1] = 1;
        else atomicOr(&S[(int)(v >> 6) * n + (int)u], 1ull << (int)(v & 63));
    }
    __threadfence();                        // this wavefront's ORs are done in L2 ...
    __syncthreads();
    __threadfence();                        // ... and, all being done, no line of the zeroed slab stays in this CU's L1
    for (int64_t e = e0 + tid; e < e1; e += kLargeBlock) {
        const int64_t u = p.ei[e], v = p.ei[p.E + e];
        if (u < 0 || u >= n || v < 0 || v >= n || u == v) continue;
        if (!((S[(int)(u >> 6) * n + (int)v] >> (int)(u & 63)) & 1ull)) flags[2] = 1;
    }
    for (int j = tid; j < n; j += kLargeBlock) {
        int d = 0;
        for (int w = 0; w < W; ++w) d += __builtin_popcountll(S[w * n + j]);
        deg[j] = d;
    }
    __syncthreads();
    {
        const int st = status_of(flags);
        if (st != KPGNN_CL_OK) {
            if (tid == 0) p.status[g] = st;
            return;
        }
    }

    // wavefront wv takes the source rows [4 (wv + 16 m), + 4): their words in LDS, the lanes over the targets j
    Sums acc = {0, 0, 0, 0, 0, 0};
    for (int i0 = wv * kRowsPerPass; i0 < n; i0 += kLargeWaves * kRowsPerPass) {
        for (int t = lane; t < kRowsPerPass * W; t += kWave) {
            const int r = t / W, w = t - r * W, i = i0 + r;
            rowbuf[wv][r][w] = i < n ? S[w * n + i] : 0ull;
        }
        team_sync<true>();
        // a lane's share, over its <= 32 targets: sum c^2 <= 32 * 2047^2 < 2^31, T and s <= 32 * 2047; widened at the wave sum
        uint32_t sq[kRowsPerPass] = {}, Ti[kRowsPerPass] = {}, s[kRowsPerPass] = {};
        for (int j = lane; j < n; j += kWave) {
            int c[kRowsPerPass] = {};
            for (int w = 0; w < W; ++w) {
                const u64 x = S[w * n + j];
#pragma unroll
                for (int r = 0; r < kRowsPerPass; ++r) c[r] += __builtin_popcountll(x & rowbuf[wv][r][w]);
            }
            const uint32_t dj = (uint32_t)deg[j];
#pragma unroll
            for (int r = 0; r < kRowsPerPass; ++r) {
                sq[r] += (uint32_t)(c[r] * c[r]);
                if ((rowbuf[wv][r][j >> 6] >> (j & 63)) & 1ull) { Ti[r] += c[r]; s[r] += dj; }
            }
        }
#pragma unroll
        for (int r = 0; r < kRowsPerPass; ++r) {
            const i64 a = wave_sum((i64)sq[r]), b = wave_sum((i64)Ti[r]), cs = wave_sum((i64)s[r]);
            const int i = i0 + r;
            if (lane == 0 && i < n) {
                const i64 d = deg[i];
                term[i] = cus_term(d, cs);
                add(acc, node_sums(b, a, d));
            }
        }
        team_sync<true>();                  // rowbuf is rewritten by the next pass
    }
    if (lane == 0) wpart[wv] = acc;
    __syncthreads();
    if (tid == 0) {
        Sums tot = wpart[0];
        for (int k = 1; k < kLargeWaves; ++k) add(tot, wpart[k]);
        finish(p, g, n, tot, term);
    }
}

inline size_t slab_words(int max_nodes) {
    return max_nodes <= kWordCap ? 0 : (size_t)max_nodes * (size_t)((max_nodes + 63) / 64);
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" size_t kpgnn_count_labels_workspace_bytes(int max_nodes) { return slab_words(max_nodes) * sizeof(u64); }

extern "C" int kpgnn_count_labels(const kpgnn_count_labels_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_count_labels";
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->G >= 0 && d->n_ids >= 0 && d->E >= 0, "%s: bad G=%d n_ids=%d E=%lld", who, d->G, d->n_ids, (long long)d->E);
    if (d->G == 0 || d->n_ids == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->max_nodes >= 1, "%s: bad max_nodes=%d", who, d->max_nodes);
    if (d->max_nodes > kMaxCap) return fail(KPGNN_ELIMIT, "%s: max_nodes=%d is beyond the cap of %d nodes per graph", who, d->max_nodes, kMaxCap);
    KPGNN_REQUIRE(d->node_ptr && d->edge_ptr && d->graph_ids, "%s: NULL node_ptr/edge_ptr/graph_ids", who);
    KPGNN_REQUIRE(d->out && d->status, "%s: NULL out/status", who);
    KPGNN_REQUIRE(d->E == 0 || d->edge_index, "%s: NULL edge_index", who);
    ClParams p = {};
    p.G = d->G; p.n_ids = d->n_ids; p.cap = d->max_nodes;
    p.node_ptr = d->node_ptr; p.edge_ptr = d->edge_ptr; p.ei = d->edge_index; p.E = d->E;
    p.ids = d->graph_ids; p.out = d->out; p.status = d->status;
    hipStream_t s = (hipStream_t)stream;
    if (d->max_nodes <= kWaveCap) {
        constexpr int per = kBlock / kWave;
        hipLaunchKernelGGL(cl_word_kernel<true>, dim3((unsigned)((d->n_ids + per - 1) / per)), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("cl_word_kernel<wave>");
    } else if (d->max_nodes <= kWordCap) {
        hipLaunchKernelGGL(cl_word_kernel<false>, dim3((unsigned)d->n_ids), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("cl_word_kernel<block>");
    } else {
        const size_t words = slab_words(d->max_nodes);
        KPGNN_REQUIRE(d->workspace != nullptr, "%s: NULL workspace for max_nodes=%d", who, d->max_nodes);
        KPGNN_REQUIRE(((uintptr_t)d->workspace % sizeof(u64)) == 0, "%s: workspace is not 8-byte aligned", who);
        KPGNN_REQUIRE(d->workspace_bytes / (words * sizeof(u64)) >= (size_t)d->n_ids, "%s: workspace_bytes=%zu is below %d slabs of %zu bytes", who,
                      d->workspace_bytes, d->n_ids, words * sizeof(u64));
        p.ws = (u64*)d->workspace;
        p.slab_words = (int64_t)words;
        hipLaunchKernelGGL(cl_large_kernel, dim3((unsigned)d->n_ids), dim3(kLargeBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("cl_large_kernel");
    }
    return KPGNN_OK;
}
