// The six labels of the synthetic graph- and node-property dataset, batched over graphs (gfx950).  Contract: include/kpgnn.h,
// kpgnn_graph_labels (graphs of up to 64 nodes) and kpgnn_graph_labels_large (up to 128).
//
// The reference (datasets/GraphPropertyDataset.py genereate_dataset, datasets/graph_algorithms.py) labels one graph at a time
// on the host: a triple Python loop for the all-pairs shortest paths, run three times, np.linalg.eig, and repeated float64
// squaring.  Here one team (a wavefront, or a block) owns one graph, whose adjacency is n rows of W 64-bit words in LDS (bit
// j & 63 of word j >> 6 of row i: the edge i - j; bit 64 is bit 0 of the second word; duplicates collapse under the OR):
//   1. the rows by LDS atomic OR on the word that holds the bit; an endpoint outside [0, n) ends the graph with status 3, a self
//      loop with 4, a source outside [0, n) with 5 - every range is checked before anything is indexed with it - and A != A^T
//      with status 1;
//   2. all-source BFS, lane i the source i: the next frontier is the OR of the rows of the frontier's set bits without the
//      nodes seen.  Every node enters a frontier once: O(n) row reads per lane.  eccentricity[i] is the last level that was
//      not empty, sssp[i] the level at which lane i met the source node (the graph is symmetric), 0 when it never did;
//   3. the reference's is_connected: m = 1 + ceil(log2 n) boolean squarings B <- B B of the word matrix, then "every row full",
//      the full row being ~0 in a word the graph fills, (1 << (n & 63)) - 1 in its last, partial word and 0 in a word it does
//      not reach - no shift by 64.  For 65 <= n <= 128, m = 8 and every entry of A^(2^7) is at most 127^128 < 2^895, so the
//      reference's last float64 squaring multiplies no inf by 0: it makes no nan, rounds no positive integer to zero, and
//      min > 0 holds iff the eighth boolean squaring has no zero.  At n = 129, m = 9 and stage 8 can hold inf next to zeros:
//      the cap of 128;
//   4. laplacian[i] = deg(i) F[i] - sum_{j in adj(i)} F[j], in double, ascending j (the first word, then the second), rounded
//      to float once;
//   5. the spectral radius, the largest eigenvalue of the non-negative symmetric matrix: Householder tridiagonalisation of
//      the n x n double matrix in LDS, then Sturm-count multisection for the top eigenvalue - the 64 lanes of the team's first
//      wavefront evaluate 64 probe points of the bracket per round, which shrinks it 65-fold; 11 rounds from a bracket of
//      width <= 129 end below 1e-17.  An edgeless graph answers exactly 0.
// Every sum that crosses lanes is taken by each lane on its own, serially in index order, from LDS; every matrix element is
// updated by one expression whichever thread holds it; floating-point contraction is off in this file.  So the bits of a
// graph do not depend on the team's width, on the row's, on the edge order, on the other graphs of the launch or on graph_ids.
// ONE kernel template over <WAVE, W>, three instantiations: a wavefront per graph for n <= 32 (W = 1; four graphs per
// 256-thread block, wave-level synchronisation only) and a block per graph up to n = 64 (W = 1), both in static LDS, as in
// resistance.hip; and a block per graph up to n = 128 (W = 2), whose LDS is dynamic, sized for the launch's max_nodes: 143,888
// bytes at 128, one block per CU.  256 threads there too: per column the three serial sums (3 (n - k) dependent adds in every
// lane) outweigh the rank-2 update ((n - k)^2 / 256 elements a thread), so a wider block would shorten the smaller term only.
// The matrix has an ODD row stride (n | 1).  No global atomics, no float atomics.
#include "kpgnn_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace kpgnn {
namespace {

constexpr int kBlock = 256;
constexpr int kWaveCap = KPGNN_GL_WAVE_NODES;
constexpr int kMaxCap = KPGNN_GL_MAX_NODES;
constexpr int kLargeCap = KPGNN_GL_LARGE_MAX_NODES;
constexpr int kRounds = 11;
constexpr double kNegligible = 1e-200;
typedef unsigned long long u64;

struct GlParams {
    int G, n_ids, cap;
    const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* ei; int64_t E;
    const int32_t* ids;
    const double* feat; const int32_t* source;
    float* node_out; float* graph_out; int32_t* status;
};

// LDS of one team sized for graphs of up to `cap` nodes: M [cap][cap | 1], v, p, d, e2, F [cap] doubles; rows [cap][W],
// sq [2][cap][W] words; ecc [cap], flags [4] ints.  Every offset is a multiple of 8.
struct Team {
    double *M, *v, *p, *d, *e2, *F;
    u64 *rows, *sq[2];
    int *ecc;
    int* flags;                 // [0] endpoint, [1] self loop, [2] asymmetric, [3] a row of the squared matrix is not full
};
template <int W>
__host__ __device__ constexpr size_t lds_bytes(int cap) {
    return ((size_t)cap * (cap | 1) + 5 * (size_t)cap) * 8 + 3 * W * (size_t)cap * 8 + (size_t)cap * 4 + 16;
}
static_assert(lds_bytes<2>(kLargeCap) <= 160 * 1024, "the double matrix of the largest graph must fit the LDS of a CU");

template <int W>
__device__ __forceinline__ Team carve(double* base, int cap) {
    Team L;
    L.M = base;
    L.v = L.M + (size_t)cap * (cap | 1);
    L.p = L.v + cap;
    L.d = L.p + cap;
    L.e2 = L.d + cap;
    L.F = L.e2 + cap;
    L.rows = reinterpret_cast<u64*>(L.F + cap);
    L.sq[0] = L.rows + W * cap;
    L.sq[1] = L.sq[0] + W * cap;
    L.ecc = reinterpret_cast<int*>(L.sq[1] + W * cap);
    L.flags = L.ecc + cap;
    return L;
}

// An adjacency row in registers: node j is bit j & 63 of word j >> 6.  Only what the kernel below uses.
template <int W>
struct Row {
    u64 w[W];
    static __device__ __forceinline__ Row load(const u64* q) {
        Row r;
#pragma unroll
        for (int k = 0; k < W; ++k) r.w[k] = q[k];
        return r;
    }
    __device__ __forceinline__ void store(u64* q) const {
#pragma unroll
        for (int k = 0; k < W; ++k) q[k] = w[k];
    }
    static __device__ __forceinline__ Row single(int j) {           // the node j alone
        Row r;
#pragma unroll
        for (int k = 0; k < W; ++k) r.w[k] = (W == 1 || (j >> 6) == k) ? 1ull << (j & 63) : 0ull;
        return r;
    }
    // the nodes [0, n): a word the graph fills is ~0 (no shift by 64), a word it does not reach is 0
    static __device__ __forceinline__ Row full(int n) {
        Row r;
#pragma unroll
        for (int k = 0; k < W; ++k) r.w[k] = n >= 64 * (k + 1) ? ~0ull : n > 64 * k ? (1ull << (n - 64 * k)) - 1ull : 0ull;
        return r;
    }
    __device__ __forceinline__ bool test(int j) const {             // a select, not an indexed register array
        u64 x = w[0];
#pragma unroll
        for (int k = 1; k < W; ++k) x = (j >> 6) == k ? w[k] : x;
        return (x >> (j & 63)) & 1ull;
    }
    __device__ __forceinline__ void operator|=(const Row& o) {
#pragma unroll
        for (int k = 0; k < W; ++k) w[k] |= o.w[k];
    }
    __device__ __forceinline__ void clear(const Row& o) {           // &= ~o
#pragma unroll
        for (int k = 0; k < W; ++k) w[k] &= ~o.w[k];
    }
    __device__ __forceinline__ bool any() const {
        u64 x = 0ull;
#pragma unroll
        for (int k = 0; k < W; ++k) x |= w[k];
        return x != 0ull;
    }
    __device__ __forceinline__ int count() const {
        int c = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) c += __builtin_popcountll(w[k]);
        return c;
    }
    __device__ __forceinline__ bool operator==(const Row& o) const {
        bool eq = true;
#pragma unroll
        for (int k = 0; k < W; ++k) eq &= w[k] == o.w[k];
        return eq;
    }
    template <typename F>
    __device__ __forceinline__ void each(F&& f) const {             // f(j) for every node j of the row, ASCENDING
#pragma unroll
        for (int k = 0; k < W; ++k)
            for (u64 m = w[k]; m; m &= m - 1ull) f(64 * k + __builtin_ctzll(m));
    }
};
// the word of LDS row i that holds node j, and j's bit in it
template <int W> __device__ __forceinline__ u64* row_word(u64* rows, int i, int j) { return rows + W * i + (W == 1 ? 0 : j >> 6); }
template <int W> __device__ __forceinline__ u64 row_bit(u64* rows, int i, int j) { return (*row_word<W>(rows, i, j) >> (j & 63)) & 1ull; }

template <bool WAVE, int W>
__global__ void __launch_bounds__(kBlock) gl_kernel(const GlParams p) {
    static_assert(W == 1 || (W == 2 && !WAVE), "one word per row in a wavefront or a block, two in a block");
    constexpr int CAP = W == 2 ? kLargeCap : WAVE ? kWaveCap : kMaxCap;
    constexpr int T = WAVE ? kWave : kBlock;
    const int team = WAVE ? (int)threadIdx.x / kWave : 0;
    const int tid = WAVE ? (int)threadIdx.x % kWave : (int)threadIdx.x;
    const int64_t slot = WAVE ? (int64_t)blockIdx.x * (kBlock / kWave) + team : (int64_t)blockIdx.x;
    if (slot >= p.n_ids) return;
    const int g = p.ids[slot];
    if (g < 0 || g >= p.G) return;
    const int64_t n0 = p.node_ptr[g], n64 = p.node_ptr[g + 1] - n0;
    if (n64 <= 0) {
        if (tid == 0) {
            if (n64 == 0) p.graph_out[(int64_t)g * 3] = p.graph_out[(int64_t)g * 3 + 1] = p.graph_out[(int64_t)g * 3 + 2] = 0.f;
            p.status[g] = n64 == 0 ? KPGNN_GL_OK : KPGNN_GL_ENDPOINT;
        }
        return;
    }
    if (n64 > p.cap || n64 > CAP) {
        if (tid == 0) p.status[g] = KPGNN_GL_TOO_LARGE;
        return;
    }
    const int n = (int)n64, s = n | 1;
    int64_t e0 = p.edge_ptr[g], e1 = p.edge_ptr[g + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > p.E ? p.E : e1;
    Team L;
    if constexpr (W == 1) {     // static, sized for the class
        constexpr size_t kTeamDoubles = lds_bytes<W>(CAP) / 8;
        __shared__ double teams[(WAVE ? kBlock / kWave : 1) * kTeamDoubles];
        L = carve<W>(teams + team * kTeamDoubles, CAP);
    } else {                    // dynamic, carved by the launch's cap (n <= cap), so a graph's bits cannot depend on it: only addresses move
        extern __shared__ __attribute__((aligned(16))) double gl_lds[];
        L = carve<W>(gl_lds, p.cap);
    }

    // 1. the rows, the checks
    if (tid < n) { Row<W>{}.store(L.rows + W * tid); L.F[tid] = p.feat[n0 + tid]; }
    if (tid < 4) L.flags[tid] = 0;
    team_sync<WAVE>();
    for (int64_t e = e0 + tid; e < e1; e += T) {
        const int64_t u = p.ei[e], v = p.ei[p.E + e];
        if (u < 0 || u >= n || v < 0 || v >= n) L.flags[0] = 1;
        else if (u == v) L.flags[1] = 1;
        else atomicOr(row_word<W>(L.rows, (int)u, (int)v), 1ull << ((int)v & 63));
    }
    team_sync<WAVE>();
    Row<W> mine = {};
    if (tid < n) {
        mine = Row<W>::load(L.rows + W * tid);
        bool bad = false;
        mine.each([&](int j) { bad |= !row_bit<W>(L.rows, j, tid); });
        if (bad) L.flags[2] = 1;
    }
    team_sync<WAVE>();
    const int src = p.source[g];
    {
        const int st = L.flags[0] ? KPGNN_GL_ENDPOINT : L.flags[1] ? KPGNN_GL_SELF_LOOP
                     : (src < 0 || src >= n) ? KPGNN_GL_SOURCE : L.flags[2] ? KPGNN_GL_ASYMMETRIC : KPGNN_GL_OK;
        if (st != KPGNN_GL_OK) {
            if (tid == 0) p.status[g] = st;
            return;
        }
    }

    // 2. all-source BFS; 4. the laplacian column
    if (tid < n) {
        Row<W> seen = Row<W>::single(tid), fr = seen;
        int level = 0, sd = 0;
        for (;;) {
            Row<W> nxt = {};
            fr.each([&](int j) { nxt |= Row<W>::load(L.rows + W * j); });
            nxt.clear(seen);
            if (!nxt.any()) break;
            ++level;
            seen |= nxt;
            if (nxt.test(src)) sd = level;
            fr = nxt;
        }
        L.ecc[tid] = level;
        double acc = (double)mine.count() * L.F[tid];
        mine.each([&](int j) { acc -= L.F[j]; });
        float* o = p.node_out + (n0 + tid) * 3;
        o[0] = (float)sd;
        o[1] = (float)level;
        o[2] = (float)acc;
        mine.store(L.sq[0] + W * tid);
    }

    // 3. m boolean squarings
    int m = 1;
    while ((1 << (m - 1)) < n) ++m;                  // 1 + ceil(log2 n)
    u64* cur = L.sq[0];
    u64* nxt = L.sq[1];
    for (int r = 0; r < m; ++r) {
        team_sync<WAVE>();
        if (tid < n) {
            Row<W> acc = {};
            Row<W>::load(cur + W * tid).each([&](int j) { acc |= Row<W>::load(cur + W * j); });
            acc.store(nxt + W * tid);
        }
        u64* t = cur; cur = nxt; nxt = t;
    }
    if (tid < n && !(Row<W>::load(cur + W * tid) == Row<W>::full(n))) L.flags[3] = 1;

    // 5. the matrix, tridiagonalised in place: d the diagonal, e2 the squared off-diagonal
    int cw = 8;
    while (cw < n) cw <<= 1;
    const int j = tid & (cw - 1), i0 = tid / cw, istep = T / cw;
    for (int i = i0; i < n; i += istep)
        if (j < n) L.M[i * s + j] = (double)row_bit<W>(L.rows, i, j);
    team_sync<WAVE>();          // (also publishes ecc and flags[3])
    for (int k = 0; k + 2 < n; ++k) {
        const int k1 = k + 1;
        const double x1 = L.M[k1 * s + k];
        double rest = 0.0;
        for (int r = k1 + 1; r < n; ++r) { const double x = L.M[r * s + k]; rest += x * x; }
        if (tid == 0) L.d[k] = L.M[k * s + k];
        // the column is tridiagonal already, or as good as: entries below 1e-100 - rounding residue of a low-rank matrix, which
        // would overflow 1 / (v.v) - move an eigenvalue of a matrix of norm >= 1 by less than 1e-98 (uniform over the team)
        if (rest < kNegligible) {
            if (tid == 0) L.e2[k] = x1 * x1;
            continue;
        }
        const double sigma = rest + x1 * x1;
        const double alpha = x1 > 0.0 ? -sqrt(sigma) : sqrt(sigma);
        const double beta = 1.0 / (sigma - alpha * x1);               // 2 / v.v
        if (tid == 0) L.e2[k] = alpha * alpha;
        for (int r = k1 + tid; r < n; r += T) L.v[r] = L.M[r * s + k] - (r == k1 ? alpha : 0.0);
        team_sync<WAVE>();
        for (int r = k1 + tid; r < n; r += T) {
            double a = 0.0;
            for (int c = k1; c < n; ++c) a += L.M[r * s + c] * L.v[c];
            L.p[r] = beta * a;
        }
        team_sync<WAVE>();
        double pv = 0.0;
        for (int r = k1; r < n; ++r) pv += L.p[r] * L.v[r];
        const double kc = 0.5 * beta * pv;
        if (j >= k1 && j < n) {
            const double vj = L.v[j], wj = L.p[j] - kc * vj;
            for (int i = k1 + i0; i < n; i += istep) {
                const double vi = L.v[i], wi = L.p[i] - kc * vi;
                L.M[i * s + j] -= vi * wj + wi * vj;
            }
        }
        team_sync<WAVE>();
    }
    if (tid == 0) {
        if (n >= 2) {
            const double x = L.M[(n - 1) * s + (n - 2)];
            L.d[n - 2] = L.M[(n - 2) * s + (n - 2)];
            L.e2[n - 2] = x * x;
        }
        L.d[n - 1] = L.M[(n - 1) * s + (n - 1)];
    }
    team_sync<WAVE>();
    if (tid >= kWave) return;                         // the team's first wavefront goes on alone: no barrier below

    int maxdeg = 0, diam = 0;
    for (int i = 0; i < n; ++i) {
        const int dg = Row<W>::load(L.rows + W * i).count(), ec = L.ecc[i];
        maxdeg = dg > maxdeg ? dg : maxdeg;
        diam = ec > diam ? ec : diam;
    }
    double radius = 0.0;
    if (maxdeg > 0) {
        // the top eigenvalue lies in (0, maxdeg]; count(x) = #{eigenvalues < x} by the Sturm recurrence of the tridiagonal matrix
        double lo = 0.0, hi = (double)maxdeg + 1.0;
        for (int r = 0; r < kRounds; ++r) {
            const double step = (hi - lo) / 65.0;
            const double x = lo + step * (double)(tid + 1);
            double q = L.d[0] - x;
            int cnt = q < 0.0;
            for (int i = 1; i < n; ++i) {
                if (fabs(q) < 1e-300) q = -1e-300;
                q = (L.d[i] - x) - L.e2[i - 1] / q;
                cnt += q < 0.0;
            }
            const u64 below = __ballot(cnt < n);                        // probes with an eigenvalue at or above them
            const int jl = below ? 63 - __builtin_clzll(below) : -1;    // the last of them; the bracket is (x_jl, x_jl+1)
            const double nlo = jl < 0 ? lo : lo + step * (double)(jl + 1);
            const double nhi = jl >= 63 ? hi : lo + step * (double)(jl + 2);
            lo = nlo;
            hi = nhi;
        }
        radius = 0.5 * (lo + hi);
    }
    if (tid == 0) {
        float* o = p.graph_out + (int64_t)g * 3;
        o[0] = L.flags[3] ? 0.f : 1.f;
        o[1] = (float)diam;
        o[2] = (float)radius;
        p.status[g] = KPGNN_GL_OK;
    }
}

// Both entry points: the checks, the parameters, and the class - two words per row behind the entry whose limit is 128
// whatever max_nodes is, else by max_nodes.
int launch_labels(const char* who, int cap_limit, const kpgnn_graph_labels_desc* d, hipStream_t s) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->G >= 0 && d->n_ids >= 0 && d->E >= 0, "%s: bad G=%d n_ids=%d E=%lld", who, d->G, d->n_ids, (long long)d->E);
    if (d->G == 0 || d->n_ids == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->max_nodes >= 1, "%s: bad max_nodes=%d", who, d->max_nodes);
    if (d->max_nodes > cap_limit) return fail(KPGNN_ELIMIT, "%s: max_nodes=%d is beyond the cap of %d nodes per graph", who, d->max_nodes, cap_limit);
    KPGNN_REQUIRE(d->node_ptr && d->edge_ptr && d->graph_ids && d->features && d->source, "%s: NULL node_ptr/edge_ptr/graph_ids/features/source", who);
    KPGNN_REQUIRE(d->node_out && d->graph_out && d->status, "%s: NULL node_out/graph_out/status", who);
    KPGNN_REQUIRE(d->E == 0 || d->edge_index, "%s: NULL edge_index", who);
    GlParams p = {};
    p.G = d->G; p.n_ids = d->n_ids; p.cap = d->max_nodes;
    p.node_ptr = d->node_ptr; p.edge_ptr = d->edge_ptr; p.ei = d->edge_index; p.E = d->E;
    p.ids = d->graph_ids; p.feat = d->features; p.source = d->source;
    p.node_out = d->node_out; p.graph_out = d->graph_out; p.status = d->status;
    if (cap_limit > kMaxCap) {
        const size_t lds = lds_bytes<2>(p.cap);
        KPGNN_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&gl_kernel<false, 2>), lds));
        hipLaunchKernelGGL((gl_kernel<false, 2>), dim3((unsigned)d->n_ids), dim3(kBlock), lds, s, p);
        KPGNN_LAUNCH_CHECK("gl_large_kernel");
    } else if (d->max_nodes <= kWaveCap) {
        constexpr int per = kBlock / kWave;
        hipLaunchKernelGGL((gl_kernel<true, 1>), dim3((unsigned)((d->n_ids + per - 1) / per)), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("gl_kernel<wave>");
    } else {
        hipLaunchKernelGGL((gl_kernel<false, 1>), dim3((unsigned)d->n_ids), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("gl_kernel<block>");
    }
    return KPGNN_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_graph_labels(const kpgnn_graph_labels_desc* d, kpgnn_stream_t stream) {
    return launch_labels("kpgnn_graph_labels", kMaxCap, d, (hipStream_t)stream);
}
extern "C" int kpgnn_graph_labels_large(const kpgnn_graph_labels_desc* d, kpgnn_stream_t stream) {
    return launch_labels("kpgnn_graph_labels_large", kLargeCap, d, (hipStream_t)stream);
}
