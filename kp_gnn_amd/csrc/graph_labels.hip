// The six labels of the synthetic graph- and node-property dataset, batched over graphs (gfx950).  Contract: include/kpgnn.h,
// kpgnn_graph_labels.
//
// The reference (datasets/GraphPropertyDataset.py genereate_dataset, datasets/graph_algorithms.py) labels one graph at a time
// on the host: a triple Python loop for the all-pairs shortest paths, run three times, np.linalg.eig, and repeated float64
// squaring.  Here one team (a wavefront, or a block) owns one graph of up to 64 nodes, whose adjacency is n rows of ONE 64-bit
// word in LDS (bit j of row i: the edge i - j; duplicates collapse under the OR):
//   1. the rows by LDS atomic OR; an endpoint outside [0, n) ends the graph with status 3, a self loop with 4, a source outside
//      [0, n) with 5 - every range is checked before anything is indexed with it - and A != A^T with status 1;
//   2. all-source BFS, lane i the source i: the next frontier is the OR of the rows of the frontier's set bits without the
//      nodes seen.  Every node enters a frontier once: O(n) row reads per lane.  eccentricity[i] is the last level that was
//      not empty, sssp[i] the level at which lane i met the source node (the graph is symmetric), 0 when it never did;
//   3. the reference's is_connected: m = 1 + ceil(log2 n) boolean squarings B <- B B of the word matrix, then "every row full";
//   4. laplacian[i] = deg(i) F[i] - sum_{j in adj(i)} F[j], in double, ascending j, rounded to float once;
//   5. the spectral radius, the largest eigenvalue of the non-negative symmetric matrix: Householder tridiagonalisation of
//      the n x n double matrix in LDS, then Sturm-count multisection for the top eigenvalue - the 64 lanes of the team's first
//      wavefront evaluate 64 probe points of the bracket per round, which shrinks it 65-fold; 11 rounds from a bracket of
//      width <= 65 end below 1e-17.  An edgeless graph answers exactly 0.
// Every sum that crosses lanes is taken by each lane on its own, serially in index order, from LDS; every matrix element is
// updated by one expression whichever thread holds it; floating-point contraction is off in this file.  So the bits of a
// graph do not depend on the team's width, on the edge order, on the other graphs of the launch or on graph_ids.
// Two size classes of one kernel template, as in resistance.hip: a wavefront per graph for n <= 32 (four graphs per 256-thread
// block, wave-level synchronisation only), a block per graph up to n = 64.  The matrix has an ODD row stride.  No global
// atomics, no float atomics.
#include "kpgnn_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace kpgnn {
namespace {

constexpr int kBlock = 256;
constexpr int kWaveCap = KPGNN_GL_WAVE_NODES;
constexpr int kMaxCap = KPGNN_GL_MAX_NODES;
constexpr int kRounds = 11;
constexpr double kNegligible = 1e-200;

struct GlParams {
    int G, n_ids, cap;
    const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* ei; int64_t E;
    const int32_t* ids;
    const double* feat; const int32_t* source;
    float* node_out; float* graph_out; int32_t* status;
};

// LDS of one team sized for graphs of up to CAP nodes
template <int CAP>
struct Team {
    double M[CAP * (CAP | 1)];
    double v[CAP], p[CAP], d[CAP], e2[CAP], F[CAP];
    unsigned long long rows[CAP], sq[2][CAP];
    int ecc[CAP];
    int flags[4];               // [0] endpoint, [1] self loop, [2] asymmetric, [3] a row of the squared matrix is not full
};

template <bool WAVE>
__device__ __forceinline__ void team_sync() {
    if (WAVE) {     // one wavefront: LDS operations of a wave complete in order; keep the compiler from moving them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __syncthreads();
    }
}

template <bool WAVE>
__global__ void __launch_bounds__(kBlock) gl_kernel(const GlParams p) {
    constexpr int CAP = WAVE ? kWaveCap : kMaxCap;
    constexpr int T = WAVE ? kWave : kBlock;
    __shared__ Team<CAP> teams[WAVE ? kBlock / kWave : 1];
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
    Team<CAP>& L = teams[team];
    const unsigned long long full = n == 64 ? ~0ull : (1ull << n) - 1ull;

    // 1. the rows, the checks
    if (tid < n) { L.rows[tid] = 0ull; L.F[tid] = p.feat[n0 + tid]; }
    if (tid < 4) L.flags[tid] = 0;
    team_sync<WAVE>();
    for (int64_t e = e0 + tid; e < e1; e += T) {
        const int64_t u = p.ei[e], v = p.ei[p.E + e];
        if (u < 0 || u >= n || v < 0 || v >= n) L.flags[0] = 1;
        else if (u == v) L.flags[1] = 1;
        else atomicOr(&L.rows[(int)u], 1ull << (int)v);
    }
    team_sync<WAVE>();
    unsigned long long mine = 0ull;
    if (tid < n) {
        mine = L.rows[tid];
        bool bad = false;
        for (unsigned long long f = mine; f; f &= f - 1ull) bad |= !((L.rows[__builtin_ctzll(f)] >> tid) & 1ull);
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
        unsigned long long seen = 1ull << tid, fr = seen;
        int level = 0, sd = 0;
        for (;;) {
            unsigned long long nxt = 0ull;
            for (unsigned long long f = fr; f; f &= f - 1ull) nxt |= L.rows[__builtin_ctzll(f)];
            nxt &= ~seen;
            if (!nxt) break;
            ++level;
            seen |= nxt;
            if ((nxt >> src) & 1ull) sd = level;
            fr = nxt;
        }
        L.ecc[tid] = level;
        double acc = (double)__builtin_popcountll(mine) * L.F[tid];
        for (unsigned long long f = mine; f; f &= f - 1ull) acc -= L.F[__builtin_ctzll(f)];
        float* o = p.node_out + (n0 + tid) * 3;
        o[0] = (float)sd;
        o[1] = (float)level;
        o[2] = (float)acc;
        L.sq[0][tid] = mine;
    }

    // 3. m boolean squarings
    int m = 1;
    while ((1 << (m - 1)) < n) ++m;                  // 1 + ceil(log2 n)
    int cur = 0;
    for (int r = 0; r < m; ++r) {
        team_sync<WAVE>();
        if (tid < n) {
            unsigned long long acc = 0ull;
            for (unsigned long long f = L.sq[cur][tid]; f; f &= f - 1ull) acc |= L.sq[cur][__builtin_ctzll(f)];
            L.sq[cur ^ 1][tid] = acc;
        }
        cur ^= 1;
    }
    if (tid < n && L.sq[cur][tid] != full) L.flags[3] = 1;

    // 5. the matrix, tridiagonalised in place: d the diagonal, e2 the squared off-diagonal
    int cw = 8;
    while (cw < n) cw <<= 1;
    const int j = tid & (cw - 1), i0 = tid / cw, istep = T / cw;
    for (int i = i0; i < n; i += istep)
        if (j < n) L.M[i * s + j] = (double)((L.rows[i] >> j) & 1ull);
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
        const int dg = __builtin_popcountll(L.rows[i]), ec = L.ecc[i];
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
            const unsigned long long below = __ballot(cnt < n);       // probes with an eigenvalue at or above them
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

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_graph_labels(const kpgnn_graph_labels_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_graph_labels";
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->G >= 0 && d->n_ids >= 0 && d->E >= 0, "%s: bad G=%d n_ids=%d E=%lld", who, d->G, d->n_ids, (long long)d->E);
    if (d->G == 0 || d->n_ids == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->max_nodes >= 1, "%s: bad max_nodes=%d", who, d->max_nodes);
    if (d->max_nodes > kMaxCap) return fail(KPGNN_ELIMIT, "%s: max_nodes=%d is beyond the cap of %d nodes per graph", who, d->max_nodes, kMaxCap);
    KPGNN_REQUIRE(d->node_ptr && d->edge_ptr && d->graph_ids && d->features && d->source, "%s: NULL node_ptr/edge_ptr/graph_ids/features/source", who);
    KPGNN_REQUIRE(d->node_out && d->graph_out && d->status, "%s: NULL node_out/graph_out/status", who);
    KPGNN_REQUIRE(d->E == 0 || d->edge_index, "%s: NULL edge_index", who);
    GlParams p = {};
    p.G = d->G; p.n_ids = d->n_ids; p.cap = d->max_nodes;
    p.node_ptr = d->node_ptr; p.edge_ptr = d->edge_ptr; p.ei = d->edge_index; p.E = d->E;
    p.ids = d->graph_ids; p.feat = d->features; p.source = d->source;
    p.node_out = d->node_out; p.graph_out = d->graph_out; p.status = d->status;
    hipStream_t s = (hipStream_t)stream;
    if (d->max_nodes <= kWaveCap) {
        constexpr int per = kBlock / kWave;
        hipLaunchKernelGGL(gl_kernel<true>, dim3((unsigned)((d->n_ids + per - 1) / per)), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("gl_kernel<wave>");
    } else {
        hipLaunchKernelGGL(gl_kernel<false>, dim3((unsigned)d->n_ids), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("gl_kernel<block>");
    }
    return KPGNN_OK;
}
