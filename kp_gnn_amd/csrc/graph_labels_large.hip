// The six labels of the synthetic graph- and node-property dataset for graphs of up to 128 nodes, batched over graphs (gfx950).
// Contract: include/kpgnn.h, kpgnn_graph_labels_large.  The third size class of csrc/graph_labels.hip, whose method this file
// keeps step by step; what changes is the row, which is TWO 64-bit words in LDS (bit j & 63 of word j >> 6 of row i: the
// edge i - j; bit 64 is bit 0 of the second word), and the team, which is always one 256-thread block per graph:
//   1. the rows by LDS atomic OR on the word that holds the bit; an endpoint outside [0, n) ends the graph with status 3, a self
//      loop with 4, a source outside [0, n) with 5 - every range is checked before anything is indexed with it - and A != A^T
//      with status 1;
//   2. all-source BFS, lane i the source i, over both words: eccentricity, sssp and (from the eccentricities) the diameter;
//   3. the reference's is_connected as m = 1 + ceil(log2 n) boolean squarings of the two-word matrix, then "every row full",
//      the full row being ~0 in a word the graph fills and (1 << (n & 63)) - 1 in its last, partial word - no shift by 64.
//      For n <= 64 that is graph_labels.hip's own argument; for 65 <= n <= 128, m = 8 and every entry of A^(2^7) is at most
//      127^128 < 2^895, so the reference's last float64 squaring multiplies no inf by 0: it makes no nan, rounds no positive
//      integer to zero, and min > 0 holds iff the eighth boolean squaring has no zero.  At n = 129, m = 9 and stage 8 can hold
//      inf next to zeros: the cap of this file;
//   4. laplacian[i] = deg(i) F[i] - sum_{j in adj(i)} F[j], in double, ascending j (the first word, then the second), rounded
//      to float once;
//   5. the spectral radius: Householder tridiagonalisation of the n x n double matrix in LDS, then Sturm-count multisection
//      for the top eigenvalue from (0, maxdeg + 1] - the 64 lanes of the block's first wavefront evaluate 64 probes a round,
//      11 rounds.  An edgeless graph answers exactly 0.
// Every sum that crosses lanes is taken by each lane on its own, serially in index order, from LDS; every matrix element is
// updated by one expression whichever thread holds it; floating-point contraction is off in this file.  So the bits of a
// graph do not depend on the edge order, on the other graphs of the launch or on graph_ids.  The matrix has an ODD row stride
// (n | 1) and, with the vectors and the bit rows, lives in dynamic LDS sized for the launch's max_nodes: 143,888 bytes at 128,
// one block per CU.  256 threads: per column the three serial sums (3 (n - k) dependent adds in every lane) outweigh the
// rank-2 update ((n - k)^2 / 256 elements a thread), so a wider block would shorten the smaller term only.  No global
// atomics, no float atomics.
#include "kpgnn_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace kpgnn {
namespace {

constexpr int kBlock = 256;
constexpr int kCap = KPGNN_GL_LARGE_MAX_NODES;
constexpr int kRounds = 11;
constexpr double kNegligible = 1e-200;
typedef unsigned long long u64;

struct GllParams {
    int G, n_ids, cap;
    const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* ei; int64_t E;
    const int32_t* ids;
    const double* feat; const int32_t* source;
    float* node_out; float* graph_out; int32_t* status;
};

// LDS of a block sized for graphs of up to `cap` nodes: M [cap][cap | 1], v, p, d, e2, F [cap] doubles; rows [cap][2],
// sq [2][cap][2] words; ecc [cap], flags [4] ints.  Every offset is a multiple of 8.
__host__ __device__ constexpr size_t lds_bytes(int cap) {
    return ((size_t)cap * (cap | 1) + 5 * (size_t)cap) * 8 + 6 * (size_t)cap * 8 + (size_t)cap * 4 + 16;
}
static_assert(lds_bytes(kCap) <= 160 * 1024, "the double matrix of the largest graph must fit the LDS of a CU");

__device__ __forceinline__ int popc2(u64 a, u64 b) { return __builtin_popcountll(a) + __builtin_popcountll(b); }

__global__ void __launch_bounds__(kBlock) gl_large_kernel(const GllParams p) {
    extern __shared__ __attribute__((aligned(16))) double gll_lds[];
    constexpr int T = kBlock;
    const int tid = (int)threadIdx.x;
    const int64_t slot = (int64_t)blockIdx.x;
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
    if (n64 > p.cap || n64 > kCap) {
        if (tid == 0) p.status[g] = KPGNN_GL_TOO_LARGE;
        return;
    }
    const int n = (int)n64, s = n | 1, cap = p.cap;
    int64_t e0 = p.edge_ptr[g], e1 = p.edge_ptr[g + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > p.E ? p.E : e1;
    // the carve is by the launch's cap (n <= cap), so a graph's bits cannot depend on it: only addresses move
    double* M = gll_lds;
    double* Lv = M + (size_t)cap * (cap | 1);
    double* Lp = Lv + cap;
    double* Ld = Lp + cap;
    double* Le2 = Ld + cap;
    double* LF = Le2 + cap;
    u64* rows = reinterpret_cast<u64*>(LF + cap);           // [cap][2]
    u64* sq0 = rows + 2 * cap;                              // [2][cap][2]
    u64* sq1 = sq0 + 2 * cap;
    int* ecc = reinterpret_cast<int*>(sq1 + 2 * cap);
    int* flags = ecc + cap;     // [0] endpoint, [1] self loop, [2] asymmetric, [3] a row of the squared matrix is not full
    // a full row: word 0 and word 1 (n == 64 and n == 128 fill their last word; a word the graph does not reach is 0)
    const u64 full0 = n >= 64 ? ~0ull : (1ull << n) - 1ull;
    const u64 full1 = n <= 64 ? 0ull : n == 128 ? ~0ull : (1ull << (n - 64)) - 1ull;
    const int myw = tid >> 6, myb = tid & 63;               // (used where tid < n only)

    // 1. the rows, the checks
    if (tid < n) { rows[2 * tid] = 0ull; rows[2 * tid + 1] = 0ull; LF[tid] = p.feat[n0 + tid]; }
    if (tid < 4) flags[tid] = 0;
    __syncthreads();
    for (int64_t e = e0 + tid; e < e1; e += T) {
        const int64_t u = p.ei[e], v = p.ei[p.E + e];
        if (u < 0 || u >= n || v < 0 || v >= n) flags[0] = 1;
        else if (u == v) flags[1] = 1;
        else atomicOr(&rows[2 * (int)u + ((int)v >> 6)], 1ull << ((int)v & 63));
    }
    __syncthreads();
    u64 mine0 = 0ull, mine1 = 0ull;
    if (tid < n) {
        mine0 = rows[2 * tid];
        mine1 = rows[2 * tid + 1];
        bool bad = false;
        for (u64 f = mine0; f; f &= f - 1ull) bad |= !((rows[2 * __builtin_ctzll(f) + myw] >> myb) & 1ull);
        for (u64 f = mine1; f; f &= f - 1ull) bad |= !((rows[2 * (64 + __builtin_ctzll(f)) + myw] >> myb) & 1ull);
        if (bad) flags[2] = 1;
    }
    __syncthreads();
    const int src = p.source[g];
    {
        const int st = flags[0] ? KPGNN_GL_ENDPOINT : flags[1] ? KPGNN_GL_SELF_LOOP
                     : (src < 0 || src >= n) ? KPGNN_GL_SOURCE : flags[2] ? KPGNN_GL_ASYMMETRIC : KPGNN_GL_OK;
        if (st != KPGNN_GL_OK) {
            if (tid == 0) p.status[g] = st;
            return;
        }
    }

    // 2. all-source BFS; 4. the laplacian column
    if (tid < n) {
        u64 seen0 = myw == 0 ? 1ull << myb : 0ull, seen1 = myw == 1 ? 1ull << myb : 0ull;
        u64 fr0 = seen0, fr1 = seen1;
        const int sb = src & 63;
        int level = 0, sd = 0;
        for (;;) {
            u64 nx0 = 0ull, nx1 = 0ull;
            for (u64 f = fr0; f; f &= f - 1ull) { const int j = __builtin_ctzll(f); nx0 |= rows[2 * j]; nx1 |= rows[2 * j + 1]; }
            for (u64 f = fr1; f; f &= f - 1ull) { const int j = 64 + __builtin_ctzll(f); nx0 |= rows[2 * j]; nx1 |= rows[2 * j + 1]; }
            nx0 &= ~seen0;
            nx1 &= ~seen1;
            if (!(nx0 | nx1)) break;
            ++level;
            seen0 |= nx0;
            seen1 |= nx1;
            if (((src < 64 ? nx0 : nx1) >> sb) & 1ull) sd = level;
            fr0 = nx0;
            fr1 = nx1;
        }
        ecc[tid] = level;
        double acc = (double)popc2(mine0, mine1) * LF[tid];
        for (u64 f = mine0; f; f &= f - 1ull) acc -= LF[__builtin_ctzll(f)];
        for (u64 f = mine1; f; f &= f - 1ull) acc -= LF[64 + __builtin_ctzll(f)];
        float* o = p.node_out + (n0 + tid) * 3;
        o[0] = (float)sd;
        o[1] = (float)level;
        o[2] = (float)acc;
        sq0[2 * tid] = mine0;
        sq0[2 * tid + 1] = mine1;
    }

    // 3. m boolean squarings
    int m = 1;
    while ((1 << (m - 1)) < n) ++m;                  // 1 + ceil(log2 n)
    u64* cur = sq0;
    u64* nxt = sq1;
    for (int r = 0; r < m; ++r) {
        __syncthreads();
        if (tid < n) {
            u64 a0 = 0ull, a1 = 0ull;
            for (u64 f = cur[2 * tid]; f; f &= f - 1ull) { const int j = __builtin_ctzll(f); a0 |= cur[2 * j]; a1 |= cur[2 * j + 1]; }
            for (u64 f = cur[2 * tid + 1]; f; f &= f - 1ull) { const int j = 64 + __builtin_ctzll(f); a0 |= cur[2 * j]; a1 |= cur[2 * j + 1]; }
            nxt[2 * tid] = a0;
            nxt[2 * tid + 1] = a1;
        }
        u64* t = cur; cur = nxt; nxt = t;
    }
    if (tid < n && (cur[2 * tid] != full0 || cur[2 * tid + 1] != full1)) flags[3] = 1;

    // 5. the matrix, tridiagonalised in place: d the diagonal, e2 the squared off-diagonal
    int cw = 8;
    while (cw < n) cw <<= 1;
    const int j = tid & (cw - 1), i0 = tid / cw, istep = T / cw;
    for (int i = i0; i < n; i += istep)
        if (j < n) M[i * s + j] = (double)((rows[2 * i + (j >> 6)] >> (j & 63)) & 1ull);
    __syncthreads();            // (also publishes ecc and flags[3])
    for (int k = 0; k + 2 < n; ++k) {
        const int k1 = k + 1;
        const double x1 = M[k1 * s + k];
        double rest = 0.0;
        for (int r = k1 + 1; r < n; ++r) { const double x = M[r * s + k]; rest += x * x; }
        if (tid == 0) Ld[k] = M[k * s + k];
        // the column is tridiagonal already, or as good as: entries below 1e-100 - rounding residue of a low-rank matrix, which
        // would overflow 1 / (v.v) - move an eigenvalue of a matrix of norm >= 1 by less than 1e-98 (uniform over the block)
        if (rest < kNegligible) {
            if (tid == 0) Le2[k] = x1 * x1;
            continue;
        }
        const double sigma = rest + x1 * x1;
        const double alpha = x1 > 0.0 ? -sqrt(sigma) : sqrt(sigma);
        const double beta = 1.0 / (sigma - alpha * x1);               // 2 / v.v
        if (tid == 0) Le2[k] = alpha * alpha;
        for (int r = k1 + tid; r < n; r += T) Lv[r] = M[r * s + k] - (r == k1 ? alpha : 0.0);
        __syncthreads();
        for (int r = k1 + tid; r < n; r += T) {
            double a = 0.0;
            for (int c = k1; c < n; ++c) a += M[r * s + c] * Lv[c];
            Lp[r] = beta * a;
        }
        __syncthreads();
        double pv = 0.0;
        for (int r = k1; r < n; ++r) pv += Lp[r] * Lv[r];
        const double kc = 0.5 * beta * pv;
        if (j >= k1 && j < n) {
            const double vj = Lv[j], wj = Lp[j] - kc * vj;
            for (int i = k1 + i0; i < n; i += istep) {
                const double vi = Lv[i], wi = Lp[i] - kc * vi;
                M[i * s + j] -= vi * wj + wi * vj;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (n >= 2) {
            const double x = M[(n - 1) * s + (n - 2)];
            Ld[n - 2] = M[(n - 2) * s + (n - 2)];
            Le2[n - 2] = x * x;
        }
        Ld[n - 1] = M[(n - 1) * s + (n - 1)];
    }
    __syncthreads();
    if (tid >= kWave) return;                         // the block's first wavefront goes on alone: no barrier below

    int maxdeg = 0, diam = 0;
    for (int i = 0; i < n; ++i) {
        const int dg = popc2(rows[2 * i], rows[2 * i + 1]), ec = ecc[i];
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
            double q = Ld[0] - x;
            int cnt = q < 0.0;
            for (int i = 1; i < n; ++i) {
                if (fabs(q) < 1e-300) q = -1e-300;
                q = (Ld[i] - x) - Le2[i - 1] / q;
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
        o[0] = flags[3] ? 0.f : 1.f;
        o[1] = (float)diam;
        o[2] = (float)radius;
        p.status[g] = KPGNN_GL_OK;
    }
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_graph_labels_large(const kpgnn_graph_labels_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_graph_labels_large";
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->G >= 0 && d->n_ids >= 0 && d->E >= 0, "%s: bad G=%d n_ids=%d E=%lld", who, d->G, d->n_ids, (long long)d->E);
    if (d->G == 0 || d->n_ids == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->max_nodes >= 1, "%s: bad max_nodes=%d", who, d->max_nodes);
    if (d->max_nodes > kCap) return fail(KPGNN_ELIMIT, "%s: max_nodes=%d is beyond the cap of %d nodes per graph", who, d->max_nodes, kCap);
    KPGNN_REQUIRE(d->node_ptr && d->edge_ptr && d->graph_ids && d->features && d->source, "%s: NULL node_ptr/edge_ptr/graph_ids/features/source", who);
    KPGNN_REQUIRE(d->node_out && d->graph_out && d->status, "%s: NULL node_out/graph_out/status", who);
    KPGNN_REQUIRE(d->E == 0 || d->edge_index, "%s: NULL edge_index", who);
    GllParams p = {};
    p.G = d->G; p.n_ids = d->n_ids; p.cap = d->max_nodes;
    p.node_ptr = d->node_ptr; p.edge_ptr = d->edge_ptr; p.ei = d->edge_index; p.E = d->E;
    p.ids = d->graph_ids; p.feat = d->features; p.source = d->source;
    p.node_out = d->node_out; p.graph_out = d->graph_out; p.status = d->status;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = lds_bytes(p.cap);
    KPGNN_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&gl_large_kernel), lds));
    hipLaunchKernelGGL(gl_large_kernel, dim3((unsigned)d->n_ids), dim3(kBlock), lds, s, p);
    KPGNN_LAUNCH_CHECK("gl_large_kernel");
    return KPGNN_OK;
}
