// The random graphs of the graph- and node-property dataset (gfx950).  Contract and the definition of the draw:
// include/kpgnn.h, kpgnn_property_graphs_generate / _fill.
//
// The reference draws one graph at a time on the host (datasets/graph_generation.py generate_graph: a networkx constructor, a
// shuffle, `randomize`, a retry while a node has no neighbour).  Here one team - a wavefront up to 64 nodes, a 256-thread
// block up to 128 - owns one graph for its whole rejection loop, and every random word is a Philox4x32-10 output at a counter
// made of (index, attempt, stream, graph id), so a graph does not depend on its team, its launch or its neighbours.
// One attempt:
//   1. structure on canonical labels: each type writes the LOWER neighbours of every node (bit j < i of row i) - in closed
//      form (grid, caveman, ladder, line, star), from a parent table (caterpillar, lobster, the power-law tree), or from the
//      one lane that walks Barabasi-Albert's attachment; Erdos-Renyi decides its pairs team-parallel into a byte per pair.
//      The two sequential walks (BA's attachment, the tree's degree swaps) run on lane 0, but their Philox words are drawn by
//      the whole team, T at a time, into LDS: lane 0 only multiplies, compares and carries the sum along.
//   2. the rows are made symmetric row-parallel: thread (u, h) owns word h of row u and reads column u of the later rows.
//   3. relabel: a 64-bit key per node, its rank by n comparisons, the inverse permutation in LDS.
//   4. randomize: team-parallel over the n (n - 1) / 2 pairs of the NEW labels, the pair index carried incrementally (no
//      division, no square root); each pair's fate is a byte, and thread (u, h) assembles its word from 64 bytes.  No atomics.
//   5. the vote on a node without neighbour and the edge count are team-wide reductions.
// Integer arithmetic only, but for the feature's exact conversion.  LDS: 6.2 KiB a graph in the wavefront class (25 KiB a block
// of four), 23.5 KiB in the block class - the rows, the keys, a byte per pair (2,016 | 8,128) and BA's list (2,048 | 8,192).
#include "kpgnn_common.h"
#include "philox.h"

namespace kpgnn {
namespace {

typedef unsigned long long u64;
constexpr int kPgBlock = 256;
constexpr int kSwaps = KPGNN_PG_TREE_SWAPS;

struct PgParams {
    int G, n_ids, type, flags, max_attempts;
    uint32_t k0, k1;
    u64 first;
    const int64_t* node_ptr; const int32_t* ids;
    u64* rows; float* features; int32_t* info;
    const int64_t* edge_ptr; int64_t* ei; int64_t E;
};

template <int W, int T>
struct PgLds {
    static constexpr int N = 64 * W;
    u64 low[N * W];                 // bit j < i of row i: the structure as each type writes it
    u64 adj[N * W];                 // the canonical rows, symmetric
    u64 keys[N];
    uint32_t words[T];              // BA: a batch of words for lane 0
    int32_t scal[4];                // what lane 0 tells the team
    int32_t red[4];                 // the block class's partial sums
    uint8_t inv[N], deg[N], par[N];
    uint8_t swp[T], swd[T];         // the tree: a batch of swaps (position, degree)
    uint8_t dec[(N * (N - 1) / 2 + 7) / 8 * 8];     // a byte per pair
    uint8_t rep[2 * (N / 2) * (N / 2)];             // BA's `repeated`: at most 2 m (n - m) entries
};

struct PgStream {
    uint32_t id_lo, id_hi, k0, k1;
    __device__ __forceinline__ Philox4 operator()(int stream, int a, uint32_t i) const {
        return philox4x32_10(i, ((uint32_t)a << 4) | (uint32_t)stream, id_lo, id_hi, k0, k1);
    }
};

__device__ __forceinline__ int below(uint32_t w, int L) { return (int)(((u64)w * (u64)(uint32_t)L) >> 32); }

// round(paretovariate(2)) of a 32-bit word, at most n: the smallest k with v / 2^32 < 1 - 4 / (2k+1)^2
__device__ __forceinline__ int pg_degree(uint32_t v, int n) {
    int k = 1;
    for (; k < n; ++k) {
        const u64 q = (u64)(2 * k + 1) * (u64)(2 * k + 1);
        if ((u64)v * q < ((q - 4) << 32)) break;
    }
    return k;
}

template <bool WAVE>
__device__ __forceinline__ int team_sum(int v, int32_t* red) {
#pragma unroll
    for (int o = kWave >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    if constexpr (!WAVE) {
        if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
        __syncthreads();
        v = red[0] + red[1] + red[2] + red[3];
        __syncthreads();
    }
    return v;
}

template <bool WAVE>
__device__ __forceinline__ bool team_any(bool b) {
    if constexpr (WAVE) {
        const bool r = __ballot(b) != 0ull;
        team_sync<true>();
        return r;
    } else {
        return __syncthreads_or(b) != 0;
    }
}

// f(u, v, q) for the pairs q = u (u - 1) / 2 + v, v < u < n, that thread tid of T takes: q = tid, tid + T, ..
template <typename F>
__device__ __forceinline__ void for_pairs(int n, int tid, int T, F f) {
    int u = 1, v = tid, q = tid;
    while (v >= u && u < n) { v -= u; ++u; }
    while (u < n) {
        f(u, v, q);
        v += T; q += T;
        while (v >= u && u < n) { v -= u; ++u; }
    }
}

// word h of row u from the bytes per pair
__device__ __forceinline__ u64 row_of_pairs(const uint8_t* dec, int u, int lo, int hi) {
    u64 w = 0;
    for (int v = lo; v < hi; ++v) {
        if (v == u) continue;
        const int a = u > v ? u : v, b = u > v ? v : u;
        w |= (u64)(dec[a * (a - 1) / 2 + b] & 1) << (v - lo);
    }
    return w;
}

template <bool WAVE, int W>
__global__ void __launch_bounds__(kPgBlock) pg_kernel(const PgParams p) {
    constexpr int T = WAVE ? kWave : kPgBlock;
    constexpr int N = 64 * W;
    static_assert(T == N * W, "thread (u, h) owns word h of row u");
    constexpr int kTeams = WAVE ? kPgBlock / kWave : 1;
    __shared__ PgLds<W, T> lds[kTeams];
    const int team = WAVE ? (int)threadIdx.x / kWave : 0;
    const int tid = WAVE ? (int)threadIdx.x % kWave : (int)threadIdx.x;
    const int64_t slot = WAVE ? (int64_t)blockIdx.x * kTeams + team : (int64_t)blockIdx.x;
    if (slot >= p.n_ids) return;                    // (a whole team: nobody waits for it below)
    const int g = p.ids ? p.ids[slot] : (int)slot;
    if (g < 0 || g >= p.G) return;
    PgLds<W, T>& L = lds[team];
    const int64_t n0 = p.node_ptr[g];
    const int64_t n64 = p.node_ptr[g + 1] - n0;
    const u64 id = p.first + (u64)g;
    const PgStream rnd = {(uint32_t)id, (uint32_t)(id >> 32), p.k0, p.k1};

    int type = p.type;
    if (type == KPGNN_PG_RANDOM) {
        const int x = below(rnd(KPGNN_PG_STREAM_TYPE, 0, 0).w[0], 20);
        type = x < 4 ? KPGNN_PG_ERDOS_RENYI : x < 8 ? KPGNN_PG_BARABASI_ALBERT : x < 9 ? KPGNN_PG_GRID : x < 10 ? KPGNN_PG_CAVEMAN
             : x < 13 ? KPGNN_PG_TREE : x < 14 ? KPGNN_PG_LADDER : x < 15 ? KPGNN_PG_LINE : x < 16 ? KPGNN_PG_STAR
             : x < 18 ? KPGNN_PG_CATERPILLAR : KPGNN_PG_LOBSTER;
    }
    int32_t* info = p.info + g;
    if (n64 < KPGNN_PG_MIN_NODES || n64 > N) {      // not this class's: nothing but the columns
        if (tid == 0) { info[0] = 0; info[p.G] = 0; info[2 * (int64_t)p.G] = type; info[3 * (int64_t)p.G] = 0; info[4 * (int64_t)p.G] = KPGNN_PG_EXHAUSTED; }
        return;
    }
    const int n = (int)n64;
    const int u = tid / W, h = tid % W, lo = 64 * h, hi = n < lo + 64 ? n : lo + 64;
    const bool shuffle = !(p.flags & KPGNN_PG_NO_SHUFFLE), randomize = !(p.flags & KPGNN_PG_NO_RANDOMIZE);
    const int npairs = n * (n - 1) / 2;
    // bit j of this thread's word, and the bits [a, b) of it
    auto bit = [&](int j) -> u64 { return j >= lo && j < hi ? 1ull << (j - lo) : 0ull; };
    auto span = [&](int a, int b) -> u64 {
        a = a > lo ? a : lo; b = b < hi ? b : hi;
        if (a >= b) return 0ull;
        const int c = b - a;
        return (c == 64 ? ~0ull : (1ull << c) - 1) << (a - lo);
    };
    int r = 1;                                      // the largest divisor of n not above sqrt(n)
    if (type == KPGNN_PG_GRID || type == KPGNN_PG_CAVEMAN)
        for (int i = 2; i * i <= n; ++i) if (n % i == 0) r = i;

    int a = 0;
    bool accepted = false;
    u64 word = 0;
    for (; a < p.max_attempts; ++a) {
        // ---------------------------------------------------------------- 1. the structure
        if (type == KPGNN_PG_ERDOS_RENYI) {
            const uint32_t prob = rnd(KPGNN_PG_STREAM_PARAM, a, 0).w[0];
            for_pairs(n, tid, T, [&](int, int, int q) { L.dec[q] = rnd(KPGNN_PG_STREAM_PAIR, a, (uint32_t)q).w[2] < prob; });
            team_sync<WAVE>();
            L.adj[tid] = u < n ? row_of_pairs(L.dec, u, lo, hi) : 0ull;
        } else {
            u64 lw = 0;
            bool rejected = false;
            if (type == KPGNN_PG_BARABASI_ALBERT) {
                const int m = 1 + below(rnd(KPGNN_PG_STREAM_PARAM, a, 0).w[0], n - 1);
                for (int j = tid; j < 2 * m; j += T) L.rep[j] = (uint8_t)(j < m ? 0 : j - m + 1);
                L.low[tid] = u >= 1 && u <= m ? bit(0) : 0ull;      // the star; lane 0 writes the rows above m
                int s = m + 1, cnt = 0, len = 2 * m;
                u64 m0 = 0, m1 = 0;
                uint32_t t0 = 0;
                bool done = s >= n;
                while (!done) {
                    L.words[tid] = rnd(KPGNN_PG_STREAM_BA, a, t0 + (uint32_t)tid).w[0];
                    team_sync<WAVE>();
                    if (tid == 0) {
                        for (int k = 0; k < T && s < n; ++k) {
                            const int x = L.rep[below(L.words[k], len)];
                            const u64 b = 1ull << (x & 63);
                            if ((x < 64 ? m0 : m1) & b) continue;      // held already: draw again
                            if (x < 64) m0 |= b; else m1 |= b;
                            if (++cnt < m) continue;
                            L.low[s * W] = m0;
                            if (W == 2) L.low[s * W + W - 1] = m1;
                            int l = len;
                            for (u64 mm = m0; mm; mm &= mm - 1) L.rep[l++] = (uint8_t)(__ffsll(mm) - 1);
                            for (u64 mm = m1; mm; mm &= mm - 1) L.rep[l++] = (uint8_t)(64 + __ffsll(mm) - 1);
                            for (int j = 0; j < m; ++j) L.rep[l++] = (uint8_t)s;
                            len = l; ++s; cnt = 0; m0 = m1 = 0;
                        }
                        L.scal[0] = s >= n;
                    }
                    team_sync<WAVE>();
                    done = L.scal[0] != 0;
                    t0 += T;
                }
                team_sync<WAVE>();
                lw = L.low[tid];
            } else if (type == KPGNN_PG_GRID) {
                const int c = n / r;
                if (u < n) lw = (u % c ? bit(u - 1) : 0ull) | (u >= c ? bit(u - c) : 0ull);
            } else if (type == KPGNN_PG_CAVEMAN) {
                const int k = n / r;
                if (u < n) lw = span(u / k * k, u);
            } else if (type == KPGNN_PG_LADDER) {
                const int hh = n >> 1;
                if (u < 2 * hh) lw = (u != 0 && u != hh ? bit(u - 1) : 0ull) | (u >= hh ? bit(u - hh) : 0ull);
                else if (u < n) lw = bit(0);
            } else if (type == KPGNN_PG_LINE) {
                if (u >= 1 && u < n) lw = bit(u - 1);
            } else if (type == KPGNN_PG_STAR) {
                if (u >= 1 && u < n) lw = bit(0);
            } else {                                // a parent per node: caterpillar, lobster, tree
                if (type == KPGNN_PG_TREE) {
                    for (int i = tid; i < n; i += T) L.deg[i] = (uint8_t)pg_degree(rnd(KPGNN_PG_STREAM_TREE, a, (uint32_t)i).w[0], n);
                    team_sync<WAVE>();
                    int sum = team_sum<WAVE>(tid < n ? (int)L.deg[tid] : 0, L.red);
                    const int want = 2 * n - 2;
                    for (int s0 = 0; sum != want && s0 < kSwaps; s0 += T) {
                        const uint32_t i = (uint32_t)n + 2u * (uint32_t)(s0 + tid);
                        L.swp[tid] = (uint8_t)below(rnd(KPGNN_PG_STREAM_TREE, a, i).w[0], n);
                        L.swd[tid] = (uint8_t)pg_degree(rnd(KPGNN_PG_STREAM_TREE, a, i + 1).w[0], n);
                        team_sync<WAVE>();
                        if (tid == 0) {
                            int sm = sum;
                            for (int k = 0; k < T && sm != want && s0 + k < kSwaps; ++k) {
                                const int pos = L.swp[k];
                                sm += (int)L.swd[k] - (int)L.deg[pos];
                                L.deg[pos] = L.swd[k];
                            }
                            L.scal[1] = sm;
                        }
                        team_sync<WAVE>();
                        sum = L.scal[1];
                        team_sync<WAVE>();
                    }
                    rejected = sum != want;
                    if (!rejected) {
                        // the degrees above 1 ascending along the backbone 1 .. I; leaves numbered after it
                        for (int i = tid; i < n; i += T) {
                            const int d = L.deg[i];
                            int inner = 0, rank = 0, before = 0;
                            for (int j = 0; j < n; ++j) {
                                const int dj = L.deg[j];
                                if (dj <= 1) continue;
                                ++inner;
                                if (dj < d || (dj == d && j < i)) { ++rank; before += dj - 2; }
                            }
                            if (i >= 1 && i < inner + 2) L.par[i] = (uint8_t)(i - 1);
                            if (d > 1)
                                for (int l = 0; l < d - 2; ++l)
                                    if (inner + 2 + before + l < n) L.par[inner + 2 + before + l] = (uint8_t)(rank + 1);
                        }
                    }
                } else {
                    const int B = 1 + below(rnd(KPGNN_PG_STREAM_PARAM, a, 0).w[0], n - 1);
                    const int F = type == KPGNN_PG_LOBSTER ? B + 1 + below(rnd(KPGNN_PG_STREAM_PARAM, a, 1).w[0], n - B) : n;
                    for (int i = 1 + tid; i < n; i += T) {
                        const uint32_t w = rnd(KPGNN_PG_STREAM_ATTACH, a, (uint32_t)i).w[0];
                        L.par[i] = (uint8_t)(i < B ? i - 1 : i < F ? below(w, B) : B + below(w, F - B));
                    }
                }
                team_sync<WAVE>();
                if (rejected) continue;             // (the whole team: `sum` is the same in every thread)
                if (u >= 1 && u < n) lw = bit(L.par[u]);
            }
            // ------------------------------------------------------------ 2. symmetric rows
            L.low[tid] = lw;
            team_sync<WAVE>();
            if (u < n)
                for (int j = u + 1 > lo ? u + 1 : lo; j < hi; ++j)
                    lw |= ((L.low[j * W + (u >> 6)] >> (u & 63)) & 1ull) << (j - lo);
            L.adj[tid] = lw;
        }
        team_sync<WAVE>();
        const int e = team_sum<WAVE>(__popcll(L.adj[tid]), L.red) >> 1, miss = npairs - e;
        // ---------------------------------------------------------------- 3. the relabelling
        if (shuffle) {
            for (int i = tid; i < n; i += T) {
                const Philox4 w = rnd(KPGNN_PG_STREAM_SHUFFLE, a, (uint32_t)i);
                L.keys[i] = ((((u64)w.w[1] << 32) | w.w[0]) & ~127ull) | (u64)i;
            }
            team_sync<WAVE>();
            for (int i = tid; i < n; i += T) {
                const u64 key = L.keys[i];
                int rank = 0;
                for (int j = 0; j < n; ++j) rank += L.keys[j] < key;
                L.inv[rank] = (uint8_t)i;
            }
        } else {
            for (int i = tid; i < n; i += T) L.inv[i] = (uint8_t)i;
        }
        team_sync<WAVE>();
        // ---------------------------------------------------------------- 4. randomize, a byte per pair of the new labels
        for_pairs(n, tid, T, [&](int x, int y, int q) {
            const int i = L.inv[x], j = L.inv[y];
            const bool has = (L.adj[i * W + (j >> 6)] >> (j & 63)) & 1ull;
            bool res = has;
            if (randomize) {
                const Philox4 w = rnd(KPGNN_PG_STREAM_PAIR, a, (uint32_t)q);
                const u64 t = (u64)w.w[0] + (u64)w.w[1];
                if (e <= miss) res = has ? 10 * t < (9ull << 33) : 10 * t * (u64)miss < ((u64)e << 33);
                else res = has ? 10 * t * (u64)e < ((u64)(10 * e - miss) << 33) : 10 * t < (1ull << 33);
            }
            L.dec[q] = res;
        });
        team_sync<WAVE>();
        word = u < n ? row_of_pairs(L.dec, u, lo, hi) : 0ull;
        // ---------------------------------------------------------------- 5. every node has a neighbour
        u64 row = word;
        if (W == 2) row |= __shfl_xor(word, 1, kWave);
        if (!team_any<WAVE>(u < n && row == 0ull)) { accepted = true; break; }
    }

    const int edges = team_sum<WAVE>(accepted ? __popcll(word) : 0, L.red);
    if (accepted) {
        if (u < n) {
            p.rows[(n0 + u) * 2 + h] = word;
            if (W == 1) p.rows[(n0 + u) * 2 + 1] = 0ull;
        }
        for (int i = tid; i < n; i += T)
            p.features[n0 + i] = (float)(rnd(KPGNN_PG_STREAM_FEATURE, a, (uint32_t)i).w[0] >> 8) * 0x1p-24f;
    }
    if (tid == 0) {
        const int64_t G = p.G;
        info[0] = edges;
        info[G] = accepted ? below(rnd(KPGNN_PG_STREAM_SOURCE, a, 0).w[0], n) : 0;
        info[2 * G] = type;
        info[3 * G] = accepted ? a + 1 : p.max_attempts;
        info[4 * G] = accepted ? KPGNN_PG_OK : KPGNN_PG_EXHAUSTED;
    }
}

// A block per graph, a wavefront per row: lane l owns bit l of both words; the row's first column is the popcount of the rows before it.
__global__ void __launch_bounds__(kPgBlock) pg_fill_kernel(const PgParams p) {
    const int64_t slot = blockIdx.x;
    if (slot >= p.n_ids) return;
    const int g = p.ids ? p.ids[slot] : (int)slot;
    if (g < 0 || g >= p.G) return;
    const int64_t G = p.G, n0 = p.node_ptr[g], n = p.node_ptr[g + 1] - n0;
    const int64_t e0 = p.edge_ptr[g], count = p.edge_ptr[g + 1] - e0;
    if (p.info[4 * G + g] != KPGNN_PG_OK || n < KPGNN_PG_MIN_NODES || n > KPGNN_PG_MAX_NODES) return;
    if (count != p.info[g] || e0 < 0 || e0 + count > p.E) return;
    const int lane = (int)threadIdx.x % kWave, wave = (int)threadIdx.x / kWave;
    const u64* rows = p.rows + n0 * 2;
    for (int u = wave; u < n; u += kPgBlock / kWave) {
        int before = 0;
        for (int v = lane; v < u; v += kWave) before += __popcll(rows[2 * v]) + __popcll(rows[2 * v + 1]);
#pragma unroll
        for (int o = kWave >> 1; o > 0; o >>= 1) before += __shfl_xor(before, o, kWave);
        const u64 w0 = rows[2 * u], w1 = rows[2 * u + 1], under = (1ull << lane) - 1;
        const int64_t at0 = before + __popcll(w0 & under), at1 = before + __popcll(w0) + __popcll(w1 & under);
        if (((w0 >> lane) & 1ull) && at0 < count) { p.ei[e0 + at0] = u; p.ei[p.E + e0 + at0] = lane; }
        if (((w1 >> lane) & 1ull) && at1 < count) { p.ei[e0 + at1] = u; p.ei[p.E + e0 + at1] = 64 + lane; }
    }
}

int pg_check(const kpgnn_pg_desc* d, const char* who, PgParams* p) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->G >= 0 && d->n_ids >= 0 && d->n_ids <= d->G, "%s: bad G=%d n_ids=%d", who, d->G, d->n_ids);
    KPGNN_REQUIRE(d->max_attempts >= 1 && d->max_attempts <= (1 << 27) && d->first_graph >= 0,
                  "%s: bad max_attempts=%d first_graph=%lld", who, d->max_attempts, (long long)d->first_graph);
    const int t = d->graph_type;
    KPGNN_REQUIRE(t >= KPGNN_PG_RANDOM && t <= KPGNN_PG_LOBSTER && t != 4, "%s: unknown graph_type %d", who, t);
    KPGNN_REQUIRE((d->flags & ~(KPGNN_PG_NO_SHUFFLE | KPGNN_PG_NO_RANDOMIZE)) == 0, "%s: unknown flags 0x%x", who, d->flags);
    KPGNN_REQUIRE(d->max_nodes >= 1 && d->max_nodes <= KPGNN_PG_MAX_NODES, "%s: max_nodes=%d outside [1, %d]", who, d->max_nodes, KPGNN_PG_MAX_NODES);
    if (d->G == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->nodes && d->node_ptr && d->rows && d->info, "%s: NULL nodes/node_ptr/rows/info", who);
    for (int g = 0; g < d->G; ++g)
        if (d->nodes[g] < KPGNN_PG_MIN_NODES || d->nodes[g] > KPGNN_PG_MAX_NODES)
            return fail(KPGNN_ELIMIT, "%s: graph %d has %d nodes, outside [%d, %d]", who, g, d->nodes[g], KPGNN_PG_MIN_NODES, KPGNN_PG_MAX_NODES);
    p->G = d->G; p->n_ids = d->n_ids; p->type = t; p->flags = d->flags; p->max_attempts = d->max_attempts;
    p->k0 = (uint32_t)(uint64_t)d->seed; p->k1 = (uint32_t)((uint64_t)d->seed >> 32);
    p->first = (u64)d->first_graph;
    p->node_ptr = d->node_ptr; p->ids = d->graph_ids;
    p->rows = reinterpret_cast<u64*>(d->rows); p->features = d->features; p->info = d->info;
    p->edge_ptr = d->edge_ptr; p->ei = d->edge_index; p->E = d->E;
    return KPGNN_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_property_graphs_generate(const kpgnn_pg_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_property_graphs_generate";
    PgParams p = {};
    const int rc = pg_check(d, who, &p);
    if (rc != KPGNN_OK || d->G == 0) return rc;
    KPGNN_REQUIRE(d->features != nullptr, "%s: NULL features", who);
    if (d->n_ids == 0) return KPGNN_OK;
    hipStream_t s = (hipStream_t)stream;
    if (d->max_nodes <= KPGNN_PG_WAVE_NODES && !d->force_block) {
        constexpr int per = kPgBlock / kWave;
        hipLaunchKernelGGL((pg_kernel<true, 1>), dim3((unsigned)((d->n_ids + per - 1) / per)), dim3(kPgBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("pg_kernel<wave>");
    } else {
        hipLaunchKernelGGL((pg_kernel<false, 2>), dim3((unsigned)d->n_ids), dim3(kPgBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("pg_kernel<block>");
    }
    return KPGNN_OK;
}

extern "C" int kpgnn_property_graphs_fill(const kpgnn_pg_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_property_graphs_fill";
    PgParams p = {};
    const int rc = pg_check(d, who, &p);
    if (rc != KPGNN_OK || d->G == 0) return rc;
    KPGNN_REQUIRE(d->E >= 0 && d->edge_ptr != nullptr && (d->E == 0 || d->edge_index != nullptr), "%s: bad E=%lld or NULL edge_ptr/edge_index", who, (long long)d->E);
    if (d->n_ids == 0 || d->E == 0) return KPGNN_OK;
    hipLaunchKernelGGL(pg_fill_kernel, dim3((unsigned)d->n_ids), dim3(kPgBlock), 0, (hipStream_t)stream, p);
    KPGNN_LAUNCH_CHECK("pg_fill_kernel");
    return KPGNN_OK;
}
