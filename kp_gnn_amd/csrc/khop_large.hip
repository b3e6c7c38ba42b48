// The K-hop pre-transform for graphs above 64 nodes (gfx950).  Contract: include/kpgnn.h, kpgnn_khop_large_*.
//
// The second device restatement of transform_graph / peripheral_stats of khop_host.cpp, which stays the specification (SURVEY
// Q1 - Q8).  Row i of every W_k depends only on row i of W_{k-1}, so the unit of work is a SOURCE NODE, not a graph; what a
// graph's rows share - its adjacency - is built once per graph in the workspace by the count pass and read by both passes.
//   large_prep (count pass, one block per graph): checks the edges (ENDPOINT / TYPE), then two STABLE counting sorts of the
//     graph's edge slice, by destination and then by source.  A position is bucket start + edges of the key in earlier chunks
//     of 256 + equal keys at lower threads of this chunk - counted, not raced for, so the lists are the same bits on every run.
//     The first sort is the in-list (sources of the raw edges into j, duplicates kept: they supply the multiplicity of the pull
//     sum); the second leaves the edges in (source, destination) order, where the first edge of each run of duplicates gets the
//     run's summed type and the others 0 (the per-row merge; a sum above 63 is TYPE), and the non-zero-type neighbour words
//     nzt[u] follow from one walk of the row by one thread.
//   large_walk<FILL> (both passes, one wavefront per source row, four rows per block, blockIdx.y strides the rows): two uint32
//     count rows in LDS; W_1[i] = the out-row of i, W_{k+1}[i][j] = sum of W_k[i][u] over the in-list of j, summed in 64 bits
//     and clamped to 2^32 - 1 (any order gives min(2^32 - 1, true count): kpgnn.h).  A hop's set is the ballot of "count > 0,
//     j != i" word by word (spd: and not reached before); an off-diagonal count >= 2^31 is RANGE.  The count pass leaves the
//     any-hop words and their popcount; the fill pass writes every (edge, hop) slot of the row exactly once - the target's rank
//     is the word prefix + popcount below the lane - and then the peripheral statistics of its K hop sets, the wavefront
//     working one (node, hop) item at a time with lane l holding word l of the reach / frontier sets: a BFS level is the OR of
//     the nzt rows of the frontier masked by S & ~reach, the edge-type histogram 64 bins of 32 bits in LDS.
//   large_finish (count pass, one block per graph): degree 0 for every node of a graph whose status is not 0 (RANGE is found
//     by whichever row meets it, after other rows have written their degrees).
// LDS per wavefront: 8 W (K + 4) + 4 W' + 256 + 8 * 64 W bytes, W = ceil(max_nodes / 64), W' = W rounded up to even: 21,888
// at max_nodes = 2048, K = 16 (87,552 per block).  LDS integer atomics only where the sum is the result (the histograms, the
// bucket counts, W_1); no global atomics, no float; every global write of the fill pass is range-checked, and every index read
// back from the workspace is checked before it addresses LDS or the workspace.
#include "kpgnn_common.h"

namespace kpgnn {
namespace {

constexpr int kBlock = 256;
constexpr int kRows = kBlock / kWave;           // source rows (wavefronts) per block of the walk
constexpr int kCap = KPGNN_KHOP_LARGE_MAX_NODES;
constexpr int kMaxType = KPGNN_KHOP_MAX_TYPE;
constexpr int kMaxK = KPGNN_KHOP_MAX_K, kMaxT = KPGNN_KHOP_MAX_T, kMaxH = KPGNN_KHOP_MAX_H;
constexpr int kBins = kMaxType + 1;
constexpr int kMaxRowBlocks = 128;              // blockIdx.y of the walk: a wavefront takes rows y * 4 + wave, + 4 * gridDim.y, ...
constexpr uint32_t kSat = 0xFFFFFFFFu;
constexpr uint32_t kInt32Limit = 0x80000000u;
static_assert(kBins == kWave, "one histogram bin per lane");
static_assert(kCap % 64 == 0 && kCap / 64 <= kWave, "lane l holds word l of a node set");

struct LargeParams {
    int G, n_ids, cap, W;
    int64_t N, E_in, E_out;
    const int32_t* ids;
    const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* ei; const int64_t* ea;
    int K, max_attr, H, T, max_edge_count, max_dist_count, gd;
    int64_t* deg; uint64_t* any; uint64_t* nzt;
    int32_t* in_start; int32_t* in_cnt; int32_t* out_start; int32_t* out_cnt;
    int32_t* in_src; int32_t* s_dst; int32_t* m_typ; int32_t* o_src; int32_t* o_dst; int32_t* o_typ;
    int32_t* status;
    const int64_t* node_off;
    int64_t* o_ei; int64_t* o_ea; int64_t* o_pe; int64_t* o_pea; int64_t* o_pca; int64_t* o_batch;
};

__host__ __device__ constexpr int words_of(int nodes) { return (nodes + 63) >> 6; }
__host__ __device__ constexpr size_t wave_bytes(int W, int K) {
    return (size_t)8 * W * (K + 4) + (size_t)4 * ((W + 1) & ~1) + (size_t)4 * kBins + (size_t)8 * 64 * W;
}

__device__ __forceinline__ void wave_sync() {   // one wavefront: its LDS operations complete in order; keep the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ uint64_t below(int j) { return ((uint64_t)1 << j) - 1; }     // j in [0, 63]
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = kWave >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int o = kWave >> 1; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, kWave), hi = (uint32_t)__shfl_xor((int)(v >> 32), o, kWave);
        v += (int64_t)(((uint64_t)hi << 32) | lo);
    }
    return v;
}

// The graph of a slot and its node / edge ranges; false: nothing to do here (an id outside [0, G)), *bad: offsets that do not
// describe nodes of this call.
__device__ __forceinline__ bool graph_of(const LargeParams& p, int64_t slot, int* g, int64_t* n0, int64_t* n, bool* bad) {
    *bad = false;
    if (slot >= p.n_ids) return false;
    *g = p.ids[slot];
    if (*g < 0 || *g >= p.G) return false;
    *n0 = p.node_ptr[*g];
    *n = p.node_ptr[*g + 1] - *n0;
    *bad = *n0 < 0 || *n < 0 || *n0 + *n > p.N;
    return true;
}

// a[q] -> the exclusive running sum of a[0 .. n) plus base, the counts themselves to cnt_out / the sums to start_out
__device__ void block_scan(int* a, int n, int base, int* part, int32_t* start_out, int32_t* cnt_out) {
    const int tid = threadIdx.x, per = (n + kBlock - 1) / kBlock;
    const int lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    int s = 0;
    for (int q = lo; q < hi; ++q) s += a[q];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = base;
        for (int t = 0; t < kBlock; ++t) { const int c = part[t]; part[t] = run; run += c; }
    }
    __syncthreads();
    int run = part[tid];
    for (int q = lo; q < hi; ++q) {
        const int c = a[q];
        a[q] = run;
        start_out[q] = run;
        cnt_out[q] = c;
        run += c;
    }
    __syncthreads();
}

// Stable counting sort of the positions [e0, e1) by key(e) into put(e, position); cursor[key]: the bucket's next free position.
template <typename KeyF, typename PutF>
__device__ void stable_place(int64_t e0, int64_t e1, int* cursor, int* keys, KeyF key, PutF put) {
    const int tid = threadIdx.x;
    for (int64_t base = e0; base < e1; base += kBlock) {
        const int64_t e = base + tid;
        const bool live = e < e1;
        const int k = live ? key(e) : -1;
        keys[tid] = k;
        __syncthreads();
        int pos = 0;
        if (live) {
            int rank = 0;
            for (int t = 0; t < tid; ++t) rank += keys[t] == k;
            pos = cursor[k] + rank;
        }
        __syncthreads();
        if (live) {
            put(e, pos);
            atomicAdd(&cursor[k], 1);
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kBlock) large_prep(const LargeParams p) {
    __shared__ int cnt_in[kCap], cnt_out[kCap], keys[kBlock], part[kBlock], flags[2];      // flags: [0] endpoint, [1] type
    const int tid = threadIdx.x;
    int g;
    int64_t n0, n64;
    bool bad;
    if (!graph_of(p, blockIdx.x, &g, &n0, &n64, &bad)) return;
    int st = KPGNN_KHOP_OK;
    if (bad) st = KPGNN_KHOP_ENDPOINT;
    else if (p.K > kMaxK || p.T > kMaxT || p.H > kMaxH) st = KPGNN_KHOP_SHAPE;
    else if (n64 > p.cap) st = KPGNN_KHOP_TOO_LARGE;
    if (st != KPGNN_KHOP_OK || n64 == 0) {
        if (tid == 0) p.status[g] = st;
        return;
    }
    const int n = (int)n64, nW = words_of(n);
    int64_t e0 = p.edge_ptr[g], e1 = p.edge_ptr[g + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > p.E_in ? p.E_in : e1;
    if (e1 < e0) e1 = e0;

    for (int q = tid; q < n; q += kBlock) { cnt_in[q] = 0; cnt_out[q] = 0; }
    if (tid < 2) flags[tid] = 0;
    __syncthreads();
    for (int64_t e = e0 + tid; e < e1; e += kBlock) {
        const int64_t u = p.ei[e], v = p.ei[p.E_in + e], t = p.ea ? p.ea[e] : 2;
        if (u < 0 || u >= n || v < 0 || v >= n) flags[0] = 1;
        else if (t < 0 || t > kMaxType) flags[1] = 1;
        else {
            atomicAdd(&cnt_in[(int)v], 1);
            atomicAdd(&cnt_out[(int)u], 1);
        }
    }
    __syncthreads();
    if (flags[0] || flags[1]) {
        if (tid == 0) p.status[g] = flags[0] ? KPGNN_KHOP_ENDPOINT : KPGNN_KHOP_TYPE;
        return;
    }
    block_scan(cnt_in, n, (int)e0, part, p.in_start + n0, p.in_cnt + n0);
    block_scan(cnt_out, n, (int)e0, part, p.out_start + n0, p.out_cnt + n0);
    // by destination: the in-lists
    stable_place(e0, e1, cnt_in, keys, [&](int64_t e) { return (int)p.ei[p.E_in + e]; },
                 [&](int64_t e, int pos) {
                     p.in_src[pos] = (int32_t)p.ei[e];
                     p.s_dst[pos] = (int32_t)p.ei[p.E_in + e];
                     p.m_typ[pos] = p.ea ? (int32_t)p.ea[e] : 2;
                 });
    // ... then by source: (source, destination) order
    stable_place(e0, e1, cnt_out, keys, [&](int64_t e) { return (int)p.in_src[e]; },
                 [&](int64_t e, int pos) {
                     p.o_src[pos] = p.in_src[e];
                     p.o_dst[pos] = p.s_dst[e];
                     p.o_typ[pos] = p.m_typ[e];
                 });
    // the merge: the first edge of a run of duplicates carries the run's summed type, the others 0
    for (int64_t q = e0 + tid; q < e1; q += kBlock) {
        const int32_t u = p.o_src[q], v = p.o_dst[q];
        int sum = 0;
        if (q == e0 || p.o_src[q - 1] != u || p.o_dst[q - 1] != v) {
            sum = p.o_typ[q];
            for (int64_t r = q + 1; r < e1 && p.o_src[r] == u && p.o_dst[r] == v; ++r)
                sum = sum > kMaxType ? sum : sum + p.o_typ[r];
            if (sum > kMaxType) flags[1] = 1;
        }
        p.m_typ[q] = sum;
    }
    __syncthreads();
    if (flags[1]) {
        if (tid == 0) p.status[g] = KPGNN_KHOP_TYPE;
        return;
    }
    for (int u = tid; u < n; u += kBlock) {         // the non-zero-type neighbour words of row u (its row is in target order)
        uint64_t* row = p.nzt + (size_t)(n0 + u) * p.W;
        for (int w = 0; w < nW; ++w) row[w] = 0;
        const int64_t s = p.out_start[n0 + u], c = p.out_cnt[n0 + u];
        int at = -1;
        uint64_t word = 0;
        for (int64_t q = s; q < s + c; ++q) {
            if (p.m_typ[q] == 0) continue;
            const int v = p.o_dst[q];
            if ((v >> 6) != at) {
                if (at >= 0) row[at] = word;
                at = v >> 6;
                word = 0;
            }
            word |= (uint64_t)1 << (v & 63);
        }
        if (at >= 0) row[at] = word;
    }
    if (tid == 0) p.status[g] = KPGNN_KHOP_OK;
}

__global__ void __launch_bounds__(kBlock) large_finish(const LargeParams p) {
    int g;
    int64_t n0, n64;
    bool bad;
    if (!graph_of(p, blockIdx.x, &g, &n0, &n64, &bad) || bad) return;
    if (p.status[g] == KPGNN_KHOP_OK) return;
    for (int64_t i = threadIdx.x; i < n64; i += kBlock) p.deg[n0 + i] = 0;
}

// What a wavefront keeps in LDS for its row.
struct RowLds {
    uint64_t* hs;       // [K][W] hop sets
    uint64_t* reach;    // [W]
    uint64_t* anyw;     // [W] the any-hop words being built
    uint64_t* afw;      // [W] fill: the any-hop words of the count pass
    uint64_t* fr;       // [W] a node set the whole wavefront enumerates
    int* pref;          // [W] targets in the any-hop words before word w
    uint32_t* hist;     // [64]
    uint32_t* cur;      // [64 W] walk counts of this hop
    uint32_t* nxt;      // [64 W] ... of the next (fill: first the summed types of the row's 1-hop edges)
};

// The checked out-row of node u of the graph at n0: positions [*s, *s + count) of o_dst / m_typ.
__device__ __forceinline__ int out_row(const LargeParams& p, int64_t n0, int u, int64_t* s) {
    *s = p.out_start[n0 + u];
    const int64_t c = p.out_cnt[n0 + u];
    return (*s < 0 || c < 0 || *s + c > p.E_in) ? 0 : (int)c;
}

// Peripheral statistics of the subgraph induced on S ([nW] words in LDS): peripheral_stats of khop_host.cpp, by one wavefront.
__device__ void peripheral_item(const LargeParams& p, const RowLds& L, int64_t n0, int n, int nW, const uint64_t* S, int lane,
                                int64_t* pe_out, int64_t* pc_out) {
    const int T = p.T, H = p.H;
    int m = 0;
    for (int w = 0; w < nW; ++w) m += __builtin_popcountll(S[w]);
    int64_t total = 0;
    if (m >= 2) {
        L.hist[lane] = 0;
        wave_sync();
        for (int w = 0; w < nW; ++w)
            for (uint64_t us = S[w]; us; us &= us - 1) {
                int64_t s;
                const int c = out_row(p, n0, w * 64 + __ffsll((long long)us) - 1, &s);
                for (int q = lane; q < c; q += kWave) {
                    const uint32_t t = (uint32_t)p.m_typ[s + q], v = (uint32_t)p.o_dst[s + q];
                    if (t > 0 && t < (uint32_t)kBins && v < (uint32_t)n && ((S[v >> 6] >> (v & 63)) & 1)) atomicAdd(&L.hist[t], 1u);
                }
            }
        wave_sync();
        total = wave_sum((int64_t)L.hist[lane]);
    }
    if (total == 0) {       // fewer than two nodes, or no typed edge among them: zeros
        if (lane < 2 * T) pe_out[lane] = 0;
        if (lane <= H) pc_out[lane] = 0;
        return;
    }
    if (lane == 0) {        // stable descending: the largest count, the lowest type among equals
        uint64_t taken = 0;
        for (int t = 0; t < T; ++t) {
            int best = 2;
            int64_t bc = -1;
            for (int b = 2; b < kBins; ++b)
                if (!((taken >> b) & 1) && (int64_t)L.hist[b] > bc) { bc = L.hist[b]; best = b; }
            taken |= (uint64_t)1 << best;
            pe_out[2 * t] = best - 2;                           // index into edge_count[2:], i.e. type - 2 (Q4)
            pe_out[2 * t + 1] = bc < p.max_edge_count ? bc : p.max_edge_count;
        }
    }
    int64_t conf[kMaxH + 1];                                    // this lane's share
#pragma unroll
    for (int h = 0; h <= kMaxH; ++h) conf[h] = 0;
    const uint64_t Sw = lane < nW ? S[lane] : 0;
    for (int w = 0; w < nW; ++w)
        for (uint64_t ss = S[w]; ss; ss &= ss - 1) {
            const int src = w * 64 + __ffsll((long long)ss) - 1;
            uint64_t reachw = lane == (src >> 6) ? (uint64_t)1 << (src & 63) : 0, frontw = reachw;
#pragma unroll
            for (int h = 1; h <= kMaxH; ++h) {
                if (h > H) break;
                if (lane < nW) L.fr[lane] = frontw;
                wave_sync();
                uint64_t next = 0;
                for (int fw = 0; fw < nW; ++fw)
                    for (uint64_t us = L.fr[fw]; us; us &= us - 1) {
                        const int u = fw * 64 + __ffsll((long long)us) - 1;
                        if (lane < nW) next |= p.nzt[(size_t)(n0 + u) * p.W + lane];
                    }
                next &= Sw & ~reachw;
                reachw |= next;
                frontw = next;
                const int mine = __builtin_popcountll(next);
                const int cls = wave_sum(mine);
                wave_sync();
                if (cls == 0) break;
                conf[h] += mine;
                if (cls >= 2) {                                 // sum of edge-type VALUES inside the distance class (Q5)
                    if (lane < nW) L.fr[lane] = next;
                    wave_sync();
                    for (int fw = 0; fw < nW; ++fw)
                        for (uint64_t us = L.fr[fw]; us; us &= us - 1) {
                            int64_t s;
                            const int c = out_row(p, n0, fw * 64 + __ffsll((long long)us) - 1, &s);
                            for (int q = lane; q < c; q += kWave) {
                                const uint32_t v = (uint32_t)p.o_dst[s + q];
                                if (v < (uint32_t)n && ((L.fr[v >> 6] >> (v & 63)) & 1)) conf[0] += p.m_typ[s + q];
                            }
                        }
                    wave_sync();
                }
            }
        }
#pragma unroll
    for (int h = 0; h <= kMaxH; ++h)
        if (h <= H) {
            const int64_t c = wave_sum(conf[h]);
            if (lane == 0) pc_out[h] = c < p.max_dist_count ? c : p.max_dist_count;
        }
}

template <bool FILL>
__global__ void __launch_bounds__(kBlock) large_walk(const LargeParams p) {
    extern __shared__ uint64_t khop_large_lds[];
    const int lane = (int)threadIdx.x % kWave, wave = (int)threadIdx.x / kWave;
    int g;
    int64_t n0, n64;
    bool bad;
    if (!graph_of(p, blockIdx.x, &g, &n0, &n64, &bad) || bad) return;
    if (p.status[g] != KPGNN_KHOP_OK || n64 > p.cap || n64 == 0) return;        // (count: large_prep has judged the graph)
    const int n = (int)n64, nW = words_of(n), W = p.W, K = p.K;

    RowLds L;
    L.hs = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(khop_large_lds) + (size_t)wave * wave_bytes(W, K));
    L.reach = L.hs + (size_t)K * W;
    L.anyw = L.reach + W;
    L.afw = L.anyw + W;
    L.fr = L.afw + W;
    L.pref = reinterpret_cast<int*>(L.fr + W);
    L.hist = reinterpret_cast<uint32_t*>(L.pref + ((W + 1) & ~1));
    L.cur = L.hist + kBins;
    L.nxt = L.cur + 64 * W;

    for (int i = (int)blockIdx.y * kRows + wave; i < n; i += (int)gridDim.y * kRows) {
        const int64_t gi = n0 + i;
        for (int j = lane; j < nW * 64; j += kWave) { L.cur[j] = 0; L.nxt[j] = 0; }
        if (lane < nW) { L.reach[lane] = 0; L.anyw[lane] = 0; }
        if (FILL && lane < nW) L.afw[lane] = p.any[(size_t)gi * W + lane];
        wave_sync();
        {   // W_1 = the out-row of i with its duplicates; fill: the summed types of the 1-hop edges beside it
            int64_t s;
            const int c = out_row(p, n0, i, &s);
            for (int q = lane; q < c; q += kWave) {
                const uint32_t v = (uint32_t)p.o_dst[s + q];
                if (v >= (uint32_t)n) continue;
                atomicAdd(&L.cur[v], 1u);
                if (FILL) {
                    const int t = p.m_typ[s + q];
                    if (t) L.nxt[v] = (uint32_t)t;              // (one edge of a run of duplicates carries the sum)
                }
            }
        }
        bool rowok = false;
        int64_t off = 0;
        if (FILL) {
            int d = 0;
            for (int w = 0; w < nW; ++w) {
                if (lane == 0) L.pref[w] = d;
                d += __builtin_popcountll(L.afw[w]);
            }
            off = p.node_off[gi];
            rowok = off >= 0 && off + d <= p.E_out;             // a scan that does not fit the outputs: no edge of this row is written
            if (lane == 0 && p.o_batch) p.o_batch[gi] = g;
            if (p.o_pe && lane < K - 1) p.o_pe[gi * (K - 1) + lane] = 0;
        }
        wave_sync();
        if (FILL && rowok)
            for (int w = 0; w < nW; ++w) {
                const uint64_t af = L.afw[w];
                if ((af >> lane) & 1) {
                    const int64_t e = off + L.pref[w] + __builtin_popcountll(af & below(lane));
                    p.o_ei[e] = gi;
                    p.o_ei[p.E_out + e] = n0 + w * 64 + lane;
                    p.o_ea[e * K] = L.nxt[w * 64 + lane];       // column 0: the 1-hop edge's summed type, or 0
                }
            }
        wave_sync();

        uint32_t* cur = L.cur;
        uint32_t* nxt = L.nxt;
        bool range = false;
        for (int k = 0; k < K; ++k) {
            if (k > 0) {
                for (int j = lane; j < n; j += kWave) {
                    const int64_t s = p.in_start[n0 + j], c = p.in_cnt[n0 + j];
                    uint64_t acc = 0;
                    if (s >= 0 && c >= 0 && s + c <= p.E_in)
                        for (int64_t q = s; q < s + c; ++q) {
                            const uint32_t u = (uint32_t)p.in_src[q];
                            if (u < (uint32_t)n) acc += cur[u];
                        }
                    nxt[j] = acc > kSat ? kSat : (uint32_t)acc;
                }
                wave_sync();
                uint32_t* t = cur; cur = nxt; nxt = t;
            }
            for (int w = 0; w < nW; ++w) {
                const int j = w * 64 + lane;
                const uint32_t cnt = j < n ? cur[j] : 0;
                const bool pos = cnt != 0 && j != i;
                const uint64_t posw = __ballot(pos);
                if (__ballot(pos && cnt >= kInt32Limit)) range = true;
                const uint64_t hop = (!p.gd && k > 0) ? posw & ~L.reach[w] : posw;
                if (FILL && rowok && k > 0) {
                    const uint64_t af = L.afw[w];
                    if ((af >> lane) & 1) {
                        const int64_t e = off + L.pref[w] + __builtin_popcountll(af & below(lane));
                        const uint32_t code = cnt < (uint32_t)p.max_attr ? cnt : (uint32_t)p.max_attr;
                        p.o_ea[e * K + k] = ((hop >> lane) & 1) ? (int64_t)code + 1 : 0;
                    }
                }
                wave_sync();                                    // (every lane has read reach[w])
                if (lane == 0) {
                    L.reach[w] |= hop;
                    L.anyw[w] |= hop;
                    L.hs[(size_t)k * W + w] = hop;
                }
            }
            wave_sync();
            if (range) break;
        }
        if (!FILL) {
            if (range) {
                if (lane == 0) p.status[g] = KPGNN_KHOP_RANGE;  // (large_finish then clears the graph's degrees)
            } else {
                int d = 0;
                for (int w = 0; w < nW; ++w) d += __builtin_popcountll(L.anyw[w]);
                if (lane < nW) p.any[(size_t)gi * W + lane] = L.anyw[lane];
                if (lane == 0) p.deg[gi] = d;
            }
        } else if (p.H > 0 && p.T > 0 && p.o_pea && p.o_pca && !range) {
            for (int k = 0; k < K; ++k) {
                const int64_t at = gi * K + k;
                peripheral_item(p, L, n0, n, nW, L.hs + (size_t)k * W, lane, p.o_pea + at * p.T * 2, p.o_pca + at * (p.H + 1));
                wave_sync();
            }
        }
        wave_sync();
    }
}

size_t ws_bytes(int64_t N, int64_t E_in, int max_nodes) {
    const size_t W = (size_t)words_of(max_nodes);
    return (size_t)N * 8 + 2 * (size_t)N * W * 8 + 4 * (size_t)N * 4 + 6 * (size_t)E_in * 4;
}

int validate(const kpgnn_khop_dev_desc* d, const char* who, bool fill, bool* empty) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->G >= 0 && d->n_ids >= 0 && d->N >= 0 && d->E_in >= 0 && d->E_in < ((int64_t)1 << 31),
                  "%s: bad G=%d n_ids=%d N=%lld E_in=%lld", who, d->G, d->n_ids, (long long)d->N, (long long)d->E_in);
    KPGNN_REQUIRE(d->K >= 1 && d->max_edge_attr_num >= 0 && d->max_hop_num >= 0 && d->max_edge_type >= 0 && d->max_edge_count >= 0 &&
                      d->max_distance_count >= 0,
                  "%s: bad args (K=%d max_edge_attr_num=%d max_hop_num=%d max_edge_type=%d)", who, d->K, d->max_edge_attr_num,
                  d->max_hop_num, d->max_edge_type);
    KPGNN_REQUIRE(d->kernel == 0 || d->kernel == 1, "%s: unknown kernel id %d (0 = spd, 1 = gd)", who, d->kernel);
    *empty = d->G == 0 || d->n_ids == 0;
    if (*empty) return KPGNN_OK;
    KPGNN_REQUIRE(d->node_ptr && d->edge_ptr && d->graph_ids && d->status && d->workspace,
                  "%s: NULL node_ptr/edge_ptr/graph_ids/status/workspace", who);
    KPGNN_REQUIRE(d->E_in == 0 || d->edge_index, "%s: NULL edge_index", who);
    KPGNN_REQUIRE(d->max_nodes >= 1, "%s: bad max_nodes=%d", who, d->max_nodes);
    if (d->max_nodes > kCap) return fail(KPGNN_ELIMIT, "%s: max_nodes=%d is beyond the cap of %d nodes per graph", who, d->max_nodes, kCap);
    const size_t need = ws_bytes(d->N, d->E_in, d->max_nodes);
    KPGNN_REQUIRE(((uintptr_t)d->workspace & 7) == 0 && d->workspace_bytes >= need,
                  "%s: workspace of %zu bytes (need %zu, 8-byte aligned)", who, d->workspace_bytes, need);
    if (fill) {
        const bool periph = d->max_hop_num > 0 && d->max_edge_type > 0;
        KPGNN_REQUIRE(d->E_out >= 0, "%s: bad E_out=%lld", who, (long long)d->E_out);
        KPGNN_REQUIRE(d->N == 0 || d->node_off, "%s: NULL node_off", who);
        KPGNN_REQUIRE(d->E_out == 0 || (d->out_edge_index && d->out_edge_attr), "%s: NULL out_edge_index/out_edge_attr", who);
        KPGNN_REQUIRE(!periph || d->N == 0 || (d->out_pea && d->out_pca), "%s: NULL out_pea/out_pca", who);
    }
    return KPGNN_OK;
}

template <bool FILL>
int launch(const kpgnn_khop_dev_desc* d, hipStream_t s, const char* who) {
    bool empty = false;
    const int rc = validate(d, who, FILL, &empty);
    if (rc != KPGNN_OK || empty) return rc;
    LargeParams p = {};
    p.G = d->G; p.n_ids = d->n_ids; p.cap = d->max_nodes; p.W = words_of(d->max_nodes);
    p.N = d->N; p.E_in = d->E_in; p.E_out = d->E_out; p.ids = d->graph_ids;
    p.node_ptr = d->node_ptr; p.edge_ptr = d->edge_ptr; p.ei = d->edge_index; p.ea = d->edge_attr;
    p.K = d->K; p.max_attr = d->max_edge_attr_num; p.H = d->max_hop_num; p.T = d->max_edge_type;
    p.max_edge_count = d->max_edge_count; p.max_dist_count = d->max_distance_count; p.gd = d->kernel;
    const size_t NW = (size_t)d->N * p.W;
    p.deg = static_cast<int64_t*>(d->workspace);
    p.any = reinterpret_cast<uint64_t*>(p.deg + d->N);
    p.nzt = p.any + NW;
    p.in_start = reinterpret_cast<int32_t*>(p.nzt + NW);
    p.in_cnt = p.in_start + d->N;
    p.out_start = p.in_cnt + d->N;
    p.out_cnt = p.out_start + d->N;
    p.in_src = p.out_cnt + d->N;
    p.s_dst = p.in_src + d->E_in;
    p.m_typ = p.s_dst + d->E_in;
    p.o_src = p.m_typ + d->E_in;
    p.o_dst = p.o_src + d->E_in;
    p.o_typ = p.o_dst + d->E_in;
    p.status = d->status;
    p.node_off = d->node_off;
    p.o_ei = d->out_edge_index; p.o_ea = d->out_edge_attr; p.o_pe = d->out_pe_attr; p.o_pea = d->out_pea; p.o_pca = d->out_pca;
    p.o_batch = d->out_batch;
    const int Klds = d->K > kMaxK ? 1 : d->K;       // (K beyond the kernel: every graph gets SHAPE and no row is walked)
    if (d->K > kMaxK) p.K = kMaxK + 1;
    const size_t lds = kRows * wave_bytes(p.W, Klds);
    int gy = (d->max_nodes + kRows - 1) / kRows;
    gy = gy > kMaxRowBlocks ? kMaxRowBlocks : gy;
    const dim3 graphs((unsigned)d->n_ids), rows((unsigned)d->n_ids, (unsigned)gy);
    KPGNN_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&large_walk<FILL>), lds));
    if (!FILL) {
        hipLaunchKernelGGL(large_prep, graphs, dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("large_prep");
    }
    hipLaunchKernelGGL((large_walk<FILL>), rows, dim3(kBlock), lds, s, p);
    KPGNN_LAUNCH_CHECK("large_walk");
    if (!FILL) {
        hipLaunchKernelGGL(large_finish, graphs, dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("large_finish");
    }
    return KPGNN_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" size_t kpgnn_khop_large_workspace_bytes(int64_t N, int64_t E_in, int32_t max_nodes) {
    return (N < 0 || E_in < 0 || max_nodes < 1) ? 0 : ws_bytes(N, E_in, max_nodes);
}

extern "C" int kpgnn_khop_large_count(const kpgnn_khop_dev_desc* d, kpgnn_stream_t stream) {
    return launch<false>(d, (hipStream_t)stream, "kpgnn_khop_large_count");
}

extern "C" int kpgnn_khop_large_fill(const kpgnn_khop_dev_desc* d, kpgnn_stream_t stream) {
    return launch<true>(d, (hipStream_t)stream, "kpgnn_khop_large_fill");
}
