// The K-hop pre-transform, batched over graphs (gfx950).  Contract: include/kpgnn.h, kpgnn_khop_dev_desc.
//
// A device restatement of transform_graph / peripheral_stats of khop_host.cpp, which is the specification.
// One team owns one graph - a wavefront for n <= 32 (four graphs per 256-thread block, wave-level synchronisation only), a
// block for n <= 64 - and runs the same walk in both passes:
//   1. mult[i][j] / type[i][j] in LDS by LDS integer atomics (duplicates add; independent of the edge order); an endpoint
//      outside the graph, a negative type or a summed type above 63 end the graph with a status;
//   2. W_1 = mult, W_{k+1} = W_k mult as dense n x n products of uint32 counts saturating at 2^32 - 1 (kpgnn.h says why that
//      equals the host's 2^40), diagonal kept for the recurrence;
//   3. after every product thread i owns row i: its hop set as ONE 64-bit word (count > 0, j != i, spd: not reached before),
//      the reached and any-hop words in registers; an off-diagonal count >= 2^31 ends the graph with RANGE.
// The count pass leaves any[i] and popcount(any[i]) in the workspace.  The fill pass reads the caller's scan of the degrees,
// zeroes row i's slice of edge_attr, writes each edge at node_off[i] + popcount(any[i] & below(j)), the codes of hop k as the
// hop is emitted, and then the peripheral statistics with one thread per (node, hop): S is the hop word, the induced edges of
// u are nzt[u] & S (nzt: the non-zero-type word of a row), a BFS level is an OR of nzt rows masked by S & ~reach, the
// edge-type histogram is 64 uint16 bins per thread in LDS, bin-major (lane-consecutive), aliased over the two count matrices
// that nobody reads any more; the stable descending sort is T rounds of "largest count, lowest type".
// LDS per team of cap nodes: mult + type 2 * cap * (cap|1) * 4, the two count matrices (or the histograms, whichever is
// larger) max(2 * cap * (cap|1) * 4, 128 * threads), hop words cap * K * 8, nzt cap * 8, 16 of flags:
// 75,280 bytes at cap = 64, K = 16 (block), 21,264 at cap = 32, K = 16 (wavefront).  Rows have an ODD stride (n | 1 words), so
// thread-per-row walks stay off one bank.  No global atomics, no float; every global write of the fill pass is range-checked.
#include "kpgnn_common.h"

namespace kpgnn {
namespace {

constexpr int kBlock = 256;
constexpr int kWaveCap = KPGNN_KHOP_WAVE_NODES;
constexpr int kMaxCap = KPGNN_KHOP_MAX_NODES;
constexpr int kMaxType = KPGNN_KHOP_MAX_TYPE;
constexpr int kMaxK = KPGNN_KHOP_MAX_K, kMaxT = KPGNN_KHOP_MAX_T, kMaxH = KPGNN_KHOP_MAX_H;
constexpr int kBins = kMaxType + 1;
constexpr uint32_t kSat = 0xFFFFFFFFu;
constexpr uint32_t kInt32Limit = 0x80000000u;
constexpr uint16_t kTaken = 0xFFFFu;          // a histogram bin the sort has handed out (counts are <= 64 * 64)

struct KhopParams {
    int G, n_ids, cap;
    int64_t N, E_in, E_out;
    const int32_t* ids;
    const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* ei; const int64_t* ea;
    int K, max_attr, H, T, max_edge_count, max_dist_count, gd;
    uint64_t* any; int64_t* deg; int32_t* status;
    const int64_t* node_off;
    int64_t* o_ei; int64_t* o_ea; int64_t* o_pe; int64_t* o_pea; int64_t* o_pca; int64_t* o_batch;
};

__host__ __device__ constexpr size_t mat_words(int cap) { return (size_t)cap * (cap | 1); }
__host__ __device__ constexpr size_t w_bytes(int cap, int threads) {
    return 2 * mat_words(cap) * 4 > (size_t)threads * kBins * 2 ? 2 * mat_words(cap) * 4 : (size_t)threads * kBins * 2;
}
// (8-byte multiples throughout: the hop words follow the matrices)
__host__ __device__ constexpr size_t team_bytes(int cap, int K, int threads) {
    return ((2 * mat_words(cap) * 4 + w_bytes(cap, threads) + 7) & ~(size_t)7) + (size_t)cap * K * 8 + (size_t)cap * 8 + 16;
}

__device__ __forceinline__ uint64_t below(int j) { return ((uint64_t)1 << j) - 1; }     // j in [0, 63]

// Peripheral statistics of the subgraph induced on S, the hop word of (node, hop): peripheral_stats of khop_host.cpp.
__device__ void peripheral_item(const KhopParams& p, int s, const int* type, const uint64_t* nzt, uint64_t S, uint16_t* hist,
                                int hstride, int64_t* pe_out, int64_t* pc_out) {
    const int T = p.T, H = p.H;
    for (int t = 0; t < 2 * T; ++t) pe_out[t] = 0;
    for (int h = 0; h <= H; ++h) pc_out[h] = 0;
    if (__builtin_popcountll(S) < 2) return;
    for (int b = 0; b < kBins; ++b) hist[b * hstride] = 0;
    int n_edges = 0;
    for (uint64_t us = S; us; us &= us - 1) {
        const int u = __ffsll((long long)us) - 1;
        for (uint64_t vs = nzt[u] & S; vs; vs &= vs - 1) {
            const int v = __ffsll((long long)vs) - 1;
            hist[type[u * s + v] * hstride] += 1;           // (a summed type is <= 63: checked before the walk)
            ++n_edges;
        }
    }
    if (n_edges == 0) return;
    for (int t = 0; t < T; ++t) {       // stable descending: the largest count, the lowest type among equals
        int best = 0, bc = -1;
        for (int b = 2; b < kBins; ++b) {
            const uint16_t c = hist[b * hstride];
            if (c != kTaken && (int)c > bc) { bc = c; best = b; }
        }
        hist[best * hstride] = kTaken;
        pe_out[2 * t] = best - 2;                           // index into edge_count[2:], i.e. type - 2 (Q4)
        pe_out[2 * t + 1] = bc < p.max_edge_count ? bc : p.max_edge_count;
    }
    int64_t conf[kMaxH + 1];
#pragma unroll
    for (int h = 0; h <= kMaxH; ++h) conf[h] = 0;
    for (uint64_t ss = S; ss; ss &= ss - 1) {
        const int src = __ffsll((long long)ss) - 1;
        uint64_t reach = (uint64_t)1 << src, frontier = reach;
#pragma unroll
        for (int h = 1; h <= kMaxH; ++h) {
            if (h > H || !frontier) break;
            uint64_t next = 0;
            for (uint64_t us = frontier; us; us &= us - 1) next |= nzt[__ffsll((long long)us) - 1];
            next &= S & ~reach;
            reach |= next;
            frontier = next;
            const int m = __builtin_popcountll(next);
            conf[h] += m;
            if (m >= 2)                                     // sum of edge-type VALUES inside the distance class (Q5)
                for (uint64_t us = next; us; us &= us - 1) {
                    const int u = __ffsll((long long)us) - 1;
                    for (uint64_t vs = nzt[u] & next; vs; vs &= vs - 1) conf[0] += type[u * s + __ffsll((long long)vs) - 1];
                }
        }
    }
#pragma unroll
    for (int h = 0; h <= kMaxH; ++h)
        if (h <= H) pc_out[h] = conf[h] < p.max_dist_count ? conf[h] : p.max_dist_count;
}

template <bool WAVE, bool FILL>
__global__ void __launch_bounds__(kBlock) khop_kernel(const KhopParams p) {
    extern __shared__ uint64_t khop_lds[];
    constexpr int T = WAVE ? kWave : kBlock;
    const int team = WAVE ? (int)threadIdx.x / kWave : 0;
    const int tid = WAVE ? (int)threadIdx.x % kWave : (int)threadIdx.x;
    const int64_t slot = WAVE ? (int64_t)blockIdx.x * (kBlock / kWave) + team : (int64_t)blockIdx.x;
    if (slot >= p.n_ids) return;
    const int g = p.ids[slot];
    if (g < 0 || g >= p.G) return;
    const int64_t n0 = p.node_ptr[g], n64 = p.node_ptr[g + 1] - n0;
    if (n0 < 0 || n64 < 0 || n0 + n64 > p.N) {              // offsets that do not describe nodes of this call
        if (!FILL && tid == 0) p.status[g] = KPGNN_KHOP_ENDPOINT;
        return;
    }
    if (FILL) {
        if (p.status[g] != KPGNN_KHOP_OK || n64 > p.cap) return;
    } else {
        int st = KPGNN_KHOP_OK;
        if (p.K > kMaxK || p.T > kMaxT || p.H > kMaxH) st = KPGNN_KHOP_SHAPE;
        else if (n64 > p.cap) st = KPGNN_KHOP_TOO_LARGE;
        if (st != KPGNN_KHOP_OK || n64 == 0) {
            for (int64_t i = tid; i < n64; i += T) { p.any[n0 + i] = 0; p.deg[n0 + i] = 0; }
            if (tid == 0) p.status[g] = st;
            return;
        }
    }
    if (n64 == 0) return;
    const int n = (int)n64, s = n | 1, K = p.K;
    int64_t e0 = p.edge_ptr[g], e1 = p.edge_ptr[g + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > p.E_in ? p.E_in : e1;

    char* base = reinterpret_cast<char*>(khop_lds) + (size_t)team * team_bytes(p.cap, K, T);
    int* mult = reinterpret_cast<int*>(base);
    int* type = mult + mat_words(p.cap);
    uint32_t* Wa = reinterpret_cast<uint32_t*>(type + mat_words(p.cap));
    uint32_t* Wb = Wa + mat_words(p.cap);
    uint16_t* hist = reinterpret_cast<uint16_t*>(Wa);       // after the last product
    uint64_t* hs = reinterpret_cast<uint64_t*>(base + ((2 * mat_words(p.cap) * 4 + w_bytes(p.cap, T) + 7) & ~(size_t)7));
    uint64_t* nzt = hs + (size_t)p.cap * K;
    int* flags = reinterpret_cast<int*>(nzt + p.cap);       // [0] endpoint, [1] type, [2] range

    // 1. adjacency
    for (int q = tid; q < n * s; q += T) { mult[q] = 0; type[q] = 0; }
    if (tid < 3) flags[tid] = 0;
    team_sync<WAVE>();
    for (int64_t e = e0 + tid; e < e1; e += T) {
        const int64_t u = p.ei[e], v = p.ei[p.E_in + e], t = p.ea ? p.ea[e] : 2;
        if (u < 0 || u >= n || v < 0 || v >= n) flags[0] = 1;
        else if (t < 0 || t > kMaxType) flags[1] = 1;
        else {
            atomicAdd(&mult[(int)u * s + (int)v], 1);
            atomicAdd(&type[(int)u * s + (int)v], (int)t);
        }
    }
    team_sync<WAVE>();
    for (int q = tid; q < n * n; q += T) {
        const int i = q / n, j = q - i * n;
        if (type[i * s + j] > kMaxType) flags[1] = 1;
        Wa[i * s + j] = (uint32_t)mult[i * s + j];
    }
    if (tid < n) {
        uint64_t w = 0;
        for (int j = 0; j < n; ++j) w |= (uint64_t)(type[tid * s + j] != 0) << j;
        nzt[tid] = w;
    }
    team_sync<WAVE>();
    if (flags[0] || flags[1]) {
        if (!FILL) {
            for (int i = tid; i < n; i += T) { p.any[n0 + i] = 0; p.deg[n0 + i] = 0; }
            if (tid == 0) p.status[g] = flags[0] ? KPGNN_KHOP_ENDPOINT : KPGNN_KHOP_TYPE;
        }
        return;
    }

    // the row this thread owns (n <= T): its words live in registers across the hops
    const bool row = tid < n;
    uint64_t reached = 0, any = 0, any_final = 0;
    int64_t off = 0;
    if (FILL && row) {
        any_final = p.any[n0 + tid];
        off = p.node_off[n0 + tid];
        const int d = __builtin_popcountll(any_final);
        if (off < 0 || off + d > p.E_out) any_final = 0;    // a scan that does not fit the outputs: write nothing for this row
        else {
            for (int r = 0; r < d * K; ++r) p.o_ea[off * K + r] = 0;
            int r = 0;
            for (uint64_t js = any_final; js; js &= js - 1, ++r) {
                const int j = __ffsll((long long)js) - 1;
                p.o_ei[off + r] = n0 + tid;
                p.o_ei[p.E_out + off + r] = n0 + j;
                if (mult[tid * s + j] > 0) p.o_ea[(off + r) * K] = type[tid * s + j];      // column 0: the 1-hop edge's type
            }
        }
        if (p.o_batch) p.o_batch[n0 + tid] = g;
        if (p.o_pe)
            for (int k = 0; k + 1 < K; ++k) p.o_pe[(n0 + tid) * (K - 1) + k] = 0;
    }

    // 2. / 3. hops
    uint32_t* cur = Wa;
    uint32_t* nxt = Wb;
    for (int k = 0; k < K; ++k) {
        if (k > 0) {
            for (int q = tid; q < n * n; q += T) {
                const int i = q / n, j = q - i * n;
                uint64_t acc = 0;
                for (int m = 0; m < n; ++m) {
                    const uint32_t a = cur[i * s + m];
                    if (a) {
                        const uint64_t pr = (uint64_t)a * (uint32_t)mult[m * s + j];
                        acc += pr > kSat ? kSat : pr;
                    }
                }
                nxt[i * s + j] = acc > kSat ? kSat : (uint32_t)acc;
            }
            team_sync<WAVE>();
            uint32_t* t = cur; cur = nxt; nxt = t;
        }
        if (row) {
            uint64_t pos = 0;
            bool big = false;
            for (int j = 0; j < n; ++j) {
                const uint32_t w = cur[tid * s + j];
                if (j != tid && w) {
                    pos |= (uint64_t)1 << j;
                    big |= w >= kInt32Limit;
                }
            }
            if (big) flags[2] = 1;
            const uint64_t hop = (!p.gd && k > 0) ? pos & ~reached : pos;
            reached |= hop;
            any |= hop;
            hs[tid * K + k] = hop;
            if (FILL && k > 0)
                for (uint64_t js = hop & any_final; js; js &= js - 1) {
                    const int j = __ffsll((long long)js) - 1;
                    const uint32_t w = cur[tid * s + j];
                    const int64_t e = off + __builtin_popcountll(any_final & below(j));
                    p.o_ea[e * K + k] = (int64_t)(w < (uint32_t)p.max_attr ? w : (uint32_t)p.max_attr) + 1;
                }
        }
        team_sync<WAVE>();          // (the next product overwrites the matrix this emit read)
        if (flags[2]) break;
    }
    if (!FILL) {
        const bool bad = flags[2] != 0;
        if (row) {
            p.any[n0 + tid] = bad ? 0 : any;
            p.deg[n0 + tid] = bad ? 0 : __builtin_popcountll(any);
        }
        if (tid == 0) p.status[g] = bad ? KPGNN_KHOP_RANGE : KPGNN_KHOP_OK;
        return;
    }
    // peripheral statistics, one thread per (node, hop); the histograms lie over the count matrices
    if (p.H > 0 && p.T > 0 && p.o_pea && p.o_pca && !flags[2])
        for (int it = tid; it < n * K; it += T) {
            const int64_t at = (n0 + it / K) * K + it % K;
            peripheral_item(p, s, type, nzt, hs[it], hist + tid, T, p.o_pea + at * p.T * 2, p.o_pca + at * (p.H + 1));
        }
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
    KPGNN_REQUIRE(((uintptr_t)d->workspace & 7) == 0 && d->workspace_bytes >= kpgnn_khop_dev_workspace_bytes(d->N),
                  "%s: workspace of %zu bytes (need %zu, 8-byte aligned)", who, d->workspace_bytes, kpgnn_khop_dev_workspace_bytes(d->N));
    KPGNN_REQUIRE(d->max_nodes >= 1, "%s: bad max_nodes=%d", who, d->max_nodes);
    if (d->max_nodes > kMaxCap) return fail(KPGNN_ELIMIT, "%s: max_nodes=%d is beyond the cap of %d nodes per graph", who, d->max_nodes, kMaxCap);
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
    KhopParams p = {};
    p.G = d->G; p.n_ids = d->n_ids; p.N = d->N; p.E_in = d->E_in; p.E_out = d->E_out; p.ids = d->graph_ids;
    p.node_ptr = d->node_ptr; p.edge_ptr = d->edge_ptr; p.ei = d->edge_index; p.ea = d->edge_attr;
    p.K = d->K; p.max_attr = d->max_edge_attr_num; p.H = d->max_hop_num; p.T = d->max_edge_type;
    p.max_edge_count = d->max_edge_count; p.max_dist_count = d->max_distance_count; p.gd = d->kernel;
    p.any = static_cast<uint64_t*>(d->workspace); p.deg = static_cast<int64_t*>(d->workspace) + d->N; p.status = d->status;
    p.node_off = d->node_off;
    p.o_ei = d->out_edge_index; p.o_ea = d->out_edge_attr; p.o_pe = d->out_pe_attr; p.o_pea = d->out_pea; p.o_pca = d->out_pca;
    p.o_batch = d->out_batch;
    const int Klds = d->K > kMaxK ? 1 : d->K;       // (K beyond the kernel: every graph gets SHAPE before LDS is touched)
    if (d->K > kMaxK) p.K = kMaxK + 1;
    if (d->max_nodes <= kWaveCap) {
        p.cap = kWaveCap;
        constexpr int per = kBlock / kWave;
        const size_t lds = per * team_bytes(kWaveCap, Klds, kWave);
        KPGNN_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&khop_kernel<true, FILL>), lds));
        hipLaunchKernelGGL((khop_kernel<true, FILL>), dim3((unsigned)((d->n_ids + per - 1) / per)), dim3(kBlock), lds, s, p);
        KPGNN_LAUNCH_CHECK("khop_kernel<wave>");
    } else {
        p.cap = d->max_nodes;
        const size_t lds = team_bytes(p.cap, Klds, kBlock);
        KPGNN_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&khop_kernel<false, FILL>), lds));
        hipLaunchKernelGGL((khop_kernel<false, FILL>), dim3((unsigned)d->n_ids), dim3(kBlock), lds, s, p);
        KPGNN_LAUNCH_CHECK("khop_kernel<block>");
    }
    return KPGNN_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" size_t kpgnn_khop_dev_workspace_bytes(int64_t N) { return N < 0 ? 0 : (size_t)N * 16; }

extern "C" int kpgnn_khop_dev_count(const kpgnn_khop_dev_desc* d, kpgnn_stream_t stream) {
    return launch<false>(d, (hipStream_t)stream, "kpgnn_khop_dev_count");
}

extern "C" int kpgnn_khop_dev_fill(const kpgnn_khop_dev_desc* d, kpgnn_stream_t stream) {
    return launch<true>(d, (hipStream_t)stream, "kpgnn_khop_dev_fill");
}
