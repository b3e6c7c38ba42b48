// Uniform random simple d-regular graphs by the pairing model with rejection (gfx950).  Contract and the definition of the
// draw: include/kpgnn.h, kpgnn_random_regular_graphs.
//
// The reference's simulation (run_simulation.py:119-129) asks networkx for one graph at a time on the host (Steger-Wormald:
// uniform only asymptotically, and four fifths of the experiment's time once everything behind it runs on the device,
// DESIGN.md 5.31).  Here one team - a wavefront, or a block - owns one graph for its whole rejection loop:
//   1. one Philox4x32-10 call per PAIR of stubs (counter: stub >> 1, attempt, graph id) gives each stub its 64-bit word; the
//      key keeps the word's upper 51 bits above the 13-bit stub index, so all keys differ;
//   2. a bitonic network sorts the keys in LDS, P / 2 compare-exchanges per step over log2 P (log2 P + 1) / 2 steps; the
//      all-ones keys that pad m up to the power of two P are larger than every key of a stub (one that has the index 8191 has
//      no padding beside it) and end behind them;
//   3. the stubs at the sorted positions 2 i and 2 i + 1 become partners: a table of 16-bit stub indices in LDS;
//   4. a thread per node reads its d partners' nodes and looks for itself (a self loop) or a repeat (a double edge); the
//      team votes - a ballot in a wavefront, a block-wide OR otherwise - and a rejected pairing starts over at 1 with the
//      next attempt number;
//   5. the accepted graph: a thread per node orders its d <= 4 neighbours in registers and stores the d directed edges.
// Every decision is a function of the sorted ORDER, which is total, so the graph does not depend on the network, on the team's
// width or on the other graphs of the launch.  Integer arithmetic only; no atomics; no global memory but the outputs.
// A step's two LDS accesses per lane are 8-byte ones at a stride of j keys: for j >= 32 a wavefront's lanes touch consecutive
// keys, below that the lanes of a group fall 2 j keys apart in pairs - a 2-way conflict at worst on the 64-bank 8-byte read.
// The block class takes P / 2 threads, one compare-exchange each per step, at least 256 and at most 1024 (four exchanges a
// step at P = 8192): a rejection loop is a chain of ~log^2 P barriers, so a graph wants its step short.  The 2048
// threads of a CU hold two such blocks and so does its LDS (8 P + 2 m bytes and the vote's 256 static ones a block) up to
// m = 8064; the last step to the limit, 80 KiB, leaves room for one.  22 VGPRs (35 in the wavefront class, 10 KiB of static LDS a block), no scratch.
#include "kpgnn_common.h"
#include "philox.h"

namespace kpgnn {
namespace {

constexpr int kWaveBlock = 256;                     // the wavefront class: four graphs per block
constexpr int kMinBlock = 256, kMaxBlock = 1024;    // the block class: P / 2 threads within these
constexpr int kWaveStubs = KPGNN_RRG_WAVE_STUBS;
constexpr int kMaxStubs = KPGNN_RRG_MAX_STUBS;
constexpr int kMaxDegree = KPGNN_RRG_MAX_DEGREE;
typedef unsigned long long u64;
constexpr u64 kIndexMask = (u64)kMaxStubs - 1;      // the 13 index bits of a key
static_assert((kMaxStubs & (kMaxStubs - 1)) == 0 && (kWaveStubs & (kWaveStubs - 1)) == 0, "the bounds are powers of two");
static_assert(kMaxDegree == 4, "the row sort below is a network over four values");

struct RrgParams {
    int G, n, d, m, P, max_attempts;
    uint32_t k0, k1;
    u64 first;
    int64_t* ei; int32_t* attempts; int32_t* status;
};

constexpr size_t lds_bytes(int P, int m) { return (size_t)P * 8 + (size_t)m * 2; }
static_assert(lds_bytes(kMaxStubs, kMaxStubs) + 256 <= 160 * 1024, "the largest graph fits the LDS of a CU");

__device__ __forceinline__ int node_of(int stub, int d) {       // stub / d, d in 1 .. 4, without an integer division
    return d == 3 ? (int)((unsigned)stub / 3u) : d == 4 ? stub >> 2 : d == 2 ? stub >> 1 : stub;
}

// the nodes at the other end of node u's d stubs; the slots from d on hold distinct values above every node
__device__ __forceinline__ void neighbours(const uint16_t* part, int u, int d, int (&v)[kMaxDegree]) {
#pragma unroll
    for (int j = 0; j < kMaxDegree; ++j) v[j] = j < d ? node_of(part[u * d + j], d) : kMaxStubs + j;
}

__device__ __forceinline__ void order(int& a, int& b) { const int lo = a < b ? a : b, hi = a < b ? b : a; a = lo; b = hi; }

template <bool WAVE>
__global__ void __launch_bounds__(WAVE ? kWaveBlock : kMaxBlock) rrg_kernel(const RrgParams p) {
    const int T = WAVE ? kWave : (int)blockDim.x;
    const int team = WAVE ? (int)threadIdx.x / kWave : 0;
    const int tid = WAVE ? (int)threadIdx.x % kWave : (int)threadIdx.x;
    const int64_t g = WAVE ? (int64_t)blockIdx.x * (kWaveBlock / kWave) + team : (int64_t)blockIdx.x;
    if (g >= p.G) return;                           // (a whole team: nobody waits for it below)
    u64* keys;
    uint16_t* part;
    if constexpr (WAVE) {
        __shared__ u64 wave_keys[kWaveBlock / kWave][kWaveStubs];
        __shared__ uint16_t wave_part[kWaveBlock / kWave][kWaveStubs];
        keys = wave_keys[team];
        part = wave_part[team];
    } else {
        extern __shared__ __attribute__((aligned(16))) u64 rrg_lds[];
        keys = rrg_lds;
        part = reinterpret_cast<uint16_t*>(rrg_lds + p.P);
    }
    const int n = p.n, d = p.d, m = p.m, P = p.P, half = P >> 1;
    const u64 id = p.first + (u64)g;
    const uint32_t id_lo = (uint32_t)id, id_hi = (uint32_t)(id >> 32);
    for (int s = m + tid; s < P; s += T) keys[s] = ~0ull;       // the padding: written once, it sorts back to [m, P)

    int a = 0;
    bool accepted = false;
    for (; a < p.max_attempts; ++a) {
        // 1. the keys of the stubs 2 q and 2 q + 1 from one call (m is even)
        for (int q = tid; 2 * q < m; q += T) {
            const Philox4 r = philox4x32_10((uint32_t)q, (uint32_t)a, id_lo, id_hi, p.k0, p.k1);
            keys[2 * q] = ((((u64)r.w[1] << 32) | r.w[0]) & ~kIndexMask) | (u64)(2 * q);
            keys[2 * q + 1] = ((((u64)r.w[3] << 32) | r.w[2]) & ~kIndexMask) | (u64)(2 * q + 1);
        }
        // 2. the bitonic network, ascending
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                team_sync<WAVE>();
                for (int t = tid; t < half; t += T) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                    const u64 x = keys[i], y = keys[l];
                    if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[l] = x; }
                }
            }
        }
        team_sync<WAVE>();
        // 3. the partners (the first m sorted keys are the stubs': their index bits are below m)
        for (int i = tid; 2 * i < m; i += T) {
            const int s0 = (int)(keys[2 * i] & kIndexMask), s1 = (int)(keys[2 * i + 1] & kIndexMask);
            part[s0] = (uint16_t)s1;
            part[s1] = (uint16_t)s0;
        }
        team_sync<WAVE>();
        // 4. the two checks and the vote
        bool bad = false;
        for (int u = tid; u < n; u += T) {
            int v[kMaxDegree];
            neighbours(part, u, d, v);
#pragma unroll
            for (int j = 0; j < kMaxDegree; ++j) {
                bad |= v[j] == u;
#pragma unroll
                for (int l = j + 1; l < kMaxDegree; ++l) bad |= v[j] == v[l];
            }
        }
        bool rejected;
        if constexpr (WAVE) {
            rejected = __ballot(bad) != 0ull;
            team_sync<WAVE>();
        } else {
            rejected = __syncthreads_or(bad) != 0;      // (also: every read of the table is done before the next keys)
        }
        if (!rejected) { accepted = true; break; }
    }

    // 5. the rows of the accepted graph
    if (accepted) {
        const int64_t cols = (int64_t)p.G * m;
        for (int u = tid; u < n; u += T) {
            int v[kMaxDegree];
            neighbours(part, u, d, v);
            order(v[0], v[1]); order(v[2], v[3]); order(v[0], v[2]); order(v[1], v[3]); order(v[1], v[2]);
            int64_t* row = p.ei + g * m + (int64_t)u * d;
#pragma unroll
            for (int j = 0; j < kMaxDegree; ++j)
                if (j < d) { row[j] = u; row[cols + j] = v[j]; }
        }
    }
    if (tid == 0) {
        p.attempts[g] = accepted ? a + 1 : p.max_attempts;
        p.status[g] = accepted ? KPGNN_RRG_OK : KPGNN_RRG_EXHAUSTED;
    }
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_random_regular_graphs(const kpgnn_rrg_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_random_regular_graphs";
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->G >= 0 && d->n >= 1 && d->d >= 1 && d->max_attempts >= 1 && d->first_graph >= 0,
                  "%s: bad G=%d n=%d d=%d max_attempts=%d first_graph=%lld", who, d->G, d->n, d->d, d->max_attempts, (long long)d->first_graph);
    KPGNN_REQUIRE(d->d < d->n, "%s: no simple %d-regular graph on n=%d nodes (d >= n)", who, d->d, d->n);
    KPGNN_REQUIRE((((int64_t)d->n * d->d) & 1) == 0, "%s: n * d = %d * %d is odd", who, d->n, d->d);
    if (d->d > kMaxDegree) return fail(KPGNN_ELIMIT, "%s: d=%d is beyond the degree limit of %d", who, d->d, kMaxDegree);
    if (d->n > KPGNN_RRG_MAX_NODES || (int64_t)d->n * d->d > kMaxStubs)
        return fail(KPGNN_ELIMIT, "%s: n=%d d=%d is beyond the limits of %d nodes and %d stubs", who, d->n, d->d, KPGNN_RRG_MAX_NODES, kMaxStubs);
    if (d->G == 0) return KPGNN_OK;
    KPGNN_REQUIRE(d->edge_index && d->attempts && d->status, "%s: NULL edge_index/attempts/status", who);
    RrgParams p = {};
    p.G = d->G; p.n = d->n; p.d = d->d; p.m = d->n * d->d; p.max_attempts = d->max_attempts;
    p.P = 2;
    while (p.P < p.m) p.P <<= 1;
    p.k0 = (uint32_t)(uint64_t)d->seed; p.k1 = (uint32_t)((uint64_t)d->seed >> 32);
    p.first = (u64)d->first_graph;
    p.ei = d->edge_index; p.attempts = d->attempts; p.status = d->status;
    hipStream_t s = (hipStream_t)stream;
    if (p.m <= kWaveStubs) {
        constexpr int per = kWaveBlock / kWave;
        hipLaunchKernelGGL((rrg_kernel<true>), dim3((unsigned)((d->G + per - 1) / per)), dim3(kWaveBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("rrg_kernel<wave>");
    } else {
        const int half = p.P / 2, threads = half < kMinBlock ? kMinBlock : half > kMaxBlock ? kMaxBlock : half;
        const size_t lds = lds_bytes(p.P, p.m);
        KPGNN_HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&rrg_kernel<false>), lds));
        hipLaunchKernelGGL((rrg_kernel<false>), dim3((unsigned)d->G), dim3(threads), lds, s, p);
        KPGNN_LAUNCH_CHECK("rrg_kernel<block>");
    }
    return KPGNN_OK;
}
