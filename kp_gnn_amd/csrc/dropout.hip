// Dropout (+ residual) with counter-based masks (gfx950).  Contract: include/kpgnn.h, kpgnn_dropout_fwd / _bwd / _mask.
//
// The bodies drop out after every layer but the last, inside the virtual-node update and after the jumping-knowledge
// projection (models/GNNs.py, the self.dropout sites; train_TU.py:276 trains with drop_prob = 0.5).  nn.Dropout is one
// framework launch per direction plus a saved [N,H] bool mask per site, the residual a further add, and its masks depend on the
// launch geometry.  Here the mask of the LOGICAL element e = row * C + col is word e & 3 of Philox4x32-10 at counter
// (e >> 2, call) under key (seed): a function of (seed, call, row, col, C) alone - the same on an exact-shape batch and on a
// capacity-shaped one - recomputed in the backward instead of stored.  One Philox call (~60 integer ops) serves the four
// elements of a 16-byte access, against 32-48 bytes of traffic: the 16-byte path stays memory-bound.  The scalar path (C not a
// multiple of 4, or rows / pointers that are not 16-byte aligned) runs the ten rounds for EVERY element, four times the
// arithmetic against 8-12 bytes: it is the correct fallback, not a tuned one, and may well be bound by the integer pipe (not
// measured).  The bodies' widths (32, 104, 120) never take it.
//
// The call id lives on the device: every block reads state[1] as it starts, block 0 leaves it in call_io for the backward, and
// the block that FINISHES last (ticket, as in adam.hip) bumps state[1] - after every other block has read it.  A replayed
// graph therefore draws a fresh mask on every replay.
#include "kpgnn_common.h"
#include "philox.h"

namespace kpgnn {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;      // 256 CUs x 8 blocks: grid-stride beyond (and at most that many ticket arrivals)

enum { OP_FWD = 0, OP_BWD = 1, OP_MASK = 2 };

struct DropParams {
    const int32_t* n_dyn;
    int64_t N; int C;
    const float* x; int64_t xs;
    float* out; int64_t os;
    const float* res; int64_t rs;
    uint8_t* mask;
    uint32_t thr; float scale;
    long long* state; long long* call_io; unsigned long long* ticket;
    long long seed, call;           // OP_MASK: given; otherwise read from state / call_io
    int flat;                       // every row stride equals C: the rows are one run of N * C elements
    int lanes_log2;                 // strided rows: 1 << lanes_log2 lanes walk a row, kBlock >> lanes_log2 rows per block
};

// VEC consecutive logical elements from e (VEC == 4: e % 4 == 0, one Philox call; VEC == 1: word e & 3 of the call of e >> 2)
template <int OP, int VEC>
__device__ __forceinline__ void drop_elems(const DropParams& p, int64_t e, int64_t xo, int64_t oo, int64_t ro,
                                           uint32_t k0, uint32_t k1, uint32_t c2, uint32_t c3) {
    const uint64_t q = (uint64_t)e >> 2;
    const Philox4 r = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), c2, c3, k0, k1);
    bool keep[VEC];
    if (VEC == 4) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) keep[j] = r.w[j] >= p.thr;
    } else {
        const int j = (int)(e & 3);
        keep[0] = (j == 0 ? r.w[0] : j == 1 ? r.w[1] : j == 2 ? r.w[2] : r.w[3]) >= p.thr;
    }
    if (OP == OP_MASK) {
        if (VEC == 4) {
            *reinterpret_cast<uint32_t*>(p.mask + e) = (uint32_t)keep[0] | ((uint32_t)keep[1 % VEC] << 8) |
                                                       ((uint32_t)keep[2 % VEC] << 16) | ((uint32_t)keep[3 % VEC] << 24);
        } else {
            p.mask[e] = (uint8_t)keep[0];
        }
        return;
    }
    float v[VEC], o[VEC];
    ldv<VEC>(p.x + xo, v);
    if (OP == OP_FWD && p.res) {
        float w[VEC];
        ldv<VEC>(p.res + ro, w);
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = keep[j] ? fmaf(v[j], p.scale, w[j]) : w[j];
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = keep[j] ? v[j] * p.scale : 0.f;
    }
    stv<VEC>(p.out + oo, o);
}

template <int OP, int VEC>
__global__ void __launch_bounds__(kBlock) dropout_kernel(DropParams p) {
    const int64_t n = live_rows(p.N, p.n_dyn);
    long long seed = p.seed, call = p.call;
    if (OP != OP_MASK) {
        seed = p.state[0];
        call = OP == OP_FWD ? p.state[1] : p.call_io[0];
    }
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)((uint64_t)seed >> 32);
    const uint32_t c2 = (uint32_t)call, c3 = (uint32_t)((uint64_t)call >> 32);
    if (p.flat) {
        const int64_t total = n * (p.C / VEC), step = (int64_t)gridDim.x * kBlock;
        for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < total; g += step)
            drop_elems<OP, VEC>(p, g * VEC, g * VEC, g * VEC, g * VEC, k0, k1, c2, c3);
    } else {
        const int lanes = 1 << p.lanes_log2, lane = threadIdx.x & (lanes - 1), rows = kBlock >> p.lanes_log2;
        for (int64_t row = (int64_t)blockIdx.x * rows + (threadIdx.x >> p.lanes_log2); row < n; row += (int64_t)gridDim.x * rows)
            for (int c = lane * VEC; c < p.C; c += lanes * VEC)
                drop_elems<OP, VEC>(p, row * p.C + c, row * p.xs + c, row * p.os + c, row * p.rs + c, k0, k1, c2, c3);
    }
    if (OP == OP_FWD) {
        if (blockIdx.x == 0 && threadIdx.x == 0) p.call_io[0] = call;
        __syncthreads();
        if (threadIdx.x == 0) {
            // Nothing is published through the ticket: the one requirement is that this block's read of state[1] has
            // COMPLETED before its arrival counts (a wave that used the value waited for it before its stores, which are
            // before the barrier; this wave waits for all of its own outstanding loads here).  A device-scope fence
            // (__threadfence: an L2 write-back and invalidate per block, up to 2048 a launch) is not needed for that.
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __builtin_amdgcn_s_waitcnt(0);                  // vmcnt, expcnt and lgkmcnt all zero
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            const unsigned long long t = __hip_atomic_fetch_add(p.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t == (unsigned long long)gridDim.x - 1) { *p.ticket = 0; p.state[1] = call + 1; }
        }
    }
}

template <int OP>
int dropout_launch(DropParams& p, const char* who, hipStream_t s) {
    // 16 B per lane when the width, every row stride and every pointer allow it; the scalar path otherwise
    const int vec = OP == OP_MASK ? ((p.C % 4 == 0 && ((uintptr_t)p.mask & 3) == 0) ? 4 : 1)
                                  : (row_vec(p.C, {p.x, p.out, p.res}, {p.xs, p.os, p.res ? p.rs : 0}) == 4 ? 4 : 1);
    const int cg = (p.C + vec - 1) / vec;
    int64_t blocks;
    if (p.flat) {
        blocks = (p.N * cg + kBlock - 1) / kBlock;
    } else {
        p.lanes_log2 = 0;
        while ((1 << p.lanes_log2) < cg && p.lanes_log2 < 8) ++p.lanes_log2;
        const int rows = kBlock >> p.lanes_log2;
        blocks = (p.N + rows - 1) / rows;
    }
    const unsigned grid = (unsigned)(blocks > kMaxGrid ? kMaxGrid : blocks);
    if (vec == 4) hipLaunchKernelGGL((dropout_kernel<OP, 4>), dim3(grid), dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL((dropout_kernel<OP, 1>), dim3(grid), dim3(kBlock), 0, s, p);
    KPGNN_LAUNCH_CHECK(who);
    return KPGNN_OK;
}

int check_desc(const kpgnn_dropout_desc* d, const char* who) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->N >= 0 && d->C >= 1, "%s: bad N=%lld C=%d", who, (long long)d->N, d->C);
    KPGNN_REQUIRE(d->x && d->out, "%s: NULL x/out", who);
    KPGNN_REQUIRE(d->state && d->call_io, "%s: NULL state/call_io", who);
    KPGNN_REQUIRE(d->x_stride >= d->C && d->out_stride >= d->C, "%s: x/out row stride shorter than C=%d", who, d->C);
    return KPGNN_OK;
}

DropParams params_of(const kpgnn_dropout_desc* d, bool with_residual) {
    DropParams p = {};
    p.n_dyn = d->n_dyn; p.N = d->N; p.C = d->C;
    p.x = d->x; p.xs = d->x_stride; p.out = d->out; p.os = d->out_stride;
    if (with_residual && d->residual) { p.res = d->residual; p.rs = d->r_stride; }
    p.thr = d->thr; p.scale = d->scale;
    p.state = reinterpret_cast<long long*>(d->state); p.call_io = reinterpret_cast<long long*>(d->call_io);
    p.ticket = reinterpret_cast<unsigned long long*>(d->ticket);
    p.flat = p.xs == p.C && p.os == p.C && (!p.res || p.rs == p.C);
    return p;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_dropout_fwd(const kpgnn_dropout_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_dropout_fwd";
    if (int rc = check_desc(d, who)) return rc;
    KPGNN_REQUIRE(d->ticket != nullptr, "%s: NULL ticket", who);
    KPGNN_REQUIRE(!d->residual || d->r_stride >= d->C, "%s: residual row stride shorter than C=%d", who, d->C);
    if (d->N == 0) return KPGNN_OK;         // (nothing is launched: no call id is consumed)
    DropParams p = params_of(d, true);
    return dropout_launch<OP_FWD>(p, "dropout_kernel<fwd>", (hipStream_t)stream);
}

extern "C" int kpgnn_dropout_bwd(const kpgnn_dropout_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_dropout_bwd";
    if (int rc = check_desc(d, who)) return rc;
    if (d->N == 0) return KPGNN_OK;
    DropParams p = params_of(d, false);
    return dropout_launch<OP_BWD>(p, "dropout_kernel<bwd>", (hipStream_t)stream);
}

extern "C" int kpgnn_dropout_mask(const kpgnn_dropout_mask_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_dropout_mask";
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->N >= 0 && d->C >= 1, "%s: bad N=%lld C=%d", who, (long long)d->N, d->C);
    KPGNN_REQUIRE(d->mask != nullptr, "%s: NULL mask", who);
    if (d->N == 0) return KPGNN_OK;
    DropParams p = {};
    p.N = d->N; p.C = d->C; p.mask = d->mask; p.thr = d->thr; p.seed = d->seed; p.call = d->call; p.flat = 1;
    return dropout_launch<OP_MASK>(p, "dropout_kernel<mask>", (hipStream_t)stream);
}
