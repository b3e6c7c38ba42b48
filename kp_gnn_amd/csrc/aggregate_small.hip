// K-hop aggregation for SMALL batches (a few thousand nodes): one block per node, one 32-lane unit per hop.
// Contract: include/kpgnn.h, kpgnn_aggregate_fwd / kpgnn_aggregate_bwd (this file is one of their kernels).
//
// The sub-group kernels of aggregate.hip walk a node's hops one after the other - ~10 dependent round trips per node.  With
// 47k nodes that latency hides behind the other resident nodes; with 1.5k nodes (the reference's batch of 64 molecules)
// there are fewer nodes than sub-group slots on the chip and a launch costs what ONE node's chain costs: 18 us forward,
// 12 us backward at N = 1495, K = 8, D = 104.  Here the K hops of a node are gathered by K units of one block at the same
// time (lane = four feature columns, as there), so the chain is three loads deep - row pointers -> pair list -> rows -
// whatever K is; the hops meet in LDS for the fused geometric combine.  Same order of every sum as the sub-group kernels
// (pairs in list order, hops in order): S and gx are theirs bit for bit.  Two exceptions, equal to rounding only: theta * v
// is rounded before the hop sum here, fused there (hout, K > 1); an accumulating slot's old value follows the segment's last
// pair here, agg_bwd_kernel's chunked loop adds it behind the hop's first PF pairs, where it arrives.
//   forward : the KP-GIN+ training epilogue only (GELU, theta from alphas or given, dictionary P, code tables, S saved, per-hop
//             slot inputs) - the configuration `FAST` of aggregate.hip;
//   backward: the plain transposed gather gx = sum g[dst] into per-hop slot outputs (accumulate_mask honoured).
#include "kpgnn_common.h"

namespace kpgnn {
namespace {

constexpr int kUnit = 32;                 // lanes per (node, hop): 4 columns each -> D <= 128
constexpr int kMaxHops = 8;
constexpr int kBlockS = kUnit * kMaxHops; // 256

__device__ __forceinline__ float gelu_exact_s(float x) {
    float e2;
    return 0.5f * x * (1.0f + fast_erf(x * 0.70710678118654752440f, &e2));
}

struct SmallFwd {
    int N, K, D, K_csr, n_dict;
    const int32_t* rowptr; const int32_t* col; const uint16_t* code;
    const float* xs[kMaxHops]; int64_t x_sn;
    const float* table0; const float* tablek;
    const float* ptab; const int32_t* uid; int64_t uid_stride;
    const float* theta; const float* alphas; float* theta_out;
    const float* xbias;
    float* pre; float* hout;
};

__global__ void __launch_bounds__(kBlockS)
agg_fwd_small_kernel(const SmallFwd p) {
    __shared__ __attribute__((aligned(16))) float part[kMaxHops][kUnit * 4];
    const int k = threadIdx.x / kUnit, sl = threadIdx.x % kUnit;
    const int lane = threadIdx.x & (kWave - 1);
    const int u0 = lane - sl;                          // first lane of this unit inside its wave
    const int c0 = sl * 4, D = p.D;
    const bool col_ok = c0 < D, hop_ok = k < p.K;
    // theta[k, c0..c0+3]: given, or softmax_k(a (1-a)^k) from alphas (block 0 publishes it for the backward)
    float th[4] = {0.f, 0.f, 0.f, 0.f};
    if (hop_ok && col_ok) {
        if (p.alphas) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float a = 1.0f / (1.0f + __expf(-p.alphas[c0 + q]));
                const float qq = 1.0f - a;
                float pw = 1.0f, mx = -INFINITY;
                for (int j = 0; j < p.K; ++j) { mx = fmaxf(mx, a * pw); pw *= qq; }
                float sum = 0.f, mine = 0.f;
                pw = 1.0f;
                for (int j = 0; j < p.K; ++j) { const float e = __expf(a * pw - mx); sum += e; if (j == k) mine = e; pw *= qq; }
                th[q] = mine * (1.0f / sum);
            }
            if (blockIdx.x == 0) *reinterpret_cast<float4*>(p.theta_out + (int64_t)k * D + c0) = make_float4(th[0], th[1], th[2], th[3]);
        } else {
            const float4 t = *reinterpret_cast<const float4*>(p.theta + (int64_t)k * D + c0);
            th[0] = t.x; th[1] = t.y; th[2] = t.z; th[3] = t.w;
        }
    }
    const float* tab = k == 0 ? p.table0 : p.tablek;
    const float* xk = hop_ok ? p.xs[k] : p.xs[0];
    for (int64_t i = blockIdx.x; i < p.N; i += gridDim.x) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        int seglen = 0;
        float4 pr = make_float4(0.f, 0.f, 0.f, 0.f);               // the dictionary row: requested up front (uid -> row is its own chain)
        if (hop_ok && col_ok) pr = *reinterpret_cast<const float4*>(p.ptab + (int64_t)p.uid[i * p.uid_stride + k] * D + c0);
        if (hop_ok) {
            const int32_t* rp = p.rowptr + i * p.K_csr + k;
            const int beg = rp[0], end = rp[1];
            seglen = end - beg;
            for (int base = beg; base < end; base += kUnit) {      // a chunk of the pair list: one pair per lane
                int myj = 0, myc = 0;
                if (base + sl < end) { myj = p.col[base + sl]; myc = p.code[base + sl]; }
                const int cnt = min(kUnit, end - base);
                int t = 0;
                for (; t + 3 < cnt; t += 4) {                      // four pairs in flight, added in list order
                    float4 r[4], e[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int j = __shfl(myj, u0 + t + q), cd = __shfl(myc, u0 + t + q);
                        if (col_ok) {
                            r[q] = *reinterpret_cast<const float4*>(xk + (int64_t)j * p.x_sn + c0);
                            e[q] = *reinterpret_cast<const float4*>(tab + (int64_t)cd * D + c0);
                        }
                    }
                    if (col_ok) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            v[0] += r[q].x + e[q].x; v[1] += r[q].y + e[q].y; v[2] += r[q].z + e[q].z; v[3] += r[q].w + e[q].w;
                        }
                    }
                }
                for (; t < cnt; ++t) {
                    const int j = __shfl(myj, u0 + t), cd = __shfl(myc, u0 + t);
                    if (col_ok) {
                        const float4 r = *reinterpret_cast<const float4*>(xk + (int64_t)j * p.x_sn + c0);
                        const float4 e = *reinterpret_cast<const float4*>(tab + (int64_t)cd * D + c0);
                        v[0] += r.x + e.x; v[1] += r.y + e.y; v[2] += r.z + e.z; v[3] += r.w + e.w;
                    }
                }
            }
        }
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (hop_ok && col_ok) {
            if (p.xbias && k >= 1) {                               // hopk_node_path_emb(pe_attr == 0) row, KPGINplus.py:70-72
                const float4 xb = *reinterpret_cast<const float4*>(p.xbias + c0);
                const float sl_f = (float)seglen;
                v[0] = fmaf(sl_f, xb.x, v[0]); v[1] = fmaf(sl_f, xb.y, v[1]); v[2] = fmaf(sl_f, xb.z, v[2]); v[3] = fmaf(sl_f, xb.w, v[3]);
            }
            *reinterpret_cast<float4*>(p.pre + (i * p.K + k) * (int64_t)D + c0) = make_float4(v[0], v[1], v[2], v[3]);
            o[0] = th[0] * (gelu_exact_s(v[0]) + pr.x); o[1] = th[1] * (gelu_exact_s(v[1]) + pr.y);
            o[2] = th[2] * (gelu_exact_s(v[2]) + pr.z); o[3] = th[3] * (gelu_exact_s(v[3]) + pr.w);
        }
        *reinterpret_cast<float4*>(&part[k][c0]) = make_float4(o[0], o[1], o[2], o[3]);
        __syncthreads();
        if (k == 0 && col_ok) {                                    // hops in order
            float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f;
            for (int j = 0; j < p.K; ++j) {
                const float4 q = *reinterpret_cast<const float4*>(&part[j][c0]);
                h0 += q.x; h1 += q.y; h2 += q.z; h3 += q.w;
            }
            *reinterpret_cast<float4*>(p.hout + i * (int64_t)D + c0) = make_float4(h0, h1, h2, h3);
        }
        __syncthreads();
    }
}

struct SmallBwd {
    int N, K, D, K_csr;
    const int32_t* rowptr; const int32_t* col;
    const float* g; int64_t g_sn, g_sk;
    float* gxs[kMaxHops]; int64_t gx_sn;
    uint32_t acc_mask;
};

__global__ void __launch_bounds__(kBlockS)
agg_bwd_small_kernel(const SmallBwd p) {
    const int k = threadIdx.x / kUnit, sl = threadIdx.x % kUnit;
    const int lane = threadIdx.x & (kWave - 1);
    const int u0 = lane - sl;
    const int c0 = sl * 4, D = p.D;
    const bool col_ok = c0 < D;
    if (k >= p.K) return;
    const float* gk = p.g + (int64_t)k * p.g_sk;
    for (int64_t j = blockIdx.x; j < p.N; j += gridDim.x) {
        const int32_t* rp = p.rowptr + j * p.K_csr + k;
        const int beg = rp[0], end = rp[1];
        float* dst = p.gxs[k] + j * p.gx_sn + c0;
        float4 old = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool accum = (p.acc_mask >> k) & 1u;
        if (accum && col_ok) old = *reinterpret_cast<const float4*>(dst);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        for (int base = beg; base < end; base += kUnit) {
            int myi = 0;
            if (base + sl < end) myi = p.col[base + sl];
            const int cnt = min(kUnit, end - base);
            int t = 0;
            for (; t + 3 < cnt; t += 4) {
                float4 r[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = __shfl(myi, u0 + t + q);
                    if (col_ok) r[q] = *reinterpret_cast<const float4*>(gk + (int64_t)i * p.g_sn + c0);
                }
                if (col_ok) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) { v[0] += r[q].x; v[1] += r[q].y; v[2] += r[q].z; v[3] += r[q].w; }
                }
            }
            for (; t < cnt; ++t) {
                const int i = __shfl(myi, u0 + t);
                if (col_ok) {
                    const float4 r = *reinterpret_cast<const float4*>(gk + (int64_t)i * p.g_sn + c0);
                    v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
                }
            }
        }
        if (col_ok) *reinterpret_cast<float4*>(dst) = make_float4(v[0] + old.x, v[1] + old.y, v[2] + old.z, v[3] + old.w);
    }
}

// Measured crossover against the sub-group kernels (KP-GIN+ step, K = L = 8, D = 104): N = 1.5k 1.32 vs 1.42 ms, 3.0k 1.47 vs
// 1.50, 6.0k 1.86 vs 1.74, 12k 2.58 vs 2.22 - above ~4k nodes the sub-group kernels have enough nodes in flight.
constexpr int kSmallMaxNodes = 4096;

bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

int agg_small_fwd(const kpgnn_agg_fwd_desc* d, hipStream_t s, bool* handled) {
    *handled = false;
    const bool tables = d->use_tables != 0;
    if (d->N > kSmallMaxNodes || d->K > kMaxHops || d->D % 4 || d->D > kUnit * 4 || d->x || d->mode != KPGNN_MODE_GINPLUS ||
        !d->theta || !d->hout || d->periph || !d->uid || !d->ptab || !d->pre || !tables || !d->table0 ||
        (d->K > 1 && !d->tablek) || d->storage != KPGNN_STORE_F32 || d->x_sn % 4 || d->uid_stride < d->K)
        return KPGNN_OK;
    if (!al16(d->table0) || !al16(d->tablek) || !al16(d->ptab) || !al16(d->theta) || !al16(d->hout) || !al16(d->pre) ||
        !al16(d->xbias) || !al16(d->alphas))
        return KPGNN_OK;
    SmallFwd p;
    p.N = d->N; p.K = d->K; p.D = d->D; p.K_csr = d->K_csr; p.n_dict = d->n_dict;
    p.rowptr = d->rowptr; p.col = d->col; p.code = d->code;
    for (int k = 0; k < kMaxHops; ++k) {
        p.xs[k] = k < d->K ? d->x_slot[k] : d->x_slot[0];
        if (!p.xs[k] || !al16(p.xs[k])) return KPGNN_OK;
    }
    p.x_sn = d->x_sn;
    p.table0 = d->table0; p.tablek = d->K > 1 ? d->tablek : d->table0;
    p.ptab = d->ptab; p.uid = d->uid; p.uid_stride = d->uid_stride;
    p.theta = d->theta; p.alphas = d->alphas; p.theta_out = const_cast<float*>(d->theta);
    p.xbias = d->xbias; p.pre = d->pre; p.hout = d->hout;
    *handled = true;
    hipLaunchKernelGGL(agg_fwd_small_kernel, dim3((unsigned)d->N), dim3(kBlockS), 0, s, p);
    KPGNN_LAUNCH_CHECK("agg_fwd_small_kernel");
    agg_route_bump(0, KPGNN_AGG_ROUTE_SMALL);
    return KPGNN_OK;
}

int agg_small_bwd(const kpgnn_agg_bwd_desc* d, hipStream_t s, bool* handled) {
    *handled = false;
    const bool want_tables = d->use_tables && d->gtable0;
    if (d->N > kSmallMaxNodes || d->K > kMaxHops || d->D % 4 || d->D > kUnit * 4 || d->gx || want_tables ||
        (d->mode != KPGNN_MODE_GINPLUS && d->mode != KPGNN_MODE_SUM) || d->storage != KPGNN_STORE_F32 ||
        d->g_sn % 4 || d->g_sk % 4 || d->gx_sn % 4 || !al16(d->g))
        return KPGNN_OK;
    SmallBwd p;
    p.N = d->N; p.K = d->K; p.D = d->D; p.K_csr = d->K_csr;
    p.rowptr = d->rowptr_src; p.col = d->col_src;
    p.g = d->g; p.g_sn = d->g_sn; p.g_sk = d->g_sk;
    for (int k = 0; k < kMaxHops; ++k) {
        p.gxs[k] = k < d->K ? d->gx_slot[k] : d->gx_slot[0];
        if (!p.gxs[k] || !al16(p.gxs[k])) return KPGNN_OK;
    }
    // (two hop slots of one call sharing an accumulating buffer are refused by the caller's check in kpgnn_aggregate_bwd)
    p.gx_sn = d->gx_sn; p.acc_mask = d->accumulate_mask;
    *handled = true;
    hipLaunchKernelGGL(agg_bwd_small_kernel, dim3((unsigned)d->N), dim3(kBlockS), 0, s, p);
    KPGNN_LAUNCH_CHECK("agg_bwd_small_kernel");
    agg_route_bump(1, KPGNN_AGG_ROUTE_SMALL);
    return KPGNN_OK;
}

}  // namespace kpgnn
