// The scoring LSTM of the attention jumping-knowledge readout: nn.LSTM(H, P, bidirectional) over the S states of a body,
// summed over its 2P outputs (gfx950).  Contract: include/kpgnn.h, kpgnn_jk_lstm_fwd / _bwd.
//
// models/GNNs.py runs the scorer over torch.stack(h_list): a [N,S,H] copy, a gradient buffer of the same size, and a vendor
// recurrence of hidden size P = num_layer <= 16.  Here the S state pointers travel BY VALUE in the kernel arguments (as in
// jk_reduce.hip); the slot index is uniform in every kernel, so the table is read with scalar loads.
//   forward   jk_lstm_prep_kernel   W_ih of both directions transposed to [H,8P] (coalesced operand reads), b_ih + b_hh
//             jk_lstm_gemm_kernel   gin[n,t,:] = x[t][n,:] W^T + b on v_mfma_f32_32x32x2_f32: a block stages 64 rows of ONE
//                                   state in LDS, a wave owns 32 rows x 32 gate columns
//             jk_lstm_fwd_kernel<P> the recurrence, one thread per (node, direction), h / c / the 4P gates in registers, W_hh
//                                   wave-uniform; leaves the gate activations in place of gin and c beside them (training)
//   backward  jk_lstm_bwd_kernel<P> BPTT in registers -> dgin [N,S,8P], h_prev [N,S,2P]
//             jk_lstm_gemm_kernel   gx[t] = dgin[:,t,:] W_ih, the same kernel with the roles of the widths exchanged
//             jk_lstm_wgrad_kernel  [dW_ih | db | dW_hh] = dgin^T [x | 1 | h_prev] on the matrix instruction: one block per
//                                   FIXED range of 64 rows (all S slots), one partial [8P, H+1+2P] per block
//             jk_lstm_reduce_kernel the partials added in tile order, scattered to the six parameter gradients
// No atomics; every sum has a fixed order that depends on the live rows alone, so the bits do not depend on the capacity.
// Rows at or beyond *n_dyn are never loaded (they may hold NaN) and never stored.
// sigmoid is 1 / (1 + expf(-x)) with a true division and tanh is tanhf: the operator is held to float64 with the fp32 CPU
// module as the yardstick, and the activations are not where this launch spends its time.
#include <cmath>

#include "mfma_tile.h"

namespace kpgnn {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxP = 16, kMaxH = 256, kMaxS = KPGNN_JK_MAX_STATES;
constexpr int kGemmRows = 64;       // rows of a projection tile (two 32-row MFMA tiles)
constexpr int kRecNodes = 128;      // nodes of a recurrence block: waves 0, 1 walk forward, waves 2, 3 in reverse
constexpr int kGradRows = 64;       // rows of a parameter-gradient tile - FIXED: the partial sums must not depend on N
constexpr int kGradBlock = 512;     // eight waves, one 32 x 32 output tile each at P = 8, H = 104

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

struct LstmParams {
    const int32_t* n_dyn;
    int64_t N; int H, P, S; int64_t xs;
    const float* w_ih[2]; const float* w_hh[2]; const float* b_ih[2]; const float* b_hh[2];
    float* wt; float* bias;                      // prep: [H,8P], [8P]
    float* gin; float* cst; int save;            // [N,S,2,4P] pre-activations in / activations out, [N,S,2,P] cell states
    float* score;
    const float* acts; const float* cs;          // backward: what the forward left in gin / cst
    const float* gscore; float* dgin; float* hprev; float* slab;
    float* dw_ih[2]; float* dw_hh[2]; float* db[2];
    const float* x[kMaxS];
};

// ---- W_ih of both directions -> wt [H][8P] (column dir * 4P + gate row), bias [8P] = b_ih + b_hh
__global__ void __launch_bounds__(kBlock) jk_lstm_prep_kernel(const LstmParams p) {
    const int G = 8 * p.P, G4 = 4 * p.P;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e < p.H * G) {
        const int k = e / G, g = e % G, dir = g >= G4, gg = g - dir * G4;
        p.wt[e] = (dir ? p.w_ih[1] : p.w_ih[0])[(int64_t)gg * p.H + k];
    } else if (e < p.H * G + G) {
        const int g = e - p.H * G, dir = g >= G4, gg = g - dir * G4;
        p.bias[g] = (dir ? p.b_ih[1] : p.b_ih[0])[gg] + (dir ? p.b_hh[1] : p.b_hh[0])[gg];
    }
}

// ---- out[t][row, 0..O) = in[t][row, 0..I) Wm (+ bias), Wm [I][O] row-major in up to two pieces (rows < split, rows >= split)
struct GemmParams {
    const int32_t* n_dyn;
    int64_t N; int S, I, O, ipad, pitch;
    int from_states;                             // input rows of slot t: x[t] (1) or in + t * in_ts (0); row stride in_rs
    const float* in; int64_t in_rs, in_ts;
    const float* wm0; const float* wm1; int split;
    const float* bias;
    float* out; int64_t out_rs, out_ts;
    int vec_in;                                  // 16-byte loads of the input rows (I % 4 == 0, strides and pointers aligned)
    const float* x[kMaxS];
};

template <bool VOUT>
__global__ void __launch_bounds__(kBlock) jk_lstm_gemm_kernel(const GemmParams p) {
    extern __shared__ __align__(16) float tile[];                  // [kGemmRows][pitch]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kk = lane >> 5, c = lane & 31;
    const int64_t n = live_rows(p.N, p.n_dyn);
    const int64_t units = (n + kGemmRows - 1) / kGemmRows * p.S;   // (64-row tile, slot), the slot running fastest
    const int OB = (p.O + 31) >> 5, ipad = p.ipad, pitch = p.pitch, I = p.I, O = p.O, split = p.split;
    const float* wm0 = p.wm0;
    const float* wm1 = p.wm1;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int t = (int)(u % p.S);
        const int64_t r0 = u / p.S * kGemmRows;
        const float* src = p.from_states ? p.x[t] : p.in + (int64_t)t * p.in_ts;
        __syncthreads();                                           // the previous unit is fully consumed
        if (p.vec_in) {
            const int q4 = ipad >> 2;
            for (int e = tid; e < kGemmRows * q4; e += kBlock) {
                const int r = e / q4, cq = (e - r * q4) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r0 + r < n) v = ld4(src + (r0 + r) * p.in_rs + cq);
                st4(tile + r * pitch + cq, v);
            }
        } else {
            for (int e = tid; e < kGemmRows * ipad; e += kBlock) {
                const int r = e / ipad, cc = e - r * ipad;
                tile[r * pitch + cc] = (r0 + r < n && cc < p.I) ? src[(r0 + r) * p.in_rs + cc] : 0.f;
            }
        }
        __syncthreads();
        for (int item = wave; item < 2 * OB; item += kBlock / kWave) {
            const int rs = item & 1, ob = item >> 1;
            if (r0 + rs * 32 >= n) continue;                       // (uniform: the whole 32-row half is dead)
            const int o = ob * 32 + c;
            const bool o_ok = o < p.O;
            const int oc = o_ok ? o : 0;
            f32x16 acc;
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[v] = 0.f;
            const float* b = tile + (rs * 32 + c) * pitch + kk;
            // (an unconditional load from a clamped address, then a select; four k-steps by hand, so that four operand loads are
            //  in flight before the first product - `#pragma unroll` is refused on this loop)
            auto wload = [&](int ks) {
                const int k = 2 * ks + kk, kc = k < I ? k : I - 1;
                const float* wrow = kc < split ? wm0 + (int64_t)kc * O : wm1 + (int64_t)(kc - split) * O;
                const float a = wrow[oc];
                return (o_ok && k < I) ? a : 0.f;
            };
            const int nks = ipad >> 1;
            int ks = 0;
            for (; ks + 4 <= nks; ks += 4) {
                const float a0 = wload(ks), a1 = wload(ks + 1), a2 = wload(ks + 2), a3 = wload(ks + 3);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[2 * ks], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[2 * ks + 2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b[2 * ks + 4], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b[2 * ks + 6], acc, 0, 0, 0);
            }
            for (; ks < nks; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wload(ks), b[2 * ks], acc, 0, 0, 0);
            const int64_t row = r0 + rs * 32 + c;
            if (row < n) {
                float* q = p.out + (int64_t)t * p.out_ts + row * p.out_rs;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int o0 = ob * 32 + 8 * g + 4 * kk;
                    if (VOUT) {
                        if (o0 < p.O) {                            // (O % 4 == 0: the four columns are in or out together)
                            float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
                            if (p.bias) bb = ld4(p.bias + o0);
                            st4(q + o0, make_float4(acc[4 * g] + bb.x, acc[4 * g + 1] + bb.y, acc[4 * g + 2] + bb.z,
                                                    acc[4 * g + 3] + bb.w));
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (o0 + j < p.O) q[o0 + j] = acc[4 * g + j] + (p.bias ? p.bias[o0 + j] : 0.f);
                    }
                }
            }
        }
    }
}

// ---- forward recurrence: thread = (node, direction); the two directions of a node meet in LDS for the score
template <int P>
__global__ void __launch_bounds__(kBlock) jk_lstm_fwd_kernel(const LstmParams p) {
    __shared__ float hs[2][kMaxS][kRecNodes];
    const int dir = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kRecNodes);
    const int i = threadIdx.x % kRecNodes;
    const int64_t nl = live_rows(p.N, p.n_dyn);
    const int64_t n0 = (int64_t)blockIdx.x * kRecNodes, n = n0 + i;
    const int S = p.S;
    // W_hh [4P][P] of this wave's direction, read back at uniform addresses (broadcast).  From global memory the loads are
    // vector loads (the kernel stores through other pointers, so they are not provably invariant) and all 4 P^2 of a step
    // are issued ahead of their use: 256 + 55 registers at P = 8, spills from P = 11
    __shared__ float whl[2][4 * P * P];
    for (int e = threadIdx.x; e < 8 * P * P; e += kBlock) whl[e / (4 * P * P)][e % (4 * P * P)] = (e < 4 * P * P ? p.w_hh[0] : p.w_hh[1])[e % (4 * P * P)];
    __syncthreads();
    if (n < nl) {
        float h[P], c[P];
#pragma unroll
        for (int q = 0; q < P; ++q) { h[q] = 0.f; c[q] = 0.f; }
        for (int s = 0; s < S; ++s) {
            const int t = dir ? S - 1 - s : s;
            const int64_t cell = (n * S + t) * 2 + dir;
            int z = 0;
            asm volatile("" : "+v"(z));                            // (opaque: the reads of W_hh stay inside the step, not
            const float* whh = whl[dir] + z;                       //  hoisted into 4 P^2 registers that live across the loop)
            float* gi = p.gin + cell * (4 * P);
            float g[4 * P];
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const float4 v = ld4(gi + 4 * q);
                g[4 * q] = v.x; g[4 * q + 1] = v.y; g[4 * q + 2] = v.z; g[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int q = 0; q < 4 * P; ++q) {
#pragma unroll
                for (int r = 0; r < P; ++r) g[q] = fmaf(whh[q * P + r], h[r], g[q]);
                // (the gate is finished HERE: tanhf branches, and left alone the multiplies sink into the blocks that use them
                //  while all 4 P^2 reads of W_hh stay in front - 256 + 54 registers at P = 8, spills from P = 11)
                asm volatile("" : "+v"(g[q]));
            }
            float hsum = 0.f;
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const float ig = sigm(g[q]), fg = sigm(g[P + q]), gg = tanhf(g[2 * P + q]), og = sigm(g[3 * P + q]);
                c[q] = fmaf(fg, c[q], ig * gg);
                h[q] = og * tanhf(c[q]);
                hsum += h[q];
                g[q] = ig; g[P + q] = fg; g[2 * P + q] = gg; g[3 * P + q] = og;
            }
            if (p.save) {
#pragma unroll
                for (int q = 0; q < P; ++q) st4(gi + 4 * q, make_float4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]));
                if constexpr (P % 4 == 0) {
#pragma unroll
                    for (int q = 0; q < P; q += 4) st4(p.cst + cell * P + q, make_float4(c[q], c[q + 1], c[q + 2], c[q + 3]));
                } else {
#pragma unroll
                    for (int q = 0; q < P; ++q) p.cst[cell * P + q] = c[q];
                }
            }
            hs[dir][t][i] = hsum;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kRecNodes * S; e += kBlock) {     // the block's [128,S] piece of score is one run
        const int ii = e / S, t = e - ii * S;
        if (n0 + ii < nl) p.score[(n0 + ii) * S + t] = hs[0][t][ii] + hs[1][t][ii];
    }
}

// ---- BPTT: thread = (node, direction)
template <int P>
__global__ void __launch_bounds__(kBlock) jk_lstm_bwd_kernel(const LstmParams p) {
    const int dir = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kRecNodes);
    const int64_t n = (int64_t)blockIdx.x * kRecNodes + threadIdx.x % kRecNodes;
    __shared__ float whl[2][4 * P * P];                             // (as in the forward)
    for (int e = threadIdx.x; e < 8 * P * P; e += kBlock) whl[e / (4 * P * P)][e % (4 * P * P)] = (e < 4 * P * P ? p.w_hh[0] : p.w_hh[1])[e % (4 * P * P)];
    __syncthreads();
    if (n >= live_rows(p.N, p.n_dyn)) return;
    const int S = p.S;
    float dh[P], dc[P];
#pragma unroll
    for (int q = 0; q < P; ++q) { dh[q] = 0.f; dc[q] = 0.f; }
    for (int s = S - 1; s >= 0; --s) {                              // reverse of the forward visiting order
        const int t = dir ? S - 1 - s : s;
        const int tp = dir ? t + 1 : t - 1;                         // the slot visited just before t
        int z = 0;
        asm volatile("" : "+v"(z));                                 // (as in the forward)
        const float* whh = whl[dir] + z;
        const int64_t cell = (n * S + t) * 2 + dir, cellp = (n * S + (s > 0 ? tp : t)) * 2 + dir;
        const float dst = p.gscore[n * S + t];
        // the cell's 4P activations as P 16-byte loads (a cell starts 16 P bytes into the array); c, c_prev, o_prev and the
        // h_prev store likewise where P % 4 == 0 makes them aligned
        float a[4 * P], cc[P], cpv[P], opv[P], hpv[P], dg[4 * P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const float4 v = ld4(p.acts + cell * (4 * P) + 4 * q);
            a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
        }
        if constexpr (P % 4 == 0) {
#pragma unroll
            for (int q = 0; q < P; q += 4) {
                const float4 v = ld4(p.cs + cell * P + q), w = ld4(p.cs + cellp * P + q), o = ld4(p.acts + cellp * (4 * P) + 3 * P + q);
                cc[q] = v.x; cc[q + 1] = v.y; cc[q + 2] = v.z; cc[q + 3] = v.w;
                cpv[q] = w.x; cpv[q + 1] = w.y; cpv[q + 2] = w.z; cpv[q + 3] = w.w;
                opv[q] = o.x; opv[q + 1] = o.y; opv[q + 2] = o.z; opv[q + 3] = o.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < P; ++q) { cc[q] = p.cs[cell * P + q]; cpv[q] = p.cs[cellp * P + q]; opv[q] = p.acts[cellp * (4 * P) + 3 * P + q]; }
        }
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const float ig = a[q], fg = a[P + q], gg = a[2 * P + q], og = a[3 * P + q], ct = cc[q];
            const float cp = s > 0 ? cpv[q] : 0.f;
            const float hp = s > 0 ? opv[q] * tanhf(cp) : 0.f;
            hpv[q] = hp;
            const float tc = tanhf(ct);
            const float dhq = dh[q] + dst;
            const float dcq = fmaf(dhq * og, 1.0f - tc * tc, dc[q]);
            dg[q] = dcq * gg * ig * (1.0f - ig);
            dg[P + q] = dcq * cp * fg * (1.0f - fg);
            dg[2 * P + q] = dcq * ig * (1.0f - gg * gg);
            dg[3 * P + q] = dhq * tc * og * (1.0f - og);
            dc[q] = dcq * fg;
        }
        if constexpr (P % 4 == 0) {
#pragma unroll
            for (int q = 0; q < P; q += 4) st4(p.hprev + cell * P + q, make_float4(hpv[q], hpv[q + 1], hpv[q + 2], hpv[q + 3]));
        } else {
#pragma unroll
            for (int q = 0; q < P; ++q) p.hprev[cell * P + q] = hpv[q];
        }
        float* dgo = p.dgin + cell * (4 * P);
#pragma unroll
        for (int q = 0; q < P; ++q) st4(dgo + 4 * q, make_float4(dg[4 * q], dg[4 * q + 1], dg[4 * q + 2], dg[4 * q + 3]));
#pragma unroll
        for (int r = 0; r < P; ++r) {
            float acc = 0.f;
#pragma unroll
            for (int q = 0; q < 4 * P; ++q) acc = fmaf(whh[q * P + r], dg[q], acc);
            dh[r] = acc;
        }
    }
}

// ---- slab[tile][8P][HE] = sum over the tile's live rows and all S slots of dgin^T [x | 1 | h_prev], HE = H + 1 + 2P
__global__ void __launch_bounds__(kGradBlock) jk_lstm_wgrad_kernel(const LstmParams p) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kk = lane >> 5, c = lane & 31;
    const int64_t nl = live_rows(p.N, p.n_dyn);
    const int64_t r0 = (int64_t)blockIdx.x * kGradRows;
    if (r0 >= nl) return;                                           // (the reduce stops at the last live tile)
    const int H = p.H, S = p.S, G = 8 * p.P, HP = 2 * p.P, HE = H + 1 + HP;
    const int GT = (G + 31) >> 5, HB = (HE + 31) >> 5;
    float* slab = p.slab + (int64_t)blockIdx.x * G * HE;
    for (int o = wave; o < GT * HB; o += kGradBlock / kWave) {
        const int gt = o % GT, hb = o / GT;
        const int ga = gt * 32 + c, cb = hb * 32 + c;
        const bool a_ok = ga < G;
        const int mode = cb < H ? 2 : cb == H ? 1 : cb < HE ? 3 : 0;   // B column: a state's, the constant 1, h_prev's, padding
        f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.f;
        for (int t = 0; t < S; ++t) {
            const float* ap = p.dgin + (int64_t)t * G + (a_ok ? ga : 0);
            const float* bp = mode == 2 ? p.x[t] + cb : p.hprev + (int64_t)t * HP + (mode == 3 ? cb - H - 1 : 0);
            const int64_t as = (int64_t)S * G, bs = mode == 2 ? p.xs : (int64_t)S * HP;
#pragma unroll 4
            for (int ks = 0; ks < kGradRows / 2; ++ks) {
                const int64_t row = r0 + 2 * ks + kk;
                const bool live = row < nl;
                const float a = (live && a_ok) ? ap[row * as] : 0.f;
                float b = 0.f;
                if (live) b = mode == 1 ? 1.0f : (mode == 0 ? 0.f : bp[row * bs]);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
            }
        }
        if (cb < HE) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int gate = gt * 32 + 8 * (v >> 2) + 4 * kk + (v & 3);
                if (gate < G) slab[(int64_t)gate * HE + cb] = acc[v];
            }
        }
    }
}

// ---- the live tiles' partials added in tile order; element (gate column g8, extended column) goes to its gradient
__global__ void __launch_bounds__(kBlock) jk_lstm_reduce_kernel(const LstmParams p) {
    const int H = p.H, P = p.P, G = 8 * P, G4 = 4 * P, HE = H + 1 + 2 * P;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= G * HE) return;
    const int64_t nl = live_rows(p.N, p.n_dyn);
    const int tiles = (int)((nl + kGradRows - 1) / kGradRows);
    const int64_t stride = (int64_t)G * HE;
    const float* q = p.slab + e;
    float s = 0.f;
    int b = 0;
    for (; b + 4 <= tiles; b += 4) {
        const float v0 = q[b * stride], v1 = q[(b + 1) * stride], v2 = q[(b + 2) * stride], v3 = q[(b + 3) * stride];
        s += v0; s += v1; s += v2; s += v3;
    }
    for (; b < tiles; ++b) s += q[b * stride];
    const int g8 = e / HE, col = e - g8 * HE, dir = g8 >= G4, g = g8 - dir * G4;
    if (col < H) {
        (dir ? p.dw_ih[1] : p.dw_ih[0])[(int64_t)g * H + col] = s;
    } else if (col == H) {
        (dir ? p.db[1] : p.db[0])[g] = s;
    } else {
        const int r = col - H - 1;
        if ((r >= P) == (dir != 0)) (dir ? p.dw_hh[1] : p.dw_hh[0])[g * P + (r - dir * P)] = s;
    }
}

// ------------------------------------------------------------------------------------------------ host side
size_t align4(size_t floats) { return (floats + 3) / 4 * 4; }
size_t prep_floats(int H, int P) { return align4((size_t)H * 8 * P + 8 * P); }
int64_t grad_tiles(int64_t N) { return (N + kGradRows - 1) / kGradRows; }
size_t fwd_ws_floats(int64_t N, int H, int P, int S, bool saved) {
    return prep_floats(H, P) + (saved ? 0 : (size_t)N * S * 8 * P);
}
size_t bwd_ws_floats(int64_t N, int H, int P, int S) {
    return (size_t)N * S * 8 * P + (size_t)N * S * 2 * P + (size_t)grad_tiles(N) * 8 * P * (H + 1 + 2 * P);
}
bool covered(int64_t N, int H, int P, int S) {
    return N >= 0 && H >= 1 && H <= kMaxH && P >= 1 && P <= kMaxP && S >= 1 && S <= kMaxS;
}

int check(const kpgnn_jk_lstm_desc* d, const char* who) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->N >= 0 && d->H >= 1 && d->P >= 1 && d->S >= 1, "%s: bad N=%lld H=%d P=%d S=%d", who, (long long)d->N, d->H,
                  d->P, d->S);
    if (d->P > kMaxP || d->H > kMaxH || d->S > kMaxS)
        return fail(KPGNN_ELIMIT, "%s: H=%d P=%d S=%d exceeds the limits H <= %d, P <= %d, S <= %d", who, d->H, d->P, d->S, kMaxH,
                    kMaxP, kMaxS);
    for (int l = 0; l < d->S; ++l) KPGNN_REQUIRE(d->x[l] != nullptr, "%s: NULL x[%d]", who, l);
    KPGNN_REQUIRE(d->x_stride >= d->H, "%s: x row stride shorter than H=%d", who, d->H);
    for (int k = 0; k < 2; ++k)
        KPGNN_REQUIRE(d->w_ih[k] != nullptr && d->w_hh[k] != nullptr, "%s: NULL w_ih[%d] / w_hh[%d]", who, k, k);
    KPGNN_REQUIRE(((uintptr_t)d->saved & 15) == 0 && ((uintptr_t)d->workspace & 15) == 0,
                  "%s: saved / workspace must be 16-byte aligned", who);
    return KPGNN_OK;
}

int check_workspace(const kpgnn_jk_lstm_desc* d, size_t floats, const char* who) {
    KPGNN_REQUIRE(d->workspace != nullptr && d->workspace_bytes >= floats * sizeof(float), "%s: workspace of %zu bytes, %zu needed",
                  who, d->workspace ? d->workspace_bytes : (size_t)0, floats * sizeof(float));
    return KPGNN_OK;
}

LstmParams params_of(const kpgnn_jk_lstm_desc* d) {
    LstmParams p = {};
    p.n_dyn = d->n_dyn; p.N = d->N; p.H = d->H; p.P = d->P; p.S = d->S; p.xs = d->x_stride;
    for (int k = 0; k < 2; ++k) {
        p.w_ih[k] = d->w_ih[k]; p.w_hh[k] = d->w_hh[k]; p.b_ih[k] = d->b_ih[k]; p.b_hh[k] = d->b_hh[k];
        p.dw_ih[k] = d->dw_ih[k]; p.dw_hh[k] = d->dw_hh[k]; p.db[k] = d->db[k];
    }
    for (int l = 0; l < kMaxS; ++l) p.x[l] = l < d->S ? d->x[l] : nullptr;
    return p;
}

int gemm_launch(GemmParams& g, bool vout, hipStream_t s) {
    g.ipad = g.vec_in ? g.I : (g.I + 1) / 2 * 2;
    g.pitch = mfma_pitch(g.ipad);
    const size_t lds = sizeof(float) * kGemmRows * (size_t)g.pitch;
    const int64_t units = (g.N + kGemmRows - 1) / kGemmRows * g.S;
    const int64_t cap = (int64_t)device_facts().cu_count * 4;
    const unsigned grid = (unsigned)(units < cap ? units : cap);
    if (vout) {
        KPGNN_HIP_TRY(ensure_dynamic_lds((const void*)jk_lstm_gemm_kernel<true>, lds));
        hipLaunchKernelGGL((jk_lstm_gemm_kernel<true>), dim3(grid), dim3(kBlock), lds, s, g);
    } else {
        KPGNN_HIP_TRY(ensure_dynamic_lds((const void*)jk_lstm_gemm_kernel<false>, lds));
        hipLaunchKernelGGL((jk_lstm_gemm_kernel<false>), dim3(grid), dim3(kBlock), lds, s, g);
    }
    KPGNN_LAUNCH_CHECK("jk_lstm_gemm_kernel");
    return KPGNN_OK;
}

template <typename F>
int dispatch_p(int P, const char* who, F&& f) {
#define KPGNN_P_CASE(K) case K: return f(std::integral_constant<int, K>{});
    switch (P) {
        KPGNN_P_CASE(1) KPGNN_P_CASE(2) KPGNN_P_CASE(3) KPGNN_P_CASE(4) KPGNN_P_CASE(5) KPGNN_P_CASE(6) KPGNN_P_CASE(7)
        KPGNN_P_CASE(8) KPGNN_P_CASE(9) KPGNN_P_CASE(10) KPGNN_P_CASE(11) KPGNN_P_CASE(12) KPGNN_P_CASE(13) KPGNN_P_CASE(14)
        KPGNN_P_CASE(15) KPGNN_P_CASE(16)
    }
#undef KPGNN_P_CASE
    return fail(KPGNN_ELIMIT, "%s: no kernel for P=%d", who, P);
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" size_t kpgnn_jk_lstm_saved_bytes(int64_t N, int32_t H, int32_t P, int32_t S) {
    if (!covered(N, H, P, S)) return 0;
    return ((size_t)N * S * 8 * P + (size_t)N * S * 2 * P) * sizeof(float);
}

extern "C" size_t kpgnn_jk_lstm_workspace_bytes(int64_t N, int32_t H, int32_t P, int32_t S) {
    if (!covered(N, H, P, S)) return 0;
    const size_t f = fwd_ws_floats(N, H, P, S, false), b = bwd_ws_floats(N, H, P, S);
    return (f > b ? f : b) * sizeof(float);
}

extern "C" int kpgnn_jk_lstm_fwd(const kpgnn_jk_lstm_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_jk_lstm_fwd";
    if (int rc = check(d, who)) return rc;
    for (int k = 0; k < 2; ++k) KPGNN_REQUIRE(d->b_ih[k] != nullptr && d->b_hh[k] != nullptr, "%s: NULL b_ih[%d] / b_hh[%d]", who, k, k);
    KPGNN_REQUIRE(d->score != nullptr, "%s: NULL score", who);
    if (int rc = check_workspace(d, fwd_ws_floats(d->N, d->H, d->P, d->S, d->saved != nullptr), who)) return rc;
    if (d->N == 0) return KPGNN_OK;
    hipStream_t s = (hipStream_t)stream;
    const int H = d->H, P = d->P, S = d->S, G = 8 * P;
    LstmParams p = params_of(d);
    float* ws = (float*)d->workspace;
    p.wt = ws; p.bias = ws + (size_t)H * G;
    p.save = d->saved != nullptr;
    p.gin = p.save ? (float*)d->saved : ws + prep_floats(H, P);
    p.cst = p.save ? p.gin + (size_t)d->N * S * G : nullptr;
    p.score = d->score;
    hipLaunchKernelGGL(jk_lstm_prep_kernel, dim3((H * G + G + kBlock - 1) / kBlock), dim3(kBlock), 0, s, p);
    KPGNN_LAUNCH_CHECK("jk_lstm_prep_kernel");
    GemmParams g = {};
    g.n_dyn = d->n_dyn; g.N = d->N; g.S = S; g.I = H; g.O = G;
    g.from_states = 1; g.in_rs = d->x_stride;
    g.wm0 = p.wt; g.wm1 = p.wt; g.split = H; g.bias = p.bias;
    g.out = p.gin; g.out_rs = (int64_t)S * G; g.out_ts = G;
    g.vec_in = (H % 4 == 0) && (d->x_stride % 4 == 0);
    for (int l = 0; l < kMaxS; ++l) {
        g.x[l] = p.x[l];
        if (l < S && ((uintptr_t)p.x[l] & 15)) g.vec_in = 0;
    }
    if (int rc = gemm_launch(g, true, s)) return rc;
    const unsigned grid = (unsigned)((d->N + kRecNodes - 1) / kRecNodes);
    return dispatch_p(P, who, [&](auto K) {
        hipLaunchKernelGGL((jk_lstm_fwd_kernel<K()>), dim3(grid), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("jk_lstm_fwd_kernel");
        return (int)KPGNN_OK;
    });
}

extern "C" int kpgnn_jk_lstm_bwd(const kpgnn_jk_lstm_desc* d, kpgnn_stream_t stream) {
    const char* who = "kpgnn_jk_lstm_bwd";
    if (int rc = check(d, who)) return rc;
    KPGNN_REQUIRE(d->saved != nullptr && d->gscore != nullptr, "%s: NULL saved / gscore", who);
    for (int k = 0; k < 2; ++k)
        KPGNN_REQUIRE(d->dw_ih[k] != nullptr && d->dw_hh[k] != nullptr && d->db[k] != nullptr, "%s: NULL dw_ih[%d] / dw_hh[%d] / db[%d]",
                      who, k, k, k);
    if (int rc = check_workspace(d, bwd_ws_floats(d->N, d->H, d->P, d->S), who)) return rc;
    if (d->N == 0) return KPGNN_OK;
    hipStream_t s = (hipStream_t)stream;
    const int H = d->H, P = d->P, S = d->S, G = 8 * P;
    LstmParams p = params_of(d);
    p.acts = (const float*)d->saved; p.cs = p.acts + (size_t)d->N * S * G;
    p.gscore = d->gscore;
    p.dgin = (float*)d->workspace; p.hprev = p.dgin + (size_t)d->N * S * G; p.slab = p.hprev + (size_t)d->N * S * 2 * P;
    const unsigned grid = (unsigned)((d->N + kRecNodes - 1) / kRecNodes);
    int rc = dispatch_p(P, who, [&](auto K) {
        hipLaunchKernelGGL((jk_lstm_bwd_kernel<K()>), dim3(grid), dim3(kBlock), 0, s, p);
        KPGNN_LAUNCH_CHECK("jk_lstm_bwd_kernel");
        return (int)KPGNN_OK;
    });
    if (rc != KPGNN_OK) return rc;
    if (d->gx) {                                                  // gx[t] = dgin[:,t,:] [W_ih[0]; W_ih[1]]
        GemmParams g = {};
        g.n_dyn = d->n_dyn; g.N = d->N; g.S = S; g.I = G; g.O = H;
        g.from_states = 0; g.in = p.dgin; g.in_rs = (int64_t)S * G; g.in_ts = G;
        g.wm0 = d->w_ih[0]; g.wm1 = d->w_ih[1]; g.split = 4 * P; g.bias = nullptr;
        g.out = d->gx; g.out_rs = H; g.out_ts = d->N * (int64_t)H;
        g.vec_in = 1;
        if (int rc2 = gemm_launch(g, (H % 4 == 0) && ((uintptr_t)d->gx & 15) == 0, s)) return rc2;
    }
    hipLaunchKernelGGL(jk_lstm_wgrad_kernel, dim3((unsigned)grad_tiles(d->N)), dim3(kGradBlock), 0, s, p);
    KPGNN_LAUNCH_CHECK("jk_lstm_wgrad_kernel");
    hipLaunchKernelGGL(jk_lstm_reduce_kernel, dim3((G * (H + 1 + 2 * P) + kBlock - 1) / kBlock), dim3(kBlock), 0, s, p);
    KPGNN_LAUNCH_CHECK("jk_lstm_reduce_kernel");
    return KPGNN_OK;
}
