// KP-GraphSAGE tail: per-hop projection of [x | x_n] + ReLU + L2-normalise (+ geometric hop-combine (+ combine_proj)),
// forward and backward, on the fp32 matrix cores (gfx950).
// Contract: include/kpgnn.h, kpgnn_sage_tail_fwd / _bwd  (reference layers/KPGraphSAGE.py:88-96, combine.py:52-58).
//
// Same shapes and the same plan as hop_mlp.hip: [N, K, dk] activations, K tiny [2 dk, dk] weights, one 256-thread block
// with a 32-node tile of x and of x_n resident in LDS (row pitch LD = 4 mod 8) next to the zero-padded weights.  The
// concatenation never exists: the two halves of W[k] multiply the two tiles into one accumulator.
//   fwd:  z = x W[:DI] + xn W[DI:] + b -> r = relu(z); the row norm is summed in the accumulator registers (the 16 lanes
//         of a row group hold one row's columns) -> y = r / max(|r|, eps) in place over x -> comb = sum_k theta_k * y_k ->
//         out = comb Wc^T + bc.  y and rinv are written once, coalesced, from LDS; the next tiles are in flight meanwhile.
//   bwd:  gcomb = gout Wc; dWc += gout^T comb; gy = gcomb (x) theta; gz = rinv (gy - y <gy, y>) [y > 0] in place over y;
//         dW[k] += [x_k | xn_k]^T gz_k; gx = gz W[:DI]^T, gxn = gz W[DI:]^T; db, dbc, dtheta ride along as column sums.
// MFMA operand map, the weight-gradient accumulators and the slab: as in hop_mlp.hip.
#include "mfma_tile.h"

namespace kpgnn {
namespace {

constexpr float kNormEps = 1e-12f;   // F.normalize's eps

struct StParams {
    int64_t N, tiles;
    int K, DI, DO, H, LD, Hp;    // H = 0: no projection; Hp = LDS pitch of the transposed projection weight
    int vec_i, vec_o, vec_h, vec_g;   // 16-B staging allowed for x/xn/gx/gxn, y, out/gout[N,H], gout[N,K,DO]
    const float *x, *xn, *w, *b, *theta, *wc, *bc;
    float *y, *rinv, *out;       // fwd: y / rinv may both be NULL (nothing is saved)
    const float* gout;
    float *gx, *gxn;
    float* slab;                 // [gridDim.x][slab_w]
    int64_t slab_w;
};

__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

// ---------------------------------------------------------------------------------------------------------- forward
template <int T>
__global__ void __launch_bounds__(kHmThreads)
sage_tail_fwd_kernel(const StParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int P = 16 * T, PP = P * P, CP = P + 4;
    const int K = p.K, DI = p.DI, DO = p.DO, H = p.H, LD = p.LD, Hp = p.Hp;
    const int Dm = DI > DO ? DI : DO;
    float* wl = lds;                  // [K][2][P][P]  wl[k][h][i][j] = W[k][h * DI + i][j]
    float* bl = wl + 2 * K * PP;      // [K][P]
    float* th = bl + K * P;           // [K][P]
    float* wct = th + K * P;          // [P][Hp]    wct[j][o] = Wc[o][j]   (H > 0)
    float* bcl = wct + (H ? P * Hp : 0);   // [Hp]
    float* cmb = bcl + (H ? Hp : 0);  // [kTN][CP]
    float* rin = cmb + kTN * CP;      // [kTN][K]   1 / max(|relu(z)|, eps)
    float* bufX = rin + kTN * K;      // [kTN][LD]  x, then y
    float* bufN = bufX + kTN * LD;    // [kTN][LD]  xn, then out
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;

    for (int idx = tid; idx < 2 * K * PP; idx += kHmThreads) {
        const int k = idx / (2 * PP), r = idx - k * 2 * PP, h = r / PP, r2 = r - h * PP, i = r2 / P, j = r2 - i * P;
        wl[idx] = (i < DI && j < DO) ? p.w[((int64_t)k * 2 * DI + h * DI + i) * DO + j] : 0.f;
    }
    for (int idx = tid; idx < K * P; idx += kHmThreads) {
        const int k = idx / P, j = idx - k * P;
        bl[idx] = j < DO ? p.b[k * DO + j] : 0.f;
        th[idx] = (p.theta && j < DO) ? p.theta[k * DO + j] : 0.f;
    }
    if (H) {
        for (int idx = tid; idx < P * Hp; idx += kHmThreads) {
            const int j = idx / Hp, o = idx - j * Hp;
            wct[idx] = (j < DO && o < H) ? p.wc[(int64_t)o * DO + j] : 0.f;
        }
        for (int o = tid; o < Hp; o += kHmThreads) bcl[o] = (o < H && p.bc) ? p.bc[o] : 0.f;
    }
    const int ncol_i = K * DI, ncol_o = K * DO;
    TileIO io_i, io_o, io_h;
    io_i.init(ncol_i, DI, Dm, LD, p.vec_i);
    io_o.init(ncol_o, DO, Dm, LD, p.vec_o);
    io_h.init(H ? H : 4, H ? H : 4, H ? H : 4, LD, p.vec_h);
    float4 pfx[kNPF], pfn[kNPF];
    if ((int64_t)blockIdx.x < p.tiles) {
        const int64_t n0 = (int64_t)blockIdx.x * kTN;
        const int rows = (int)((p.N - n0) < kTN ? (p.N - n0) : kTN);
        io_i.issue(pfx, p.x + n0 * ncol_i, rows);
        io_i.issue(pfn, p.xn + n0 * ncol_i, rows);
    }
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t n0 = tile * kTN;
        const int rows = (int)((p.N - n0) < kTN ? (p.N - n0) : kTN);
        __syncthreads();                                        // previous tile's readers; first pass: the weight fill
        io_i.commit(pfx, bufX, p.x + n0 * ncol_i, rows);
        io_i.commit(pfn, bufN, p.xn + n0 * ncol_i, rows);
        __syncthreads();
        {
            const int64_t nt = tile + gridDim.x;
            if (nt < p.tiles) {
                const int64_t m0 = nt * kTN;
                const int nrows = (int)((p.N - m0) < kTN ? (p.N - m0) : kTN);
                io_i.issue(pfx, p.x + m0 * ncol_i, nrows);
                io_i.issue(pfn, p.xn + m0 * ncol_i, nrows);
            }
        }
        for (int k = wave; k < K; k += kHmWaves) {              // slot k (x) -> slot k (y), in place
            f32x4 acc[2][T];
#pragma unroll
            for (int jt = 0; jt < T; ++jt) { const float b = bl[k * P + jt * 16 + lr]; acc[0][jt] = {b, b, b, b}; acc[1][jt] = acc[0][jt]; }
            tile_times_weights<T>(acc, bufX, k * Dm, DI, wl + k * 2 * PP, P, LD, lr, lq);
            tile_times_weights<T>(acc, bufN, k * Dm, DI, wl + k * 2 * PP + PP, P, LD, lr, lq);
            // (padded columns: zero weights and a zero bias give z = 0 there, so they add nothing to the norm)
#pragma unroll
            for (int rg = 0; rg < 2; ++rg) {
                float ss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int jt = 0; jt < T; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = relu_keep_nan(acc[rg][jt][r]);
                        acc[rg][jt][r] = v;
                        ss[r] = fmaf(v, v, ss[r]);
                    }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int m = 1; m < 16; m <<= 1) ss[r] += __shfl_xor(ss[r], m, 16);   // the row's 16 column lanes
                    // y = r / max(nrm, eps) by division, as F.normalize does: a row with one positive entry gives exactly 1
                    // (sqrt(v * v) == v), and then its gradient cancels exactly in the backward instead of leaving
                    // rinv * ulp * gy - which a row with a tiny norm would blow up
                    const float nrm = sqrtf(ss[r]);
                    const float den = nrm > kNormEps ? nrm : kNormEps;
                    const int row = rg * 16 + 4 * lq + r;
                    if (lr == 0) rin[row * K + k] = 1.f / den;     // (clamped: exactly 1 / eps, the backward tests for it)
#pragma unroll
                    for (int jt = 0; jt < T; ++jt) {
                        const int col = jt * 16 + lr;
                        if (col < DO) bufX[row * LD + k * Dm + col] = acc[rg][jt][r] / den;
                    }
                }
            }
        }
        __syncthreads();
        if (p.y) {
            io_o.store(p.y + n0 * ncol_o, bufX, rows);
            for (int c = tid; c < rows * K; c += kHmThreads) p.rinv[n0 * K + c] = rin[c];
        }
        if (p.theta) {                                          // comb[n, j] = sum_k theta[k, j] y[n, k, j]
            for (int c = tid; c < kTN * DO; c += kHmThreads) {
                const int node = c / DO, j = c - node * DO;
                const float* yrow = bufX + node * LD + j;
                float acc = 0.f;
                for (int k = 0; k < K; ++k) acc = fmaf(th[k * P + j], yrow[k * Dm], acc);
                if (H) cmb[node * CP + j] = acc;
                else if (node < rows) p.out[(n0 + node) * DO + j] = acc;
            }
        }
        if (H) {                                                // out = comb Wc^T + bc, staged through xn's buffer
            __syncthreads();
            const int not16 = (H + 15) >> 4;
            for (int ot = wave; ot < not16; ot += kHmWaves) {
                f32x4 acc[2][1];
                const float b = bcl[ot * 16 + lr];
                acc[0][0] = {b, b, b, b}; acc[1][0] = acc[0][0];
                tile_times_weights<1>(acc, cmb, 0, DO, wct + ot * 16, Hp, CP, lr, lq);
                const int col = ot * 16 + lr;
                if (col < H)
#pragma unroll
                    for (int rg = 0; rg < 2; ++rg)
#pragma unroll
                        for (int r = 0; r < 4; ++r) bufN[(rg * 16 + 4 * lq + r) * LD + col] = acc[rg][0][r];
            }
            __syncthreads();
            io_h.store(p.out + n0 * H, bufN, rows);
        }
    }
}

// --------------------------------------------------------------------------------------------------------- backward
// (MAXI = 8: 96 accumulator registers next to two tiles in flight do not fit 256 registers without scratch, so those
//  instantiations take one block per CU; the plan sizes the grid with the same figure)
constexpr int bwd_blocks(int maxi) { return maxi == 8 ? 1 : 2; }

template <int T, int MAXI>
__global__ void __launch_bounds__(kHmThreads, bwd_blocks(MAXI))
sage_tail_bwd_kernel(const StParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int P = 16 * T, PP = P * P, TT = T * T, CP = P + 4, PC = (T == 1) ? 16 : 48;
    const int K = p.K, DI = p.DI, DO = p.DO, H = p.H, LD = p.LD;
    const int Dm = DI > DO ? DI : DO;
    const int H4 = (H + 3) & ~3;
    float* wt = lds;                  // [K][2][P][P]  wt[k][h][j][i] = W[k][h * DI + i][j]
    float* th = wt + 2 * K * PP;      // [K][P]
    float* wcn = th + K * P;          // [H4][PC]   wcn[o][j] = Wc[o][j]   (H > 0)
    float* cmb = wcn + (H ? H4 * PC : 0);   // [kTN][CP]  comb
    float* gcm = cmb + kTN * CP;      // [kTN][CP]  d(comb)
    float* rin = gcm + kTN * CP;      // [kTN][K]
    float* bufG = rin + kTN * K;      // [kTN][LD]  y, then gz
    float* bufX = bufG + kTN * LD;    // [kTN][LD]  x, then gx
    float* bufN = bufX + kTN * LD;    // [kTN][LD]  gout, then xn, then gxn
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;

    for (int idx = tid; idx < 2 * K * PP; idx += kHmThreads) {
        const int k = idx / (2 * PP), r = idx - k * 2 * PP, h = r / PP, r2 = r - h * PP, j = r2 / P, i = r2 - j * P;
        wt[idx] = (i < DI && j < DO) ? p.w[((int64_t)k * 2 * DI + h * DI + i) * DO + j] : 0.f;
    }
    for (int idx = tid; idx < K * P; idx += kHmThreads) {
        const int k = idx / P, j = idx - k * P;
        th[idx] = (p.theta && j < DO) ? p.theta[k * DO + j] : 0.f;
    }
    if (H)
        for (int idx = tid; idx < H4 * PC; idx += kHmThreads) {
            const int o = idx / PC, j = idx - o * PC;
            wcn[idx] = (o < H && j < DO) ? p.wc[(int64_t)o * DO + j] : 0.f;
        }
    const int ncol_i = K * DI, ncol_o = K * DO;
    const bool plain = p.theta == nullptr;           // gout is [N,K,DO]
    const int gcols = H ? H : ncol_o;                // row width of a gout tile staged in bufN (H, or plain mode)
    TileIO io_i, io_o, io_g;
    io_i.init(ncol_i, DI, Dm, LD, p.vec_i);
    io_o.init(ncol_o, DO, Dm, LD, p.vec_o);
    if (H) io_g.init(H, H, H, LD, p.vec_h);
    else io_g.init(ncol_o, DO, Dm, LD, p.vec_g);
    const bool gtile = H || plain;
    ColMap cm, ch;
    cm.init(ncol_o);
    ch.init(H ? H : 1);
    float gb[kMaxCols], gth[kMaxCols], gbc[kMaxCols];
#pragma unroll
    for (int m = 0; m < kMaxCols; ++m) gb[m] = gth[m] = gbc[m] = 0.f;
    const int nitems = K * TT;
    const int not16 = (H + 15) >> 4, nitems_c = not16 * T;
    f32x4 accA[MAXI], accB[MAXI], accC[MAXI];        // dW[k][:DI], dW[k][DI:], dWc
#pragma unroll
    for (int m = 0; m < MAXI; ++m) { accA[m] = {0.f, 0.f, 0.f, 0.f}; accB[m] = accA[m]; accC[m] = accA[m]; }
    const float rinv_clamped = 1.f / kNormEps;       // what the forward saved where the norm was below eps

    float4 r1[kNPF], r2[kNPF];        // tiles in flight: r1 = gout -> x, r2 = y -> xn
    if ((int64_t)blockIdx.x < p.tiles) {
        const int64_t n0 = (int64_t)blockIdx.x * kTN;
        const int rows = (int)((p.N - n0) < kTN ? (p.N - n0) : kTN);
        if (gtile) io_g.issue(r1, p.gout + n0 * gcols, rows);
        io_o.issue(r2, p.y + n0 * ncol_o, rows);
    }
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t n0 = tile * kTN;
        const int rows = (int)((p.N - n0) < kTN ? (p.N - n0) : kTN);
        // (the coordinates of the weight-gradient tiles are recomputed per tile, as in hop_mlp_bwd_kernel)
        int wv = __builtin_amdgcn_readfirstlane(wave);
        asm volatile("" : "+s"(wv));
        __syncthreads();
        if (gtile) io_g.commit(r1, bufN, p.gout + n0 * gcols, rows);
        io_o.commit(r2, bufG, p.y + n0 * ncol_o, rows);
        for (int c = tid; c < kTN * K; c += kHmThreads) rin[c] = c < rows * K ? p.rinv[n0 * K + c] : 0.f;
        if (!gtile)                                             // theta without projection: gout [N, DO] is d(comb)
            for (int c = tid; c < kTN * DO; c += kHmThreads) {
                const int n = c / DO, j = c - n * DO;
                gcm[n * CP + j] = n < rows ? p.gout[(n0 + n) * DO + j] : 0.f;
            }
        __syncthreads();
        io_i.issue(r1, p.x + n0 * ncol_i, rows);
        io_i.issue(r2, p.xn + n0 * ncol_i, rows);
        if (H) {
            // comb (needed by dWc), d(comb) = gout Wc, dbc
            for (int c = tid; c < kTN * DO; c += kHmThreads) {
                const int n = c / DO, j = c - n * DO;
                const float* yrow = bufG + n * LD + j;
                float a = 0.f;
                for (int k = 0; k < K; ++k) a = fmaf(th[k * P + j], yrow[k * Dm], a);
                cmb[n * CP + j] = a;
            }
            if (wv < T) {                                       // wave jt: both row groups, K-dim = the H outputs
                f32x4 acc[2][1];
                acc[0][0] = {0.f, 0.f, 0.f, 0.f}; acc[1][0] = acc[0][0];
                tile_times_weights<1>(acc, bufN, 0, H, wcn + wv * 16, PC, LD, lr, lq);
                const int col = wv * 16 + lr;
                if (col < DO)
#pragma unroll
                    for (int rg = 0; rg < 2; ++rg)
#pragma unroll
                        for (int r = 0; r < 4; ++r) gcm[(rg * 16 + 4 * lq + r) * CP + col] = acc[rg][0][r];
            }
            if (ch.on) {
#pragma unroll
                for (int m = 0; m < kMaxCols; ++m) {
                    const int c = ch.c0 + m * kHmThreads;
                    if (c < H)
#pragma unroll 4
                        for (int n = ch.rl; n < kTN; n += ch.R) gbc[m] += bufN[n * LD + c];
                }
            }
            __syncthreads();
            // dWc[o][j] += sum_n gout[n][o] comb[n][j]
#pragma unroll
            for (int m = 0; m < MAXI; ++m) {
                const int it = wv + m * kHmWaves;
                if (it < nitems_c) {
                    const int ot = it / T, jt = it - ot * T;
                    const int ca = ot * 16 + lr, cb = jt * 16 + lr;
                    const float* pa = bufN + (ca < H ? ca : H - 1) + lq * LD;
                    const float* pb = cmb + (cb < DO ? cb : DO - 1) + lq * CP;
#pragma unroll 4
                    for (int q = 0; q < kTN / 4; ++q) {
                        float a = pa[4 * q * LD], b = pb[4 * q * CP];
                        a = ca < H ? a : 0.f;
                        b = cb < DO ? b : 0.f;
                        accC[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, accC[m], 0, 0, 0);
                    }
                }
            }
        }
        // A. dtheta column sums: dtheta[k][j] += d(comb)[n][j] y[n][k][j]
        if (!plain && cm.on) {
#pragma unroll
            for (int m = 0; m < kMaxCols; ++m) {
                const int c = cm.c0 + m * kHmThreads;
                if (c < ncol_o) {
                    const int k = c / DO, j = c - k * DO, lc = k * Dm + j;
#pragma unroll 4
                    for (int n = cm.rl; n < kTN; n += cm.R) gth[m] = fmaf(gcm[n * CP + j], bufG[n * LD + lc], gth[m]);
                }
            }
        }
        __syncthreads();
        // B. one thread per (node, hop) row: gz = rinv (gy - y <gy, y>) [y > 0], in place over y.  Where the forward's
        //    clamp was active y = r / eps and the projection term is absent; an all-zero row gives gz = 0 through [y > 0].
        for (int pr = tid; pr < kTN * K; pr += kHmThreads) {
            const int n = pr / K, k = pr - n * K;
            float* yrow = bufG + n * LD + k * Dm;
            const float* grow = plain ? bufN + n * LD + k * Dm : gcm + n * CP;
            const float* trow = th + k * P;
            const float ri = rin[pr];
            float dot = 0.f;
            for (int j = 0; j < DO; ++j) {
                const float gy = plain ? grow[j] : grow[j] * trow[j];
                dot = fmaf(gy, yrow[j], dot);
            }
            dot = ri >= rinv_clamped ? 0.f : dot;
            for (int j = 0; j < DO; ++j) {
                const float gy = plain ? grow[j] : grow[j] * trow[j];
                const float yv = yrow[j];
                yrow[j] = yv > 0.f ? ri * (gy - yv * dot) : 0.f;
            }
        }
        io_i.commit(r1, bufX, p.x + n0 * ncol_i, rows);        // (bufX: the previous tile's gx left at the top barrier)
        __syncthreads();
        io_i.commit(r2, bufN, p.xn + n0 * ncol_i, rows);       // gout is dead: xn takes its place
        {
            const int64_t nt = tile + gridDim.x;
            if (nt < p.tiles) {
                const int64_t m0 = nt * kTN;
                const int nrows = (int)((p.N - m0) < kTN ? (p.N - m0) : kTN);
                if (gtile) io_g.issue(r1, p.gout + m0 * gcols, nrows);
                io_o.issue(r2, p.y + m0 * ncol_o, nrows);
            }
        }
        __syncthreads();
        // C. dW[k][:DI] += x_k^T gz_k, dW[k][DI:] += xn_k^T gz_k ; db column sums
#pragma unroll
        for (int m = 0; m < MAXI; ++m) {
            const int it = wv + m * kHmWaves;
            if (it < nitems) {
                const int k = it / TT, tt = it - k * TT, ti = tt / T, tj = tt - ti * T;
                const int ca = ti * 16 + lr, cb = tj * 16 + lr;
                const int oa = k * Dm + (ca < DI ? ca : DI - 1) + lq * LD;
                const float* pa = bufX + oa;
                const float* pn = bufN + oa;
                const float* pb = bufG + k * Dm + (cb < DO ? cb : DO - 1) + lq * LD;
#pragma unroll 4
                for (int q = 0; q < kTN / 4; ++q) {
                    float a = pa[4 * q * LD], an = pn[4 * q * LD], b = pb[4 * q * LD];
                    a = ca < DI ? a : 0.f;
                    an = ca < DI ? an : 0.f;
                    b = cb < DO ? b : 0.f;
                    accA[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, accA[m], 0, 0, 0);
                    accB[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(an, b, accB[m], 0, 0, 0);
                }
            }
        }
        if (cm.on) {
#pragma unroll
            for (int m = 0; m < kMaxCols; ++m) {
                const int c = cm.c0 + m * kHmThreads;
                if (c < ncol_o) {
                    const int k = c / DO, lc = k * Dm + (c - k * DO);
#pragma unroll 4
                    for (int n = cm.rl; n < kTN; n += cm.R) gb[m] += bufG[n * LD + lc];
                }
            }
        }
        __syncthreads();
        // D. gx = gz W[:DI]^T -> bufX (over x), gxn = gz W[DI:]^T -> bufN (over xn); a hop slot belongs to one wave
        for (int k = wv; k < K; k += kHmWaves) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x4 acc[2][T];
#pragma unroll
                for (int ti = 0; ti < T; ++ti) { acc[0][ti] = {0.f, 0.f, 0.f, 0.f}; acc[1][ti] = acc[0][ti]; }
                tile_times_weights<T>(acc, bufG, k * Dm, DO, wt + k * 2 * PP + h * PP, P, LD, lr, lq);
                float* dst = h ? bufN : bufX;
#pragma unroll
                for (int rg = 0; rg < 2; ++rg)
#pragma unroll
                    for (int ti = 0; ti < T; ++ti) {
                        const int col = ti * 16 + lr;
                        if (col < DI)
#pragma unroll
                            for (int r = 0; r < 4; ++r) dst[(rg * 16 + 4 * lq + r) * LD + k * Dm + col] = acc[rg][ti][r];
                    }
            }
        }
        __syncthreads();
        io_i.store(p.gx + n0 * ncol_i, bufX, rows);
        io_i.store(p.gxn + n0 * ncol_i, bufN, rows);
    }

    // per-block partials -> slab row [dW | db | dtheta | dWc | dbc]
    float* row = p.slab + (int64_t)blockIdx.x * p.slab_w;
    const int64_t o_b = (int64_t)K * 2 * DI * DO, o_th = o_b + ncol_o;
    const int64_t o_wc = o_th + (p.theta ? ncol_o : 0), o_bc = o_wc + (int64_t)H * DO;
#pragma unroll
    for (int m = 0; m < MAXI; ++m) {
        const int it = wave + m * kHmWaves;
        if (it < nitems) {
            const int k = it / TT, tt = it - k * TT, ti = tt / T, tj = tt - ti * T;
            const int j = tj * 16 + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ti * 16 + 4 * lq + r;
                if (i < DI && j < DO) {
                    row[((int64_t)k * 2 * DI + i) * DO + j] = accA[m][r];
                    row[((int64_t)k * 2 * DI + DI + i) * DO + j] = accB[m][r];
                }
            }
        }
        if (it < nitems_c) {
            const int ot = it / T, jt = it - ot * T;
            const int j = jt * 16 + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = ot * 16 + 4 * lq + r;
                if (o < H && j < DO) row[o_wc + (int64_t)o * DO + j] = accC[m][r];
            }
        }
    }
    // column sums: the row lanes of a column meet in LDS (bufG is free after the barrier)
    for (int which = 0; which < 3; ++which) {
        if (which == 1 && !p.theta) continue;
        if (which == 2 && !H) continue;
        const ColMap& mp = which == 2 ? ch : cm;
        const int ncol = which == 2 ? H : ncol_o;
        __syncthreads();
        if (mp.on) {
#pragma unroll
            for (int m = 0; m < kMaxCols; ++m) {
                const int c = mp.c0 + m * kHmThreads;
                if (c < ncol) bufG[mp.rl * ncol + c] = which == 0 ? gb[m] : (which == 1 ? gth[m] : gbc[m]);
            }
        }
        __syncthreads();
        const int64_t off = which == 0 ? o_b : (which == 1 ? o_th : o_bc);
        for (int c = tid; c < ncol; c += kHmThreads) {
            float tot = 0.f;
            for (int r = 0; r < mp.R; ++r) tot += bufG[r * ncol + c];
            row[off + c] = tot;
        }
    }
}

struct StPlan { int T, maxi, LD, Hp, grid_fwd, grid_bwd; size_t lds_fwd, lds_bwd; int64_t slab_w; };

int st_plan(int64_t N, int K, int DI, int DO, int H, bool theta, StPlan* pl) {
    const int D = DI > DO ? DI : DO;
    if (D > 32) return fail(KPGNN_ELIMIT, "sage_tail: per-hop width %d exceeds 32", D);
    if (H < 0 || H > 1024) return fail(KPGNN_ELIMIT, "sage_tail: projection width %d exceeds 1024", H);
    const int T = (D + 15) / 16;
    pl->T = T;
    if (K > 8 * kHmWaves) return fail(KPGNN_ELIMIT, "sage_tail: K=%d exceeds %d", K, 8 * kHmWaves);
    int items = K * T * T;
    const int items_c = ((H + 15) / 16) * T;
    if (items_c > items) items = items_c;
    if (items > 8 * kHmWaves) return fail(KPGNN_ELIMIT, "sage_tail: %d weight-gradient tiles exceed %d", items, 8 * kHmWaves);
    pl->maxi = items <= 2 * kHmWaves ? 2 : (items <= 4 * kHmWaves ? 4 : 8);
    if ((int64_t)K * D > (int64_t)kMaxCols * kHmThreads)
        return fail(KPGNN_ELIMIT, "sage_tail: K*D=%lld exceeds %d", (long long)K * D, kMaxCols * kHmThreads);
    int v = K * D;
    if (H > v) v = H;
    pl->LD = mfma_pitch(v);
    int Hp = (H + 15) & ~15;
    if (Hp % 32 == 0) Hp += 16;                              // pitch = 16 (mod 32): the 4 k-rows of a B read are 16 banks apart
    pl->Hp = H ? Hp : 0;
    const size_t P = 16 * (size_t)T, CP = P + 4, PC = T == 1 ? 16 : 48, H4 = (size_t)((H + 3) & ~3);
    pl->lds_fwd = sizeof(float) * (2 * K * P * P + 2 * K * P + (H ? P * Hp + Hp : 0) + kTN * CP + (size_t)kTN * K +
                                   2 * (size_t)kTN * pl->LD);
    pl->lds_bwd = sizeof(float) * (2 * K * P * P + K * P + (H ? H4 * PC : 0) + 2 * kTN * CP + (size_t)kTN * K +
                                   3 * (size_t)kTN * pl->LD);
    const size_t cap = (size_t)device_facts().lds_per_block;
    if (pl->lds_fwd > cap || pl->lds_bwd > cap)
        return fail(KPGNN_ELIMIT, "sage_tail: %zu B of LDS needed", pl->lds_fwd > pl->lds_bwd ? pl->lds_fwd : pl->lds_bwd);
    const int64_t tiles = (N + kTN - 1) / kTN;
    const int cu = device_facts().cu_count;
    auto grid_for = [&](size_t lds, int reg_blocks) {
        int per_cu = (int)(cap / lds);
        per_cu = per_cu < 1 ? 1 : (per_cu > reg_blocks ? reg_blocks : per_cu);
        int64_t g = (int64_t)cu * per_cu;
        if (g > tiles) g = tiles;
        return (int)(g < 1 ? 1 : g);
    };
    pl->grid_fwd = grid_for(pl->lds_fwd, 8);
    pl->grid_bwd = grid_for(pl->lds_bwd, bwd_blocks(pl->maxi));
    pl->slab_w = (int64_t)K * 2 * DI * DO + (int64_t)K * DO + (theta ? (int64_t)K * DO : 0) + (int64_t)H * DO + H;
    return KPGNN_OK;
}

void st_fill(const kpgnn_sage_tail_desc* d, const StPlan& pl, StParams* p) {
    p->N = d->N; p->tiles = (d->N + kTN - 1) / kTN;
    p->K = d->K; p->DI = d->DI; p->DO = d->DO; p->H = d->H; p->LD = pl.LD; p->Hp = pl.Hp;
    p->x = d->x; p->xn = d->xn; p->w = d->w; p->b = d->b; p->theta = d->theta; p->wc = d->wc; p->bc = d->bc;
    p->y = d->y; p->rinv = d->rinv; p->out = d->out; p->gout = d->gout; p->gx = d->gx; p->gxn = d->gxn;
    p->slab = (float*)d->workspace; p->slab_w = pl.slab_w;
    auto al16 = [](const void* q) { return (((uintptr_t)q) & 15) == 0; };   // (NULL counts as aligned: it is not accessed)
    // (tiles start at multiples of 32 rows, so a row width that is a multiple of 4 floats keeps every tile 16-B aligned)
    p->vec_i = ((d->K * d->DI) % 4 == 0) && al16(d->x) && al16(d->xn) && al16(d->gx) && al16(d->gxn);
    p->vec_o = ((d->K * d->DO) % 4 == 0) && al16(d->y);
    p->vec_h = d->H > 0 && (d->H % 4 == 0) && al16(d->out) && al16(d->gout);
    p->vec_g = ((d->K * d->DO) % 4 == 0) && al16(d->gout);
}

int st_check(const kpgnn_sage_tail_desc* d, const char* who) {
    KPGNN_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
    KPGNN_REQUIRE(d->N >= 0 && d->K >= 1 && d->DI >= 1 && d->DO >= 1 && d->H >= 0, "%s: bad N=%lld K=%d DI=%d DO=%d H=%d", who,
                  (long long)d->N, d->K, d->DI, d->DO, d->H);
    KPGNN_REQUIRE(d->x && d->xn && d->w && d->b, "%s: NULL tensor", who);
    KPGNN_REQUIRE((d->H > 0) == (d->wc != nullptr), "%s: H > 0 goes with wc, H = 0 with none", who);
    KPGNN_REQUIRE(d->wc == nullptr || d->theta != nullptr, "%s: the projection (wc) needs theta", who);
    return KPGNN_OK;
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" size_t kpgnn_sage_tail_workspace_bytes(int64_t N, int32_t K, int32_t DI, int32_t DO, int32_t H) {
    StPlan pl;
    if (N < 1 || K < 1 || DI < 1 || DO < 1 || H < 0) return 0;
    if (st_plan(N, K, DI, DO, H, true, &pl) != KPGNN_OK) return 0;  // 0 = "not covered": the caller keeps the framework tail
    return sizeof(float) * (size_t)pl.grid_bwd * (size_t)pl.slab_w;
}

extern "C" int kpgnn_sage_tail_fwd(const kpgnn_sage_tail_desc* d, kpgnn_stream_t stream) {
    if (int rc = st_check(d, "kpgnn_sage_tail_fwd")) return rc;
    KPGNN_REQUIRE(!d->theta || d->out, "kpgnn_sage_tail_fwd: theta without out");
    KPGNN_REQUIRE((d->y != nullptr) == (d->rinv != nullptr), "kpgnn_sage_tail_fwd: y and rinv go together");
    KPGNN_REQUIRE(d->theta || d->y, "kpgnn_sage_tail_fwd: without theta y is the result and may not be NULL");
    if (d->N == 0) return KPGNN_OK;
    StPlan pl;
    if (int rc = st_plan(d->N, d->K, d->DI, d->DO, d->H, d->theta != nullptr, &pl)) return rc;
    StParams p;
    st_fill(d, pl, &p);
    hipStream_t s = (hipStream_t)stream;
    // (persistent tile loop: the grid is one resident round - the plan sizes it by LDS, the registers may allow fewer)
    auto one_round = [&](int nb, int grid) {
        const int64_t cap = (int64_t)nb * device_facts().cu_count;
        return nb > 0 && cap < grid ? (int)cap : grid;
    };
    if (pl.T == 1) {
        KPGNN_HIP_TRY(ensure_dynamic_lds((const void*)sage_tail_fwd_kernel<1>, pl.lds_fwd));
        const int grid = one_round(resident_blocks(sage_tail_fwd_kernel<1>, kHmThreads, pl.lds_fwd), pl.grid_fwd);
        hipLaunchKernelGGL(sage_tail_fwd_kernel<1>, dim3(grid), dim3(kHmThreads), pl.lds_fwd, s, p);
    } else {
        KPGNN_HIP_TRY(ensure_dynamic_lds((const void*)sage_tail_fwd_kernel<2>, pl.lds_fwd));
        const int grid = one_round(resident_blocks(sage_tail_fwd_kernel<2>, kHmThreads, pl.lds_fwd), pl.grid_fwd);
        hipLaunchKernelGGL(sage_tail_fwd_kernel<2>, dim3(grid), dim3(kHmThreads), pl.lds_fwd, s, p);
    }
    KPGNN_LAUNCH_CHECK("sage_tail_fwd_kernel");
    return KPGNN_OK;
}

extern "C" int kpgnn_sage_tail_bwd(const kpgnn_sage_tail_desc* d, kpgnn_stream_t stream) {
    if (int rc = st_check(d, "kpgnn_sage_tail_bwd")) return rc;
    KPGNN_REQUIRE(d->y && d->rinv, "kpgnn_sage_tail_bwd: NULL saved tensor (y, rinv)");
    KPGNN_REQUIRE(d->gout && d->gx && d->gxn && d->gflat, "kpgnn_sage_tail_bwd: NULL gradient tensor");
    StPlan pl;
    if (int rc = st_plan(d->N > 0 ? d->N : 1, d->K, d->DI, d->DO, d->H, d->theta != nullptr, &pl)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (d->N == 0) {
        KPGNN_HIP_TRY(hipMemsetAsync(d->gflat, 0, sizeof(float) * (size_t)pl.slab_w, s));
        return KPGNN_OK;
    }
    KPGNN_REQUIRE(d->workspace && d->workspace_bytes >= sizeof(float) * (size_t)pl.grid_bwd * (size_t)pl.slab_w,
                  "kpgnn_sage_tail_bwd: workspace too small");
    StParams p;
    st_fill(d, pl, &p);
#define KP_ST_BWD(TV, MV) do { \
        KPGNN_HIP_TRY(ensure_dynamic_lds((const void*)sage_tail_bwd_kernel<TV, MV>, pl.lds_bwd)); \
        hipLaunchKernelGGL((sage_tail_bwd_kernel<TV, MV>), dim3(pl.grid_bwd), dim3(kHmThreads), pl.lds_bwd, s, p); } while (0)
    if (pl.T == 1) {
        if (pl.maxi == 2) KP_ST_BWD(1, 2); else if (pl.maxi == 4) KP_ST_BWD(1, 4); else KP_ST_BWD(1, 8);
    } else {
        if (pl.maxi == 2) KP_ST_BWD(2, 2); else if (pl.maxi == 4) KP_ST_BWD(2, 4); else KP_ST_BWD(2, 8);
    }
#undef KP_ST_BWD
    KPGNN_LAUNCH_CHECK("sage_tail_bwd_kernel");
    return slab_reduce(p.slab, pl.grid_bwd, pl.slab_w, d->gflat, pl.slab_w, nullptr, 0, nullptr, s);
}
