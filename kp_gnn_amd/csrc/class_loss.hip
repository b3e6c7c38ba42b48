// Negative log-likelihood of a batch of logits, its gradient and the count of correct predictions in one launch (gfx950).
// Contract: include/kpgnn.h, kpgnn_nll_loss.
//
// The classification scripts end a step with  F.nll_loss(F.log_softmax(model(data), dim=-1), y)  (train_TU.py:45-46,
// train_EXP.py:81-82) or  nn.CrossEntropyLoss()  (train_CSL.py:41, train_SR.py:38), and count  pred.eq(y).sum()  in val() /
// test() (train_TU.py:66-67).  As framework ops that is a softmax, a gather, a mean and their three backward launches for
// a few thousand numbers.  One block, as regression_loss_kernel: a sub-group of lanes owns a row (row maximum, sum of
// exponentials and arg-max by a fixed butterfly), every sub-group sums its rows in row order, the 1024 partials meet in LDS
// (fixed tree): bitwise reproducible.  The mean's denominator (rows with a label inside [0, C)) is counted first, so
// the gradient is written already scaled.
// Sized for graph-level row counts (a few thousand rows, as regression_loss_kernel): the one block reads y twice and the logits
// three times (row maximum, sum of exponentials, gradient; the re-reads hit the cache).  Node-level losses over tens of
// thousands of rows run correctly, on one CU.  M = 0 is accepted like the other heads' entries: a sum of 0, a mean of 0 / 0.
#include "kpgnn_common.h"

namespace kpgnn {
namespace {

constexpr int kLossBlock = 1024;

struct LossParams {
    const int32_t* n_dyn;
    int64_t M; int C, mean, L;             // L: lanes of a row's sub-group (power of two, 1 .. 64)
    const float* logits; int64_t ls;
    const int64_t* y;
    float* loss; float* dl; int64_t dls;
    int32_t* correct;
};

__device__ __forceinline__ int block_sum_int(int v, int* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = kLossBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

__global__ void __launch_bounds__(kLossBlock) nll_loss_kernel(LossParams p) {
    __shared__ float red[kLossBlock];
    int* redi = reinterpret_cast<int*>(red);
    const int64_t M = live_rows(p.M, p.n_dyn);
    const int C = p.C, L = p.L;
    const int sl = threadIdx.x & (L - 1), sg = threadIdx.x / L, S = kLossBlock / L;

    // rows that count: a label outside [0, C) is skipped like ignore_index (kpgnn.h)
    int cnt = 0;
    for (int64_t m = threadIdx.x; m < M; m += kLossBlock) {
        const int64_t t = p.y[m];
        cnt += (t >= 0 && t < C) ? 1 : 0;
    }
    const int count = block_sum_int(cnt, redi);
    const float scale = p.mean ? 1.0f / (float)count : 1.0f;       // (count == 0: no row reads it)

    float lsum = 0.f;
    int right = 0;
    for (int64_t m = sg; m < M; m += S) {
        const float* row = p.logits + m * p.ls;
        const int64_t t = p.y[m];
        const bool ok = t >= 0 && t < C;
        if (!ok) {                                                   // (uniform over the sub-group)
            if (p.dl) for (int c = sl; c < C; c += L) p.dl[m * p.dls + c] = 0.f;
            continue;
        }
        float mx = -INFINITY;
        int am = 0;
        for (int c = sl; c < C; c += L) {
            const float v = row[c];
            if (v > mx) { mx = v; am = c; }                          // (the first of equal maxima, as the lanes' columns ascend)
        }
        for (int o = L >> 1; o > 0; o >>= 1) {
            const float omx = __shfl_xor(mx, o, 64);
            const int oam = __shfl_xor(am, o, 64);
            if (omx > mx || (omx == mx && oam < am)) { mx = omx; am = oam; }
        }
        float se = 0.f;
        for (int c = sl; c < C; c += L) se += expf(row[c] - mx);
        se = group_sum(se, L);
        const float lt = row[t];
        if (sl == 0) {
            lsum += (logf(se) + mx) - lt;
            right += (am == (int)t) ? 1 : 0;
        }
        if (p.dl) {
            const float inv = scale / se;
            for (int c = sl; c < C; c += L) {
                const float sm = expf(row[c] - mx) * inv;
                p.dl[m * p.dls + c] = (c == (int)t) ? sm - scale : sm;
            }
        }
    }
    __syncthreads();
    red[threadIdx.x] = lsum;
    __syncthreads();
    for (int w = kLossBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const float total = red[0];
    const int nright = p.correct ? block_sum_int(right, redi) : 0;
    if (threadIdx.x == 0) {
        *p.loss = p.mean ? total / (float)count : total;              // (no counted row: 0 / 0, the framework's NaN)
        if (p.correct) *p.correct = nright;
    }
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_nll_loss(const kpgnn_nll_loss_desc* d, kpgnn_stream_t stream) {
    KPGNN_REQUIRE(d != nullptr, "nll_loss: NULL descriptor");
    KPGNN_REQUIRE(d->M >= 0 && d->C >= 1, "nll_loss: bad M=%lld C=%d", (long long)d->M, d->C);
    KPGNN_REQUIRE(d->reduction == 0 || d->reduction == 1, "nll_loss: reduction must be 0 (mean) or 1 (sum)");
    KPGNN_REQUIRE(d->loss && (d->M == 0 || (d->logits && d->y)), "nll_loss: NULL logits/y/loss");
    KPGNN_REQUIRE(d->M == 0 || d->logits_stride >= d->C, "nll_loss: logits_stride=%lld below C=%d", (long long)d->logits_stride, d->C);
    KPGNN_REQUIRE(!d->dlogits || d->dlogits_stride >= d->C, "nll_loss: bad dlogits stride");
    if (d->C > 1024) return fail(KPGNN_ELIMIT, "nll_loss: C=%d exceeds 1024 classes", d->C);
    LossParams p = {};
    p.n_dyn = d->n_dyn; p.M = d->M; p.C = d->C; p.mean = d->reduction == 0;
    p.L = 1;
    while (p.L < d->C && p.L < kWave) p.L <<= 1;
    p.logits = d->logits; p.ls = d->logits_stride; p.y = d->y; p.loss = d->loss; p.dl = d->dlogits; p.dls = d->dlogits_stride;
    p.correct = d->correct;
    hipLaunchKernelGGL(nll_loss_kernel, dim3(1), dim3(kLossBlock), 0, (hipStream_t)stream, p);
    KPGNN_LAUNCH_CHECK("nll_loss_kernel");
    return KPGNN_OK;
}
