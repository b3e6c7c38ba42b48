// y = [outer(] relu(bn2(relu(bn1(x W0^T + b0)) W3^T + b3)) [)] [+ residual] with running statistics, one launch (gfx950).
// Contract: include/kpgnn.h, kpgnn_mlp_eval.
//
// In evaluation mode a BatchNorm1d is a per-column map, so - unlike the training path (lin_fused.h: three launches around
// column-statistics slots, two [N,H] round trips) - nothing needs a grid-wide reduction between the two Linears of the layers'
// MLP: a row tile stays resident from the read of x to the store of the result.
//
// Tile mechanics are lin_fused_kernel's: a 32M-row tile of x goes through LDS once, each wave keeps its 32-output strip of
// a weight as v_mfma_f32_32x32x2_f32 A-fragments - here of BOTH weights -, the next tile travels in registers
// (unconditional loads from clamped rows), the result leaves through the same buffer as whole rows.  Per tile:
//   x tile -> GEMM 1 -> (+ b0, bn1, relu) written back over the x tile in the accumulator layout -> GEMM 2 over that tile ->
//   (+ b3, bn2, relu, [outer norm]) written back -> coalesced row stores (+ residual, read coalesced as well).
// The per-column coefficients (mean, 1 / sqrt(var + eps), gamma, beta of the three norms, both biases) are formed by every block
// in its prologue and live in LDS behind the tile; the accumulator-layout phases fetch them as broadcast 16-B reads.
//
// Registers at I = O = 128: 64 + 64 for the two strips, 32 accumulators (M <= 2), 32 for the next tile, the rest addresses:
// 242 of the 256 that two blocks per CU leave a wave, no scratch (compiler's resource report; DESIGN.md, "Evaluation forward").
#include "lin_fused.h"      // KPGNN_BN_AFFINE, mfma_tile.h

namespace kpgnn {
namespace {

struct BnRun { const float* gamma; const float* beta; const float* mean; const float* var; float eps; };

struct MlpEvalParams {
    const int32_t* n_dyn;
    int64_t N; int pitch;
    const float* x; int64_t xs;
    const float* w0; const float* b0; const float* w3; const float* b3;
    BnRun bn[3];                      // bn1, bn2, outer (gamma NULL: absent)
    const float* res; int64_t rs;
    float* y; int64_t ys;
};

// coefficient rows in LDS, one value per output column: [3][4][O] = mean, invstd, gamma, beta of bn1 / bn2 / outer, then b0, b3
constexpr int kEvalCoefRows = 14;

template <int KSI, int KSO, int M>
__global__ void __launch_bounds__(256, 2)
mlp_eval_kernel(MlpEvalParams p) {
    p.N = live_rows(p.N, p.n_dyn);
    if (p.N <= 0) return;                             // (only under a dynamic count of zero)
    extern __shared__ __attribute__((aligned(16))) float xl[];      // [32*M][pitch] tile, then the coefficient rows
    constexpr int ROWS = 32 * M;
    constexpr int I = 2 * KSI, CGI = I / 4, RLI = 256 / CGI, NAI = CGI * RLI, PFI = (ROWS + RLI - 1) / RLI;
    constexpr int O = 2 * KSO, CGO = O / 4, RLO = 256 / CGO, NAO = CGO * RLO;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int kk = lane >> 5, c = lane & 31;
    const int pitch = p.pitch;
    float* co = xl + ROWS * pitch;
    const int o = wave * 32 + c;
    // this wave's strips of both weights as MFMA A-fragments: a[ks] = W[o][2 ks + kk]; every lane streams ITS row 16 B at a time
    float a0[KSI], a3[KSO];
#pragma unroll
    for (int j = 0; j < KSI / 2; ++j) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (O == 128 || o < O) v = ld4(p.w0 + (int64_t)o * I + 4 * j);
        a0[2 * j] = kk ? v.y : v.x;
        a0[2 * j + 1] = kk ? v.w : v.z;
    }
    // (a use of the strip in front of the loop: the wait for its loads happens here, once - lin_fused.h; and before the second
    //  strip's loads, so that only one strip's 16-B fetches, twice what is kept of them, are ever in flight)
#pragma unroll
    for (int ks = 0; ks < KSI; ++ks) asm volatile("" : "+v"(a0[ks]));
#pragma unroll
    for (int j = 0; j < KSO / 2; ++j) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (O == 128 || o < O) v = ld4(p.w3 + (int64_t)o * O + 4 * j);
        a3[2 * j] = kk ? v.y : v.x;
        a3[2 * j + 1] = kk ? v.w : v.z;
    }
#pragma unroll
    for (int ks = 0; ks < KSO; ++ks) asm volatile("" : "+v"(a3[ks]));
    // the per-column coefficients, from the running statistics as they are (read-only)
    if (tid < O) {                                    // (O <= 128 < the block)
#pragma unroll
        for (int n = 0; n < 3; ++n) {
            const BnRun& b = p.bn[n];
            if (b.gamma) {
                co[(4 * n + 0) * O + tid] = b.mean[tid];
                co[(4 * n + 1) * O + tid] = 1.0f / sqrtf(b.var[tid] + b.eps);
                co[(4 * n + 2) * O + tid] = b.gamma[tid];
                co[(4 * n + 3) * O + tid] = b.beta[tid];
            }
        }
        co[12 * O + tid] = p.b0 ? p.b0[tid] : 0.f;
        co[13 * O + tid] = p.b3 ? p.b3[tid] : 0.f;
    }
    const bool outer = p.bn[2].gamma != nullptr;
    // ---- input side: thread -> (column group, row lane); a tile is NAI float4s per row-lane step
    const int cgi = tid % CGI, rli = tid / CGI;
    const bool act_i = tid < NAI;
    const int64_t tiles = (p.N + ROWS - 1) / ROWS;
    float4 pf[PFI];
    // unconditional loads from rows clamped to N - 1 (lin_fused.h explains): what they bring only reaches tile rows that are
    // never stored
    const int64_t lastrow = p.N - 1;
    auto issue = [&](int64_t tl) {
        const int64_t r0 = tl * ROWS;
#pragma unroll
        for (int j = 0; j < PFI; ++j) {
            int64_t r = r0 + rli + j * RLI;
            r = r < lastrow ? r : lastrow;
            pf[j] = ld4(p.x + r * p.xs + 4 * cgi);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int j = 0; j < PFI; ++j)
            if (act_i && rli + j * RLI < ROWS) st4(xl + (rli + j * RLI) * pitch + 4 * cgi, pf[j]);
    };
    // ---- output side: the same mapping over the O / 4 column groups
    const int cgo = tid % CGO, rlo = tid / CGO;
    const bool act_o = tid < NAO;
    int64_t tile = blockIdx.x;
    if (tile < tiles) { issue(tile); commit(); }
    __syncthreads();                                   // the coefficient rows and the first tile are in place
    const float* bt0 = xl + c * pitch + kk;
    for (; tile < tiles; tile += gridDim.x) {
        const bool more = tile + gridDim.x < tiles;
        if (more) issue(tile + gridDim.x);
        f32x16 acc[M];
#pragma unroll
        for (int m = 0; m < M; ++m)
            for (int v = 0; v < 16; ++v) acc[m][v] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KSI; ++ks) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float xv = bt0[m * 32 * pitch + 2 * ks];
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[ks], xv, acc[m], 0, 0, 0);
            }
        }
        __syncthreads();                               // every wave is done reading the x tile: it becomes relu(bn1(.))
        // C/D map: col = lane & 31 (tile row), row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (output o)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ob = wave * 32 + 8 * q + 4 * kk;
            if (ob < O) {                              // O % 4 == 0: the 4 outputs of a group are in or out together
                const float4 bb = ld4(co + 12 * O + ob);
                const float4 mean = ld4(co + ob), istd = ld4(co + O + ob), g = ld4(co + 2 * O + ob), bt = ld4(co + 3 * O + ob);
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    float4 v = make_float4(acc[m][4 * q] + bb.x, acc[m][4 * q + 1] + bb.y, acc[m][4 * q + 2] + bb.z, acc[m][4 * q + 3] + bb.w);
                    KPGNN_BN_AFFINE(v)
                    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                    st4(xl + (m * 32 + c) * pitch + ob, v);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < M; ++m)
            for (int v = 0; v < 16; ++v) acc[m][v] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KSO; ++ks) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float xv = bt0[m * 32 * pitch + 2 * ks];
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3[ks], xv, acc[m], 0, 0, 0);
            }
        }
        __syncthreads();                               // the intermediate tile is consumed: it becomes the result
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ob = wave * 32 + 8 * q + 4 * kk;
            if (ob < O) {
                const float4 bb = ld4(co + 13 * O + ob);
                float4 v[M];
                {
                    const float4 mean = ld4(co + 4 * O + ob), istd = ld4(co + 5 * O + ob), g = ld4(co + 6 * O + ob), bt = ld4(co + 7 * O + ob);
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        v[m] = make_float4(acc[m][4 * q] + bb.x, acc[m][4 * q + 1] + bb.y, acc[m][4 * q + 2] + bb.z, acc[m][4 * q + 3] + bb.w);
                        KPGNN_BN_AFFINE(v[m])
                        v[m].x = fmaxf(v[m].x, 0.f); v[m].y = fmaxf(v[m].y, 0.f); v[m].z = fmaxf(v[m].z, 0.f); v[m].w = fmaxf(v[m].w, 0.f);
                    }
                }
                if (outer) {
                    const float4 mean = ld4(co + 8 * O + ob), istd = ld4(co + 9 * O + ob), g = ld4(co + 10 * O + ob), bt = ld4(co + 11 * O + ob);
#pragma unroll
                    for (int m = 0; m < M; ++m) { KPGNN_BN_AFFINE(v[m]) }
                }
#pragma unroll
                for (int m = 0; m < M; ++m) st4(xl + (m * 32 + c) * pitch + ob, v[m]);
            }
        }
        __syncthreads();
        {
            const int64_t r0 = tile * ROWS;
            const int rows = (int)(p.N - r0 < ROWS ? p.N - r0 : ROWS);
            if (act_o)
                for (int r = rlo; r < rows; r += RLO) {
                    float4 v = ld4(xl + r * pitch + 4 * cgo);
                    if (p.res) {
                        const float4 rr = ld4(p.res + (r0 + r) * p.rs + 4 * cgo);
                        v.x += rr.x; v.y += rr.y; v.z += rr.z; v.w += rr.w;
                    }
                    st4(p.y + (r0 + r) * p.ys + 4 * cgo, v);
                }
        }
        __syncthreads();                               // the result is out: the buffer takes the next x tile
        if (more) commit();
        __syncthreads();
    }
}

int mlp_eval_launch(const MlpEvalParams& p0, int I, int O, hipStream_t s) {
    MlpEvalParams p = p0;
    p.pitch = mfma_pitch(I > O ? I : O);
    const TilePlan t = tile_plan(p.N, (int64_t)device_facts().cu_count * 2, {1, 2}, true);
    const size_t lds = sizeof(float) * ((size_t)t.rows * p.pitch + (size_t)kEvalCoefRows * O);
    const int rc = LinWidths::dispatch(I, "mlp_eval", [&](auto KSI) {
        return LinWidths::dispatch(O, "mlp_eval (second Linear)", [&](auto KSO) {
            auto go = [&](auto M) {
                KPGNN_HIP_TRY(ensure_dynamic_lds((const void*)mlp_eval_kernel<KSI(), KSO(), M()>, lds));
                hipLaunchKernelGGL((mlp_eval_kernel<KSI(), KSO(), M()>), dim3(t.grid), dim3(256), lds, s, p);
                return (int)KPGNN_OK;
            };
            return t.m == 1 ? go(std::integral_constant<int, 1>{}) : go(std::integral_constant<int, 2>{});
        });
    });
    if (rc != KPGNN_OK) return rc;
    KPGNN_LAUNCH_CHECK("mlp_eval_kernel");
    return KPGNN_OK;
}

bool bn_complete(const kpgnn_bn_running& b) { return b.gamma && b.beta && b.running_mean && b.running_var; }
BnRun bn_of(const kpgnn_bn_running& b) { return BnRun{b.gamma, b.beta, b.running_mean, b.running_var, b.eps}; }

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_mlp_eval(const kpgnn_mlp_eval_desc* d, kpgnn_stream_t stream) {
    KPGNN_REQUIRE(d != nullptr, "mlp_eval: NULL descriptor");
    KPGNN_REQUIRE(d->N >= 1 && d->O >= 1 && d->I >= 1, "mlp_eval: bad N=%lld O=%d I=%d", (long long)d->N, d->O, d->I);
    KPGNN_REQUIRE(d->x && d->w0 && d->w3 && d->y, "mlp_eval: NULL pointer");
    KPGNN_REQUIRE(bn_complete(d->bn1) && bn_complete(d->bn2),
                  "mlp_eval: bn1 / bn2 need gamma, beta, running_mean and running_var (evaluation mode runs on the running statistics)");
    KPGNN_REQUIRE(!d->outer.gamma || bn_complete(d->outer), "mlp_eval: the outer norm needs beta, running_mean and running_var");
    KPGNN_REQUIRE(d->x_stride >= d->I && d->y_stride >= d->O && (!d->residual || d->r_stride >= d->O), "mlp_eval: bad strides");
    if (!LinWidths::has(d->I)) return LinWidths::refuse(d->I, "mlp_eval");
    if (!LinWidths::has(d->O)) return LinWidths::refuse(d->O, "mlp_eval (second Linear)");
    uintptr_t al = (uintptr_t)d->x | (uintptr_t)d->y | (uintptr_t)d->w0 | (uintptr_t)d->w3 | (uintptr_t)d->residual;
    if ((al & 15) || (d->x_stride & 3) || (d->y_stride & 3) || (d->residual && (d->r_stride & 3)))
        return fail(KPGNN_ELIMIT, "mlp_eval: operands must be 16-B aligned (row strides multiples of 4)");
    MlpEvalParams p = {};
    p.N = d->N; p.n_dyn = d->n_dyn;
    p.x = d->x; p.xs = d->x_stride; p.w0 = d->w0; p.b0 = d->b0; p.w3 = d->w3; p.b3 = d->b3;
    p.bn[0] = bn_of(d->bn1); p.bn[1] = bn_of(d->bn2);
    if (d->outer.gamma) p.bn[2] = bn_of(d->outer);
    p.res = d->residual; p.rs = d->r_stride; p.y = d->y; p.ys = d->y_stride;
    return mlp_eval_launch(p, d->I, d->O, (hipStream_t)stream);
}
