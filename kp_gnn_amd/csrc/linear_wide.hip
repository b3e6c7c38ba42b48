// y = x W^T + b for wide outputs (O > 128) on the fp32 matrix cores, and the C-ABI entry kpgnn_linear_fwd, which sends
// O <= 128 to the fused kernel's plain variant (lin_fused.h) and blocked outputs to the bf16-split kernel where it applies
// (linear_bf3.hip).  gfx950.  Contract: include/kpgnn.h, kpgnn_linear_fwd.
#include "mfma_tile.h"

namespace kpgnn {
namespace {

struct LinParams {
    int64_t N; int O, I, pitch, ypitch, wt;
    const float* x; int64_t xs;
    const float* xmask; const int32_t* n_dyn;   // optional ReLU mask of x (same layout), optional live-row count
    const float* w; const float* bias;
    float* y; int64_t ys;
    int yb; int64_t ybs;   // wide kernel: output column o lands in block o / yb at column o % yb; blocks are ybs floats apart (yb == O: plain rows)
};

// Wide outputs (O > 128, e.g. the input gradient of the jumping-knowledge projection: [N,104] x [104,936]): the x tile
// stays resident in LDS while the block walks the outputs 128 at a time - per chunk every wave reloads its strip of the
// weight (L2-resident) and runs its MFMA chains; results go straight from the accumulators to y (64 x 16-B segments per
// store: measured as fast as staging through LDS), so no barrier separates the chunks.
template <int KS, int M>
__global__ void __launch_bounds__(256, 2)
linear_wide_kernel(const LinParams p) {
    extern __shared__ __attribute__((aligned(16))) float xl[];      // [32*M][pitch]
    constexpr int ROWS = 32 * M;
    constexpr int IC = 2 * KS;                        // == I (host)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int kk = lane >> 5, c = lane & 31;
    const int O = p.O, pitch = p.pitch;
    const int64_t N = p.n_dyn ? (int64_t)min((int64_t)*p.n_dyn, p.N) : p.N;
    const int64_t tiles = (N + ROWS - 1) / ROWS;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        __syncthreads();                               // previous tile fully consumed
        {   // x tile -> LDS (no register double-buffer: the eight output chunks dwarf this load)
            const int64_t r0 = tile * ROWS;
            const int lim = (int)(N - r0 < ROWS ? N - r0 : ROWS) * IC;
            const float* base = p.x + r0 * p.xs;
            for (int e = 4 * tid; e < ROWS * IC; e += 4 * 256) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e < lim) {
                    v = *reinterpret_cast<const float4*>(base + e);
                    if (p.xmask) {
                        const float4 mk = *reinterpret_cast<const float4*>(p.xmask + r0 * p.xs + e);
                        if (mk.x <= 0.f) v.x = 0.f; if (mk.y <= 0.f) v.y = 0.f; if (mk.z <= 0.f) v.z = 0.f; if (mk.w <= 0.f) v.w = 0.f;
                    }
                }
                *reinterpret_cast<float4*>(xl + (e / IC) * pitch + (e % IC)) = v;
            }
        }
        __syncthreads();
        const int64_t r0 = tile * ROWS;
        const float* b0 = xl + c * pitch + kk;
#pragma unroll 1
        for (int chunk = (int)blockIdx.y * 128; chunk < O; chunk += 128 * (int)gridDim.y) {   // (few row tiles: chunks over blockIdx.y)
            // the operand reads below do not depend on the chunk: without this the compiler hoists all of them out of
            // the loop and spills ~500 registers
            int z = 0;
            asm volatile("" : "+v"(z));
            const float* bz = b0 + z;
            const int o = chunk + wave * 32 + c;
            float a[KS];
            if (p.wt) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) a[ks] = o < O ? p.w[(int64_t)(2 * ks + kk) * O + o] : 0.f;
            } else {
#pragma unroll
                for (int j = 0; j < KS / 2; ++j) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (o < O) v = *reinterpret_cast<const float4*>(p.w + (int64_t)o * IC + 4 * j);
                    a[2 * j] = kk ? v.y : v.x;
                    a[2 * j + 1] = kk ? v.w : v.z;
                }
            }
            f32x16 acc[M];
#pragma unroll
            for (int m = 0; m < M; ++m)
                for (int v = 0; v < 16; ++v) acc[m][v] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const float xv = bz[m * 32 * pitch + 2 * ks];
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ks], xv, acc[m], 0, 0, 0);
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ob = chunk + wave * 32 + 8 * g + 4 * kk;
                if (ob < O) {
                    float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (p.bias) bb = *reinterpret_cast<const float4*>(p.bias + ob);
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        const int64_t r = r0 + m * 32 + c;
                        if (r < N)
                            *reinterpret_cast<float4*>(p.y + (int64_t)(ob / p.yb) * p.ybs + r * p.ys + (ob % p.yb)) =
                                make_float4(acc[m][4 * g] + bb.x, acc[m][4 * g + 1] + bb.y, acc[m][4 * g + 2] + bb.z, acc[m][4 * g + 3] + bb.w);
                    }
                }
            }
        }
    }
}

}  // namespace
}  // namespace kpgnn

using namespace kpgnn;

extern "C" int kpgnn_linear_fwd(const kpgnn_linear_desc* d, kpgnn_stream_t stream) {
    KPGNN_REQUIRE(d != nullptr, "linear_fwd: NULL descriptor");
    KPGNN_REQUIRE(d->N >= 1 && d->O >= 1 && d->I >= 1, "linear_fwd: bad N=%lld O=%d I=%d", (long long)d->N, d->O, d->I);
    if (d->O > 4096 || d->I > 128) return fail(KPGNN_ELIMIT, "linear_fwd: O=%d exceeds 4096 or I=%d exceeds 128", d->O, d->I);
    KPGNN_REQUIRE(d->x && d->w && d->y, "linear_fwd: NULL pointer");
    const bool blocked = d->y_block_cols > 0 && d->y_block_cols < d->O;   // output split into column blocks ([S, N, yb] layout)
    if (blocked && ((d->y_block_cols % 4) != 0 || (d->O % d->y_block_cols) != 0 || d->y_stride != d->y_block_cols ||
                    (d->y_block_stride % 4) != 0 || d->O <= 128))
        return fail(KPGNN_ELIMIT, "linear_fwd: blocked output needs O > 128, O %% y_block_cols == 0, y_block_cols %% 4 == 0, "
                                  "y_stride == y_block_cols and a 16-B aligned block stride");
    if ((d->O % 4) != 0 || (d->I % 4) != 0 || d->x_stride != d->I || (!blocked && d->y_stride != d->O) ||
        (((uintptr_t)d->x | (uintptr_t)d->y) & 15) != 0 || (d->bias && (((uintptr_t)d->bias) & 15) != 0))
        return fail(KPGNN_ELIMIT, "linear_fwd: needs contiguous 16-B aligned x / y with I %% 4 == 0 and O %% 4 == 0");
    hipStream_t s = (hipStream_t)stream;
    if (d->O <= 128 && d->x_mask) return fail(KPGNN_ELIMIT, "linear_fwd: x_mask is implemented for O > 128");
    if (d->x_mask && (((uintptr_t)d->x_mask) & 15) != 0) return fail(KPGNN_ELIMIT, "linear_fwd: x_mask must be 16-B aligned");
    if (d->O <= 128) {                                  // the plain variant of the fused kernel (lin_fused.h)
        kpgnn_linear_bn_desc f = {};
        f.N = d->N; f.n_dyn = d->n_dyn; f.O = d->O; f.I = d->I; f.x = d->x; f.w = d->w; f.bias = d->bias; f.y = d->y; f.w_transposed = d->w_transposed;
        return kpgnn_linear_bn(&f, stream);
    }
    if (blocked && (((uintptr_t)d->w) & 15) == 0) {
        bool handled = false;
        const int rc = linear3_blocked(d, s, &handled);                            // the bf16-split kernel, where it applies
        if (handled || rc != KPGNN_OK) return rc;
    }
    if (!WideWidths::has(d->I)) return WideWidths::refuse(d->I, "linear_fwd (wide outputs)");
    LinParams p;
    p.N = d->N; p.O = d->O; p.I = d->I; p.wt = d->w_transposed ? 1 : 0;
    const int rowp = mfma_pitch(d->I);
    p.pitch = rowp; p.ypitch = rowp;
    p.x = d->x; p.xs = d->x_stride; p.w = d->w; p.bias = d->bias; p.y = d->y; p.ys = d->y_stride;
    p.xmask = d->x_mask; p.n_dyn = d->n_dyn;
    p.yb = blocked ? d->y_block_cols : d->O; p.ybs = blocked ? d->y_block_stride : 0;
    const int64_t slots = (int64_t)device_facts().cu_count * 2;      // two blocks per CU
    const TilePlan t = tile_plan(d->N, slots, {1, 2, 3}, true);
    const size_t lds = sizeof(float) * (size_t)t.rows * rowp;
    // a small batch has fewer row tiles than the chip has block slots: the output chunks of a tile are then spread over
    // blockIdx.y instead of walked one after the other (batch 64, [1.5k,104] x [104,936]: one block chain of 8 chunks, 31 us)
    const int64_t nchunks = (d->O + 127) / 128;
    int64_t gy = t.tiles < slots ? (slots + t.tiles - 1) / t.tiles : 1;
    if (gy > nchunks) gy = nchunks;
    const int rc = WideWidths::dispatch(d->I, "linear_fwd (wide outputs)", [&](auto KS) {
        auto go = [&](auto M) {
            KPGNN_HIP_TRY(ensure_dynamic_lds((const void*)linear_wide_kernel<KS(), M()>, lds));
            hipLaunchKernelGGL((linear_wide_kernel<KS(), M()>), dim3(t.grid, (unsigned)gy), dim3(256), lds, s, p);
            return (int)KPGNN_OK;
        };
        return t.m == 1 ? go(std::integral_constant<int, 1>{}) : t.m == 2 ? go(std::integral_constant<int, 2>{}) : go(std::integral_constant<int, 3>{});
    });
    if (rc != KPGNN_OK) return rc;
    KPGNN_LAUNCH_CHECK("linear_wide_kernel");
    return KPGNN_OK;
}
