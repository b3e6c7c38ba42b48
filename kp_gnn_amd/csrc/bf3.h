// Exact three-way bf16 split of fp32 values, for fp32-grade products on the bf16 matrix cores (gfx950).
//
// An fp32 value v is EXACTLY h + m + l with three bf16 pieces of 8 significant bits each, obtained by truncation:
//     h = top 16 bits of v,   m = top 16 bits of (v - h),   l = v - h - m   (at most 8 significant bits are left: l is a bf16)
// and for two such values  a b = ah bh + (ah bm + am bh) + (am bm + ah bl + al bh) + [am bl + al bm + al bl: dropped]:
// six exact bf16 products, accumulated in fp32 (smallest first), at 6/16 of the matrix time of v_mfma_f32_32x32x2_f32 (which
// runs at the vector rate).  The dropped terms sum to at most 7.83 * 2^-24 |a b| (about 2^-21), reached when the low 16
// mantissa bits of both operands are set (a = b = 0x3F80FFFF: m = 255 * 2^-15, l = 255 * 2^-23, 2 m l + l l = 7.95 * 2^-24
// against a b = 1.0157); truncation makes them all of one sign, so over a row of such operands they add up instead of
// averaging out.  Per element the result is within fp32 accumulation's own error plus 8 * 2^-24 sum_k |a_k b_k|
// (tests/test_bf16_split_products.py holds every kernel to that; DESIGN.md has the measured figures).
// Users: linear_bf3.hip (lin3_kernel: store_planes, mma6; lin3_wsplit*: split2 / pack), linear_bf3_fused.hip (lin3f_kernel:
// store_planes, mma6), attention.hip (attn_scan_fwd_kernel, attn_dx_kernel: mma6, split2 / pack), wgrad.hip (wgrad3_kernel:
// split2 / pack - it stages 8 ROWS of a column per item, and its six products run product by product over its TI column tiles,
// so that consecutive instructions feed different accumulators), table_grad.hip (the vector types).
// The helpers take everything by reference, bf3_store_planes forms its address after the split: with values, or with the
// address formed by the caller, the compiler scheduled lin3_kernel differently.  A helper for "eight values -> three 16-byte
// pieces" (the two lin3_wsplit kernels, attn_scan_fwd_kernel's x split) and bf3_store_planes in attn_dx_kernel did not keep
// those kernels' instruction order in any form tried: they stay written out.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace kpgnn {

using f32x16 = __attribute__((ext_vector_type(16))) float;     // accumulator of a 32x32 matrix instruction (fp32 and bf16 alike)
typedef __attribute__((ext_vector_type(8))) __bf16 bf3_x8;
typedef __attribute__((ext_vector_type(2))) float bf3_f2;
typedef __attribute__((ext_vector_type(2))) uint32_t bf3_u2;

// the split of two values at once (packed subtracts): word pairs whose TOP halves are the bf16 pieces
__device__ __forceinline__ void bf3_split2(const bf3_f2 v, bf3_u2& h, bf3_u2& m, bf3_u2& l) {
    h = __builtin_bit_cast(bf3_u2, v) & 0xffff0000u;
    const bf3_f2 r1 = v - __builtin_bit_cast(bf3_f2, h);
    m = __builtin_bit_cast(bf3_u2, r1) & 0xffff0000u;
    l = __builtin_bit_cast(bf3_u2, r1 - __builtin_bit_cast(bf3_f2, m));
}

// the top halves of two words side by side: low half <- a, high half <- b
__device__ __forceinline__ uint32_t bf3_pack(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }


// four values -> three packed bf16 planes (h, m, l), one 8-byte store each: item (row, col) of a plane whose rows are `pitch`
// elements of T long, the planes `plane` elements apart
template <typename T>
__device__ __forceinline__ void bf3_store_planes(T* buf, int row, int pitch, int col, int plane, const float4 v) {
    bf3_u2 h0, m0, l0, h1, m1, l1;
    bf3_split2(bf3_f2{v.x, v.y}, h0, m0, l0);
    bf3_split2(bf3_f2{v.z, v.w}, h1, m1, l1);
    T* q = buf + row * pitch + col;
    *reinterpret_cast<uint2*>(q) = make_uint2(bf3_pack(h0.x, h0.y), bf3_pack(h1.x, h1.y));
    *reinterpret_cast<uint2*>(q + plane) = make_uint2(bf3_pack(m0.x, m0.y), bf3_pack(m1.x, m1.y));
    *reinterpret_cast<uint2*>(q + 2 * plane) = make_uint2(bf3_pack(l0.x, l0.y), bf3_pack(l1.x, l1.y));
}

// acc += a b from the pieces: the six products, smallest terms first.  The order is part of the result's bits: one place.
__device__ __forceinline__ void bf3_mma6(f32x16& acc, const bf3_x8& ah, const bf3_x8& am, const bf3_x8& al, const bf3_x8& bh,
                                         const bf3_x8& bm, const bf3_x8& bl) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

}  // namespace kpgnn
