// The split-fp16 x3 scheme ("f16x3"): the one definition behind every dense contraction of the library -- the GEMMs and convolutions
// (gemm_bf16.hip, gemm_small.hip), the weight gradients (gemm_tn.hip), the encoder FFN (ffn.hip), attention (attn.hip), the matcher.
//
// fp32-class accuracy (~3*2^-22) on the fp16 matrix cores at three MFMAs per product:
//   x = h + l * 2^-11,   h = fp16_rtz(x),   l = fp16_rtz((x - h) * 2^11)          (22+ significant bits while h is a
//   A.B^T = [Ah.Bh^T] + 2^-11 * [Ah.Bl^T + Al.Bh^T]                                 normal fp16 number, |x| >= 2^-14)
// The two brackets are accumulated in separate f32 accumulators (main / cross) and combined at the end: join(main, cross).
// The accuracy window is an operand amax in [2^-14, 65504]: below it h is subnormal or zero and l loses bits too (the error grows
// ~10x per decade of scale), above it the RTZ conversion saturates (x -> 65535.98, no inf).  The forward's activations and weights
// are O(1e-3..1e3); the gradients are brought into the window by the backward's power-of-two root scale (backward.grad_scale).
#pragma once
#include "common.h"

typedef __fp16 h16x2 __attribute__((ext_vector_type(2)));       // what v_cvt_pkrtz_f16_f32 returns
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));     // one lane's MFMA operand fragment
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr float SPLIT_SCALE = 2048.f, SPLIT_INV = 1.0f / 2048.0f;

// main + cross * 2^-11; the fma form where a site accumulates the cross part into a running sum
__device__ __forceinline__ float join(float m, float x) { return m + x * SPLIT_INV; }
__device__ __forceinline__ float join_fma(float m, float x) { return __builtin_fmaf(x, SPLIT_INV, m); }

// The split, in the instruction forms the kernels were tuned with (same bits from each).  Its steps are separate functions so
// that a software pipeline can place them apart (the pipelined GEMM spreads one split over three MFMA shadows):
__device__ __forceinline__ h16x2 split_hi(float a, float b) { return __builtin_amdgcn_cvt_pkrtz(a, b); }
__device__ __forceinline__ f32x2 split_hi_f32(const h16x2 h) { return __builtin_convertvector(h, f32x2); }
__device__ __forceinline__ f32x2 split_rem(const f32x2 x, const f32x2 hf) { return (x - hf) * SPLIT_SCALE; }      // exact; packed f32 ops
__device__ __forceinline__ h16x2 split_lo(const f32x2 r) { return __builtin_amdgcn_cvt_pkrtz(r[0], r[1]); }

// two values that are consecutive along the contraction -> one word of high parts, one of low parts; subtract-multiply per value
__device__ __forceinline__ void split2(float a, float b, unsigned int &hi, unsigned int &lo)
{
    const h16x2 h = split_hi(a, b);
    const f32x2 f = split_hi_f32(h);
    const h16x2 l = __builtin_amdgcn_cvt_pkrtz((a - f[0]) * SPLIT_SCALE, (b - f[1]) * SPLIT_SCALE);
    hi = __builtin_bit_cast(unsigned int, h);
    lo = __builtin_bit_cast(unsigned int, l);
}
// the fma form: (a - h) * 2048 == fma(h, -2048, a * 2048) exactly (a - h is exact, the factor a power of two): one multiply and one
// v_fma_mix_f32 (the fp16 operand converted inside the fma) per value instead of convert, subtract, multiply
__device__ __forceinline__ unsigned int split2_hi(float a, float b) { return __builtin_bit_cast(unsigned int, split_hi(a, b)); }
__device__ __forceinline__ unsigned int split2_lo_fma(float a, float b, unsigned int hi)
{
    const h16x2 h = __builtin_bit_cast(h16x2, hi);
    return __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_pkrtz(__builtin_fmaf((float)h[0], -SPLIT_SCALE, a * SPLIT_SCALE),
                                                                       __builtin_fmaf((float)h[1], -SPLIT_SCALE, b * SPLIT_SCALE)));
}
__device__ __forceinline__ void split2_fma(float a, float b, unsigned int &hi, unsigned int &lo)
{
    hi = split2_hi(a, b);
    lo = split2_lo_fma(a, b, hi);
}

// four values -> two words of high parts, two of low parts (the 8-B pieces of an LDS operand row): both pairs step by step
__device__ __forceinline__ void split4(const f32x4 v, u32x2 &hi, u32x2 &lo)
{
    const h16x2 ha = split_hi(v[0], v[1]), hb = split_hi(v[2], v[3]);
    const f32x2 a = {v[0], v[1]}, b = {v[2], v[3]};
    const f32x2 ra = split_rem(a, split_hi_f32(ha)), rb = split_rem(b, split_hi_f32(hb));
    const h16x2 la = split_lo(ra), lb = split_lo(rb);
    hi[0] = __builtin_bit_cast(unsigned int, ha); hi[1] = __builtin_bit_cast(unsigned int, hb);
    lo[0] = __builtin_bit_cast(unsigned int, la); lo[1] = __builtin_bit_cast(unsigned int, lb);
}
// 8 consecutive values of a row (one lane's share of an MFMA k-step) -> hi / lo operand fragments
__device__ __forceinline__ void split8(const f32x4 a, const f32x4 b, f16x8 &hi, f16x8 &lo)
{
    u32x2 h0, l0, h1, l1;
    split4(a, h0, l0);
    split4(b, h1, l1);
    hi = __builtin_bit_cast(f16x8, u32x4{h0[0], h0[1], h1[0], h1[1]});
    lo = __builtin_bit_cast(f16x8, u32x4{l0[0], l0[1], l1[0], l1[1]});
}
