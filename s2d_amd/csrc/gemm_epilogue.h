// The row epilogue of the dense kernels, C = gate(act(acc * scale + bias + res)) (gemm_params.h), once: the tail of one 16-B row
// piece and the tail of one value where the shapes do not allow 16-B rows.  A kernel keeps its geometry (which row and column a lane owns,
// trip counts, unroll factors), its dropout block, any prefetched residual, and the loop that parks its accumulators in LDS: as a
// function, with the accumulators by reference or tile by tile by value, that loop compiles to other address arithmetic.
#pragma once
#include "split_f16.h"
#include "gemm_params.h"

// residual of the 4 columns from `col` of `row`: rows wrap at res_rows, columns from res_cols on get none.  res: the batch slice, or null
__device__ __forceinline__ f32x4 row_residual(const GemmParams &p, const float *res, f32x4 v, int row, int col)
{
    if (res && col < p.res_cols) v += *reinterpret_cast<const f32x4 *>(res + (long)(p.res_rows ? row % p.res_rows : row) * p.ldr + col);
    return v;
}
// ReLU, then (GATE: the kernels whose launches may carry one) the gate
template <bool GATE>
__device__ __forceinline__ f32x4 row_act(const GemmParams &p, f32x4 v, long row, int col)
{
    if (p.relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
    if (GATE && p.gate) {
        const f32x4 g = *reinterpret_cast<const f32x4 *>(p.gate + row * p.ldg + col);
        v[0] = g[0] > 0.f ? v[0] * p.gate_scale : 0.f; v[1] = g[1] > 0.f ? v[1] * p.gate_scale : 0.f;
        v[2] = g[2] > 0.f ? v[2] * p.gate_scale : 0.f; v[3] = g[3] > 0.f ? v[3] * p.gate_scale : 0.f;
    }
    return v;
}
// the whole tail of one 16-B row piece; a kernel with a residual of its own (prefetched, or a plain NHWC row) calls the steps
template <bool GATE>
__device__ __forceinline__ f32x4 row_tail(const GemmParams &p, const float *res, f32x4 v, const f32x4 sc, const f32x4 bi, int row, int col)
{
    v = v * sc + bi;
    v = row_residual(p, res, v, row, col);
    return row_act<GATE>(p, v, row, col);
}
// the same for one value (no gate: gated launches have 16-B rows)
__device__ __forceinline__ float scalar_tail(const GemmParams &p, const float *res, float v, float sc, float bi, int row, int col)
{
    v = v * sc + bi;
    if (res && col < p.res_cols) v += res[(long)(p.res_rows ? row % p.res_rows : row) * p.ldr + col];
    if (p.relu) v = fmaxf(v, 0.f);
    return v;
}
