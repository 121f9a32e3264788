// The per-frame draw order of instance areas, shared by the mask-plane path (render.hip, s2d_mask_frame_areas_i32) and the plane-free
// one (infer.hip, s2d_infer_frame_areas_i32).
#pragma once
#include "common.h"

namespace {

// order[t][r] = the instance of rank r in frame t: rank = #{j : a_j > a_k or (a_j == a_k and j < k)}, a stable descending sort
__global__ __launch_bounds__(256) void draw_order_kernel(const int *__restrict__ areas, int K, int T, int *__restrict__ order)
{
    __shared__ int a[256];
    const int t = blockIdx.x, k = threadIdx.x;
    if (k < K) a[k] = areas[(long)k * T + t];
    __syncthreads();
    if (k >= K) return;
    const int ak = a[k];
    int r = 0;
    for (int j = 0; j < K; ++j) r += (a[j] > ak) | ((a[j] == ak) & (j < k));
    order[(long)t * K + r] = k;
}

}  // namespace
