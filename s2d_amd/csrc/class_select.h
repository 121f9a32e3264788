// Class-aware score selection shared by the distillation-target selection (loss.hip) and the inference top-K (infer.hip) when
// a query carries C1 = C + 1 class logits (C foreground classes + "no object").
//
// The scores are softmax(logits)[:, :-1] flattened over [Q][C] (flat index f = q*C + c, kd_video_maskformer_model.py:436-440,
// :532-538).  Per clip:
//   1. cls_row_stats_kernel: per query row, max and sum of exp(l - max) in ascending class order (the expression tree every
//      two-logit kernel of the library uses, so C1 = 2 gives the same bits), and the row's best foreground score;
//   2. cls_scores_kernel:    the flat scores, expf(l - max) / sum, into a workspace row of Q*C floats;
//   3. flat_rank_kernel:     the rank of every candidate score among the clip's Q*C (descending score, ties -> lower flat index
//      first, which is torch.topk(sorted=True)'s order on the reference's CPU path for distinct scores).  A score below
//      max(thr, K-th largest row best) cannot be in the top K -- the row bests are K entries at least that large -- so it is not
//      ranked (rank = n), a workgroup without a candidate skips the O(n) walk, and a walking workgroup skips the
//      256-score tiles that hold no score at or above the floor (only those can beat a candidate).
// Ranks are exact integers, so the selection is deterministic and independent of the launch geometry.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ void softmax_row_stats(const float *__restrict__ l, int C1, float &mx, float &sum)
{
    mx = l[0];
    for (int c = 1; c < C1; ++c) mx = fmaxf(mx, l[c]);
    sum = 0.f;
    for (int c = 0; c < C1; ++c) sum += expf(l[c] - mx);
}

// stats[row] = (max, sum exp), rbest[row] = max_c<C softmax   (one thread per row of C1 logits)
__global__ __launch_bounds__(256) void cls_row_stats_kernel(const float *__restrict__ cls, long rows, int C1, float2 *__restrict__ stats,
                                                            float *__restrict__ rbest)
{
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float *l = cls + r * C1;
    float mx, sum;
    softmax_row_stats(l, C1, mx, sum);
    float best = 0.f;
    for (int c = 0; c + 1 < C1; ++c) best = fmaxf(best, expf(l[c] - mx) / sum);
    stats[r] = make_float2(mx, sum);
    rbest[r] = best;
}

// sc[b][q*C + c] = softmax(cls[b][q])[c]
__global__ __launch_bounds__(256) void cls_scores_kernel(const float *__restrict__ cls, const float2 *__restrict__ stats, int B, int Q, int C,
                                                         float *__restrict__ sc)
{
    const long n = (long)Q * C;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * n) return;
    const long row = i / C;                       // = b*Q + q
    const int c = (int)(i - row * C);
    const float2 st = stats[row];
    sc[i] = expf(cls[row * (C + 1) + c] - st.x) / st.y;
}

// rank[b][i] of score i among the clip's n = Q*C scores, or n when it is not a candidate (see the file comment).  The floor is
// found by the first 256 rows' threads; when the K-th row best sits beyond them the floor is just thr (still exact, less pruned).
// With `scores` set, the top K (rank < K) are also written in rank order: scores / query / label [b][K].
constexpr int FR_THREADS = 256;
__global__ __launch_bounds__(FR_THREADS) void flat_rank_kernel(const float *__restrict__ sc, const float *__restrict__ rbest, int Q, int C, int K,
                                                               float thr, int *__restrict__ rank, float *__restrict__ scores,
                                                               int *__restrict__ query, int *__restrict__ label)
{
    __shared__ float tile[FR_THREADS];
    __shared__ float kth;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = Q * C;
    const float *s = sc + (long)b * n;
    if (tid == 0) kth = -1.f;
    __syncthreads();
    if (K <= Q && tid < Q) {                       // the K-th largest row best (ties by row index: one thread matches)
        const float v = rbest[(long)b * Q + tid];
        int r = 0;
        for (int j = 0; j < Q; ++j) {
            const float o = rbest[(long)b * Q + j];
            r += (o > v) || (o == v && j < tid);
        }
        if (r == K - 1) kth = v;
    }
    __syncthreads();
    const float floor_ = fmaxf(thr, kth);
    const int i = blockIdx.x * FR_THREADS + tid;
    const float v = i < n ? s[i] : -1.f;
    const bool cand = i < n && v >= floor_;
    if (!__syncthreads_or(cand)) {
        if (i < n) rank[(long)b * n + i] = n;
        return;
    }
    int r = 0;
    for (int j0 = 0; j0 < n; j0 += FR_THREADS) {
        const int m = n - j0 < FR_THREADS ? n - j0 : FR_THREADS;
        const float t = tid < m ? s[j0 + tid] : -1.f;
        __syncthreads();
        tile[tid] = t;
        // scores below the floor never beat a candidate (they are < floor <= v): a tile holding none above it is skipped
        if (__syncthreads_or(t >= floor_) && cand)
            for (int jj = 0; jj < m; ++jj) {
                const float o = tile[jj];
                r += (o > v) || (o == v && j0 + jj < i);
            }
    }
    if (i < n) rank[(long)b * n + i] = cand ? r : n;
    if (scores && cand && r < K) {
        scores[(long)b * K + r] = v;
        query[(long)b * K + r] = i / C;
        label[(long)b * K + r] = i % C;
    }
}

// bytes of workspace the three kernels above need for B clips of Q queries x C1 logits
static inline long cls_select_workspace_bytes(int B, int Q, int C1)
{
    const long rows = (long)B * Q, n = rows * (C1 - 1);
    return rows * 8 + rows * 4 + n * 4 + n * 4 + 256;
}

// carve the workspace and enqueue the three kernels; rank [B][Q*C] is returned through `rank_out`
static inline int cls_select_launch(const float *cls, int B, int Q, int C1, int K, float thr, void *workspace, int **rank_out,
                                    float *scores, int *query, int *label, hipStream_t stream)
{
    const int C = C1 - 1;
    const long rows = (long)B * Q, n = rows * C;
    char *w = (char *)workspace;
    float2 *stats = (float2 *)w; w += rows * 8;
    float *rbest = (float *)w; w += rows * 4;
    float *sc = (float *)w; w += n * 4;
    int *rank = (int *)w;
    hipLaunchKernelGGL(cls_row_stats_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, stream, cls, rows, C1, stats, rbest);
    hipLaunchKernelGGL(cls_scores_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, cls, stats, B, Q, C, sc);
    hipLaunchKernelGGL(flat_rank_kernel, dim3(cdiv((long)Q * C, FR_THREADS), B), dim3(FR_THREADS), 0, stream, sc, rbest, Q, C, K, thr, rank,
                       scores, query, label);
    *rank_out = rank;
    return S2D_OK;
}

}  // namespace
