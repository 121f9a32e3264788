// Windowed inference of long videos (s2d_amd/modeling/window_inference.py; DESIGN.md section 1, "Windowed inference"): the two
// device steps between consecutive windows of frames.
//
//   s2d_window_pair_counts      the Q x Q intersection counts and the 2 Q areas of the binary masks `logit > 0` of ALL queries
//                               of two windows on the frames they share, straight from the two pixel-major fp32 logit blocks
//                               (no query-major planes, no byte masks in memory);
//   s2d_window_scatter_columns  the owned rows of a window written into the stitched buffer with its columns permuted into
//                               track order, one pass.
//
// Both are bandwidth-bound: the first reads 2 * n * ldq * 4 bytes once and writes a few KB, the second copies its rows.
#include "common.h"

namespace {

constexpr int WQ = 128;            // query columns a workgroup's LDS words cover (the library's MAX_QUERIES)
constexpr int WWORDS = 32;         // 32-pixel words of one block a workgroup folds per pass, at most
constexpr int WT = 8;              // a thread accumulates a WT x WT tile of query pairs

// Pass structure, per run of `wp` words (wp * 32 pixels):
//   1. thread (word w, column group g) walks the 32 rows of its word with one float4 load per row and block -- the lanes of a
//      word cover one row's ldq floats contiguously -- and folds the signs of its 4 columns into 4 words per block;
//   2. the words go to LDS as [word][column] (16-byte writes, consecutive lanes consecutive slots);
//   3. thread (ti, tj) adds popcount(a[ti*8 + x] & b[tj*8 + y]) of every word into its 8 x 8 register tile (the a words are a
//      broadcast within a wave, the b words 32 contiguous bytes per lane), threads 0 .. 2Q-1 add the areas.
// At the end one 64-bit integer atomic per non-zero pair and workgroup, row by row: the sums do not depend on any order.
__global__ __launch_bounds__(256) void window_pair_counts_kernel(const float *__restrict__ A, const float *__restrict__ B, long n,
                                                                 int ldq, int Q, int wp, long nruns,
                                                                 unsigned long long *__restrict__ inter,
                                                                 unsigned long long *__restrict__ area_a,
                                                                 unsigned long long *__restrict__ area_b)
{
    __shared__ __attribute__((aligned(16))) unsigned int lds[2 * WWORDS * WQ];
    unsigned int *const sa = lds, *const sb = lds + WWORDS * WQ;
    const int t = threadIdx.x;
    const int G = ldq >> 2;                              // float4 groups per row
    for (int i = t; i < WWORDS * WQ; i += 256) { sa[i] = 0u; sb[i] = 0u; }      // columns >= ldq are never written: they stay 0
    const int w = t / G, g = t - w * G;
    const bool loader = w < wp;
    const int ti = t >> 4, tj = t & 15;
    const bool pairs = ti * WT < Q && tj * WT < Q;
    unsigned int acc[WT][WT];
#pragma unroll
    for (int x = 0; x < WT; ++x)
#pragma unroll
        for (int y = 0; y < WT; ++y) acc[x][y] = 0u;
    unsigned int area = 0u;
    const f32x4 *A4 = reinterpret_cast<const f32x4 *>(A), *B4 = reinterpret_cast<const f32x4 *>(B);
    __syncthreads();
    for (long run = blockIdx.x; run < nruns; run += gridDim.x) {
        if (loader) {
            const long p0 = (run * wp + w) * 32;
            unsigned int a0 = 0u, a1 = 0u, a2 = 0u, a3 = 0u, b0 = 0u, b1 = 0u, b2 = 0u, b3 = 0u;
            if (p0 + 32 <= n) {
#pragma unroll 8
                for (int r = 0; r < 32; ++r) {
                    const f32x4 va = A4[(p0 + r) * G + g], vb = B4[(p0 + r) * G + g];
                    a0 |= (va.x > 0.f ? 1u : 0u) << r; a1 |= (va.y > 0.f ? 1u : 0u) << r;
                    a2 |= (va.z > 0.f ? 1u : 0u) << r; a3 |= (va.w > 0.f ? 1u : 0u) << r;
                    b0 |= (vb.x > 0.f ? 1u : 0u) << r; b1 |= (vb.y > 0.f ? 1u : 0u) << r;
                    b2 |= (vb.z > 0.f ? 1u : 0u) << r; b3 |= (vb.w > 0.f ? 1u : 0u) << r;
                }
            } else {
                for (int r = 0; r < 32 && p0 + r < n; ++r) {
                    const f32x4 va = A4[(p0 + r) * G + g], vb = B4[(p0 + r) * G + g];
                    a0 |= (va.x > 0.f ? 1u : 0u) << r; a1 |= (va.y > 0.f ? 1u : 0u) << r;
                    a2 |= (va.z > 0.f ? 1u : 0u) << r; a3 |= (va.w > 0.f ? 1u : 0u) << r;
                    b0 |= (vb.x > 0.f ? 1u : 0u) << r; b1 |= (vb.y > 0.f ? 1u : 0u) << r;
                    b2 |= (vb.z > 0.f ? 1u : 0u) << r; b3 |= (vb.w > 0.f ? 1u : 0u) << r;
                }
            }
            const int c = g * 4;                             // pad columns Q .. ldq-1 hold anything: not part of any mask
            if (c + 1 >= Q) { a1 = 0u; b1 = 0u; }
            if (c + 2 >= Q) { a2 = 0u; b2 = 0u; }
            if (c + 3 >= Q) { a3 = 0u; b3 = 0u; }
            if (c >= Q) { a0 = 0u; b0 = 0u; }
            *reinterpret_cast<uint4 *>(&sa[w * WQ + c]) = make_uint4(a0, a1, a2, a3);
            *reinterpret_cast<uint4 *>(&sb[w * WQ + c]) = make_uint4(b0, b1, b2, b3);
        }
        __syncthreads();
        if (pairs) {
            for (int k = 0; k < wp; ++k) {
                unsigned int va[WT], vb[WT];
                const uint4 x0 = *reinterpret_cast<const uint4 *>(&sa[k * WQ + ti * WT]);
                const uint4 x1 = *reinterpret_cast<const uint4 *>(&sa[k * WQ + ti * WT + 4]);
                const uint4 y0 = *reinterpret_cast<const uint4 *>(&sb[k * WQ + tj * WT]);
                const uint4 y1 = *reinterpret_cast<const uint4 *>(&sb[k * WQ + tj * WT + 4]);
                va[0] = x0.x; va[1] = x0.y; va[2] = x0.z; va[3] = x0.w; va[4] = x1.x; va[5] = x1.y; va[6] = x1.z; va[7] = x1.w;
                vb[0] = y0.x; vb[1] = y0.y; vb[2] = y0.z; vb[3] = y0.w; vb[4] = y1.x; vb[5] = y1.y; vb[6] = y1.z; vb[7] = y1.w;
#pragma unroll
                for (int x = 0; x < WT; ++x)
#pragma unroll
                    for (int y = 0; y < WT; ++y) acc[x][y] += __popc(va[x] & vb[y]);
            }
        }
        if (t < 2 * Q) {
            const unsigned int *s = t < Q ? sa + t : sb + (t - Q);
            for (int k = 0; k < wp; ++k) area += __popc(s[k * WQ]);
        }
        __syncthreads();
    }
    // the register tiles go through LDS (64 rows of the Q x Q matrix at a time: the 32 KB of the word buffers), so that a wave's
    // atomics fall on consecutive addresses of a row instead of 64 scattered ones (the last barrier of the loop, or the one behind
    // the zero fill, has made the word buffers free)
    for (int half = 0; half * 64 < Q; ++half) {
        if (pairs && (ti >> 3) == half) {
#pragma unroll
            for (int x = 0; x < WT; ++x)
#pragma unroll
                for (int y = 0; y < WT; ++y) lds[((ti & 7) * WT + x) * WQ + tj * WT + y] = acc[x][y];
        }
        __syncthreads();
        for (int idx = t; idx < 64 * WQ; idx += 256) {
            const int i = half * 64 + idx / WQ, j = idx % WQ;
            if (i < Q && j < Q) {                           // every such entry was written: its tile's thread has `pairs`
                const unsigned int v = lds[idx];
                if (v) atomicAdd(&inter[(long)i * Q + j], (unsigned long long)v);
            }
        }
        __syncthreads();
    }
    if (t < 2 * Q && area) atomicAdd(t < Q ? &area_a[t] : &area_b[t - Q], (unsigned long long)area);
}

// dst[row0 + r][p] = src[r][perm[p]] for p < Q, = src[r][p] for the pad columns Q <= p < ldq.  A thread writes one float4 of a
// destination row; its four sources lie in the same ldq-float source row its neighbours read.  A perm entry outside [0, Q) (never
// produced by the association) reads its own column instead of memory outside the row.
__global__ __launch_bounds__(256) void window_scatter_columns_kernel(const float *__restrict__ src, long rows, int ldq, int Q,
                                                                     const int *__restrict__ perm, float *__restrict__ dst)
{
    __shared__ int sp[WQ];
    for (int p = threadIdx.x; p < ldq; p += 256) {
        int q = p;
        if (p < Q) {
            q = perm[p];
            if (q < 0 || q >= Q) q = p;
        }
        sp[p] = q;
    }
    __syncthreads();
    const int G = ldq >> 2;
    const long total = rows * G;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / G;
        const int c = (int)(i - r * G) * 4;
        const float *s = src + r * ldq;
        f32x4 v;
        v.x = s[sp[c]]; v.y = s[sp[c + 1]]; v.z = s[sp[c + 2]]; v.w = s[sp[c + 3]];
        *reinterpret_cast<f32x4 *>(dst + r * ldq + c) = v;
    }
}

}  // namespace

extern "C" {

int s2d_window_pair_counts(const float *A, const float *B, long n, int ldq, int Q, int64_t *inter, int64_t *area_a,
                           int64_t *area_b, hipStream_t stream)
{
    if (Q < 1 || Q > WQ || ldq < Q || ldq > WQ || (ldq & 3) || n < 0 || n >= (1L << 31)) return S2D_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) return S2D_ERR_ARG;       // rows are read as float4
    if (s2d_zero_async(inter, sizeof(int64_t) * (size_t)Q * Q, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    if (s2d_zero_async(area_a, sizeof(int64_t) * (size_t)Q, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    if (s2d_zero_async(area_b, sizeof(int64_t) * (size_t)Q, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    if (n == 0) return S2D_OK;
    const int G = ldq >> 2;
    int wp = 256 / G;                                    // words whose rows 256 threads cover, one float4 column group each
    if (wp > WWORDS) wp = WWORDS;
    const long nruns = (n + (long)wp * 32 - 1) / ((long)wp * 32);
    const int grid = nruns < 1024 ? (int)nruns : 1024;
    hipLaunchKernelGGL(window_pair_counts_kernel, dim3(grid), dim3(256), 0, stream, A, B, n, ldq, Q, wp, nruns,
                       reinterpret_cast<unsigned long long *>(inter), reinterpret_cast<unsigned long long *>(area_a),
                       reinterpret_cast<unsigned long long *>(area_b));
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_window_scatter_columns(const float *src, long rows, int ldq, int Q, const int *perm, float *dst, long row0,
                               hipStream_t stream)
{
    if (Q < 1 || Q > WQ || ldq < Q || ldq > WQ || (ldq & 3) || rows < 0 || row0 < 0) return S2D_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(dst) & 15) return S2D_ERR_ARG;                                          // rows are written as float4
    if (rows == 0) return S2D_OK;
    const long blocks = (rows * (ldq >> 2) + 255) / 256;
    hipLaunchKernelGGL(window_scatter_columns_kernel, dim3(blocks < 2048 ? (int)blocks : 2048), dim3(256), 0, stream, src, rows,
                       ldq, Q, perm, dst + row0 * ldq);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
