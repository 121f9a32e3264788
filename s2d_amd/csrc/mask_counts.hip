// Popcounts over packed bit planes (layout: bitplane.h): per-plane areas and the intersection counts of plane pairs, exact
// integers from which the callers form IoUs on the host -- the greedy mask-NMS of inference (modeling/postprocess.py), the video
// IoU of the YTVIS evaluator (sum_t |d_t & g_t| over a track's frames, s2d_amd/ytvis_eval.py) and the per-frame J and F counts of
// the DAVIS evaluator (s2d_amd/davis_eval.py).
//
//   plane_popcount_kernel  per-plane areas (mask_util.area), one workgroup per plane;
//   pair_tile_kernel       out[i][j][t] += popcount(a[i][t] & b[j][t]) over a chunk of the words of frame t, an 8 x 8 tile of
//                          (i, j) pairs per workgroup (bitplane.h PopcTile: each word loaded once per tile).  A track is the
//                          case T = 1 with all its frames as one plane.  Integer atomics: the result does not depend on the order.
#include "bitplane.h"

namespace {

__global__ __launch_bounds__(256) void plane_popcount_kernel(const uint32_t *__restrict__ bits, long wpf, unsigned int *__restrict__ area)
{
    plane_popcount(bits + (long)blockIdx.x * wpf, wpf, area + blockIdx.x);
}

constexpr int PT = 8;

// a [D][T][wpf], b [G][T][wpf] -> out [D][G][T].  grid (chunks of the words, tiles, T).  SYM: a == b and D == G, blockIdx.y
// enumerates only the tile pairs ti <= tj (ntg tiles a side; the diagonal holds the areas) and a tile off the diagonal is
// written to both (i, j) and (j, i); otherwise blockIdx.y = ti * ntg + tj.
template <typename Out, bool SYM>
__global__ __launch_bounds__(256) void pair_tile_kernel(const uint32_t *__restrict__ a, int D, const uint32_t *__restrict__ b, int G,
                                                        int T, long wpf, int ntg, Out *__restrict__ out)
{
    __shared__ unsigned int red[4][PT * PT];
    int ti = 0, tj;
    if (SYM) {
        int rem = blockIdx.y;
        while (rem >= ntg - ti) { rem -= ntg - ti; ++ti; }
        tj = ti + rem;
    } else {
        ti = blockIdx.y / ntg;
        tj = blockIdx.y - ti * ntg;
    }
    const int t = blockIdx.z;
    PopcTile<PT> tile;
    tile.zero();
    const long per = (wpf + gridDim.x - 1) / gridDim.x;
    const long w0 = (long)blockIdx.x * per, w1 = w0 + per < wpf ? w0 + per : wpf;
    for (long w = w0 + threadIdx.x; w < w1; w += 256) {
        unsigned int va[PT], vb[PT];
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            const int i = ti * PT + p, j = tj * PT + p;
            va[p] = i < D ? a[((long)i * T + t) * wpf + w] : 0u;
            vb[p] = j < G ? b[((long)j * T + t) * wpf + w] : 0u;
        }
        tile.add(va, vb);
    }
    const Out v = (Out)tile.reduce(red);
    if (threadIdx.x < PT * PT) {
        const int p = threadIdx.x / PT, q = threadIdx.x % PT;
        const int i = ti * PT + p, j = tj * PT + q;
        if (i < D && j < G && v) {
            atomicAdd(&out[((long)i * G + j) * T + t], v);
            if (SYM && ti != tj) atomicAdd(&out[((long)j * G + i) * T + t], v);
        }
    }
}

}  // namespace

extern "C" {

int s2d_mask_plane_areas_u32(const uint32_t *bits, int F, long words_per_plane, unsigned *area, hipStream_t stream)
{
    if (F < 0 || words_per_plane < 1) return S2D_ERR_ARG;
    if (F == 0) return S2D_OK;
    hipLaunchKernelGGL(plane_popcount_kernel, dim3(F), dim3(256), 0, stream, bits, words_per_plane, area);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_mask_pair_counts_u64(const uint32_t *bits, int K, long words, unsigned long long *inter, hipStream_t stream)
{
    if (K < 0 || words < 0) return S2D_ERR_ARG;
    if (K == 0) return S2D_OK;
    if (s2d_zero_async(inter, sizeof(unsigned long long) * (size_t)K * K, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    if (words == 0) return S2D_OK;
    const int ntile = (K + PT - 1) / PT;
    const int npairs = ntile * (ntile + 1) / 2;
    hipLaunchKernelGGL((pair_tile_kernel<unsigned long long, true>), dim3(popc_chunks(words, npairs), npairs), dim3(256), 0, stream, bits,
                       K, bits, K, 1, words, ntile, inter);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_mask_cross_counts_u64(const uint32_t *a, int D, const uint32_t *b, int G, long words, unsigned long long *inter,
                              hipStream_t stream)
{
    if (D < 0 || G < 0 || words < 0) return S2D_ERR_ARG;
    if (D == 0 || G == 0) return S2D_OK;
    if (s2d_zero_async(inter, sizeof(unsigned long long) * (size_t)D * G, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    if (words == 0) return S2D_OK;
    const int ntd = (D + PT - 1) / PT, ntg = (G + PT - 1) / PT;
    const long ntiles = (long)ntd * ntg;
    if (ntiles >= 65536) return S2D_ERR_ARG;
    hipLaunchKernelGGL((pair_tile_kernel<unsigned long long, false>), dim3(popc_chunks(words, ntiles), (unsigned)ntiles), dim3(256), 0,
                       stream, a, D, b, G, 1, words, ntg, inter);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_mask_frame_cross_counts_i32(const uint32_t *a, int P, const uint32_t *b, int G, int T, long words_per_frame, int *out,
                                    hipStream_t stream)
{
    if (P < 0 || G < 0 || T < 0 || T >= 65536 || words_per_frame < 0 || words_per_frame >= (1L << 26)) return S2D_ERR_ARG;
    if (P == 0 || G == 0 || T == 0) return S2D_OK;
    if (!a || !b || !out) return S2D_ERR_ARG;
    if (s2d_zero_async(out, sizeof(int) * (size_t)P * G * T, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    if (words_per_frame == 0) return S2D_OK;
    const int ntp = (P + PT - 1) / PT, ntg = (G + PT - 1) / PT;
    const long ntiles = (long)ntp * ntg;
    if (ntiles >= 65536) return S2D_ERR_ARG;
    hipLaunchKernelGGL((pair_tile_kernel<int, false>), dim3(popc_chunks(words_per_frame, ntiles * T), (unsigned)ntiles, T), dim3(256), 0,
                       stream, a, P, b, G, T, words_per_frame, ntg, out);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
