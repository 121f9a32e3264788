// Per-pixel work of the YTVIS video-instance evaluator (s2d_amd/ytvis_eval.py; the reference's YTVOSeval.computeIoU,
// mask2former_video/data_video/datasets/ytvis_api/ytvoseval.py:176-222, and YTVOS.loadRes areas, ytvos.py:239-252).
// A pair's video IoU is sum_t |d_t & g_t| / sum_t |d_t | g_t| with absent frames counting as empty planes, so it is exact
// from three integer quantities: the cross intersection counts of the two tracks and each track's area sum (the popcount kernels
// of mask_counts.hip: s2d_mask_cross_counts_u64, s2d_mask_plane_areas_u32).  This file makes the planes they count.
//
//   rle_parse_kernel       RLE strings -> run ends, one wave per string;
//   rle_decode_bits_kernel run ends -> one flat bit plane per frame (the layout of bitplane.h), a wave per 64 columns;
//   plane_bbox_kernel      per-plane tight boxes (mask_util.toBbox);
// each a thin wrapper of its body in rle_planes.h (rle_parse_string, rle_decode_columns, plane_tight_box).
#include "rle_planes.h"

// The three kernels are thin: the bodies live in rle_planes.h, shared with the ragged entry points of rle_ragged.hip.
namespace {

// nrun[f] < 0 on entry: parse string f (chars[str_off[f] .. str_off[f+1])) into ends[str_off[f] + j], j < nrun[f] out.
// nrun[f] >= 0: the frame's run ends are already in place (uncompressed RLE, or an absent frame with 0 runs): untouched.
__global__ __launch_bounds__(RLE_PARSE_T) void rle_parse_kernel(const uint8_t *__restrict__ chars, const long *__restrict__ str_off,
                                                                int F, long hw, int *__restrict__ ends, int *__restrict__ nrun)
{
    const int f = blockIdx.x * (RLE_PARSE_T / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= F || nrun[f] >= 0) return;                     // whole waves
    const long b = str_off[f];
    const int m = rle_parse_string(chars + b, str_off[f + 1] - b, hw, ends + b, lane);
    if (lane == 0) nrun[f] = m;
}

// planes must be zero on entry (the unaligned path ORs row segments that straddle words).  grid (ceil(W / 256), F)
__global__ __launch_bounds__(RLE_DEC_T) void rle_decode_bits_kernel(const int *__restrict__ ends, const long *__restrict__ run_off,
                                                                    const int *__restrict__ nrun, int H, int W, long wpf,
                                                                    uint32_t *__restrict__ bits)
{
    const int f = blockIdx.y;
    const int x0 = (blockIdx.x * (RLE_DEC_T / 64) + (threadIdx.x >> 6)) * 64;
    if (x0 >= W) return;                                   // whole waves
    rle_decode_columns(ends + run_off[f], nrun[f], H, W, x0, threadIdx.x & 63, bits + (long)f * wpf);
}

// bbox[f] = [x, y, w, h] of plane f; one workgroup per plane
__global__ __launch_bounds__(256) void plane_bbox_kernel(const uint32_t *__restrict__ bits, int H, int W, long wpf, int *__restrict__ bbox)
{
    plane_tight_box(bits + (long)blockIdx.x * wpf, H, W, wpf, bbox + 4L * blockIdx.x);
}

}  // namespace

extern "C" {

int s2d_rle_parse_strings(const uint8_t *chars, const long *str_off, int F, long hw, int *ends, int *nrun, hipStream_t stream)
{
    if (F < 0 || hw < 1 || hw >= (1L << 31)) return S2D_ERR_ARG;
    if (F == 0) return S2D_OK;
    hipLaunchKernelGGL(rle_parse_kernel, dim3(cdiv(F, RLE_PARSE_T / 64)), dim3(RLE_PARSE_T), 0, stream, chars, str_off, F, hw, ends, nrun);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_rle_decode_bits(const int *ends, const long *run_off, const int *nrun, int F, int H, int W, uint32_t *bits, hipStream_t stream)
{
    if (F < 0 || H < 1 || W < 1 || (long)H * W >= (1L << 31) || F >= 65536) return S2D_ERR_ARG;
    if (F == 0) return S2D_OK;
    const long wpf = ((long)H * W + 31) / 32;
    if (s2d_zero_async(bits, sizeof(uint32_t) * (size_t)F * wpf, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    hipLaunchKernelGGL(rle_decode_bits_kernel, dim3(cdiv(W, RLE_DEC_T), F), dim3(RLE_DEC_T), 0, stream, ends, run_off, nrun, H, W, wpf, bits);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_mask_plane_bbox_u32(const uint32_t *bits, int F, int H, int W, long words_per_plane, int *bbox, hipStream_t stream)
{
    if (F < 0 || H < 1 || W < 1 || (long)H * W >= (1L << 31) || words_per_plane != ((long)H * W + 31) / 32) return S2D_ERR_ARG;
    if (F == 0) return S2D_OK;
    hipLaunchKernelGGL(plane_bbox_kernel, dim3(F), dim3(256), 0, stream, bits, H, W, words_per_plane, bbox);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
