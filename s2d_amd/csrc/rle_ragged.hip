// RLE parse, decode, tight boxes and areas for a CHUNK of planes of different sizes, one launch each however many images the chunk holds
// (s2d_amd/rle_ragged.py), and the keep rule of the image self-training merge (s2d_amd/selftrain.py; the reference's
// model_training/cutler/tools/get_self_training_ann.py:161-166).  The per-plane bodies are those of the fixed-size entry points
// (rle_planes.h; ytvis_eval.hip): here H, W and the word base of a plane come from its row of the plane table
//
//   plane int64 [P][4] = {word0, H, W, 0}     plane p: H x W, ceil(H*W/32) words from word word0 of the flat buffer
//
// which is the COCO chunk layout (include/s2d_hip.h, "Ragged layout"), so s2d_coco_mask_iou_ragged reads the decoded buffer in place.
// A row the buffer cannot hold (H or W < 1, H*W >= 2^31, words outside [0, total_words)) is skipped by every kernel: nothing is read
// or written for it.  The host checks the table before the call; the kernels do not rely on that.
//
// The way back, bit planes -> RLE strings, is the dual: s2d_rle_count_ragged_u32 and s2d_rle_positions_ragged_u32 run the bodies of
// s2d_rle_count_u8 / s2d_rle_positions_u8 (rle_encode.h) over a SELECTION of planes, sel int32 [S] (only the planes a cleanup changed
// are encoded again), reading pixels from the flat planes; s2d_rle_strings_ragged (rle.hip, beside the string kernels it launches)
// takes each plane's own H*W for the last run.
#include "bitplane.h"
#include "rle_encode.h"
#include "rle_planes.h"

namespace {

// rle_parse_kernel with the clamp taken from the plane's own size
__global__ __launch_bounds__(RLE_PARSE_T) void rle_parse_ragged_kernel(const uint8_t *__restrict__ chars, const long *__restrict__ str_off,
                                                                       const long *__restrict__ plane, int P, int *__restrict__ ends,
                                                                       int *__restrict__ nrun)
{
    const int f = blockIdx.x * (RLE_PARSE_T / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= P || nrun[f] >= 0) return;                     // whole waves
    const long H = plane[4L * f + 1], W = plane[4L * f + 2];
    const long hw = H >= 1 && W >= 1 && H < (1L << 31) && W < (1L << 31) && H * W < (1L << 31) ? H * W : 0;   // a bad row: every end 0
    const long b = str_off[f];
    const int m = rle_parse_string(chars + b, str_off[f + 1] - b, hw, ends + b, lane);
    if (lane == 0) nrun[f] = m;
}

// tiles [n_tiles][2] = {plane, column block of 256}; one workgroup per tile, a wave per 64 columns.  bits must be zero on entry
__global__ __launch_bounds__(RLE_DEC_T) void rle_decode_ragged_kernel(const int *__restrict__ ends, const long *__restrict__ run_off,
                                                                      const int *__restrict__ nrun, const long *__restrict__ plane, int P,
                                                                      const int *__restrict__ tiles, uint32_t *__restrict__ bits,
                                                                      long total_words)
{
    const int f = tiles[2L * blockIdx.x], cb = tiles[2L * blockIdx.x + 1];
    if (f < 0 || f >= P || cb < 0) return;
    const PlaneRow q = plane_row(plane, f, total_words);
    const long x0 = ((long)cb * (RLE_DEC_T / 64) + (threadIdx.x >> 6)) * 64;
    if (!q.ok || x0 >= q.W) return;                         // whole waves
    const long r0 = run_off[f];
    int n = nrun[f];
    const long cap = run_off[f + 1] - r0;                   // the plane's slots
    n = n < 0 ? 0 : ((long)n > cap ? (int)cap : n);
    rle_decode_columns(ends + r0, n, q.H, q.W, (int)x0, threadIdx.x & 63, bits + q.word0);
}

__global__ __launch_bounds__(256) void plane_bbox_ragged_kernel(const uint32_t *__restrict__ bits, const long *__restrict__ plane,
                                                                long total_words, int *__restrict__ bbox)
{
    const PlaneRow q = plane_row(plane, blockIdx.x, total_words);     // uniform over the workgroup
    int *b = bbox + 4L * blockIdx.x;
    if (!q.ok) {
        if (threadIdx.x < 4) b[threadIdx.x] = 0;
        return;
    }
    plane_tight_box(bits + q.word0, q.H, q.W, q.wpp, b);
}

// plane_popcount_kernel (mask_counts.hip) with the plane taken from its table row: the same body, a skipped row has area 0
__global__ __launch_bounds__(256) void plane_areas_ragged_kernel(const uint32_t *__restrict__ bits, const long *__restrict__ plane,
                                                                 long total_words, unsigned int *__restrict__ area)
{
    const PlaneRow q = plane_row(plane, blockIdx.x, total_words);     // uniform over the workgroup
    if (!q.ok) {
        if (threadIdx.x == 0) area[blockIdx.x] = 0u;
        return;
    }
    plane_popcount(bits + q.word0, q.wpp, area + blockIdx.x);
}

// rle_count_kernel / rle_positions_kernel (rle.hip) with the mask taken from the plane table: workgroup s encodes plane sel[s]; its
// column offsets start at col0[s] (the widths of the selection before it, summed on the host).  A selection entry that names no plane
// the buffer holds has no boundaries, area 0 and a zero box, and nothing else is read or written for it.
__global__ __launch_bounds__(RLE_ENC_T) void rle_count_ragged_kernel(const uint32_t *__restrict__ bits, const long *__restrict__ plane,
                                                                     int P, long total_words, const int *__restrict__ sel,
                                                                     const long *__restrict__ col0, int *__restrict__ col_off,
                                                                     int *__restrict__ nbound, int *__restrict__ area, int *__restrict__ bbox)
{
    const int s = blockIdx.x, f = sel[s];
    PlaneRow q;
    q.ok = f >= 0 && f < P;
    if (q.ok) q = plane_row(plane, f, total_words);
    if (!q.ok) {                                            // uniform over the workgroup
        if (threadIdx.x == 0) nbound[s] = area[s] = 0;
        if (threadIdx.x < 4) bbox[4L * s + threadIdx.x] = 0;
        return;
    }
    rle_count_body(RleBitFrame(bits + q.word0, q.wpp, q.W), q.H, q.W, col_off + col0[s], nbound + s, area + s, bbox + 4L * s);
}

__global__ __launch_bounds__(RLE_ENC_T) void rle_positions_ragged_kernel(const uint32_t *__restrict__ bits, const long *__restrict__ plane,
                                                                         int P, long total_words, const int *__restrict__ sel,
                                                                         const long *__restrict__ col0, const int *__restrict__ col_off,
                                                                         const long *__restrict__ frame_off, int *__restrict__ positions)
{
    const int s = blockIdx.x, f = sel[s];
    if (f < 0 || f >= P) return;
    const PlaneRow q = plane_row(plane, f, total_words);
    if (!q.ok) return;
    rle_positions_body(RleBitFrame(bits + q.word0, q.wpp, q.W), q.H, q.W, col_off + col0[s], positions + frame_off[s]);
}

constexpr int KEEP_T = 64;

// one workgroup (a wave) per image, a thread per previous-round mask d: keep[dt0 + d] = every g has 2 * inter < union
__global__ __launch_bounds__(KEEP_T) void selftrain_keep_kernel(const long long *__restrict__ inter, const int *__restrict__ area_d,
                                                                const int *__restrict__ area_g, const long *__restrict__ img,
                                                                int *__restrict__ keep)
{
    const long *r = img + 9L * blockIdx.x;
    const long D = r[4], G = r[5], dt0 = r[6], gt0 = r[7], pair0 = r[8];
    for (long d = threadIdx.x; d < D; d += KEEP_T) {
        const long ad = area_d[dt0 + d];
        int k = 1;
        for (long g = 0; g < G; ++g) {
            const long i = inter[pair0 + d * G + g];
            const long u = ad + (long)area_g[gt0 + g] - i;
            if (!(2 * i < u)) k = 0;                        // iou >= 0.5, or u == 0 (the reference's NaN < 0.5 is false)
        }
        keep[dt0 + d] = k;
    }
}

}  // namespace

extern "C" {

int s2d_rle_parse_ragged(const uint8_t *chars, const long *str_off, const long *plane, int P, int *ends, int *nrun, hipStream_t stream)
{
    if (P < 0) return S2D_ERR_ARG;
    if (P == 0) return S2D_OK;
    if (!chars || !str_off || !plane || !ends || !nrun) return S2D_ERR_ARG;
    hipLaunchKernelGGL(rle_parse_ragged_kernel, dim3(cdiv(P, RLE_PARSE_T / 64)), dim3(RLE_PARSE_T), 0, stream, chars, str_off, plane, P,
                       ends, nrun);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_rle_decode_ragged(const int *ends, const long *run_off, const int *nrun, const long *plane, int P, const int *tiles, int n_tiles,
                          uint32_t *bits, long total_words, hipStream_t stream)
{
    if (P < 0 || n_tiles < 0 || total_words < 0) return S2D_ERR_ARG;
    if (P == 0) return S2D_OK;
    if (!ends || !run_off || !nrun || !plane || !bits || (n_tiles && !tiles)) return S2D_ERR_ARG;
    if (total_words && s2d_zero_async(bits, sizeof(uint32_t) * (size_t)total_words, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    if (n_tiles == 0 || total_words == 0) return S2D_OK;
    hipLaunchKernelGGL(rle_decode_ragged_kernel, dim3(n_tiles), dim3(RLE_DEC_T), 0, stream, ends, run_off, nrun, plane, P, tiles, bits,
                       total_words);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_mask_plane_bbox_ragged_u32(const uint32_t *bits, const long *plane, int P, long total_words, int *bbox, hipStream_t stream)
{
    if (P < 0 || total_words < 0) return S2D_ERR_ARG;
    if (P == 0) return S2D_OK;
    if (!bits || !plane || !bbox) return S2D_ERR_ARG;
    hipLaunchKernelGGL(plane_bbox_ragged_kernel, dim3(P), dim3(256), 0, stream, bits, plane, total_words, bbox);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_mask_plane_areas_ragged_u32(const uint32_t *bits, const long *plane, int P, long total_words, unsigned *area, hipStream_t stream)
{
    if (P < 0 || total_words < 0) return S2D_ERR_ARG;
    if (P == 0) return S2D_OK;
    if (!bits || !plane || !area) return S2D_ERR_ARG;
    hipLaunchKernelGGL(plane_areas_ragged_kernel, dim3(P), dim3(256), 0, stream, bits, plane, total_words, area);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_rle_count_ragged_u32(const uint32_t *bits, const long *plane, int P, long total_words, const int *sel, int S, const long *col0,
                             int *col_off, int *nbound, int *area, int *bbox, hipStream_t stream)
{
    if (P < 0 || S < 0 || total_words < 0) return S2D_ERR_ARG;
    if (S == 0) return S2D_OK;
    if (!bits || !plane || !sel || !col0 || !col_off || !nbound || !area || !bbox) return S2D_ERR_ARG;
    hipLaunchKernelGGL(rle_count_ragged_kernel, dim3(S), dim3(RLE_ENC_T), 0, stream, bits, plane, P, total_words, sel, col0, col_off, nbound,
                       area, bbox);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_rle_positions_ragged_u32(const uint32_t *bits, const long *plane, int P, long total_words, const int *sel, int S, const long *col0,
                                 const int *col_off, const long *frame_off, int *positions, hipStream_t stream)
{
    if (P < 0 || S < 0 || total_words < 0) return S2D_ERR_ARG;
    if (S == 0) return S2D_OK;
    if (!bits || !plane || !sel || !col0 || !col_off || !frame_off || !positions) return S2D_ERR_ARG;
    hipLaunchKernelGGL(rle_positions_ragged_kernel, dim3(S), dim3(RLE_ENC_T), 0, stream, bits, plane, P, total_words, sel, col0, col_off,
                       frame_off, positions);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_selftrain_keep_ragged(const long long *inter, const int *area_d, const int *area_g, const long *img, int N, int *keep,
                              hipStream_t stream)
{
    if (N < 0) return S2D_ERR_ARG;
    if (N == 0) return S2D_OK;
    if (!img) return S2D_ERR_ARG;
    hipLaunchKernelGGL(selftrain_keep_kernel, dim3(N), dim3(KEEP_T), 0, stream, inter, area_d, area_g, img, keep);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
