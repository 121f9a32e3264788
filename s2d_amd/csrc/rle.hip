// COCO run-length encoding of binary masks on the device: the wire format either side of the path --
// `mask_util.encode(np.array(mask[:, :, None], order="F"))` in the evaluator (mask2former_video/data_video/ytvis_eval.py:
// 345-350) and in the keymask annotation writer (keymask_ident/annotations.py:100-106, with `area` and `toBbox`).
// pycocotools is a third-party dependency absent from the reference tree; this restates its published algorithm
// (maskApi.c rleEncode: runs of the COLUMN-major flattened mask, alternating 0s / 1s, starting with the zero run).
//
// A boolean [T,H,W] prediction is 0.9 MB per 720p frame as bytes and a few KB as runs, so encoding where the mask was
// made removes the device->host copy that dominates inference_video (eval row).  Two passes over a frame, one
// workgroup per frame, a thread owning 4 adjacent columns and walking down the rows (row-major memory is read 4 bytes per
// lane, coalesced along x; the run order is column-major, so the ownership is by column):
//   pass 1 counts the run boundaries of every column (a boundary = pixel != its column-major predecessor), scans the
//          counts over the columns (exclusive), and reduces area and the tight box;
//   pass 2 walks the same way and writes each boundary's column-major position x*H + y at its slot.
// The host turns positions into run lengths (differences) and into the LEB-like ASCII string (s2d_amd/rle.py).
// The bodies of both passes and of the string kernels are rle_encode.h's, shared with the ragged bit-plane encoder (rle_ragged.hip).
#include "rle_encode.h"

namespace {

constexpr int RT = RLE_ENC_T;

// the bodies are rle_encode.h's, shared with the ragged bit-plane encoder (rle_ragged.hip); here a workgroup takes byte mask f
__global__ __launch_bounds__(RT) void rle_count_kernel(const uint8_t *__restrict__ masks, int H, int W, int *__restrict__ col_off,
                                                       int *__restrict__ nbound, int *__restrict__ area, int *__restrict__ bbox)
{
    const int f = blockIdx.x;
    rle_count_body(RleU8Frame(masks + (long)f * H * W, W), H, W, col_off + (long)f * W, nbound + f, area + f, bbox + 4 * f);
}

__global__ __launch_bounds__(RT) void rle_positions_kernel(const uint8_t *__restrict__ masks, int H, int W, const int *__restrict__ col_off,
                                                           const long *__restrict__ frame_off, int *__restrict__ positions)
{
    const int f = blockIdx.x;
    rle_positions_body(RleU8Frame(masks + (long)f * H * W, W), H, W, col_off + (long)f * W, positions + frame_off[f]);
}

__global__ __launch_bounds__(256) void rle_len_kernel(RleStr p, int *__restrict__ len)
{
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c < p.ncounts) rle_len_body(p, c, len);
}
__global__ __launch_bounds__(256) void rle_chars_kernel(RleStr p, const int *__restrict__ len, const int *__restrict__ off,
                                                        uint8_t *__restrict__ chars, long *__restrict__ str_off)
{
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c < p.ncounts) rle_chars_body(p, c, len, off, chars, str_off);
}

}  // namespace

extern "C" {

long s2d_rle_string_workspace_bytes(long ncounts)
{
    if (ncounts <= 0) return 0;
    return 2 * ((ncounts * 4 + 255) / 256 * 256) + (long)s2d_exclusive_scan_i32_temp_bytes((size_t)ncounts) + 256;
}

// positions -> strings for F masks; plane / sel / P: the ragged form (RleStr), NULL / NULL / 0 for masks of one size hw
static int rle_strings(const int *positions, const long *frame_off, int F, long hw, const long *plane, const int *sel, int P, long ncounts,
                       void *workspace, long workspace_bytes, uint8_t *chars, long *str_off, hipStream_t stream)
{
    if (F < 0 || ncounts < F || ncounts * 7 >= (1L << 31)) return S2D_ERR_ARG;
    if (F == 0) return S2D_OK;
    if (workspace_bytes < s2d_rle_string_workspace_bytes(ncounts)) return S2D_ERR_ARG;
    const long slab = (ncounts * 4 + 255) / 256 * 256;
    int *len = reinterpret_cast<int *>(workspace);
    int *off = reinterpret_cast<int *>(reinterpret_cast<char *>(workspace) + slab);
    void *tmp = reinterpret_cast<char *>(workspace) + 2 * slab;
    RleStr p{positions, frame_off, F, hw, ncounts, plane, sel, P};
    hipLaunchKernelGGL(rle_len_kernel, dim3(cdiv(ncounts, 256)), dim3(256), 0, stream, p, len);
    if (int e = s2d_exclusive_scan_i32(len, off, (size_t)ncounts, tmp, (size_t)(workspace_bytes - 2 * slab), stream)) return e;
    hipLaunchKernelGGL(rle_chars_kernel, dim3(cdiv(ncounts, 256)), dim3(256), 0, stream, p, len, off, chars, str_off);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_rle_strings_u8(const int *positions, const long *frame_off, int F, long hw, long ncounts, void *workspace, long workspace_bytes,
                       uint8_t *chars, long *str_off, hipStream_t stream)
{
    if (hw < 1 || hw >= (1L << 31)) return S2D_ERR_ARG;
    return rle_strings(positions, frame_off, F, hw, nullptr, nullptr, 0, ncounts, workspace, workspace_bytes, chars, str_off, stream);
}

long s2d_rle_strings_ragged_workspace_bytes(long ncounts) { return s2d_rle_string_workspace_bytes(ncounts); }

int s2d_rle_strings_ragged(const int *positions, const long *frame_off, const long *plane, int P, const int *sel, int S, long ncounts,
                           void *workspace, long workspace_bytes, uint8_t *chars, long *str_off, hipStream_t stream)
{
    if (P < 0 || S < 0) return S2D_ERR_ARG;
    if (S == 0) return S2D_OK;
    if (!positions || !frame_off || !plane || !sel || !workspace || !chars || !str_off) return S2D_ERR_ARG;
    return rle_strings(positions, frame_off, S, 0, plane, sel, P, ncounts, workspace, workspace_bytes, chars, str_off, stream);
}

int s2d_rle_count_u8(const uint8_t *masks, int F, int H, int W, int *col_off, int *nbound, int *area, int *bbox, hipStream_t stream)
{
    if (F < 0 || H < 1 || W < 1 || (long)H * W >= (1L << 31)) return S2D_ERR_ARG;
    if (F == 0) return S2D_OK;
    hipLaunchKernelGGL(rle_count_kernel, dim3(F), dim3(RT), 0, stream, masks, H, W, col_off, nbound, area, bbox);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_rle_positions_u8(const uint8_t *masks, int F, int H, int W, const int *col_off, const long *frame_off, int *positions,
                         hipStream_t stream)
{
    if (F < 0 || H < 1 || W < 1 || (long)H * W >= (1L << 31)) return S2D_ERR_ARG;
    if (F == 0) return S2D_OK;
    hipLaunchKernelGGL(rle_positions_kernel, dim3(F), dim3(RT), 0, stream, masks, H, W, col_off, frame_off, positions);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
