// Video demo rendering (s2d_amd/demo.py; model_training/demo_video/demo.py + predictor.py of the reference): the instance
// overlay and the palette-PNG index map of every frame, made on the device from the u8 masks [K][T][H][W] that
// s2d_infer_masks_u8 writes.  Bandwidth-bound; no MFMA.
//
//  areas       per (instance, frame) set-pixel counts, 16-byte loads and a zero-byte count per dword
//  draw order  per frame: instances by descending area, ties in instance order (a stable sort), one workgroup per frame
//  render      one pass per frame: fill (c*a + p*(256-a) + 128) >> 8, then the 4-neighbour boundary painted opaque, in draw order;
//              index = 1 + the highest instance set at the pixel (the last-writer-wins loop of save_masks)
//
// A render thread owns 4 consecutive pixels of one row.  Per instance it reads the row's 4 mask bytes once; only when one of them is
// set does it read the 4 bytes above and below and the byte on each side, which its neighbours read as their own centre words,
// so those come from L1 / L2 and every mask byte leaves HBM about once.
#include "common.h"
#include "draw_order.h"

namespace {

// number of non-zero bytes of a dword: the exact zero-byte test (0x80 in every zero byte, no false positives)
__device__ __forceinline__ int nonzero_bytes(uint32_t x)
{
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    return 4 - __popc(z);
}

// areas[p] = set bytes of plane p (p = k * T + t, planes of HW bytes).  VEC: HW % 16 == 0 and the base 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void plane_areas_kernel(const uint8_t *__restrict__ masks, long HW, int *__restrict__ areas)
{
    const int p = blockIdx.y;
    const uint8_t *m = masks + (long)p * HW;
    int c = 0;
    if (VEC) {
        const uint4 *m4 = reinterpret_cast<const uint4 *>(m);
        const long n16 = HW >> 4;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) {
            const uint4 v = m4[i];
            c += nonzero_bytes(v.x) + nonzero_bytes(v.y) + nonzero_bytes(v.z) + nonzero_bytes(v.w);
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long)gridDim.x * 256) c += m[i] != 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&areas[p], c);
}

// 4 bytes of a row from x0 on; bytes at x >= W read as 0.  VEC: W % 4 == 0 and the row 4-byte aligned.
template <bool VEC>
__device__ __forceinline__ uint32_t load4(const uint8_t *__restrict__ row, int x0, int W)
{
    if (VEC) return *reinterpret_cast<const uint32_t *>(row + x0);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x0 + j < W) v |= (uint32_t)row[x0 + j] << (8 * j);
    return v;
}

__device__ __forceinline__ bool byte_set(uint32_t w, int j) { return ((w >> (8 * j)) & 0xFFu) != 0; }

// frames u8 [T][H][W][3] -> overlay u8 [T][H][W][3] (+ index u8 [T][H][W] unless null).  Grid (cdiv(H * ceil(W/4), 256), T).
// VEC: W % 4 == 0 and frames / masks / overlay / index 4-byte aligned (every row start then is).
template <bool VEC>
__global__ __launch_bounds__(256) void render_instances_kernel(const uint8_t *__restrict__ frames, int T, int H, int W,
                                                               const uint8_t *__restrict__ masks, int K, const int *__restrict__ order,
                                                               const uint8_t *__restrict__ colors, int alpha,
                                                               uint8_t *__restrict__ overlay, uint8_t *__restrict__ index)
{
    const int t = blockIdx.y;
    const int Wg = (W + 3) >> 2;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)H * Wg) return;
    const int y = (int)(g / Wg), x0 = (int)(g - (long)y * Wg) * 4;
    const int nx = min(4, W - x0);
    const long HW = (long)H * W;
    const long pix = (long)t * HW + (long)y * W + x0;

    int px[4][3];
    const uint8_t *fp = frames + pix * 3;
    if (VEC) {
        const uint32_t w0 = reinterpret_cast<const uint32_t *>(fp)[0], w1 = reinterpret_cast<const uint32_t *>(fp)[1],
                       w2 = reinterpret_cast<const uint32_t *>(fp)[2];
        const uint32_t w[3] = {w0, w1, w2};
#pragma unroll
        for (int b = 0; b < 12; ++b) px[b / 3][b % 3] = (w[b >> 2] >> (8 * (b & 3))) & 0xFF;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) px[j][c] = j < nx ? fp[j * 3 + c] : 0;
    }
    int idx[4] = {0, 0, 0, 0};
    const int inv = 256 - alpha;
    for (int r = 0; r < K; ++r) {
        const int k = order[(long)t * K + r];
        if ((unsigned)k >= (unsigned)K) continue;                       // a malformed order array reads nothing out of range
        const uint8_t *row = masks + ((long)k * T + t) * HW + (long)y * W;
        const uint32_t cw = load4<VEC>(row, x0, W);
        if (!cw) continue;
        const uint32_t up = y > 0 ? load4<VEC>(row - W, x0, W) : 0u;
        const uint32_t dn = y + 1 < H ? load4<VEC>(row + W, x0, W) : 0u;
        const bool lft = x0 > 0 && row[x0 - 1] != 0;
        const bool rgt = x0 + 4 < W && row[x0 + 4] != 0;
        const int cc[3] = {colors[3 * k], colors[3 * k + 1], colors[3 * k + 2]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!byte_set(cw, j)) continue;                              // bytes past the row end were loaded as 0
            const bool l = j == 0 ? lft : byte_set(cw, j - 1);
            const bool rr = j == 3 ? rgt : byte_set(cw, j + 1);
            const bool inner = l && rr && byte_set(up, j) && byte_set(dn, j);
#pragma unroll
            for (int c = 0; c < 3; ++c) px[j][c] = inner ? (cc[c] * alpha + px[j][c] * inv + 128) >> 8 : cc[c];
            idx[j] = max(idx[j], k + 1);
        }
    }

    uint8_t *op = overlay + pix * 3;
    if (VEC) {
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 12; ++b) w[b >> 2] |= (uint32_t)px[b / 3][b % 3] << (8 * (b & 3));
        reinterpret_cast<uint32_t *>(op)[0] = w[0];
        reinterpret_cast<uint32_t *>(op)[1] = w[1];
        reinterpret_cast<uint32_t *>(op)[2] = w[2];
        if (index) *reinterpret_cast<uint32_t *>(index + pix) = idx[0] | idx[1] << 8 | idx[2] << 16 | idx[3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nx) {
#pragma unroll
                for (int c = 0; c < 3; ++c) op[j * 3 + c] = (uint8_t)px[j][c];
                if (index) index[pix + j] = (uint8_t)idx[j];
            }
    }
}

constexpr int RENDER_MAX_K = 255;

}  // namespace

extern "C" {

int s2d_mask_frame_areas_i32(const uint8_t *masks, int K, int T, int H, int W, int *areas, int *order, hipStream_t stream)
{
    if (K < 0 || K > RENDER_MAX_K || T < 0 || T > 65535 || H < 1 || W < 1) return S2D_ERR_ARG;
    if (K == 0 || T == 0) return S2D_OK;
    const long HW = (long)H * W;
    if (s2d_zero_async(areas, sizeof(int) * (size_t)K * T, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    const bool vec = HW % 16 == 0 && reinterpret_cast<uintptr_t>(masks) % 16 == 0;
    const long per_block = 256L * 16 * 4;                                // 4 uint4 per thread per plane
    const int bx = (int)(HW / per_block < 1 ? 1 : (HW / per_block > 64 ? 64 : HW / per_block));
    if (vec)
        hipLaunchKernelGGL(plane_areas_kernel<true>, dim3(bx, K * T), dim3(256), 0, stream, masks, HW, areas);
    else
        hipLaunchKernelGGL(plane_areas_kernel<false>, dim3(bx, K * T), dim3(256), 0, stream, masks, HW, areas);
    if (order) hipLaunchKernelGGL(draw_order_kernel, dim3(T), dim3(256), 0, stream, areas, K, T, order);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_render_instances_u8(const uint8_t *frames, int T, int H, int W, const uint8_t *masks, int K, const int *order,
                            const uint8_t *colors, int alpha, uint8_t *overlay, uint8_t *index, hipStream_t stream)
{
    if (K < 0 || K > RENDER_MAX_K || T < 0 || T > 65535 || H < 1 || W < 1 || alpha < 0 || alpha > 256) return S2D_ERR_ARG;
    if (K > 0 && (!masks || !order || !colors)) return S2D_ERR_ARG;
    if (T == 0) return S2D_OK;
    const long groups = (long)H * ((W + 3) / 4);
    if (cdiv(groups, 256) > 0x7FFFFFFF / 2) return S2D_ERR_ARG;
    auto al4 = [](const void *p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; };
    const bool vec = W % 4 == 0 && al4(frames) && (K == 0 || al4(masks)) && al4(overlay) && (!index || al4(index));
    const dim3 grid(cdiv(groups, 256), T);
    if (vec)
        hipLaunchKernelGGL(render_instances_kernel<true>, grid, dim3(256), 0, stream, frames, T, H, W, masks, K, order, colors, alpha,
                           overlay, index);
    else
        hipLaunchKernelGGL(render_instances_kernel<false>, grid, dim3(256), 0, stream, frames, T, H, W, masks, K, order, colors,
                           alpha, overlay, index);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
