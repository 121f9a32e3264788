// Test-time frame resize of the YTVIS loader (s2d_amd/data/test_loader.py): detectron2's ResizeTransform.apply_image on uint8
// frames, i.e. PIL Image.resize(BILINEAR) (third party, restated: libImaging/Resample.c, ImagingResample for 8-bit images).
// PIL's bilinear antialiases (the triangle's support widens with the downscale factor), works in 22-bit fixed point and runs two
// separable passes, horizontal first, with a uint8 intermediate.  The per-axis coefficient tables are built on the host in
// float64 exactly as PIL builds them (s2d_amd/data/resize.py); this kernel does integer arithmetic only.
//
// One workgroup owns a tile of RS_BW output columns x BH output rows of one frame:
//   1. the input rectangle its taps reach (the band's input rows x the tile's input columns, HWC bytes) is staged in LDS
//      with 16-byte loads (a chunk that is not wholly inside the source buffer falls back to byte loads);
//   2. the horizontal pass runs over every staged row into a channel-planar u8 intermediate in LDS;
//   3. the vertical pass reads the intermediate and writes the CHW output.
// An axis whose size does not change gets an identity table (one tap of weight 2^22), which reproduces PIL skipping that pass.
#include "common.h"

namespace {

constexpr int RS_T = 256;    // 4 waves
constexpr int RS_BW = 64;    // output columns per workgroup: one per lane
constexpr int RS_PREC = 22;  // PIL's PRECISION_BITS for 8-bit images (32 - 8 - 2)

__device__ __forceinline__ uint8_t clip8(int v)
{
    if (v >= (1 << RS_PREC << 8)) return 255;
    if (v <= 0) return 0;
    return (uint8_t)(v >> RS_PREC);
}

// hb / vb: (min, size) per output column / row; hk [W1][KH], vk [H1][KV]: 22-bit fixed-point weights.  The tables are monotone
// (min and min + size never decrease along the axis; the host checks it), so a tile's input span is fixed by its first and last
// output.  LDS: rect [rows_max][span_q] uint4 | tmp [3][rows_max][RS_BW] u8 | weights [KH][RS_BW] int.  grid (ceil(W1/64), ceil(H1/BH), T)
__global__ __launch_bounds__(RS_T) void resize_bilinear_u8_kernel(const uint8_t *__restrict__ src, long src_bytes, int H0, int W0,
                                                                  const int *__restrict__ hb, const int *__restrict__ hk, int KH,
                                                                  const int *__restrict__ vb, const int *__restrict__ vk, int KV,
                                                                  int H1, int W1, int BH, int rows_max, int span_q,
                                                                  uint8_t *__restrict__ dst)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
    uint4 *rect = reinterpret_cast<uint4 *>(rs_lds);
    uint8_t *tmp = rs_lds + (size_t)rows_max * span_q * 16;
    int *wk = reinterpret_cast<int *>(tmp + (size_t)3 * rows_max * RS_BW);      // 3 * rows_max * 64 is a multiple of 4

    const int f = blockIdx.z;
    const int x0 = blockIdx.x * RS_BW, y0 = blockIdx.y * BH;
    const int nx = W1 - x0 < RS_BW ? W1 - x0 : RS_BW;
    const int ny = H1 - y0 < BH ? H1 - y0 : BH;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;

    // the input rectangle of the tile
    const int ry0 = vb[2 * y0];
    int nrows = vb[2 * (y0 + ny - 1)] + vb[2 * (y0 + ny - 1) + 1] - ry0;
    if (nrows > rows_max) nrows = rows_max;
    if (ry0 + nrows > H0) nrows = H0 - ry0;
    const int cx0 = hb[2 * x0];
    int ncols = hb[2 * (x0 + nx - 1)] + hb[2 * (x0 + nx - 1) + 1] - cx0;
    if (cx0 + ncols > W0) ncols = W0 - cx0;
    if (ncols < 0) ncols = 0;
    const long nbytes = (long)ncols * 3;

    // 1. stage rows [ry0, ry0 + nrows) x bytes [3 cx0, 3 (cx0 + ncols)) of frame f; row rr starts `sh` bytes into its first chunk
    const uintptr_t s_lo = (uintptr_t)src, s_hi = s_lo + (uintptr_t)src_bytes;
    for (int rr = wv; rr < nrows; rr += RS_T / 64) {
        const uintptr_t a = (uintptr_t)(src + ((long)f * H0 + ry0 + rr) * W0 * 3 + (long)cx0 * 3);
        const uintptr_t a16 = a & ~(uintptr_t)15;
        int nq = (int)((a - a16 + nbytes + 15) >> 4);
        if (nq > span_q) nq = span_q;
        for (int q = lane; q < nq; q += 64) {
            const uintptr_t p = a16 + (uintptr_t)q * 16;
            uint4 v;
            if (p >= s_lo && p + 16 <= s_hi) {
                v = *reinterpret_cast<const uint4 *>(p);
            } else {                                       // the buffer's first or last chunk: only the bytes inside it
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                for (int b = 0; b < 16; ++b)
                    if (p + b >= s_lo && p + b < s_hi) w[b >> 2] |= (uint32_t)(*reinterpret_cast<const uint8_t *>(p + b)) << (8 * (b & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            rect[(size_t)rr * span_q + q] = v;
        }
    }
    // the horizontal weights of the tile's columns, [k][column]: lane-contiguous reads in pass 2
    for (int i = threadIdx.x; i < KH * RS_BW; i += RS_T) {
        const int k = i / RS_BW, xl = i - k * RS_BW;
        wk[i] = xl < nx ? hk[(long)(x0 + xl) * KH + k] : 0;
    }
    __syncthreads();

    // 2. horizontal pass: lane = output column, waves stride the staged rows
    if (lane < nx) {
        const int x = x0 + lane;
        int xm = hb[2 * x] - cx0, xs = hb[2 * x + 1];
        if (xm < 0) xm = 0;
        if (xs > KH) xs = KH;
        if (xm + xs > ncols) xs = ncols - xm;
        for (int rr = wv; rr < nrows; rr += RS_T / 64) {
            const uintptr_t a = (uintptr_t)(src + ((long)f * H0 + ry0 + rr) * W0 * 3 + (long)cx0 * 3);
            const uint8_t *p = reinterpret_cast<const uint8_t *>(rect + (size_t)rr * span_q) + (a & 15) + xm * 3;
            int s0 = 1 << (RS_PREC - 1), s1 = s0, s2 = s0;
            for (int k = 0; k < xs; ++k) {
                const int w = wk[k * RS_BW + lane];
                s0 += (int)p[3 * k] * w;
                s1 += (int)p[3 * k + 1] * w;
                s2 += (int)p[3 * k + 2] * w;
            }
            tmp[(0 * rows_max + rr) * RS_BW + lane] = clip8(s0);
            tmp[(1 * rows_max + rr) * RS_BW + lane] = clip8(s1);
            tmp[(2 * rows_max + rr) * RS_BW + lane] = clip8(s2);
        }
    }
    __syncthreads();

    // 3. vertical pass: lane = output column, waves stride the band's output rows (the row's taps are wave-uniform)
    if (lane < nx) {
        const int x = x0 + lane;
        for (int yl = wv; yl < ny; yl += RS_T / 64) {
            const int y = y0 + yl;
            int ym = vb[2 * y] - ry0, ys = vb[2 * y + 1];
            if (ym < 0) ym = 0;
            if (ys > KV) ys = KV;
            if (ym + ys > nrows) ys = nrows - ym;
            int s0 = 1 << (RS_PREC - 1), s1 = s0, s2 = s0;
            for (int k = 0; k < ys; ++k) {
                const int w = vk[(long)y * KV + k];
                const int r = ym + k;
                s0 += (int)tmp[(0 * rows_max + r) * RS_BW + lane] * w;
                s1 += (int)tmp[(1 * rows_max + r) * RS_BW + lane] * w;
                s2 += (int)tmp[(2 * rows_max + r) * RS_BW + lane] * w;
            }
            const long plane = (long)H1 * W1;
            uint8_t *o = dst + (long)f * 3 * plane + (long)y * W1 + x;
            o[0] = clip8(s0);
            o[plane] = clip8(s1);
            o[2 * plane] = clip8(s2);
        }
    }
}

}  // namespace

extern "C" {

long s2d_resize_lds_bytes(int rows_max, int span_q, int kh)
{
    return (long)rows_max * span_q * 16 + (long)3 * rows_max * RS_BW + (long)kh * RS_BW * 4;
}

int s2d_resize_bilinear_u8(const uint8_t *src, int T, int H0, int W0, const int *h_bounds, const int *h_coeffs, int kh,
                           const int *v_bounds, const int *v_coeffs, int kv, int H1, int W1, int band_rows, int rows_max,
                           int span_q, uint8_t *dst, hipStream_t stream)
{
    if (T < 0 || H0 < 1 || W0 < 1 || H1 < 1 || W1 < 1 || kh < 1 || kv < 1 || band_rows < 1 || rows_max < 1 || span_q < 1)
        return S2D_ERR_ARG;
    if (T > 65535 || (long)T * H0 * W0 * 3 >= (1L << 40) || (long)H0 * W0 * 3 >= (1L << 31) || (long)H1 * W1 >= (1L << 31))
        return S2D_ERR_ARG;
    const long lds = s2d_resize_lds_bytes(rows_max, span_q, kh);
    if (lds > 65536) return S2D_ERR_ARG;
    if (T == 0) return S2D_OK;
    const dim3 grid(cdiv(W1, RS_BW), cdiv(H1, band_rows), T);
    if (grid.y > 65535) return S2D_ERR_ARG;
    hipLaunchKernelGGL(resize_bilinear_u8_kernel, grid, dim3(RS_T), (size_t)lds, stream, src, (long)T * H0 * W0 * 3, H0, W0,
                       h_bounds, h_coeffs, kh, v_bounds, v_coeffs, kv, H1, W1, band_rows, rows_max, span_q, dst);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
