// Per-pixel work of the YTVIS video-instance evaluator (s2d_amd/ytvis_eval.py; the reference's YTVOSeval.computeIoU,
// mask2former_video/data_video/datasets/ytvis_api/ytvoseval.py:176-222, and YTVOS.loadRes areas, ytvos.py:239-252).
// A pair's video IoU is sum_t |d_t & g_t| / sum_t |d_t | g_t| with absent frames counting as empty planes, so it is exact
// from three integer quantities: the cross intersection counts of the two tracks and each track's area sum (the popcount kernels
// of mask_counts.hip: s2d_mask_cross_counts_u64, s2d_mask_plane_areas_u32).  This file makes the planes they count.
//
//   rle_parse_kernel      pycocotools rleFrString (third party, restated): one wave per string, writing the running END
//                         of every run (the prefix the decoder searches) instead of the run lengths;
//   rle_decode_bits_kernel run ends -> one flat bit plane per frame (the layout of bitplane.h).  Runs are column-major, so a
//                         wave owns 64 adjacent columns and walks down the rows: every lane advances its own run cursor (found once by
//                         a binary search at the top of its column) and the wave's ballot is one row segment of the plane;
//   plane_bbox_kernel     per-plane tight boxes (mask_util.toBbox).
#include "common.h"

namespace {

constexpr int PARSE_T = 256;   // 4 waves, one string each

__device__ __forceinline__ unsigned int wave_scan_u32(unsigned int v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
__device__ __forceinline__ long wave_scan_i64(long v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// nrun[f] < 0 on entry: parse string f (chars[str_off[f] .. str_off[f+1])) into ends[str_off[f] + j], j < nrun[f] out.
// nrun[f] >= 0: the frame's run ends are already in place (uncompressed RLE, or an absent frame with 0 runs): untouched.
// A string of L chars holds at most L counts, so its slots never spill into the next frame's.
// One wave per string, 64 chars per step: a count ends at a char without the 0x20 "more" bit (terminal); its lane rebuilds the
// value from the chars since the previous terminal.  maskApi.c's delta (count m > 2 adds count m-2, in uint arithmetic) is
// two strided prefix sums -- odd m from 1, even m from 2 -- done as wave scans with running carries; the ends are one more
// scan.  A string that stops on a non-terminal char ends with that partial count, as the sequential parse does.
__global__ __launch_bounds__(PARSE_T) void rle_parse_kernel(const uint8_t *__restrict__ chars, const long *__restrict__ str_off,
                                                            int F, long hw, int *__restrict__ ends, int *__restrict__ nrun)
{
    const int f = blockIdx.x * (PARSE_T / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= F || nrun[f] >= 0) return;                     // whole waves
    const long b = str_off[f], len = str_off[f + 1] - b;
    const uint8_t *s = chars + b;
    int *e = ends + b;
    long start = 0, end_carry = 0;                          // first char of the open count; ends so far
    unsigned int odd_carry = 0u, even_carry = 0u;            // running sums of the odd (m >= 1) and even (m >= 2) chains
    int m0 = 0;                                             // counts before this step
    for (long p0 = 0; p0 < len; p0 += 64) {
        const long p = p0 + lane;
        const int ch = p < len ? (int)s[p] - 48 : 0x20;
        const bool term = p < len && (!(ch & 0x20) || p == len - 1);
        const unsigned long long tm = __ballot(term);
        const unsigned long long below = tm & ((1ull << lane) - 1ull);
        const int m = m0 + __popcll(below);
        long x = 0;
        if (term) {
            const long q0 = below ? p0 + 63 - __clzll(below) + 1 : start;
            int k = 0;
            for (long q = q0; q <= p; ++q, ++k) {
                const int c = (int)s[q] - 48;
                if (k < 13) x |= (long)(c & 0x1f) << (5 * k);
            }
            if (!(ch & 0x20) && (ch & 0x10) && 5 * k < 64) x |= -1L << (5 * k);
        }
        const unsigned int xv = (unsigned int)x;
        const unsigned int so = wave_scan_u32(term && (m & 1) ? xv : 0u, lane);
        const unsigned int se = wave_scan_u32(term && m >= 2 && !(m & 1) ? xv : 0u, lane);
        const unsigned int cnt = m == 0 ? xv : ((m & 1) ? odd_carry + so : even_carry + se);
        const long ce = wave_scan_i64(term ? (long)cnt : 0L, lane);
        if (term) {
            const long en = end_carry + ce;
            e[m] = (int)(en < hw ? en : hw);
        }
        odd_carry += __shfl(so, 63, 64);
        even_carry += __shfl(se, 63, 64);
        end_carry += __shfl(ce, 63, 64);
        m0 += __popcll(tm);
        if (tm) start = p0 + 63 - __clzll(tm) + 1;
    }
    if (lane == 0) nrun[f] = m0;
}

constexpr int DEC_T = 256;   // 4 waves, 64 columns each

// planes must be zero on entry (the unaligned path ORs row segments that straddle words).  grid (ceil(W / 256), F)
__global__ __launch_bounds__(DEC_T) void rle_decode_bits_kernel(const int *__restrict__ ends, const long *__restrict__ run_off,
                                                                const int *__restrict__ nrun, int H, int W, long wpf,
                                                                uint32_t *__restrict__ bits)
{
    const int f = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int x0 = (blockIdx.x * (DEC_T / 64) + (threadIdx.x >> 6)) * 64;
    if (x0 >= W) return;                                   // whole waves
    const int x = x0 + lane;
    const int n = nrun[f];
    const int *e = ends + run_off[f];
    uint32_t *pl = bits + (long)f * wpf;
    long c = (long)x * H;                                  // column-major index of (0, x)
    int j = n;                                             // first run whose end lies past c
    if (x < W) {
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((long)e[mid] > c) hi = mid; else lo = mid + 1;
        }
        j = lo;
    }
    long ej = j < n ? (long)e[j] : 0;
    const int nb = W - x0 < 64 ? W - x0 : 64;
    const bool aligned = (W & 31) == 0;                    // x0 % 64 == 0: every row segment starts a word
    for (int y = 0; y < H; ++y, ++c) {
        bool v = false;
        if (x < W) {
            while (j < n && ej <= c) { ++j; ej = j < n ? (long)e[j] : 0; }
            v = j < n && (j & 1);
        }
        const unsigned long long bm = __ballot(v);
        const long p = (long)y * W + x0;                   // flat index of this wave's first pixel of row y
        if (aligned) {
            if (lane == 0) pl[p >> 5] = (uint32_t)bm;
            else if (lane == 32 && nb > 32) pl[(p >> 5) + 1] = (uint32_t)(bm >> 32);
        } else if (lane == 0 && bm) {
            // pixel p + k -> bit (off + k) counted from word w: up to three words; set bits are valid pixels (< H*W)
            const int off = (int)(p & 31);
            const long w = p >> 5;
            atomicOr(&pl[w], (uint32_t)(bm << off));
            const uint32_t w1 = (uint32_t)(off ? bm >> (32 - off) : bm >> 32);
            if (w1) atomicOr(&pl[w + 1], w1);
            const uint32_t w2 = off ? (uint32_t)(bm >> (64 - off)) : 0u;
            if (w2) atomicOr(&pl[w + 2], w2);
        }
    }
}

// bbox[f] = [x, y, w, h] of plane f: pycocotools rleToBbox (third party, restated; what mask_util.toBbox returns for the pseudo
// annotations of keymask_ident/convert_results_to_annotations.py:72).  rleToBbox takes the extremes of the first and last pixel
// of every run of ones (column-major), and sets the row range to [0, H-1] when a run starts in one column and ends in a later one.
// Such a run holds pixel (H-1, c) and pixel (0, c+1), so that row range is the tight one as well: the box is the tight box of the
// set pixels, [0, 0, 0, 0] for an empty plane.  Each thread walks its words row segment by row segment (a word spans
// ceil(32 / W) + 1 rows at most); one workgroup per plane.
__global__ __launch_bounds__(256) void plane_bbox_kernel(const uint32_t *__restrict__ bits, int H, int W, long wpf, int *__restrict__ bbox)
{
    __shared__ int red[4][4];
    const uint32_t *pl = bits + (long)blockIdx.x * wpf;
    int x_lo = 0x7fffffff, y_lo = 0x7fffffff, x_hi = -1, y_hi = -1;
    for (long w = threadIdx.x; w < wpf; w += 256) {
        uint32_t v = pl[w];
        if (!v) continue;
        const long p = w * 32;
        int y = (int)(p / W), c = (int)(p - (long)y * W);
        int used = 0;
        while (v) {
            const int len = 32 - used < W - c ? 32 - used : W - c;
            const uint32_t seg = len >= 32 ? v : (v & ((1u << len) - 1u));
            if (seg) {
                const int lo = __builtin_ctz(seg), hi = 31 - __builtin_clz(seg);
                x_lo = min(x_lo, c + lo); x_hi = max(x_hi, c + hi);
                y_lo = min(y_lo, y); y_hi = max(y_hi, y);
            }
            v = len >= 32 ? 0u : v >> len;
            used += len; c = 0; ++y;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x_lo = min(x_lo, __shfl_xor(x_lo, o, 64)); y_lo = min(y_lo, __shfl_xor(y_lo, o, 64));
        x_hi = max(x_hi, __shfl_xor(x_hi, o, 64)); y_hi = max(y_hi, __shfl_xor(y_hi, o, 64));
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wv][0] = x_lo; red[wv][1] = y_lo; red[wv][2] = x_hi; red[wv][3] = y_hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) {
            x_lo = min(x_lo, red[i][0]); y_lo = min(y_lo, red[i][1]); x_hi = max(x_hi, red[i][2]); y_hi = max(y_hi, red[i][3]);
        }
        int *b = bbox + 4L * blockIdx.x;
        if (x_hi < 0) {
            b[0] = b[1] = b[2] = b[3] = 0;
        } else {
            b[0] = x_lo; b[1] = y_lo; b[2] = x_hi - x_lo + 1; b[3] = y_hi - y_lo + 1;
        }
    }
}

}  // namespace

extern "C" {

int s2d_rle_parse_strings(const uint8_t *chars, const long *str_off, int F, long hw, int *ends, int *nrun, hipStream_t stream)
{
    if (F < 0 || hw < 1 || hw >= (1L << 31)) return S2D_ERR_ARG;
    if (F == 0) return S2D_OK;
    hipLaunchKernelGGL(rle_parse_kernel, dim3(cdiv(F, PARSE_T / 64)), dim3(PARSE_T), 0, stream, chars, str_off, F, hw, ends, nrun);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_rle_decode_bits(const int *ends, const long *run_off, const int *nrun, int F, int H, int W, uint32_t *bits, hipStream_t stream)
{
    if (F < 0 || H < 1 || W < 1 || (long)H * W >= (1L << 31) || F >= 65536) return S2D_ERR_ARG;
    if (F == 0) return S2D_OK;
    const long wpf = ((long)H * W + 31) / 32;
    if (s2d_zero_async(bits, sizeof(uint32_t) * (size_t)F * wpf, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    hipLaunchKernelGGL(rle_decode_bits_kernel, dim3(cdiv(W, DEC_T), F), dim3(DEC_T), 0, stream, ends, run_off, nrun, H, W, wpf, bits);
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
