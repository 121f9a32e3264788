// The three per-plane bodies of the COCO RLE -> bit plane path, defined once for the fixed-size entry points (ytvis_eval.hip: F planes
// of one H x W) and the ragged ones (rle_ragged.hip: a chunk of planes, each with its own H, W and word base from a plane table):
//
//   rle_parse_string     pycocotools rleFrString (third party, restated): one wave per string, writing the running END of every run
//                        (the prefix the decoder searches) instead of the run lengths;
//   rle_decode_columns   run ends -> the flat bit plane (the layout of bitplane.h).  Runs are column-major, so a wave owns 64 adjacent
//                        columns and walks down the rows: every lane advances its own run cursor (found once by a binary search at
//                        the top of its column) and the wave's ballot is one row segment of the plane;
//   plane_tight_box      the plane's tight box (mask_util.toBbox), one workgroup of 256 threads per plane.
//
// A caller supplies the plane's geometry and pointers; the bodies read nothing else, so both callers compute the same bits.
#pragma once
#include "common.h"

constexpr int RLE_PARSE_T = 256;   // 4 waves, one string each
constexpr int RLE_DEC_T = 256;     // 4 waves, 64 columns each

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

// Parse the string s[0 .. len) into e[j], j < the returned number of counts (every lane returns it); ends are clamped to hw.
// A string of L chars holds at most L counts, so a caller that gives every string its own L slots never spills into the next one's.
// The whole wave calls this.  64 chars per step: a count ends at a char without the 0x20 "more" bit (terminal); its lane rebuilds the
// value from the chars since the previous terminal.  maskApi.c's delta (count m > 2 adds count m-2, in uint arithmetic) is
// two strided prefix sums -- odd m from 1, even m from 2 -- done as wave scans with running carries; the ends are one more
// scan.  A string that stops on a non-terminal char ends with that partial count, as the sequential parse does.
__device__ __forceinline__ int rle_parse_string(const uint8_t *__restrict__ s, long len, long hw, int *__restrict__ e, int lane)
{
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
    return m0;
}

// Columns x0 .. x0 + 63 (x0 % 64 == 0, x0 < W) of the H x W plane pl from its n run ends e; the whole wave calls this.  pl must be
// zero on entry unless W % 32 == 0 (the unaligned path ORs row segments that straddle words).
__device__ __forceinline__ void rle_decode_columns(const int *__restrict__ e, int n, int H, int W, int x0, int lane,
                                                   uint32_t *__restrict__ pl)
{
    const int x = x0 + lane;
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

// b[0..4) = [x, y, w, h] of the H x W plane pl (wpf = ceil(H*W/32) words): pycocotools rleToBbox (third party, restated; what
// mask_util.toBbox returns for the pseudo annotations of keymask_ident/convert_results_to_annotations.py:72).  rleToBbox takes the
// extremes of the first and last pixel of every run of ones (column-major), and sets the row range to [0, H-1] when a run starts in
// one column and ends in a later one.  Such a run holds pixel (H-1, c) and pixel (0, c+1), so that row range is the tight one as
// well: the box is the tight box of the set pixels, [0, 0, 0, 0] for an empty plane.  Each thread walks its words row segment by
// row segment (a word spans ceil(32 / W) + 1 rows at most).  All 256 threads of the workgroup call this (it holds a barrier).
__device__ __forceinline__ void plane_tight_box(const uint32_t *__restrict__ pl, int H, int W, long wpf, int *__restrict__ b)
{
    __shared__ int red[4][4];
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
        if (x_hi < 0) {
            b[0] = b[1] = b[2] = b[3] = 0;
        } else {
            b[0] = x_lo; b[1] = y_lo; b[2] = x_hi - x_lo + 1; b[3] = y_hi - y_lo + 1;
        }
    }
}
