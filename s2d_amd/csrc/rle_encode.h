// The per-mask bodies of the mask -> COCO RLE path, defined once for the fixed-size entry points (rle.hip: F byte masks of one H x W)
// and the ragged ones (rle_ragged.hip: a selection of bit planes, each with its own H, W and word base from a plane table) -- the
// dual of rle_planes.h, which holds the bodies of the decode:
//
//   rle_count_body       pass 1: the run boundaries of every column (a boundary = pixel != its column-major predecessor), their
//                        exclusive scan over the columns, the area and the tight box;
//   rle_positions_body   pass 2: each boundary's column-major position x*H + y at its slot;
//   rle_len_body / rle_chars_body   run lengths -> the ASCII string of maskApi.c rleToString.
//
// A body reads its pixels through a frame type (RleU8Frame: a byte mask, RleBitFrame: a flat bit plane of bitplane.h) and nothing
// else depends on where the pixels came from, so a plane's string comes out byte for byte as the string of the same byte mask.
#pragma once
#include "bitplane.h"

constexpr int RLE_ENC_T = 1024;   // threads per mask workgroup: 4096 columns per sweep, a thread owning 4 adjacent columns

struct RleU8Frame {
    const uint8_t *fr;
    int W;
    bool vec;
    __device__ __forceinline__ RleU8Frame(const uint8_t *f, int W_) : fr(f), W(W_), vec((W_ & 3) == 0 && (reinterpret_cast<uintptr_t>(f) & 3) == 0) {}
    __device__ __forceinline__ unsigned int at(int y, int x) const { return fr[(long)y * W + x] != 0; }
    // pixels (y, x .. x + 3), x % 4 == 0, 0 at and beyond W
    __device__ __forceinline__ void row4(int y, int x, unsigned int (&v)[4]) const
    {
        if (vec) {
            const unsigned int w4 = *reinterpret_cast<const unsigned int *>(fr + (long)y * W + x);
            v[0] = (w4 & 0xFFu) != 0; v[1] = (w4 & 0xFF00u) != 0; v[2] = (w4 & 0xFF0000u) != 0; v[3] = (w4 & 0xFF000000u) != 0;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = x + j < W ? (fr[(long)y * W + x + j] != 0) : 0u;
        }
    }
};

struct RleBitFrame {
    const uint32_t *pl;
    long wpp;
    int W;
    __device__ __forceinline__ RleBitFrame(const uint32_t *p, long wpp_, int W_) : pl(p), wpp(wpp_), W(W_) {}
    __device__ __forceinline__ unsigned int at(int y, int x) const { return flat_bits(pl, wpp, (long)y * W + x) & 1u; }
    __device__ __forceinline__ void row4(int y, int x, unsigned int (&v)[4]) const
    {
        const unsigned int b = flat_bits(pl, wpp, (long)y * W + x);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = x + j < W ? ((b >> j) & 1u) : 0u;
    }
};

// value of the column-major predecessor of (0, x): (H-1, x-1), or 0 before the first pixel
template <class Frame> __device__ __forceinline__ unsigned int rle_col_pred(const Frame &fr, int H, int x)
{
    return x > 0 ? fr.at(H - 1, x - 1) : 0u;
}

// col_off[x] = boundaries in the columns before x, nbound[0] = all of them, area[0], bbox[0..4) = x, y, w, h (rleToBbox: zeros for an
// empty mask).  All RLE_ENC_T threads of the workgroup call this (it holds barriers).
template <class Frame>
__device__ __forceinline__ void rle_count_body(const Frame &fr, int H, int W, int *__restrict__ col_off, int *__restrict__ nbound,
                                               int *__restrict__ area, int *__restrict__ bbox)
{
    constexpr int RT = RLE_ENC_T;
    __shared__ int scan[RT];
    __shared__ int carry;
    int t_area = 0, xs = W, xe = -1, ys = H, ye = -1;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int x0 = 0; x0 < W; x0 += 4 * RT) {
        const int x = x0 + 4 * threadIdx.x;
        int cnt[4] = {0, 0, 0, 0};
        if (x < W) {
            unsigned int prev[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) prev[j] = x + j < W ? rle_col_pred(fr, H, x + j) : 0u;
            for (int y = 0; y < H; ++y) {
                unsigned int v[4];
                fr.row4(y, x, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    cnt[j] += (int)(v[j] != prev[j]);
                    prev[j] = v[j];
                    if (v[j]) { ++t_area; xs = min(xs, x + j); xe = max(xe, x + j); }
                }
                if (v[0] | v[1] | v[2] | v[3]) { ys = min(ys, y); ye = max(ye, y); }
            }
        }
        // exclusive scan of the 4*RT column counts of this sweep (+ carry from earlier sweeps)
        const int mine = cnt[0] + cnt[1] + cnt[2] + cnt[3];
        scan[threadIdx.x] = mine;
        __syncthreads();
        for (int o = 1; o < RT; o <<= 1) {
            const int add = threadIdx.x >= o ? scan[threadIdx.x - o] : 0;
            __syncthreads();
            scan[threadIdx.x] += add;
            __syncthreads();
        }
        int base = carry + scan[threadIdx.x] - mine;
        if (x < W) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < W) { col_off[x + j] = base; base += cnt[j]; }
        }
        __syncthreads();
        if (threadIdx.x == RT - 1) carry += scan[RT - 1];
        __syncthreads();
    }
    // reductions: area (sum), box (min / max)
    auto wave_red = [&](int v, int op) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int u = __shfl_xor(v, o, 64);
            v = op == 0 ? v + u : (op == 1 ? min(v, u) : max(v, u));
        }
        return v;
    };
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int vals[5] = {wave_red(t_area, 0), wave_red(xs, 1), wave_red(ys, 1), wave_red(xe, 2), wave_red(ye, 2)};
    __shared__ int r5[5][RT / 64];
    if (lane == 0)
        for (int i = 0; i < 5; ++i) r5[i][wv] = vals[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, bxs = W, bys = H, bxe = -1, bye = -1;
        for (int w = 0; w < RT / 64; ++w) { a += r5[0][w]; bxs = min(bxs, r5[1][w]); bys = min(bys, r5[2][w]); bxe = max(bxe, r5[3][w]); bye = max(bye, r5[4][w]); }
        nbound[0] = carry;
        area[0] = a;
        if (a == 0) { bbox[0] = bbox[1] = bbox[2] = bbox[3] = 0; }   // rleToBbox of an empty mask
        else { bbox[0] = bxs; bbox[1] = bys; bbox[2] = bxe - bxs + 1; bbox[3] = bye - bys + 1; }
    }
}

// out[col_off[x] ...] = the column-major positions of column x's boundaries
template <class Frame>
__device__ __forceinline__ void rle_positions_body(const Frame &fr, int H, int W, const int *__restrict__ col_off, int *__restrict__ out)
{
    constexpr int RT = RLE_ENC_T;
    for (int x0 = 0; x0 < W; x0 += 4 * RT) {
        const int x = x0 + 4 * threadIdx.x;
        if (x >= W) continue;
        unsigned int prev[4];
        int slot[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            prev[j] = x + j < W ? rle_col_pred(fr, H, x + j) : 0u;
            slot[j] = x + j < W ? col_off[x + j] : 0;
        }
        for (int y = 0; y < H; ++y) {
            unsigned int v[4];
            fr.row4(y, x, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (v[j] != prev[j]) out[slot[j]++] = (x + j) * H + y;
                prev[j] = v[j];
            }
        }
    }
}

// ---- run lengths -> the ASCII string of maskApi.c rleToString, on the device --------------------------------------------
// count c of mask f (local index i, n boundaries): cnt(i) = pos(i) - pos(i-1) with pos(-1) = 0, pos(n) = H*W; the value
// written is x = cnt(i) - cnt(i-2) for i > 2; chars: 5 bits each, bit 5 = "more", + 48.
struct RleStr {
    const int *pos;
    const long *frame_off;     // [F+1]
    int F;
    long hw, ncounts;
    const long *plane;         // ragged: mask f is plane sel[f] of the table and hw its own H*W (0 for a row that is none); else NULL
    const int *sel;
    int P;
};
__device__ __forceinline__ long rle_frame_hw(const RleStr &p, int f)
{
    if (!p.plane) return p.hw;
    const int q = p.sel[f];
    if (q < 0 || q >= p.P) return 0;
    const long H = p.plane[4L * q + 1], W = p.plane[4L * q + 2];
    return H >= 1 && W >= 1 && H < (1L << 31) && W < (1L << 31) && H * W < (1L << 31) ? H * W : 0;
}
__device__ __forceinline__ long rle_value(const RleStr &p, long c, int &f_out, long &i_out)
{
    int lo = 0, hi = p.F;                                  // largest f with frame_off[f] + f <= c
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p.frame_off[mid] + mid <= c) lo = mid; else hi = mid;
    }
    const int f = lo;
    const long b = p.frame_off[f], n = p.frame_off[f + 1] - b, i = c - (b + f);
    const long hw = rle_frame_hw(p, f);
    auto at = [&](long k) -> long { return k < 0 ? 0 : (k < n ? (long)p.pos[b + k] : hw); };
    long x = at(i) - at(i - 1);
    if (i > 2) x -= at(i - 2) - at(i - 3);
    f_out = f; i_out = i;
    return x;
}
__device__ __forceinline__ void rle_len_body(const RleStr &p, long c, int *__restrict__ len)
{
    int f; long i;
    long x = rle_value(p, c, f, i);
    int k = 0;
    bool more = true;
    while (more) {
        const int ch = (int)(x & 0x1f);
        x >>= 5;
        more = (ch & 0x10) ? x != -1 : x != 0;
        ++k;
    }
    len[c] = k;
}
__device__ __forceinline__ void rle_chars_body(const RleStr &p, long c, const int *__restrict__ len, const int *__restrict__ off,
                                               uint8_t *__restrict__ chars, long *__restrict__ str_off)
{
    int f; long i;
    long x = rle_value(p, c, f, i);
    uint8_t *o = chars + off[c];
    if (i == 0) str_off[f] = off[c];
    if (c == p.ncounts - 1) str_off[p.F] = (long)off[c] + len[c];
    bool more = true;
    while (more) {
        int ch = (int)(x & 0x1f);
        x >>= 5;
        more = (ch & 0x10) ? x != -1 : x != 0;
        if (more) ch |= 0x20;
        *o++ = (uint8_t)(ch + 48);
    }
}
