// Device and host pieces shared by the kernels that work on packed bit planes: mask_counts.hip, coco_eval.hip and
// selftrain_video.hip (pair popcounts), mask_counts.hip and rle_ragged.hip (plane areas), mask_boundary.hip and davis_eval.hip
// (morphology on rows that are not word-aligned), rle_ragged.hip and plane_components.hip (the ragged plane table).
//
// THE PLANE LAYOUT.  A plane of H x W pixels is FLAT: pixel i = y * W + x -> word i / 32, bit i % 32, ceil(H * W / 32) words (what
// s2d_pack_mask_bits_u8 and s2d_rle_decode_bits write), so rows are not word-aligned unless W % 32 == 0.  The padding bits of a
// plane's last word are ignored on input and 0 on output.  The morphology kernels work on ROW-ALIGNED words (row y, word k = pixels
// 32k .. 32k+31 of that row; S = ceil(W / 32) words per row): pixels at and beyond W, words outside the row and rows outside the
// image are 0.  That zero border keeps a row from bleeding into its flat neighbour.
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------------------ pair counts
// An N x N register tile of popcount(va[p] & vb[q]) sums for a workgroup of 256 threads: every word of the 2N planes is loaded
// once per tile.  reduce() needs red[4][>= N * N] in LDS; it ends in a barrier, so a caller may hand further values over through
// the columns beyond N * N by writing them before the call.
template <int N> struct PopcTile {
    unsigned int acc[N][N];

    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int p = 0; p < N; ++p)
#pragma unroll
            for (int q = 0; q < N; ++q) acc[p][q] = 0u;
    }
    __device__ __forceinline__ void add(const unsigned int (&va)[N], const unsigned int (&vb)[N])
    {
#pragma unroll
        for (int p = 0; p < N; ++p)
#pragma unroll
            for (int q = 0; q < N; ++q) acc[p][q] += __popc(va[p] & vb[q]);
    }
    // thread x < N * N gets the workgroup's sum of entry (x / N, x % N), every other thread 0
    template <int LD> __device__ __forceinline__ unsigned long long reduce(unsigned int (&red)[4][LD])
    {
        static_assert(LD >= N * N, "one LDS column per tile entry");
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
        for (int p = 0; p < N; ++p)
#pragma unroll
            for (int q = 0; q < N; ++q) {
                unsigned int v = acc[p][q];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0) red[wv][p * N + q] = v;
            }
        __syncthreads();
        const int x = threadIdx.x;
        return x < N * N ? (unsigned long long)red[0][x] + red[1][x] + red[2][x] + red[3][x] : 0ull;
    }
};

// area[0] = the set bits of the wpf words of plane pl (mask_util.area), for the fixed-size and the ragged entry point alike.  All
// 256 threads of the workgroup call this (it holds a barrier).
__device__ __forceinline__ void plane_popcount(const uint32_t *__restrict__ pl, long wpf, unsigned int *__restrict__ area)
{
    __shared__ unsigned int red[4];
    unsigned int s = 0;
    for (long w = threadIdx.x; w < wpf; w += 256) s += __popc(pl[w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) area[0] = red[0] + red[1] + red[2] + red[3];
}

// Chunks of the word range for a launch of `tiles` tile workgroups per chunk that add their partial sums with atomics.
static inline int popc_chunks(long words, long tiles)
{
    int chunks = cdiv(words, 256 * 16);                 // >= 16 words per thread
    const int want = cdiv(2048, tiles);                 // enough workgroups to fill 256 CUs
    if (chunks > want) chunks = want;
    return chunks < 1 ? 1 : chunks;
}

// ------------------------------------------------------------------------------------------------------------ rows of a flat plane
// the 32 bits at flat offset p >= 0 of a plane, bits at and beyond 32 * wpf zero
__device__ __forceinline__ unsigned int flat_bits(const uint32_t *__restrict__ pl, long wpf, long p)
{
    const long wb = p >> 5;
    const int o = (int)(p & 31);
    const unsigned int g0 = wb < wpf ? pl[wb] : 0u;
    const unsigned int g1 = wb + 1 < wpf ? pl[wb + 1] : 0u;
    return (unsigned int)(((((unsigned long long)g1) << 32) | g0) >> o);
}

// row-aligned word k of row y, pixels at and beyond W zero (the row mask); 0 <= y < H, 0 <= k < S
__device__ __forceinline__ unsigned int row_word(const uint32_t *__restrict__ pl, long wpf, int y, int W, int k)
{
    const unsigned int v = flat_bits(pl, wpf, (long)y * W + 32 * k);
    const int n = W - 32 * k;
    return n >= 32 ? v : (v & ((1u << n) - 1u));            // 1 <= n: the word starts inside the row
}

// Row-aligned word k of row y, bits at and beyond W already 0, to plane `op`: a plain store when rows are word-aligned, otherwise
// ORed into the one or two flat words it covers (the plane zeroed first; only pixel bits are ever set, so padding bits stay 0).
// OR commutes: the result is bitwise deterministic.
__device__ __forceinline__ void store_row_word(uint32_t *__restrict__ op, int y, int W, int k, unsigned int v, int aligned)
{
    const long P = (long)y * W + 32 * k;
    if (aligned) {
        op[P >> 5] = v;
    } else if (v) {
        const int o = (int)(P & 31);
        atomicOr(&op[P >> 5], v << o);                      // set bits are pixels of the plane: the words exist
        const unsigned int hi = o ? v >> (32 - o) : 0u;
        if (hi) atomicOr(&op[(P >> 5) + 1], hi);
    }
}

// ------------------------------------------------------------------------------------------------------------ ragged plane table
// Row p of the table plane int64 [P][4] = {word0, H, W, 0} of a chunk of planes of different sizes over one flat buffer of
// total_words words (rle_ragged.hip, plane_components.hip).  ok = the buffer holds the plane: a row with H or W < 1, H*W >= 2^31 or
// words outside [0, total_words) is skipped by every kernel that reads the table.
struct PlaneRow {
    long word0, wpp;
    int H, W;
    bool ok;
};

__device__ __forceinline__ PlaneRow plane_row(const long *__restrict__ plane, int p, long total_words)
{
    const long *r = plane + 4L * p;
    PlaneRow q;
    const long H = r[1], W = r[2];
    q.word0 = r[0];
    q.ok = H >= 1 && W >= 1 && H < (1L << 31) && W < (1L << 31) && H * W < (1L << 31);
    q.H = (int)H; q.W = (int)W;
    q.wpp = q.ok ? (H * W + 31) / 32 : 0;
    q.ok = q.ok && q.word0 >= 0 && q.word0 <= total_words - q.wpp;
    return q;
}

// ------------------------------------------------------------------------------------------------------------ 192-bit row windows
struct u192 { unsigned long long a, b, c; };   // bit i of the window: a = 0..63, b = 64..127, c = 128..191

// bits i + s -> i, zeros in at the top; 1 <= s <= 64
__device__ __forceinline__ u192 shr192(u192 v, int s)
{
    u192 o;
    if (s == 64) { o.a = v.b; o.b = v.c; o.c = 0ull; return o; }
    o.a = (v.a >> s) | (v.b << (64 - s));
    o.b = (v.b >> s) | (v.c << (64 - s));
    o.c = v.c >> s;
    return o;
}

struct BitAnd { static __device__ __forceinline__ u192 f(u192 x, u192 y) { u192 o = {x.a & y.a, x.b & y.b, x.c & y.c}; return o; } };
struct BitOr { static __device__ __forceinline__ u192 f(u192 x, u192 y) { u192 o = {x.a | y.a, x.b | y.b, x.c | y.c}; return o; } };

// the largest power of two <= n; n >= 1.  Straight-line, so that a caller's loop over words does not repeat a search for it
__device__ __forceinline__ int pow2_floor(int n) { return 1 << (31 - __builtin_clz((unsigned int)n)); }

// bit q of the result = Op over bits q .. q + n - 1 of A, by doubling: A_1 = A, A_2a = Op(A_a, A_a >> a) up to p = pow2_floor(n),
// then Op(A_p, A_p >> (n - p)) -- AND and OR are idempotent, so two overlapping windows of p make one of n.  1 <= n <= 129
template <class Op> __device__ __forceinline__ u192 window192(u192 A, int n)
{
    const int p = pow2_floor(n);
    for (int a = 1; a < p; a <<= 1) A = Op::f(A, shr192(A, a));
    if (n > p) A = Op::f(A, shr192(A, n - p));
    return A;
}

// With window bit 64 + q = pixel 32k + q and A = window192(., 2r + 1): word k of the row with every pixel the Op of its r
// neighbours either side (pixel 32k + q is the centre of the window that starts at bit 64 + q - r); 1 <= r <= 64
__device__ __forceinline__ unsigned int centre_word(u192 A, int r)
{
    const int pos = 64 - r;
    return pos == 0 ? (unsigned int)A.a : (unsigned int)((A.a >> pos) | (A.b << (64 - pos)));
}

// ------------------------------------------------------------------------------------------------------------ host: tile plan
// One workgroup per tile of TR rows x TW row-aligned words of one plane: at most tw_max words wide (rows of more words are cut
// evenly), at most tr_max(TW) >= 1 rows (what the kernel's LDS budget holds at that width), cut evenly over H.  nb = tiles per
// plane; false for a negative F, an empty image, H * W >= 2^31 or F * nb >= 2^31.
struct TilePlan { int TW, TR, ntx, nty, S; long wpf, nb; };

template <class RowsFn> static inline bool tile_plan(int F, int H, int W, int tw_max, RowsFn tr_max, TilePlan *pp)
{
    if (F < 0 || H < 1 || W < 1 || (long)H * W >= (1L << 31)) return false;
    TilePlan q;
    q.wpf = ((long)H * W + 31) / 32;
    q.S = (W + 31) / 32;
    q.ntx = cdiv(q.S, tw_max);
    q.TW = cdiv(q.S, q.ntx);
    q.nty = cdiv(H, tr_max(q.TW));
    q.TR = cdiv(H, q.nty);
    q.nb = (long)q.ntx * q.nty;
    if ((long)F * q.nb >= (1L << 31)) return false;
    *pp = q;
    return true;
}
