// Device side of the DAVIS J&F evaluator (s2d_amd/davis_eval.py; Pont-Tuset et al., "The 2017 DAVIS Challenge on Video Object
// Segmentation", and the davis2017 evaluation code, restated -- the toolkit is not part of this stack, parity with it is
// unpinned).  Integer work only: index maps -> bit planes, planes -> boundary maps, boundary maps -> disk dilations, and
// per-frame pair popcounts.  Planes are flat (pixel i -> word i/32, bit i%32: rows are not word-aligned unless W % 32 == 0), the
// layout of mask_boundary.hip; padding bits of a plane's last word are ignored on input and 0 on output.
//
//   index_planes_kernel   one workgroup per 32 flat words (1024 pixels) of one frame: every pixel ORs its bit into the LDS row of
//     its label (1..K -> row label-1, 255 -> row K, anything else nowhere), then the K + 1 rows go out as whole words: every
//     output word is stored exactly once, no zero fill, O(pixels + K words) instead of K compares per pixel.
//
//   seg2bmap_kernel   one thread per flat output word.  With M, E, S, SE the 32 bits at flat offsets i, i+1, i+W, i+W+1
//     (funnelled from the unaligned words), b = (M^E) | (M^S) | (M^SE) after the edge is replicated: in the last column E := M
//     and SE := S, in the last row S := M and SE := E.  The last-column bits of a word sit W apart from (W-1 - i%W).
//
//   disk_dilate_kernel   the disk {dx^2 + dy^2 <= R^2} is not separable as the Boundary-AP square is, but row by row it is a run:
//     D[y] = OR_dy hdil(B[y+dy], w(dy)), w(dy) = floor(sqrt(R^2 - dy^2)).  hdil distributes over OR, so with the DISTINCT
//     half-widths w_0 > w_1 > ... and h_j = the largest |dy| with w(dy) >= w_j,  D[y] = OR_j hdil(V_{h_j}[y], w_j), where
//     V_h[y] = OR_{|dy| <= h} B[y+dy] grows by two rows per step of h.  One workgroup per tile of TR rows x TW row-aligned words
//     (row y, word k = pixels 32k .. 32k+31 of that row; pixels at and beyond W, words outside the row and rows outside the
//     image are 0: that is the zero border, and it keeps a row from bleeding into its flat neighbour):
//       1. stage the tile with R halo rows above and below and two halo words (64 pixels >= R) left and right in LDS;
//       2. for j = 0 ..: V (LDS, one word per tile word incl. the halo words) |= the rows h_{j-1} < |dy| <= h_j; barrier;
//          every output word takes the 160 row bits around it from V (five words, three u64), ORs them over a window of
//          2 w_j + 1 bits by doubling (O_2a = O_a | O_a >> a up to the largest power of two p <= n, then O_p | O_p >> (n - p):
//          OR is idempotent) and ORs the centre word into its accumulator (LDS, only ever touched by its own thread); barrier;
//       3. accumulators, masked to the row, to the flat layout: plain stores when rows are word-aligned, otherwise ORed into
//          the one or two flat words they cover (out zeroed first; OR commutes, so the result is bitwise deterministic).
//     6 distinct widths at R = 8 (DAVIS 480p), 9 at 12, 39 at 64.  One workgroup per tile, no grid cap or stride loop.
//
//   frame_cross_kernel   popcount(a[p][t] & b[g][t]) for all (p, g) of one frame: the 8 x 8 register tile of the track-sum kernel
//     of ytvis_eval.hip, with the frame as the third grid dimension.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ index -> planes
constexpr int IP_T = 256;
constexpr int IP_WORDS = 32;          // flat words per workgroup

__global__ __launch_bounds__(IP_T) void index_planes_kernel(const uint8_t *__restrict__ idx, int T, long HW, long wpf, int K,
                                                             int nwb, uint32_t *__restrict__ planes, uint32_t *__restrict__ vplane)
{
    extern __shared__ unsigned int lds[];                   // [K + 1][IP_WORDS]
    const int t = blockIdx.x / nwb, wb = blockIdx.x - t * nwb;
    const long w0 = (long)wb * IP_WORDS;
    const int n = (K + 1) * IP_WORDS;
    for (int i = threadIdx.x; i < n; i += IP_T) lds[i] = 0u;
    __syncthreads();
    const uint8_t *fr = idx + (long)t * HW;
    for (int i = threadIdx.x; i < IP_WORDS * 32; i += IP_T) {
        const long p = w0 * 32 + i;
        if (p >= HW) break;                                 // i grows with the trip: nothing further is inside either
        const int l = fr[p];
        const int row = l == 255 ? K : (l >= 1 && l <= K ? l - 1 : -1);
        if (row >= 0) atomicOr(&lds[row * IP_WORDS + (i >> 5)], 1u << (i & 31));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += IP_T) {
        const int row = i / IP_WORDS;
        const long w = w0 + (i - row * IP_WORDS);
        if (w >= wpf) continue;
        if (row < K) planes[((long)row * T + t) * wpf + w] = lds[i];
        else vplane[(long)t * wpf + w] = lds[i];
    }
}

// ------------------------------------------------------------------------------------------------------------ boundary maps
// the 32 bits at flat offset p >= 0 of a plane, bits at and beyond 32 * wpf zero
__device__ __forceinline__ unsigned int flat_bits(const uint32_t *__restrict__ pl, long wpf, long p)
{
    const long wb = p >> 5;
    const int o = (int)(p & 31);
    const unsigned int g0 = wb < wpf ? pl[wb] : 0u;
    const unsigned int g1 = wb + 1 < wpf ? pl[wb + 1] : 0u;
    return (unsigned int)(((((unsigned long long)g1) << 32) | g0) >> o);
}

__global__ __launch_bounds__(256) void seg2bmap_kernel(const uint32_t *__restrict__ bits, long total, int H, int W, long wpf,
                                                       uint32_t *__restrict__ out)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const long f = g / wpf, w = g - f * wpf;
    const uint32_t *pl = bits + f * wpf;
    const long i = w * 32, HW = (long)H * W;
    const unsigned int M = pl[w];
    unsigned int E = flat_bits(pl, wpf, i + 1), S = flat_bits(pl, wpf, i + W), SE = flat_bits(pl, wpf, i + W + 1);
    unsigned int lc = 0u;                                   // bits of the word that are a last column
    for (long j = W - 1 - i % W; j < 32; j += W) lc |= 1u << j;
    const long r0 = HW - W - i;                             // first bit of the word in the last row
    const unsigned int lr = r0 <= 0 ? ~0u : (r0 >= 32 ? 0u : ~0u << r0);
    const long nv = HW - i;                                 // pixels of the plane from bit 0 of this word: >= 1
    const unsigned int valid = nv >= 32 ? ~0u : (1u << nv) - 1u;
    E = (E & ~lc) | (M & lc);
    SE = (SE & ~lc) | (S & lc);
    S = (S & ~lr) | (M & lr);
    SE = (SE & ~lr) | (E & lr);
    out[g] = ((M ^ E) | (M ^ S) | (M ^ SE)) & valid;
}

// ------------------------------------------------------------------------------------------------------------ disk dilation
constexpr int DD_T = 256;
constexpr int DD_RMAX = 64;           // two halo words hold 64 pixels either side of a word
constexpr int DD_CAP = 10240;         // LDS words per workgroup (40 KiB: four workgroups per CU)
constexpr int DD_TW = 32;             // row-aligned words per tile row at most
constexpr int DD_HALO = 2;            // halo words either side

// the distinct half-widths of the disk, widest first: run j is hdil(V_{h[j]}, w[j])
struct DiskRuns { int n; unsigned char h[DD_RMAX + 1], w[DD_RMAX + 1]; };

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
__device__ __forceinline__ u192 or192(u192 x, u192 y) { u192 o = {x.a | y.a, x.b | y.b, x.c | y.c}; return o; }

// pixels 32k .. 32k+31 of row y of a flat plane, pixels at and beyond W zero (the row mask); 0 <= k < ceil(W/32)
__device__ __forceinline__ unsigned int row_word(const uint32_t *__restrict__ pl, long wpf, int y, int W, int k)
{
    const unsigned int v = flat_bits(pl, wpf, (long)y * W + 32 * k);
    const int n = W - 32 * k;
    return n >= 32 ? v : (v & ((1u << n) - 1u));            // 1 <= n: the word starts inside the row
}

// Workgroup b: plane b / (ntx * nty), row tile (b / ntx) % nty, word tile b % ntx.  Dynamic LDS, with TWh = TW + 4:
// src [TR + 2R][TWh], V [TR][TWh], acc [TR][TW].
__global__ __launch_bounds__(DD_T) void disk_dilate_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int H, int W,
                                                           int R, long wpf, int S, int TW, int TR, int ntx, int nty, int aligned,
                                                           DiskRuns runs)
{
    extern __shared__ unsigned int lds[];
    const unsigned int nb = (unsigned int)ntx * nty;
    const unsigned int f = blockIdx.x / nb, t = blockIdx.x - f * nb;
    const int ty = t / ntx, tx = t - ty * ntx;
    const int y0 = ty * TR, k0 = tx * TW;
    const int TWh = TW + 2 * DD_HALO, LR = TR + 2 * R;
    const int NS = LR * TWh, NV = TR * TWh, NA = TR * TW;
    unsigned int *sb = lds, *vb = lds + NS, *ab = vb + NV;
    const uint32_t *pl = src + (long)f * wpf;

    for (int i = threadIdx.x; i < NS; i += DD_T) {
        const int ry = i / TWh, k = k0 - DD_HALO + (i - ry * TWh), y = y0 - R + ry;
        sb[i] = (y >= 0 && y < H && k >= 0 && k < S) ? row_word(pl, wpf, y, W, k) : 0u;
    }
    for (int i = threadIdx.x; i < NV; i += DD_T) vb[i] = 0u;
    for (int i = threadIdx.x; i < NA; i += DD_T) ab[i] = 0u;
    __syncthreads();

    int h_done = -1;                                        // V holds the rows |dy| <= h_done
    for (int j = 0; j < runs.n; ++j) {
        const int hj = runs.h[j], wj = runs.w[j];
        for (int i = threadIdx.x; i < NV; i += DD_T) {
            const int c = R * TWh + i;                      // the word's own row in src: tile row ry is src row ry + R
            unsigned int v = vb[i];
            for (int dy = h_done + 1; dy <= hj; ++dy) v |= sb[c - dy * TWh] | sb[c + dy * TWh];   // 0 <= ry + R -+ dy < LR
            vb[i] = v;
        }
        h_done = hj;
        __syncthreads();
        const int n = 2 * wj + 1;
        int p = 1;
        while (2 * p <= n) p *= 2;                          // largest power of two <= n
        for (int i = threadIdx.x; i < NA; i += DD_T) {
            const int ry = i / TW, kk = i - ry * TW;
            const unsigned int *vr = vb + ry * TWh + kk;    // words k-2 .. k+2 of the row: window bit 64 + q is pixel 32k + q
            u192 A;
            A.a = ((unsigned long long)vr[1] << 32) | vr[0];
            A.b = ((unsigned long long)vr[3] << 32) | vr[2];
            A.c = vr[4];
            unsigned int d;
            if (wj == 0) {
                d = (unsigned int)A.b;
            } else {
                for (int a = 1; a < p; a <<= 1) A = or192(A, shr192(A, a));
                if (n > p) A = or192(A, shr192(A, n - p));  // window bit q = OR of window bits q .. q + 2w
                const int pos = 64 - wj;                    // pixel 32k + q is the centre of the window that starts at 64 + q - w
                d = pos == 0 ? (unsigned int)A.a : (unsigned int)((A.a >> pos) | (A.b << (64 - pos)));    // 0 <= pos <= 63
            }
            ab[i] |= d;
        }
        __syncthreads();
    }

    uint32_t *op = dst + (long)f * wpf;
    for (int i = threadIdx.x; i < NA; i += DD_T) {
        const int ry = i / TW, k = k0 + (i - ry * TW), y = y0 + ry;
        if (y >= H || k >= S) continue;
        unsigned int v = ab[i];
        const int nn = W - 32 * k;
        if (nn < 32) v &= (1u << nn) - 1u;                  // the dilation reaches past the row's end inside its last word
        const long P = (long)y * W + 32 * k;
        if (aligned) {
            op[P >> 5] = v;
        } else if (v) {
            const int o = (int)(P & 31);
            atomicOr(&op[P >> 5], v << o);                  // set bits are pixels of the plane: the words exist
            const unsigned int hi = o ? v >> (32 - o) : 0u;
            if (hi) atomicOr(&op[(P >> 5) + 1], hi);
        }
    }
}

struct DdPlan { int TW, TR, ntx, nty, S; long wpf, nb; };

// the tile: at most DD_TW words wide (rows of more words are cut evenly), as many rows as the LDS budget holds beside the 2R
// halo rows (>= 54), cut evenly over H
bool dd_plan(int F, int H, int W, int R, DdPlan *pp)
{
    if (F < 0 || H < 1 || W < 1 || R < 1 || R > DD_RMAX || (long)H * W >= (1L << 31)) return false;
    DdPlan q;
    q.wpf = ((long)H * W + 31) / 32;
    q.S = (W + 31) / 32;
    q.ntx = cdiv(q.S, DD_TW);
    q.TW = cdiv(q.S, q.ntx);
    const int TWh = q.TW + 2 * DD_HALO;
    const int tr_max = (DD_CAP - 2 * R * TWh) / (2 * TWh + q.TW);
    q.nty = cdiv(H, tr_max);
    q.TR = cdiv(H, q.nty);
    q.nb = (long)q.ntx * q.nty;
    if ((long)F * q.nb >= (1L << 31)) return false;
    *pp = q;
    return true;
}

DiskRuns disk_runs(int R)
{
    DiskRuns r;
    r.n = 0;
    int prev = -1;
    for (int dy = 0; dy <= R; ++dy) {
        int w = 0;
        while ((w + 1) * (w + 1) + dy * dy <= R * R) ++w;   // w(dy) = floor(sqrt(R^2 - dy^2)), in integers
        if (w != prev) {                                    // a new, narrower width starts at this dy
            r.w[r.n] = (unsigned char)w;
            r.h[r.n] = (unsigned char)dy;
            ++r.n;
            prev = w;
        } else {
            r.h[r.n - 1] = (unsigned char)dy;               // the width still holds: h = the largest |dy| with w(dy) >= w
        }
    }
    return r;
}

// ------------------------------------------------------------------------------------------------------------ per-frame counts
constexpr int FC = 8;
__global__ __launch_bounds__(256) void frame_cross_kernel(const uint32_t *__restrict__ a, int P, const uint32_t *__restrict__ b, int G,
                                                          int T, long wpf, int ntg, int *__restrict__ out)
{
    __shared__ unsigned int red[4][FC * FC];
    const int ti = blockIdx.y / ntg, tj = blockIdx.y - ti * ntg, t = blockIdx.z;
    unsigned int acc[FC][FC];
#pragma unroll
    for (int p = 0; p < FC; ++p)
#pragma unroll
        for (int q = 0; q < FC; ++q) acc[p][q] = 0u;
    const long per = (wpf + gridDim.x - 1) / gridDim.x;
    const long w0 = (long)blockIdx.x * per, w1 = w0 + per < wpf ? w0 + per : wpf;
    for (long w = w0 + threadIdx.x; w < w1; w += 256) {
        unsigned int va[FC], vb[FC];
#pragma unroll
        for (int p = 0; p < FC; ++p) {
            const int i = ti * FC + p, j = tj * FC + p;
            va[p] = i < P ? a[((long)i * T + t) * wpf + w] : 0u;
            vb[p] = j < G ? b[((long)j * T + t) * wpf + w] : 0u;
        }
#pragma unroll
        for (int p = 0; p < FC; ++p)
#pragma unroll
            for (int q = 0; q < FC; ++q) acc[p][q] += __popc(va[p] & vb[q]);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < FC; ++p)
#pragma unroll
        for (int q = 0; q < FC; ++q) {
            unsigned int v = acc[p][q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) red[wv][p * FC + q] = v;
        }
    __syncthreads();
    if (threadIdx.x < FC * FC) {
        const int p = threadIdx.x / FC, q = threadIdx.x % FC;
        const int i = ti * FC + p, j = tj * FC + q;
        const unsigned int v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (i < P && j < G && v) atomicAdd(&out[((long)i * G + j) * T + t], (int)v);     // integer adds: any order, one result
    }
}

}  // namespace

extern "C" {

int s2d_index_planes_u32(const uint8_t *index, int T, int H, int W, int K, uint32_t *planes, uint32_t *void_plane, hipStream_t stream)
{
    if (!index || !void_plane || T < 0 || H < 1 || W < 1 || K < 0 || K > 254 || (K > 0 && !planes) || (long)H * W >= (1L << 31))
        return S2D_ERR_ARG;
    if (T == 0) return S2D_OK;
    const long HW = (long)H * W, wpf = (HW + 31) / 32;
    const int nwb = cdiv(wpf, IP_WORDS);
    if ((long)T * nwb >= (1L << 31)) return S2D_ERR_ARG;
    const size_t lds = sizeof(unsigned int) * (size_t)(K + 1) * IP_WORDS;
    hipLaunchKernelGGL(index_planes_kernel, dim3((unsigned)(T * nwb)), dim3(IP_T), lds, stream, index, T, HW, wpf, K, nwb, planes, void_plane);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_seg2bmap_bits_u32(const uint32_t *bits, int F, int H, int W, uint32_t *out, hipStream_t stream)
{
    if (!bits || !out || bits == out || F < 0 || H < 1 || W < 1 || (long)H * W >= (1L << 31)) return S2D_ERR_ARG;
    if (F == 0) return S2D_OK;
    const long wpf = ((long)H * W + 31) / 32, total = (long)F * wpf;
    if ((total + 255) / 256 >= (1L << 31)) return S2D_ERR_ARG;
    hipLaunchKernelGGL(seg2bmap_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, bits, total, H, W, wpf, out);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_disk_dilate_bits_u32(const uint32_t *bits, int F, int H, int W, int R, uint32_t *out, hipStream_t stream)
{
    DdPlan q;
    if (!bits || !out || bits == out || !dd_plan(F, H, W, R, &q)) return S2D_ERR_ARG;
    if (F == 0) return S2D_OK;
    const int aligned = (W & 31) == 0;
    if (!aligned && s2d_zero_async(out, sizeof(uint32_t) * (size_t)F * q.wpf, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    const int TWh = q.TW + 2 * DD_HALO;
    const size_t lds = sizeof(unsigned int) * ((size_t)(q.TR + 2 * R) * TWh + (size_t)q.TR * TWh + (size_t)q.TR * q.TW);
    hipLaunchKernelGGL(disk_dilate_kernel, dim3((unsigned)(F * q.nb)), dim3(DD_T), lds, stream, bits, out, H, W, R, q.wpf, q.S, q.TW,
                       q.TR, q.ntx, q.nty, aligned, disk_runs(R));
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
    const int ntp = (P + FC - 1) / FC, ntg = (G + FC - 1) / FC;
    const long ntiles = (long)ntp * ntg;
    if (ntiles >= 65536) return S2D_ERR_ARG;
    int chunks = cdiv(words_per_frame, 256 * 16);       // >= 16 words per thread
    const int want = cdiv(2048, ntiles * T);            // enough workgroups to fill 256 CUs
    if (chunks > want) chunks = want;
    if (chunks < 1) chunks = 1;
    hipLaunchKernelGGL(frame_cross_kernel, dim3(chunks, (unsigned)ntiles, T), dim3(256), 0, stream, a, P, b, G, T, words_per_frame, ntg, out);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
