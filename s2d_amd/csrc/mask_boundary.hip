// Mask -> boundary band on bit planes, the per-pixel work of Boundary AP (s2d_amd/ytvis_eval.py; Cheng et al., "Boundary IoU",
// CVPR 2021, and the published mask_to_boundary routine, restated): Bd = M & ~E, where E is M eroded d times by a 3 x 3 square
// with everything outside the image counting as 0.  d such erosions are one erosion by a (2d+1) x (2d+1) square with a zero
// border, and that square is separable:  E[y][x] = AND_{|dy| <= d} Eh[y + dy][x],  Eh[y][x] = AND_{|dx| <= d} M[y][x + dx].
//
// Planes are flat and the kernel works on row-aligned words: the layout and the helpers shared with the disk dilation of
// davis_eval.hip are in bitplane.h.
//
//   erode_tile_kernel   one workgroup per tile of TR rows x TW row-aligned words of one plane, r <= 64:
//     1. horizontal, in registers: for every word of the tile and of its r halo rows above and below, the 192 row bits
//        around it (pixels 32k-64 .. 32k+127, seven flat words funnelled into three u64, pixels outside the row masked to
//        0: that is the zero border, and it drops whatever sits in a plane's padding bits) are ANDed over a window of
//        n = 2r+1 bits by doubling (window192).  The word goes to LDS; halo rows outside the image are 0.
//     2. vertical, in LDS: the same doubling over rows as plain word ANDs, ping-pong between two buffers (flat indices,
//        adjacent lanes on adjacent words: no bank conflicts), one barrier per step.
//     3. M & ~E (or E itself for an intermediate pass), written back to the flat layout (store_row_word; out zeroed first
//        when rows are not word-aligned).
//
// d > 64 (frames beyond 4K at the default ratio) chains erosions: squares add up, erode(r1 + r2) = erode(r2) o erode(r1),
// also with the zero border (an eroded plane is zero outside the image like its input).  The intermediates alternate between
// the caller's workspace and `out`, the last one in the workspace.  A window that does not fit the image (2d+1 > min(H, W))
// leaves E empty whatever d is, so d is first clamped to (min(H, W) + 1) / 2: no frame of the evaluator needs a second pass.
//
//   erode_ragged_kernel  the same tile body for a chunk of images of different sizes in ONE launch (the COCO image evaluator,
//     s2d_amd/coco_eval.py): every image has its own H, W, d and tile shape, listed in a plan table that the host derives and
//     re-checks before the launch; one pass only (clamped d <= 64), the last one: out = M & ~E.
#include "bitplane.h"

#include <vector>

namespace {

constexpr int BD_T = 256;
constexpr int BD_RMAX = 64;         // one pass: the 192-bit window holds 64 pixels either side of a word
constexpr int BD_CAP = 8192;        // words per LDS buffer (two buffers: 64 KiB, two workgroups per CU)
constexpr int BD_TW = 32;           // row-aligned words per tile row at most

// bits [lo, hi) of a 64-bit chunk whose first bit is window bit `base`
__device__ __forceinline__ unsigned long long chunk_mask(int lo, int hi, int base)
{
    int a = lo - base, b = hi - base;
    a = a < 0 ? 0 : a;
    b = b > 64 ? 64 : b;
    if (b <= a) return 0ull;
    const unsigned long long upto = b == 64 ? ~0ull : (1ull << b) - 1ull;
    return upto & ~((1ull << a) - 1ull);                 // a < b <= 64: the shift is defined
}

// pixels 32k-64 .. 32k+127 of row y of a flat plane, pixels outside [0, W) zero
__device__ __forceinline__ u192 row_window(const uint32_t *__restrict__ pl, long wpf, int y, int W, int k)
{
    const int x0 = 32 * k - 64;
    const long P = (long)y * W + x0;                        // flat bit of window bit 0: >= -64
    const long wb = P >> 5;                                 // floor, also below zero
    const int o = (int)(P & 31);
    unsigned int g[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) g[j] = (wb + j >= 0 && wb + j < wpf) ? pl[wb + j] : 0u;
    unsigned int v[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = (unsigned int)(((((unsigned long long)g[j + 1]) << 32) | g[j]) >> o);
    const int lo = x0 < 0 ? -x0 : 0;
    const int hi = W - x0 < 192 ? W - x0 : 192;
    u192 w;
    w.a = ((((unsigned long long)v[1]) << 32) | v[0]) & chunk_mask(lo, hi, 0);
    w.b = ((((unsigned long long)v[3]) << 32) | v[2]) & chunk_mask(lo, hi, 64);
    w.c = ((((unsigned long long)v[5]) << 32) | v[4]) & chunk_mask(lo, hi, 128);
    return w;
}

// One tile (row tile ty, word tile tx) of ONE plane: pl the plane to erode by r, ml the plane M for the last pass (op = M & ~E)
// or null (op = E), op the output plane; lds: 2 * TW * (TR + 2r) words.  The body both kernels below share.
__device__ __forceinline__ void erode_tile(const uint32_t *__restrict__ pl, const uint32_t *__restrict__ ml, uint32_t *__restrict__ op,
                                           int H, int W, int r, long wpf, int S, int TW, int TR, int ty, int tx, int aligned,
                                           unsigned int *lds)
{
    const int y0 = ty * TR, k0 = tx * TW;
    const int LR = TR + 2 * r, N = TW * LR;
    const int n = 2 * r + 1, p = pow2_floor(n);
    unsigned int *cur = lds, *nxt = lds + N;

    for (int i = threadIdx.x; i < N; i += BD_T) {
        const int ry = i / TW, k = k0 + (i - ry * TW), y = y0 - r + ry;
        unsigned int e = 0u;
        if (y >= 0 && y < H && k < S) e = centre_word(window192<BitAnd>(row_window(pl, wpf, y, W, k), n), r);
        cur[i] = e;
    }
    __syncthreads();
    for (int a = 1; a < p; a <<= 1) {                       // rows: cur[row q] = AND of Eh rows q .. q + a - 1
        const int sh = a * TW;
        for (int i = threadIdx.x; i < N; i += BD_T) nxt[i] = i + sh < N ? (cur[i] & cur[i + sh]) : 0u;
        __syncthreads();
        unsigned int *s = cur; cur = nxt; nxt = s;
    }
    const int sh = (n - p) * TW;                            // n is odd and >= 3: n > p
    for (int i = threadIdx.x; i < TR * TW; i += BD_T) {      // output row y0 + ry: window rows ry .. ry + 2r of the tile
        const int ry = i / TW, k = k0 + (i - ry * TW), y = y0 + ry;
        if (y >= H || k >= S) continue;
        unsigned int v = cur[i] & cur[i + sh];              // i + sh <= (TR - 1 + 2r) * TW + TW - 1 < N
        // y < H and k < S: the word starts inside the plane.  Said aloud, row_word's first load needs no test of its own, and with
        // that load in flight the second one does not wait for it (2.5 % of the kernel at 720p)
        __builtin_assume(((long)y * W + 32 * k) >> 5 < wpf);
        if (ml) v = row_word(ml, wpf, y, W, k) & ~v;
        store_row_word(op, y, W, k, v, aligned);
    }
}

// src: planes to erode by r; orig: planes M for the last pass (dst = M & ~E) or null (dst = E).  Workgroup b: plane
// b / (ntx * nty), row tile (b / ntx) % nty, word tile b % ntx.  Dynamic LDS: 2 * TW * (TR + 2r) words.
__global__ __launch_bounds__(BD_T) void erode_tile_kernel(const uint32_t *__restrict__ src, const uint32_t *__restrict__ orig,
                                                          uint32_t *__restrict__ dst, int H, int W, int r, long wpf, int S,
                                                          int TW, int TR, int ntx, int nty, int aligned)
{
    extern __shared__ unsigned int lds[];
    const unsigned int nb = (unsigned int)ntx * nty;
    const unsigned int f = blockIdx.x / nb, t = blockIdx.x - f * nb;
    const int ty = t / ntx, tx = t - ty * ntx;
    erode_tile(src + (long)f * wpf, orig ? orig + (long)f * wpf : nullptr, dst + (long)f * wpf, H, W, r, wpf, S, TW, TR, ty, tx,
               aligned, lds);
}

constexpr int RP_COLS = 12;         // plan row: word0 F H W d wpp S TW TR ntx nty wg0 (include/s2d_hip.h)

// The band of every plane of a chunk of N images of different sizes, one pass (every d <= 64).  Workgroup b belongs to the
// last image n with wg0[n] <= b (binary search over the plan rows; an image without planes shares its wg0 with its successor
// and is never found), and inside it to plane (b - wg0) / (ntx * nty), row tile ((b - wg0) / ntx) % nty, word tile
// (b - wg0) % ntx.  Everything a workgroup reads from the plan is uniform over it; the tile body is erode_tile with the image's
// own H, W, d, TW, TR.
// Occupancy: dynamic LDS is one figure per launch, the largest 2 * TW * (TR + 2d) words of any image, so one large image in
// the chunk sets the residency of every workgroup: at the 64 KiB of a tile that fills the cap, two workgroups (8 waves) per CU
// of 160 KiB, also for the workgroups of a 32 x 32 image that use a few hundred bytes and, launched alone, would be resident
// up to the wave limit.  A small image's workgroup is short (one or two trips per loop), so what it loses is overlap of its
// load latency, not capacity; a chunk of small images only gets a small figure.
__global__ __launch_bounds__(BD_T) void erode_ragged_kernel(const uint32_t *__restrict__ bits, uint32_t *__restrict__ out,
                                                            const long *__restrict__ plan, int N)
{
    extern __shared__ unsigned int lds[];
    const long b = blockIdx.x;
    int lo = 0, hi = N;                                     // answer in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (plan[(long)RP_COLS * mid + 11] <= b) lo = mid; else hi = mid;
    }
    const long *q = plan + (long)RP_COLS * lo;
    const int H = (int)q[2], W = (int)q[3], r = (int)q[4], S = (int)q[6], TW = (int)q[7], TR = (int)q[8];
    const int ntx = (int)q[9], nty = (int)q[10];
    const long wpp = q[5];
    const unsigned int local = (unsigned int)(b - q[11]), nb = (unsigned int)ntx * nty;
    const unsigned int f = local / nb, t = local - f * nb;
    if ((long)f >= q[1]) return;                            // not reached with a plan the host call accepted
    const int ty = t / ntx, tx = t - ty * ntx;
    const long at = q[0] + (long)f * wpp;
    erode_tile(bits + at, bits + at, out + at, H, W, r, wpp, S, TW, TR, ty, tx, (W & 31) == 0, lds);
}

struct BdPlan : TilePlan { int d; };

// d clamped to where E is empty anyway; as many rows as one LDS buffer holds beside the 2r halo rows of the widest pass (>= 128)
bool bd_plan(int F, int H, int W, int d, BdPlan *pp)
{
    if (d < 1) return false;
    const int m = H < W ? H : W;                            // an empty image is refused below, before d is used
    pp->d = d < (m + 1) / 2 ? d : (m + 1) / 2;
    const int r = pp->d < BD_RMAX ? pp->d : BD_RMAX;
    return tile_plan(F, H, W, BD_TW, [r](int TW) { return BD_CAP / TW - 2 * r; }, pp);
}

// spec [N][5] = {word0, F, H, W, d} -> plan rows, total workgroups, launch LDS bytes; false (nothing written) for a table the
// ragged call refuses.  rows may be null (validation only).
bool ragged_plan(const long *spec, int N, long total_words, long *rows, long *n_wg, long *lds_bytes)
{
    if (N < 0 || total_words < 0 || (N > 0 && !spec)) return false;
    for (int pass = 0; pass < 2; ++pass) {                  // pass 0 checks everything, pass 1 writes
        long end = 0, wg = 0, lds = 0;
        for (int n = 0; n < N; ++n) {
            const long *s = spec + 5L * n;
            const long word0 = s[0], F = s[1], H = s[2], W = s[3], d = s[4];
            if (F < 0 || F >= (1L << 31) || H < 1 || W < 1 || H >= (1L << 31) || W >= (1L << 31) || d < 1) return false;
            BdPlan q;
            if (!bd_plan((int)F, (int)H, (int)W, (int)(d < (1L << 30) ? d : (1L << 30)), &q) || q.d > BD_RMAX) return false;
            if (word0 < end || word0 > total_words || F > (total_words - word0) / q.wpf) return false;   // ascending, disjoint, inside
            end = word0 + F * q.wpf;
            const long bytes = 2L * q.TW * (q.TR + 2 * q.d) * (long)sizeof(unsigned int);
            if (bytes > 65536) return false;
            if (F && bytes > lds) lds = bytes;
            if (pass && rows) {
                const long row[RP_COLS] = {word0, F, H, W, q.d, q.wpf, q.S, q.TW, q.TR, q.ntx, q.nty, wg};
                for (int c = 0; c < RP_COLS; ++c) rows[(long)RP_COLS * n + c] = row[c];
            }
            wg += F * q.nb;
            if (wg >= (1L << 31)) return false;
        }
        if (pass) { *n_wg = wg; *lds_bytes = lds; }
    }
    return true;
}

}  // namespace

extern "C" {

int s2d_mask_boundary_ragged_plan(const long *spec, int N, long total_words, long *plan, long *n_workgroups, long *lds_bytes)
{
    if (!n_workgroups || !lds_bytes || (N > 0 && !plan)) return S2D_ERR_ARG;
    return ragged_plan(spec, N, total_words, plan, n_workgroups, lds_bytes) ? S2D_OK : S2D_ERR_ARG;
}

int s2d_mask_boundary_ragged_u32(const uint32_t *bits, long total_words, const long *plan_host, const long *plan_dev, int N,
                                 uint32_t *out, hipStream_t stream)
{
    if (N < 0 || total_words < 0 || !bits || !out || bits == out || !plan_host || !plan_dev) return S2D_ERR_ARG;
    std::vector<long> spec(5 * (size_t)N), rows((size_t)RP_COLS * N);
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < 5; ++c) spec[5 * (size_t)n + c] = plan_host[(size_t)RP_COLS * n + c];
    long n_wg = 0, lds = 0;
    if (!ragged_plan(spec.data(), N, total_words, rows.data(), &n_wg, &lds)) return S2D_ERR_ARG;
    for (size_t i = 0; i < rows.size(); ++i)
        if (rows[i] != plan_host[i]) return S2D_ERR_ARG;     // a table that is not what the plan call wrote: nothing is launched
    if (n_wg == 0) return S2D_OK;
    bool unaligned = false;
    for (int n = 0; n < N; ++n) unaligned |= rows[(size_t)RP_COLS * n + 1] > 0 && (rows[(size_t)RP_COLS * n + 3] & 31) != 0;
    if (unaligned && s2d_zero_async(out, sizeof(uint32_t) * (size_t)total_words, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    hipLaunchKernelGGL(erode_ragged_kernel, dim3((unsigned)n_wg), dim3(BD_T), (size_t)lds, stream, bits, out, plan_dev, N);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

long s2d_mask_boundary_workspace_words(int F, int H, int W, int d)
{
    BdPlan q;
    if (!bd_plan(F, H, W, d, &q)) return -1;
    return q.d <= BD_RMAX ? 0 : (long)F * q.wpf;
}

int s2d_mask_boundary_bits_u32(const uint32_t *bits, int F, int H, int W, int d, uint32_t *workspace, long workspace_words,
                               uint32_t *out, hipStream_t stream)
{
    BdPlan q;
    if (!bits || !out || bits == out || !bd_plan(F, H, W, d, &q)) return S2D_ERR_ARG;
    const long need = q.d <= BD_RMAX ? 0 : (long)F * q.wpf;
    if (need && (!workspace || workspace_words < need || workspace == out || workspace == bits)) return S2D_ERR_ARG;
    if (F == 0) return S2D_OK;
    const int aligned = (W & 31) == 0;
    const int passes = cdiv(q.d, BD_RMAX);
    const uint32_t *src = bits;
    int left = q.d;
    for (int j = 1; j <= passes; ++j) {
        const int r = left < BD_RMAX ? left : BD_RMAX;
        left -= r;
        const bool last = j == passes;
        uint32_t *dst = last || ((passes - 1 - j) & 1) ? out : workspace;     // the last intermediate lies in the workspace
        if (!aligned && s2d_zero_async(dst, sizeof(uint32_t) * (size_t)F * q.wpf, stream) != S2D_OK) return S2D_ERR_LAUNCH;
        const size_t lds = sizeof(unsigned int) * 2 * (size_t)q.TW * (q.TR + 2 * r);
        hipLaunchKernelGGL(erode_tile_kernel, dim3((unsigned)(F * q.nb)), dim3(BD_T), lds, stream, src, last ? bits : nullptr, dst, H, W,
                           r, q.wpf, q.S, q.TW, q.TR, q.ntx, q.nty, aligned);
        S2D_CHECK_LAUNCH();
        src = dst;
    }
    return S2D_OK;
}

}  // extern "C"
