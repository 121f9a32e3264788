// Device side of the DAVIS J&F evaluator (s2d_amd/davis_eval.py; Pont-Tuset et al., "The 2017 DAVIS Challenge on Video Object
// Segmentation", and the davis2017 evaluation code, restated -- the toolkit is not part of this stack, parity with it is
// unpinned).  Integer work only: index maps -> bit planes, planes -> boundary maps, boundary maps -> disk dilations; the per-frame
// pair popcounts are s2d_mask_frame_cross_counts_i32 of mask_counts.hip.  Planes are flat: the layout and the row helpers shared
// with the erosion of mask_boundary.hip are in bitplane.h.
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
//     (the zero border of bitplane.h):
//       1. stage the tile with R halo rows above and below and two halo words (64 pixels >= R) left and right in LDS;
//       2. for j = 0 ..: V (LDS, one word per tile word incl. the halo words) |= the rows h_{j-1} < |dy| <= h_j; barrier;
//          every output word takes the 160 row bits around it from V (five words, three u64), ORs them over a window of
//          2 w_j + 1 bits by doubling (window192) and ORs the centre word into its accumulator (LDS, only ever touched by its
//          own thread); barrier;
//       3. accumulators, masked to the row, to the flat layout (store_row_word; out zeroed first when rows are not
//          word-aligned).
//     6 distinct widths at R = 8 (DAVIS 480p), 9 at 12, 39 at 64.  One workgroup per tile, no grid cap or stride loop.
#include "bitplane.h"

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
        for (int i = threadIdx.x; i < NA; i += DD_T) {
            const int ry = i / TW, kk = i - ry * TW;
            const unsigned int *vr = vb + ry * TWh + kk;    // words k-2 .. k+2 of the row: window bit 64 + q is pixel 32k + q
            u192 A;
            A.a = ((unsigned long long)vr[1] << 32) | vr[0];
            A.b = ((unsigned long long)vr[3] << 32) | vr[2];
            A.c = vr[4];
            ab[i] |= wj == 0 ? (unsigned int)A.b : centre_word(window192<BitOr>(A, 2 * wj + 1), wj);
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
        store_row_word(op, y, W, k, v, aligned);
    }
}

// as many tile rows as the LDS budget holds beside the 2R halo rows (>= 54)
bool dd_plan(int F, int H, int W, int R, TilePlan *pp)
{
    if (R < 1 || R > DD_RMAX) return false;
    const auto tr_max = [R](int TW) { const int TWh = TW + 2 * DD_HALO; return (DD_CAP - 2 * R * TWh) / (2 * TWh + TW); };
    return tile_plan(F, H, W, DD_TW, tr_max, pp);
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
    TilePlan q;
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

}  // extern "C"
