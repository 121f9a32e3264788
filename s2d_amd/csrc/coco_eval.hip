// COCO image evaluation (s2d_amd/coco_eval.py; COCOeval.computeIoU / evaluateImg restated, pycocotools parity unpinned): the
// per-pair and per-problem work of a CHUNK of images of different sizes, each kernel launched once per chunk whatever the chunk
// holds.  The ragged layout (flat buffers + per-image offset tables) is documented in include/s2d_hip.h.
//
//   ragged_mask_iou_kernel  one workgroup per 8 x 8 tile of (detection, ground truth) pairs of one image (the host lists the
//                           tiles): every word of the 16 planes is loaded once per tile (PopcTile of bitplane.h, which also
//                           states the plane layout), the tile's 64 intersection counts and 16 plane areas are exact integers,
//                           and the IoU is one float64 division of them in the epilogue.  A tile is owned by one workgroup: no
//                           atomics, no zero fill, bitwise deterministic.
//   ragged_box_iou_kernel   one thread per pair, maskApi.c bbIou's operation order in float64 (the build has -ffp-contract=off).
//   coco_match_kernel       COCOeval.evaluateImg's greedy loop.  One workgroup per group (an image, or an image and a category):
//                           lane (a, t) runs area range a at threshold t -- the thresholds and the ranges are independent, the
//                           detection loop is sequential by definition.
#include "bitplane.h"

namespace {

constexpr int CT = 8;                       // pair tile edge
constexpr int IMG_COLS = 9;                 // columns of an image-table row (s2d_hip.h)
constexpr int GRP_COLS = 8;                 // columns of a group-table row

__global__ __launch_bounds__(256) void ragged_mask_iou_kernel(const uint32_t *__restrict__ bits, const long *__restrict__ img,
                                                              const int *__restrict__ tiles, const uint8_t *__restrict__ crowd,
                                                              long long *__restrict__ inter, int *__restrict__ area_d,
                                                              int *__restrict__ area_g, double *__restrict__ iou)
{
    __shared__ unsigned int red[4][CT * CT + 2 * CT];
    const int *tl = tiles + 3L * blockIdx.x;
    const long *im = img + (long)IMG_COLS * tl[0];
    const int ti = tl[1], tj = tl[2];
    const long dt_word = im[0], gt_word = im[1], wpp = im[2], hw = im[3];
    const int D = (int)im[4], G = (int)im[5];
    const long dt0 = im[6], gt0 = im[7], pair0 = im[8];
    const uint32_t tail = (hw & 31) ? ((1u << (hw & 31)) - 1u) : 0xffffffffu;       // bits past H*W in the last word do not count

    PopcTile<CT> tile;
    tile.zero();
    unsigned int pa[CT], pb[CT];
#pragma unroll
    for (int p = 0; p < CT; ++p) pa[p] = pb[p] = 0u;
    for (long w = threadIdx.x; w < wpp; w += 256) {
        const uint32_t keep = w == wpp - 1 ? tail : 0xffffffffu;
        unsigned int va[CT], vb[CT];
#pragma unroll
        for (int p = 0; p < CT; ++p) {
            const int i = ti * CT + p, j = tj * CT + p;
            va[p] = i < D ? bits[dt_word + (long)i * wpp + w] & keep : 0u;
            vb[p] = j < G ? bits[gt_word + (long)j * wpp + w] & keep : 0u;
            pa[p] += __popc(va[p]);
            pb[p] += __popc(vb[p]);
        }
        tile.add(va, vb);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < CT; ++p) {                                            // the areas ride in the columns behind the tile's
        unsigned int a = pa[p], b = pb[p];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o, 64);
            b += __shfl_xor(b, o, 64);
        }
        if (lane == 0) {
            red[wv][CT * CT + p] = a;
            red[wv][CT * CT + CT + p] = b;
        }
    }
    const long long n = (long long)tile.reduce(red);                          // ends in the barrier that covers the areas too
    const int x = threadIdx.x;
    if (x < CT * CT) {
        const int p = x / CT, q = x % CT;
        const int i = ti * CT + p, j = tj * CT + q;
        if (i < D && j < G) {
            const int ap = CT * CT + p, aq = CT * CT + CT + q;
            const long long ad = (long long)red[0][ap] + red[1][ap] + red[2][ap] + red[3][ap];
            const long long ag = (long long)red[0][aq] + red[1][aq] + red[2][aq] + red[3][aq];
            const long long u = crowd[gt0 + j] ? ad : ad + ag - n;
            inter[pair0 + (long)i * G + j] = n;
            iou[pair0 + (long)i * G + j] = u > 0 ? (double)n / (double)u : 0.0;
        }
    } else if (x < CT * CT + CT) {                                            // the areas: once per image row / column of tiles
        const int p = x - CT * CT, i = ti * CT + p;
        if (tj == 0 && i < D) area_d[dt0 + i] = (int)(red[0][x] + red[1][x] + red[2][x] + red[3][x]);
    } else if (x < CT * CT + 2 * CT) {
        const int q = x - CT * CT - CT, j = tj * CT + q;
        if (ti == 0 && j < G) area_g[gt0 + j] = (int)(red[0][x] + red[1][x] + red[2][x] + red[3][x]);
    }
}

// pair index -> its image: the last i with pair_off[i] <= idx (pair_off [N+1] ascending, empty images repeat a value)
__device__ __forceinline__ int image_of_pair(const long *__restrict__ pair_off, int N, long idx)
{
    int lo = 0, hi = N;                                                       // answer in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pair_off[mid] <= idx) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void ragged_box_iou_kernel(const double *__restrict__ dt, const double *__restrict__ gt,
                                                             const uint8_t *__restrict__ crowd, const long *__restrict__ img, int N,
                                                             const long *__restrict__ pair_off, long P, double *__restrict__ iou)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= P) return;
    const long *im = img + (long)IMG_COLS * image_of_pair(pair_off, N, idx);
    const int G = (int)im[5];
    const long local = idx - im[8];
    const long d = im[6] + local / G, g = im[7] + local % G;
    const double *a = dt + 4 * d, *b = gt + 4 * g;
    const double da = a[2] * a[3], ga = b[2] * b[3];
    double o = 0.0;
    const double w = fmin(a[2] + a[0], b[2] + b[0]) - fmax(a[0], b[0]);
    if (w > 0.0) {
        const double h = fmin(a[3] + a[1], b[3] + b[1]) - fmax(a[1], b[1]);
        if (h > 0.0) {
            const double i = w * h;
            const double u = crowd[g] ? da : da + ga - i;
            o = i / u;
        }
    }
    iou[idx] = o;
}

// One workgroup per group.  grp row: {iou0, ldg, dt0, gt0, dsel0, D, gsel0, G}: the image's IoU matrix iou[iou0 + r * ldg + c]
// (r, c = detection / ground truth of the image), its first detection / ground truth in the flat arrays, and the group's
// detections dsel[dsel0 .. +D) (flat indices, descending score, already cut at maxDets[-1]) and ground truths gsel[gsel0 .. +G)
// (flat indices, document order).  Outputs of problem (group, a): see s2d_hip.h.
__global__ __launch_bounds__(64) void coco_match_kernel(const double *__restrict__ iou, const long *__restrict__ grp,
                                                        const int *__restrict__ dsel, const int *__restrict__ gsel,
                                                        const double *__restrict__ dt_area, const double *__restrict__ gt_area,
                                                        const uint8_t *__restrict__ gt_ignore, const uint8_t *__restrict__ crowd,
                                                        const double *__restrict__ thrs, int T, const double *__restrict__ rng, int A,
                                                        int *__restrict__ dtm, int *__restrict__ gtm, int *__restrict__ dt_ig,
                                                        int *__restrict__ gt_ig, int *__restrict__ gperm)
{
    const long *gr = grp + (long)GRP_COLS * blockIdx.x;
    const long iou0 = gr[0], ldg = gr[1], dt0 = gr[2], gt0 = gr[3], dsel0 = gr[4], gsel0 = gr[6];
    const int D = (int)gr[5], G = (int)gr[7];
    const int *ds = dsel + dsel0, *gs = gsel + gsel0;

    // ground truths of every range, stably sorted with the ignored ones last: one lane per range
    for (int a = threadIdx.x; a < A; a += 64) {
        const double lo = rng[2 * a], hi = rng[2 * a + 1];
        int *ig = gt_ig + A * gsel0 + (long)a * G, *pm = gperm + A * gsel0 + (long)a * G;
        int k = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int j = 0; j < G; ++j) {
                const int g = gs[j];
                const int ign = (gt_ignore[g] || gt_area[g] < lo || gt_area[g] > hi) ? 1 : 0;
                if (ign == pass) {
                    ig[k] = ign;
                    pm[k] = j;
                    ++k;
                }
            }
    }
    __syncthreads();                                                          // the lists above are read by the range's T lanes

    for (int l = threadIdx.x; l < A * T; l += 64) {
        const int a = l / T, t = l - a * T;
        const double lo = rng[2 * a], hi = rng[2 * a + 1], thr = thrs[t];
        const int *ig = gt_ig + A * gsel0 + (long)a * G, *pm = gperm + A * gsel0 + (long)a * G;
        int *gm = gtm + (long)T * (A * gsel0 + (long)a * G) + (long)t * G;
        int *dm = dtm + (long)T * (A * dsel0 + (long)a * D) + (long)t * D;
        int *di = dt_ig + (long)T * (A * dsel0 + (long)a * D) + (long)t * D;
        for (int k = 0; k < G; ++k) gm[k] = -1;
        for (int d = 0; d < D; ++d) {
            const long row = iou0 + (long)(ds[d] - dt0) * ldg;
            double best = fmin(thr, 1.0 - 1e-10);
            int m = -1;
            for (int k = 0; k < G; ++k) {
                const int g = gs[pm[k]];
                if (gm[k] >= 0 && !crowd[g]) continue;                        // taken, and not a crowd
                if (m > -1 && ig[m] == 0 && ig[k] == 1) break;                // matched a regular gt: ignored ones come last
                const double v = iou[row + (g - gt0)];
                if (v < best) continue;                                       // equal IoU: the later ground truth wins
                best = v;
                m = k;
            }
            const double ar = dt_area[ds[d]];
            dm[d] = m;
            if (m >= 0) {
                gm[m] = d;
                di[d] = ig[m];
            } else {
                di[d] = (ar < lo || ar > hi) ? 1 : 0;
            }
        }
    }
}

}  // namespace

extern "C" {

int s2d_coco_mask_iou_ragged(const uint32_t *bits, const long *img, int N, const int *tiles, int n_tiles, const uint8_t *crowd,
                             long long *inter, int *area_d, int *area_g, double *iou, hipStream_t stream)
{
    if (N < 0 || n_tiles < 0) return S2D_ERR_ARG;
    if (N == 0 || n_tiles == 0) return S2D_OK;
    hipLaunchKernelGGL(ragged_mask_iou_kernel, dim3(n_tiles), dim3(256), 0, stream, bits, img, tiles, crowd, inter, area_d, area_g, iou);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_coco_box_iou_ragged(const double *dt_box, const double *gt_box, const uint8_t *crowd, const long *img, int N,
                            const long *pair_off, long n_pairs, double *iou, hipStream_t stream)
{
    if (N < 0 || n_pairs < 0 || n_pairs >= (1L << 31) * 256) return S2D_ERR_ARG;
    if (N == 0 || n_pairs == 0) return S2D_OK;
    hipLaunchKernelGGL(ragged_box_iou_kernel, dim3(cdiv(n_pairs, 256)), dim3(256), 0, stream, dt_box, gt_box, crowd, img, N, pair_off,
                       n_pairs, iou);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_coco_match(const double *iou, const long *groups, int n_groups, const int *dsel, const int *gsel, const double *dt_area,
                   const double *gt_area, const uint8_t *gt_ignore, const uint8_t *crowd, const double *iou_thrs, int T,
                   const double *area_rng, int A, int *dt_match, int *gt_match, int *dt_ignore, int *gt_ignore_out, int *gt_perm,
                   hipStream_t stream)
{
    if (n_groups < 0 || T < 1 || A < 1) return S2D_ERR_ARG;
    if (n_groups == 0) return S2D_OK;
    hipLaunchKernelGGL(coco_match_kernel, dim3(n_groups), dim3(64), 0, stream, iou, groups, dsel, gsel, dt_area, gt_area, gt_ignore,
                       crowd, iou_thrs, T, area_rng, A, dt_match, gt_match, dt_ignore, gt_ignore_out, gt_perm);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
