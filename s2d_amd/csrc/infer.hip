// Eval-side step after the path: what KDVideoMaskFormer.forward does with the network outputs when
// not training (model_training/mask2former_video/kd_video_maskformer_model.py:327-356) and inference_video (:530-610;
// video_maskformer_model.py:298-360 is the same code for the non-KD model):
//
//   scores = softmax(class logits)[:, :-1]; sorted top-K over the flattened [Q*C] scores;           (:532-538)
//   masks  = bilinear(mask logits -> padded input size) [:341-346], crop to the unpadded size [:545],
//            bilinear -> output size [:546-548], > 0 [:550];
//   optional greedy same-label mask-NMS with IoU from pairwise sum(a & b) / sum(a | b)               (:552-583)
//
// The reference materialises the [Q,T,Hp,Wp] fp32 upsample of ALL queries (0.94 GB per 10 frames at 720p, Q = 100), then
// the [K,T,oh,ow] fp32 resize, and runs the NMS as O(K^2) pairs of full-tensor reductions with a device->host sync each.
// Here: one selection kernel; the K selected queries' logits are gathered from the pixel-major maps into small planes;
// one kernel evaluates both bilinear stages per output pixel (16 low-resolution taps, the same fp32 expression tree as
// two consecutive F.interpolate calls) and writes the boolean mask once, as bytes (the tensor the caller gets) and as
// bit words; the tiled popcount kernel of mask_counts.hip (s2d_mask_pair_counts_u64) turns the bit words into the K x K
// intersection counts, from which the host runs the greedy loop without touching the masks again.
#include "common.h"
#include "class_select.h"
#include "draw_order.h"

namespace {

constexpr int SEL_THREADS = 1024;

// one workgroup: softmax per query, then rank every flat score (ties -> lower flat index comes first)
__global__ __launch_bounds__(SEL_THREADS) void infer_select_kernel(const float *__restrict__ cls, int Q, int C, int K,
                                                                   float *__restrict__ scores, int *__restrict__ query,
                                                                   int *__restrict__ label)
{
    extern __shared__ float sc[];                       // [Q*C]
    const int n = Q * C;
    for (int q = threadIdx.x; q < Q; q += SEL_THREADS) {
        const float *l = cls + (long)q * (C + 1);
        float mx = l[0];
        for (int c = 1; c <= C; ++c) mx = fmaxf(mx, l[c]);
        float sum = 0.f;
        for (int c = 0; c <= C; ++c) sum += expf(l[c] - mx);
        for (int c = 0; c < C; ++c) sc[q * C + c] = expf(l[c] - mx) / sum;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += SEL_THREADS) {
        const float s = sc[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float o = sc[j];
            rank += (o > s) || (o == s && j < i);
        }
        if (rank < K) { scores[rank] = s; query[rank] = i / C; label[rank] = i % C; }
    }
}

// planes[k][pix] = ml[pix][query[k]]   (pixel-major [T*hm*wm, ldq] -> K query-major planes), transposed through LDS: a
// workgroup takes 64 pixels; lanes run over k within a pixel's 512-B row when reading and over pixels when writing.
constexpr int GP = 64, GK = 128;
__global__ __launch_bounds__(256) void infer_gather_kernel(const float *__restrict__ ml, int ldq, long npix,
                                                           const int *__restrict__ query, int K, float *__restrict__ planes)
{
    __shared__ float tile[GK][GP + 1];
    __shared__ int qs[GK];
    const long pix0 = (long)blockIdx.x * GP;
    const int np = npix - pix0 < GP ? (int)(npix - pix0) : GP;
    for (int k0 = 0; k0 < K; k0 += GK) {
        const int kc = K - k0 < GK ? K - k0 : GK;
        __syncthreads();
        if ((int)threadIdx.x < kc) qs[threadIdx.x] = query[k0 + threadIdx.x];
        __syncthreads();
        for (int idx = threadIdx.x; idx < np * kc; idx += 256) {
            const int pp = idx / kc, k = idx - pp * kc;
            tile[k][pp] = ml[(pix0 + pp) * ldq + qs[k]];
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < kc * GP; idx += 256) {
            const int k = idx >> 6, pp = idx & 63;
            if (pp < np) planes[(long)(k0 + k) * npix + pix0 + pp] = tile[k][pp];
        }
    }
}

struct ResizeParams {
    const float *planes;       // [K][T][hm][wm]
    int T, hm, wm, Hp, Wp, ih, iw, oh, ow;
    long N;                    // T*oh*ow, elements of one mask
    long words;                // bit words per mask = ceil(N / 32)
    float s1y, s1x, s2y, s2x;  // hm/Hp, wm/Wp, ih/oh, iw/ow as float (area_pixel_compute_scale)
    int same;                  // output size == unpadded size: the second resize is the identity
    uint8_t *masks;            // [K][N]
    uint32_t *bits;            // [K][words] or null
};

// source index / weights of F.interpolate(mode="bilinear", align_corners=False)
__host__ __device__ __forceinline__ void src_tap(float scale, int dst, int in_size, int &i0, int &i1, float &l0, float &l1)
{
    float s = scale * (dst + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    i0 = (int)s;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = s - i0;
    l0 = 1.f - l1;
}

// value of the padded-size upsample (:341-346) from its two low-resolution rows and their weights
__device__ __forceinline__ float stage1(const float *__restrict__ r0, const float *__restrict__ r1, float hy, float ly, int x0,
                                        int x1, float hx, float lx)
{
    return hy * (hx * r0[x0] + lx * r0[x1]) + ly * (hx * r1[x0] + lx * r1[x1]);
}

// The vertical half of one output row's taps: stage-1 rows under stage-2 row Y0 (qa0, qa1 with weights hya, lya) and, two-stage
// only, under Y1 (qb0, qb1; hyb, lyb), with the stage-2 weights HY, LY (1, 0 when SAME: the second resize is the identity).
struct RowTaps {
    int qa0, qa1, qb0, qb1;
    float hya, lya, hyb, lyb, HY, LY;
};

template <bool SAME>
__device__ __forceinline__ RowTaps row_taps(float s1y, float s2y, int y, int hm, int ih)
{
    RowTaps r;
    r.qb0 = r.qb1 = 0; r.hyb = r.lyb = 0.f; r.HY = 1.f; r.LY = 0.f;
    if (SAME) {
        src_tap(s1y, y, hm, r.qa0, r.qa1, r.hya, r.lya);
    } else {
        int Y0, Y1;
        src_tap(s2y, y, ih, Y0, Y1, r.HY, r.LY);
        src_tap(s1y, Y0, hm, r.qa0, r.qa1, r.hya, r.lya);
        src_tap(s1y, Y1, hm, r.qb0, r.qb1, r.hyb, r.lyb);
    }
    return r;
}

// The horizontal half, per output column; the column indices come back multiplied by xs, the element stride of a low-resolution
// row (1 in a gathered plane, ldq in the pixel-major logits) and shifted by -x_org (the first column a staged window holds).
struct ColTaps {
    int xa0, xa1, xb0, xb1;
    float ha, la, hb, lb, HX, LX;
};

template <bool SAME>
__device__ __forceinline__ ColTaps col_taps(float s1x, float s2x, int x, int wm, int iw, int x_org = 0, int xs = 1)
{
    ColTaps c;
    c.xb0 = c.xb1 = 0; c.hb = c.lb = 0.f; c.HX = 1.f; c.LX = 0.f;
    if (SAME) {
        src_tap(s1x, x, wm, c.xa0, c.xa1, c.ha, c.la);
    } else {
        int X0, X1;
        src_tap(s2x, x, iw, X0, X1, c.HX, c.LX);
        src_tap(s1x, X0, wm, c.xa0, c.xa1, c.ha, c.la);
        src_tap(s1x, X1, wm, c.xb0, c.xb1, c.hb, c.lb);
        c.xb0 = (c.xb0 - x_org) * xs; c.xb1 = (c.xb1 - x_org) * xs;
    }
    c.xa0 = (c.xa0 - x_org) * xs; c.xa1 = (c.xa1 - x_org) * xs;
    return c;
}

// The value of the two-stage resize at one output pixel, from the four low-resolution rows a0, a1 (under Y0), b0, b1 (under Y1):
// THE float32 expression tree of masks and index maps alike (SAME: stage 1 alone).  Both kernels call this and nothing else, so
// the sign of v, which is all either of them keeps of it, is the same bit in both.
template <bool SAME>
__device__ __forceinline__ float resize_value(const float *__restrict__ a0, const float *__restrict__ a1, const float *__restrict__ b0,
                                              const float *__restrict__ b1, const RowTaps &r, const ColTaps &c)
{
    if (SAME) return stage1(a0, a1, r.hya, r.lya, c.xa0, c.xa1, c.ha, c.la);
    return r.HY * (c.HX * stage1(a0, a1, r.hya, r.lya, c.xa0, c.xa1, c.ha, c.la) + c.LX * stage1(a0, a1, r.hya, r.lya, c.xb0, c.xb1, c.hb, c.lb)) +
           r.LY * (c.HX * stage1(b0, b1, r.hyb, r.lyb, c.xa0, c.xa1, c.ha, c.la) + c.LX * stage1(b0, b1, r.hyb, r.lyb, c.xb0, c.xb1, c.hb, c.lb));
}

// A thread owns 4 consecutive elements of one mask (flat index over [T][oh][ow]); 8 lanes make one 32-bit word.  The
// vertical taps are formed once per thread and again only when its 4 elements wrap into the next row.
template <bool SAME>
__global__ __launch_bounds__(256) void infer_resize_kernel(ResizeParams p)
{
    const int k = blockIdx.y;
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    unsigned int nib = 0u;
    if (i0 < p.N) {
        int t, y, x;
        if (p.N < (1L << 31)) {                          // 32-bit index arithmetic (the usual case)
            const unsigned int frame = (unsigned int)p.oh * (unsigned int)p.ow, i = (unsigned int)i0;
            const unsigned int tt = i / frame, r = i - tt * frame, yy = r / (unsigned int)p.ow;
            t = (int)tt; y = (int)yy; x = (int)(r - yy * (unsigned int)p.ow);
        } else {
            const long frame = (long)p.oh * p.ow;
            t = (int)(i0 / frame);
            const long r = i0 - (long)t * frame;
            y = (int)(r / p.ow); x = (int)(r - (long)y * p.ow);
        }
        // stage-1 rows (a: under stage-2 row Y0, b: under Y1; SAME uses a only) and the stage-2 vertical weights
        const float *a0 = nullptr, *a1 = nullptr, *b0 = nullptr, *b1 = nullptr;
        RowTaps r;
#define S2D_SET_ROW()                                                                           \
        do {                                                                                    \
            const float *pl = p.planes + ((long)k * p.T + t) * p.hm * p.wm;                     \
            r = row_taps<SAME>(p.s1y, p.s2y, y, p.hm, p.ih);                                    \
            a0 = pl + r.qa0 * p.wm; a1 = pl + r.qa1 * p.wm;                                     \
            if (!SAME) { b0 = pl + r.qb0 * p.wm; b1 = pl + r.qb1 * p.wm; }                      \
        } while (0)
        S2D_SET_ROW();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j < p.N) {
                const ColTaps c = col_taps<SAME>(p.s1x, p.s2x, x, p.wm, p.iw);
                const float v = resize_value<SAME>(a0, a1, b0, b1, r, c);
                nib |= (v > 0.f ? 1u : 0u) << j;
            }
            if (++x == p.ow) {
                x = 0;
                if (++y == p.oh) { y = 0; ++t; }
                if (j < 3 && i0 + j + 1 < p.N) S2D_SET_ROW();
            }
        }
#undef S2D_SET_ROW
        uint8_t *mo = p.masks + (long)k * p.N + i0;
        if (i0 + 4 <= p.N && (reinterpret_cast<uintptr_t>(mo) & 3) == 0)
            *reinterpret_cast<uint32_t *>(mo) = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
        else
            for (int j = 0; j < 4 && i0 + j < p.N; ++j) mo[j] = (nib >> j) & 1u;
    }
    if (p.bits) {                                       // whole waves reach this point: lanes past N carry 0
        unsigned int w = nib << (4 * (threadIdx.x & 7));
        w |= __shfl_xor(w, 1, 64);
        w |= __shfl_xor(w, 2, 64);
        w |= __shfl_xor(w, 4, 64);
        const long wi = i0 >> 5;
        if ((threadIdx.x & 7) == 0 && wi < p.words) p.bits[(long)k * p.words + wi] = w;
    }
}

// u8 mask planes [K][n] (0 / non-0) -> bit words [K][ceil(n / 32)] (flat index i -> word i / 32, bit i % 32; tail bits zero):
// the input format of s2d_mask_pair_counts_u64 (mask_counts.hip), for masks that exist as byte planes (the KD pseudo targets, DISTILLATION_NMS)
__global__ __launch_bounds__(256) void pack_bits_kernel(const uint8_t *__restrict__ masks, long n, long words, uint32_t *__restrict__ bits)
{
    const int k = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;                  // element index; a wave covers two words
    const bool v = i < n && masks[(long)k * n + i] != 0;
    const unsigned long long b = __ballot(v);
    const int lane = threadIdx.x & 63;
    const long w = i >> 5;
    if ((lane & 31) == 0 && w < words) bits[(long)k * words + w] = (uint32_t)(lane ? (b >> 32) : (b & 0xFFFFFFFFull));
}

// ---- proposal index maps (DAVIS): low-resolution logits -> one label per output pixel, no [K][T][oh][ow] tensor -------------
//
// One workgroup of 256 threads owns an IX_TH x IX_TW = 16 x 64 tile of one output frame; a thread owns 4 consecutive pixels of
// one tile row and writes them as one dword.  The low-resolution window under the tile (rows win_lo(first tile row) ..
// win_hi(last tile row), the same for columns: src_tap is monotone in dst, so the taps of every pixel of the tile lie inside)
// is gathered once into LDS as K planes [K][wh*ww] -- only the K selected columns of each 4*ldq-byte logit row -- and the 16 taps
// x K of every pixel are LDS reads.  Without it every output pixel would do 16 x K scattered global reads; a low-resolution
// pixel feeds about (oh/hm)^2 output pixels (28 at DAVIS 480p from a 360-pixel test size).
//
// Tile, LDS and occupancy: at that size the window is 6 x 15 pixels, at K = 20 7.2 KB (+ 2 KB of query / score).  The two-stage
// kernel holds the four pixels' column taps in registers (132 VGPRs; 63 for SAME), so three workgroups (12 waves) run per CU,
// four or eight for SAME: registers, not the 28 KB of LDS those three take of 160 KB, bound occupancy there.  A wider tile would amortise the one-pixel window apron better (the
// window is (16/5.3 + 3) x (64/5.3 + 3) for 1024 pixels: the apron is a third of it), but 64 is the widest at which a 256-thread
// workgroup still has 16 rows, and a 4-row wave reads few distinct LDS rows per instruction.  IX_LDS_BYTES = 40 KB is the budget:
// the three workgroups the registers admit still fit a CU (126 of 160 KB), so a large K costs no occupancy; K * window
// beyond it (K = 254 over more than 40 window pixels, or a strong downscale) takes the direct path: the same arithmetic on
// the pixel-major logits themselves, column indices scaled by ldq.  The launcher computes the largest window over all tiles
// with the same win_lo / win_hi the kernel uses; a workgroup whose own window would still not fit what was allocated (it cannot
// happen: host and device evaluate the same float32 operations) reads directly instead of past its LDS.
constexpr int IX_TH = 16, IX_TW = 64, IX_KMAX = 254, IX_LDS_BYTES = 40 * 1024;

template <bool SAME>
__host__ __device__ __forceinline__ int win_lo(float s1, float s2, int dst, int in_low, int in_mid)
{
    int i0, i1; float l0, l1;
    if (!SAME) { src_tap(s2, dst, in_mid, i0, i1, l0, l1); dst = i0; }
    src_tap(s1, dst, in_low, i0, i1, l0, l1);
    return i0;
}

template <bool SAME>
__host__ __device__ __forceinline__ int win_hi(float s1, float s2, int dst, int in_low, int in_mid)
{
    int i0, i1; float l0, l1;
    if (!SAME) { src_tap(s2, dst, in_mid, i0, i1, l0, l1); dst = i1; }
    src_tap(s1, dst, in_low, i0, i1, l0, l1);
    return i1;
}

// four labels of one tile row: one dword where the address allows, else nx bytes
__device__ __forceinline__ void store_labels(uint8_t *o, const unsigned int (&lab)[4], int nx)
{
    if (nx == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0)
        *reinterpret_cast<uint32_t *>(o) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
    else
        for (int j = 0; j < nx; ++j) o[j] = (uint8_t)lab[j];
}

// What the tiled kernels (index maps, frame areas, paint) share of one call: the logits, the selection and the geometry that
// index_geometry fills.
struct TileParams {
    const float *ml;           // [T*hm*wm][ldq]
    const int *query;          // [K]
    int ldq, T, hm, wm, ih, iw, oh, ow, K;
    int tiles_x, tiles_y;
    int cap;                   // window pixels the dynamic LDS holds per proposal (0: every workgroup reads directly)
    float s1y, s1x, s2y, s2x;
};

struct IndexParams : TileParams {
    const float *score;        // [K] (rule 1)
    uint8_t *index;            // [T][oh][ow]
    int rule;
};

struct AreaParams : TileParams {
    int *areas;                // [K][T], zero before the launch
};

struct PaintParams : TileParams {
    const int *order;          // [T][K]
    const uint8_t *colors;     // [K][3]
    uint8_t *rgb;              // [T][oh][ow][3]
    uint8_t *index;            // [T][oh][ow] or null
};

// The tile of blockIdx.x and the low-resolution window under it (workgroup-uniform)
struct TileWindow {
    int t, y0, x0;             // frame, first output row / column of the tile
    int rlo, clo, ww, np;      // first window row / column, window width, window pixels
    bool staged;               // the window fits the dynamic LDS: the taps are LDS reads, else reads of the logits themselves
    const float *frame;        // the frame's logits [hm*wm][ldq]
};

template <bool SAME>
__device__ __forceinline__ TileWindow tile_window(const TileParams &p)
{
    TileWindow w;
    const unsigned int per_frame = (unsigned int)p.tiles_x * (unsigned int)p.tiles_y;
    w.t = (int)(blockIdx.x / per_frame);
    const unsigned int rem = blockIdx.x - (unsigned int)w.t * per_frame;
    const int ty = (int)(rem / (unsigned int)p.tiles_x), tx = (int)(rem - (unsigned int)ty * (unsigned int)p.tiles_x);
    w.y0 = ty * IX_TH; w.x0 = tx * IX_TW;
    const int ylast = (w.y0 + IX_TH < p.oh ? w.y0 + IX_TH : p.oh) - 1, xlast = (w.x0 + IX_TW < p.ow ? w.x0 + IX_TW : p.ow) - 1;
    // the window; clamped to the map so that no tap arithmetic, however it rounds, makes the gather read outside the logits
    w.rlo = win_lo<SAME>(p.s1y, p.s2y, w.y0, p.hm, p.ih); w.clo = win_lo<SAME>(p.s1x, p.s2x, w.x0, p.wm, p.iw);
    int rhi = win_hi<SAME>(p.s1y, p.s2y, ylast, p.hm, p.ih), chi = win_hi<SAME>(p.s1x, p.s2x, xlast, p.wm, p.iw);
    if (rhi > p.hm - 1) rhi = p.hm - 1;
    if (chi > p.wm - 1) chi = p.wm - 1;
    w.ww = chi - w.clo + 1;
    w.np = (rhi - w.rlo + 1) * w.ww;
    w.staged = w.np >= 1 && w.np <= p.cap;
    w.frame = p.ml + (long)w.t * p.hm * p.wm * p.ldq;
    return w;
}

// qs[k] = query[k] clamped into [0, ldq); staged: win[k][window pixel] = that column of the logits under the tile.  Every thread
// of the workgroup calls it; what the caller wrote to LDS before the call is visible after it.
__device__ __forceinline__ void stage_window(const TileParams &p, const TileWindow &w, int *qs, float *win)
{
    for (int k = threadIdx.x; k < p.K; k += 256) {
        int q = p.query[k];
        qs[k] = q < 0 ? 0 : (q > p.ldq - 1 ? p.ldq - 1 : q);
    }
    __syncthreads();
    if (w.staged) {
        for (int idx = threadIdx.x; idx < w.np * p.K; idx += 256) {
            const int pp = idx / p.K, k = idx - pp * p.K;
            const int wr = pp / w.ww, wc = pp - wr * w.ww;
            win[k * w.np + pp] = w.frame[((long)(w.rlo + wr) * p.wm + (w.clo + wc)) * p.ldq + qs[k]];
        }
        __syncthreads();
    }
}

// The taps of a thread's 4 consecutive pixels (y, xb .. xb + 3) of one tile row, (y, xb) inside the frame
struct PixelTaps {
    RowTaps r;
    ColTaps c[4];
    long oa0, oa1, ob0, ob1;   // element offsets of the four rows inside one proposal's plane (staged) or the frame's logits (direct)
    int nx;                    // pixels of the four inside the frame
};

template <bool SAME>
__device__ __forceinline__ PixelTaps pixel_taps(const TileParams &p, const TileWindow &w, int y, int xb)
{
    PixelTaps t;
    t.nx = p.ow - xb < 4 ? p.ow - xb : 4;
    t.r = row_taps<SAME>(p.s1y, p.s2y, y, p.hm, p.ih);
#pragma unroll
    for (int j = 0; j < 4; ++j)                         // a column past the frame edge repeats the last one; its result is not stored
        t.c[j] = col_taps<SAME>(p.s1x, p.s2x, xb + (j < t.nx ? j : t.nx - 1), p.wm, p.iw, w.staged ? w.clo : 0, w.staged ? 1 : p.ldq);
    const long rs = w.staged ? (long)w.ww : (long)p.wm * p.ldq;
    const int ro = w.staged ? w.rlo : 0;
    t.oa0 = (t.r.qa0 - ro) * rs; t.oa1 = (t.r.qa1 - ro) * rs;
    t.ob0 = SAME ? 0 : (t.r.qb0 - ro) * rs; t.ob1 = SAME ? 0 : (t.r.qb1 - ro) * rs;
    return t;
}

// where proposal k's taps are read from: its staged plane, or its column of the frame's logits
__device__ __forceinline__ const float *proposal_base(const TileWindow &w, const float *win, const int *qs, int k)
{
    return w.staged ? win + k * w.np : w.frame + qs[k];
}

// resize_value of proposal `base` at pixel j of the thread's four
template <bool SAME>
__device__ __forceinline__ float pixel_value(const float *__restrict__ base, const PixelTaps &t, int j)
{
    return resize_value<SAME>(base + t.oa0, base + t.oa1, base + t.ob0, base + t.ob1, t.r, t.c[j]);
}

template <bool SAME>
__global__ __launch_bounds__(256) void infer_index_kernel(IndexParams p)
{
    extern __shared__ float win[];                      // [K][wh*ww]
    __shared__ int qs[IX_KMAX];
    __shared__ float ss[IX_KMAX];
    const TileWindow w = tile_window<SAME>(p);
    for (int k = threadIdx.x; k < p.K; k += 256) ss[k] = p.rule ? p.score[k] : 0.f;
    stage_window(p, w, qs, win);

    const int y = w.y0 + (int)(threadIdx.x >> 4), xb = w.x0 + (int)(threadIdx.x & 15) * 4;
    if (y >= p.oh || xb >= p.ow) return;
    const PixelTaps px = pixel_taps<SAME>(p, w, y, xb);

    unsigned int lab[4] = {0u, 0u, 0u, 0u};
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < p.K; ++k) {
        const float *base = proposal_base(w, win, qs, k);
        if (p.rule == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (lab[j] == 0u && pixel_value<SAME>(base, px, j) > 0.f) lab[j] = (unsigned int)k + 1u;
            if (lab[0] && lab[1] && lab[2] && lab[3]) break;
        } else {
            const float s = ss[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = pixel_value<SAME>(base, px, j);
                if (v > 0.f) {
                    const float pr = s / (1.f + expf(-v));
                    if (lab[j] == 0u || pr > best[j]) { lab[j] = (unsigned int)k + 1u; best[j] = pr; }
                }
            }
        }
    }
    store_labels(p.index + ((long)w.t * p.oh + y) * p.ow + xb, lab, px.nx);
}

// ---- stage-1 frame masks (keymask/frame_masks.py): the paint rule of the reference's overlay_masks_numpy, plane-free -------------
//
// The reference (cutler/demo/predictor.py:237-355) sorts a frame's instances by descending mask area and paints them on black
// in that order, each in the colour of its own index, so the smallest holder of a pixel shows.  Two kernels on the index kernel's
// tile scheme (same window, staging and taps: tile_window / stage_window / pixel_taps above, so "proposal k holds the pixel" is the
// bit s2d_infer_masks_u8 writes):
//
//  areas  every proposal at every pixel of the tile (no early exit: a covered pixel still counts); the holders of a wave are
//         counted per pixel slot with a ballot and a popcount -- scalar instructions -- and lane 0 writes the wave's count of
//         proposal k to cnt[wave][k]; after the loop one integer atomicAdd per (k, t) and workgroup, skipped for a count of 0.
//         Integer sums do not depend on the order of the adds, so a second call gives the same bits.
//  paint  the frame's draw order in LDS, walked from the last position (painted last, on top) to the first; the first holder met
//         owns the pixel, and a thread leaves the loop when its four pixels are owned, as rule 0 of the index kernel does.
//
// Registers and LDS: areas 87 VGPRs two-stage (5 waves per SIMD; 64 for SAME) and 5 KB of static LDS (qs, cnt) beside the staged
// window; paint 124 VGPRs two-stage (4 waves per SIMD; 60 for SAME) and 2 KB (qs, ord).  Registers bound occupancy below 18 KB of
// staging; at the 40 KB limit three workgroups of either fit a CU, as for the index kernel.
template <bool SAME>
__global__ __launch_bounds__(256) void infer_frame_areas_kernel(AreaParams p)
{
    extern __shared__ float win[];                      // [K][wh*ww]
    __shared__ int qs[IX_KMAX];
    __shared__ int cnt[4][IX_KMAX];                     // [wave][k]
    const TileWindow w = tile_window<SAME>(p);
    stage_window(p, w, qs, win);

    // no thread leaves before the barrier below: one outside the frame forms the taps of the tile's first pixel and counts nothing
    const int y = w.y0 + (int)(threadIdx.x >> 4), xb = w.x0 + (int)(threadIdx.x & 15) * 4;
    const bool inside = y < p.oh && xb < p.ow;
    const PixelTaps px = pixel_taps<SAME>(p, w, inside ? y : w.y0, inside ? xb : w.x0);
    const int n = inside ? px.nx : 0;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    for (int k = 0; k < p.K; ++k) {
        const float *base = proposal_base(w, win, qs, k);
        int c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = pixel_value<SAME>(base, px, j);
            c += __popcll(__ballot(j < n && v > 0.f));
        }
        if (lane == 0) cnt[wave][k] = c;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < p.K; k += 256) {
        const int c = cnt[0][k] + cnt[1][k] + cnt[2][k] + cnt[3][k];
        if (c) atomicAdd(&p.areas[(long)k * p.T + w.t], c);
    }
}

template <bool SAME>
__global__ __launch_bounds__(256) void infer_paint_kernel(PaintParams p)
{
    extern __shared__ float win[];                      // [K][wh*ww]
    __shared__ int qs[IX_KMAX];
    __shared__ int ord[IX_KMAX];
    const TileWindow w = tile_window<SAME>(p);
    for (int r = threadIdx.x; r < p.K; r += 256) {      // an entry outside [0, K) is clamped: nothing is read out of range
        const int k = p.order[(long)w.t * p.K + r];
        ord[r] = k < 0 ? 0 : (k > p.K - 1 ? p.K - 1 : k);
    }
    stage_window(p, w, qs, win);

    const int y = w.y0 + (int)(threadIdx.x >> 4), xb = w.x0 + (int)(threadIdx.x & 15) * 4;
    if (y >= p.oh || xb >= p.ow) return;
    const PixelTaps px = pixel_taps<SAME>(p, w, y, xb);

    unsigned int own[4] = {0u, 0u, 0u, 0u};
    for (int r = p.K - 1; r >= 0; --r) {
        const int k = ord[r];
        const float *base = proposal_base(w, win, qs, k);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (own[j] == 0u && pixel_value<SAME>(base, px, j) > 0.f) own[j] = (unsigned int)k + 1u;
        if (own[0] && own[1] && own[2] && own[3]) break;
    }

    uint32_t wd[3] = {0u, 0u, 0u};                      // the 12 bytes of the four pixels
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (own[j]) {
            const uint8_t *col = p.colors + 3 * (own[j] - 1u);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) wd[(3 * j + ch) >> 2] |= (uint32_t)col[ch] << (8 * ((3 * j + ch) & 3));
        }
    const long pix = ((long)w.t * p.oh + y) * p.ow + xb;
    uint8_t *o = p.rgb + pix * 3;
    if (px.nx == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        reinterpret_cast<uint32_t *>(o)[0] = wd[0];
        reinterpret_cast<uint32_t *>(o)[1] = wd[1];
        reinterpret_cast<uint32_t *>(o)[2] = wd[2];
    } else {
        for (int b = 0; b < 3 * px.nx; ++b) o[b] = (uint8_t)(wd[b >> 2] >> (8 * (b & 3)));
    }
    if (p.index) store_labels(p.index + pix, own, px.nx);
}

// largest window (pixels) of any tile, from the same tap functions the kernel evaluates
template <bool SAME>
long index_max_window(const TileParams &p)
{
    int mh = 0, mw = 0;
    for (int ty = 0; ty < p.tiles_y; ++ty) {
        const int ylast = (ty * IX_TH + IX_TH < p.oh ? ty * IX_TH + IX_TH : p.oh) - 1;
        int hi = win_hi<SAME>(p.s1y, p.s2y, ylast, p.hm, p.ih);
        if (hi > p.hm - 1) hi = p.hm - 1;
        const int h = hi - win_lo<SAME>(p.s1y, p.s2y, ty * IX_TH, p.hm, p.ih) + 1;
        if (h > mh) mh = h;
    }
    for (int tx = 0; tx < p.tiles_x; ++tx) {
        const int xlast = (tx * IX_TW + IX_TW < p.ow ? tx * IX_TW + IX_TW : p.ow) - 1;
        int hi = win_hi<SAME>(p.s1x, p.s2x, xlast, p.wm, p.iw);
        if (hi > p.wm - 1) hi = p.wm - 1;
        const int w = hi - win_lo<SAME>(p.s1x, p.s2x, tx * IX_TW, p.wm, p.iw) + 1;
        if (w > mw) mw = w;
    }
    return (long)mh * mw;
}

}  // namespace

extern "C" {

int s2d_infer_select_f32(const float *cls_logits, int Q, int C, int K, float *scores, int *query, int *label, hipStream_t stream)
{
    if (Q < 1 || C < 1 || K < 1 || K > Q * C) return S2D_ERR_ARG;
    const size_t lds = sizeof(float) * (size_t)Q * C;
    if (lds > 64 * 1024) return S2D_ERR_ARG;
    hipLaunchKernelGGL(infer_select_kernel, dim3(1), dim3(SEL_THREADS), lds, stream, cls_logits, Q, C, K, scores, query, label);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

long s2d_infer_select_c_workspace_bytes(int Q, int C1) { return C1 < 2 ? 0 : cls_select_workspace_bytes(1, Q, C1); }

// s2d_infer_select_f32 for any Q*C (class_select.h): the same scores, order and tie rule, without the 64 KB LDS bound
int s2d_infer_select_c_f32(const float *cls_logits, int Q, int C1, int K, void *workspace, float *scores, int *query, int *label,
                           hipStream_t stream)
{
    if (Q < 1 || C1 < 2 || K < 1 || (long)K > (long)Q * (C1 - 1) || (long)Q * (C1 - 1) > 0x7FFFFFFFL / 2) return S2D_ERR_ARG;
    int *rank = nullptr;
    cls_select_launch(cls_logits, 1, Q, C1, K, -1.f, workspace, &rank, scores, query, label, stream);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

long s2d_infer_workspace_floats(int K, int T, int hm, int wm) { return (long)K * T * hm * wm; }

long s2d_mask_bit_words(int T, int oh, int ow) { return ((long)T * oh * ow + 31) / 32; }

int s2d_infer_masks_u8(const float *mask_logits, int ldq, int T, int hm, int wm, int Hp, int Wp, int ih, int iw, int oh, int ow,
                       const int *query, int K, float *workspace, uint8_t *masks, uint32_t *bits, hipStream_t stream)
{
    if (K < 0 || T < 1 || hm < 1 || wm < 1 || ih < 1 || iw < 1 || ih > Hp || iw > Wp || oh < 1 || ow < 1) return S2D_ERR_ARG;
    if (K == 0) return S2D_OK;
    const long npix = (long)T * hm * wm;
    hipLaunchKernelGGL(infer_gather_kernel, dim3(cdiv(npix, GP)), dim3(256), 0, stream, mask_logits, ldq, npix, query, K, workspace);
    ResizeParams p;
    p.planes = workspace;
    p.T = T; p.hm = hm; p.wm = wm; p.Hp = Hp; p.Wp = Wp; p.ih = ih; p.iw = iw; p.oh = oh; p.ow = ow;
    p.N = (long)T * oh * ow;
    p.words = (p.N + 31) / 32;
    p.s1y = (float)hm / Hp; p.s1x = (float)wm / Wp; p.s2y = (float)ih / oh; p.s2x = (float)iw / ow;
    p.same = (ih == oh && iw == ow) ? 1 : 0;
    p.masks = masks; p.bits = bits;
    const long nthreads = (p.words * 32 + 3) / 4;       // whole words: the tail lanes write the zero padding bits
    if (p.same) hipLaunchKernelGGL(infer_resize_kernel<true>, dim3(cdiv(nthreads, 256), K), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(infer_resize_kernel<false>, dim3(cdiv(nthreads, 256), K), dim3(256), 0, stream, p);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

// geometry of one tiled call (s2d_infer_index_u8, s2d_infer_frame_areas_i32, s2d_infer_paint_u8) -> p (pointers left alone); false:
// the sizes are refused
static bool index_geometry(TileParams &p, int ldq, int T, int hm, int wm, int Hp, int Wp, int ih, int iw, int oh, int ow, int K)
{
    if (K < 1 || K > IX_KMAX || ldq < 4 || ldq > 128 || (ldq & 3)) return false;
    if (T < 1 || hm < 1 || wm < 1 || ih < 1 || iw < 1 || ih > Hp || iw > Wp || oh < 1 || ow < 1) return false;
    if ((long)hm * wm * ldq > 0x7FFFFFFFL) return false;
    p.ldq = ldq; p.T = T; p.hm = hm; p.wm = wm; p.ih = ih; p.iw = iw; p.oh = oh; p.ow = ow; p.K = K;
    p.tiles_x = cdiv(ow, IX_TW); p.tiles_y = cdiv(oh, IX_TH);
    if ((long)T * p.tiles_x * p.tiles_y >= (1L << 31)) return false;
    p.s1y = (float)hm / Hp; p.s1x = (float)wm / Wp; p.s2y = (float)ih / oh; p.s2x = (float)iw / ow;
    const long maxwin = (ih == oh && iw == ow) ? index_max_window<true>(p) : index_max_window<false>(p);
    p.cap = (maxwin >= 1 && maxwin * K * (long)sizeof(float) <= IX_LDS_BYTES) ? (int)maxwin : 0;
    return true;
}

long s2d_infer_index_lds_bytes(int ldq, int T, int hm, int wm, int Hp, int Wp, int ih, int iw, int oh, int ow, int K)
{
    TileParams p;
    if (!index_geometry(p, ldq, T, hm, wm, Hp, Wp, ih, iw, oh, ow, K)) return -1;
    return (long)p.cap * K * (long)sizeof(float);
}

int s2d_infer_index_u8(const float *mask_logits, int ldq, int T, int hm, int wm, int Hp, int Wp, int ih, int iw, int oh, int ow,
                       const int *query, const float *score, int K, int rule, uint8_t *index, hipStream_t stream)
{
    if (!mask_logits || !query || !index || (rule != 0 && rule != 1) || (rule == 1 && !score)) return S2D_ERR_ARG;
    IndexParams p;
    if (!index_geometry(p, ldq, T, hm, wm, Hp, Wp, ih, iw, oh, ow, K)) return S2D_ERR_ARG;
    p.ml = mask_logits; p.query = query; p.score = score; p.index = index; p.rule = rule;
    const bool same = ih == oh && iw == ow;
    const long nblocks = (long)T * p.tiles_x * p.tiles_y;
    const size_t lds = (size_t)p.cap * K * sizeof(float);
    if (same) hipLaunchKernelGGL(infer_index_kernel<true>, dim3((unsigned int)nblocks), dim3(256), lds, stream, p);
    else hipLaunchKernelGGL(infer_index_kernel<false>, dim3((unsigned int)nblocks), dim3(256), lds, stream, p);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_infer_frame_areas_i32(const float *mask_logits, int ldq, int T, int hm, int wm, int Hp, int Wp, int ih, int iw, int oh, int ow,
                              const int *query, int K, int *areas, int *order, hipStream_t stream)
{
    if (!mask_logits || !query || !areas) return S2D_ERR_ARG;
    AreaParams p;
    if (!index_geometry(p, ldq, T, hm, wm, Hp, Wp, ih, iw, oh, ow, K)) return S2D_ERR_ARG;
    p.ml = mask_logits; p.query = query; p.areas = areas;
    if (s2d_zero_async(areas, sizeof(int) * (size_t)K * T, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    const long nblocks = (long)T * p.tiles_x * p.tiles_y;
    const size_t lds = (size_t)p.cap * K * sizeof(float);
    if (ih == oh && iw == ow) hipLaunchKernelGGL(infer_frame_areas_kernel<true>, dim3((unsigned int)nblocks), dim3(256), lds, stream, p);
    else hipLaunchKernelGGL(infer_frame_areas_kernel<false>, dim3((unsigned int)nblocks), dim3(256), lds, stream, p);
    if (order) hipLaunchKernelGGL(draw_order_kernel, dim3(T), dim3(256), 0, stream, areas, K, T, order);   // K <= 254 threads rank
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_infer_paint_u8(const float *mask_logits, int ldq, int T, int hm, int wm, int Hp, int Wp, int ih, int iw, int oh, int ow,
                       const int *query, int K, const int *order, const uint8_t *colors, uint8_t *rgb, uint8_t *index, hipStream_t stream)
{
    if (!mask_logits || !query || !order || !colors || !rgb) return S2D_ERR_ARG;
    PaintParams p;
    if (!index_geometry(p, ldq, T, hm, wm, Hp, Wp, ih, iw, oh, ow, K)) return S2D_ERR_ARG;
    p.ml = mask_logits; p.query = query; p.order = order; p.colors = colors; p.rgb = rgb; p.index = index;
    const long nblocks = (long)T * p.tiles_x * p.tiles_y;
    const size_t lds = (size_t)p.cap * K * sizeof(float);
    if (ih == oh && iw == ow) hipLaunchKernelGGL(infer_paint_kernel<true>, dim3((unsigned int)nblocks), dim3(256), lds, stream, p);
    else hipLaunchKernelGGL(infer_paint_kernel<false>, dim3((unsigned int)nblocks), dim3(256), lds, stream, p);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_pack_mask_bits_u8(const uint8_t *masks, int K, long n, uint32_t *bits, hipStream_t stream)
{
    if (K < 0 || n <= 0) return S2D_ERR_ARG;
    if (K == 0) return S2D_OK;
    const long words = (n + 31) / 32;
    if ((words * 32 + 255) / 256 >= (1L << 31)) return S2D_ERR_ARG;
    hipLaunchKernelGGL(pack_bits_kernel, dim3(cdiv(words * 32, 256), K), dim3(256), 0, stream, masks, n, words, bits);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
