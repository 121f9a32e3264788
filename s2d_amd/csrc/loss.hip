// VideoSetCriterion on the device (model_training/mask2former_video/modeling/criterion.py) and the
// distillation-target preparation (kd_video_maskformer_model.py:418-528), batched over all prediction layers
// and clips of a criterion pass, with no device->host synchronisation (the reference syncs once per target
// row in the DropLoss loop, criterion.py:310-322, and materialises [R,3P] point tensors + a full topk).
//
// loss_masks (criterion.py:292-356 + point_features.py:63-116) only needs SUMS over the selected points, so:
//   1. matched query maps are gathered once from the pixel-major logits into query-major rows (L2-resident);
//   2. the 0.75P most-uncertain of 3P uniform points (smallest |logit|) are found EXACTLY by a 3-level radix
//      select on the float bits of |x| (11+10+10 bits, LDS-privatised histograms) -- no sort, no [R,3P] tensor;
//   3. one more pass re-samples the points, keeps those under the threshold, samples the target there and
//      accumulates BCE / dice sums; the 0.25P extra uniform points are added in the same pass.
// Points come from an injected coordinate buffer (parity mode: the recorded torch.rand draws) or from a
// counter-based RNG keyed by (seed, row, index), so re-sampling in every pass is free of HBM traffic.
// All partial sums land in fixed slots and are reduced in a fixed order (double): deterministic losses.
//
// THE TIE RULE.  The selected set is "the n_unc smallest |logit|"; among points whose |logit| equals the n_unc-th smallest bit for bit
// the reference's torch.topk leaves the choice open.  Here it is defined: ascending |x|, then ascending POINT INDEX within the row's
// oversampled points (what a stable argsort gives, and what oracle/ does).  With `take` = n_unc - #(keys below the threshold), the
// take tied points of lowest index are kept, on every path:
//   - rows whose samples are kept (accumulate_stream_kernel, forward and backward): a list of up to TIECAP ties ranked by index, a
//     block scan beyond; the backward applies a per-tie ownership test per map part (injected points) or carries the ties spent by
//     the earlier parts' index ranges (generated points, tie_before);
//   - rows whose samples are not kept (3P or P/4 not a multiple of 4, H*W not a multiple of 32, active rows beyond XBUF_MAX_ROWS):
//     accumulate_kernel keeps every tie when take equals their number (select_kernel<2> leaves that number in LossParams::tie) and
//     none otherwise; accumulate_ties_kernel then adds the first `take` by index.
// The rule depends on neither the map part a point lies in nor on how workgroups are scheduled, so two runs give the same bits.
// tests/test_gpu_point_loss_ties.py pins it with inputs whose keys tie exactly.
#include "common.h"
#include "class_select.h"
#include <climits>

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t hash32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// per-(seed, stream) key, computed once per work item (wave-uniform)
__device__ __forceinline__ uint32_t rand_key(uint64_t seed, uint64_t stream)
{
    return (uint32_t)mix64(seed ^ mix64(stream * 0xD1342543DE82EF95ull));
}
// Two uniforms in [0,1) with 24 random bits each (torch.rand's float construction) for counter i.  Round 5: u from hash32(key + i), v from ONE
// more multiply-xorshift round of that hash (3 quarter-rate integer multiplies per point instead of the 4 of two independent hashes: the
// point generator is 70 % of hist_kernel<0>).  Statistics of the pair stream over i (480 000 points, three keys; profiles/r5_experiments/
// not_adopted.txt item 6 has the method): KS of u and of v, corr(u, v), serial correlations, 2-D chi-square of (u, v) and of the serial pairs
// (u_i, u_i+1), (v_i, v_i+1) on 128 x 128 cells -- all |z| < 2.2; the two-hash generator it replaces scored z = 2.5-4.5 on the serial pairs
// (its counters key + 2 i and key + 2 i + 1 are neighbours).
__device__ __forceinline__ uint32_t rand_u_bits(uint32_t key, uint32_t i) { return hash32(key + i); }
__device__ __forceinline__ uint32_t rand_v_bits(uint32_t a)
{
    uint32_t b = a * 0x9E3779B1u;
    b ^= b >> 15;
    return b ^ 0x85ebca6bu;
}
__device__ __forceinline__ void rand2(uint32_t key, uint32_t i, float &u, float &v)
{
    const uint32_t a = rand_u_bits(key, i);
    u = (float)(a >> 8) * (1.0f / 16777216.0f);
    v = (float)(rand_v_bits(a) >> 8) * (1.0f / 16777216.0f);
}

// bilinear sample (grid_sample, zeros padding, align_corners=False) of a [H,W] plane at (u,v) in [0,1]
template <typename T>
__device__ __forceinline__ float sample_plane(const T *__restrict__ pl, int H, int W, float u, float v)
{
    const float gx = 2.f * u - 1.f, gy = 2.f * v - 1.f;
    const float x = ((gx + 1.f) * W - 1.f) * 0.5f, y = ((gy + 1.f) * H - 1.f) * 0.5f;
    const int x0 = (int)floorf(x), y0 = (int)floorf(y), x1 = x0 + 1, y1 = y0 + 1;
    const float fx = x - x0, fy = y - y0;
    // zero padding without branches: clamp the tap into the plane and zero its weight (4 unconditional loads)
    const float wxa = (x0 >= 0 && x0 < W) ? 1.f - fx : 0.f, wxb = (x1 >= 0 && x1 < W) ? fx : 0.f;
    const float wya = (y0 >= 0 && y0 < H) ? 1.f - fy : 0.f, wyb = (y1 >= 0 && y1 < H) ? fy : 0.f;
    const int xa = min(max(x0, 0), W - 1), xb = min(max(x1, 0), W - 1);
    const int ya = min(max(y0, 0), H - 1) * W, yb = min(max(y1, 0), H - 1) * W;
    float acc = (float)pl[ya + xa] * (wxa * wya);
    acc += (float)pl[ya + xb] * (wxb * wya);
    acc += (float)pl[yb + xa] * (wxa * wyb);
    acc += (float)pl[yb + xb] * (wxb * wyb);
    return acc;
}

// ------------------------------------------------------------------------------------------------ KD targets
// kd_video_maskformer_model.py:436-456: scores = softmax(logits)[:, :-1]; top-K; keep score >= thr.
// Kept queries are emitted in ascending query order (the reference's topk(sorted=False) order is
// implementation-defined; every downstream quantity is invariant to a permutation of the targets).
__global__ void kd_select_kernel(const float *__restrict__ cls, int Q, int K, float thr, int Nmax, int *__restrict__ count,
                                 int *__restrict__ kept)
{
    __shared__ float sc[128];
    __shared__ int keep[128];
    const int b = blockIdx.x, q = threadIdx.x;
    if (q < Q) {
        const float l0 = cls[((long)b * Q + q) * 2], l1 = cls[((long)b * Q + q) * 2 + 1];
        const float mx = fmaxf(l0, l1);
        const float e0 = expf(l0 - mx), e1 = expf(l1 - mx);
        sc[q] = e0 / (e0 + e1);
    }
    __syncthreads();
    if (q < Q) {
        int rank = 0;
        for (int j = 0; j < Q; ++j) rank += (sc[j] > sc[q]) || (sc[j] == sc[q] && j < q);
        keep[q] = (rank < K) && (sc[q] >= thr);
    }
    __syncthreads();
    if (q == 0) {
        int c = 0;
        for (int j = 0; j < Q; ++j)
            if (keep[j] && c < Nmax) kept[b * Nmax + c++] = j;
        count[b] = c;
    }
}

// masks = bilinear(teacher mask logits -> (H,W), align_corners=False) > 0   (:462-468), written as u8 planes
__global__ __launch_bounds__(256) void kd_upsample_kernel(const float *__restrict__ ml, int ldq, int T, int hm, int wm, int H,
                                                          int W, int Nmax, const int *__restrict__ count,
                                                          const int *__restrict__ kept, uint8_t *__restrict__ tgt,
                                                          int *__restrict__ nonempty)
{
    __shared__ int kq[128];
    __shared__ unsigned int anyset[128];
    const int bt = blockIdx.z, b = bt / T, t = bt % T;
    const int Y = blockIdx.y, X = blockIdx.x * 256 + threadIdx.x;
    const int cnt = count[b];
    if (threadIdx.x < 128) {
        kq[threadIdx.x] = threadIdx.x < cnt ? kept[b * Nmax + threadIdx.x] : 0;
        anyset[threadIdx.x] = 0u;
    }
    __syncthreads();
    if (X < W) {
        float sy = ((float)hm / H) * (Y + 0.5f) - 0.5f; if (sy < 0.f) sy = 0.f;
        float sx = ((float)wm / W) * (X + 0.5f) - 0.5f; if (sx < 0.f) sx = 0.f;
        const int y0 = (int)sy, x0 = (int)sx, y1 = y0 + (y0 < hm - 1 ? 1 : 0), x1 = x0 + (x0 < wm - 1 ? 1 : 0);
        const float ly = sy - y0, lx = sx - x0, hy = 1.f - ly, hx = 1.f - lx;
        const float *fr = ml + ((long)b * T + t) * hm * wm * ldq;
        const float *r00 = fr + ((long)y0 * wm + x0) * ldq, *r01 = fr + ((long)y0 * wm + x1) * ldq;
        const float *r10 = fr + ((long)y1 * wm + x0) * ldq, *r11 = fr + ((long)y1 * wm + x1) * ldq;
        for (int k = 0; k < cnt; ++k) {
            const int q = kq[k];
            const float val = hy * (hx * r00[q] + lx * r01[q]) + ly * (hx * r10[q] + lx * r11[q]);
            const uint8_t m = val > 0.f ? 1 : 0;
            tgt[((((long)b * Nmax + k) * T + t) * H + Y) * W + X] = m;
            if (m) anyset[k] = 1u;  // benign race: all writers store 1
        }
    }
    __syncthreads();
    if (threadIdx.x < cnt && anyset[threadIdx.x]) nonempty[((long)b * Nmax + threadIdx.x) * T + t] = 1;
}

// The same masks, tiled: a workgroup owns 16 output rows x 256 output columns of a frame.  The logits are pixel-major
// ([pixel][query]) and only the kept queries are wanted, so the form above re-fetches every source pixel's lines for each of the
// output rows and columns it feeds (x 4 upsampling: 16 outputs per source pixel, spread over 4 workgroups): 3.9 GB through L1 for a
// 0.38 GB tensor.  Here the tile's source window (<= 8 x 72 pixels) is read once per chunk of 8 kept queries -- lanes along the
// query index, so a pixel's lines are fetched by neighbouring lanes -- into LDS planes, and every output takes its 4 taps from
// there; 4 output columns per thread, one 32-bit store.  Same arithmetic per output, bit for bit.
constexpr int KDT_H = 16, KDT_W = 256, KDT_SH = 8, KDT_SW = 72, KDT_KC = 8;
__global__ __launch_bounds__(256) void kd_upsample_tile_kernel(const float *__restrict__ ml, int ldq, int T, int hm, int wm, int H,
                                                               int W, int Nmax, const int *__restrict__ count,
                                                               const int *__restrict__ kept, uint8_t *__restrict__ tgt,
                                                               int *__restrict__ nonempty)
{
    __shared__ int kq[128];
    __shared__ unsigned int anyset[128];
    __shared__ float src[KDT_KC][KDT_SH][KDT_SW];
    const int bt = blockIdx.z, b = bt / T, t = bt % T;
    const int Y0 = blockIdx.y * KDT_H, X0 = blockIdx.x * KDT_W;
    const int cnt = count[b];
    if (threadIdx.x < 128) {
        kq[threadIdx.x] = threadIdx.x < cnt ? kept[b * Nmax + threadIdx.x] : 0;
        anyset[threadIdx.x] = 0u;
    }
    auto srcpos = [](int o, int n_out, int n_in, int &i0, int &i1, float &l) {
        float s = ((float)n_in / n_out) * (o + 0.5f) - 0.5f; if (s < 0.f) s = 0.f;
        i0 = (int)s; i1 = i0 + (i0 < n_in - 1 ? 1 : 0); l = s - i0;
    };
    int ya, yb_, xa, xb_; float dummy;
    srcpos(Y0, H, hm, ya, yb_, dummy);
    srcpos(X0, W, wm, xa, xb_, dummy);
    const float *fr = ml + ((long)b * T + t) * hm * wm * ldq;
    // this thread's outputs: rows Y0 + (tid >> 6) + 4 p (p = 0 .. 3), columns X0 + 4 (tid & 63) .. + 3
    const int xg = X0 + 4 * (threadIdx.x & 63);
    int x0[4], x1[4]; float lx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) srcpos(min(xg + e, W - 1), W, wm, x0[e], x1[e], lx[e]);
    __syncthreads();
    for (int k0 = 0; k0 < cnt; k0 += KDT_KC) {
        const int kc = min(KDT_KC, cnt - k0);
        for (int i = threadIdx.x; i < KDT_SH * KDT_SW * KDT_KC; i += 256) {
            const int kk = i % KDT_KC, pix = i / KDT_KC, sx = pix % KDT_SW, sy = pix / KDT_SW;
            const int gy = min(ya + sy, hm - 1), gx = min(xa + sx, wm - 1);
            if (kk < kc) src[kk][sy][sx] = fr[((long)gy * wm + gx) * ldq + kq[k0 + kk]];
        }
        __syncthreads();
#pragma unroll
        for (int pss = 0; pss < 4; ++pss) {
            const int Y = Y0 + (threadIdx.x >> 6) + 4 * pss;
            if (Y >= H || xg >= W) continue;
            int y0, y1; float ly;
            srcpos(Y, H, hm, y0, y1, ly);
            const float hy = 1.f - ly;
            for (int kk = 0; kk < kc; ++kk) {
                unsigned int word = 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float hx = 1.f - lx[e];
                    const float val = hy * (hx * src[kk][y0 - ya][x0[e] - xa] + lx[e] * src[kk][y0 - ya][x1[e] - xa]) +
                                      ly * (hx * src[kk][y1 - ya][x0[e] - xa] + lx[e] * src[kk][y1 - ya][x1[e] - xa]);
                    word |= (val > 0.f ? 1u : 0u) << (8 * e);
                }
                *reinterpret_cast<unsigned int *>(tgt + ((((long)b * Nmax + k0 + kk) * T + t) * H + Y) * W + xg) = word;
                if (word) anyset[k0 + kk] = 1u;  // benign race: all writers store 1
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < cnt && anyset[threadIdx.x]) atomicOr(&nonempty[((long)b * Nmax + threadIdx.x) * T + t], 1);
}

// nonempty[b][n][t] = any(tgt[b][n][t])   (the DropLoss predicate, criterion.py:310-313).  A plane is cut into NE_CHUNKS pieces
// (one workgroup each: 160 planes alone leave a third of the CUs idle); `nonempty` is zeroed by the launcher and pieces OR into it.
constexpr int NE_CHUNKS = 8;
__global__ __launch_bounds__(256) void nonempty_kernel(const uint8_t *__restrict__ tgt, const int *__restrict__ count, int Nmax,
                                                       int T, long HW, int *__restrict__ nonempty)
{
    const int plane = blockIdx.x;  // (b*Nmax + n)*T + t
    const int n = (plane / T) % Nmax, b = plane / (T * Nmax);
    if (n >= count[b]) return;
    const uint8_t *p = tgt + (long)plane * HW;
    int any = 0;
    const long n16 = HW / 16, per = (n16 + NE_CHUNKS - 1) / NE_CHUNKS;
    const long lo = blockIdx.y * per, hi = min(lo + per, n16);
    const uint4 *p4 = reinterpret_cast<const uint4 *>(p);
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        const uint4 v = p4[i];
        any |= (v.x | v.y | v.z | v.w) != 0u;
    }
    if (blockIdx.y == 0)
        for (long i = n16 * 16 + threadIdx.x; i < HW; i += 256) any |= p[i] != 0;
    any = __syncthreads_or(any);
    if (threadIdx.x == 0 && any) atomicOr(&nonempty[plane], 1);
}

// ------------------------------------------------------------------------------------------------ rows
struct LossParams {
    const float *ml;          // [NL][B][T*hm*wm][ldq] pixel-major mask logits
    const uint8_t *tgt;       // [B][Nmax][T][H][W]
    const int *tgt_count;     // [B]
    const int *nonempty;      // [B][Nmax][T]
    const int *idx_q, *idx_t; // [NL*B][maxm]
    const int *n_match;       // [NL*B]
    const float *coords_over; // [NL][Rmax_l][n_over][2] or null (Rmax_l = B*maxm*T; slot = rank among kept rows of the layer)
    const float *coords_rand; // [NL][Rmax_l][n_rand][2] or null
    uint64_t seed;
    int NL, B, Q, ldq, T, hm, wm, H, W, Nmax, maxm, n_over, n_unc, n_rand, drop;
    float world_size;
    // workspace
    int *active, *rank;       // [rows]
    int *list;                // [rows] compact list of active row ids (deterministic order: layer, clip, slot, frame)
    int *lcount;              // [NL + 1]: kept rows per layer; [NL] = total
    float *mq;                // [rows][hm*wm]
    unsigned int *hist;       // [rows][2048]
    unsigned int *prefix;     // [rows]  key prefix found so far
    int *krem;                // [rows]  how many still to take inside the prefix
    unsigned int *tie;        // [rows]  how many points sit AT the threshold key (select_kernel<2>); krem of them are taken
    float *part;              // [rows][chunks][4]
    int chunks;
    float *xbuf;              // [xcap][n_over + n_rand]: sampled logits of the first xcap active rows (sampled ONCE)
    unsigned int *tpack;       // [B][Nmax][T][H*W/32]: every target plane of the pass bit-packed once (pack_planes_kernel); bit i of word w = pixel 32 w + i
    int bits_global;           // the accumulate pass reads a row's plane from tpack directly (it does not fit LDS) instead of copying it to LDS
    int xcap;
    int *pbound;              // [rows][PB_STRIDE]: RNG mode, first oversampled-point index of every map part of the row (strata)
};

// The row a point stream is keyed by: (layer, clip, slot, frame) with the slot stride fixed at Q instead of maxm = min(Q, Nmax), so that the points
// of a matched (pair, frame) do not depend on how far the target planes are padded (the training iteration hands the KD pass planes cut to the
// number of pseudo targets it found; forward + loss alone pads them to Q).  NL == 0: the test hook s2d_point_loss_rng_points, whose rows ARE keys.
__device__ __forceinline__ uint64_t key_row(const LossParams &p, long rowid)
{
    if (p.NL == 0) return (uint64_t)rowid;
    const long per = (long)p.maxm * p.T;
    const long lb = rowid / per;
    return (uint64_t)(lb * ((long)p.Q * p.T) + (rowid - lb * per));
}

constexpr int PB_STRIDE = 9;  // LOSS_CHUNKS + 1
struct VRange {
    float v0, dv;             // v band of one map part: v = v0 + dv * r, r uniform in [0, 1)
};

// one block per layer: active flag + rank (= position among the kept rows of this layer, reference row order
// (clip, slot, frame): criterion.py:298-322)
__global__ void row_prep_kernel(LossParams p)
{
    const int layer = blockIdx.x;
    const int rows_l = p.B * p.maxm * p.T;
    __shared__ int base;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int r0 = 0; r0 < rows_l; r0 += blockDim.x) {
        const int r = r0 + threadIdx.x;
        int act = 0;
        if (r < rows_l) {
            const int t = r % p.T, s = (r / p.T) % p.maxm, b = r / (p.T * p.maxm);
            const int prob = layer * p.B + b;
            if (s < p.n_match[prob]) {
                const int n = p.idx_t[(long)prob * p.maxm + s];
                act = p.drop ? p.nonempty[((long)b * p.Nmax + n) * p.T + t] : 1;
            }
        }
        // block-wide exclusive scan of `act` in thread order (blockDim.x == 256: 4 waves)
        __shared__ int wsum[4];
        const unsigned long long m = __ballot(act);
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const int inw = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wv; ++w) off += wsum[w];
        if (r < rows_l) {
            const long rowid = (long)layer * rows_l + r;
            p.active[rowid] = act;
            p.rank[rowid] = off + inw;
        }
        __syncthreads();
        if (threadIdx.x == 0) base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.lcount[layer] = base;
}

__global__ void row_list_kernel(LossParams p)
{
    const int layer = blockIdx.x;
    const int rows_l = p.B * p.maxm * p.T;
    int base = 0;
    for (int l = 0; l < layer; ++l) base += p.lcount[l];
    for (int r = threadIdx.x; r < rows_l; r += blockDim.x) {
        const long rowid = (long)layer * rows_l + r;
        if (p.active[rowid]) p.list[base + p.rank[rowid]] = (int)rowid;
    }
    if (layer == p.NL - 1 && threadIdx.x == 0) p.lcount[p.NL] = base + p.lcount[layer];
}

// RNG mode: the multinomial split of every active row's n_over oversampled points over its map parts (see part_vrange below);
// one thread per row, sequential conditional binomials
__device__ int binomial_inv(int N, double p, double U);
__global__ __launch_bounds__(256) void row_strata_kernel(LossParams p, int nparts, int rpp)
{
    const int n = p.lcount[p.NL];
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = gridDim.x * 4;
    for (int li = wave; li < n; li += nwaves) {                  // one wave per row: binomial_inv is a wave-wide call
        const long rowid = p.list[li];
        int *pb = p.pbound + rowid * PB_STRIDE;
        int rem = p.n_over, at = 0;
        double mass = 1.0;
        for (int j = 0; j < nparts; ++j) {
            if ((threadIdx.x & 63) == 0) pb[j] = at;
            const double ya = j == 0 ? -0.5 : (double)(j * rpp), yb = j == nparts - 1 ? (double)p.hm - 0.5 : (double)((j + 1) * rpp);
            const double pj = (yb - ya) / (double)p.hm;
            int nj = rem;
            if (j < nparts - 1) {
                const uint64_t h = mix64(p.seed ^ mix64((key_row(p, rowid) * 16u + (uint64_t)j) * 0xD1342543DE82EF95ull + 0x5851F42D4C957F2Dull));
                const double U = (double)(h >> 11) * (1.0 / 9007199254740992.0);      // 53-bit uniform in [0, 1)
                const double pc = pj / mass;
                nj = binomial_inv(rem, pc < 1.0 ? pc : 1.0, U);
            }
            at += nj; rem -= nj; mass -= pj;
        }
        if ((threadIdx.x & 63) == 0) pb[nparts] = at;
    }
}

__global__ void rng_points_prep_kernel(int *list, int nrows)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nrows) list[i] = i;
    else if (i == nrows) list[i] = nrows;
}
__device__ __forceinline__ void over_point_rng(uint32_t key0, int i, const int *pb, const float *v0, const float *dv, int nparts, float &u, float &v);
__device__ __forceinline__ VRange part_vrange(int j, int nparts, int rpp, int hm);
__global__ void rng_points_kernel(LossParams p, int nparts, int rpp, float *__restrict__ uv)
{
    const int row = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    __shared__ float s_v0[PB_STRIDE], s_dv[PB_STRIDE];
    if ((int)threadIdx.x < nparts) { const VRange vr = part_vrange(threadIdx.x, nparts, rpp, p.hm); s_v0[threadIdx.x] = vr.v0; s_dv[threadIdx.x] = vr.dv; }
    __syncthreads();
    if (i >= p.n_over) return;
    float u, v;
    over_point_rng(rand_key(p.seed, (uint64_t)row * 2), i, p.pbound + (long)row * PB_STRIDE, s_v0, s_dv, nparts, u, v);
    uv[((long)row * p.n_over + i) * 2] = u;
    uv[((long)row * p.n_over + i) * 2 + 1] = v;
}

// gather matched query maps: mq[row][pix] = ml[layer][b][t][pix][q]; 64 pixels per block through LDS
__global__ __launch_bounds__(256) void gather_rows_kernel(LossParams p)
{
    __shared__ float tile[64][129];
    const int prob = blockIdx.z, t = blockIdx.y, pix0 = blockIdx.x * 64;
    const int layer = prob / p.B, b = prob % p.B;
    const int hw = p.hm * p.wm;
    const int nm = p.n_match[prob];
    const long row_base = (((long)layer * p.B + b) * p.maxm) * p.T;
    bool any = false;
    for (int s = 0; s < nm; ++s) any = any || p.active[row_base + (long)s * p.T + t];
    if (!any) return;
    const float *src = p.ml + (((long)prob * p.T + t) * hw + pix0) * p.ldq;
    const int npix = min(64, hw - pix0);
    // the tile is one contiguous run of npix * ldq floats (ldq % 4 == 0, 16-B aligned): 16-B loads, scalar LDS writes
    // (odd row stride: the column reads below stay conflict-free)
    const int l4 = p.ldq >> 2;
    // all of a thread's 16-B loads first (64 pixels x ldq <= 128 floats: at most 8 per thread), then the LDS writes: with one load
    // per loop trip the kernel read its 3.8 GB at 3.7 TB/s
    f32x4 v[8];
    const int tot = npix * l4;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int e = threadIdx.x + 256 * k;
        if (e < tot) v[k] = *reinterpret_cast<const f32x4 *>(src + (long)e * 4);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int e = threadIdx.x + 256 * k;
        if (e < tot) {
            const int px = e / l4, q = (e - px * l4) * 4;
            if (q < 128) { tile[px][q] = v[k][0]; tile[px][q + 1] = v[k][1]; tile[px][q + 2] = v[k][2]; tile[px][q + 3] = v[k][3]; }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int s = wv; s < nm; s += 4) {
        const long rowid = row_base + (long)s * p.T + t;
        if (!p.active[rowid]) continue;
        const int q = p.idx_q[(long)prob * p.maxm + s];
        if (lane < npix) p.mq[rowid * hw + pix0 + lane] = tile[lane][q];
    }
}

__device__ __forceinline__ const float *coord_rows(const LossParams &p, long rowid, bool over)
{
    const float *c = over ? p.coords_over : p.coords_rand;
    if (!c) return nullptr;
    const long rows_l = (long)p.B * p.maxm * p.T;
    const long n = over ? p.n_over : p.n_rand;
    return c + ((rowid / rows_l) * rows_l + p.rank[rowid]) * n * 2;
}

// ---- LDS-staged sampling --------------------------------------------------------------------------------------
// The radix-select passes evaluate 3P = 480 000 bilinear samples per matched row on a 235 KB logit map.  Read from
// L2 every 4-byte tap moves a 64-B sector (measured: ~12 ms per pass, fabric-bound).  Instead a work item = (row,
// part): the workgroup copies one horizontal part of the map (<= 120 KB, + 1 overlap row) into LDS once, regenerates
// the row's points from the counter RNG and handles those whose upper tap row falls in its part; all four taps
// are then LDS reads.  v (the y coordinate) is drawn first so foreign points are dropped after one hash.
constexpr int PART_BYTES = 124 * 1024;
constexpr int PADC = 4;                 // zero columns either side of a staged row (16-B aligned copies; x0 = -1 / x1 = wm land on them)
constexpr int LTHREADS = 512;
struct PartGeom {
    int rows_per_part, nparts;
};
__host__ __device__ inline PartGeom part_geom(int hm, int wm)
{
    PartGeom g;
    // RNG mode stages a part with a zero border -- rows_per_part + 1 map rows, a zero row above and below, PADC zero columns either
    // side -- so that the bilinear taps need no border tests (stage_part_padded); that block must fit PART_BYTES
    g.rows_per_part = PART_BYTES / ((wm + 2 * PADC) * 4) - 3;
    if (g.rows_per_part > hm) g.rows_per_part = hm;
    g.nparts = (hm + g.rows_per_part - 1) / g.rows_per_part;
    return g;
}

// ---- RNG mode: the oversampled points of a row are generated per map part (stratified, same law) ---------------------------
// point_features.py:89-93 draws the 3P oversampled points of a row i.i.d. uniform on [0,1]^2.  A map part owns the points whose
// upper tap row falls in it, i.e. a band of v.  N i.i.d. uniform points are, in law, exactly: a multinomial split (n_0, ..,
// n_{k-1}) of N over the bands with the bands' areas as probabilities, then n_j points i.i.d. uniform inside band j.  The device
// generator (timing mode; parity mode injects the reference's recorded draws and keeps the test-every-point path) draws that
// multinomial once per row -- exact binomial inversion in double, row_strata_kernel -- and point i of the row then lies in the
// band j with bound[j] <= i < bound[j+1]: v = v0_j + dv_j * r_i, u = r'_i with 24-bit uniforms r, r' as before.  A (row, part)
// work item walks only its own index range: no per-point ownership test, no compaction (they were ~40 % of hist_kernel<0>'s
// 1.4 G vector instructions per criterion pass: every point was tested by both parts).
__host__ __device__ inline void part_yrange(int j, int nparts, int rpp, int hm, double &ya, double &yb)
{
    ya = j == 0 ? -0.5 : (double)(j * rpp);                       // y = v * hm - 0.5 in [-0.5, hm - 0.5); part j owns floor(y) in [j * rpp, (j+1) * rpp)
    yb = j == nparts - 1 ? (double)hm - 0.5 : (double)((j + 1) * rpp);
}
__device__ __forceinline__ VRange part_vrange(int j, int nparts, int rpp, int hm)
{
    double ya, yb;
    part_yrange(j, nparts, rpp, hm, ya, yb);
    VRange r;
    r.v0 = (float)((ya + 0.5) / (double)hm);
    r.dv = (float)((yb - ya) / (double)hm);
    return r;
}
// (u, v) of oversampled point i of a row in RNG mode.  pb: the row's strata bounds, v0 / dv: the bands of the map's parts (LDS
// tables filled once per workgroup: part_vrange divides in double)
__device__ __forceinline__ void over_point_rng(uint32_t key0, int i, const int *pb, const float *v0, const float *dv, int nparts, float &u, float &v)
{
    int j = 0;
    while (j + 1 < nparts && i >= pb[j + 1]) ++j;
    const uint32_t ra_ = rand_u_bits(key0, (uint32_t)i);
    u = (float)(ra_ >> 8) * (1.0f / 16777216.0f);
    v = fmaf((float)(rand_v_bits(ra_) >> 8) * (1.0f / 16777216.0f), dv[j], v0[j]);
}

// Binomial(N, p) by inversion of U, one WAVE per draw (all 64 lanes call with the same arguments and receive the same value).
// Any fixed enumeration order of the support gives an exact sampler; the order here is: the mode m, then alternately the next
// 32 values above and the next 32 below.  A step evaluates one such 64-value block: lane's pmf = frontier pmf x prefix product
// of the two-sided recurrence ratios (6 shuffle steps), block prefix sum (6 more), first lane where U goes negative.  ~1.6 sigma /
// 32 = ~17 steps for N = 480 000, p = 1/2 (the one-thread walk took 0.3 ms per criterion pass, all in double divisions).
__device__ int binomial_inv(int N, double p, double U)
{
    if (N <= 0 || p <= 0.0) return 0;
    if (p >= 1.0) return N;
    const int lane = threadIdx.x & 63, l = lane & 31;
    const bool isup = lane < 32;
    const double q = 1.0 - p, r = p / q, ri = q / p;
    int m = (int)floor((double)(N + 1) * p);
    if (m > N) m = N;
    const double f0 = exp(lgamma((double)N + 1.0) - lgamma((double)m + 1.0) - lgamma((double)(N - m) + 1.0) + (double)m * log(p) +
                          (double)(N - m) * log1p(-p));
    U -= f0;
    if (U < 0.0) return m;
    double fu = f0, fd = f0;                                     // pmf at the two frontiers
    int up = m, dn = m;
    for (int it = 0; it < (1 << 15); ++it) {
        const int k = isup ? up + 1 + l : dn - 1 - l;
        const bool valid = isup ? k <= N : k >= 0;
        // pmf(k) = pmf(k-1) (N-k+1)/k p/q  going up;  pmf(k) = pmf(k+1) (k+1)/(N-k) q/p  going down
        double pr = !valid ? 0.0 : isup ? (double)(N - k + 1) / (double)k * r : (double)(k + 1) / (double)(N - k) * ri;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const double t = __shfl_up(pr, o, 32);
            if (l >= o) pr *= t;
        }
        const double f = (isup ? fu : fd) * pr;
        double cs = f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double t = __shfl_up(cs, o, 64);
            if (lane >= o) cs += t;
        }
        const unsigned long long hit = __ballot(U - cs < 0.0);
        if (hit) return __shfl(k, __ffsll((long long)hit) - 1, 64);
        U -= __shfl(cs, 63, 64);
        fu = __shfl(f, 31, 64);
        fd = __shfl(f, 63, 64);
        up += 32; dn -= 32;
        if ((up >= N && dn <= 0) || (fu < 1e-300 && fd < 1e-300)) break;   // U fell into the rounding residue of the total mass
    }
    return m;
}

// persistent item loop: item = (active row index li, part)
struct PartIter {
    int w, n_items, nparts;
    __device__ PartIter(const LossParams &p, int nparts_, int first_row = 0)
        : w(blockIdx.x + first_row * nparts_), n_items(p.lcount[p.NL] * nparts_), nparts(nparts_) {}
    __device__ bool next(const LossParams &p, long &rowid, int &part, int &li)
    {
        if (w >= n_items) return false;
        li = w / nparts;
        rowid = p.list[li];
        part = w % nparts;
        w += gridDim.x;
        return true;
    }
};

// copy rows [r0, r0+nr) of the row's map into LDS (16-B loads)
__device__ __forceinline__ void stage_part(const float *__restrict__ map, int wm, int r0, int nr, float *__restrict__ sm)
{
    const int n4 = nr * wm / 4;   // wm % 4 == 0 is checked on the host
    const f32x4 *src = reinterpret_cast<const f32x4 *>(map + (long)r0 * wm);
    f32x4 *dst = reinterpret_cast<f32x4 *>(sm);
    for (int i = threadIdx.x; i < n4; i += LTHREADS) dst[i] = src[i];
}

// The same rows with a zero border: LDS row 1 + (y - r0), column PADC + x.  Row 0 (y = r0 - 1: the row above the map for part 0)
// and the row after the last staged one (y = hm for the last part) are zero, as are PADC columns either side of every row.
__device__ __forceinline__ void stage_part_padded(const float *__restrict__ map, int wm, int r0, int nr, float *__restrict__ sm)
{
    const int wp = wm + 2 * PADC, w4 = wm / 4;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < wp / 4; i += LTHREADS) {
        reinterpret_cast<f32x4 *>(sm)[i] = z;
        reinterpret_cast<f32x4 *>(sm + (long)(nr + 1) * wp)[i] = z;
    }
    for (int i = threadIdx.x; i < nr; i += LTHREADS) {
        *reinterpret_cast<f32x4 *>(sm + (long)(i + 1) * wp) = z;
        *reinterpret_cast<f32x4 *>(sm + (long)(i + 1) * wp + PADC + wm) = z;
    }
    const f32x4 *src = reinterpret_cast<const f32x4 *>(map + (long)r0 * wm);
    for (int e = threadIdx.x; e < nr * w4; e += LTHREADS) {
        const int row = e / w4, c4 = e - row * w4;
        *reinterpret_cast<f32x4 *>(sm + (long)(row + 1) * wp + PADC + 4 * c4) = src[e];
    }
}

// bilinear sample from the padded block: no border tests, no clamps (a tap outside the map reads a zero).  Same products and the
// same order of additions as sample_part, whose out-of-map taps carry weight 0: same bits.
__device__ __forceinline__ float sample_part_padded(const float *__restrict__ sm, int wp, int r0, float x, float y, int x0, int y0)
{
    const float fx = x - x0, fy = y - y0;
    const float *b = sm + (y0 - r0 + 1) * wp + x0 + PADC;
    float acc = b[0] * ((1.f - fx) * (1.f - fy));
    acc += b[1] * (fx * (1.f - fy));
    acc += b[wp] * ((1.f - fx) * fy);
    acc += b[wp + 1] * (fx * fy);
    return acc;
}

// bilinear sample from the staged part; (y0 - r0, y0 + 1 - r0) are guaranteed inside the part for owned points
__device__ __forceinline__ float sample_part(const float *__restrict__ sm, int hm, int wm, int r0, int nr, float x, float y, int x0, int y0)
{
    const int x1 = x0 + 1, y1 = y0 + 1;
    const float fx = x - x0, fy = y - y0;
    const float wxa = (x0 >= 0) ? 1.f - fx : 0.f, wxb = (x1 < wm) ? fx : 0.f;
    const float wya = (y0 >= 0) ? 1.f - fy : 0.f, wyb = (y1 < hm) ? fy : 0.f;
    const int xa = max(x0, 0), xb = min(x1, wm - 1);
    // rows are clamped into the staged part, so points owned by another part still read valid LDS (result unused)
    const int ya = min(max(y0 - r0, 0), nr - 1) * wm, yb = min(max(min(y1, hm - 1) - r0, 0), nr - 1) * wm;
    float acc = sm[ya + xa] * (wxa * wya);
    acc += sm[ya + xb] * (wxb * wya);
    acc += sm[yb + xa] * (wxa * wyb);
    acc += sm[yb + xb] * (wxb * wyb);
    return acc;
}

// timing experiments only (scripts/build_loss_dbg.sh; results wrong by construction): 1 no histogram atomics, 2 no LDS taps, 4 no sample store
#ifndef S2D_LOSS_DBG
#define S2D_LOSS_DBG 0
#endif
// level 0: bits 30..20, level 1: bits 19..10, level 2: bits 9..0 of |x|
template <int LEVEL>
__global__ __launch_bounds__(LTHREADS) void hist_kernel(LossParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int hq_idx[LTHREADS / 64][128];
    __shared__ float hq_y[LTHREADS / 64][128];
    constexpr int nb = LEVEL == 0 ? 2048 : 1024;
    const PartGeom g = part_geom(p.hm, p.wm);
    unsigned int *h = reinterpret_cast<unsigned int *>(smem);
    float *sm = smem + 2048;
    PartIter it(p, g.nparts, LEVEL == 0 ? 0 : p.xcap);
    long rowid; int part, li;
    while (it.next(p, rowid, part, li)) {
        __syncthreads();
        for (int i = threadIdx.x; i < nb; i += LTHREADS) h[i] = 0u;
        const int r0 = part * g.rows_per_part;
        const int nr = min(g.rows_per_part + 1, p.hm - r0);
        const float *cr = coord_rows(p, rowid, true);
        const bool padded = cr == nullptr;                        // RNG mode (uniform over the workgroup)
        const int wp = p.wm + 2 * PADC;
        if (padded) stage_part_padded(p.mq + rowid * p.hm * p.wm, p.wm, r0, nr, sm);
        else stage_part(p.mq + rowid * p.hm * p.wm, p.wm, r0, nr, sm);
        __syncthreads();
        const unsigned int pre = LEVEL > 0 ? p.prefix[rowid] : 0u;
        const uint32_t key0 = rand_key(p.seed, key_row(p, rowid) * 2);
        // this part owns points with y0 in [r0, r0 + rows_per_part); y0 = -1 belongs to part 0
        const int ylo = part == 0 ? -1 : r0, yhi = r0 + g.rows_per_part;
        auto tally = [&](int i, float xv) {
            const unsigned int key = __float_as_uint(fabsf(xv));
            if (LEVEL == 0 && li < p.xcap && !(S2D_LOSS_DBG & 4)) p.xbuf[(long)li * (p.n_over + p.n_rand) + i] = xv;
            if ((S2D_LOSS_DBG & 1) && LEVEL == 0) { if (key == 0x12345u) h[0] = 1u; return; }
            if (LEVEL == 0) atomicAdd(&h[key >> 20], 1u);
            else if (LEVEL == 1) { if ((key >> 20) == (pre >> 20)) atomicAdd(&h[(key >> 10) & 1023u], 1u); }
            else { if ((key >> 10) == (pre >> 10)) atomicAdd(&h[key & 1023u], 1u); }
        };
        if (!cr) {
            // RNG mode: this item's points are the index range [pb[part], pb[part + 1]) of the row (stratified generation above): every
            // lane does full work, nothing is tested or compacted.  floor(y) is clamped into the part: v = v0 + dv * r may round onto
            // the band's upper edge (one point in ~1e7), which then extrapolates the part's last row pair by an ulp.
            const int *pb = p.pbound + rowid * PB_STRIDE;
            const int lo = pb[part], hi = pb[part + 1];
            const VRange vr = part_vrange(part, g.nparts, g.rows_per_part, p.hm);
            const int y0max = min(yhi, p.hm) - 1;
#pragma unroll 2
            for (int i = lo + (int)threadIdx.x; i < hi; i += LTHREADS) {
                const uint32_t ra_ = rand_u_bits(key0, (uint32_t)i);
                const float u = (float)(ra_ >> 8) * (1.0f / 16777216.0f);
                const float v = fmaf((float)(rand_v_bits(ra_) >> 8) * (1.0f / 16777216.0f), vr.dv, vr.v0);
                const float y = ((2.f * v - 1.f + 1.f) * p.hm - 1.f) * 0.5f;
                const float x = ((2.f * u - 1.f + 1.f) * p.wm - 1.f) * 0.5f;
                const int y0 = min(max((int)floorf(y), ylo), y0max);
                if (S2D_LOSS_DBG & 2) tally(i, x * y + (float)y0); else
                tally(i, sample_part_padded(sm, wp, r0, x, y, (int)floorf(x), y0));
            }
        } else {
        // Parity mode (injected coordinates, any order): a part owns about half of the row's points (those whose upper tap row
        // falls in it).  Every point is tested; the owned ones are compacted per wave (ballot + LDS queue) and only full waves of
        // owned points pay for the four LDS taps and the histogram update.
            const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
            int *qi = hq_idx[wv];
            float *qy = hq_y[wv];
            int qn = 0;                                   // wave-uniform
            auto heavy = [&](int i, float y) {
                const float u = cr[2 * i];
                const float x = ((2.f * u - 1.f + 1.f) * p.wm - 1.f) * 0.5f;
                tally(i, sample_part(sm, p.hm, p.wm, r0, nr, x, y, (int)floorf(x), (int)floorf(y)));
            };
            const int iters = (p.n_over + LTHREADS - 1) / LTHREADS;      // uniform: the ballots need whole waves
            for (int k = 0; k < iters; ++k) {
                const int i = k * LTHREADS + threadIdx.x;
                const bool live = i < p.n_over;
                const int ic = live ? i : p.n_over - 1;
                const float v = cr[2 * ic + 1];
                const float y = ((2.f * v - 1.f + 1.f) * p.hm - 1.f) * 0.5f;
                const int y0 = (int)floorf(y);
                const bool own = live && y0 >= ylo && y0 < yhi;
                const unsigned long long m = __ballot(own);
                if (own) {
                    const int pos = qn + (int)__popcll(m & ((1ull << lane) - 1ull));
                    qi[pos] = i; qy[pos] = y;
                }
                qn += (int)__popcll(m);
                if (qn >= 64) {
                    heavy(qi[lane], qy[lane]);
                    const int rest = qn - 64;
                    int ti = 0; float ty = 0.f;
                    if (lane < rest) { ti = qi[64 + lane]; ty = qy[64 + lane]; }
                    if (lane < rest) { qi[lane] = ti; qy[lane] = ty; }
                    qn = rest;
                }
            }
            if (lane < qn) heavy(qi[lane], qy[lane]);
        }
        if (LEVEL == 0 && li < p.xcap) {
            // the extra uniform points (point_features.py:112): sample their logits now too, so that the later passes
            // of this row never touch the logit map again
            const float *cr2 = coord_rows(p, rowid, false);
            const uint32_t key1 = rand_key(p.seed, key_row(p, rowid) * 2 + 1);
            for (int i = threadIdx.x; i < p.n_rand; i += LTHREADS) {
                float u, v;
                if (cr2) { u = cr2[2 * i]; v = cr2[2 * i + 1]; }
                else {
                    const uint32_t ra_ = rand_u_bits(key1, (uint32_t)i);
                    u = (float)(ra_ >> 8) * (1.0f / 16777216.0f);
                    v = (float)(rand_v_bits(ra_) >> 8) * (1.0f / 16777216.0f);
                }
                const float y = ((2.f * v - 1.f + 1.f) * p.hm - 1.f) * 0.5f;
                const float x = ((2.f * u - 1.f + 1.f) * p.wm - 1.f) * 0.5f;
                const int y0 = (int)floorf(y);
                if (y0 >= ylo && y0 < yhi)
                    p.xbuf[(long)li * (p.n_over + p.n_rand) + p.n_over + i] =
                        padded ? sample_part_padded(sm, wp, r0, x, y, (int)floorf(x), y0) : sample_part(sm, p.hm, p.wm, r0, nr, x, y, (int)floorf(x), y0);
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < nb; i += LTHREADS)
            if (h[i]) atomicAdd(&p.hist[rowid * 2048 + i], h[i]);
    }
}

// levels 1 and 2 for the rows whose samples were kept: stream the stored logits (coalesced), no map, no RNG
template <int LEVEL>
__global__ __launch_bounds__(256) void hist_stream_kernel(LossParams p)
{
    __shared__ unsigned int h[1024];
    constexpr int SCH = 8;                                       // chunks per row
    const int nrows = min(p.lcount[p.NL], p.xcap);
    for (int w = blockIdx.x; w < nrows * SCH; w += gridDim.x) {
        const int li = w / SCH, chunk = w % SCH;
        const long rowid = p.list[li];
        __syncthreads();
        for (int i = threadIdx.x; i < 1024; i += 256) h[i] = 0u;
        __syncthreads();
        const unsigned int pre = p.prefix[rowid];
        const float *xb = p.xbuf + (long)li * (p.n_over + p.n_rand);
        const int per = ((p.n_over + SCH - 1) / SCH + 3) & ~3;
        const int i0 = chunk * per, i1 = min(p.n_over, i0 + per);
        for (int i = i0 + threadIdx.x * 4; i < i1; i += 256 * 4) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(xb + i);          // n_over % 4 == 0 checked on the host
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i + j >= i1) break;
                const unsigned int key = __float_as_uint(fabsf(v[j]));
                if (LEVEL == 1) { if ((key >> 20) == (pre >> 20)) atomicAdd(&h[(key >> 10) & 1023u], 1u); }
                else { if ((key >> 10) == (pre >> 10)) atomicAdd(&h[key & 1023u], 1u); }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 1024; i += 256)
            if (h[i]) atomicAdd(&p.hist[rowid * 2048 + i], h[i]);
    }
}

// bilinear sample of a bit-packed [H,W] plane held in LDS (bit = 1 -> 1.0f)
template <bool COH = false>
__device__ __forceinline__ float sample_bits(const unsigned int *bits, int H, int W, float u, float v)
{
    const float gx = 2.f * u - 1.f, gy = 2.f * v - 1.f;
    const float x = ((gx + 1.f) * W - 1.f) * 0.5f, y = ((gy + 1.f) * H - 1.f) * 0.5f;
    const int x0 = (int)floorf(x), y0 = (int)floorf(y), x1 = x0 + 1, y1 = y0 + 1;
    const float fx = x - x0, fy = y - y0;
    const float wxa = (x0 >= 0 && x0 < W) ? 1.f - fx : 0.f, wxb = (x1 >= 0 && x1 < W) ? fx : 0.f;
    const float wya = (y0 >= 0 && y0 < H) ? 1.f - fy : 0.f, wyb = (y1 >= 0 && y1 < H) ? fy : 0.f;
    const int xa = min(max(x0, 0), W - 1), xb = min(max(x1, 0), W - 1);
    const int ya = min(max(y0, 0), H - 1) * W, yb = min(max(y1, 0), H - 1) * W;
    // COH: the words were written to global memory by this workgroup a moment ago (backward: the plane does not fit LDS
    // next to the gradient tile) -> read them past the L1
    auto bit = [&](int idx) {
        const unsigned int w = COH ? __hip_atomic_load(bits + (idx >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : bits[idx >> 5];
        return (float)((w >> (idx & 31)) & 1u);
    };
    float acc = bit(ya + xa) * (wxa * wya);
    acc += bit(ya + xb) * (wxb * wya);
    acc += bit(yb + xa) * (wxa * wyb);
    acc += bit(yb + xb) * (wxb * wyb);
    return acc;
}

// find the bin holding the krem-th smallest key; one block per row
template <int LEVEL>
__global__ __launch_bounds__(256) void select_kernel(LossParams p)
{
    __shared__ unsigned int csum[256];
    if ((int)blockIdx.x >= p.lcount[p.NL]) return;
    const long rowid = p.list[blockIdx.x];
    const int nb = LEVEL == 0 ? 2048 : 1024, per = nb / 256;
    const int k = LEVEL == 0 ? p.n_unc : p.krem[rowid];
    unsigned int *h = p.hist + rowid * 2048;
    unsigned int loc[8], s = 0;
    for (int j = 0; j < per; ++j) { loc[j] = h[threadIdx.x * per + j]; s += loc[j]; }
    csum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int run = 0;
        for (int i = 0; i < 256; ++i) { const unsigned int c = csum[i]; csum[i] = run; run += c; }
    }
    __syncthreads();
    unsigned int before = csum[threadIdx.x];
    if (k == 0 && LEVEL == 0 && threadIdx.x == 0) { p.prefix[rowid] = 0u; p.krem[rowid] = 0; }   // importance ratio 0: nothing to select
    for (int j = 0; j < per; ++j) {
        if (before < (unsigned)k && before + loc[j] >= (unsigned)k) {
            const unsigned int bin = threadIdx.x * per + j;
            const unsigned int pre = LEVEL == 0 ? 0u : p.prefix[rowid];
            p.prefix[rowid] = LEVEL == 0 ? (bin << 20) : LEVEL == 1 ? (pre | (bin << 10)) : (pre | bin);
            p.krem[rowid] = k - (int)before;
            if (LEVEL == 2) p.tie[rowid] = loc[j];                 // a level-2 bin is one key: the number of points AT the threshold
        }
        before += loc[j];
    }
    __syncthreads();
    for (int j = 0; j < per; ++j) h[threadIdx.x * per + j] = 0u;  // ready for the next level
}

__device__ __forceinline__ void acc_point(float x, float t, float &bce, float &sgt, float &sg, float &ts)
{
    const float e = __expf(-fabsf(x));
    const float inv = __builtin_amdgcn_rcpf(1.f + e);
    const float s = x >= 0.f ? inv : e * inv;
    bce += fmaxf(x, 0.f) - x * t + __logf(1.f + e);   // F.binary_cross_entropy_with_logits (criterion.py:74)
    sgt += s * t; sg += s; ts += t;             // dice terms (criterion.py:37-41)
}

__global__ __launch_bounds__(LTHREADS) void accumulate_kernel(LossParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[LTHREADS / 64][4];
    const PartGeom g = part_geom(p.hm, p.wm);
    float *sm = smem;
    const int rows_l = p.B * p.maxm * p.T;
    PartIter it(p, g.nparts, p.xcap);
    long rowid; int part, li;
    while (it.next(p, rowid, part, li)) {
        __syncthreads();
        const int r0 = part * g.rows_per_part;
        const int nr = min(g.rows_per_part + 1, p.hm - r0);
        stage_part(p.mq + rowid * p.hm * p.wm, p.wm, r0, nr, sm);
        __syncthreads();
        const int layer = (int)(rowid / rows_l);
        const int r = (int)(rowid % rows_l);
        const int t = r % p.T, s = (r / p.T) % p.maxm, b = r / (p.T * p.maxm);
        const int prob = layer * p.B + b;
        const int n = p.idx_t[(long)prob * p.maxm + s];
        const uint8_t *pl = p.tgt + (((long)b * p.Nmax + n) * p.T + t) * p.H * p.W;
        const unsigned int thr = p.prefix[rowid];
        const unsigned int take = (unsigned int)p.krem[rowid];
        // points AT the threshold (select_kernel<2> counted them: take <= p.tie[rowid]): all of them are kept -- the usual row, whose only
        // such point is the threshold element itself -- or the `take` with the smallest point index, which no part of the row can tell on
        // its own: those are left out here and added by accumulate_ties_kernel
        const bool all_ties = take > 0u && take == p.tie[rowid];
        const int ylo = part == 0 ? -1 : r0, yhi = r0 + g.rows_per_part;
        float bce = 0.f, sgt = 0.f, sg = 0.f, ts = 0.f;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {          // pass 0: the 3P oversampled points, pass 1: the extra uniform points
            const bool over = pass == 0;
            const float *cr = coord_rows(p, rowid, over);
            const uint32_t key0 = rand_key(p.seed, key_row(p, rowid) * 2 + (over ? 0 : 1));
            // RNG mode, oversampled points: this part's own index range of the row (stratified generation), else every point + test
            const bool strat = over && !cr;
            const int *pb = p.pbound + rowid * PB_STRIDE;
            const int ibeg = strat ? pb[part] : 0, cnt = strat ? pb[part + 1] : (over ? p.n_over : p.n_rand);
            const VRange vr = part_vrange(part, g.nparts, g.rows_per_part, p.hm);
            const int y0max = min(yhi, p.hm) - 1;
            for (int i0 = ibeg + (int)threadIdx.x; i0 < cnt; i0 += 4 * LTHREADS) {
                float xv[4], uu[4], vv[4];
                bool own[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = i0 + j * LTHREADS;
                    const int ic = min(i, cnt - 1);
                    float u, v;
                    if (cr) { u = cr[2 * ic]; v = cr[2 * ic + 1]; }
                    else {
                        const uint32_t ra_ = rand_u_bits(key0, (uint32_t)ic);
                        u = (float)(ra_ >> 8) * (1.0f / 16777216.0f);
                        v = (float)(rand_v_bits(ra_) >> 8) * (1.0f / 16777216.0f);
                        if (strat) v = fmaf(v, vr.dv, vr.v0);
                    }
                    const float y = ((2.f * v - 1.f + 1.f) * p.hm - 1.f) * 0.5f;
                    const float x = ((2.f * u - 1.f + 1.f) * p.wm - 1.f) * 0.5f;
                    int y0 = (int)floorf(y);
                    if (strat) y0 = min(max(y0, ylo), y0max);
                    own[j] = i < cnt && y0 >= ylo && y0 < yhi;
                    xv[j] = sample_part(sm, p.hm, p.wm, r0, nr, x, y, (int)floorf(x), y0);
                    uu[j] = u; vv[j] = v;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bool sel = own[j];
                    if (over && sel) {
                        const unsigned int key = __float_as_uint(fabsf(xv[j]));
                        sel = key < thr || (all_ties && key == thr);
                    }
                    if (sel) acc_point(xv[j], sample_plane(pl, p.H, p.W, uu[j], vv[j]), bce, sgt, sg, ts);
                }
            }
        }
        bce = wave_sum(bce); sgt = wave_sum(sgt); sg = wave_sum(sg); ts = wave_sum(ts);
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        if (lane == 0) { red[wv][0] = bce; red[wv][1] = sgt; red[wv][2] = sg; red[wv][3] = ts; }
        __syncthreads();
        if (threadIdx.x < 4) {
            const int j = threadIdx.x;
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < LTHREADS / 64; ++w) tot += red[w][j];
            p.part[(rowid * p.chunks + part) * 4 + j] = tot;
        }
    }
}

// bilinear sample of a row's [hm,wm] map in global memory at (x, y) with the tap corner (x0, y0) given: the products and the order of
// additions of sample_part / sample_part_padded (a tap outside the map contributes a zero), so |result| has the bits the select saw
__device__ __forceinline__ float sample_map_at(const float *__restrict__ map, int hm, int wm, float x, float y, int x0, int y0)
{
    const int x1 = x0 + 1, y1 = y0 + 1;
    const float fx = x - x0, fy = y - y0;
    const bool xa_in = x0 >= 0 && x0 < wm, xb_in = x1 >= 0 && x1 < wm, ya_in = y0 >= 0 && y0 < hm, yb_in = y1 >= 0 && y1 < hm;
    const int xa = min(max(x0, 0), wm - 1), xb = min(max(x1, 0), wm - 1);
    const int ya = min(max(y0, 0), hm - 1) * wm, yb = min(max(y1, 0), hm - 1) * wm;
    float acc = (xa_in && ya_in ? map[ya + xa] : 0.f) * ((1.f - fx) * (1.f - fy));
    acc += (xb_in && ya_in ? map[ya + xb] : 0.f) * (fx * (1.f - fy));
    acc += (xa_in && yb_in ? map[yb + xa] : 0.f) * ((1.f - fx) * fy);
    acc += (xb_in && yb_in ? map[yb + xb] : 0.f) * (fx * fy);
    return acc;
}

// The tie rule for the rows accumulate_kernel handles (samples not kept): of the points whose |logit| EQUALS the threshold, the `take`
// with the smallest point index over the whole row are kept -- the streamed kernel's rule, whatever the map part a point lies in and
// however the workgroups are scheduled.  One workgroup per such row that has more ties than it takes (a row of a smooth map has one,
// the threshold element, and is skipped): the oversampled points are walked in index order, 512 at a time, re-sampled from the row's
// map in global memory, ranked among the ties by a block scan (as accumulate_stream_kernel's scan path), and the first `take` are
// evaluated; the walk ends with the take-th tie.  The sums go on top of the row's part-0 slot: this kernel runs after
// accumulate_kernel, one thread per slot entry, so the order of the additions is fixed.
__global__ __launch_bounds__(LTHREADS) void accumulate_ties_kernel(LossParams p)
{
    __shared__ float red[LTHREADS / 64][4];
    __shared__ unsigned int wtie[LTHREADS / 64], tie_base;
    __shared__ float s_v0[PB_STRIDE], s_dv[PB_STRIDE];
    const int nrows = p.lcount[p.NL];
    if (p.xcap + (int)blockIdx.x >= nrows) return;                   // the launch is decided on the padded row count: usually no row is left
    const PartGeom g = part_geom(p.hm, p.wm);
    if ((int)threadIdx.x < g.nparts) { const VRange vr = part_vrange(threadIdx.x, g.nparts, g.rows_per_part, p.hm); s_v0[threadIdx.x] = vr.v0; s_dv[threadIdx.x] = vr.dv; }
    const int rows_l = p.B * p.maxm * p.T;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int li = p.xcap + (int)blockIdx.x; li < nrows; li += gridDim.x) {
        const long rowid = p.list[li];
        const unsigned int thr = p.prefix[rowid];
        const unsigned int take = (unsigned int)p.krem[rowid];
        if (take == 0u || take >= p.tie[rowid]) continue;            // uniform over the workgroup: accumulate_kernel kept every tie
        __syncthreads();
        if (threadIdx.x == 0) tie_base = 0u;
        __syncthreads();
        const int r = (int)(rowid % rows_l);
        const int t = r % p.T, s = (r / p.T) % p.maxm, b = r / (p.T * p.maxm);
        const int prob = (int)(rowid / rows_l) * p.B + b;
        const int n = p.idx_t[(long)prob * p.maxm + s];
        const uint8_t *pl = p.tgt + (((long)b * p.Nmax + n) * p.T + t) * p.H * p.W;
        const float *map = p.mq + rowid * p.hm * p.wm;
        const float *cr = coord_rows(p, rowid, true);
        const uint32_t key0 = rand_key(p.seed, key_row(p, rowid) * 2);
        const int *pb = p.pbound + rowid * PB_STRIDE;
        float bce = 0.f, sgt = 0.f, sg = 0.f, ts = 0.f;
        for (int i0 = 0; i0 < p.n_over; i0 += LTHREADS) {
            const int i = i0 + (int)threadIdx.x;
            float u = 0.f, v = 0.f, xv = 0.f;
            bool istie = false;
            if (i < p.n_over) {
                int ylo = INT_MIN, y0max = INT_MAX;                 // generator mode: floor(y) is clamped into the point's own part, as the select did
                if (cr) { u = cr[2 * i]; v = cr[2 * i + 1]; }
                else {
                    int j = 0;
                    while (j + 1 < g.nparts && i >= pb[j + 1]) ++j;
                    over_point_rng(key0, i, pb, s_v0, s_dv, g.nparts, u, v);
                    ylo = j == 0 ? -1 : j * g.rows_per_part;
                    y0max = min((j + 1) * g.rows_per_part, p.hm) - 1;
                }
                const float y = ((2.f * v - 1.f + 1.f) * p.hm - 1.f) * 0.5f;
                const float x = ((2.f * u - 1.f + 1.f) * p.wm - 1.f) * 0.5f;
                xv = sample_map_at(map, p.hm, p.wm, x, y, (int)floorf(x), min(max((int)floorf(y), ylo), y0max));
                istie = __float_as_uint(fabsf(xv)) == thr;
            }
            const unsigned long long bal = __ballot(istie);
            if (lane == 0) wtie[wv] = (unsigned int)__popcll(bal);
            __syncthreads();
            unsigned int rank = tie_base + (unsigned int)__popcll(bal & ((1ull << lane) - 1ull));
            for (int w = 0; w < wv; ++w) rank += wtie[w];
            if (istie && rank < take) acc_point(xv, sample_plane(pl, p.H, p.W, u, v), bce, sgt, sg, ts);
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned int tot = 0u;
                for (int w = 0; w < LTHREADS / 64; ++w) tot += wtie[w];
                tie_base += tot;
            }
            __syncthreads();
            if (tie_base >= take) break;                             // uniform: read after the barrier, written again only after the next two
        }
        bce = wave_sum(bce); sgt = wave_sum(sgt); sg = wave_sum(sg); ts = wave_sum(ts);
        if (lane == 0) { red[wv][0] = bce; red[wv][1] = sgt; red[wv][2] = sg; red[wv][3] = ts; }
        __syncthreads();
        if (threadIdx.x < 4) {
            const int j = threadIdx.x;
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < LTHREADS / 64; ++w) tot += red[w][j];
            p.part[(rowid * p.chunks + 0) * 4 + j] += tot;
        }
    }
}

// every target plane of the pass (clip b, target n < count[b], frame t) as bits, once: one thread = 32 pixels = one word
__global__ __launch_bounds__(256) void pack_planes_kernel(LossParams p)
{
    const long HW = (long)p.H * p.W, wpp = HW / 32;
    const int plane = blockIdx.y;                              // (b * Nmax + n) * T + t
    const int n = (plane / p.T) % p.Nmax, b = plane / (p.T * p.Nmax);
    if (n >= min(p.tgt_count[b], p.Nmax)) return;
    const long wd = (long)blockIdx.x * 256 + threadIdx.x;
    if (wd >= wpp) return;
    const uint8_t *pl = p.tgt + (long)plane * HW;
    const uint4 a = reinterpret_cast<const uint4 *>(pl)[wd * 2], c = reinterpret_cast<const uint4 *>(pl)[wd * 2 + 1];
    const unsigned int ws[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
    unsigned int out = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned int w4 = ws[k];
        out |= ((w4 & 0xFFu) ? 1u : 0u) << (4 * k);
        out |= ((w4 & 0xFF00u) ? 1u : 0u) << (4 * k + 1);
        out |= ((w4 & 0xFF0000u) ? 1u : 0u) << (4 * k + 2);
        out |= ((w4 & 0xFF000000u) ? 1u : 0u) << (4 * k + 3);
    }
    p.tpack[(long)plane * wpp + wd] = out;
}

// accumulate for rows with stored samples: item = row.  The row's whole target plane is bit-packed into LDS
// (H*W/8 bytes: 118 KB at 736x1280), the stored logits are streamed, only (u,v) is regenerated for the target taps.
// BWD = true: the same walk over the same selected points (same threshold, same tie rule), but instead of summing the loss
// terms every point scatters d(loss)/d(logit at the point) through the bilinear taps of its sample position.  The row's
// gradient plane (235 KB at 184 x 320) is built in LDS one half (top / bottom rows) at a time with LDS float atomics -- the
// points are walked once per half, each tap lands in exactly one half -- and written out with plain stores; the bit-packed
// target plane lives in a per-workgroup global scratch meanwhile (global float atomics took 37 ms per pass, this 1/5).
struct LossBwdArgs {
    float *gplane;            // [rows][hm*wm], zero-initialised
    float w_mask, w_dice;     // loss weights (weight_dict) of loss_mask / loss_dice
    unsigned int *bit_scratch; // unused since the planes are packed once per pass (LossParams::tpack); kept for the entry point's signature
};
// GBITS: the row's bit-packed target plane is read in place from the pass's packed planes (backward: LDS holds the gradient tile;
// forward: frames beyond 1.15 M pixels) instead of from a copy in the dynamic LDS
template <bool BWD, bool GBITS = BWD>
__global__ __launch_bounds__(LTHREADS) void accumulate_stream_kernel(LossParams p, LossBwdArgs ba)
{
    extern __shared__ __attribute__((aligned(16))) unsigned int tbits[];
    __shared__ float red[LTHREADS / 64][4];
    // Points whose |logit| equals the top-k threshold exactly: the `take` of them with the smallest point index are kept
    // (a fixed rule, so the loss is bitwise reproducible whatever else shares the GPU).  They are parked in a small
    // list, ranked by index and evaluated by thread = rank; a row with more ties than the list holds (a constant logit
    // map) takes the block-scan path below.
    constexpr int TIECAP = 512;
    __shared__ unsigned int tie_n, tie_base, wtie[LTHREADS / 64];
    __shared__ int tie_idx[TIECAP], tie_sorted[TIECAP];
    __shared__ int cq_idx[LTHREADS / 64][128];
    __shared__ float cq_val[LTHREADS / 64][128];
    const int rows_l = p.B * p.maxm * p.T;
    const int nrows = min(p.lcount[p.NL], p.xcap);
    const long HW = (long)p.H * p.W;
    __shared__ float s_v0[PB_STRIDE], s_dv[PB_STRIDE];           // RNG mode: v bands of the map parts, strata bounds of the row
    __shared__ int s_pb[PB_STRIDE];
    const PartGeom sg_ = part_geom(p.hm, p.wm);
    if ((int)threadIdx.x < sg_.nparts) { const VRange vr = part_vrange(threadIdx.x, sg_.nparts, sg_.rows_per_part, p.hm); s_v0[threadIdx.x] = vr.v0; s_dv[threadIdx.x] = vr.dv; }
    static_assert(GBITS || !BWD, "the backward keeps its gradient tile in the dynamic LDS");
    const unsigned int *tb = tbits;                           // GBITS: the row's words in p.tpack (set per row below)
    // BWD: the dynamic LDS is the gradient tile [hh][wm], accumulated in FIXED POINT (int32, LDS integer atomics): integer sums
    // do not depend on the order the points arrive in, so the gradient is bitwise reproducible -- float atomics made it the last
    // gradient of the training step that was not.  Scale per row: a power of two such that FX_CAP tap weights of the largest
    // possible per-point gradient fit 31 bits (a pixel collects ~11 taps on average at the shipped point counts, a few dozen in
    // the densest importance-sampled spots); one contribution is then rounded to <= 2^-21 of that bound.
    // The tile is one MAP PART of the forward's geometry (part_geom: rows [j rpp, (j + 1) rpp)) plus one row above and two below:
    // a part owns the points whose upper tap row y0 lies in it, so both tap rows of an owned point are inside the tile -- also for a
    // point the RNG mode generated for this part whose v sits on the band edge and whose y0 rounds one row out of it.  In RNG mode the
    // oversampled points of a part are an INDEX RANGE of the row (row_strata_kernel), so the part walks only that range; the random
    // points (and, with injected coordinates, all points) are tested for ownership before they are queued.  Every point is
    // evaluated once per row -- the first version cut the map in two halves and evaluated every point in both -- and any map size
    // fits ((rpp + 3) wm ints <= PART_BYTES by part_geom).  The up-to-three rows two consecutive tiles share are carried over as
    // integers, so a pixel's sum is still one integer sum over all its taps.
    int *gh = reinterpret_cast<int *>(tbits);
    // FX_CAP = the number of unit tap weights a pixel may collect without its int32 sum wrapping.  A point adds at most weight 1 to a
    // pixel, so n_unc + n_rand is a PROVABLE cap; 1024 is the density argument above and holds only for generator-drawn (i.i.d. uniform)
    // points on maps much larger than the point density: with injected coordinates (any clustering / duplicates) and on small maps
    // (expected taps per pixel x 64 > 1024) the provable cap is used instead -- ~3.6 bits coarser at 12 544 points, still <= 2^-17 of
    // the bound per contribution.
    const float n_pts = (float)(p.n_unc + p.n_rand);
    const bool injected = p.coords_over != nullptr || p.coords_rand != nullptr;
    const float FX_CAP = injected ? fmaxf(n_pts, 1.f) : fminf(fmaxf(n_pts, 1.f), fmaxf(1024.f, 256.f * n_pts / (float)(p.hm * p.wm)));
    __shared__ unsigned int tie_before;                      // ties with a smaller point index than the current part's (earlier parts)
    for (int li = blockIdx.x; li < nrows; li += gridDim.x) {
        const long rowid = p.list[li];
        const int layer = (int)(rowid / rows_l);
        const int r = (int)(rowid % rows_l);
        const int t = r % p.T, s = (r / p.T) % p.maxm, b = r / (p.T * p.maxm);
        const int prob = layer * p.B + b;
        const int n = p.idx_t[(long)prob * p.maxm + s];
        // the row's target plane as bits: packed once per criterion pass for every (clip, target, frame) by pack_planes_kernel -- each
        // plane is the target of up to NL rows -- and copied to LDS here (H * W / 8 bytes instead of H * W read per row), or read in place
        const unsigned int *pk = p.tpack + (((long)b * p.Nmax + n) * p.T + t) * (HW / 32);
        __syncthreads();
        if (threadIdx.x < PB_STRIDE) s_pb[threadIdx.x] = p.pbound[rowid * PB_STRIDE + threadIdx.x];   // visible after the barrier below
        if constexpr (GBITS) tb = pk;
        else {
#pragma unroll 4
            for (long w4 = threadIdx.x; w4 < HW / 128; w4 += LTHREADS) reinterpret_cast<uint4 *>(tbits)[w4] = reinterpret_cast<const uint4 *>(pk)[w4];
            for (long wd = (HW / 128) * 4 + threadIdx.x; wd < HW / 32; wd += LTHREADS) tbits[wd] = pk[wd];
        }
        if (threadIdx.x == 0) { tie_n = 0u; tie_base = 0u; }
        __syncthreads();
        const unsigned int thr = p.prefix[rowid];
        const unsigned int take = (unsigned int)p.krem[rowid];
        const float *xb = p.xbuf + (long)li * (p.n_over + p.n_rand);
        float bce = 0.f, sgt = 0.f, sg = 0.f, ts = 0.f;
        // backward: per-row constants of d(w_mask * loss_mask + w_dice * loss_dice) / d(logit at a point)
        float g_bce = 0.f, g_dice = 0.f, dA = 0.f, dD = 1.f, fx_scale = 0.f, fx_inv = 0.f;
        float *gp = nullptr;
        if constexpr (BWD) {
            double num = 0.;
            for (int bb = 0; bb < p.B; ++bb) num += (double)min(p.tgt_count[bb], p.Nmax);
            num = fmax(num / (double)p.world_size, 1.0);
            float a = 0.f, bsum = 0.f, c = 0.f;
            for (int ch = 0; ch < p.chunks; ++ch) {
                const float *qd = p.part + (rowid * p.chunks + ch) * 4;
                a += qd[1]; bsum += qd[2]; c += qd[3];
            }
            dA = 2.f * a + 1.f; dD = bsum + c + 1.f;
            g_bce = ba.w_mask / ((float)num * (float)(p.n_unc + p.n_rand));
            g_dice = ba.w_dice / (float)num;
            gp = ba.gplane + rowid * (long)p.hm * p.wm;
            // |g| <= |g_bce| |sigma - t| + |g_dice| |2 t D - A| / D^2 sigma (1 - sigma) <= |g_bce| + |g_dice| (2 D + |A|) / (4 D^2)
            const float gmax = fabsf(g_bce) + fabsf(g_dice) * (2.f * dD + fabsf(dA)) / (4.f * dD * dD);
            fx_scale = gmax > 0.f ? exp2f(floorf(log2f(2147483648.f / (FX_CAP * gmax)))) : 0.f;
            fx_inv = fx_scale > 0.f ? 1.f / fx_scale : 0.f;
        }
        int ylo = 0, yhi = p.hm;                              // BWD: the rows [ylo, yhi) of the gradient tile being built
        int own_lo = -1, own_hi = p.hm;                       // ... and the y0 range of the points the current part owns
        auto y0_of = [&](float v) { return (int)floorf((((2.f * v - 1.f) + 1.f) * p.hm - 1.f) * 0.5f); };   // as point() forms it
        auto point = [&](float xv, float tt, float u, float v) {
            if constexpr (!BWD) {
                acc_point(xv, tt, bce, sgt, sg, ts);
            } else {
                const float e = __expf(-fabsf(xv));
                const float inv = 1.f / (1.f + e);
                const float sgm = xv >= 0.f ? inv : e * inv;
                // d bce / dx = sigma - t;  d dice / d sigma = -(2 t D - A) / D^2,  d sigma / dx = sigma (1 - sigma)
                const float g = g_bce * (sgm - tt) - g_dice * ((2.f * tt * dD - dA) / (dD * dD)) * sgm * (1.f - sgm);
                const float gx = 2.f * u - 1.f, gy = 2.f * v - 1.f;                      // point_sample of the logit row
                const float x = ((gx + 1.f) * p.wm - 1.f) * 0.5f, y = ((gy + 1.f) * p.hm - 1.f) * 0.5f;
                const int x0 = (int)floorf(x), y0 = (int)floorf(y), x1 = x0 + 1, y1 = y0 + 1;
                const float fx = x - x0, fy = y - y0;
                const float gs = g * fx_scale;
                if (y0 >= ylo && y0 < yhi) {                   // rows outside [0, hm) are outside every tile
                    if (x0 >= 0 && x0 < p.wm) atomicAdd(gh + (y0 - ylo) * p.wm + x0, __float2int_rn(gs * (1.f - fx) * (1.f - fy)));
                    if (x1 >= 0 && x1 < p.wm) atomicAdd(gh + (y0 - ylo) * p.wm + x1, __float2int_rn(gs * fx * (1.f - fy)));
                }
                if (y1 >= ylo && y1 < yhi) {
                    if (x0 >= 0 && x0 < p.wm) atomicAdd(gh + (y1 - ylo) * p.wm + x0, __float2int_rn(gs * (1.f - fx) * fy));
                    if (x1 >= 0 && x1 < p.wm) atomicAdd(gh + (y1 - ylo) * p.wm + x1, __float2int_rn(gs * fx * fy));
                }
            }
        };
        const int nparts_b = BWD ? sg_.nparts : 1;
        if (BWD && threadIdx.x == 0) tie_before = 0u;
#pragma unroll 1
        for (int part = 0; part < nparts_b; ++part) {
        int r_lo = 0, r_hi = 0;                               // RNG mode, BWD: the part's index range of the oversampled points
        bool ranged = false;
        if constexpr (BWD) {
            const int rpp = sg_.rows_per_part;
            const int nlo = max(part * rpp - 1, 0), nhi = min((part + 1) * rpp + 2, p.hm);
            // rows [nlo, yhi) of the previous tile are this tile's first rows: carry their integer sums over
            __syncthreads();
            const int ncarry = part > 0 ? max(yhi - nlo, 0) * p.wm : 0;
            constexpr int CARRY = 4;                            // <= 3 rows x wm ints over LTHREADS threads (wm <= 4 * 512 / 3)
            int keep[CARRY];
#pragma unroll
            for (int c = 0; c < CARRY; ++c) {
                const int i = threadIdx.x + c * LTHREADS;
                keep[c] = i < ncarry ? gh[(nlo - ylo) * p.wm + i] : 0;
            }
            __syncthreads();
            ylo = nlo; yhi = nhi;
            own_lo = part == 0 ? -1 : part * rpp; own_hi = part == nparts_b - 1 ? p.hm : (part + 1) * rpp;
            for (int i = threadIdx.x; i < (yhi - ylo) * p.wm; i += LTHREADS) gh[i] = 0;
            if (threadIdx.x == 0) { tie_n = 0u; tie_base = 0u; }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < CARRY; ++c) {
                const int i = threadIdx.x + c * LTHREADS;
                if (i < ncarry) gh[i] = keep[c];
            }
            __syncthreads();
            ranged = coord_rows(p, rowid, true) == nullptr;
            r_lo = s_pb[part]; r_hi = s_pb[part + 1];
        }
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            const bool over = pass == 0;
            const float *cr = coord_rows(p, rowid, over);
            const uint32_t key0 = rand_key(p.seed, key_row(p, rowid) * 2 + (over ? 0 : 1));
            const int cnt = over ? p.n_over : p.n_rand;
            const float *xs = xb + (over ? 0 : p.n_over);
            const bool walk_range = BWD && over && ranged;    // only the part's own index range; its points need no ownership test
            const int lo = walk_range ? r_lo : 0, hi = walk_range ? r_hi : cnt;
            auto heavy = [&](int i, float xv) {           // one selected point: regenerate (u,v), sample the target bits
                float u, v;
                if (cr) { u = cr[2 * i]; v = cr[2 * i + 1]; }
                else if (over) over_point_rng(key0, i, s_pb, s_v0, s_dv, sg_.nparts, u, v);
                else {
                    const uint32_t ra_ = rand_u_bits(key0, (uint32_t)i);
                    u = (float)(ra_ >> 8) * (1.0f / 16777216.0f);
                    v = (float)(rand_v_bits(ra_) >> 8) * (1.0f / 16777216.0f);
                }
                point(xv, sample_bits(tb, p.H, p.W, u, v), u, v);
            };
            // Only ~1 in 4 oversampled points passes the threshold, scattered over the lanes: evaluating them in place
            // would run the heavy path at 25 % lane utilisation.  Each wave instead compacts its selected points (ballot
            // + prefix count) into a small LDS queue and evaluates a full wave of 64 whenever one is ready; the order is
            // a function of the point indices only, so the sums stay reproducible.
            const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
            int *qi = cq_idx[wv];
            float *qx = cq_val[wv];
            int qn = 0;                                   // wave-uniform
            auto push = [&](bool sel, int i, float xv) {
                const unsigned long long m = __ballot(sel);
                if (sel) {
                    const int pos = qn + (int)__popcll(m & ((1ull << lane) - 1ull));
                    qi[pos] = i; qx[pos] = xv;
                }
                qn += (int)__popcll(m);
                if (qn >= 64) {
                    heavy(qi[lane], qx[lane]);
                    const int rest = qn - 64;             // < 64
                    int ti = 0; float tx = 0.f;
                    if (lane < rest) { ti = qi[64 + lane]; tx = qx[64 + lane]; }
                    if (lane < rest) { qi[lane] = ti; qx[lane] = tx; }
                    qn = rest;
                }
            };
            auto test = [&](int i, float xv, bool live) {
                const bool inr = live && i >= lo && i < hi;
                bool owned = inr;
                if (BWD && !walk_range && inr) {              // ownership by the upper tap row, before the point is queued
                    float v;
                    if (cr) v = cr[2 * i + 1];
                    else if (over) { float u; over_point_rng(key0, i, s_pb, s_v0, s_dv, sg_.nparts, u, v); }
                    else v = (float)(rand_v_bits(rand_u_bits(key0, (uint32_t)i)) >> 8) * (1.0f / 16777216.0f);
                    const int y0 = y0_of(v);
                    owned = y0 >= own_lo && y0 < own_hi;
                }
                bool sel = owned;
                if (over) {
                    const unsigned int key = __float_as_uint(fabsf(xv));
                    sel = owned && key < thr;
                    if (inr && key == thr) {                  // every tie of the walked range is listed (ranks are by index); tie_point tests ownership
                        const unsigned int slot = atomicAdd(&tie_n, 1u);
                        if (slot < TIECAP) tie_idx[slot] = i;
                    }
                }
                push(sel, i, xv);
            };
            // the stored logits are streamed 16 B per lane (4 consecutive points), two loads in flight: with one
            // workgroup per CU the loop is bound by the round trip of each load, not by bandwidth
            const int cnt4 = ((reinterpret_cast<uintptr_t>(xs) & 15) == 0) ? cnt >> 2 : 0;
            const int b4 = min(lo >> 2, cnt4), e4 = min((hi + 3) >> 2, cnt4);    // the 4-point groups that overlap [lo, hi)
            const int it4 = (e4 - b4 + LTHREADS - 1) / LTHREADS;      // uniform trip counts: ballots need whole waves
            auto load4 = [&](int k) {
                const int i4 = b4 + k * LTHREADS + threadIdx.x;
                f32x4 x4 = {0.f, 0.f, 0.f, 0.f};
                if (i4 < e4) x4 = *reinterpret_cast<const f32x4 *>(xs + 4 * i4);
                return x4;
            };
            // DEPTH loads ahead of the consumer (a ring in registers, the loop unrolled over it): one workgroup per CU streams its
            // row at the latency x depth product -- with two loads in flight the pass ran at ~8 GB/s per CU
            constexpr int DEPTH = 8;
            f32x4 ring[DEPTH];
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) ring[d] = load4(d);
            for (int k0 = 0; k0 < it4; k0 += DEPTH) {
#pragma unroll
                for (int d = 0; d < DEPTH; ++d) {
                    const int k = k0 + d;
                    if (k >= it4) break;                           // uniform over the workgroup
                    const int i4 = b4 + k * LTHREADS + threadIdx.x;
                    const bool live = i4 < e4;
                    const f32x4 x4 = ring[d];
                    ring[d] = load4(k + DEPTH);
#pragma unroll
                    for (int j = 0; j < 4; ++j) test(4 * i4 + j, x4[j], live);
                }
            }
            const int tail0 = 4 * cnt4, itt = (cnt - tail0 + LTHREADS - 1) / LTHREADS;
            for (int k = 0; k < itt; ++k) {
                const int i = tail0 + k * LTHREADS + threadIdx.x;
                const bool live = i < cnt;
                test(i, live ? xs[i] : 0.f, live);
            }
            if (lane < qn) heavy(qi[lane], qx[lane]);     // drain
        }
        __syncthreads();
        const unsigned int nties = tie_n;
        // ties are kept by ascending point index over the whole row; a part that walked only its own index range holds the ties of
        // that range, and the earlier parts' ranges lie below it: `before` of the row's first `take` ties are already spent
        const bool ranged_ties = BWD && ranged;
        const unsigned int before = ranged_ties ? tie_before : 0u;
        __syncthreads();
        if (ranged_ties && threadIdx.x == 0) tie_before = before + nties;
        if (nties > 0u && take > before) {                    // uniform over the workgroup
            const float *cr = coord_rows(p, rowid, true);
            const uint32_t key0 = rand_key(p.seed, key_row(p, rowid) * 2);
            auto tie_point = [&](int i) {
                float u, v;
                if (cr) { u = cr[2 * i]; v = cr[2 * i + 1]; }
                else over_point_rng(key0, i, s_pb, s_v0, s_dv, sg_.nparts, u, v);
                if (BWD && !ranged_ties) { const int y0 = y0_of(v); if (y0 < own_lo || y0 >= own_hi) return; }
                point(xb[i], sample_bits(tb, p.H, p.W, u, v), u, v);
            };
            if (nties <= (unsigned int)TIECAP) {
                for (unsigned int j = threadIdx.x; j < nties; j += LTHREADS) {
                    const int mine = tie_idx[j];
                    unsigned int rank = 0u;
                    for (unsigned int k2 = 0; k2 < nties; ++k2) rank += tie_idx[k2] < mine ? 1u : 0u;
                    tie_sorted[rank] = mine;
                }
                __syncthreads();
                for (unsigned int j = threadIdx.x; j < min(nties, take - before); j += LTHREADS) tie_point(tie_sorted[j]);
            } else {
                const int lane_ = threadIdx.x & 63, wv_ = threadIdx.x >> 6;
                const int t_lo = ranged_ties ? r_lo : 0, t_hi = ranged_ties ? r_hi : p.n_over;
                for (int i0 = t_lo; i0 < t_hi; i0 += LTHREADS) {
                    const int i = i0 + threadIdx.x;
                    const bool istie = i < t_hi && __float_as_uint(fabsf(xb[i])) == thr;
                    const unsigned long long bal = __ballot(istie);
                    if (lane_ == 0) wtie[wv_] = (unsigned int)__popcll(bal);
                    __syncthreads();
                    unsigned int rank = before + tie_base + (unsigned int)__popcll(bal & ((1ull << lane_) - 1ull));
                    for (int w = 0; w < wv_; ++w) rank += wtie[w];
                    if (istie && rank < take) tie_point(i);
                    __syncthreads();
                    if (threadIdx.x == 0) {
                        unsigned int tot = 0u;
                        for (int w = 0; w < LTHREADS / 64; ++w) tot += wtie[w];
                        tie_base += tot;
                    }
                    __syncthreads();
                }
            }
        }
        if constexpr (BWD) {                                  // write the rows of the tile that no later tile adds to
            __syncthreads();
            const int nxt = part + 1 < nparts_b ? max((part + 1) * sg_.rows_per_part - 1, 0) : p.hm;
            for (int i = threadIdx.x; i < (min(nxt, yhi) - ylo) * p.wm; i += LTHREADS) gp[ylo * p.wm + i] = (float)gh[i] * fx_inv;
        }
        }   // part
        if constexpr (!BWD) {
            bce = wave_sum(bce); sgt = wave_sum(sgt); sg = wave_sum(sg); ts = wave_sum(ts);
            const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
            if (lane == 0) { red[wv][0] = bce; red[wv][1] = sgt; red[wv][2] = sg; red[wv][3] = ts; }
            __syncthreads();
            if (threadIdx.x < 4) {
                const int j = threadIdx.x;
                float tot = 0.f;
#pragma unroll
                for (int w = 0; w < LTHREADS / 64; ++w) tot += red[w][j];
                p.part[(rowid * p.chunks + 0) * 4 + j] = tot;
#pragma unroll 1
                for (int c = 1; c < p.chunks; ++c) p.part[(rowid * p.chunks + c) * 4 + j] = 0.f;
            }
        }
    }
}

// losses[layer][0] = loss_mask, [1] = loss_dice  (criterion.py:349-352; normaliser = num_masks :404-409)
__global__ void loss_finalize_kernel(LossParams p, float *__restrict__ losses)
{
    const int layer = blockIdx.x;
    if (threadIdx.x != 0) return;
    const int rows_l = p.B * p.maxm * p.T;
    double num = 0.;
    for (int b = 0; b < p.B; ++b) num += (double)min(p.tgt_count[b], p.Nmax);
    num = fmax(num / (double)p.world_size, 1.0);
    const double P = (double)(p.n_unc + p.n_rand);
    double lm = 0., ld = 0.;
    for (int r = 0; r < rows_l; ++r) {
        const long rowid = (long)layer * rows_l + r;
        if (!p.active[rowid]) continue;
        double bce = 0., sgt = 0., sg = 0., ts = 0.;
        for (int c = 0; c < p.chunks; ++c) {
            const float *q = p.part + (rowid * p.chunks + c) * 4;
            bce += q[0]; sgt += q[1]; sg += q[2]; ts += q[3];
        }
        lm += bce / P;
        ld += 1.0 - (2.0 * sgt + 1.0) / (sg + ts + 1.0);
    }
    losses[layer * 2 + 0] = (float)(lm / num);
    losses[layer * 2 + 1] = (float)(ld / num);
}

// loss_labels (criterion.py:227-251): weighted CE, matched queries -> class 0, others -> class 1 (= no object)
__global__ void class_loss_kernel(const float *__restrict__ cls, const int *__restrict__ idx_q, const int *__restrict__ n_match,
                                  int B, int Q, int maxm, float eos, float *__restrict__ out)
{
    __shared__ unsigned char matched[128];
    __shared__ double wnum[16], wden[16];
    double num = 0., den = 0.;
    for (int b = 0; b < B; ++b) {
        __syncthreads();
        if (threadIdx.x < 128) matched[threadIdx.x] = 0;
        __syncthreads();
        if (threadIdx.x < n_match[b]) matched[idx_q[(long)b * maxm + threadIdx.x]] = 1;
        __syncthreads();
        const int q = threadIdx.x;
        if (q < Q) {
            const float l0 = cls[((long)b * Q + q) * 2], l1 = cls[((long)b * Q + q) * 2 + 1];
            const float mx = fmaxf(l0, l1);
            const float lse = mx + logf(expf(l0 - mx) + expf(l1 - mx));
            const bool m = matched[q];
            const float w = m ? 1.f : eos;
            num += (double)(w * (lse - (m ? l0 : l1)));
            den += (double)w;
        }
    }
    num = wave_sum_d(num); den = wave_sum_d(den);
    if ((threadIdx.x & 63) == 0) { wnum[threadIdx.x >> 6] = num; wden[threadIdx.x >> 6] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sn = 0., sd = 0.;
        for (unsigned int w = 0; w < (blockDim.x + 63) / 64; ++w) { sn += wnum[w]; sd += wden[w]; }   // fixed order
        out[0] = (float)(sn / sd);
    }
}

// d(w_ce * loss_labels)/d(class logits): w_i (softmax_i - onehot_i) / sum_j w_j  (criterion.py:227-251 differentiated)
__global__ void class_loss_backward_kernel(const float *__restrict__ cls, const int *__restrict__ idx_q, const int *__restrict__ n_match,
                                           int B, int Q, int maxm, float eos, float w_ce, float *__restrict__ dcls)
{
    __shared__ unsigned char matched[128];
    __shared__ float wsum;
    double den = 0.;
    if (threadIdx.x == 0) {
        for (int b = 0; b < B; ++b) den += (double)n_match[b] + (double)eos * (Q - n_match[b]);
        wsum = (float)den;
    }
    for (int b = 0; b < B; ++b) {
        __syncthreads();
        if (threadIdx.x < 128) matched[threadIdx.x] = 0;
        __syncthreads();
        if (threadIdx.x < n_match[b]) matched[idx_q[(long)b * maxm + threadIdx.x]] = 1;
        __syncthreads();
        const int q = threadIdx.x;
        if (q < Q) {
            const float l0 = cls[((long)b * Q + q) * 2], l1 = cls[((long)b * Q + q) * 2 + 1];
            const float mx = fmaxf(l0, l1);
            const float e0 = expf(l0 - mx), e1 = expf(l1 - mx);
            const float p0 = e0 / (e0 + e1), p1 = e1 / (e0 + e1);
            const bool m = matched[q];
            const float w = (m ? 1.f : eos) * w_ce / wsum;
            dcls[((long)b * Q + q) * 2] = w * (p0 - (m ? 1.f : 0.f));
            dcls[((long)b * Q + q) * 2 + 1] = w * (p1 - (m ? 0.f : 1.f));
        }
    }
}

// class_loss_kernel over C1 logits per query: matched -> class 0, others -> class C1 - 1 (= no object; criterion.py:227-251 with the
// target labels zeroed).  Same per-query expression tree (max, then sum of exp in class order) and the same fixed-order reduction,
// so C1 = 2 gives class_loss_kernel's bits.
__global__ void class_loss_c_kernel(const float *__restrict__ cls, int C1, const int *__restrict__ idx_q, const int *__restrict__ n_match,
                                    int B, int Q, int maxm, float eos, float *__restrict__ out)
{
    __shared__ unsigned char matched[128];
    __shared__ double wnum[16], wden[16];
    double num = 0., den = 0.;
    for (int b = 0; b < B; ++b) {
        __syncthreads();
        if (threadIdx.x < 128) matched[threadIdx.x] = 0;
        __syncthreads();
        if (threadIdx.x < n_match[b]) matched[idx_q[(long)b * maxm + threadIdx.x]] = 1;
        __syncthreads();
        const int q = threadIdx.x;
        if (q < Q) {
            const float *l = cls + ((long)b * Q + q) * C1;
            float mx, sum;
            softmax_row_stats(l, C1, mx, sum);
            const float lse = mx + logf(sum);
            const bool m = matched[q];
            const float w = m ? 1.f : eos;
            num += (double)(w * (lse - (m ? l[0] : l[C1 - 1])));
            den += (double)w;
        }
    }
    num = wave_sum_d(num); den = wave_sum_d(den);
    if ((threadIdx.x & 63) == 0) { wnum[threadIdx.x >> 6] = num; wden[threadIdx.x >> 6] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sn = 0., sd = 0.;
        for (unsigned int w = 0; w < (blockDim.x + 63) / 64; ++w) { sn += wnum[w]; sd += wden[w]; }   // fixed order
        out[0] = (float)(sn / sd);
    }
}

// class_loss_backward_kernel over C1 logits: one workgroup per clip, a query's C1 gradients written by consecutive lanes
__global__ __launch_bounds__(256) void class_loss_backward_c_kernel(const float *__restrict__ cls, int C1, const int *__restrict__ idx_q,
                                                                    const int *__restrict__ n_match, int B, int Q, int maxm, float eos,
                                                                    float w_ce, float *__restrict__ dcls)
{
    __shared__ unsigned char matched[128];
    __shared__ float mxs[128], sums[128];
    const int b = blockIdx.x;
    double den = 0.;
    for (int bb = 0; bb < B; ++bb) den += (double)n_match[bb] + (double)eos * (Q - n_match[bb]);
    const float wsum = (float)den;
    if (threadIdx.x < 128) matched[threadIdx.x] = 0;
    __syncthreads();
    if ((int)threadIdx.x < n_match[b]) matched[idx_q[(long)b * maxm + threadIdx.x]] = 1;
    if ((int)threadIdx.x < Q) {
        float mx, sum;
        softmax_row_stats(cls + ((long)b * Q + threadIdx.x) * C1, C1, mx, sum);
        mxs[threadIdx.x] = mx; sums[threadIdx.x] = sum;
    }
    __syncthreads();
    const long n = (long)Q * C1;
    for (long i = threadIdx.x; i < n; i += 256) {
        const int q = (int)(i / C1), c = (int)(i - (long)q * C1);
        const float e = expf(cls[(long)b * n + i] - mxs[q]);
        const float pc = e / sums[q];
        const bool m = matched[q];
        const float w = (m ? 1.f : eos) * w_ce / wsum;
        const float onehot = (c == (m ? 0 : C1 - 1)) ? 1.f : 0.f;
        dcls[(long)b * n + i] = w * (pc - onehot);
    }
}

// kd_select_kernel's outputs from the flat ranks of class_select.h: targets are the top-K flat scores that reach the threshold
// (rank < K; a non-candidate has rank n >= K), emitted in ascending flat index q*C + c, so a query may appear once per label.
// One workgroup per clip walks the ranks in 256-wide steps with a ballot prefix count.
__global__ __launch_bounds__(256) void kd_compact_kernel(const int *__restrict__ rank, int n, int C, int K, int Nmax, int *__restrict__ count,
                                                         int *__restrict__ kept, int *__restrict__ label)
{
    __shared__ int wcnt[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int base = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int i = j0 + threadIdx.x;
        const bool keep = i < n && rank[(long)b * n + i] < K;
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) wcnt[w] = __popcll(bal);
        __syncthreads();
        int off = base + before;
        for (int v = 0; v < w; ++v) off += wcnt[v];
        if (keep && off < Nmax) {
            kept[(long)b * Nmax + off] = i / C;
            label[(long)b * Nmax + off] = i % C;
        }
        base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
    if (threadIdx.x == 0) count[b] = base < Nmax ? base : Nmax;
}

}  // namespace

// masks of the selected queries, upsampled and thresholded into tgt / nonempty (the launches shared by both selections)
static int kd_upsample_launch(const float *t_mask_logits, int B, int ldq, int T, int hm, int wm, int H, int W, int Nmax, uint8_t *tgt,
                              const int *count, const int *kept_q, int *nonempty, hipStream_t stream)
{
    // tiled form: whole 4-column groups, 32-bit stores, and a tile's source window inside the staged 8 x 72 pixels
    // (floor(s (o + 15.5) - 0.5) + 1 - floor(s (o + 0.5) - 0.5) <= 16 s + 2 rows, 256 s + 2 columns)
    if (W % 4 == 0 && (reinterpret_cast<uintptr_t>(tgt) & 3) == 0 && 16L * hm + 2L * H <= (long)KDT_SH * H && 256L * wm + 2L * W <= (long)KDT_SW * W)
        hipLaunchKernelGGL(kd_upsample_tile_kernel, dim3(cdiv(W, KDT_W), cdiv(H, KDT_H), B * T), dim3(256), 0, stream, t_mask_logits, ldq, T, hm, wm,
                           H, W, Nmax, count, kept_q, tgt, nonempty);
    else
        hipLaunchKernelGGL(kd_upsample_kernel, dim3(cdiv(W, 256), H, B * T), dim3(256), 0, stream, t_mask_logits, ldq, T, hm, wm,
                           H, W, Nmax, count, kept_q, tgt, nonempty);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

extern "C" {

int s2d_kd_targets_u8(const float *t_class_logits, const float *t_mask_logits, float score_thr, int topk, int B, int Q,
                      int ldq, int T, int hm, int wm, int H, int W, int Nmax, uint8_t *tgt, int *count, int *kept_q,
                      int *nonempty, hipStream_t stream)
{
    if (Q > 128 || Nmax > 128) return S2D_ERR_ARG;
    if (B == 0) return S2D_OK;
    if (s2d_zero_async(nonempty, sizeof(int) * (size_t)B * Nmax * T, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    hipLaunchKernelGGL(kd_select_kernel, dim3(B), dim3(128), 0, stream, t_class_logits, Q, topk < Q ? topk : Q, score_thr,
                       Nmax, count, kept_q);
    return kd_upsample_launch(t_mask_logits, B, ldq, T, hm, wm, H, W, Nmax, tgt, count, kept_q, nonempty, stream);
}

long s2d_kd_targets_c_workspace_bytes(int B, int Q, int C1)
{
    return C1 < 2 ? 0 : cls_select_workspace_bytes(B, Q, C1);
}

int s2d_kd_targets_c_u8(const float *t_class_logits, int C1, const float *t_mask_logits, float score_thr, int topk, int B, int Q,
                        int ldq, int T, int hm, int wm, int H, int W, int Nmax, void *workspace, uint8_t *tgt, int *count, int *kept_q,
                        int *label, int *nonempty, hipStream_t stream)
{
    if (Q > 128 || Nmax > 128 || C1 < 2 || topk < 0 || (long)Q * (C1 - 1) > 0x7FFFFFFFL / 2) return S2D_ERR_ARG;
    if (B == 0) return S2D_OK;
    const int n = Q * (C1 - 1);
    if (s2d_zero_async(nonempty, sizeof(int) * (size_t)B * Nmax * T, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    int *rank = nullptr;
    cls_select_launch(t_class_logits, B, Q, C1, topk < n ? topk : n, score_thr, workspace, &rank, nullptr, nullptr, nullptr, stream);
    hipLaunchKernelGGL(kd_compact_kernel, dim3(B), dim3(256), 0, stream, rank, n, C1 - 1, topk < n ? topk : n, Nmax, count, kept_q, label);
    return kd_upsample_launch(t_mask_logits, B, ldq, T, hm, wm, H, W, Nmax, tgt, count, kept_q, nonempty, stream);
}


int s2d_target_nonempty(const uint8_t *tgt, const int *count, int B, int Nmax, int T, int H, int W, int *nonempty,
                        hipStream_t stream)
{
    if (B * Nmax * T == 0) return S2D_OK;
    if (((long)H * W) % 16) return S2D_ERR_ARG;
    if (s2d_zero_async(nonempty, sizeof(int) * (size_t)B * Nmax * T, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    hipLaunchKernelGGL(nonempty_kernel, dim3(B * Nmax * T, NE_CHUNKS), dim3(256), 0, stream, tgt, count, Nmax, T, (long)H * W, nonempty);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

static const int LOSS_CHUNKS = 8;   // >= number of map parts per row (partial-sum slots)

static const long XBUF_MAX_ROWS = 4096;   // rows whose sampled logits are kept (8.5 GB at P = 160000); the rest recompute

static void point_counts(int num_points, float oversample_ratio, float importance_ratio, int &n_over, int &n_unc, int &n_rand)
{
    n_over = (int)(num_points * oversample_ratio);                 // point_features.py:89
    n_unc = (int)(importance_ratio * num_points);                  // :99
    n_rand = num_points - n_unc;                                   // :100
}

// frames whose bit-packed target plane (H * W / 8 bytes) does not fit LDS keep it in a per-workgroup scratch behind the workspace
static inline bool plane_in_lds(long HW) { return HW / 8 <= 140 * 1024; }
constexpr int ACC_BLOCKS = 512;          // workgroups of the accumulate pass (persistent over the rows)

long s2d_point_loss_workspace_bytes(int NL, int B, int Q, int Nmax, int T, int hm, int wm, int num_points,
                                    float oversample_ratio, float importance_ratio, int H, int W)
{
    const long maxm = Q < Nmax ? Q : Nmax;
    const long rows = (long)NL * B * maxm * T;
    int n_over, n_unc, n_rand;
    point_counts(num_points, oversample_ratio, importance_ratio, n_over, n_unc, n_rand);
    const long xrows = rows < XBUF_MAX_ROWS ? rows : XBUF_MAX_ROWS;
    const long HW = (long)H * W;
    return rows * (3 * 4 + (long)hm * wm * 4 + 2048 * 4 + 4 + 4 + 4 + LOSS_CHUNKS * 16 + PB_STRIDE * 4) + 4L * (NL + 1) + 1024 +
           xrows * (long)(n_over + n_rand + 8) * 4 + 256 + (long)B * Nmax * T * (HW / 32 + 1) * 4;      // + the packed target planes
}

// parameter block + workspace carve-up shared by the forward and the backward entry points (same arguments, same layout)
static int loss_setup(LossParams &p, long &rows, const float *mask_logits, const uint8_t *tgt, const int *tgt_count, const int *nonempty,
                      const int *idx_q, const int *idx_t, const int *n_match, const float *coords_over, const float *coords_rand,
                      uint64_t seed, int NL, int B, int Q, int ldq, int T, int hm, int wm, int H, int W, int Nmax, int num_points,
                      float oversample_ratio, float importance_ratio, int drop_empty, float world_size, void *workspace)
{
    if (Q > 128 || Nmax > 128 || ldq > 128 || ldq < Q || (ldq & 3)) return S2D_ERR_ARG;
    p.ml = mask_logits; p.tgt = tgt; p.tgt_count = tgt_count; p.nonempty = nonempty;
    p.idx_q = idx_q; p.idx_t = idx_t; p.n_match = n_match; p.coords_over = coords_over; p.coords_rand = coords_rand;
    p.seed = seed; p.NL = NL; p.B = B; p.Q = Q; p.ldq = ldq; p.T = T; p.hm = hm; p.wm = wm; p.H = H; p.W = W; p.Nmax = Nmax;
    p.maxm = Q < Nmax ? Q : Nmax;
    point_counts(num_points, oversample_ratio, importance_ratio, p.n_over, p.n_unc, p.n_rand);
    p.drop = drop_empty; p.world_size = world_size; p.chunks = LOSS_CHUNKS;
    rows = (long)NL * B * p.maxm * T;
    if (rows == 0) return S2D_OK;
    char *w = (char *)workspace;
    p.active = (int *)w; w += rows * 4;
    p.rank = (int *)w; w += rows * 4;
    p.prefix = (unsigned int *)w; w += rows * 4;
    p.krem = (int *)w; w += rows * 4;
    p.tie = (unsigned int *)w; w += rows * 4;
    p.list = (int *)w; w += rows * 4;
    p.lcount = (int *)w; w += 4L * (NL + 1);
    w = (char *)(((uintptr_t)w + 255) & ~(uintptr_t)255);
    p.hist = (unsigned int *)w; w += rows * 2048 * 4;
    p.part = (float *)w; w += rows * LOSS_CHUNKS * 16;
    p.pbound = (int *)w; w += rows * PB_STRIDE * 4;
    p.mq = (float *)w; w += rows * (long)hm * wm * 4;
    w = (char *)(((uintptr_t)w + 255) & ~(uintptr_t)255);
    p.xbuf = (float *)w;
    // samples are kept when vector loads line up; the row's target plane is sampled as bits from LDS when it fits (H * W / 8 <= 140 KB
    // beside ~13 KB of static LDS: up to 1.15 M pixels) and from a per-workgroup scratch behind the sample buffer otherwise
    const bool can_stream = (p.n_over % 4 == 0) && (p.n_rand % 4 == 0) && ((long)H * W % 32 == 0);
    p.xcap = can_stream ? (int)(rows < XBUF_MAX_ROWS ? rows : XBUF_MAX_ROWS) : 0;
    {
        char *e = (char *)p.xbuf + (long)(rows < XBUF_MAX_ROWS ? rows : XBUF_MAX_ROWS) * (p.n_over + p.n_rand + 8) * 4;
        p.tpack = (unsigned int *)(((uintptr_t)e + 255) & ~(uintptr_t)255);
    }
    p.bits_global = can_stream && !plane_in_lds((long)H * W);
    const PartGeom pg = part_geom(hm, wm);
    if ((wm & 3) || pg.rows_per_part < 1 || pg.nparts > LOSS_CHUNKS) return S2D_ERR_ARG;
    p.chunks = pg.nparts;
    return S2D_OK;
}

static int loss_attrs()
{
    static S2dDevOnce attr_set;
    if (!attr_set.done()) {
        const int cap = PART_BYTES + 8192 + 4096;
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(hist_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, cap) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void *>(hist_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, cap) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void *>(hist_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, cap) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void *>(accumulate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, cap) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void *>(accumulate_stream_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void *>(accumulate_stream_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void *>(accumulate_stream_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024) != hipSuccess)
            return S2D_ERR_LAUNCH;
        attr_set.mark();
    }
    return S2D_OK;
}

int s2d_point_loss_f32(const float *mask_logits, const uint8_t *tgt, const int *tgt_count, const int *nonempty,
                       const int *idx_q, const int *idx_t, const int *n_match, const float *coords_over,
                       const float *coords_rand, uint64_t seed, int NL, int B, int Q, int ldq, int T, int hm, int wm, int H,
                       int W, int Nmax, int num_points, float oversample_ratio, float importance_ratio, int drop_empty,
                       float world_size, void *workspace, float *losses, hipStream_t stream)
{
    LossParams p;
    long rows = 0;
    if (int e = loss_setup(p, rows, mask_logits, tgt, tgt_count, nonempty, idx_q, idx_t, n_match, coords_over, coords_rand, seed, NL, B, Q, ldq,
                           T, hm, wm, H, W, Nmax, num_points, oversample_ratio, importance_ratio, drop_empty, world_size, workspace))
        return e;
    if (rows == 0) return S2D_OK;
    if (s2d_zero_async(p.hist, (size_t)rows * 2048 * 4, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    if (s2d_zero_async(p.tie, (size_t)rows * 4, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    hipLaunchKernelGGL(row_prep_kernel, dim3(NL), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(row_list_kernel, dim3(NL), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(cdiv((long)hm * wm, 64), T, NL * B), dim3(256), 0, stream, p);
    const PartGeom pg = part_geom(hm, wm);
    static_assert(PB_STRIDE == LOSS_CHUNKS + 1, "one bound per part + the end");
    if (!coords_over) hipLaunchKernelGGL(row_strata_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, p, pg.nparts, pg.rows_per_part);
    const size_t lds_map = sizeof(float) * (size_t)(pg.rows_per_part + 3) * (wm + 2 * PADC);      // the padded block (>= the plain (rows + 1) x wm one)
    const size_t lds_hist = lds_map + sizeof(float) * 2048;
    if (int e = loss_attrs()) return e;
    const dim3 g(512);      // persistent: 2 blocks per CU's worth of items in flight
    hipLaunchKernelGGL(hist_kernel<0>, g, dim3(LTHREADS), lds_hist, stream, p);
    hipLaunchKernelGGL(select_kernel<0>, dim3((unsigned)rows), dim3(256), 0, stream, p);
    if (p.xcap > 0) hipLaunchKernelGGL(hist_stream_kernel<1>, dim3(2048), dim3(256), 0, stream, p);
    if (rows > p.xcap) hipLaunchKernelGGL(hist_kernel<1>, g, dim3(LTHREADS), lds_hist, stream, p);
    hipLaunchKernelGGL(select_kernel<1>, dim3((unsigned)rows), dim3(256), 0, stream, p);
    if (p.xcap > 0) hipLaunchKernelGGL(hist_stream_kernel<2>, dim3(2048), dim3(256), 0, stream, p);
    if (rows > p.xcap) hipLaunchKernelGGL(hist_kernel<2>, g, dim3(LTHREADS), lds_hist, stream, p);
    hipLaunchKernelGGL(select_kernel<2>, dim3((unsigned)rows), dim3(256), 0, stream, p);
    if (p.xcap > 0)
        hipLaunchKernelGGL(pack_planes_kernel, dim3(cdiv((long)H * W / 32, 256), B * Nmax * T), dim3(256), 0, stream, p);
    if (p.xcap > 0 && !p.bits_global)
        hipLaunchKernelGGL(accumulate_stream_kernel<false>, dim3(ACC_BLOCKS), dim3(LTHREADS), (size_t)((long)H * W / 8), stream, p, LossBwdArgs{nullptr, 0.f, 0.f, nullptr});
    else if (p.xcap > 0)
        hipLaunchKernelGGL((accumulate_stream_kernel<false, true>), dim3(ACC_BLOCKS), dim3(LTHREADS), 16, stream, p, LossBwdArgs{nullptr, 0.f, 0.f, nullptr});
    if (rows > p.xcap) {
        hipLaunchKernelGGL(accumulate_kernel, g, dim3(LTHREADS), lds_map, stream, p);
        hipLaunchKernelGGL(accumulate_ties_kernel, g, dim3(LTHREADS), 0, stream, p);
    }
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(NL), dim3(64), 0, stream, p, losses);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

/* Backward of s2d_point_loss_f32 with the SAME arguments and the workspace the forward left behind (thresholds, tie
 * state, stored samples, per-row sums): grad_rows [NL*B*maxm*T][hm*wm] receives d(w_mask*loss_mask + w_dice*loss_dice of
 * every layer)/d(logit map of the row); rows of unmatched slots / dropped frames stay zero. */
int s2d_point_loss_backward_f32(const float *mask_logits, const uint8_t *tgt, const int *tgt_count, const int *nonempty,
                                const int *idx_q, const int *idx_t, const int *n_match, const float *coords_over,
                                const float *coords_rand, uint64_t seed, int NL, int B, int Q, int ldq, int T, int hm, int wm, int H,
                                int W, int Nmax, int num_points, float oversample_ratio, float importance_ratio, int drop_empty,
                                float world_size, void *workspace, float w_mask, float w_dice, float *grad_rows,
                                unsigned int *bit_scratch, hipStream_t stream)
{
    LossParams p;
    long rows = 0;
    if (int e = loss_setup(p, rows, mask_logits, tgt, tgt_count, nonempty, idx_q, idx_t, n_match, coords_over, coords_rand, seed, NL, B, Q, ldq,
                           T, hm, wm, H, W, Nmax, num_points, oversample_ratio, importance_ratio, drop_empty, world_size, workspace))
        return e;
    if (rows == 0) return S2D_OK;
    if (p.xcap <= 0) return S2D_ERR_ARG;               // only the stored-sample path has a backward (every real configuration takes it;
                                                       // the caller checks that the ACTIVE rows, lcount[NL], fit xcap = min(rows, 4096))
    if (int e = loss_attrs()) return e;
    if (s2d_zero_async(grad_rows, sizeof(float) * (size_t)rows * hm * wm, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    const PartGeom pg = part_geom(hm, wm);
    const size_t lds = sizeof(int) * (size_t)(pg.rows_per_part + 3 < hm ? pg.rows_per_part + 3 : hm) * wm;     // one map part + 3 shared rows
    if (lds > 140 * 1024 || 3L * wm > 4L * LTHREADS || pg.nparts + 1 > PB_STRIDE) return S2D_ERR_ARG;
    // the bit-packed target planes of the rows in flight: the tail of the workspace's sample buffer is not used by the
    // backward walk beyond xcap rows; a dedicated scratch keeps it simple
    hipLaunchKernelGGL(accumulate_stream_kernel<true>, dim3(ACC_BLOCKS), dim3(LTHREADS), lds, stream, p,
                       LossBwdArgs{grad_rows, w_mask, w_dice, bit_scratch});
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

/* Test hook: the oversampled points the RNG mode of s2d_point_loss_f32 generates for rows [row0, row0 + nrows) under `seed` on an
 * (hm, wm) logit map -- uv [nrows][n_over][2] and the strata bounds [nrows][9] -- produced by the same device functions the loss
 * kernels call (row_strata_kernel, over_point_rng), so the generator's law can be checked without going through a loss value. */
int s2d_point_loss_rng_points(uint64_t seed, int hm, int wm, int row0, int nrows, int n_over, float *uv, int *bounds, int *scratch_list,
                              hipStream_t stream)
{
    const PartGeom pg = part_geom(hm, wm);
    if ((wm & 3) || pg.rows_per_part < 1 || pg.nparts > LOSS_CHUNKS || nrows <= 0 || row0 != 0) return S2D_ERR_ARG;
    LossParams p = {};
    p.seed = seed; p.hm = hm; p.wm = wm; p.n_over = n_over; p.NL = 0;
    p.list = scratch_list;            // [nrows + 1]: identity list, then lcount[NL = 0] = nrows
    p.lcount = scratch_list + nrows;
    p.pbound = bounds;
    hipLaunchKernelGGL(rng_points_prep_kernel, dim3(cdiv(nrows + 1, 256)), dim3(256), 0, stream, scratch_list, nrows);
    hipLaunchKernelGGL(row_strata_kernel, dim3(cdiv(nrows, 4)), dim3(256), 0, stream, p, pg.nparts, pg.rows_per_part);
    hipLaunchKernelGGL(rng_points_kernel, dim3(cdiv(n_over, 256), nrows), dim3(256), 0, stream, p, pg.nparts, pg.rows_per_part, uv);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_class_loss_backward_f32(const float *class_logits, const int *idx_q, const int *n_match, int B, int Q, int maxm, float eos_coef,
                                float w_ce, float *d_class_logits, hipStream_t stream)
{
    if (Q > 128) return S2D_ERR_ARG;
    hipLaunchKernelGGL(class_loss_backward_kernel, dim3(1), dim3(128), 0, stream, class_logits, idx_q, n_match, B, Q, maxm, eos_coef, w_ce,
                       d_class_logits);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_class_loss_f32(const float *class_logits, const int *idx_q, const int *n_match, int B, int Q, int maxm,
                       float eos_coef, float *loss_ce, hipStream_t stream)
{
    if (Q > 128) return S2D_ERR_ARG;
    hipLaunchKernelGGL(class_loss_kernel, dim3(1), dim3(128), 0, stream, class_logits, idx_q, n_match, B, Q, maxm, eos_coef,
                       loss_ce);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_class_loss_c_f32(const float *class_logits, int C1, const int *idx_q, const int *n_match, int B, int Q, int maxm,
                         float eos_coef, float *loss_ce, hipStream_t stream)
{
    if (Q > 128 || C1 < 2) return S2D_ERR_ARG;
    hipLaunchKernelGGL(class_loss_c_kernel, dim3(1), dim3(128), 0, stream, class_logits, C1, idx_q, n_match, B, Q, maxm, eos_coef,
                       loss_ce);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_class_loss_backward_c_f32(const float *class_logits, int C1, const int *idx_q, const int *n_match, int B, int Q, int maxm,
                                  float eos_coef, float w_ce, float *d_class_logits, hipStream_t stream)
{
    if (Q > 128 || C1 < 2) return S2D_ERR_ARG;
    if (B == 0) return S2D_OK;
    hipLaunchKernelGGL(class_loss_backward_c_kernel, dim3(B), dim3(256), 0, stream, class_logits, C1, idx_q, n_match, B, Q, maxm,
                       eos_coef, w_ce, d_class_logits);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
