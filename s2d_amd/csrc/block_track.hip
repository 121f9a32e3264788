// Block-matching point trackers for keymask discovery (s2d_amd/keymask/block_tracker.py): integer searches on u8 grey frames.
// Self-defined (the reference's tracker is CoTracker, third party): a baseline, not a restatement.  Every output is an integer
// decision, so tests/block_tracker_ref.py, tests/live_tracker_ref.py and tests/zm_tracker_ref.py reproduce the exports bit for bit.
//
//  grey pass   video f32 [T][3][H][W] (RGB, nominally 0..255) -> u8 [T][H][W]: per channel round-half-even of the value clamped
//              to [0, 255] (NaN -> 0), then (77 r + 150 g + 29 b + 128) >> 8
//  tracker     one body, track_point: one wave per (point, direction).  Template = the (2R+1)^2 patch round the point in the query
//              frame.  Per frame the wave stages the (2(R+S)+1)^2 region round its current centre into LDS (border replicate), its
//              lanes take the (2S+1)^2 displacements in rounds of 64, and the minimum of (cost, dx^2+dy^2, dy, dx) is reduced as one
//              packed 64-bit key.  cost <= tau (2R+1)^2: visible, the centre moves; otherwise the centre stays and the point keeps
//              searching round its last good position.  A visible point whose cost is at most tau_u (2R+1)^2 takes the patch round
//              its new centre as its template (tau_u = -1: never).
//  two costs   SadCost: the sum of absolute differences (s2d_block_track_live_u8 with S up to 64, and s2d_block_track_u8, which is
//              the same search with S up to 24 and tau_u = -1); ZeroMeanCost: the patch means removed first and a gate on
//              untextured templates (s2d_block_track_zm_u8).  Each is described in front of its struct below.
//
// LDS image: region rows of `pitch` dwords (odd: consecutive rows start on different banks), the row's bytes packed 4 per dword;
// a patch row that starts at byte b is read as K + 1 aligned dwords from b >> 2 and shifted into place (v_alignbyte_b32), then
// v_sad_u8 against the template dword.  The template's pad bytes are zero and the same mask clears the region's.  The region is
// dynamic LDS, D rows of `pitch` dwords (at R = 7, S = 64: 143 x 37 dwords, 21 KB; at S = 24: 63 x 17), so a small S keeps a
// high occupancy.
#include "common.h"

namespace {

constexpr int BT_MAX_R = 7, BT_MAX_S = 24, BTL_MAX_S = 64;

__global__ __launch_bounds__(256) void video_grey_kernel(const float *__restrict__ video, long HW, long n, uint8_t *__restrict__ grey)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long t = i / HW, p = i - t * HW;
    const float *src = video + t * 3 * HW + p;
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (int)rintf(fminf(fmaxf(src[k * HW], 0.f), 255.f));   // fmaxf(NaN, 0) = 0
    grey[i] = (uint8_t)((77 * c[0] + 150 * c[1] + 29 * c[2] + 128) >> 8);
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// 4 bytes of row `row` from column x0 on, columns clamped to the frame
__device__ __forceinline__ unsigned int load4_clamped(const uint8_t *__restrict__ row, int x0, int W)
{
    unsigned int w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) w |= (unsigned int)row[clampi(x0 + b, W - 1)] << (8 * b);
    return w;
}

__device__ __forceinline__ unsigned int wave_sum(unsigned int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void write_point(float *__restrict__ tracks, uint8_t *__restrict__ vis, int N, int t, int n, int x, int y,
                                            bool visible)
{
    tracks[((long)t * N + n) * 2] = (float)x;
    tracks[((long)t * N + n) * 2 + 1] = (float)y;
    vis[(long)t * N + n] = visible;
}

// What both costs know of a lane.  K = dwords per patch row = ceil((2R+1) / 4); lanes below 4 P hold template dword tk of row tj.
template <int K>
struct PatchLane {
    const int tj, tk;
    const bool tlane;                                         // this lane holds a patch dword (tk < K)
    const unsigned int lastmask;                              // the valid bytes of a row's last dword
    __device__ __forceinline__ PatchLane(int P, int lane)
        : tj(lane >> 2), tk(lane & 3), tlane(lane < P * 4 && tk < K), lastmask(0xFFFFFFFFu >> (8 * (4 * K - P))) {}

    // v_sad_u8 of the patch row that starts at byte sh of row[0] (pad bytes cleared) against the K dwords t, or against zero
    template <bool AGAINST_TEMPLATE>
    __device__ __forceinline__ unsigned int sad_row(const unsigned int *row, unsigned int sh, const unsigned int *t, unsigned int acc) const
    {
        unsigned int lo = row[0];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const unsigned int hi = row[k + 1];
            unsigned int v = __builtin_amdgcn_alignbyte(hi, lo, sh);
            if (k == K - 1) v &= lastmask;
            acc = __builtin_amdgcn_sad_u8(v, AGAINST_TEMPLATE ? t[k] : 0u, acc);
            lo = hi;
        }
        return acc;
    }
};

// ---- the sum of absolute differences (s2d_block_track_u8, s2d_block_track_live_u8) ----------------------------------------------
// Template: 4 dwords per patch row, the patch bytes as they are (dwords K .. 3 are never read).
template <int K>
struct SadCost : PatchLane<K> {
    static constexpr int ROW = 4;                             // template dwords per patch row
    static constexpr bool GATED = false;
    static constexpr unsigned int min_dev = 0;
    struct Candidate {
        unsigned int sh;
    };
    __device__ __forceinline__ SadCost(int P, int lane) : PatchLane<K>(P, lane) {}

    // the template from this lane's patch dword v (pad bytes zero); returns no deviation
    __device__ __forceinline__ unsigned int store_template(unsigned int *tmpl, unsigned int v) const
    {
        if (this->tlane) tmpl[this->tj * ROW + this->tk] = v;
        return 0;
    }
    __device__ __forceinline__ Candidate candidate(const unsigned int *, int, int, unsigned int sh) const { return {sh}; }
    __device__ __forceinline__ unsigned int add_row(const Candidate &c, const unsigned int *row, const unsigned int *t, unsigned int cost) const
    {
        return this->template sad_row<true>(row, c.sh, t, cost);
    }
};

// ---- the zero-mean cost (s2d_block_track_zm_u8) -----------------------------------------------------------------------------------
// Both patches lose their rounded mean first, mean(X) = (2 sum(X) + n) / (2 n), n = (2R+1)^2,
//     zcost(L, X) = sum_i |(L_i - mean(L)) - (X_i - mean(X))|,
// so a brightness offset of a whole frame cancels exactly, and a gate: a point whose query-frame template deviates from its own
// mean by less than texture * n in total (dev(L) = sum_i |L_i - mean(L)|) is not searched at all -- under a zero-mean cost a flat
// template costs about 0 against every flat patch.
//
// Both sides of the difference are kept biased by 255, L_i - mean(L) + 255 and X_i - mean(X) + 255, which lie in 0 .. 510: two
// pixels per dword as u16 pairs, and v_sad_u16 takes two absolute differences at once.  The template is stored in that form (two
// dwords per patch dword, pad halves zero).  A candidate first takes its patch sum (v_sad_u8 against zero over the dwords the
// cost loop reads), then per patch dword two v_perm_b32 -- byte shift, zero extension and, in a row's last dword, clearing of
// the pad bytes in one instruction each --, two adds of the pair (255 - mean(X)) and two v_sad_u16.  The division by 2 n is a
// multiplication: 2 sum + n < 2^17 and 2 n <= 450, for which mulhi(x, ceil(2^32 / (2 n))) is the exact quotient.
template <int K>
struct ZeroMeanCost : PatchLane<K> {
    static constexpr int ROW = 8;                             // row j, patch dword k: u16 pairs of bytes (0, 1) at 8 j + 2 k, (2, 3) behind
    static constexpr bool GATED = true;
    struct Candidate {
        unsigned int sello, selhi, lastlo, lasthi, c2, c2lo, c2hi;
    };
    const unsigned int nn, magic;                             // 2 n is no power of two: magic = ceil(2^32 / 2n)
    const bool one;                                           // a row's last dword holds 1 valid byte, otherwise 3
    const unsigned int padlo, padhi;                          // its valid u16 halves
    const unsigned int min_dev;                               // the gate: texture * n
    uint8_t *__restrict__ const trackable;
    __device__ __forceinline__ ZeroMeanCost(int P, int lane, int texture, uint8_t *__restrict__ trackable_)
        : PatchLane<K>(P, lane), nn((unsigned int)(P * P)), magic(0xFFFFFFFFu / (2 * nn) + 1), one(P - 4 * (K - 1) == 1),
          padlo(one ? 0x0000FFFFu : 0xFFFFFFFFu), padhi(one ? 0u : 0x0000FFFFu), min_dev((unsigned int)texture * nn),
          trackable(trackable_) {}

    // the template from this lane's patch dword v (pad bytes zero; 0 in the other lanes); returns dev(L)
    __device__ __forceinline__ unsigned int store_template(unsigned int *tmpl, unsigned int v) const
    {
        const unsigned int mean = __umulhi(2 * wave_sum(__builtin_amdgcn_sad_u8(v, 0u, 0u)) + nn, magic);
        const unsigned int c2 = (255 - mean) * 0x00010001u;
        const bool last = this->tk == K - 1;
        const unsigned int mlo = last ? padlo : 0xFFFFFFFFu, mhi = last ? padhi : 0xFFFFFFFFu;
        unsigned int dev = 0;
        if (this->tlane) {
            const unsigned int lo = __builtin_amdgcn_perm(0u, v, 0x0c010c00u) + (c2 & mlo);
            const unsigned int hi = __builtin_amdgcn_perm(0u, v, 0x0c030c02u) + (c2 & mhi);
            tmpl[this->tj * ROW + 2 * this->tk] = lo;
            tmpl[this->tj * ROW + 2 * this->tk + 1] = hi;
            dev = __builtin_amdgcn_sad_u16(hi, 0x00FF00FFu & mhi, __builtin_amdgcn_sad_u16(lo, 0x00FF00FFu & mlo, 0u));
        }
        return wave_sum(dev);
    }
    // the candidate's patch sum, and from it the pair (255 - mean) and the selectors of its byte shift
    __device__ __forceinline__ Candidate candidate(const unsigned int *row, int pitch, int P, unsigned int sh) const
    {
        unsigned int sum = 0;
        for (int j = 0; j < P; ++j) sum = this->template sad_row<false>(row + j * pitch, sh, nullptr, sum);
        // v_perm_b32 selectors over the bytes of hi:lo (0 .. 3 lo, 4 .. 7 hi, 0x0c a zero byte): bytes sh, sh + 1 and
        // sh + 2, sh + 3 zero-extended to u16 pairs; in a row's last dword the pad bytes come out zero
        const unsigned int sello = 0x0c000c00u | sh | ((sh + 1) << 16), selhi = 0x0c000c00u | (sh + 2) | ((sh + 3) << 16);
        const unsigned int c2 = (255 - __umulhi(2 * sum + nn, magic)) * 0x00010001u;
        return {sello, selhi, one ? 0x0c0c0c00u | sh : sello, one ? 0x0c0c0c0cu : 0x0c0c0c00u | (sh + 2), c2, c2 & padlo, c2 & padhi};
    }
    __device__ __forceinline__ unsigned int add_row(const Candidate &c, const unsigned int *row, const unsigned int *t, unsigned int cost) const
    {
        unsigned int lo = row[0];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const unsigned int hi = row[k + 1];
            const bool last = k == K - 1;
            const unsigned int a = __builtin_amdgcn_perm(hi, lo, last ? c.lastlo : c.sello) + (last ? c.c2lo : c.c2);
            const unsigned int b = __builtin_amdgcn_perm(hi, lo, last ? c.lasthi : c.selhi) + (last ? c.c2hi : c.c2);
            cost = __builtin_amdgcn_sad_u16(a, t[2 * k], cost);
            cost = __builtin_amdgcn_sad_u16(b, t[2 * k + 1], cost);
            lo = hi;
        }
        return cost;
    }
};

// ---- the tracker -----------------------------------------------------------------------------------------------------------------
// The live template: after the decision of frame t the new patch lies inside the staged region (|dx|, |dy| <= S), whose bytes
// already are the border-replicated frame, so it is copied from LDS with the aligned read of the cost loop.
//
// Key: cost <= 510 * 15^2 < 2^17 (SAD: 255 * 15^2 < 2^16), d^2 <= 2 * 64^2 < 2^14, dy + S and dx + S <= 128 < 2^8 each:
// 17 + 14 + 8 + 8 = 47 bits.
//
// Pruning (exact): a candidate whose partial cost exceeds tau (2R+1)^2 can only be the minimum when every candidate exceeds it,
// and then the point is invisible, stays where it is and keeps its template -- the minimum itself is never looked at; a
// candidate whose partial cost exceeds the lane's best cost so far cannot be the lane's minimum.  Rows only add to the cost, so
// the row loop stops at either bound.
template <int K, class Cost, class... Gate>
__device__ __forceinline__ void track_point(const uint8_t *__restrict__ grey, int T, int H, int W, const int *__restrict__ points,
                                            int N, int q, int R, int S, int tau, int tau_u, float *__restrict__ tracks,
                                            uint8_t *__restrict__ vis, Gate... gate)
{
    extern __shared__ unsigned int region[];
    __shared__ unsigned int tmpl[(2 * BT_MAX_R + 1) * Cost::ROW];
    const int n = blockIdx.x, backward = blockIdx.y, lane = threadIdx.x;
    const int P = 2 * R + 1, D = 2 * (R + S) + 1, C = 2 * S + 1;
    const int pitch = (((2 * S) >> 2) + K + 1) | 1;
    const long HW = (long)H * W;
    // a point outside the frame (outside the contract) is clamped into it: the centre then always has a valid candidate
    const int px = clampi(points[2 * n], W - 1), py = clampi(points[2 * n + 1], H - 1);
    const Cost cost_of(P, lane, gate...);

    unsigned int v0 = 0;
    if (cost_of.tlane) {
        v0 = load4_clamped(grey + (long)q * HW + (long)clampi(py - R + cost_of.tj, H - 1) * W, px - R + 4 * cost_of.tk, W);
        if (cost_of.tk == K - 1) v0 &= cost_of.lastmask;
    }
    const bool ok = cost_of.store_template(tmpl, v0) >= cost_of.min_dev;   // the texture gate (SadCost has none: 0 >= 0)
    if (!backward && lane == 0) {
        // the query frame; without a backward wave (gridDim.y == 1) the frames before it hold the point, invisible
        for (int t = gridDim.y == 1 ? 0 : q; t <= q; ++t) write_point(tracks, vis, N, t, n, px, py, t == q);
        if constexpr (Cost::GATED) cost_of.trackable[n] = ok;
    }
    if (!ok) {                                              // the same decision in every lane: the frames of this direction hold p
        for (int t = (backward ? 0 : q + 1) + lane; t < (backward ? q : T); t += 64) write_point(tracks, vis, N, t, n, px, py, false);
        return;
    }
    int cx = px, cy = py;
    const int step = backward ? -1 : 1;
    const unsigned int limit = (unsigned int)(tau * P * P);
    const int limit_u = tau_u * P * P;                        // negative: never refreshed
    for (int t = q + step; t >= 0 && t < T; t += step) {
        __syncthreads();                                    // the template stores / the previous frame's reads are done
        const uint8_t *fr = grey + (long)t * HW;
        const int ox = cx - S - R, oy = cy - S - R;
        for (int e = lane; e < D * pitch; e += 64) {
            const int ry = e / pitch, wx = e - ry * pitch;
            region[e] = load4_clamped(fr + (long)clampi(oy + ry, H - 1) * W, ox + 4 * wx, W);
        }
        __syncthreads();
        // The search loops below run 1-1.5 % slower or faster with where they start within a 64-byte fetch line (measured: 8 bytes
        // more or less code in front of them), so their start is fixed here, once per frame, whatever precedes it.
        asm volatile(".p2align 6");
        unsigned long long best = ~0ull;
        unsigned int bound = limit;                         // min(limit, the lane's best cost)
        for (int cand = lane; cand < C * C; cand += 64) {
            const int dyi = cand / C, dxi = cand - dyi * C;
            const int nx = cx + dxi - S, ny = cy + dyi - S;
            if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
            const unsigned int *row = region + dyi * pitch + (dxi >> 2);
            const typename Cost::Candidate c = cost_of.candidate(row, pitch, P, (unsigned int)(dxi & 3));
            unsigned int cost = 0;
            for (int j = 0; j < P && cost <= bound; ++j, row += pitch) cost = cost_of.add_row(c, row, tmpl + j * Cost::ROW, cost);
            if (cost > bound) continue;
            bound = cost;
            const int dx = dxi - S, dy = dyi - S;
            const unsigned long long key = ((unsigned long long)cost << 30) | ((unsigned long long)(dx * dx + dy * dy) << 16) |
                                           ((unsigned long long)dyi << 8) | (unsigned long long)dxi;
            best = key < best ? key : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other < best ? other : best;
        }
        // no candidate within the bound: best is still ~0, whose cost field exceeds every limit
        const unsigned long long cost = best >> 30;
        const bool visible = cost <= limit;
        const int bxi = (int)(best & 255), byi = (int)((best >> 8) & 255);
        if (visible) {
            cx += bxi - S;
            cy += byi - S;
        }
        if (lane == 0) write_point(tracks, vis, N, t, n, cx, cy, visible);
        if (visible && (long long)cost <= limit_u) {        // the same decision in every lane
            __syncthreads();                                // every lane is done with the old template
            unsigned int v = 0;
            if (cost_of.tlane) {
                const unsigned int *row = region + (byi + cost_of.tj) * pitch + (bxi >> 2) + cost_of.tk;
                v = __builtin_amdgcn_alignbyte(row[1], row[0], (unsigned int)(bxi & 3));
                if (cost_of.tk == K - 1) v &= cost_of.lastmask;
            }
            cost_of.store_template(tmpl, v);
        }
    }
}

template <int K>
__global__ __launch_bounds__(64) void block_track_live_kernel(const uint8_t *__restrict__ grey, int T, int H, int W,
                                                              const int *__restrict__ points, int N, int q, int R, int S, int tau,
                                                              int tau_u, float *__restrict__ tracks, uint8_t *__restrict__ vis)
{
    track_point<K, SadCost<K>>(grey, T, H, W, points, N, q, R, S, tau, tau_u, tracks, vis);
}

template <int K>
__global__ __launch_bounds__(64) void block_track_zm_kernel(const uint8_t *__restrict__ grey, int T, int H, int W,
                                                            const int *__restrict__ points, int N, int q, int R, int S, int tau,
                                                            int tau_u, int texture, float *__restrict__ tracks,
                                                            uint8_t *__restrict__ vis, uint8_t *__restrict__ trackable)
{
    track_point<K, ZeroMeanCost<K>>(grey, T, H, W, points, N, q, R, S, tau, tau_u, tracks, vis, texture, trackable);
}

// what the three exports ask of the arguments they share
bool track_args_ok(int T, int H, int W, int N, int q, int R, int tau)
{
    return R >= 1 && R <= BT_MAX_R && tau >= 0 && tau <= 255 && T >= 1 && q >= 0 && q < T && N >= 0 && H >= 1 && W >= 1 &&
           H < (1 << 15) && W < (1 << 15);
}

// the instantiations a launch chooses from
struct LiveKernel {
    template <int K>
    static constexpr auto of = block_track_live_kernel<K>;
};
struct ZeroMeanKernel {
    template <int K>
    static constexpr auto of = block_track_zm_kernel<K>;
};

// One wave per (point, direction) of the kernel for K = ceil((2R+1) / 4), with the region as dynamic LDS.  `args` are the
// kernel's arguments, checked by the caller.
template <class Kernel, class... Args>
int launch_tracker(int N, int q, int backward, int R, int S, hipStream_t stream, Args... args)
{
    if (N == 0) return S2D_OK;
    const dim3 grid(N, backward && q > 0 ? 2 : 1);
    const int K = (2 * R + 1 + 3) / 4, pitch = (((2 * S) >> 2) + K + 1) | 1;
    const size_t lds = (size_t)(2 * (R + S) + 1) * pitch * sizeof(unsigned int);          // at most 143 * 37 * 4 = 21,164 bytes
    switch (K) {
    case 1: hipLaunchKernelGGL(Kernel::template of<1>, grid, dim3(64), lds, stream, args...); break;
    case 2: hipLaunchKernelGGL(Kernel::template of<2>, grid, dim3(64), lds, stream, args...); break;
    case 3: hipLaunchKernelGGL(Kernel::template of<3>, grid, dim3(64), lds, stream, args...); break;
    case 4: hipLaunchKernelGGL(Kernel::template of<4>, grid, dim3(64), lds, stream, args...); break;
    default: return S2D_ERR_ARG;
    }
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // namespace

extern "C" {

int s2d_video_grey_u8(const float *video, int T, int H, int W, uint8_t *grey, hipStream_t stream)
{
    if (T < 0 || H < 1 || W < 1) return S2D_ERR_ARG;
    const long HW = (long)H * W, n = (long)T * HW;
    if (n == 0) return S2D_OK;
    if (n > 256L * 0x7FFFFFFF) return S2D_ERR_ARG;
    hipLaunchKernelGGL(video_grey_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, video, HW, n, grey);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

// the live search with a template that is never refreshed
int s2d_block_track_u8(const uint8_t *grey, int T, int H, int W, const int *points, int N, int q, int backward, int R, int S,
                       int tau, float *tracks, uint8_t *vis, hipStream_t stream)
{
    if (!track_args_ok(T, H, W, N, q, R, tau) || S < 1 || S > BT_MAX_S) return S2D_ERR_ARG;
    return launch_tracker<LiveKernel>(N, q, backward, R, S, stream, grey, T, H, W, points, N, q, R, S, tau, -1, tracks, vis);
}

int s2d_block_track_live_u8(const uint8_t *grey, int T, int H, int W, const int *points, int N, int q, int backward, int R, int S,
                            int tau, int tau_u, float *tracks, uint8_t *vis, hipStream_t stream)
{
    if (!track_args_ok(T, H, W, N, q, R, tau) || S < 1 || S > BTL_MAX_S || tau_u < -1 || tau_u > tau) return S2D_ERR_ARG;
    return launch_tracker<LiveKernel>(N, q, backward, R, S, stream, grey, T, H, W, points, N, q, R, S, tau, tau_u, tracks, vis);
}

int s2d_block_track_zm_u8(const uint8_t *grey, int T, int H, int W, const int *points, int N, int q, int backward, int R, int S,
                          int tau, int tau_u, int texture, float *tracks, uint8_t *vis, uint8_t *trackable, hipStream_t stream)
{
    if (!track_args_ok(T, H, W, N, q, R, tau) || S < 1 || S > BTL_MAX_S || tau_u < -1 || tau_u > tau) return S2D_ERR_ARG;
    if (texture < 0 || texture > 127) return S2D_ERR_ARG;
    return launch_tracker<ZeroMeanKernel>(N, q, backward, R, S, stream, grey, T, H, W, points, N, q, R, S, tau, tau_u, texture, tracks,
                                          vis, trackable);
}

}  // extern "C"
