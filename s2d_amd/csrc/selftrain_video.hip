// The video self-training merge (s2d_amd/selftrain_video.py): tube counts of every (previous track, kept prediction) pair of a
// CHUNK of videos of different sizes and lengths, and the keep rule on them.  The layout (one flat plane buffer, a per-video
// table, a present table, a tile list) is documented in include/s2d_hip.h, "Tube layout".
//
//   tube_counts_kernel  grid (tiles, splits).  A workgroup owns one 8 x 8 tile of (p, q) pairs of one video and one contiguous
//                       range of that video's T * wpp frame-words.  It walks the range frame by frame.  The presence of the 8
//                       P-side tracks at a frame is uniform over the workgroup: a frame at which none of them is present is
//                       skipped without a load, and an absent track's words are not loaded.  Inside a frame every word of the 16
//                       planes is loaded once; the intersections go through PopcTile (bitplane.h), the frame's plane areas are
//                       kept per thread and folded into a second PopcTile at the end of the frame:
//                       sum[p][q] += present[p] ? |p_t| + |q_t| : 0.  union = sum - inter.  Partial sums leave the workgroup by
//                       integer atomics, so the result does not depend on the order and a second call is bitwise equal.
//   keep_tube_kernel    one wave per video, a thread per previous track.
//
// Everything is an integer.  A video row that does not fit the buffers it names is skipped: nothing is read or written for it.
#include "bitplane.h"

namespace {

constexpr int VT = 8;                        // pair tile edge
constexpr int VID_COLS = 11;                 // columns of a video-table row (s2d_hip.h)
constexpr long SPLIT_WORDS_MAX = 1L << 26;   // frame-words of one workgroup: its per-wave sums stay below 2^32 (64 bits a word pair)
constexpr int KEEP_T = 64;

struct VideoRow {
    long p_word, q_word, wpp, hw, T, D, G, d0, g0, pair0, pres0;
    bool ok;
};

__device__ __forceinline__ VideoRow video_row(const long *__restrict__ vid, int v, long total_words, long n_present, long n_pairs)
{
    const long *r = vid + (long)VID_COLS * v;
    VideoRow q;
    q.p_word = r[0]; q.q_word = r[1]; q.wpp = r[2]; q.hw = r[3]; q.T = r[4]; q.D = r[5]; q.G = r[6];
    q.d0 = r[7]; q.g0 = r[8]; q.pair0 = r[9]; q.pres0 = r[10];
    const long lim = 1L << 31;
    q.ok = q.hw >= 1 && q.hw < lim && q.wpp == (q.hw + 31) / 32 && q.T >= 0 && q.T < lim && q.D >= 0 && q.D < lim && q.G >= 0 &&
           q.G < lim && q.d0 >= 0 && q.g0 >= 0;
    if (!q.ok) return q;
    const long tw = q.T * q.wpp;                                                  // < 2^57
    q.ok = tw < (1L << 40) && q.p_word >= 0 && q.q_word >= 0 && q.D * tw <= total_words - q.p_word &&
           q.G * tw <= total_words - q.q_word && q.pres0 >= 0 && q.D * q.T <= n_present - q.pres0 && q.pair0 >= 0 &&
           q.D * q.G <= n_pairs - q.pair0;
    return q;
}

__global__ __launch_bounds__(256, 2) void tube_counts_kernel(const uint32_t *__restrict__ bits, long total_words,
                                                          const long *__restrict__ vid, int N, const uint8_t *__restrict__ present,
                                                          long n_present, const int *__restrict__ tiles,
                                                          unsigned long long *__restrict__ inter, unsigned long long *__restrict__ uni,
                                                          long n_pairs)
{
    __shared__ unsigned int red_i[4][VT * VT];
    __shared__ unsigned long long red_s[4][VT * VT];
    const int *tl = tiles + 3L * blockIdx.x;
    const int v = tl[0], ti = tl[1], tj = tl[2];
    if (v < 0 || v >= N || ti < 0 || tj < 0) return;                              // uniform over the workgroup
    const VideoRow r = video_row(vid, v, total_words, n_present, n_pairs);
    if (!r.ok || (long)ti * VT >= r.D || (long)tj * VT >= r.G) return;
    const long tw = r.T * r.wpp;
    const long per = (tw + gridDim.y - 1) / gridDim.y;
    const long f0 = (long)blockIdx.y * per, f1 = f0 + per < tw ? f0 + per : tw;
    if (f0 >= f1 || per > SPLIT_WORDS_MAX) return;                                // a track longer than max_track_words said: skipped
    const uint32_t tail = (r.hw & 31) ? ((1u << (r.hw & 31)) - 1u) : 0xffffffffu;   // bits past H*W in the last word do not count
    const int i0 = ti * VT, j0 = tj * VT;
    const int nd = r.D - i0 < VT ? (int)(r.D - i0) : VT, ng = r.G - j0 < VT ? (int)(r.G - j0) : VT;
    const uint32_t *pa = bits + r.p_word + (long)i0 * tw, *pb = bits + r.q_word + (long)j0 * tw;
    const uint8_t *pr = present + r.pres0 + (long)i0 * r.T;

    const int lane = threadIdx.x & 63, lp = lane >> 3, lq = lane & 7;
    PopcTile<VT> tile;
    tile.zero();
    unsigned long long sum = 0ull;            // this wave's share of sum over the frame set of |p_t| + |q_t|, pair (lp, lq)
    for (long t = f0 / r.wpp; t * r.wpp < f1; ++t) {
        unsigned int here = 0u;               // bit p: frame t is in the frame set of P-side track i0 + p
#pragma unroll
        for (int p = 0; p < VT; ++p) here |= (p < nd && pr[(long)p * r.T + t] != 0) ? 1u << p : 0u;
        if (!here) continue;                                                      // the frame is in no pair's frame set
        const long base = t * r.wpp;
        const long w0 = f0 > base ? f0 - base : 0, w1 = f1 - base < r.wpp ? f1 - base : r.wpp;
        unsigned int fa[VT], fb[VT];                                              // this thread's share of the frame's plane areas
#pragma unroll
        for (int p = 0; p < VT; ++p) fa[p] = fb[p] = 0u;
        for (long w = w0 + threadIdx.x; w < w1; w += 256) {
            const uint32_t keep = w == r.wpp - 1 ? tail : 0xffffffffu;
            unsigned int va[VT], vb[VT];
#pragma unroll
            for (int p = 0; p < VT; ++p) {
                va[p] = (here >> p & 1u) ? pa[(long)p * tw + base + w] & keep : 0u;
                vb[p] = p < ng ? pb[(long)p * tw + base + w] & keep : 0u;
                fa[p] += __popc(va[p]);
                fb[p] += __popc(vb[p]);
            }
            tile.add(va, vb);
        }
        // once per frame: the wave's areas, then lane (lp, lq) takes |p_t| + |q_t| if its p is present (fa is 0 where it is not)
        unsigned int sa = 0u, sb = 0u;
#pragma unroll
        for (int p = 0; p < VT; ++p) {
            unsigned int a = fa[p], b = fb[p];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                a += __shfl_xor(a, o, 64);
                b += __shfl_xor(b, o, 64);
            }
            sa = lp == p ? a : sa;
            sb = lq == p ? b : sb;
        }
        sum += (here >> lp & 1u) ? sa + sb : 0u;
    }
    red_s[threadIdx.x >> 6][lane] = sum;      // read behind the barrier that ends reduce()
    const unsigned long long ni = tile.reduce(red_i);
    const unsigned long long ns = threadIdx.x < VT * VT ? red_s[0][lane] + red_s[1][lane] + red_s[2][lane] + red_s[3][lane] : 0ull;
    if (threadIdx.x < VT * VT) {
        const int p = threadIdx.x / VT, q = threadIdx.x % VT;
        if (p < nd && q < ng) {
            const long idx = r.pair0 + (long)(i0 + p) * r.G + (j0 + q);
            if (ni) atomicAdd(&inter[idx], ni);
            if (ns - ni) atomicAdd(&uni[idx], ns - ni);                           // |a| + |b| >= |a & b| word by word
        }
    }
}

__global__ __launch_bounds__(KEEP_T) void keep_tube_kernel(const unsigned long long *__restrict__ inter,
                                                           const unsigned long long *__restrict__ uni, long n_pairs,
                                                           const long *__restrict__ vid, int *__restrict__ keep, long n_keep)
{
    const long *r = vid + (long)VID_COLS * blockIdx.x;
    const long D = r[5], G = r[6], d0 = r[7], pair0 = r[9];
    const long lim = 1L << 31;
    if (D < 0 || D >= lim || G < 0 || G >= lim || d0 < 0 || D > n_keep - d0 || pair0 < 0 || D * G > n_pairs - pair0) return;
    for (long d = threadIdx.x; d < D; d += KEEP_T) {
        int k = 1;
        for (long g = 0; g < G; ++g) {
            const long long i = (long long)inter[pair0 + d * G + g], u = (long long)uni[pair0 + d * G + g];
            if (!(2 * i < u)) k = 0;                                              // tube IoU >= 0.5, or u == 0
        }
        keep[d0 + d] = k;
    }
}

}  // namespace

extern "C" {

int s2d_tube_counts_ragged(const uint32_t *bits, long total_words, const long *videos, int N, const uint8_t *present, long n_present,
                           const int *tiles, int n_tiles, long max_track_words, unsigned long long *inter, unsigned long long *uni,
                           long n_pairs, int accumulate, hipStream_t stream)
{
    if (N < 0 || n_tiles < 0 || total_words < 0 || n_present < 0 || n_pairs < 0 || max_track_words < 0) return S2D_ERR_ARG;
    if (N == 0 || n_pairs == 0) return S2D_OK;
    if (!bits || !videos || !present || !inter || !uni || (n_tiles && !tiles)) return S2D_ERR_ARG;
    if (max_track_words >= (1L << 40)) return S2D_ERR_ARG;
    const int splits_min = cdiv(max_track_words, SPLIT_WORDS_MAX);
    if (!accumulate) {
        if (s2d_zero_async(inter, sizeof(unsigned long long) * (size_t)n_pairs, stream) != S2D_OK) return S2D_ERR_LAUNCH;
        if (s2d_zero_async(uni, sizeof(unsigned long long) * (size_t)n_pairs, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    }
    if (n_tiles == 0 || max_track_words == 0) return S2D_OK;
    int splits = popc_chunks(max_track_words, n_tiles);
    if (splits < splits_min) splits = splits_min;
    hipLaunchKernelGGL(tube_counts_kernel, dim3(n_tiles, splits), dim3(256), 0, stream, bits, total_words, videos, N, present,
                       n_present, tiles, inter, uni, n_pairs);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_selftrain_keep_tube_ragged(const unsigned long long *inter, const unsigned long long *uni, long n_pairs, const long *videos, int N,
                                   int *keep, long n_keep, hipStream_t stream)
{
    if (N < 0 || n_pairs < 0 || n_keep < 0) return S2D_ERR_ARG;
    if (N == 0) return S2D_OK;
    if (!videos || (n_keep && !keep) || (n_pairs && (!inter || !uni))) return S2D_ERR_ARG;
    if (n_keep == 0) return S2D_OK;
    hipLaunchKernelGGL(keep_tube_kernel, dim3(N), dim3(KEEP_T), 0, stream, inter, uni, n_pairs, videos, keep, n_keep);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
