// Binary morphology of a CHUNK of bit planes of different sizes, every plane with a radius of its own (s2d_plane_morph_ragged):
// s2d_amd/plane_morph.py (the rule is stated there), DESIGN.md section 1.  The planes are the flat buffer and the plane table of
// rle_ragged.hip / plane_components.hip: plane int64 [P][4] = {word0, H, W, 0}, pixel i = y*W + x in word i / 32, bit i % 32
// (bitplane.h), so rows are not word-aligned.  The rule is this project's own: the reference cleans nothing.
//
// ONE device body.  dilate(X) has a zero border; erode(X), with everything outside the image counting as set, is ~dilate(~X) with
// both complements taken INSIDE the image.  So pm_dilate_kernel is the zero-border dilation of disk_dilate_kernel (davis_eval.hip:
// the distinct half-widths w_j of the structuring element with their heights h_j, V_h[y] = OR_{|dy| <= h} B[y + dy] growing by two
// rows per step, D[y] = OR_j hdil(V_{h_j}[y], w_j) by window192 / centre_word) with two flags: complement the staged input words,
// complement the accumulators.  The row mask (pixels at and beyond W) is applied AFTER either flag, rows outside the image and
// words outside the row are staged as 0 whatever the flag: padding bits, the flat neighbours of a row and everything outside the
// plane never reach a pixel.  The square is the single run {h = r, w = r}; the runs of a plane's disk are built by one thread of
// the workgroup into LDS (at most 2r steps).
//
// The grid is 1-D over a host-built table, tiles int32 [n_tiles][3] = {plane, tile row, tile column}, as in plane_components.hip; a
// workgroup reads its plane's geometry and radius from the tables.  A tile is at most PM_TW = 32 row-aligned words wide and at most
// pm_rows(r) rows high -- what the budget of PM_CAP LDS words (40 KiB: four workgroups per CU) holds at that width beside the 2r halo
// rows and the PM_RUNW words of the run table: src [th + 2r][tw + 4], V [th][tw + 4], acc [th][tw] --, and a plane's rows are cut
// evenly: nty = ceil(H / pm_rows(r)) tile rows of ceil(H / nty) rows.  LDS is dynamic and ONE figure per launch, lds_words: the
// largest need of any tile of the chunk, PM_RUNW + (th + 2r)(tw + 4) + th (tw + 4) + th tw, which the caller that built the tile
// table knows (plane_morph.py: morph_lds_words); a chunk of small masks at small radii reserves a few KiB per workgroup, not the
// budget.  A tile that needs more than the launch was given is skipped, so a wrong figure gives wrong bits, never a wild access.
//
//   pm_prep_kernel   a workgroup per plane: r = 0 copies the plane with its padding zeroed; otherwise the plane's words are zeroed
//                    when its rows are not word-aligned (store_row_word ORs into them).  Words between planes are never written.
//   pm_dilate_kernel the body above; r = 0 planes and planes that do not fit the buffer are skipped.
//   pm_count_kernel  a workgroup per plane: cleared[p] = popcount(in & ~out), set[p] = popcount(out & ~in) over the plane's pixels
//                    (also on its own, s2d_plane_diff_counts_ragged: the annotation cleanup counts decoded against smoothed planes).
// open = dilate(erode(.)) and close = erode(dilate(.)) are two passes through a chunk-sized workspace; a tile reads its neighbours'
// halos, so neither pass may write what it reads.  Plain vector stores and integer atomicOr only; every sum is an integer one.
#include "bitplane.h"

namespace {

constexpr int PM_T = 256;
constexpr int PM_RMAX = 64;           // two halo words hold 64 pixels either side of a word
constexpr int PM_CAP = 10240;         // LDS words per workgroup at most, run table included (40 KiB: four workgroups per CU)
constexpr int PM_RUNW = 36;           // of them the run table: h[65], w[65] as bytes and n (35 words, rounded to 16 bytes)
constexpr int PM_TW = 32;             // row-aligned words per tile row at most
constexpr int PM_HALO = 2;            // halo words either side
constexpr int PM_TWH = PM_TW + 2 * PM_HALO;

enum { PM_ERODE = 0, PM_DILATE = 1, PM_OPEN = 2, PM_CLOSE = 3 };
enum { PM_DISK = 0, PM_SQUARE = 1 };

// the tile rows the budget holds at full width beside the run table and the 2r halo rows: 98 at r = 0, 53 at r = 64
__host__ __device__ inline int pm_rows(int r) { return (PM_CAP - PM_RUNW - 2 * r * PM_TWH) / (2 * PM_TWH + PM_TW); }

__device__ __forceinline__ unsigned int pm_row_mask(int W, int k)
{
    const int n = W - 32 * k;
    return n >= 32 ? 0xffffffffu : (1u << n) - 1u;          // 1 <= n: the word starts inside the row
}

// pixels of the last flat word of a plane, 1 .. 32, as a mask
__device__ __forceinline__ unsigned int pm_last_mask(const PlaneRow &q)
{
    const int n = (int)((long)q.H * q.W - 32 * (q.wpp - 1));
    return n >= 32 ? 0xffffffffu : (1u << n) - 1u;
}

__device__ __forceinline__ bool pm_radius_ok(int r) { return r >= 0 && r <= PM_RMAX; }

__global__ __launch_bounds__(PM_T) void pm_prep_kernel(const uint32_t *__restrict__ src, const long *__restrict__ plane, long total_words,
                                                       const int *__restrict__ radius, uint32_t *__restrict__ dst)
{
    const PlaneRow q = plane_row(plane, blockIdx.x, total_words);
    if (!q.ok) return;
    const int r = radius[blockIdx.x];
    if (!pm_radius_ok(r)) return;
    if (r == 0) {
        const unsigned int last = pm_last_mask(q);
        for (long w = threadIdx.x; w < q.wpp; w += PM_T) dst[q.word0 + w] = src[q.word0 + w] & (w == q.wpp - 1 ? last : 0xffffffffu);
    } else if (q.W & 31) {
        for (long w = threadIdx.x; w < q.wpp; w += PM_T) dst[q.word0 + w] = 0u;
    }
}

__global__ __launch_bounds__(PM_T) void pm_dilate_kernel(const uint32_t *__restrict__ src, const long *__restrict__ plane, int P,
                                                         long total_words, const int *__restrict__ radius, const int *__restrict__ tiles,
                                                         int square, int comp_in, int comp_out, int lds_words,
                                                         uint32_t *__restrict__ dst)
{
    extern __shared__ unsigned int pm_lds[];                // [lds_words]: the run table, then src, V, acc
    int &run_n = *reinterpret_cast<int *>(pm_lds);
    unsigned char *run_h = reinterpret_cast<unsigned char *>(pm_lds + 1), *run_w = run_h + PM_RMAX + 1;
    unsigned int *lds = pm_lds + PM_RUNW;

    // the workgroup's row of the tile table; a row that names no tile of a plane the buffer holds is skipped (uniform)
    const int *t = tiles + 3L * blockIdx.x;
    const int f = t[0], ty = t[1], tx = t[2];
    if (f < 0 || f >= P || ty < 0 || tx < 0) return;
    const PlaneRow q = plane_row(plane, f, total_words);
    if (!q.ok) return;
    const int R = radius[f];
    if (R < 1 || R > PM_RMAX) return;
    const int H = q.H, W = q.W, S = (int)(((long)W + 31) / 32);
    const int rows = pm_rows(R);
    const int nty = (int)(((long)H + rows - 1) / rows), TR = (int)(((long)H + nty - 1) / nty);
    const long y0l = (long)ty * TR, k0l = (long)tx * PM_TW;
    if (y0l >= H || k0l >= S) return;
    const int y0 = (int)y0l, k0 = (int)k0l;
    const int th = min(TR, H - y0), tw = min(PM_TW, S - k0);
    const int twh = tw + 2 * PM_HALO, LR = th + 2 * R;
    const int NS = LR * twh, NV = th * twh, NA = th * tw;   // PM_RUNW + NS + NV + NA <= PM_CAP: th <= pm_rows(R), tw <= PM_TW
    if (PM_RUNW + NS + NV + NA > lds_words) return;         // the launch was given less than this tile needs (uniform)
    unsigned int *sb = lds, *vb = lds + NS, *ab = vb + NV;
    const uint32_t *pl = src + q.word0;

    if (threadIdx.x == 0) {
        int n = 0;
        if (square) {
            run_h[0] = run_w[0] = (unsigned char)R;
            n = 1;
        } else {                                            // disk_runs of davis_eval.hip: w(dy) = floor(sqrt(R^2 - dy^2)) only falls
            int prev = -1, w = R;
            for (int dy = 0; dy <= R; ++dy) {
                while (w * w + dy * dy > R * R) --w;
                if (w != prev) {
                    run_w[n] = (unsigned char)w;
                    run_h[n] = (unsigned char)dy;
                    ++n;
                    prev = w;
                } else {
                    run_h[n - 1] = (unsigned char)dy;
                }
            }
        }
        run_n = n;
    }
    for (int i = threadIdx.x; i < NS; i += PM_T) {
        const int ry = i / twh, k = k0 - PM_HALO + (i - ry * twh);
        const long y = (long)y0 - R + ry;
        unsigned int v = 0u;
        if (y >= 0 && y < H && k >= 0 && k < S) {
            v = row_word(pl, q.wpp, (int)y, W, k);
            if (comp_in) v = ~v & pm_row_mask(W, k);
        }
        sb[i] = v;
    }
    for (int i = threadIdx.x; i < NV; i += PM_T) vb[i] = 0u;
    for (int i = threadIdx.x; i < NA; i += PM_T) ab[i] = 0u;
    __syncthreads();

    const int nruns = run_n;
    int h_done = -1;                                        // V holds the rows |dy| <= h_done
    for (int j = 0; j < nruns; ++j) {
        const int hj = run_h[j], wj = run_w[j];
        for (int i = threadIdx.x; i < NV; i += PM_T) {
            const int c = R * twh + i;                      // the word's own row in src: tile row ry is src row ry + R
            unsigned int v = vb[i];
            for (int dy = h_done + 1; dy <= hj; ++dy) v |= sb[c - dy * twh] | sb[c + dy * twh];   // 0 <= ry + R -+ dy < LR
            vb[i] = v;
        }
        h_done = hj;
        __syncthreads();
        for (int i = threadIdx.x; i < NA; i += PM_T) {
            const int ry = i / tw, kk = i - ry * tw;
            const unsigned int *vr = vb + ry * twh + kk;    // words k-2 .. k+2 of the row: window bit 64 + q is pixel 32k + q
            u192 A;
            A.a = ((unsigned long long)vr[1] << 32) | vr[0];
            A.b = ((unsigned long long)vr[3] << 32) | vr[2];
            A.c = vr[4];
            ab[i] |= wj == 0 ? (unsigned int)A.b : centre_word(window192<BitOr>(A, 2 * wj + 1), wj);
        }
        __syncthreads();
    }

    uint32_t *op = dst + q.word0;
    const int aligned = (W & 31) == 0;
    for (int i = threadIdx.x; i < NA; i += PM_T) {
        const int ry = i / tw, k = k0 + (i - ry * tw), y = y0 + ry;      // y < H, k < S: th and tw are cut to the plane
        unsigned int v = ab[i];
        if (comp_out) v = ~v;
        store_row_word(op, y, W, k, v & pm_row_mask(W, k), aligned);
    }
}

__global__ __launch_bounds__(PM_T) void pm_count_kernel(const uint32_t *__restrict__ in, const uint32_t *__restrict__ out,
                                                        const long *__restrict__ plane, long total_words, const int *__restrict__ radius,
                                                        int *__restrict__ cleared, int *__restrict__ set)
{
    __shared__ unsigned int red[2][4];
    const PlaneRow q = plane_row(plane, blockIdx.x, total_words);
    const bool ok = q.ok && (!radius || pm_radius_ok(radius[blockIdx.x]));
    unsigned int c = 0u, s = 0u;
    if (ok) {
        const unsigned int last = pm_last_mask(q);
        for (long w = threadIdx.x; w < q.wpp; w += PM_T) {
            const unsigned int m = w == q.wpp - 1 ? last : 0xffffffffu;
            const unsigned int a = in[q.word0 + w] & m, b = out[q.word0 + w] & m;
            c += __popc(a & ~b);
            s += __popc(b & ~a);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_xor(c, o, 64);
        s += __shfl_xor(s, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = c;
        red[1][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        cleared[blockIdx.x] = (int)(red[0][0] + red[0][1] + red[0][2] + red[0][3]);
        set[blockIdx.x] = (int)(red[1][0] + red[1][1] + red[1][2] + red[1][3]);
    }
}

bool pm_sizes_ok(long total_words, int P) { return total_words >= 0 && P >= 0 && total_words < (1L << 50); }
template <typename T>
bool pm_aligned(const T *p) { return reinterpret_cast<uintptr_t>(p) % sizeof(T) == 0; }
uint8_t *pm_align16(void *p) { return reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(p) + 15) / 16 * 16); }
bool pm_overlap(const void *a, long na, const void *b, long nb)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

// one pass: dst = dilate(src) (erode = 0) or erode(src) (erode = 1), plane by plane at its own radius
void pm_pass(const uint32_t *src, const long *plane, int P, long total_words, const int *radius, const int *tiles, int n_tiles, int square,
             int erode, int lds_words, uint32_t *dst, hipStream_t stream)
{
    hipLaunchKernelGGL(pm_prep_kernel, dim3((unsigned)P), dim3(PM_T), 0, stream, src, plane, total_words, radius, dst);
    if (n_tiles)
        hipLaunchKernelGGL(pm_dilate_kernel, dim3((unsigned)n_tiles), dim3(PM_T), sizeof(unsigned int) * (size_t)lds_words, stream, src, plane,
                           P, total_words, radius, tiles, square, erode, erode, lds_words, dst);
}

}  // namespace

extern "C" {

int s2d_plane_morph_tile(int r, int *rows, int *words)
{
    if (!rows || !words || r < 0 || r > PM_RMAX) return S2D_ERR_ARG;
    *rows = pm_rows(r);
    *words = PM_TW;
    return S2D_OK;
}

long s2d_plane_morph_lds_words(int r, int H, int W)
{
    if (r < 0 || r > PM_RMAX || H < 1 || W < 1) return S2D_ERR_ARG;
    if (r == 0) return 0;                                   // copied by pm_prep_kernel: no tile
    const int rows = pm_rows(r), nty = cdiv(H, rows), th = cdiv(H, nty), S = cdiv(W, 32), tw = S < PM_TW ? S : PM_TW;
    return PM_RUNW + (long)(th + 2 * r) * (tw + 2 * PM_HALO) + (long)th * (tw + 2 * PM_HALO) + (long)th * tw;
}

long s2d_plane_morph_workspace_bytes(long total_words, int P)
{
    if (!pm_sizes_ok(total_words, P)) return S2D_ERR_ARG;
    return 16 + (total_words * 4 + 15) / 16 * 16;           // 16: the workspace may start at any address
}

int s2d_plane_morph_ragged(const uint32_t *bits, const long *plane, int P, long total_words, int op, int shape, const int *radius,
                           const int *tiles, int n_tiles, int lds_words, uint32_t *out, int *cleared, int *set, void *workspace,
                           hipStream_t stream)
{
    if (lds_words < 0 || lds_words > PM_CAP || (n_tiles > 0 && lds_words <= PM_RUNW)) return S2D_ERR_ARG;
    if (!pm_sizes_ok(total_words, P) || n_tiles < 0 || op < PM_ERODE || op > PM_CLOSE || (shape != PM_DISK && shape != PM_SQUARE))
        return S2D_ERR_ARG;
    if (!bits || !plane || !radius || !out || !cleared || !set || !workspace || (n_tiles && !tiles)) return S2D_ERR_ARG;
    if (!pm_aligned(bits) || !pm_aligned(plane) || !pm_aligned(radius) || !pm_aligned(tiles) || !pm_aligned(out) || !pm_aligned(cleared) ||
        !pm_aligned(set))
        return S2D_ERR_ARG;
    // a tile reads its neighbours' halos: out may be neither the input nor the workspace
    const long bytes = total_words * 4;
    if (out == bits || pm_overlap(out, bytes, bits, bytes) || pm_overlap(out, bytes, workspace, s2d_plane_morph_workspace_bytes(total_words, P)) ||
        pm_overlap(bits, bytes, workspace, s2d_plane_morph_workspace_bytes(total_words, P)))
        return S2D_ERR_ARG;
    if (P == 0) return S2D_OK;
    const int square = shape == PM_SQUARE;
    uint32_t *tmp = reinterpret_cast<uint32_t *>(pm_align16(workspace));
    if (total_words) {
        if (op == PM_ERODE || op == PM_DILATE) {
            pm_pass(bits, plane, P, total_words, radius, tiles, n_tiles, square, op == PM_ERODE, lds_words, out, stream);
        } else {
            pm_pass(bits, plane, P, total_words, radius, tiles, n_tiles, square, op == PM_OPEN, lds_words, tmp, stream);
            pm_pass(tmp, plane, P, total_words, radius, tiles, n_tiles, square, op == PM_CLOSE, lds_words, out, stream);
        }
    }
    hipLaunchKernelGGL(pm_count_kernel, dim3((unsigned)P), dim3(PM_T), 0, stream, bits, out, plane, total_words, radius, cleared, set);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_plane_diff_counts_ragged(const uint32_t *a, const uint32_t *b, const long *plane, int P, long total_words, int *cleared, int *set,
                                 hipStream_t stream)
{
    if (!pm_sizes_ok(total_words, P) || !a || !b || !plane || !cleared || !set) return S2D_ERR_ARG;
    if (!pm_aligned(a) || !pm_aligned(b) || !pm_aligned(plane) || !pm_aligned(cleared) || !pm_aligned(set)) return S2D_ERR_ARG;
    if (P == 0) return S2D_OK;
    hipLaunchKernelGGL(pm_count_kernel, dim3((unsigned)P), dim3(PM_T), 0, stream, a, b, plane, total_words, (const int *)nullptr, cleared, set);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
